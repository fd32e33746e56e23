"""The packed-row step of the encode chain (htscodecs_amd/csrc/r4x16_enc_chain.h: chain_encode_o1_lds with packed rows,
EncOutT::emit16q, the index words of pairw(), the neutral symbols of lanes without a trip) against the CPU oracle, byte
for byte: rans4x16_hip_compress_dev with order 1 and the short-step routes off, so that the packed-row pipeline runs.

What picks a path in that loop is the stream's length (q = n >> 2 bytes per chain, npair = (q - 1) >> 3 double trips of
the pipelined loop, which is unrolled four double trips; the rest goes to the single steps behind it, the tail n & 3 in
front of it), the lengths of the other streams of its wave (lanes past their end, lanes without a stream), the
alphabet (packed rows: 20..64 symbols with byte 0, which every order-1 alphabet lists; below byte 128 the short index
and the frequency table, else the full index) and how often a step emits.  Every case asserts the route it took: a
block takes packed rows exactly if its table has 10 bits and 20..64 symbols, by the oracle's own compute_shift."""
import ctypes as C
import functools

import numpy as np
import pytest

LENGTHS = sorted(set([0, 1, 3, 4, 5, 7, 31, 32, 33, 35, 36, 37] + list(range(63, 70)) + list(range(127, 134)) +
                     [4 * (8 * p + 1) + t for p in (1, 2, 3, 4, 5, 8, 9) for t in range(4)] + [4096, 65536 + 3]))
# the same lengths behind 8,192 bytes (a whole number of unrolled passes: the same stage, tail and residue): a block of
# a few hundred uniform bytes over 46 symbols is stored raw in the end, whatever the chain made of it - these are not
LONG = [8192 + n for n in LENGTHS]
NS = (20, 21, 45, 46, 47, 64)           # ENC_PK_MIN_NS .. ENC_PK_MAX_NS: alphabet sizes, byte 0 included


def alphabet(ns, high):
    """ns - 1 byte values (byte 0 is in every order-1 alphabet without occurring); high: some at or above 128."""
    return np.arange(33, 33 + ns - 1, dtype=np.uint8) + (100 if high else 0)


def block(n, ns, high=False, seed=0):
    """n bytes over the alphabet: every symbol once, as far as n allows, then uniform draws."""
    a = alphabet(ns, high)
    rng = np.random.default_rng(1000 * ns + 7 * n + seed)
    out = a[rng.integers(0, len(a), size=n)]
    m = min(n, len(a))
    out[:m] = rng.permutation(a)[:m]
    return out.tobytes()


def skewed(n, ns, seed):
    """Text-like: long runs of one symbol with rare others (steps that emit nothing for a long while), and contexts
    whose rare symbols end up with frequency 1, 2 and 3 beside one dominant symbol."""
    a = alphabet(ns, False)
    rng = np.random.default_rng(seed)
    p = np.full(len(a), 0.05 / (len(a) - 1))          # (more skew and compute_shift moves to 12-bit tables)
    p[0] = 0.95
    out = a[rng.choice(len(a), size=n, p=p)]
    out[:len(a)] = a
    return out.tobytes()


def one_context(n, ns):
    """Every symbol of the alphabet is followed by the same byte: contexts with a single symbol (frequency 1,024)."""
    a = alphabet(ns, False)
    out = np.empty(n, dtype=np.uint8)
    out[0::2] = np.resize(a[1:], len(out[0::2]))
    out[1::2] = a[0]
    return out.tobytes()


@functools.lru_cache(maxsize=None)
def table_bits(raw):
    """The table precision the reference's compute_shift picks for `raw` (the oracle's own function, over the order-1
    histogram as orc_o1_encode builds it): a short random block is stored raw in the end, so its stream does not say."""
    import cpu_libs
    lib = cpu_libs.oracle().lib
    a = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    F = np.zeros((256, 256), dtype=np.uint32)
    np.add.at(F, (np.concatenate([[0], a[:-1]]), a), 1)
    for k in (1, 2, 3):
        F[0, a[k * (len(a) >> 2)]] += 1
    T = np.ascontiguousarray(F.sum(axis=1, dtype=np.uint32))
    F0 = np.zeros(256, dtype=np.uint32)
    F0[a] = 1
    F0[0] = 1
    S = (C.c_int * 256)()
    lib.orc_compute_shift.restype = C.c_int
    lib.orc_compute_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib.orc_compute_shift(F0.ctypes.data, F.ctypes.data, T.ctypes.data, C.addressof(S))


def takes_packed(raw):
    """Order 1 is coded as order 1 from eight bytes on; packed rows: 10-bit tables of 20..64 symbols, byte 0 included."""
    return len(raw) >= 8 and 20 <= len(set(raw) | {0}) <= 64 and table_bits(raw) == 10


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


@functools.lru_cache(maxsize=None)
def _want(raw):
    import cpu_libs
    return cpu_libs.oracle().compress(raw, 1)


def encode(H, opts, raws):
    """One rans4x16_hip_compress_dev call over `raws` with order 1: (streams, route read-out of the encode chain)."""
    import torch
    opts.set("enc_direct", 0)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    sizes = [len(r) for r in raws]
    caps = [H.rans_compress_bound_4x16(s, 1) for s in sizes]
    in_off = np.concatenate([[0], np.cumsum([(s + 63) // 64 * 64 + 64 for s in sizes])]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([(c + 255) // 256 * 256 for c in caps])]).astype(np.int64)
    arena = np.zeros(int(in_off[-1]) + 64, dtype=np.uint8)
    for r, off in zip(raws, in_off):
        arena[off:off + len(r)] = np.frombuffer(r, dtype=np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dc.dev)
    d_in, d_in_off, d_size = t(arena), t(in_off[:-1]), t(np.array(sizes, dtype=np.int32))
    d_out = torch.zeros(int(out_off[-1]) + 256, dtype=torch.uint8, device=dc.dev)
    d_out_off, d_cap = t(out_off[:-1]), t(np.array(caps, dtype=np.int32))
    d_osz, d_st = (torch.full((len(raws),), -3, dtype=torch.int32, device=dc.dev) for _ in range(2))
    dc.route_read("encode")
    rc = dc.L.rans4x16_hip_compress_dev(dc.ctx.h, len(raws), d_in.data_ptr(), d_in_off.data_ptr(), d_size.data_ptr(),
                                        d_out.data_ptr(), d_out_off.data_ptr(), d_cap.data_ptr(), d_osz.data_ptr(),
                                        d_st.data_ptr(), 1, None, max(sizes), dc._stream())
    assert rc == 0, dc.ctx.error()
    torch.cuda.synchronize()
    route = dc.route_read("encode")
    assert d_st.tolist() == [0] * len(raws), d_st.tolist()
    out, osz = d_out.cpu().numpy(), d_osz.tolist()
    return [out[o:o + z].tobytes() for o, z in zip(out_off, osz)], route


def check(H, opts, raws, high=False, all_packed=False):
    """The oracle's bytes for every block, and the route: packed rows for exactly the blocks that can take them, of the
    kind the alphabet asks for; all_packed: the case is built so that every block does."""
    want = [_want(r) for r in raws]
    got, route = encode(H, opts, raws)
    bad = [(i, len(r)) for i, (r, g, w) in enumerate(zip(raws, got, want)) if g != w]
    assert not bad, bad[:10]
    npk = sum(1 for r in raws if takes_packed(r))
    assert not all_packed or npk == len(raws), (npk, len(raws))
    assert route["records"] == 0 and route["packed"] == npk, (route, npk)
    assert route["packed_freq"] == (0 if high else npk), (route, npk)
    return npk


@pytest.mark.gpu
@pytest.mark.parametrize("high", [False, True], ids=["short-index", "full-index"])
def test_every_length_alone(H, opts, high):
    """One block per call: one quad of one wave works, every other lane has no stream.  Lengths of 31 and more hold 20
    or more distinct symbols and must take packed rows; the shorter ones cannot (too few symbols) and say so."""
    for n in LENGTHS + LONG:
        npk = check(H, opts, [block(n, 46, high)], high)
        assert npk == (1 if n >= 31 else 0), (n, npk)


@pytest.mark.gpu
@pytest.mark.parametrize("high", [False, True], ids=["short-index", "full-index"])
def test_every_length_in_one_batch(H, opts, high):
    """All the lengths side by side, shortest first: waves whose lanes drop out of the loop at different trips."""
    raws = [block(n, 46, high, seed=1) for n in LENGTHS + LONG]
    assert check(H, opts, raws, high) == sum(1 for n in LENGTHS + LONG if n >= 31)


@pytest.mark.gpu
@pytest.mark.parametrize("nblk", [16, 23, 48])
def test_wave_of_mixed_lengths(H, opts, nblk):
    """Lengths from the list and a few long ones in one batch, the shortest in the first slot: lanes past their end
    beside lanes in full swing, lanes without a stream (16 or 23 streams in a workgroup's 45 seats), several waves (48)."""
    rng = np.random.default_rng(nblk)
    pool = [n for n in LENGTHS + LONG if n >= 31]
    lens = [31] + [int(rng.choice(pool)) for _ in range(nblk - 5)] + [20000, 33333, 65539, 70000]
    raws = [block(n, 46, False, seed=2 + i) for i, n in enumerate(lens)]
    assert check(H, opts, raws, all_packed=True) == nblk


@pytest.mark.gpu
@pytest.mark.parametrize("high", [False, True], ids=["short-index", "full-index"])
@pytest.mark.parametrize("ns", NS)
def test_alphabet_sizes(H, opts, ns, high):
    """The smallest and the largest packed alphabets and the sizes around the headline's 46, each with a length of every
    residue class of the unrolled loop."""
    raws = [block(n, ns, high, seed=3) for n in (127, 260, 777, 4096, 12345)]
    check(H, opts, raws, high, all_packed=True)


@pytest.mark.gpu
def test_alphabets_outside_the_packed_rows_take_the_other_kernels(H, opts):
    """19 and 65 symbols: one off either end of the packed range, coded from u16 rows - and the route says so."""
    for ns in (19, 65):
        assert check(H, opts, [block(n, ns, False, seed=4) for n in (777, 4096)]) == 0


@pytest.mark.gpu
def test_single_symbol_contexts_rare_symbols_and_one_repeated_byte(H, opts):
    """Frequencies at the table's ends: contexts with a single symbol (1,024: no emission, nothing added), rare symbols
    beside a dominant one (frequencies 1, 2, 3: the reciprocal of a power of two and of none), one repeated byte (two
    symbols: not a packed alphabet, and the route says so)."""
    check(H, opts, [one_context(n, 46) for n in (133, 4096, 20001)], all_packed=True)
    check(H, opts, [skewed(n, 24, 5 + n) for n in (4096, 30000, 65539)], all_packed=True)
    assert check(H, opts, [b"\x41" * 4096, b"\x41" * 65539]) == 0


@pytest.mark.gpu
def test_emission_extremes(H, opts):
    """64 KiB of uniform bytes over 46 symbols (nearly every step emits: both ring halves, every flush) beside a skewed
    text of the same length (long runs that emit nothing: the dump slot)."""
    check(H, opts, [block(65536, 46, False, seed=6), skewed(65536, 46, 7)], all_packed=True)


def test_cases_are_what_they_claim():
    """No GPU: the generators' alphabets, and the lengths' coverage of the loop's stages."""
    for ns in NS:
        for high in (False, True):
            raw = block(4096, ns, high)
            assert len(set(raw) | {0}) == ns and (max(raw) >= 128) == high
    assert len(set(one_context(4096, 46)) | {0}) == 46 and len(set(skewed(4096, 24, 1)) | {0}) == 24
    npair = {((n >> 2) - 1) >> 3 for n in LENGTHS if n >= 8}
    assert {0, 1, 2, 3, 4, 5, 8, 9} <= npair                       # every double trip of an unrolled pass, and the next pass
    assert {n & 3 for n in LENGTHS} == {0, 1, 2, 3}
