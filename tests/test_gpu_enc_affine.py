"""The affine body of the encode chain's pipelined loop (htscodecs_amd/csrc/r4x16_enc_chain.h, chain_encode_o1_lds:
index words computed from the bytes) against the CPU oracle, byte for byte.

rans4x16_hip_compress_dev with order 1 and the symbol records off, as tests/test_gpu_enc_step.py calls it.  What picks a
path: the alphabet (a run of consecutive bytes below 128 is affine - k_enc_tables' rule, restated in
test_enc_affine_cpu.py - and a wave takes the body only if all its streams are), the stream's double trips
npair = ((n >> 2) - 1) >> 3 of the pipelined loop, which is unrolled four double trips (a lane computes words from its
own bytes only while it has double trips; without one its word is a constant), the other lanes of the wave (lanes without
a stream, streams that end at other trips) and option enc_affine.
Every case asserts the route: packed rows of the short-index kind ("packed_freq") and, under "encode_body", the streams
of waves that took the affine body ("packed_affine")."""
import numpy as np
import pytest

from test_enc_affine_cpu import affine_of, alpha_of
from test_gpu_enc_step import _want, takes_packed

# 0, 1, 2, 3, 4, 5 and 9 double trips, every residue of the tail; 32..35: the shortest blocks that hold twenty symbols
# (no double trip); then the same behind 8,192 bytes (256 double trips: a whole number of unrolled passes)
SHORT = [32, 33, 34, 35] + [4 * (8 * p + 1) + t for p in (1, 2, 3, 4, 5, 9) for t in range(4)]
LENGTHS = SHORT + [8192 + n for n in [4, 5, 6, 7] + SHORT]


def run_of(ns, first):
    """ns - 1 consecutive byte values from `first` on (byte 0 is the alphabet's first symbol without occurring)"""
    return np.arange(first, first + ns - 1, dtype=np.uint8)


def block(n, a, seed=0):
    """n bytes over the byte values `a` (the first n of them, if it has more: a run stays a run): every one once, then
    uniform draws"""
    a = a[:n]
    rng = np.random.default_rng(7919 * len(a) + 31 * n + seed)
    out = a[rng.integers(0, len(a), size=n)]
    m = min(n, len(a))
    out[:m] = rng.permutation(a)[:m]
    return out.tobytes()


def is_affine(raw):
    return affine_of(alpha_of(raw), 0 in raw) != 0


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def encode(H, opts, raws, enc_affine=1):
    """One rans4x16_hip_compress_dev call over `raws` with order 1: (streams, encode read-out, packed_affine)."""
    import torch
    opts.set("enc_direct", 0)
    opts.set("enc_affine", enc_affine)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    assert dc.get_option("enc_affine") == enc_affine
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
    dc.route_read("encode"), dc.route_read("encode_body")
    rc = dc.L.rans4x16_hip_compress_dev(dc.ctx.h, len(raws), d_in.data_ptr(), d_in_off.data_ptr(), d_size.data_ptr(),
                                        d_out.data_ptr(), d_out_off.data_ptr(), d_cap.data_ptr(), d_osz.data_ptr(),
                                        d_st.data_ptr(), 1, None, max(sizes), dc._stream())
    assert rc == 0, dc.ctx.error()
    torch.cuda.synchronize()
    route, body = dc.route_read("encode"), dc.route_read("encode_body")
    assert d_st.tolist() == [0] * len(raws), d_st.tolist()
    out, osz = d_out.cpu().numpy(), d_osz.tolist()
    return [out[o:o + z].tobytes() for o, z in zip(out_off, osz)], route, body["packed_affine"]


def check(H, opts, raws, affine, enc_affine=1, short=None):
    """The oracle's bytes for every block; packed rows for the blocks that can take them, the short index for those of
    them below byte 128 (`short`: how many, default all); `affine`: the streams counted by waves of the affine body."""
    want = [_want(r) for r in raws]
    got, route, naff = encode(H, opts, raws, enc_affine)
    bad = [(i, len(r)) for i, (r, g, w) in enumerate(zip(raws, got, want)) if g != w]
    assert not bad, bad[:10]
    npk = sum(1 for r in raws if takes_packed(r))
    assert route["records"] == 0 and route["packed"] == npk, (route, npk)
    assert route["packed_freq"] == (npk if short is None else short), (route, npk, short)
    assert naff == affine, (naff, affine, route)
    return npk


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
def test_every_length_alone(H, opts, enc_affine):
    """One block per call: one quad is live, every other lane of the wave has no stream.  With the option off the same
    calls give the same bytes and count nothing."""
    a = run_of(46, 33)
    for n in LENGTHS:
        raw = block(n, a)
        assert takes_packed(raw) and is_affine(raw), n
        check(H, opts, [raw], enc_affine, enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
@pytest.mark.parametrize("nblk", [13, 9])
def test_full_wave_beside_a_partly_filled_wave(H, opts, nblk, enc_affine):
    """A small batch's workgroups are one wave of eight streams: 13 blocks are a full wave beside a wave of five, 9 blocks
    a full wave beside a wave with one stream.  Equal lengths, so all streams end at the same trip; then a long block
    beside short ones."""
    a = run_of(46, 33)
    for n in (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3):
        raws = [block(n, a, seed=i) for i in range(nblk)]
        check(H, opts, raws, nblk * enc_affine, enc_affine)
    raws = [block(8192 + 4 * (8 * 3 + 1), a, seed=i) for i in range(nblk - 1)] + [block(40000, a, seed=99)]
    check(H, opts, raws, nblk * enc_affine, enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
def test_mixed_lengths_in_one_wave(H, opts, enc_affine):
    """1, 3 and 9 double trips - and the same behind 8,192 bytes - in one wave: the loop ends at different trips per
    stream, and lanes past their end compute words from their quarter's first bytes."""
    a = run_of(46, 33)
    for far in (0, 8192):
        lens = [far + 4 * (8 * p + 1) + t for p, t in ((1, 0), (3, 1), (9, 2), (9, 3), (3, 3), (1, 2), (9, 0))]
        raws = [block(n, a, seed=5 + i) for i, n in enumerate(lens)]
        check(H, opts, raws, len(raws) * enc_affine, enc_affine)
    lens = [8192 + 4 * (8 * p + 1) + t for p, t in ((5, 0), (9, 1), (13, 2), (17, 3), (40, 0))] + [65536 + 3]
    check(H, opts, [block(n, a, seed=6 + i) for i, n in enumerate(lens)], len(lens) * enc_affine, enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [33, 1, 40], ids=["c32", "c0", "c39"])
@pytest.mark.parametrize("ns", [20, 46, 64])
def test_alphabets(H, opts, ns, first):
    """Alphabets of 20, 46 and 64 symbols starting at byte 33, 1 and 40, each with lengths of every stage; c = 0 with and
    without byte 0 in the data (index = byte either way)."""
    a = run_of(ns, first)
    lens = (4 * (8 * 3 + 1) + 1, 4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3, 12345)
    raws = [block(n, a, seed=7) for n in lens]
    assert all(takes_packed(r) and is_affine(r) for r in raws)
    check(H, opts, raws, len(raws))
    check(H, opts, raws, 0, enc_affine=0)
    if first == 1:
        a0 = np.concatenate([[0], a]).astype(np.uint8)
        raws = [block(n, a0, seed=8) for n in lens]
        assert all(takes_packed(r) and is_affine(r) and 0 in r for r in raws)
        check(H, opts, raws, len(raws))


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [20, 46, 64])
def test_alphabets_that_are_not_affine_take_the_look_up(H, opts, ns):
    """A byte removed from the middle of the run, byte 0 occurring in the data, and a run that reaches byte 128 (the
    full-index kind): all coded by the look-up body, and the read-out says so."""
    lens = (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3, 12345)
    for first in (33, 1, 40):
        a = run_of(ns + 1, first)
        gap = np.delete(a, len(a) // 2)
        raws = [block(n, gap, seed=9) for n in lens]
        assert all(takes_packed(r) and not is_affine(r) for r in raws)
        check(H, opts, raws, 0)
    a = run_of(ns, 33)
    raws = [block(n, np.concatenate([[0], a]).astype(np.uint8), seed=10) for n in lens]
    assert all(takes_packed(r) and not is_affine(r) for r in raws)
    check(H, opts, raws, 0)
    high = run_of(ns, 129 - ns // 2)                                        # a run across byte 128
    raws = [block(n, high, seed=11) for n in lens]
    assert all(takes_packed(r) and max(r) >= 128 for r in raws)
    check(H, opts, raws, 0, short=0)


@pytest.mark.gpu
def test_an_affine_and_a_non_affine_block_in_one_wave(H, opts):
    """Both in the same class, so in the same wave: it takes the look-up body and counts nothing.  Alone, the affine
    block counts."""
    a = run_of(46, 33)
    gap = np.delete(run_of(47, 33), 20)
    for n in (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3):
        raws = [block(n, a, seed=12), block(n, gap, seed=13)]
        assert is_affine(raws[0]) and not is_affine(raws[1])
        check(H, opts, raws, 0)
        check(H, opts, raws[:1], 1)


@pytest.mark.gpu
def test_sampled_alphabets(H, opts):
    """256 KiB blocks, whose alphabet the front end samples from the first 64 KiB: one that stays a run, and one whose
    last quarter holds a byte beyond the run (two beyond its end: the full alphabet has a gap)."""
    a = run_of(46, 33)
    stays = block(262144, a, seed=14)
    check(H, opts, [stays], 1)
    late = bytearray(block(262144, a, seed=15))
    late[250000] = int(a[-1]) + 2
    late = bytes(late)
    assert takes_packed(late) and not is_affine(late)
    check(H, opts, [late], 0)
    # ... and one beyond its end by one: the run grows by a byte that the sample did not see, and stays affine
    grown = bytearray(block(262144, a, seed=16))
    grown[250000] = int(a[-1]) + 1
    grown = bytes(grown)
    assert takes_packed(grown) and is_affine(grown)
    check(H, opts, [grown], 1)


def test_cases_are_what_they_claim():
    """No GPU: the lengths' coverage of the loop's stages, and the generators' alphabets."""
    npair = {((n >> 2) - 1) >> 3 for n in SHORT}
    assert npair == {0, 1, 2, 3, 4, 5, 9}
    assert {n & 3 for n in SHORT} == {0, 1, 2, 3}
    assert {(((n >> 2) - 1) >> 3) - 256 for n in LENGTHS if n >= 8192} == {0, 1, 2, 3, 4, 5, 9}
    for ns in (20, 46, 64):
        for first in (33, 1, 40):
            raw = block(4096, run_of(ns, first))
            assert len(alpha_of(raw)) == ns and max(raw) < 128 and is_affine(raw)
        assert max(block(4096, run_of(ns, 129 - ns // 2))) >= 128
    assert all(len(alpha_of(block(n, run_of(46, 33)))) >= 20 for n in LENGTHS)
