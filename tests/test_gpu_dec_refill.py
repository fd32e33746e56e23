"""The decode chain on packed rows of layout 2 (htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2) where the lean ring
refill of its 16-step trips can go wrong:

  * alphabet and length: order 1 with 46 and 48 symbols (rows of 64 and 80 bytes, group 3 reached, for 48 the symbol that
    ends in the dword behind group 3), 36 and 13 (rows of 64 and 32 bytes; 13: a last group of one symbol), 37 (the first
    size with four groups); 4,096, 4,099, 16,384 and 65,537 bytes, 256 zero bytes behind every stream as
    test_gpu_dec_trip16.py pads, so that the 16-step trips and their refill run up to the last steps; 1, 7 and 15 streams
    in a call (idle lanes run the trips on garbage and must neither write the ring nor ask for a chunk);
  * alignment and crossings: `words` at each of the 16 byte alignments with the stream of test_gpu_dec_trip16.py that
    crosses two quarters in one trip (both rounds of the refill, the second behind its own test) beside 14 slower ones
    (one round, or none); the quarter stream that makes its wave leave the 16-step trips early;
  * a stream WITHOUT words: a cycle of the 45 byte values, a multiple of 180 bytes long, so that every context has one
    successor and all four chains start alike - its payload ends with the four states (avail == 0 where `words` is
    16-byte aligned), and the refill's unconditional request must read the states in front of `words`, never behind
    them.  Among 14 ordinary streams; with `words` aligned and not; as the first and as the last bytes of the device
    allocation, the input tensor sized to end exactly with it.  (A block of ONE repeated byte is decoded beside them and
    must come out as before, but with an alphabet of two symbols it never reaches packed rows: it is counted on another route.)
  * a hostile stream on this route: a stream whose last byte is a symbol seen nowhere else, so that its context has no
    table (ROW_EMPTY), with its size field raised by four - every chain runs one step more, the fourth in the context
    without a table, behind trips of sixteen with their refills.  Status ST_CONTEXT, the 14 streams beside it untouched;
  * damaged tables: tests/golden/rans/edge.bin holds no damaged stream that reaches packed rows - its order-1 streams that
    still parse have 2 to 4 symbols, packed rows start at 13 (test_cases_are_what_they_claim counts them) - so there is
    no vector to take from it; tests/test_gpu_rans_edge.py decodes every one of them on the routes they do reach.

Streams are made by the CPU oracle and decoded by rans4x16_hip_uncompress_dev_sized; the decoded bytes are compared with
the RAW INPUT, never with output of the code under test, between guard bytes, and every case asserts its route as l1."""
import functools

import numpy as np
import pytest

import rans_edge_cases as X
import test_gpu_dec_shadow as S
import test_gpu_dec_trip16 as T16
from test_gpu_confinement import pattern
from test_gpu_confinement import _varint
from test_gpu_dec_step import H, ROUTES, ST_CONTEXT, Slots, alphabet, check_route, cyclic, decode, device, mismatches, stream_info, uniform  # noqa: F401
from test_gpu_dec_trip16 import ENTRY_WORDS, PAD, _varint_put

ALPHABETS = (46, 48, 36, 13, 37)
LONG = (4096, 4099, 16384, 65537)
WAVE = 15
OPTS = S.OPTS
NOWORDS_N = 180 * 23                # 4,140 bytes: 23 cycles of 45 byte values per chain


# ---- generators ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_stream(n, i, length):
    """(name, raw, stream + PAD zero bytes): uniform successors over an alphabet the decoder counts as n symbols."""
    import cpu_libs
    raw = uniform(length, alphabet(n, 1), 31000 * n + 16 * length + i)
    return ("n%d/%d/%d" % (n, length, i), raw, cpu_libs.oracle().compress(raw, 1) + bytes(PAD))


@functools.lru_cache(maxsize=None)
def no_words():
    """(name, raw, stream): the cycle; its payload holds the table and the four states and nothing behind them."""
    import cpu_libs
    raw = cyclic(NOWORDS_N, alphabet(46, 1))
    return ("nowords", raw, cpu_libs.oracle().compress(raw, 1))


@functools.lru_cache(maxsize=None)
def one_byte():
    import cpu_libs
    raw = bytes([77]) * 4096
    return ("onebyte", raw, cpu_libs.oracle().compress(raw, 1))


@functools.lru_cache(maxsize=None)
def ordinary():
    return [long_stream(46, i, LONG[0]) for i in range(14)]


@functools.lru_cache(maxsize=None)
def hostile():
    """(name, raw, stream): 4,096 bytes, the last one a byte value seen nowhere else; the stream says 4,100."""
    import cpu_libs
    a = alphabet(46, 1)
    raw = bytearray(uniform(LONG[0], a[:-1], 5150))
    raw[-1] = int(a[-1])
    s = cpu_libs.oracle().compress(bytes(raw), 1)
    assert s[0] == 1 and _varint(s, 1) == (LONG[0], 3) and len(_varint_put(LONG[0] + 4)) == 2
    return ("hostile", bytes(raw), s[:1] + _varint_put(LONG[0] + 4) + s[3:] + bytes(PAD))


def damaged_on_packed_rows():
    """The damaged 4x16 streams of tests/golden/rans/edge.bin that parse as order 1 with 13 .. 48 symbols."""
    out = []
    for d, s in X.damaged_streams(16):
        try:
            i = stream_info(s)
        except Exception:                                   # a table the test's own parser cannot follow
            continue
        if i.coded and i.order == 1 and 13 <= i.nsym <= 48:
            out.append((d, s))
    return out


# ---- GPU ----------------------------------------------------------------------------------------------------------
def run(dc, items, shifts=None):
    what = [name for name, _, _ in items]
    raws = [raw for _, raw, _ in items]
    st, osz, got, route, in_off = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    check_route(route, {"l1": len(items)})
    return in_off


def decode_at(dc, comps, sizes, what, in_off, total):
    """test_gpu_dec_step.py's decode() with the input arena laid out by the caller: `total` bytes, stream i at in_off[i]."""
    import torch
    arena = pattern(total)
    for c, off in zip(comps, in_off):
        arena[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    lay = Slots(sizes, what)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dc.dev)
    d_in, d_in_off, d_csz = t(arena), t(np.asarray(in_off, dtype=np.int64)), t(np.array([len(c) for c in comps], dtype=np.int32))
    d_out, d_out_off, d_cap = t(lay.pattern), t(lay.offs), t(lay.caps.astype(np.int32))
    d_osz, d_st = (torch.full((len(comps),), -3, dtype=torch.int32, device=dc.dev) for _ in range(2))
    assert d_in.data_ptr() % 16 == 0 and d_in.numel() == total
    dc.route_read("decode")
    dc.uncompress(d_in, d_in_off, d_csz, d_out, d_out_off, d_cap, d_osz, d_st, max(len(c) for c in comps), max(sizes),
                  total_out_cap=sum(sizes))
    torch.cuda.synchronize()
    route = dc.route_read("decode")
    out = d_out.cpu().numpy()
    stray = lay.stray_writes(out)
    assert stray is None, stray
    assert np.array_equal(d_in.cpu().numpy(), arena), "the input arena was written to"
    return d_st.tolist(), d_osz.tolist(), lay.take(out, lay.caps), route


@pytest.mark.gpu
@pytest.mark.parametrize("length", LONG)
@pytest.mark.parametrize("n", ALPHABETS)
def test_alphabets_and_lengths(H, opts, n, length):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    streams = WAVE if length <= 16384 else 3
    run(dc, [long_stream(n, i, length) for i in range(streams)], shifts=[(3 * i + n) % 16 for i in range(streams)])


@pytest.mark.gpu
@pytest.mark.parametrize("streams", (1, 7, 15))
@pytest.mark.parametrize("n", ALPHABETS)
def test_live_and_idle_lanes_in_one_wave(H, opts, n, streams):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    run(dc, [long_stream(n, i, LONG[0]) for i in range(streams)], shifts=[(7 * i + 2) % 16 for i in range(streams)])


@pytest.mark.gpu
def test_two_quarter_crossing_at_every_alignment(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    others = list(S.the_set()[1:WAVE])
    for j, p in sorted(T16.prefix_for_alignment().items()):
        item = T16.hot_prefixed(p)
        shift = (j - stream_info(item[2]).words + 256 * 16) % 16
        in_off = run(dc, [item] + others, shifts=[shift] * WAVE)
        assert (int(in_off[0]) + stream_info(item[2]).words) % 16 == j


@pytest.mark.gpu
def test_quarter_stream_leaves_the_sixteen_step_trips_early(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(S.the_set())
    run(dc, [T16.quarter_stream()] + items[:14], shifts=[(5 * i + 1) % 16 for i in range(WAVE)])


@pytest.mark.gpu
@pytest.mark.parametrize("place", (0, 7, 14))
def test_stream_without_words_among_ordinary_ones(H, opts, place):
    """`words` of the empty stream 16-byte aligned (avail == 0) and 6 bytes behind a boundary (avail == 6, one chunk)."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    nw = no_words()
    items = ordinary()[:place] + [nw] + ordinary()[place:]
    wpos = stream_info(nw[2]).words
    for off in (0, 6):
        shifts = [(3 * i + 1) % 16 for i in range(WAVE)]
        shifts[place] = (off - wpos) % 16
        in_off = run(dc, items, shifts=shifts)
        assert (int(in_off[place]) + wpos) % 16 == off
    # one repeated byte beside them: decoded as before, on another row kind
    items = ordinary()[:place] + [one_byte()] + ordinary()[place:]
    what, raws = [name for name, _, _ in items], [raw for _, raw, _ in items]
    st, osz, got, route, _ = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    assert route["l1"] == 14 and sum(route[k] for k in ROUTES) == WAVE, route


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("first", "last"))
def test_stream_without_words_at_the_edge_of_the_allocation(H, opts, where):
    """The input tensor begins or ends exactly with the stream that has no words; `words` aligned (avail == 0: the request
    must go to the states in front) and at every other alignment the layout allows."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    nw = no_words()
    wpos, others = stream_info(nw[2]).words, ordinary()
    assert wpos == len(nw[2])
    for align in (0, 5):
        if where == "first":
            # the allocation is 16-byte aligned, so `words` of a stream at offset 0 lies at wpos: pad the others behind it
            items = [nw] + others
            offs, pos = [0], (len(nw[2]) + 255) // 256 * 256
            for _, _, s in others:
                offs.append(pos + 3)
                pos = (offs[-1] + len(s) + 511) // 256 * 256
            total = pos
            if align:
                continue                                     # (one alignment: that of wpos itself)
        else:
            items = others + [nw]
            offs, pos = [], 256
            for _, _, s in others:
                offs.append(pos + 3)
                pos = (offs[-1] + len(s) + 511) // 256 * 256
            offs.append(pos + (align - wpos) % 16)
            total = offs[-1] + len(nw[2])                     # the tensor ends with the last state byte
            assert (offs[-1] + wpos) % 16 == align and total == offs[-1] + wpos
        what = [name for name, _, _ in items]
        raws = [raw for _, raw, _ in items]
        st, osz, got, route = decode_at(dc, [s for _, _, s in items], [len(r) for r in raws], what, offs, total)
        bad = mismatches(what, st, osz, got, raws)
        assert not bad, bad
        check_route(route, {"l1": WAVE})


@pytest.mark.gpu
def test_context_without_a_table_behind_trips_of_sixteen(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = ordinary()[:6] + [hostile()] + ordinary()[6:]
    what, raws = [name for name, _, _ in items], [raw for _, raw, _ in items]
    sizes = [len(r) + (4 if name == "hostile" else 0) for name, r in zip(what, raws)]
    st, osz, got, route, _ = decode(dc, [s for _, _, s in items], sizes, what, [(3 * i + 1) % 16 for i in range(WAVE)])
    assert st[6] == ST_CONTEXT, st
    bad = mismatches(what[:6] + what[7:], st[:6] + st[7:], osz[:6] + osz[7:], got[:6] + got[7:], raws[:6] + raws[7:])
    assert not bad, bad
    check_route(route, {"l1": WAVE})


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    from test_gpu_routes import _expected_level
    for n in ALPHABETS:
        assert _expected_level(n, 0, 0) == "l1"
        for length in LONG:
            for i in range(WAVE if length <= 16384 else 3):
                name, raw, s = long_stream(n, i, length)
                info = stream_info(s)
                assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == n, (name, info)
                assert len(set(raw)) == n - 1 and info.nwords - PAD // 2 >= 4 * ENTRY_WORDS, name
    # the stream without words: coded, 46 symbols, 10 bits, and its payload ends with the states
    name, raw, s = no_words()
    info = stream_info(s)
    assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == 46, info
    assert info.nwords == 0 and info.words == len(s) and len(raw) == NOWORDS_N
    assert S.model(s)[0] == raw
    # one repeated byte: coded, order 1, but two symbols - not packed rows
    info = stream_info(one_byte()[2])
    assert info.coded and info.order == 1 and info.nsym == 2 and _expected_level(2, 0, 0) == "l2", info
    # the hostile stream: coded, 46 symbols, its last byte's value nowhere else, the size field four above the data
    name, raw, s = hostile()
    info = stream_info(s)
    assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == 46, info
    assert raw.count(raw[-1:]) == 1 and _varint(s, 1)[0] == len(raw) + 4
    assert info.nwords - PAD // 2 >= 4 * ENTRY_WORDS
    # damaged tables: none of the fixture's reaches packed rows
    assert damaged_on_packed_rows() == []
