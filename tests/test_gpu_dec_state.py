"""The state update and the output bookkeeping of the decode chain on packed rows of layout 2
(htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2).  `finish` takes the start of the symbol out of the rotated dword
with 1 added to every field, so that no mask is needed (tests/test_dec_state_cpu.py), and the body of sixteen steps books
a step's byte and flags in the shadow of the next step's group read.  What can go wrong there: the field before a row's
first symbol (it reads 1023 and must come out as 0), a carry from one field into the next, m at the first and at the last
slot of a symbol, a symbol that owns all 1,024 slots, and a byte or a flag booked once too often or not at all where the
16-step loop is entered, skipped or left.

Streams are made by the CPU oracle and decoded by rans4x16_hip_uncompress_dev_sized; the decoded bytes are compared with
the RAW INPUT, never with output of the code under test, and every case asserts its route as l1 (the options of
test_gpu_dec_shadow.py).

Alphabets of n = 46 and 48 symbols, byte values 0 .. n - 1 (byte 0 is a symbol like the others, so the rows in which it
has a frequency have first = 0), order 1, 10-bit tables.  A long stream (4,096, 4,099, 16,384 or 65,537 bytes, 256 zero
bytes behind it as test_gpu_dec_trip16.py pads, so that the 16-step trips run up to the last steps) holds
  * a hub symbol H_i followed once by every symbol of the alphabet: its row is a FULL row, whose first and last symbol are
    decoded, and with them the ranks 0, 1, 2 (the three field positions of dword 0) and 45 (46 symbols) or 45, 46, 47 (48
    symbols: the three positions of dword 15, the last one's end being the top field of the dword behind the group);
  * the last symbol Z = n - 1 there and nowhere else, always followed by byte 0: the row of Z has ONE symbol of frequency
    1,024, whose start is the 1023 of "nothing before";
  * H_i followed 1,100 times by one of a few wide symbols, one per group of twelve: H_i is seen more than 1,024 times, so
    the successors seen once get frequency 1 (m is their first AND last slot) beside wide ones of about 270, where m
    meets the first and the last slot on its own;
  * uniform draws from the other symbols up to its length.
The short streams are 63, 64, 65 and 127 uniform bytes from the order-1 coder itself (the front end stores blocks this
small): chains of 15, 16, 16 and 31 steps, the fourth chain of a stream with its 3, 0, 1 and 3 bytes more, as made (fewer
than 64 words: the 16-step loop is skipped) and padded (entered for one trip, then left with 0, 1 and 18 steps to go, or -
63 bytes - never entered because three chains have fifteen steps).
The model of test_dec_pivot_cpu.py decodes the 4,096-byte streams and says what they reach; the GPU tests assert that
coverage before they trust the GPU run."""
import functools

import numpy as np
import pytest

import test_dec_pivot_cpu as P
import test_gpu_dec_pivot as V
import test_gpu_dec_shadow as S
from test_gpu_dec_step import H, check_route, decode, device, mismatches, stream_info, uniform  # noqa: F401
from test_gpu_dec_trip16 import ENTRY_WORDS, PAD, o1_coded, padded

ALPHABETS = (46, 48)
LONG = (4096, 4099, 16384, 65537)
SHORT = (63, 64, 65, 127)
WAVE = 15
VISITS = 1100
OPTS = S.OPTS


# ---- generators ---------------------------------------------------------------------------------------------------
def hub_of(n, i):
    return (5 * i + 1) % (n - 1)                            # never Z


def wide_of(n, i):
    return [s for s in range((5 + i) % 12, n - 1, 12) if s != hub_of(n, i)]


@functools.lru_cache(maxsize=None)
def long_stream(n, i, length):
    """(name, raw, stream + PAD zero bytes)."""
    import cpu_libs
    rng = np.random.default_rng(100000 * n + 16 * length + i)
    hub, wide, z = hub_of(n, i), wide_of(n, i), n - 1
    seq = []
    for s in range(n):
        seq += [hub, s] + ([0] if s == z else [])
    for v in range(VISITS):
        seq += [hub, wide[v % len(wide)]]
    others = np.array([v for v in range(n - 1) if v != hub])
    seq += others[rng.integers(0, len(others), size=length - len(seq))].tolist()
    raw = np.array(seq, dtype=np.uint8).tobytes()
    assert len(raw) == length
    return ("n%d/%d/%d" % (n, length, i), raw, cpu_libs.oracle().compress(raw, 1) + bytes(PAD))


@functools.lru_cache(maxsize=None)
def short_wave(n, length):
    """[(name, raw, stream)]: 15 streams of `length` uniform bytes, every symbol once at the front."""
    a = np.arange(n, dtype=np.uint8)
    raws = [uniform(length, a, 7700 * n + 16 * length + i) for i in range(WAVE)]
    return [("n%d/%d/%d" % (n, length, i), raw, o1_coded(raw)) for i, raw in enumerate(raws)]


# ---- the model: what the streams reach ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reached(n, i, length):
    """The stream decoded with the layout-2 look-up of test_dec_pivot_cpu.py: (decoded bytes, the set of (g, q, r, m is
    the symbol's first slot, m is its last slot, the symbol owns the row, it is the first / the last symbol of a full row)
    of its steps)."""
    _, _, s = long_stream(n, i, length)
    info, size, syms, freqs, pos = V.table_of(s)
    assert info.nsym == n and pos + 16 == info.words and syms.tolist() == list(range(n))
    rows = {c: P.build_row(f.tolist()) for c, f in freqs.items() if f.sum()}
    full = {c for c, f in freqs.items() if (f > 0).all()}
    x = [int(v) for v in np.frombuffer(s[pos:pos + 16], dtype="<u4")]
    words = np.frombuffer(s[info.words:info.words + 2 * info.nwords], dtype="<u2").tolist()
    q = size >> 2
    out = bytearray(size)
    ctx, at, seen, memo = [0, 0, 0, 0], 0, set(), {}
    for t in range(q + (size & 3)):
        for k in (range(4) if t < q else (3,)):
            m = x[k] & 1023
            hit = memo.get((ctx[k], m))
            if hit is None:
                root, leaf, first, _ = rows[ctx[k]]
                _, _, pq, g, r, sym, freq, off = P.lookup(root, leaf, first, m, P.pick2)
                isfull = ctx[k] in full
                hit = memo[(ctx[k], m)] = (sym, freq, off, (g, pq, r, off == 0, off == freq - 1, freq == 1024,
                                                             isfull and sym == 0, isfull and sym == n - 1))
            sym, freq, off, what = hit
            seen.add(what)
            x[k] = freq * (x[k] >> 10) + off
            ctx[k] = sym
            out[k * q + t] = sym
            if x[k] < (1 << 15) and at < len(words):
                x[k] = (x[k] << 16) | words[at]
                at += 1
    assert at <= info.nwords - PAD // 2                    # a well-formed stream never asks for the padding
    return bytes(out), frozenset(seen)


def assert_coverage(n, streams=WAVE):
    seen = set()
    for i in range(streams):
        out, what = reached(n, i, LONG[0])
        assert out == long_stream(n, i, LONG[0])[1], (n, i)          # the model decodes the stream: its steps are the chain's
        seen |= what
    assert any(w[5] for w in seen), n                                 # a one-symbol row: its start is the 1023 before it
    assert any(w[6] for w in seen) and any(w[7] for w in seen), n     # the first and the last symbol of a full row
    ranks = {(w[0], w[1], w[2]) for w in seen}
    last = [(3, 3, r) for r in range(3) if 45 + r < n]
    assert {(0, 0, 0), (0, 0, 1), (0, 0, 2)} | set(last) <= ranks, (n, sorted(ranks))   # every position of dwords 0 and 15
    for g, pq, r in [(0, 0, 0), (0, 0, 1), (0, 0, 2)] + last:
        hits = [w for w in seen if w[:3] == (g, pq, r)]
        assert any(w[3] for w in hits) and any(w[4] for w in hits), (n, g, pq, r)         # m == cum and m == cur there
    assert any(w[3] and not w[4] for w in seen) and any(w[4] and not w[3] for w in seen), n
    return seen


# ---- GPU ----------------------------------------------------------------------------------------------------------
def run(dc, items, shifts=None):
    what = [name for name, _, _ in items]
    raws = [raw for _, raw, _ in items]
    st, osz, got, route, _ = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    check_route(route, {"l1": len(items)})


@pytest.mark.gpu
@pytest.mark.parametrize("length", LONG)
@pytest.mark.parametrize("n", ALPHABETS)
def test_long_streams(H, opts, n, length):
    assert_coverage(n, 3)
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    streams = WAVE if length <= 16384 else 3
    run(dc, [long_stream(n, i, length) for i in range(streams)], shifts=[(3 * i + n) % 16 for i in range(streams)])


@pytest.mark.gpu
@pytest.mark.parametrize("streams", (1, 7, 15))
@pytest.mark.parametrize("n", ALPHABETS)
def test_live_and_idle_lanes_in_one_wave(H, opts, n, streams):
    """1, 7 and 15 streams in a call: the other lanes of the wave are idle and run the fast trips on garbage."""
    assert_coverage(n, streams)
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    run(dc, [long_stream(n, i, LONG[0]) for i in range(streams)], shifts=[(7 * i + 2) % 16 for i in range(streams)])


@pytest.mark.gpu
@pytest.mark.parametrize("length", SHORT)
@pytest.mark.parametrize("n", ALPHABETS)
def test_short_streams_around_the_sixteen_step_loop(H, opts, n, length):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = short_wave(n, length)
    run(dc, items)
    run(dc, padded(items), shifts=[(3 * i + length) % 16 for i in range(WAVE)])
    run(dc, padded(items)[:7] + items[7:8])                # one stream without words to spare: the loop is skipped for all


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALPHABETS)
def test_cases_are_what_they_claim(n):
    """No GPU.  Coded, order 1, n symbols, 10 bits, on the packed-row route; the coverage the GPU tests rely on, from
    one stream alone as well; the short streams have the steps and the words that enter, skip and leave the 16-step loop."""
    from test_gpu_routes import _expected_level
    assert _expected_level(n, 0, 0) == "l1"
    for streams in (1, 3, 7, WAVE):
        assert_coverage(n, streams)
    for length in LONG:
        for i in range(WAVE if length <= 16384 else 3):
            name, raw, s = long_stream(n, i, length)
            info = stream_info(s)
            assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == n, (name, info)
            assert set(raw) == set(range(n)) and info.nwords - PAD // 2 >= 4 * ENTRY_WORDS, name
            z = np.frombuffer(raw, dtype=np.uint8)
            assert (z[1:][z[:-1] == n - 1] == 0).all() and (z == n - 1).sum() == 1, name
    for length in SHORT:
        for name, raw, s in short_wave(n, length):
            info = stream_info(s)
            assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == n, (name, info)
            assert (len(raw) >> 2, (len(raw) >> 2) + (len(raw) & 3)) == {63: (15, 18), 64: (16, 16), 65: (16, 17), 127: (31, 34)}[length]
            assert info.nwords < ENTRY_WORDS <= info.nwords + PAD // 2, (name, info.nwords)
