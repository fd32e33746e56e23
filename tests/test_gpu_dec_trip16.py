"""The 16-step trips of the decode chain on packed rows of layout 2 (htscodecs_amd/csrc/r4x16_decode.hip:
chain_decode_pk2).  A wave runs them while EVERY one of its streams has sixteen steps and 64 words left, then hands
over to the 8-step loop at a step count tb that is a multiple of 16, with everything up to tb booked and stored, the
cursor whole, all four ring quarters live and the next quarter in registers.  What can go wrong there and nowhere else:
  * the hand-over: the first 8-step trip must not book step tb again, and if no trip follows at all (every count equal
    to tb) the tail must not store queued dwords that do not exist;
  * a trip that moves the cursor over TWO quarter boundaries: both quarters waiting in registers are parked, at every
    alignment of the ring, the 8-byte wrap copy after slot 0 included;
  * waves that leave the 16-step trips early (one short stream) or never enter them (one stream of fewer than 64 words).

Streams are made by the CPU oracle and decoded by rans4x16_hip_uncompress_dev_sized; the decoded bytes are compared with
the RAW INPUT, never with output of the code under test, and every case asserts its route as l1.

Lengths around the hand-over: 15 streams (one full wave of the 46-symbol class) of 46-symbol order-1 alphabets with
10-bit tables and the same length n = 4 c + r, for c in 15, 16, 17, 31, 32, 33, 47, 48, 49 and every r in 0 .. 3.  The
oracle's front end stores blocks this small, so the streams come from its order-1 coder itself (orc_o1_encode) behind
the two header bytes the front end would write.  Each length runs twice:
  * as the coder made it: fewer than 64 words in all (a step takes at most 10 bits per chain), so the 16-step trips are
    never entered - the word test decides before the step test can;
  * with 256 zero bytes behind the stream (the decoder is given the longer size; a well-formed stream never asks for
    them: its states end at the encoder's start state): now the step test decides, the wave runs c // 16 trips of
    sixteen and leaves at tb = 16, 32, 48 with 0 .. 17 steps left for the 8-step loop.  c = 16, 32, 48 with r = 0 is the
    wave that no 8-step trip follows.
c = 1 (n = 4 .. 7) cannot hold 46 symbols and the oracle stores it; it is decoded and compared all the same and must not
reach the chain.

Two crossings in one trip: the `hot` stream of test_gpu_dec_shadow.py sustains 9/16 word per chain and step for the 52
steps of its walk, 72 bytes per trip of sixteen.  Its length decides at which step - and at which cursor - the walk
begins: `prefix` p lengthens every quarter by 2 p bytes, so the walk starts p steps later.  For each of the 16 byte
alignments of the input one prefix of 0 .. 15 is chosen (by the model below) under which a trip of the walk crosses two
quarters; the stream runs beside the 14 slower streams of that file.

The CPU test decodes every stream with the model of test_gpu_dec_shadow.py (checked against the raw input) and pins
what the cases claim."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_dec_shadow as S
from test_gpu_confinement import _varint  # noqa: F401
from test_gpu_dec_step import H, alphabet, check_route, decode, device, mismatches, stream_info, uniform  # noqa: F401

NSYM, BITS = S.NSYM, S.BITS
TRIP16, ENTRY_WORDS = 16, 64
CS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49)
PAD = 256                          # zero bytes behind a padded stream: 128 words, the cursor never comes within 64 of the end
WAVE = 15
QUARTER_N = 2053                   # the short stream of the third case: a quarter of the others' steps
OPTS = S.OPTS


# ---- generators ---------------------------------------------------------------------------------------------------
def _varint_put(v):
    out = []
    while True:
        out.insert(0, (v & 0x7f) | (0x80 if out else 0))
        v >>= 7
        if not v:
            return bytes(out)


def o1_coded(raw):
    """The order-1 stream of `raw` as the oracle's coder makes it, behind the front end's header (flags = order 1, size):
    what orc_rans_compress_to_4x16 writes when it does not fall back to a stored block."""
    import cpu_libs
    lib = cpu_libs.oracle().lib
    lib.orc_rans_compress_bound_4x16.restype = C.c_uint
    lib.orc_rans_compress_bound_4x16.argtypes = [C.c_uint, C.c_int]
    lib.orc_o1_encode.restype = C.c_int
    lib.orc_o1_encode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.POINTER(C.c_uint)]
    src = np.frombuffer(raw, dtype=np.uint8).copy()
    cap = lib.orc_rans_compress_bound_4x16(len(raw), 1)
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_uint(0)
    assert lib.orc_o1_encode(src.ctypes.data, len(raw), out.ctypes.data, cap, C.byref(n)) == 0
    return b"\x01" + _varint_put(len(raw)) + out[:n.value].tobytes()


@functools.lru_cache(maxsize=None)
def length_wave(c, r):
    """[(name, raw, stream)]: 15 streams of 4 c + r bytes.  c = 1: the oracle's own (stored) blocks."""
    import cpu_libs
    n = 4 * c + r
    a = alphabet(NSYM, 1)
    if c == 1:
        orc = cpu_libs.oracle()
        raws = [np.roll(a, i)[:n].tobytes() for i in range(WAVE)]
        return [("n%d/%d" % (n, i), raw, orc.compress(raw, 1)) for i, raw in enumerate(raws)]
    raws = [uniform(n, a, 9100 * c + 10 * r + i) for i in range(WAVE)]
    return [("n%d/%d" % (n, i), raw, o1_coded(raw)) for i, raw in enumerate(raws)]


def padded(items):
    return [(name + "+pad", raw, s + bytes(PAD)) for name, raw, s in items]


@functools.lru_cache(maxsize=None)
def hot_prefixed(p):
    import cpu_libs
    a = alphabet(NSYM, 1)
    raw = S.with_tail(S.hot(S.BASE + 3 + 8 * p, a), a, 6001)
    return ("hot+%d" % p, raw, cpu_libs.oracle().compress(raw, 1))


@functools.lru_cache(maxsize=None)
def quarter_stream():
    """Uniform successors, a quarter as long as the streams of the set: it has words to the end, so the wave runs the
    16-step trips until THIS stream runs out of steps or words, and the 8-step loop takes the others' last three quarters."""
    import cpu_libs
    raw = uniform(QUARTER_N, alphabet(NSYM, 1), 4242)
    return ("quarter", raw, cpu_libs.oracle().compress(raw, 1))


# ---- the model: when a wave leaves the 16-step trips, what a trip crosses ------------------------------------------
def steps_of(s):
    """(steps per chain 0 .. 2, words, words taken per step) of a stream."""
    n, _ = _varint(s, 1)
    _, taken = S.model(s)
    return n >> 2, stream_info(s).nwords, taken


def left_at(streams):
    """tb: the step count at which a wave of these streams leaves the 16-step trips (0: never entered)."""
    info = [steps_of(s) for s in streams]
    cum = [np.concatenate(([0], np.cumsum(taken))) for _, _, taken in info]
    t = 0
    while all(t + TRIP16 <= q and int(c[t]) + ENTRY_WORDS <= nw for (q, nw, _), c in zip(info, cum)):
        t += TRIP16
    return t


def crossings16(taken, off0, tb):
    """Ring quarters that the cursor enters in each of the tb / 16 trips of sixteen."""
    ends = off0 + 2 * np.cumsum(taken)[TRIP16 - 1:tb:TRIP16]
    return np.diff(np.concatenate(([off0], ends)) >> 6)


@functools.lru_cache(maxsize=None)
def prefix_for_alignment():
    """{alignment j: prefix p}: the smallest prefix under which the hot stream, its words starting j bytes behind a
    16-byte boundary (off0 of the ring), has a trip of sixteen that crosses two quarters while its wave is in the
    16-step trips."""
    others = [s for _, _, s in S.the_set()[1:WAVE]]
    chosen = {}
    for p in range(16):
        s = hot_prefixed(p)[2]
        tb = left_at([s] + others)
        _, _, taken = steps_of(s)
        for j in range(16):
            if j not in chosen and crossings16(taken, j, tb).max() == 2:
                chosen[j] = p
    return chosen


# ---- GPU ----------------------------------------------------------------------------------------------------------
def run(dc, items, shifts=None, l1=None):
    what = [name for name, _, _ in items]
    raws = [raw for _, raw, _ in items]
    st, osz, got, route, in_off = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    check_route(route, {"l1": len(items) if l1 is None else l1})
    return in_off


@pytest.mark.gpu
@pytest.mark.parametrize("c", CS)
def test_lengths_around_the_hand_over(H, opts, c):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    for r in range(4):
        items = length_wave(c, r)
        if c == 1:
            run(dc, items, l1=0)
            continue
        run(dc, items)
        run(dc, padded(items), shifts=[(3 * i + r) % 16 for i in range(WAVE)])


@pytest.mark.gpu
def test_two_quarter_crossings_in_one_trip(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    others = list(S.the_set()[1:WAVE])
    for j, p in sorted(prefix_for_alignment().items()):
        # the alignment of the words: the input offset plus where the words start in the stream
        item = hot_prefixed(p)
        shift = (j - stream_info(item[2]).words + 256 * 16) % 16
        in_off = run(dc, [item] + others, shifts=[shift] * WAVE)
        assert (int(in_off[0]) + stream_info(item[2]).words) % 16 == j


@pytest.mark.gpu
def test_streams_leave_at_different_times(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(S.the_set())
    run(dc, [quarter_stream()] + items[:14])
    run(dc, items[:9] + [quarter_stream()] + items[9:14], shifts=[(7 * i + 3) % 16 for i in range(WAVE)])


@pytest.mark.gpu
def test_sixteen_step_trips_never_entered(H, opts):
    """The cyclic stream of 2,053 bytes of test_gpu_dec_shadow.py has fewer than 64 words in all."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(S.the_set())
    run(dc, items[:5] + [S.short_stream()] + items[5:14], shifts=[(11 * i + 5) % 16 for i in range(WAVE)])


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    # lengths: coded, order 1, 46 symbols, 10 bits; plain never enters, padded leaves at 16 * (c // 16)
    for c in CS:
        for r in range(4):
            items = length_wave(c, r)
            assert len(items) == WAVE and all(len(raw) == 4 * c + r for _, raw, _ in items)
            if c == 1:
                assert not any(stream_info(s).coded for _, _, s in items)
                continue
            for name, raw, s in items + padded(items):
                i = stream_info(s)
                assert i.coded and i.order == 1 and i.nsym == NSYM and i.bits == BITS, (name, i)
                out, taken = S.model(s)
                assert out == raw, name
                assert int(taken.sum()) <= i.nwords - (PAD // 2 if name.endswith("+pad") else 0), name
            assert all(stream_info(s).nwords < ENTRY_WORDS for _, _, s in items), (c, r)
            assert left_at([s for _, _, s in items]) == 0
            tb = left_at([s for _, _, s in padded(items)])
            assert tb == TRIP16 * (c // TRIP16), (c, r, tb)
    left = {c: c - TRIP16 * (c // TRIP16) for c in CS if c > 1}
    assert set(left.values()) == {15, 0, 1} and {TRIP16 * (c // TRIP16) for c in left} == {0, 16, 32, 48}

    # two crossings: one prefix for every alignment, and trips with one crossing and with none in the same runs
    chosen = prefix_for_alignment()
    assert sorted(chosen) == list(range(16)), chosen
    others = [s for _, _, s in S.the_set()[1:WAVE]]
    seen = set()
    for j, p in chosen.items():
        name, raw, s = hot_prefixed(p)
        i = stream_info(s)
        assert i.coded and i.order == 1 and i.nsym == NSYM and i.bits == BITS, (name, i)
        out, taken = S.model(s)
        assert out == raw, name
        tb = left_at([s] + others)
        cr = crossings16(taken, j, tb)
        assert cr.max() == 2, (j, p)
        seen.update(cr.tolist())
        per_trip = 2 * taken[:tb].reshape(-1, TRIP16).sum(axis=1)
        assert per_trip.max() > 64 and per_trip.max() <= 128, per_trip.max()
    assert seen == {0, 1, 2}, seen
    print("prefix by alignment:", chosen)

    # the quarter stream ends the 16-step trips of its wave at about a quarter of the others' steps
    qs = quarter_stream()[2]
    i = stream_info(qs)
    assert i.coded and i.order == 1 and i.nsym == NSYM and i.bits == BITS, i
    assert S.model(qs)[0] == quarter_stream()[1]
    set_streams = [s for _, _, s in S.the_set()]
    tb_set = left_at(set_streams[:WAVE])
    tb_q = left_at([qs] + set_streams[:14])
    print("steps in 16-step trips: the set alone", tb_set, "with the quarter stream", tb_q)
    assert 0 < tb_q <= QUARTER_N >> 2 and tb_q % TRIP16 == 0
    assert tb_set >= 3 * tb_q, (tb_set, tb_q)
    # one stream of fewer than 64 words: never entered
    assert stream_info(S.short_stream()[2]).nwords < ENTRY_WORDS
    assert left_at([S.short_stream()[2]] + set_streams[:14]) == 0
