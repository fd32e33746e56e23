"""The packed-row step of the decode chain (htscodecs_amd/csrc/r4x16_decode.hip: lookup_step_pk and the layout-2 step of
chain_decode_lds) where it is laid out around its reads: in steps 1 .. 7 of a trip the ring address and the ring reads
are issued BEHIND the look-up's group read, from a cursor that is advanced over the words of the step before in that same
shadow, and the last step of a trip advances it itself.  A wrong count, a count added twice or a step late, a ring read
from the cursor of the step before: each shows as soon as the lanes of a wave take words at different rates, at every
alignment of the ring, and in slow trips (whose `take` test reads the cursor) as well as in fast ones.
test_gpu_dec_step.py stays the yardstick of the loop as a whole; this file adds waves whose streams diverge.

Streams are made by the CPU oracle and decoded by rans4x16_hip_uncompress_dev_sized; the decoded bytes are compared with
the RAW INPUT, never with output of the code under test, and every case asserts its route as l1.

The set: 15 streams of 46-symbol order-1 alphabets with 10-bit tables - 15 is what a wave of the 46-symbol class holds, so
lanes 32 .. 59 are live - of 8 KiB plus 0 .. 7 bytes, every one with another word rate:
  * `hot`: 15 hub symbols with runs of about 520 bytes each, and in the middle of every quarter of the block (where all
    four chains reach it in the same steps) a walk over the hubs that takes every ordered pair of two hubs once.  A
    context of 513 .. 1,024 symbols is normalised to 512 (compute_shift: the power of two above its total, halved below
    64 symbols) and scaled to 1,024, so a successor seen once has frequency 2 of 1,024 and costs 9 bits: 9/16 word per
    chain and step for the 52 steps of the walk, 36 bytes of words per trip - the most a 10-bit table sustains is 10/16.
    A block of 8 KiB cannot hold it for longer: a context has to be 513 symbols long for every symbol of the walk;
  * `cyclic`: every symbol followed by the same next one - next to no words before its tail;
  * 13 `drift` streams between them: the cyclic successor with probability p, any symbol otherwise, p from 0.97 down to
    0 (uniform successors: about 5.5 bits a symbol through the whole block).
Lengths 8192 + (0 .. 7): hundreds of fast trips each, many crossings of every ring quarter, slow trips at the end.  Every
stream ends each quarter in 64 bytes of uniform data: a trip is fast only while every stream of the wave has 32 words
left, and without words of their own at the end the slow streams would make the wave's last hundreds of trips slow.
The last case wants exactly that: a cyclic stream of 2,053 bytes without such a tail has fewer than 32 words in all, so
every trip of its wave is slow from the first one on, beside 14 streams that run four times as long.

The CPU test at the end decodes every stream with a model of the chain in this file (checked against the raw input) and
pins what the cases claim: entropy-coded, order 1, 46 symbols, 10 bits; the words per step of the fastest and the
slowest stream a factor of 8 apart and all 15 rates different; trips that cross a ring quarter (one crossing is the
most: a trip takes at most 32 words) and trips that cross none, at every alignment; the hot stretch at its rate."""
import collections
import functools

import numpy as np
import pytest

from test_gpu_confinement import _varint
from test_gpu_dec_step import H, _alphabet_of, alphabet, check_route, decode, device, mismatches, stream_info  # noqa: F401

NSYM, BITS, TRIP = 46, 10, 8
BASE = 8192
OPTS = {"dec_direct": 0, "dec_mid": 0, "dec_short_ring": 0}
HUBS = 15
DRIFT_P = (0.97, 0.94, 0.9, 0.85, 0.8, 0.72, 0.64, 0.55, 0.45, 0.35, 0.25, 0.12, 0.0)
TAIL = 64                         # bytes of uniform data at the end of every quarter of every stream of the set
SHORT_N = 2053                    # the short stream of the last case: cyclic, a quarter of the others' steps


# ---- generators ---------------------------------------------------------------------------------------------------
def _hub_walks():
    """An Euler circuit of the complete digraph on the hubs (every ordered pair of two hubs once), cut into four walks."""
    nxt = {h: [j for j in range(HUBS) if j != h] for h in range(HUBS)}
    stack, circuit = [0], []
    while stack:                                            # Hierholzer
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    arcs = len(circuit) - 1
    assert arcs == HUBS * (HUBS - 1) and len(set(zip(circuit, circuit[1:]))) == arcs
    cut = [arcs * k // 4 for k in range(5)]
    return [circuit[cut[k]:cut[k + 1] + 1] for k in range(4)]


def hot(n, a):
    q = n >> 2
    walks = _hub_walks()
    out = np.empty(n, dtype=np.uint8)
    hubs_of = [[h for h in range(HUBS) if h % 4 == k] for k in range(4)]         # the runs of quarter k
    others = list(range(HUBS, len(a)))
    for k in range(4):
        lo, hi = k * q, ((k + 1) * q if k < 3 else n)
        walk = walks[k]
        # the symbols that are no hubs once each (what makes the alphabet 46 symbols), then runs, the walk, runs
        head = others[k::4]
        at = (q - len(walk)) // 2                           # the walk starts at the same step in every quarter
        room = (hi - lo) - len(head) - len(walk)
        runs = hubs_of[k]
        before, after = at - len(head), room - (at - len(head))
        # runs before the walk end in the walk's first hub, runs after it start from its last: no new pair at the joints
        pre = [h for h in runs if h != walk[0]] + [walk[0]]
        post = [walk[-1]] + [h for h in runs if h != walk[-1]]
        seq = list(head)
        for part, total in ((pre, before), (None, 0), (post, after)):
            if part is None:
                seq += walk
                continue
            for i, h in enumerate(part):
                m = total // len(part) + (1 if i < total % len(part) else 0)
                seq += [h] * m
        assert len(seq) == hi - lo, (k, len(seq), hi - lo)
        out[lo:hi] = a[np.array(seq)]
    return out.tobytes()


def cyclic(n, a):
    return np.resize(a, n).tobytes()


def drift(n, a, p, seed):
    """The next symbol of the alphabet's cycle with probability p, any symbol otherwise; every symbol once at the front."""
    rng = np.random.default_rng(seed)
    step = np.where(rng.random(n) < p, 1, rng.integers(0, len(a), size=n))
    idx = np.cumsum(step) % len(a)
    idx[:len(a)] = np.arange(len(a))
    return a[idx].tobytes()


def with_tail(raw, a, seed):
    """The last TAIL bytes of every quarter replaced by uniform draws: the stream keeps more than a trip's words ahead of
    its cursor until its last trips, so it does not turn the whole wave's trips into slow ones (a trip is fast only if
    EVERY stream of the wave has 32 words left)."""
    out = np.frombuffer(raw, dtype=np.uint8).copy()
    rng = np.random.default_rng(seed)
    q = len(out) >> 2
    for k in range(4):
        out[(k + 1) * q - TAIL:(k + 1) * q] = a[rng.integers(0, len(a), size=TAIL)]
    return out.tobytes()


@functools.lru_cache(maxsize=None)
def the_set():
    """[(name, raw, stream)] of the 15 streams, lengths BASE + (0 .. 7)."""
    import cpu_libs
    a = alphabet(NSYM, 1)
    raws = [("hot", hot(BASE + 3, a)), ("cyclic", cyclic(BASE + 6, a))]
    raws += [("drift%.2f" % p, drift(BASE + (i + 1) % 8, a, p, 7001 + i)) for i, p in enumerate(DRIFT_P)]
    raws = [(name, with_tail(raw, a, 6001 + i)) for i, (name, raw) in enumerate(raws)]
    orc = cpu_libs.oracle()
    return [(name, raw, orc.compress(raw, 1)) for name, raw in raws]


@functools.lru_cache(maxsize=None)
def short_stream():
    import cpu_libs
    raw = cyclic(SHORT_N, alphabet(NSYM, 1))
    return ("short", raw, cpu_libs.oracle().compress(raw, 1))


# ---- a model of the chain: what each step takes (numpy and the table of the stream only) --------------------------
def _o1_freqs(s, pos, bits):
    """{context byte: (symbols, frequencies scaled to 1 << bits)} of an order-1 table (rANS_static4x16pr.c:869-960)."""
    syms, pos = _alphabet_of(s, pos)
    rows = {}
    for c in syms:
        f, zeros = [], 0
        for _ in syms:
            if zeros:
                zeros -= 1
                f.append(0)
                continue
            v, pos = _varint(s, pos)
            f.append(v)
            if v == 0:
                zeros = s[pos]
                pos += 1
        f = np.array(f, dtype=np.int64)
        tot = int(f.sum())
        if tot:
            assert tot & (tot - 1) == 0 and tot <= 1 << bits, (c, tot)
            f *= (1 << bits) // tot
        rows[c] = f
    return np.array(syms), rows, pos


@functools.lru_cache(maxsize=None)
def model(s):
    """(decoded bytes, words taken per step) of a plain order-1 stream: four chains, chain k on quarter k and chain 3 on
    the rest, refilled in the order 0 .. 3 in every step (rANS_static4x16pr.c:1033-1059)."""
    info = stream_info(s)
    assert info.coded and info.order == 1
    n, pos = _varint(s, 1)
    bits = s[pos] >> 4
    if info.nested:                                         # the table travels as an order-0 stream (stream_info)
        import cpu_libs
        usz, pos = _varint(s, pos + 1)
        csz, pos = _varint(s, pos)
        src = np.frombuffer(s[pos:pos + csz], dtype=np.uint8)
        tab = np.zeros(usz + 16, dtype=np.uint8)
        assert cpu_libs.oracle().lib.orc_o0_decode(src.ctypes.data, csz, tab.ctypes.data, usz) == 0
        syms, rows, used = _o1_freqs(tab.tobytes(), 0, bits)
        assert used == usz
        pos += csz
    else:
        syms, rows, pos = _o1_freqs(s, pos + 1, bits)
    assert pos + 16 == info.words
    cum = {c: np.concatenate(([0], np.cumsum(f))) for c, f in rows.items()}
    x = [int(v) for v in np.frombuffer(s[pos:pos + 16], dtype="<u4")]
    words = np.frombuffer(s[info.words:info.words + 2 * info.nwords], dtype="<u2")
    q, mask = n >> 2, (1 << bits) - 1
    out = np.zeros(n, dtype=np.uint8)
    ctx, at = [0, 0, 0, 0], 0
    steps = q + (n & 3)
    taken = np.zeros(steps, dtype=np.int64)
    for t in range(steps):
        for k in (range(4) if t < q else (3,)):
            m = x[k] & mask
            c = cum[ctx[k]]
            j = int(np.searchsorted(c, m, side="right")) - 1
            x[k] = int(c[j + 1] - c[j]) * (x[k] >> bits) + m - int(c[j])
            ctx[k] = int(syms[j])
            out[k * q + t] = ctx[k]
            if x[k] < (1 << 15) and at < len(words):
                x[k] = (x[k] << 16) | int(words[at])
                at += 1
                taken[t] += 1
    return out.tobytes(), taken


def crossings(taken, off0):
    """Ring quarters (64 bytes) that the cursor enters in each trip of eight steps, the stream's words starting off0 bytes
    behind a 16-byte boundary."""
    ends = off0 + 2 * np.cumsum(taken)[TRIP - 1::TRIP]
    return np.diff(np.concatenate(([off0], ends)) >> 6)


# ---- GPU ----------------------------------------------------------------------------------------------------------
def run(dc, items, shifts=None):
    what = [name for name, _, _ in items]
    raws = [raw for _, raw, _ in items]
    st, osz, got, route, in_off = decode(dc, [s for _, _, s in items], [len(r) for r in raws], what, shifts)
    bad = mismatches(what, st, osz, got, raws)
    assert not bad, bad
    check_route(route, {"l1": len(items)})
    return in_off


@pytest.mark.gpu
def test_diverging_cursors_at_every_alignment(H, opts):
    """The 15 streams in one wave (sched_sort = 0: in the order given), the whole set laid at each of the 16 byte
    alignments of the input arena in turn."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(the_set())
    for j in range(16):
        in_off = run(dc, items, shifts=[j] * len(items))
        assert {int(o) % 16 for o in in_off} == {j}


@pytest.mark.gpu
def test_wave_half_empty(H, opts):
    """8 streams: quads 8 .. 15 of the wave hold no stream (idle lanes run the fast trips on garbage)."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(the_set())
    run(dc, items[:2] + items[2::2][:6])
    run(dc, items[:8], shifts=[(3 * i + 1) % 16 for i in range(8)])


@pytest.mark.gpu
def test_short_stream_forces_slow_trips(H, opts):
    """A cyclic stream of 2,053 bytes in the same wave: fewer than 32 words in all, so no trip of the wave is fast, and it
    ends after a quarter of the others' steps - the long streams run their whole length in slow trips, whose `take`
    test reads the cursor that the shadow advances."""
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    items = list(the_set())
    run(dc, [short_stream()] + items[:14])
    run(dc, items[:7] + [short_stream()] + items[7:14], shifts=[(5 * i + 2) % 16 for i in range(15)])


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    items = list(the_set()) + [short_stream()]
    assert len(the_set()) == 15 and {len(r) - BASE for _, r, _ in the_set()} == set(range(8))
    rate = {}
    cross = collections.Counter()
    for name, raw, s in items:
        i = stream_info(s)
        assert i.coded and i.order == 1 and i.nsym == NSYM and i.bits == BITS, (name, i)
        out, taken = model(s)
        assert out == raw, name                             # the model decodes the stream: its word counts are the chain's
        assert int(taken.sum()) == i.nwords, (name, int(taken.sum()), i.nwords)
        rate[name] = taken.sum() / len(taken)
        for off0 in range(16):
            c = crossings(taken, off0)
            assert c.max() <= 1, name                       # (8 steps x 4 chains x 2 bytes = one quarter at the most)
            cross.update(c.tolist())
    del rate["short"]
    print("words per step:", {k: round(float(v), 3) for k, v in rate.items()})
    print("trips by quarters crossed:", dict(cross))
    # every stream another rate, the extremes a factor of 8 apart (in fact far more: the cyclic stream takes a few words in all)
    assert len({round(float(v), 4) for v in rate.values()}) == 15, rate
    assert max(rate.values()) >= 8 * max(min(rate.values()), 1e-9), rate
    assert min(rate, key=rate.get) == "cyclic" and max(rate, key=rate.get) == "drift0.00", rate
    assert cross[0] > 0 and cross[1] > 0, cross
    # the hot stretch: the walk takes every pair of hubs once, 52 or 53 steps per chain, all chains in the same steps.
    # A successor of frequency 2 / 1,024 costs 9 bits, 36 bytes of words per trip of 32 symbols; a pair that the runs' joints
    # or the tails use a second time has frequency 4 and costs 8.  So every whole trip inside the walk takes at least 32
    # bytes (8 bits a symbol) - against 22 where successors are uniform over 45 symbols.
    _, taken = model(the_set()[0][2])
    q = (BASE + 3) >> 2
    walk = HUBS * (HUBS - 1) // 4
    first = ((q - walk) // 2 + TRIP - 1) // TRIP + 1        # first whole trip inside the walk, one trip of margin
    per_trip = 2 * taken[:len(taken) // TRIP * TRIP].reshape(-1, TRIP).sum(axis=1)
    hot_trips = per_trip[first:first + 5]
    print("bytes of words per trip in the hot stretch:", hot_trips.tolist(), "elsewhere (median):", int(np.median(per_trip)))
    assert hot_trips.min() >= 32, hot_trips
    # the short stream never has a trip's words ahead of it; every stream of the set has, until its last trips
    assert stream_info(short_stream()[2]).nwords < 4 * TRIP
    for name, _, s in the_set():
        _, taken = model(s)
        left = stream_info(s).nwords - np.cumsum(taken)
        fast = int(np.argmax(left < 4 * TRIP)) if (left < 4 * TRIP).any() else len(left)
        print(name, "words", stream_info(s).nwords, "steps with 32 words left:", fast, "of", len(taken))
        assert fast >= len(taken) - TAIL - TRIP, (name, fast)
