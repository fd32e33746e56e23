"""Inputs of the arith tests (test_arith_cpu.py, test_arith_inputs_cpu.py, test_gpu_arith.py, test_gpu_arith_hostile.py,
test_gpu_arith_trips.py): the reference-made vectors of tests/golden/arith/edge.bin, constructed inputs coded by the
Python model (arith_model.py, itself pinned by those vectors and the 28 fixtures) - among them the ones that drive a
model step by step to an event no text reaches, and the payload sizes of the coder's input window - and damaged variants
of small streams.  Everything is seeded; nothing here needs a GPU."""
import collections
import functools
import os
import random
import struct

import arith_model as M


@functools.lru_cache(maxsize=None)
def edge():
    """tests/golden/arith/edge.bin (its README.md has the layout): (inputs, damaged) - inputs [(what, order, data, stream)],
    damaged [(stream, cap or None, None or (len, sha256 hex))]"""
    raw = open(os.path.join(M.GOLDEN, "edge.bin"), "rb").read()
    assert raw[:8] == b"AREDGE1\n"
    pos = [8]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, raw, pos[0])
        pos[0] += struct.calcsize("<" + fmt)
        return v[0]

    def blob(fmt="I", n=None):
        n = take(fmt) if n is None else n
        pos[0] += n
        return raw[pos[0] - n:pos[0]]

    inputs, damaged = [], []
    for _ in range(take("I")):
        order, what = take("I"), blob("H").decode()
        inputs.append((what, order, blob(), blob()))
    for _ in range(take("I")):
        s, cap = blob(), take("I")
        answer = (take("I"), blob(n=32).hex()) if take("B") else None
        damaged.append((s, None if cap == 0xffffffff else cap, answer))
    assert pos[0] == len(raw)
    return inputs, damaged


def _damage(rng, s):
    s = bytearray(s)
    k = rng.randrange(6)
    if k == 0:
        for _ in range(rng.randrange(1, 4)):
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
    elif k == 1:
        s = s[:rng.randrange(0, len(s))]
    elif k == 2:
        s[rng.randrange(min(12, len(s)))] = rng.randrange(256)
    elif k == 3:
        s[0] = rng.randrange(256)
    elif k == 4:
        a = rng.randrange(len(s))
        s[a:a + rng.randrange(1, 8)] = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 8)))
    else:
        s[rng.randrange(len(s))] = rng.choice((0, 1, 255, 128))
    return bytes(s)


def claim(s):
    """(is a stripe stream, the size it stores or None)"""
    if not s:
        return False, None
    if not s[0] & M.X_STRIPE and s[0] & M.X_NOSZ:
        return False, None
    return bool(s[0] & M.X_STRIPE), M.var_get(s, 1, len(s))[1]


@functools.lru_cache(maxsize=None)
def model_damaged(count=300, seed=7, limit=8192):
    """[(stream, cap)]: damaged variants of model-made streams of at most 8 KB of text.  A stripe stream gets the capacity
    it stores (any other is refused for capacity and tests nothing); streams that claim more than `limit` are left to
    the size tests."""
    rng = random.Random(seed)
    bases = []
    for name in ("q4", "q8", "q40+dir", "qvar"):
        t = M.text(name)
        for order in (0, 1, 64, 65, 128, 129, 192, 193, 8, 9, 8 | (5 << 8), 9 | (2 << 8), 32 | 128):
            n = rng.choice((120, 700, 2500, 8000))
            bases.append((M.compress(t[3000:3000 + n], order), n))
    out, seen = [], set()
    while len(out) < count:
        s0, n0 = rng.choice(bases)
        s = _damage(rng, s0)
        if s in seen or s == s0:
            continue
        seen.add(s)
        stripe, stored = claim(s)
        if stored is not None and stored > limit:
            continue
        cap = stored if stripe else rng.choice((n0, n0, n0 + 5, limit))
        out.append((s, cap))
    return out


def skewed(symbols, n, seed, runs=0, chain=3):
    """n bytes of `symbols`, the early ones the likelier (and every one present), each after its own successor in all but
    one case of `chain`: an order-1 coder beats order 0 on it, and both beat a copy.  runs: one byte in `runs` starts a
    short run."""
    rng = random.Random(seed)
    k = len(symbols)
    out = bytearray(symbols)
    j = 0
    while len(out) < n:
        j = (j * 5 + 1) % k if rng.randrange(chain) else min(int(rng.expovariate(0.25)), k - 1)
        out += bytes([symbols[j]]) * (rng.randrange(2, 9) if runs and not rng.randrange(runs) else 1)
    return bytes(out[:n])


def payload(s):
    """(home, bytes) of the entropy-coded piece of an unstriped stream: the payload as decode_core sees it, at the
    stream's end"""
    ev = collections.Counter()
    cap = None if not s[0] & M.X_NOSZ else 1 << 20
    assert M.uncompress_to(s, cap, events=ev)[0] == 0
    (key,) = [k for k in ev if k[1] == "payload"]
    return key[0], key[2]


# ---- halving and the comparison in one step (c_simple_model.h: halve first, compare then) ---------------------------
def tie_case(p, m, order, twin=False):
    """Raw bytes with the step that tells `halve, then compare` from `compare, then halve`, in the row of one context:
    the entry at list position p is incremented to 18 behind a 17 in the step that halves the model - 9 against 9, no
    swap - and a few symbols behind it that are coded by the list order it left.  The model is driven step by step:
    symbol p once (17, to position p - 1), the filler 0 up to the fourth halving (17 -> 9 -> 5 -> 3 -> 2), symbol p - 1
    once (17, past the 2), the filler until one more step passes MAX_FREQ, symbol p.  twin: that last symbol is p + 4 instead, an untouched 1 behind an untouched 1 - 9 against
    1, the swap in the halving step, at a position of the same kind.  Symbol m - 1 once at the start sets the alphabet.
    order 1: the row of context 0, a filler after every other symbol (decoded in that symbol's row); order 65: the row of
    context 1, the fillers 0 and 1 taking turns so that nothing repeats and the symbol model sees every byte."""
    assert order in (0, 1, 65) and 2 <= p and p + 4 < m - 2
    row, out, halvings = M.Model(m), bytearray([1] if order == 65 else []), [0]

    def put(sym, last=False):
        out.append(sym)
        before = row.tot
        row._update(row.S.index(sym))
        halvings[0] += row.tot < before
        if order and not last and (order == 65 or sym):
            out.append(1 if order == 65 else 0)
    put(m - 1)
    put(p)
    while halvings[0] < 4:
        put(0)
    assert row.F[p - 1] == 2 and row.S[p - 1] == p and row.F[p] == 1 and row.S[p] == p - 1
    put(p - 1)
    while row.tot + M.STEP <= M.MAX_FREQ:
        put(0)
    assert halvings[0] == 4 and row.F[p - 1:p + 1] == [17, 2] and row.F[p + 3:p + 5] == [1, 1]
    put(p + 4 if twin else p)
    assert halvings[0] == 5 and (row.S[p + 3] == p + 4 if twin else row.F[p - 1:p + 1] == [9, 9] and row.S[p] == p)
    # what the step left is seen by what follows: the symbols of both pairs again, their cumulative frequencies being
    # those of the list order - a decoder that swapped differently decodes other bytes from here on
    for sym in (p - 1, p, p + 3, p + 4, 0, p, p - 1, p + 4, p + 3, 0, 0):
        put(sym)
    put(p, last=True)
    return bytes(out)


def run_tie_case(twin=False):
    """the same for the run-length model of one context: `A` in runs of 1 + r, a `B` between them, r the model's symbol"""
    row, out, halvings = M.Model(4), bytearray(), [0]

    def put(r, last=False):
        out.extend(b"A" * (r + 1) + (b"" if last else b"B"))
        before = row.tot
        row._update(row.S.index(r))
        halvings[0] += row.tot < before
    put(2)
    while halvings[0] < 4:
        put(0)
    put(1)
    while row.tot + M.STEP <= M.MAX_FREQ:
        put(0)
    assert halvings[0] == 4 and row.F[1:] == [17, 2, 1] and row.S[1:] == [1, 2, 3]
    put(3 if twin else 2)
    assert halvings[0] == 5 and (row.S[2] == 3 if twin else row.F[1:3] == [9, 9] and row.S[2] == 2)
    for r in (1, 2, 3, 0, 2, 1, 3, 0):                               # (the list order shows in what follows)
        put(r)
    put(2, last=True)
    return bytes(out)


TIE_PLACES = (3, 8, 64)      # inside a lane's four entries; across a lane boundary; across the boundary at 64


@functools.lru_cache(maxsize=None)
def tie_cases():
    """[(what, raw, order)]: every placement under order 0 and, in both order-1 homes (m = 76: LDS; m = 201: global
    memory), under orders 1 and 65, each with its twin; the run-length model's pair under orders 64 and 65"""
    out = []
    for p in TIE_PLACES:
        for m, order in ((76, 0), (76, 1), (76, 65), (201, 1), (201, 65)):
            for twin in (False, True):
                out.append(("%s p=%d m=%d" % ("twin" if twin else "tie", p, m), tie_case(p, m, order, twin), order))
    for order in (64, 65):
        for twin in (False, True):
            out.append(("run %s" % ("twin" if twin else "tie"), run_tie_case(twin), order))
    assert all(12000 <= len(r) < 48 * 1024 for _, r, _ in out)
    return out


@functools.lru_cache(maxsize=None)
def tie_streams():
    out = [M.compress(r, o) for _, r, o in tie_cases()]
    assert all(s[0] == o for s, (_, _, o) in zip(out, tie_cases()))
    return out


# ---- damaged streams whose rows live in global memory -----------------------------------------------------------------
GUARDS = ("freq_gt_max", "ran_off", "range_lt_tot", "starved")


@functools.lru_cache(maxsize=None)
def global_damaged(least=60, seed=11, most=400):
    """[(stream, cap)]: damaged variants of model-made order 1 / 65 / 193 streams with an alphabet above 84 and more
    than 1 KiB of payload, drawn until there are `least` of them and the accepted ones reach each guard of the step
    twice or more in the global home"""
    rng = random.Random(seed)
    high = tuple(range(150, 230, 3))
    bases = []
    for order, raw in ((1, skewed(high, 3400, 1)), (65, skewed(high, 4500, 2, runs=5)), (193, skewed(tuple(range(3, 160, 11)), 6000, 3, runs=9)),
                       (1, skewed(high[:9] + (255,), 6000, 4)), (65, skewed(high[:12], 6500, 5, runs=4))):
        s = M.compress(raw, order)
        home, size = payload(s)
        assert s[0] == order and home == "o1_global" and size > 1024, (order, home, size)
        bases.append((s, len(raw)))
    out, seen, ev = [], set(), collections.Counter()
    while len(out) < least or any(ev["o1_global", g] < 2 for g in GUARDS):
        assert len(out) < most
        s0, n0 = rng.choice(bases)
        s = _damage(rng, s0)
        if s in seen or s == s0:
            continue
        seen.add(s)
        cap = rng.choice((n0, n0, n0 + 5))
        M.uncompress_to(s, cap, events=ev)
        out.append((s, cap))
    return out


# ---- the coder's input window: payload sizes and alignments -----------------------------------------------------------
WINDOW_SIZES = tuple(range(1, 49)) + tuple(range(1000, 1061)) + tuple(range(2030, 2081))
_WINDOW_KINDS = (("o0", 0, tuple(range(40, 72)), 0), ("o1_lds", 1, tuple(range(30, 84, 2)), 0),
                 ("o1_global", 65, tuple(range(120, 250, 5)), 6))


def _window_stream(kind, n):
    """(raw, stream, payload bytes - 0 where the coder lost to a copy): the stream stores its size and is not packed, so
    the payload is what follows the flag byte and the size"""
    home, order, symbols, runs = _WINDOW_KINDS[kind]
    raw = skewed(symbols, n, 100 + kind, runs, chain=2)
    s = M.compress(raw, order)
    if s[0] != order:
        return raw, s, 0
    size = len(s) - 1 - len(M.var_put(n))
    m = s[len(s) - size] or 256
    assert home == ("o0" if not order & 1 else "o1_lds" if M.lds_home(m) else "o1_global")
    return raw, s, size


@functools.lru_cache(maxsize=None)
def window_bases():
    """[(home, raw, stream, payload bytes)]: one valid stream a home with more than 2,100 bytes of payload, the raw
    length walked up to it"""
    out = []
    for kind, (home, order, _, _) in enumerate(_WINDOW_KINDS):
        n = 2048
        while True:
            raw, s, size = _window_stream(kind, n)
            if size > 2100:
                break
            n += 128
        out.append((home, raw, s, size))
    return out


@functools.lru_cache(maxsize=None)
def window_truncations():
    """[(home, stream, cap, payload bytes)]: the bases cut to every payload size of WINDOW_SIZES, the capacity kept"""
    return [(home, s[:len(s) - size + k], len(raw), k) for home, raw, s, size in window_bases() for k in WINDOW_SIZES]


@functools.lru_cache(maxsize=None)
def window_residues():
    """[(home, raw, stream, payload bytes)]: valid streams with more than 1,040 bytes of payload, the raw length walked
    until the payload sizes of a home have taken all 16 values mod 16 (the first stream of each value is kept)"""
    out = []
    for kind, (home, whole, _, most) in enumerate(window_bases()):
        have, n = {}, len(whole) * 1000 // most                      # (a little before the payload passes 1,040 bytes)
        while len(have) < 16:
            n += 1
            assert n < len(whole)
            raw, s, size = _window_stream(kind, n)
            if size > 1040 and size % 16 not in have:
                have[size % 16] = (home, raw, s, size)
        out += [have[r] for r in range(16)]
    return out


def climber(m, n):
    """the highest symbol repeated: its entry bubbles from the last list position to the first, one swap a symbol"""
    return bytes([0, 1 % m, 2 % m]) + bytes([m - 1]) * n


def ties(n):
    """two symbols taking turns: their frequencies tie after every pair, and the swap is strict"""
    return bytes([5, 9] * (n // 2)) + bytes([12])


def with_alphabet(m, n, seed):
    """n bytes below m, m - 1 among them: six in seven from three symbols, so that the coders beat a plain copy"""
    rng = random.Random(seed)
    return bytes(rng.randrange(min(m, 3)) if rng.randrange(7) else rng.randrange(m) for _ in range(n - 1)) + bytes([m - 1])
