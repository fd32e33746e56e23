"""Inputs of the arith tests (test_arith_cpu.py, test_gpu_arith.py, test_gpu_arith_hostile.py): the reference-made
vectors of tests/golden/arith/edge.bin, constructed inputs coded by the Python model (arith_model.py, itself pinned by
those vectors and the 28 fixtures), and damaged variants of small streams.  Everything is seeded; nothing here needs a GPU."""
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
