"""The encoder's table stage at the branches that ordinary inputs do not reach.  The stage decides every byte of a stream's
header and every frequency the chain codes with, and it is written three times on the device in code that shares nothing:
wave_normalise_freq256 (order 0, four counters a lane), normalise_freq over the compact alphabet inside k_enc_tables
(order 1, one context row a lane) and the 4x8 normalisation of k8_enc_front - with compute_shift in doubles, two alphabet
writers, the zero-run row serialiser, the nested-table rule and the switch between LDS and global pair counters around them
(htscodecs_amd/csrc/r4x16_encode.hip).  Every edge vector of tests/golden/edge.json and 300 random inputs under all eight
plain orders send the oracle's normaliser through its retry 4 times in 64,128 calls and through its last resort never; the
inputs here are constructed to take each branch, and test_inputs_hold_what_they_claim proves from the oracle - its own
compute_shift figures (orc_compute_shift_stats), orc_normalise_freq and the table bytes of its stream - that each one does.
The path through the normaliser is traced by a restatement (_trace) whose frequencies must equal both.  No GPU is needed
for that part.  On the GPU every case is compressed alone and with all the others in one batch, with enc_direct at its
default and at 0, through the host batch and the device-resident call with guarded slots, and must give the oracle's bytes
on the route the tables stage has to choose; the oracle's stream of every case is decoded on the GPU as well.

What was searched for and not found (CPU, bounded, with the oracle):
  - The last resort at order 0.  At most 255 counters can be raised to 1, so the retry scales by 0.94 at least and leaves
    less excess than the largest counter holds: the one-lane tail of wave_normalise_freq256 is not reachable through the
    interface and no case here pretends to cover it.  Order 0 has the three retry endings and the three plain ones.
  - The last resort in a row of at most 50 successors (the alphabets whose pair counters stay in LDS): none among 411,519
    two- and three-level rows under the reference's target rule; after the retry the excess is below 3 there while the
    largest entry holds 20 and more.  The 50 / 51 boundary is covered by a retry row.  The last resort itself needs no
    clamped row: "o1-last-128" (44 successors once, 15 fourteen times: target 128) takes it at any table precision.
  - A table of 1,000 bytes and more whose order-0 coding is not shorter, or exactly as long (nlen + 6 == 1 + tlen).  A
    serialised table near 1,000 bytes holds about a thousand one-byte frequencies with a mean of 32 at most, some 6.4 bits
    each, so its order-0 stream stays below 0.93 of it; the closest of 96 chains of _markov (28 .. 31 values, two skews,
    60,000 and 150,000 bytes, six seeds) is 1,005 -> 914 bytes, 86 short of the tie; "nest-dense" (1,032 -> 926) is the
    one kept.  The comparison in k_enc_finish is exercised on its "shorter" side and by the 999 / 1,000 byte rule only.

The quotient e10 / e12 against 1.01 (RATIO_SPECS: a context with k successors once and one successor c times, searched
over k in {100, 150, 200, 246} and 80 values of c around the crossing): reached distances below 1.01: 3.8e-7, 4.1e-6,
1.7e-5; above: 1.9e-5, 2.3e-5, 2.9e-5.  A wrong tiny count, table index or clamp moves the quotient by 1e-3 and more and
flips these cases; a last-bit difference in rounding moves it by 1e-16 and cannot be caught by any input of this family.
The "cs-cycle" cases sit on the other branch of that arithmetic: one successor per row, both estimates negative (fast_log
gives 0.04 for 1), a quotient above 1.01 - and 10 bits all the same while max_tot <= 1024."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_enc_freq_table import _table, _varint
from test_oracle4x8 import Codec8


# ---- inputs ------------------------------------------------------------------------------------------------------------
# Every input is a small spec, expanded by one of three builders with numpy's legacy RandomState.

def _bag(groups, seed):
    """Order-0 material: `groups` is [(first value, number of values, count of each)]; the bytes in shuffled order."""
    parts = [np.repeat(np.arange(v0, v0 + k, dtype=np.int64), c) for v0, k, c in groups]
    a = np.concatenate(parts)
    assert a.max() <= 255
    a = a.astype(np.uint8)
    np.random.RandomState(seed).shuffle(a)
    return a


def _chains(chains, filler, gap, seed, last=None, pad=None):
    """Order-1 material: `chains` is [(bytes of one chain, how often)].  The chains go out in shuffled order, each behind
    `gap` (an int, or (low, high) drawn per chain) bytes drawn evenly from `filler`; a run of filler bytes also ends the
    block; `pad` = (filler value, count) adds a run of that one value behind it - enough of it and the container codes the
    block instead of storing it - and `last` (one byte value) may follow.  A byte value that occurs in chains only, never
    in `filler`, has a context row made of exactly what follows it in its chains - which is how the rows below are made."""
    rs = np.random.RandomState(seed)
    f = np.asarray(filler, dtype=np.uint8)
    items = [np.asarray(c, dtype=np.uint8) for c, k in chains for _ in range(k)]
    order = rs.permutation(len(items))
    lo, hi = (gap, gap) if isinstance(gap, int) else gap
    out = []
    for i in order:
        g = lo if lo == hi else int(rs.randint(lo, hi + 1))
        out.append(f[rs.randint(0, len(f), size=g)])
        out.append(items[i])
    out.append(f[rs.randint(0, len(f), size=max(lo, 1))])
    if pad is not None:
        out.append(np.full(pad[1], pad[0], dtype=np.uint8))
    if last is not None:
        out.append(np.array([last], dtype=np.uint8))
    return np.concatenate(out)


def _fan(hub, groups):
    """Chains (hub, successor) for `groups` = [(first successor, number of successors, count of each)]."""
    return [((hub, s), c) for v0, k, c in groups for s in range(v0, v0 + k)]


# ---- what the oracle does with an input --------------------------------------------------------------------------------

def _trace(F, size, tot):
    """The path of a counter set through normalise_freq (rANS_static4x16pr.c:116-163; oracle/rans4x16_oracle.c
    orc_normalise_freq): (frequencies, path).  The path is "exact", "add" or "sub" for the one-pass endings,
    "retry-exact", "retry-add", "retry-sub" after the second scaling, and "last-resort:k" where the excess is taken from
    the entries >= 2 in symbol order (k of them emptied to 1, the largest one included).  A restatement: the claims test
    checks its frequencies against orc_normalise_freq and against the table bytes of the oracle's stream."""
    F = [int(x) for x in F]
    retried = ""
    while True:
        scale = ((tot << 31) // size + (1 << 30) // size) & 0xffffffffffffffff
        best, arg, total = 0, 0, 0
        for j, f in enumerate(F):
            if not f:
                continue
            if best < f:
                best, arg = f, j
            F[j] = max(1, (f * scale) >> 31)
            total += F[j]
        adjust = tot - total
        if adjust > 0:
            F[arg] += adjust
            return F, retried + "add"
        if adjust == 0:
            return F, retried + "exact"
        need = -adjust
        if F[arg] > need and (retried or F[arg] // 2 >= need):
            F[arg] -= need
            return F, retried + "sub"
        if not retried:
            retried, size = "retry-", total
            continue
        adjust += F[arg] - 1
        F[arg] = 1
        emptied = 1
        for j in range(len(F)):
            if not adjust:
                break
            if F[j] < 2:
                continue
            take = adjust if F[j] > -adjust else 1 - F[j]
            F[j] += take
            adjust -= take
            emptied += F[j] == 1
        return F, "last-resort:%d" % emptied


def _orc_normalise(lib, F, size, tot):
    arr = (C.c_uint32 * 256)(*[int(x) for x in F])
    lib.orc_normalise_freq.restype = C.c_int
    lib.orc_normalise_freq.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_uint32]
    assert lib.orc_normalise_freq(arr, int(size), int(tot)) == 0
    return list(arr)


class _ShiftStats(C.Structure):
    """orc_shift_stats (oracle/rans4x16_oracle.h)."""
    _fields_ = [("e10", C.c_double), ("e12", C.c_double), ("ratio", C.c_double),
                ("max_tot", C.c_int), ("clamped10", C.c_int), ("clamped12", C.c_int),
                ("present", C.c_int * 256), ("tiny10", C.c_int * 256), ("tiny12", C.c_int * 256), ("target0", C.c_int * 256)]


def _pow2_ceil(v):
    return 1 << max(int(v) - 1, 0).bit_length() if v else 0


def _pair_counts(a):
    """hist1_4 (utils.h:136-202) and the quarter starts (rANS_static4x16pr.c:720-723): F[previous][byte], the first byte
    and the first bytes of the quarters 1..3 in context 0."""
    a = np.asarray(a, dtype=np.int64)
    prev = np.concatenate([[0], a[:-1]])
    F = np.bincount(prev * 256 + a, minlength=65536).reshape(256, 256)
    q = len(a) >> 2
    for k in (1, 2, 3):
        F[0, a[k * q]] += 1
    return F


class _O1:
    """What the oracle makes of an order-1 block: its own compute_shift on the block's pair counters (orc_compute_shift_stats:
    bits, e10 / e12, max_tot, per-row targets and tiny counts), the path of every row through the normaliser, and the table
    as the stream carries it."""

    def __init__(self, oracle, a):
        lib = oracle.lib
        self.F = _pair_counts(a)
        self.T = self.F.sum(axis=1)
        F0 = np.zeros(256, dtype=np.uint32)
        F0[np.unique(a)] = 1
        F0[0] = 1
        self.alpha = [int(j) for j in np.nonzero(F0)[0]]
        Fc = np.ascontiguousarray(self.F, dtype=np.uint32)
        Tc = np.ascontiguousarray(self.T, dtype=np.uint32)
        S = (C.c_int * 256)()
        self.st = _ShiftStats()
        lib.orc_compute_shift_stats.restype = C.c_int
        lib.orc_compute_shift_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.bits = lib.orc_compute_shift_stats(F0.ctypes.data, Fc.ctypes.data, Tc.ctypes.data, C.addressof(S), C.addressof(self.st))
        self.S = list(S)                                                # unclamped: rows above 1,024 in a 10-bit block show here
        self.ratio, self.max_tot = self.st.ratio, self.st.max_tot
        # the bare order-1 stream (no container in front: also there where the container would store the block raw)
        n = len(a)
        src = np.ascontiguousarray(a, dtype=np.uint8)
        cap = oracle.bound(n, 1)
        out = np.zeros(cap, dtype=np.uint8)
        olen = C.c_uint32(0)
        lib.orc_o1_encode.restype = C.c_int
        lib.orc_o1_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        assert lib.orc_o1_encode(src.ctypes.data, n, out.ctypes.data, cap, C.byref(olen)) == 0
        s = out[:olen.value].tobytes()
        assert s[0] >> 4 == self.bits
        self.nested = s[0] & 1
        if self.nested:
            self.tlen, i = _varint(s, 1)
            self.nlen, i = _varint(s, i)
            tab = np.zeros(self.tlen + 16, dtype=np.uint8)
            nst = np.frombuffer(s[i:i + self.nlen], dtype=np.uint8).copy()
            lib.orc_o0_decode.restype = C.c_int
            lib.orc_o0_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
            assert lib.orc_o0_decode(nst.ctypes.data, self.nlen, tab.ctypes.data, self.tlen) == 0
            self.table = tab[:self.tlen].tobytes()
        else:
            # the table has no length field: _table walks it, and where it ends is found below by serialising the rows
            # again from what it returned
            self.table, self.nlen = None, None
        # _table reads a container without transforms whose table travels as it is: that is what it gets
        plain = bytes([1]) + _put_varint(n) + bytes([self.bits << 4]) + (self.table if self.nested else s[1:])
        bits, self.rows = _table(plain)
        assert bits == self.bits
        if not self.nested:
            self.table = _serialise(self.alpha, self.rows, self.S, self.bits)
            assert s[1:1 + len(self.table)] == self.table, "the table read back and written again is the stream's"
            self.tlen = len(self.table)
        self.paths = {}

    def target(self, r):
        return min(self.S[r], 1024) if self.bits == 10 else self.S[r]

    def path(self, oracle, r):
        """The normaliser's path of context row r; its frequencies checked against orc_normalise_freq and the stream."""
        if r not in self.paths:
            tgt = self.target(r)
            got, p = _trace(self.F[r], int(self.T[r]), tgt)
            assert got == _orc_normalise(oracle.lib, self.F[r], int(self.T[r]), tgt), (r, p)
            sh = self.bits - (tgt.bit_length() - 1)
            assert {j: f << sh for j, f in enumerate(got) if f} == self.rows[r], (r, p)
            self.paths[r] = p
        return self.paths[r]

    def stored(self, r):
        """Row r as the table holds it (before the shift up to the coder's total)."""
        sh = self.bits - (self.target(r).bit_length() - 1)
        return {j: f >> sh for j, f in self.rows[r].items()}


def _put_varint(v):
    out = [v & 0x7f]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7f))
        v >>= 7
    return bytes(reversed(out))


def _put_alphabet(alpha):
    """The alphabet's bytes (rANS_static4x16pr.c:182-206) - to tell where a table that was read back ends."""
    have, out, skip = set(alpha), [], 0
    for j in sorted(alpha):
        if skip:
            skip -= 1
            continue
        out.append(j)
        if j and j - 1 in have:
            k = j + 1
            while k < 256 and k in have:
                k += 1
            skip = k - (j + 1)
            out.append(skip)
    return bytes(out + [0])


def _serialise(alpha, rows, S, bits):
    """The table bytes of rows as _table returned them (shifted up): alphabet, then per context the row with its zero runs."""
    out = [_put_alphabet(alpha)]
    for r in alpha:
        row = rows.get(r, {})
        tot = sum(row.values())
        sh = 0
        if tot:
            tgt = min(S[r], 1 << bits)
            sh = bits - (tgt.bit_length() - 1)
        zeros = 0
        for j in alpha:
            f = row.get(j, 0) >> sh
            if f:
                if zeros:
                    out.append(bytes([0, zeros - 1]))
                    zeros = 0
                out.append(_put_varint(f))
            else:
                zeros += 1
        if zeros:
            out.append(bytes([0, zeros - 1]))
    return b"".join(out)


def _o0(oracle, a):
    """What the oracle makes of an order-0 block: (path of the first normalisation, counters, stored frequencies by byte
    value, alphabet bytes) - the frequencies of the restatement checked against orc_normalise_freq and the stream's table."""
    a = np.asarray(a, dtype=np.uint8)
    n = len(a)
    F = np.bincount(a, minlength=256)
    tgt = min(_pow2_ceil(n), 4096)
    got, p = _trace(F, n, tgt)
    assert got == _orc_normalise(oracle.lib, F, n, tgt)
    up, p2 = _trace(got, tgt, 4096)
    assert p2 == "exact" and up == [f * (4096 // tgt) for f in got], "the second normalisation is a shift"
    lib = oracle.lib
    cap = oracle.bound(n, 0)
    out = np.zeros(cap, dtype=np.uint8)
    olen = C.c_uint32(0)
    lib.orc_o0_encode.restype = C.c_int
    lib.orc_o0_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    assert lib.orc_o0_encode(a.ctypes.data, n, out.ctypes.data, cap, C.byref(olen)) == 0
    s = out[:olen.value].tobytes()
    alpha = [j for j in range(256) if F[j]]
    ab = _put_alphabet(alpha)
    assert s[:len(ab)] == ab
    i, stored = len(ab), {}
    for j in alpha:
        stored[j], i = _varint(s, i)
    assert stored == {j: f for j, f in enumerate(got) if f}, p
    return p, F, stored, ab


# ---- rANS 4x8: its two normalisers (oracle/rans4x8_oracle.c:103-121, :229-247) ---------------------------------------------

def _trace8(F, order1):
    """(frequencies, number of fixed-factor retries) of the 4x8 normalisation (to a sum of 4,095, against 4,096): order 0
    in fixed point with the retry factor 2104533975 / 2^31 where the excess is more than half the largest entry, order 1
    in doubles with 0.98 where it is half of it or more.  A restatement, checked against the oracle's table bytes by the claims test."""
    F = [int(x) for x in F]
    n = sum(F)
    tr = ((4096 << 31) // n + (1 << 30) // n) if not order1 else 4096.0 / n
    retries = 0
    while True:
        m, M, fsum = 0, 0, 0
        for j, f in enumerate(F):
            if not f:
                continue
            if m < f:
                m, M = f, j
            F[j] = max(1, int(f * tr) if order1 else (f * tr) >> 31)
            fsum += F[j]
        fsum += 1
        if fsum < 4096:
            F[M] += 4096 - fsum
            return F, retries
        over = fsum - 4096
        if (over >= F[M] // 2) if order1 else (over > F[M] // 2):
            tr = 0.98 if order1 else 2104533975
            retries += 1
            continue
        F[M] -= over
        return F, retries


def _get_table8(s, i):
    """One 4x8 frequency table at s[i:] (oracle/rans4x8_oracle.c put_table): ({byte: frequency}, next position)."""
    F, rle, j = {}, 0, s[i]
    i += 1
    while True:
        f = s[i]
        i += 1
        if f >= 128:
            f = ((f & 127) << 8) | s[i]
            i += 1
        F[j] = f
        if not rle and j + 1 == s[i]:
            j, rle = s[i], s[i + 1]
            i += 2
        elif rle:
            rle -= 1
            j += 1
        else:
            j = s[i]
            i += 1
        if j == 0:
            return F, i


def _tables8(comp):
    """{context: {byte: frequency}} of a 4x8 stream (order 0: the one table under context None)."""
    if comp[0] == 0:
        return {None: _get_table8(comp, 9)[0]}
    rows, rle, i, r = {}, 0, 10, comp[9]
    while True:
        rows[r], i = _get_table8(comp, i)
        if not rle and r + 1 == comp[i]:
            r, rle = comp[i], comp[i + 1]
            i += 2
        elif rle:
            rle -= 1
            r += 1
        else:
            r = comp[i]
            i += 1
        if r == 0:
            return rows


def _markov(ns, lo, n, seed, power):
    """n bytes of a first-order chain over the values lo .. lo + ns - 1 whose rows are drawn at random and skewed
    (uniform variates to `power`): a table of many different frequencies, which an order-0 coder shortens little."""
    rs = np.random.RandomState(seed)
    P = rs.random_sample((ns, ns)) ** power + 1e-4
    cdf = np.cumsum(P / P.sum(axis=1, keepdims=True), axis=1)
    u = rs.random_sample(n)
    out = np.empty(n, dtype=np.int64)
    cur = 0
    for i in range(n):
        cur = min(int(np.searchsorted(cdf[cur], u[i])), ns - 1)
        out[i] = cur
    return (out + lo).astype(np.uint8)


def _bagv(pairs, seed):
    """Order-0 material from [(byte value, count)]."""
    a = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in pairs])
    np.random.RandomState(seed).shuffle(a)
    return a


# ---- the cases -----------------------------------------------------------------------------------------------------------
# name -> (codec, order, bytes).  HUB rows: {name: {context byte: what the claims test demands of that row}}.

FILL_HI = [251, 252, 253, 254]                  # filler above a hub at 250 and its successors 1 .. 249
FILL_LO = [3, 4, 5, 6]                          # filler below successors 9 .. 255, hub 2
ALPHA_A = [0, 1, 2, 10, 12, 13, 14, 40, 41, 60, 62, 250, 251, 252, 253, 254, 255]
ALPHA_A_BYTES = bytes([0, 1, 1, 10, 12, 13, 1, 40, 41, 0, 60, 62, 250, 251, 4, 0])
ALPHA_B = [1, 2, 3, 9, 11, 12, 200, 254, 255]       # no byte 0 in the data: order 1 lists it by rule, and 1 then starts a run
ALPHA_B_BYTES_O0 = bytes([1, 2, 1, 9, 11, 12, 0, 200, 254, 255, 0, 0])
ALPHA_B_BYTES_O1 = bytes([0, 1, 2, 9, 11, 12, 0, 200, 254, 255, 0, 0])
RATIO_SPECS = {                                  # name -> (singles k, count c of the one frequent successor): see the docstring
    "ratio-below-1": (200, 9331), "ratio-below-2": (150, 9581), "ratio-below-3": (150, 9567),
    "ratio-above-1": (246, 9336), "ratio-above-2": (150, 9591), "ratio-above-3": (150, 9557),
}
RATIO_DISTANCE = {"ratio-below-1": 3.8e-7, "ratio-below-2": 4.1e-6, "ratio-below-3": 1.7e-5,
                  "ratio-above-1": 1.9e-5, "ratio-above-2": 2.3e-5, "ratio-above-3": 2.9e-5}


def _cases():
    c = {}
    o0 = lambda name, a: c.__setitem__(name, ("16", 0, a))
    o1 = lambda name, a: c.__setitem__(name, ("16", 1, a))
    # 1. order 0: the normaliser's endings
    o0("o0-retry-add", _bag([(10, 120, 1), (130, 111, 44)], 1))
    o0("o0-retry-exact", _bag([(10, 140, 1), (150, 46, 131)], 2))
    o0("o0-retry-sub", _bag([(10, 170, 1), (180, 51, 113)], 3))
    o0("o0-add", _bag([(33, 40, 37), (100, 3, 500)], 4))
    o0("o0-sub", _bag([(5, 244, 1), (250, 1, 3861)], 5))
    o0("o0-n512", _bag([(48, 8, 64)], 6))
    o0("o0-n513", _bag([(48, 8, 64), (60, 1, 1)], 7))
    o0("o0-n2048", _bag([(48, 4, 500), (60, 3, 16)], 8))
    o0("o0-n2049", _bag([(48, 4, 500), (60, 3, 16), (70, 1, 1)], 9))
    o0("o0-n4096", _bagv([(20, 127), (21, 128), (40, 3000), (41, 841)], 10))
    o0("o0-n4097", _bagv([(20, 127), (21, 128), (40, 3000), (41, 841), (99, 1)], 11))
    o0("o0-all256", _bag([(0, 256, 1), (65, 1, 3000), (66, 4, 200)], 12))
    for name, lo, hi in (("lanes", 70, 200), ("slots", 41, 43), ("far", 3, 252)):
        o0("o0-tie-" + name, _bagv([(lo, 1000), (hi, 1000), (33, 300), (34, 200), (35, 123)], 13))
    # 2. order 1: rows that retry, rows that end in the last resort
    o1("o1-retry", _chains(_fan(250, [(1, 198, 1), (199, 44, 20)]), FILL_HI, 1, 20))
    o1("o1-last-low", _chains(_fan(250, [(1, 168, 1), (169, 79, 27)]), FILL_HI, 1, 21))
    o1("o1-last-high", _chains(_fan(2, [(9, 168, 1), (177, 79, 27)]), FILL_LO, 1, 22))
    o1("o1-last-multi", _chains(_fan(255, [(1, 2, 7), (3, 174, 1), (177, 78, 26)]), [0], 1, 23))
    o1("o1-last-128", _chains(_fan(250, [(1, 44, 1), (45, 15, 14)]), FILL_HI, 1, 24))
    o1("o1-retry-ns50", _chains(_fan(100, [(1, 34, 1), (35, 14, 8)]), [0], 1, 25))
    o1("o1-retry-ns51", _chains(_fan(100, [(1, 34, 1), (35, 14, 8)]), [0, 101], 1, 26))
    # 3. compute_shift
    o1("cs-nz63", _chains(_fan(250, [(1, 62, 3), (63, 1, 14)]), FILL_HI, 1, 30, pad=(251, 1000)))
    o1("cs-nz64", _chains(_fan(250, [(1, 63, 3), (64, 1, 11)]), FILL_HI, 1, 31, pad=(251, 1000)))
    for T, per in ((128, 2), (1024, 16), (4096, 64), (8192, 128)):
        pad = (251, 1000) if T == 128 else None
        o1("cs-T%d" % T, _chains(_fan(250, [(1, 64, per)]), FILL_HI, 1, 32, pad=pad))
        o1("cs-T%d" % (T + 1), _chains(_fan(250, [(1, 63, per), (64, 1, per + 1)]), FILL_HI, 1, 33, pad=pad))
    # eight values in a fixed cycle: every row holds one successor, and fast_log's offset (it gives 0.04 for 1) makes both
    # estimates negative and their quotient larger than 1.01 - 10 bits all the same while no row's target exceeds 1,024
    for rep in (600, 3000, 5000):
        o1("cs-cycle-%d" % rep, np.tile(np.arange(65, 73, dtype=np.uint8), rep))
    o1("cs-10bit-2048-4096", _chains(_fan(250, [(1, 64, 40)]) + _fan(249, [(1, 64, 80)]), FILL_HI, 1, 35))
    o1("cs-12bit", _chains(_fan(250, [(1, 100, 1), (249, 1, 20000)]), FILL_HI, 1, 36))
    for k in (63, 64, 65):
        o1("cs-tiny%d" % k, _chains(_fan(250, [(1, k, 1), (249, 1, 5000)]), FILL_HI, 1, 37))
    # every byte value follows 128 once - itself included - but 7, which follows it 5,000 times; 0 or 255 behind a successor
    o1("cs-tiny255", _chains([((128, s), 1) for s in range(256) if s not in (128, 7)] + [((128, 128, 7), 1), ((128, 7), 4999)],
                             [0, 255], 1, 38))
    for name, (k, cnt) in RATIO_SPECS.items():
        o1(name, _chains(_fan(250, [(1, k, 1), (249, 1, cnt)]), FILL_HI, 1, 7))
    # 4. serialisation
    wa = [(v, 40 + 37 * i) for i, v in enumerate(ALPHA_A)]
    wb = [(v, 40 + 37 * i) for i, v in enumerate(ALPHA_B)]
    o0("ser-alpha-a-o0", _bagv(wa, 40))
    o1("ser-alpha-a-o1", _bagv(wa, 41))
    o0("ser-alpha-b-o0", _bagv(wb, 42))
    o1("ser-alpha-b-o1", _bagv(wb, 43))
    # rows over 24 values: 60 -> first and last value only (an inner zero run), 61 -> the lowest three (a trailing one),
    # 62 -> one value (a single successor); 99 is the block's last byte and nothing else (its row is all zero)
    o1("ser-rows", _chains([((60, 40), 30), ((60, 99 - 1), 50), ((61, 40), 9), ((61, 41), 20), ((61, 42), 31), ((62, 50), 64)],
                           list(range(40, 58)), 2, 44, last=99))
    o1("ser-127-128", _chains(_fan(250, [(1, 1, 127), (2, 1, 128), (3, 63, 12), (66, 1, 13)]), FILL_HI, 1, 45))
    # 5. the table in the stream: as it is at 999 bytes, as an order-0 stream from 1,000 on where that is shorter
    run = np.full(1500, 33, dtype=np.uint8)                          # (so that the container codes the block)
    o1("nest-999", np.concatenate([(np.random.RandomState(1).randint(0, 32, size=540) + 33).astype(np.uint8), run]))
    o1("nest-1000", np.concatenate([(np.random.RandomState(3).randint(0, 32, size=566) + 33).astype(np.uint8), run]))
    o1("nest-dense", _markov(30, 40, 60000, 2, 2))
    # 6. rANS 4x8: the fixed-factor retry once and twice, both orders
    c["x8-o0-retry1"] = ("8", 0, _bag([(1, 156, 1), (157, 99, 47)], 60))
    c["x8-o0-retry2"] = ("8", 0, _bag([(1, 156, 1), (157, 99, 173)], 61))
    c["x8-o1-retry1"] = ("8", 1, _chains(_fan(250, [(1, 105, 1), (106, 143, 32)]), FILL_HI, 1, 62))
    c["x8-o1-retry2"] = ("8", 1, _chains(_fan(250, [(1, 150, 1), (151, 81, 164)]), FILL_HI, 1, 63))
    return c


CASES = _cases()
O0_NAMES = [n for n, c in CASES.items() if c[0] == "16" and c[1] == 0]
O1_NAMES = [n for n, c in CASES.items() if c[0] == "16" and c[1] == 1]
X8_NAMES = [n for n, c in CASES.items() if c[0] == "8"]

# The ending of the first normalisation of every order-0 case, and of the rows that order-1 cases are named after.
O0_PATHS = {"o0-retry-add": "retry-add", "o0-retry-exact": "retry-exact", "o0-retry-sub": "retry-sub", "o0-add": "add",
            "o0-sub": "sub", "o0-n512": "exact", "o0-n513": "add", "o0-n2048": "exact", "o0-n2049": "add", "o0-n4096": "exact",
            "o0-n4097": "add", "o0-all256": "add", "o0-tie-lanes": "add", "o0-tie-slots": "add", "o0-tie-far": "add",
            "ser-alpha-a-o0": "add", "ser-alpha-b-o0": "add"}
O1_PATHS = {"o1-retry": (250, "retry-add"), "o1-last-low": (250, "last-resort:1"), "o1-last-high": (2, "last-resort:1"),
            "o1-last-multi": (255, "last-resort:3"), "o1-last-128": (250, "last-resort:1"),
            "o1-retry-ns50": (100, "retry-add"), "o1-retry-ns51": (100, "retry-add")}
# compute_shift: name -> (context, total, target before the halving rules, target, symbols in the row)
CS_ROWS = {"cs-nz63": (250, 200, 256, 128, 63), "cs-nz64": (250, 200, 256, 256, 64),
           "cs-T128": (250, 128, 128, 128, 64), "cs-T129": (250, 129, 256, 256, 64),
           "cs-T1024": (250, 1024, 1024, 1024, 64), "cs-T1025": (250, 1025, 2048, 1024, 64),
           "cs-T4096": (250, 4096, 4096, 2048, 64), "cs-T4097": (250, 4097, 8192, 4096, 64),
           "cs-T8192": (250, 8192, 8192, 4096, 64), "cs-T8193": (250, 8193, 16384, 4096, 64)}
X8_RETRIES = {"x8-o0-retry1": 1, "x8-o0-retry2": 2, "x8-o1-retry1": 1, "x8-o1-retry2": 2}

_VIEWS = {}


def _view(oracle, name):
    """The oracle's reading of a 4x16 case, made once and shared by the tests."""
    if name not in _VIEWS:
        _, order, a = CASES[name]
        _VIEWS[name] = _O1(oracle, a) if order else _o0(oracle, a)
    return _VIEWS[name]


_WANT = {}


def _want(oracle, orc8, name):
    """The oracle's stream of a case, made once."""
    if name not in _WANT:
        codec, order, a = CASES[name]
        _WANT[name] = orc8.compress(a.tobytes(), order) if codec == "8" else oracle.compress(a.tobytes(), order)
    return _WANT[name]


@pytest.fixture(scope="module")
def orc8():
    import cpu_libs
    return Codec8(cpu_libs.oracle().lib, "orc8_")


# ---- the claims, from the oracle alone (no GPU) ------------------------------------------------------------------------------

def test_catalogue_is_small():
    assert max(len(c[2]) for c in CASES.values()) <= 150000
    assert sum(len(c[2]) for c in CASES.values()) <= 1500000


@pytest.mark.parametrize("name", O0_NAMES + O1_NAMES)
def test_inputs_hold_what_they_claim(oracle, orc8, name):
    """Every 4x16 case round-trips through the oracle, goes out coded (not stored: the table is in the stream that the GPU
    has to reproduce) at the order it asks for, and takes the branch it is named after."""
    _, order, a = CASES[name]
    raw = a.tobytes()
    comp = _want(oracle, orc8, name)
    assert oracle.uncompress(comp, len(raw)) == raw
    assert comp[0] == order, "coded at its order, no fall-back to a raw copy"
    v = _view(oracle, name)
    if order == 0:
        path, F, stored, ab = v
        assert path == O0_PATHS[name], (name, path)
        n = len(a)
        if name.startswith("o0-n"):
            want_n = int(name[4:])
            assert n == want_n and sum(stored.values()) == min(_pow2_ceil(n), 4096)
            assert (n & (n - 1) == 0) == (path == "exact")
        if name == "o0-n4096":
            assert stored[20] == 127 and stored[21] == 128, "a one-byte and a two-byte frequency side by side"
        if name == "o0-all256":
            assert len(stored) == 256
        if name.startswith("o0-tie-"):
            lo, hi = {"lanes": (70, 200), "slots": (41, 43), "far": (3, 252)}[name[7:]]
            assert F[lo] == F[hi] == F.max() and stored[lo] > stored[hi], "the lower of two equal maxima takes the adjustment"
            assert (lo // 4 == hi // 4) == (name == "o0-tie-slots"), "four counters a lane"
        if name == "ser-alpha-a-o0":
            assert ab == ALPHA_A_BYTES
        if name == "ser-alpha-b-o0":
            assert ab == ALPHA_B_BYTES_O0
        return
    # order 1
    assert v.table[:len(_put_alphabet(v.alpha))] == _put_alphabet(v.alpha)
    for r in v.alpha:                                                    # every row: restatement == oracle == stream
        if v.T[r]:
            v.path(oracle, r)
    if name in O1_PATHS:
        r, path = O1_PATHS[name]
        assert v.path(oracle, r) == path and v.bits == 10, (name, v.path(oracle, r), v.bits)
        assert sum(v.stored(r).values()) == v.target(r)
    if name in ("o1-last-low", "o1-last-high", "o1-last-multi"):
        r = O1_PATHS[name][0]
        assert v.S[r] == 2048 and v.target(r) == 1024, "a row clamped to the 10-bit total"
        assert v.st.tiny10[r] >= 64 and v.st.tiny12[r] == 0, "log(1024 + k) from the table in memory, log(4096 + 0) from a lane"
        succ = sorted(v.stored(r))
        assert (succ[-1] < r) if name != "o1-last-high" else (succ[0] > r)
    if name == "o1-last-multi":
        assert [v.stored(255)[j] for j in (1, 2, 177)] == [1, 1, 1], "two entries ahead of the largest emptied as well"
    if name == "o1-last-128":
        assert v.S[250] == 128, "a last resort no clamp is needed for"
    if name.startswith("o1-retry-ns"):
        assert len(v.alpha) == int(name[11:])
    if name in CS_ROWS:
        r, T, t0, tgt, nz = CS_ROWS[name]
        assert (int(v.T[r]), v.st.target0[r], v.S[r], v.st.present[r]) == (T, t0, tgt, nz), name
    if name.startswith("cs-cycle-"):
        want = {"cs-cycle-600": (512, 10), "cs-cycle-3000": (1024, 10), "cs-cycle-5000": (2048, 12)}[name]
        assert v.st.e10 < 0 and v.st.e12 < 0 and v.ratio >= 1.01 and (v.max_tot, v.bits) == want, (v.ratio, v.max_tot, v.bits)
    if name == "cs-10bit-2048-4096":
        assert v.bits == 10 and v.S[250] == 2048 and v.S[249] == 4096 and v.target(250) == v.target(249) == 1024
    if name == "cs-12bit":
        assert v.bits == 12 and v.ratio > 1.02 and v.max_tot == 4096
    if name.startswith("cs-tiny"):
        k = int(name[7:])
        r = 128 if k == 255 else 250
        assert v.st.tiny10[r] == k and v.st.tiny12[r] == k, (v.st.tiny10[r], v.st.tiny12[r])
        assert v.st.clamped10 >= k and v.st.clamped12 >= k, "1024 f / T and 4096 f / T truncate to 0 for the rare successors"
        if k == 255:
            assert v.st.present[r] == 256 and len(v.alpha) == 256
            rows = [v.stored(s) for s in v.alpha if v.T[s]]
            assert any(list(x) == [255] for x in rows) and any(list(x) == [0] for x in rows), "zero runs of 255, ahead and behind"
            assert bytes([0, 254]) in v.table
    if name in RATIO_SPECS:
        above = "above" in name
        assert v.max_tot > 1024 and v.bits == (12 if above else 10)
        d = v.ratio - 1.01
        assert (d >= 0) == above and abs(d) <= RATIO_DISTANCE[name], (name, d)
    if name == "ser-alpha-a-o1":
        assert v.table[:len(ALPHA_A_BYTES)] == ALPHA_A_BYTES
    if name == "ser-alpha-b-o1":
        assert 0 not in a and v.table[:len(ALPHA_B_BYTES_O1)] == ALPHA_B_BYTES_O1
    if name == "ser-rows":
        assert sorted(v.stored(60)) == [40, 98] and v.alpha.index(98) - v.alpha.index(40) > 2, "an inner zero run"
        assert sorted(v.stored(61)) == [40, 41, 42] and v.alpha[1] == 40, "a trailing zero run"
        assert list(v.stored(62)) == [50], "a single successor"
        assert a[-1] == 99 and v.T[99] == 0 and 99 not in v.rows, "a row that is all zero"
        assert bytes([0, len(v.alpha) - 1]) in v.table
    if name == "ser-127-128":
        assert v.stored(250)[1] == 127 and v.stored(250)[2] == 128
    if name == "nest-999":
        assert v.tlen == 999 and not v.nested
    if name == "nest-1000":
        assert v.tlen == 1000 and v.nested and v.nlen + 6 < 1 + v.tlen
    if name == "nest-dense":
        assert v.nested and v.nlen > 0.89 * v.tlen, (v.tlen, v.nlen)


@pytest.mark.parametrize("name", X8_NAMES)
def test_4x8_inputs_hold_what_they_claim(oracle, orc8, name):
    """rANS 4x8: the block (order 0) or the row of context 250 (order 1) takes the fixed-factor retry as often as the case
    says, by a restatement whose frequencies are those of the oracle's stream."""
    _, order, a = CASES[name]
    comp = _want(oracle, orc8, name)
    assert orc8.uncompress(comp) == a.tobytes() and comp[0] == order
    tabs = _tables8(comp)
    if order == 0:
        got, retries = _trace8(np.bincount(a, minlength=256), 0)
        assert {j: f for j, f in enumerate(got) if f} == tabs[None]
    else:
        F = _pair_counts(a)
        for r in tabs:
            got, k = _trace8(F[r], 1)
            assert {j: f for j, f in enumerate(got) if f} == tabs[r], r
            if r == 250:
                retries = k
    assert retries == X8_RETRIES[name]


# ---- on the GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def _expected_route(oracle, names, direct):
    """The encode read-out of one small batch (fewer blocks than CUs: with enc_direct on, the budget admits the largest
    record class), by the rules of k_enc_tables: an order-0 stream takes symbol records from 1,088 bytes on, an order-1
    stream where its records (256 + 16 ns^2 bytes) fit the image area and the block has a byte for every four of them;
    otherwise a 10-bit table of 20 .. 64 symbols takes packed rows - with the short index below byte 128 - and everything
    else the u16 rows.  A table of 1,000 bytes and more adds an order-0 stream of its own (u16 rows), chosen or not."""
    want = {"u16": 0, "packed": 0, "records": 0, "packed_freq": 0}
    for name in names:
        _, order, a = CASES[name]
        if order == 0:
            want["records" if direct and len(a) >= 1088 else "u16"] += 1
            continue
        v = _view(oracle, name)
        ns = len(v.alpha)
        img = 256 + 16 * ns * ns
        if direct and img <= 132096 and len(a) >= img // 4:
            want["records"] += 1
        elif v.bits == 10 and 20 <= ns <= 64:
            want["packed"] += 1
            want["packed_freq"] += int(a.max()) < 128
        else:
            want["u16"] += 1
        want["u16"] += 1 + v.tlen > 1000
    return want


def _run16(H, oracle, orc8, opts, names, direct):
    """The 4x16 cases `names` as ONE single-pass host batch: the oracle's bytes out of the encoder, the raw input out of the
    decoder fed with the oracle's streams, and the route read-out of the encode chain as the tables stage must have set it."""
    from htscodecs_amd import codec
    opts.set("route_count", 1)
    opts.set("host_pipe_mb", 0)
    if not direct:
        opts.set("enc_direct", 0)
    raws = [CASES[n][2].tobytes() for n in names]
    want = [_want(oracle, orc8, n) for n in names]
    codec.route_read("encode")
    enc, st = H.compress_batch(raws, [CASES[n][1] for n in names])
    assert all(s == 0 for s in st), st
    route = codec.route_read("encode")
    bad = [n for n, e, w in zip(names, enc, want) if e != w]
    assert not bad, bad
    dec, st = H.uncompress_batch(want, [len(r) for r in raws])
    assert all(s == 0 for s in st), st
    assert dec == raws
    assert route == _expected_route(oracle, names, direct), (route, _expected_route(oracle, names, direct))


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["default", "rows"])
@pytest.mark.parametrize("name", O0_NAMES + O1_NAMES)
def test_each_case_alone(H, oracle, orc8, opts, name, direct):
    """enc_direct at its default (symbol records where they fit) and at 0 (cumulative and packed rows): both images are
    built from the frequencies of the same tables stage."""
    _run16(H, oracle, orc8, opts, [name], direct)


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["default", "rows"])
def test_all_cases_in_one_batch(H, oracle, orc8, opts, direct):
    """Neighbours share nothing: every case next to all the others, orders 0 and 1, LDS and global pair counters, 10 and
    12 bits interleaved."""
    names = sorted(O0_NAMES + O1_NAMES, key=lambda n: n[::-1])
    _run16(H, oracle, orc8, opts, names, direct)


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0], ids=["default", "rows"])
def test_device_resident_inside_guarded_slots(H, oracle, orc8, opts, direct):
    """rans4x16_hip_compress_dev_sized under per-block orders and rans4x16_hip_uncompress_dev_sized, slots of exactly the
    bound a few bytes apart in an arena filled with a pattern (test_gpu_confinement): the oracle's bytes in the slots, the
    pattern everywhere else."""
    import torch
    from test_gpu_confinement import _Guarded, _expect, _what, caps_of
    opts.set("enc_direct", 1 if direct else 0)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    names = O1_NAMES + O0_NAMES
    blocks = [CASES[n][2].tobytes() for n in names]
    orders = [CASES[n][1] for n in names]
    want = [_want(oracle, orc8, n) for n in names]
    G = _Guarded(dc.dev, blocks, caps_of([H.rans_compress_bound_4x16(len(b), o) for b, o in zip(blocks, orders)]), _what(blocks, orders))
    dc.route_read("encode")
    dc.compress(*G.args(), 0, G.max_in, d_order=torch.tensor(orders, dtype=torch.int32, device=dc.dev), total_in_size=G.total_in)
    st, osz, got = G.results(("encode", direct))
    _expect(("encode", direct), G, st, osz, got, want)
    assert dc.route_read("encode") == _expected_route(oracle, names, direct)
    G = _Guarded(dc.dev, want, caps_of([len(b) for b in blocks]), _what(blocks, orders))
    dc.uncompress(*G.args(), G.max_in, G.max_cap, total_out_cap=G.total_cap)
    st, osz, got = G.results(("decode", direct))
    _expect(("decode", direct), G, st, osz, got, blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [[n] for n in X8_NAMES] + [X8_NAMES], ids=X8_NAMES + ["together"])
def test_4x8_cases(H, oracle, orc8, names):
    """k8_enc_front's normalisers against the oracle's, each case alone and all in one batch; the oracle's streams decode."""
    raws = [CASES[n][2].tobytes() for n in names]
    want = [_want(oracle, orc8, n) for n in names]
    enc, st = H.compress_batch_4x8(raws, [CASES[n][1] for n in names])
    assert all(s == 0 for s in st), st
    bad = [n for n, e, w in zip(names, enc, want) if e != w]
    assert not bad, bad
    dec, st = H.uncompress_batch_4x8(want, [len(r) for r in raws])
    assert all(s == 0 for s in st), st
    assert dec == raws


@pytest.mark.gpu
def test_4x8_device_resident_inside_guarded_slots(H, oracle, orc8):
    import torch
    from test_gpu_confinement import _Guarded, _expect, _what, caps_of
    dc = H.DeviceCodec(0)
    blocks = [CASES[n][2].tobytes() for n in X8_NAMES]
    orders = [CASES[n][1] for n in X8_NAMES]
    want = [_want(oracle, orc8, n) for n in X8_NAMES]
    G = _Guarded(dc.dev, blocks, caps_of([dc.L.rans4x8_hip_compress_bound(len(b)) for b in blocks]), _what(blocks, orders))
    dc.compress_4x8(*G.args(), 0, G.max_in, d_order=torch.tensor(orders, dtype=torch.int32, device=dc.dev))
    st, osz, got = G.results("4x8 encode")
    _expect("4x8 encode", G, st, osz, got, want)
    G = _Guarded(dc.dev, want, caps_of([len(b) for b in blocks]), _what(blocks, orders))
    dc.uncompress_4x8(*G.args())
    st, osz, got = G.results("4x8 decode")
    _expect("4x8 decode", G, st, osz, got, blocks)
