"""No GPU.  Integer models around the ring refill of the decode chain on packed rows of layout 2
(htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2, the 256-byte ring):

  1. A property of the image layout, not of device code: all a step uses of the dword behind its group of twelve, D4, is
     the top field, L[12 g + 12], and that is field g of the root (L[12], L[24], L[36] at bits 0, 11, 22) for g = 0, 1, 2
     and 1023 for g = 3.  A step built on it (`derived_d4` below: the root rotated to the right by 11 g + 10 mod 32, all
     ones where L[36] < m) measured slower than the read and is NOT in the tree (profiles/dec_refill.md, stage 2); the
     property is what a next attempt stands on, so it is pinned here.  Checked on images laid out as write_row_pk lays
     them out - every n in 13 .. 48, every `first`, random and extreme cumulative values, the empty row: the derived
     field equals the top field of the stored dword behind the group wherever one is stored (in the row, or the next
     row's first dword with its L(0) = 1023), and the whole step comes out the same with the derived dword as with the
     stored one, GARBAGE standing behind the last row of the image.
  2. The refill of the 16-step trips, which IS in the tree: one path for both parities, the request by byte offset,
     unconditional and clamped, the mirror written by every lane (the owner of slot 0 into the mirror, the others into
     the pad), the second round only where a lane is still behind.  A model of it runs beside a model of the form it
     replaces over random cursor walks and must leave the same ring, the same `half` and ask for the same chunks; both
     are held to the stream itself: the twelve bytes a step reads at its cursor are the stream's."""
import numpy as np
import pytest

import test_dec_pivot_cpu as P

M32 = 0xffffffff
GARBAGE = P.GARBAGE


# ---- 1. the pivot dword's top field from the root ----------------------------------------------------------------------
def ror32(v, s):
    s &= 31
    return ((v >> s) | (v << (32 - s))) & M32


def derived_d4(root, g, m):
    """The pivot dword's top field from the root and g, as three instructions would make it (not in the tree: see above):
    v_mad_u32_u24 (11 g + 10), v_alignbit_b32 root, root, v_cndmask -1 / rotated."""
    ge = root >= (m << 22)                                   # L[36] >= m: what the group count took as its borrow
    return ror32(root, 11 * g + 10) if ge else M32


def step(root, D, first, m):
    """The step's arithmetic on the five dwords D (chain_decode_pk2's finish): (q, rneg, symbol, freq, m - start, the
    dword Dn was taken from is D4 and its top field was used)."""
    g, GM = P.group_of(root, m)
    Dd, Dn, q = P.pick2(*D, m << 22)
    rneg = P.popc((Dd + GM) & P.GB)
    s = 12 * g + (first + 2) + 3 * q - rneg
    r11 = 22 - 11 * rneg
    Pp = (((Dd << 11) | (Dd >> 22)) + 0x00400801) & M32
    Cc = (Dd & 0x003fffff) | (Dn & 0xffc00000)
    cum, cur = (Pp >> r11) & 1023, (Cc >> r11) & 1023
    return q, rneg, s, cur - cum + 1, m - cum, (q == 3 and rneg == 0)


def empty_row(n):
    L = lambda j: 1023
    return 1023 | (1023 << 11) | (1023 << 22), [M32 & (1023 | (1023 << 11) | (1023 << 22))] * P.row_dwords(n), 0, L


def tables_of(n, rng):
    """Frequency tables of n symbols with every possible `first`: f = 1 runs, one symbol with 1,024 - (n - 1), random
    cumulative values, a single symbol; and test_dec_pivot_cpu.py's own."""
    tabs = list(P.frequency_tables(n, rng))
    for first in range(n):
        k = n - first
        # f = 1 everywhere behind `first`, the rest on one symbol: the first, the last and a middle one
        for wide in {first, n - 1, first + k // 2}:
            f = [0] * first + [1] * k
            f[wide] += 1024 - k
            tabs.append(f)
        # random cumulative values: k - 1 distinct cuts of 1 .. 1023, so every symbol behind `first` has a frequency
        if k > 1:
            cuts = np.sort(rng.choice(np.arange(1, 1024), size=k - 1, replace=False))
            tabs.append([0] * first + np.diff(np.concatenate(([0], cuts, [1024]))).tolist())
        # random cuts WITH repeats: zero frequencies in the middle
        cuts = np.sort(rng.integers(1, 1024, size=k - 1)) if k > 1 else np.array([], dtype=np.int64)
        f = [0] * first + np.diff(np.concatenate(([0], cuts, [1024]))).tolist()
        if f[first] == 0:
            f[first], f[int(np.argmax(f))] = 1, max(f) - 1
        tabs.append(f)
        tabs.append([0] * first + [1024] + [0] * (k - 1))
    return tabs


@pytest.mark.parametrize("n", range(13, 49))
def test_pivot_from_the_root_equals_the_stored_dword(n):
    rng = np.random.default_rng(4000 + n)
    # (the last row of the image: every symbol with a frequency, so that its last group's last dword is reached)
    own = len(P.frequency_tables(n, np.random.default_rng(0)))
    rows = [empty_row(n)] + [P.build_row(f) for f in tables_of(n, rng)] + [P.build_row([1024 - (n - 1)] + [1] * (n - 1))]
    assert {r[2] for r in rows} == set(range(n)), "every possible first"
    ndw = P.row_dwords(n)
    assert 4 * ndw == 16 * ((n + 11) // 12) + (0 if n % 12 else 16)          # pk_row_bytes
    seen_g3, seen_top, seen_behind, seen_outside = 0, 0, 0, 0
    for i, (root, leaf, first, L) in enumerate(rows):
        assert len(leaf) == ndw
        last = i + 1 == len(rows)
        nxt = rows[i + 1][1] if not last else None            # the image: rows back to back, nothing known behind the last
        # every slot for the empty row, test_dec_pivot_cpu.py's tables and the last row; for the tables by `first`, every
        # slot at which the pick changes (a field's value and the slot behind it) and 32 random ones
        ms = range(1024)
        if own < i < len(rows) - 1:
            edges = {L(j) for j in range(1, n - first + 1)}
            ms = sorted({v for e in edges for v in (e, e + 1) if v < 1024} | {0, 1023} | set(rng.integers(0, 1024, size=32).tolist()))
        for m in ms:
            g, _ = P.group_of(root, m)
            stored = [(leaf[4 * g + j] if 4 * g + j < ndw else (nxt[4 * g + j - ndw] if nxt else GARBAGE)) for j in range(5)]
            d4 = derived_d4(root, g, m)
            if g <= 2:
                # field g of the root is what stands behind the group: in the row, or as the next row's L(0) = 1023
                if 4 * g + 4 < ndw or nxt:
                    assert d4 >> 22 == stored[4] >> 22, (n, first, m, g)
                    seen_behind += 4 * g + 4 >= ndw
                else:
                    assert d4 >> 22 == 1023 == L(12 * g + 12), (n, first, m, g)
            else:
                assert d4 >> 22 == 1023, (n, first, m)
            a = step(root, stored, first, m)
            b = step(root, stored[:4] + [d4], first, m)
            assert a[:5] == b[:5], (n, first, m, a, b)
            assert 0 <= b[2] < n and b[3] >= 1 and 0 <= b[4] < b[3], (n, first, m, b)
            if b[5]:                                         # the pick chose the dword behind the group and its top field
                assert d4 >> 22 == L(12 * g + 12), (n, first, m, g)
                seen_top += 1
                seen_g3 += g == 3
            seen_outside += last and 4 * g + 4 >= ndw and b[0] == 3      # the pick took Dn from outside the image (not its top)
    assert seen_top, "a step that ends in the pivot dword's top field"
    if n % 12 and n <= 36:                                   # (with four groups the dword behind the last one is g = 3's)
        assert seen_behind, "a pivot dword that is the next row's first dword"
    if n == 48:
        assert seen_g3, "n = 48: the last symbol of a row with first = 0 ends in the dword behind group 3"
    if n % 12 >= 10:                                         # (with fewer symbols in the last group its last dword is never passed)
        assert seen_outside, "the last row of the image, where that dword lies outside it"


def test_the_root_holds_what_the_rows_hold_for_every_first_of_48():
    """n = 48, first = 0: L[48] = cum[48] - 1 = 1023 because a row's frequencies sum to 1,024 (k_dec_front fails the block
    otherwise), the very value the device takes for g = 3."""
    f = [21] * 48
    f[47] += 1024 - sum(f)
    root, leaf, first, L = P.build_row(f)
    assert first == 0 and L(48) == 1023 and leaf[16] >> 22 == 1023
    g, _ = P.group_of(root, 1023)
    assert g == 3 and derived_d4(root, 3, 1023) >> 22 == 1023
    assert step(root, leaf[12:17], 0, 1023)[2] == 47


# ---- 2. the refill of the 16-step trips ---------------------------------------------------------------------------------
RB, TRIP = 256, 16


class Stream:
    """A word stream as the chain sees it: `pre` bytes in front of the words (the table's end and the four states: at
    least sixteen), the words, and what lies behind them in the same aligned sixteen."""

    def __init__(self, rng, off0, words_len):
        self.off0, self.words_len = off0, words_len
        self.avail = off0 + words_len
        self.lastc = (self.avail - 1) >> 4 if self.avail else 0
        size = 16 * (self.lastc + 1)
        # aligned[0:] is abase; the 16 bytes in front of it exist (states and table)
        self.front = rng.integers(0, 256, size=16, dtype=np.uint8)
        self.aligned = rng.integers(0, 256, size=size, dtype=np.uint8)

    def chunk(self, c):
        return self.aligned[16 * c:16 * c + 16].copy()


class Old:
    """The refill as it was: two sides by the parity of `half`, load_chunk by chunk index with a zero fill."""

    def __init__(self, st):
        self.st, self.ring, self.half, self.asked = st, np.zeros(RB + 16, dtype=np.uint8), 0, []
        for qi in range(4):
            for k in range(4):
                self.park(qi, k, self.load(4 * qi + k))
        self.pend = [[self.load(16 + k) for k in range(4)], [self.load(20 + k) for k in range(4)]]

    def load(self, c):
        if not self.st.avail:
            return np.zeros(16, dtype=np.uint8)
        c = min(c, self.st.lastc)
        self.asked.append(c)
        return self.st.chunk(c)

    def park(self, qi, k, v):
        slot = (qi & 3) * 64 + 16 * k
        self.ring[slot:slot + 16] = v
        if slot == 0:
            self.ring[RB:RB + 8] = v[:8]

    def refill(self, nh):
        for _ in range(2):
            if nh != self.half:
                side = self.half & 1
                for k in range(4):
                    self.park(self.half, k, self.pend[side][k])
                    self.pend[side][k] = self.load(4 * (self.half + 6) + k)
                self.half += 1


class New(Old):
    """The refill as it is: the request by byte offset, unconditional; the mirror or the pad written by every lane; the
    second round behind a test of its own."""

    def __init__(self, st):
        self.rounds = 0
        Old.__init__(self, st)

    def request(self, o):
        st = self.st
        o = min(o, 16 * st.lastc)
        if st.avail:
            self.asked.append(o >> 4)
            return st.chunk(o >> 4)
        assert o == 0                                        # rbase = words - 16: the sixteen bytes in front, never behind
        return st.front.copy()

    def park(self, qi, k, v):
        slot = (qi & 3) * 64 + 16 * k
        self.ring[slot:slot + 16] = v
        at = RB if slot == 0 else RB + 8
        self.ring[at:at + 8] = v[:8]

    def refill(self, nh):
        for r in range(2):
            if r == 1 and nh == self.half:
                break
            need = nh != self.half
            self.rounds += 1
            odd = self.half & 1
            if need:
                for k in range(4):
                    self.park(self.half, k, self.pend[odd][k])
                    self.pend[odd][k] = self.request(self.half * 64 + 16 * k + 384)
            self.half += 1 if need else 0


def walk(rng, off0, words_len, rate):
    """One stream through the 16-step trips, both models side by side; `rate`: the chance that a chain takes a word in a
    step (four chains, so 0 .. 4 words = 0 .. 8 bytes a step, at most 128 bytes a trip: what the ring is made for).
    Returns the set of quarters crossed per trip and whether a request was clamped."""
    st = Stream(rng, off0, words_len)
    old, new = Old(st), New(st)
    assert np.array_equal(old.ring[:RB + 8], new.ring[:RB + 8])
    nwords, cursor, crossed, clamped = words_len >> 1, 0, set(), False
    while cursor + 64 <= nwords:                             # the wave stays in the 16-step trips
        for _ in range(TRIP):
            cb = off0 + 2 * cursor
            ra = cb & (RB - 4)
            got = new.ring[ra:ra + 12]
            assert np.array_equal(got, st.aligned[cb & ~3:(cb & ~3) + 12]), (off0, words_len, cursor)
            assert np.array_equal(got, old.ring[ra:ra + 12])
            cursor += int((rng.random(4) < rate).sum())
        nh = (off0 + 2 * cursor) >> 6
        crossed.add(nh - new.half)
        before = len(new.asked)
        old.refill(nh)
        new.refill(nh)
        clamped |= any(c == st.lastc for c in new.asked[before:])
        assert old.half == new.half == nh
        assert old.asked == new.asked, "the same chunks, in the same order"
        assert np.array_equal(old.ring[:RB + 8], new.ring[:RB + 8]), "the ring and its mirror (the pad is nobody's)"
        for a, b in zip(old.pend, new.pend):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return crossed, clamped


def test_refill_model_against_the_old_one():
    rng = np.random.default_rng(77)
    for off0 in range(16):
        seen, clamp = set(), False
        for rate, words_len in ((0.05, 700), (0.45, 3000), (0.98, 4000), (1.0, 2 * 64 + 2 * 37), (0.7, 1234), (0.3, 130)):
            crossed, clamped = walk(rng, off0, words_len, rate)
            seen |= crossed
            clamp |= clamped
        assert seen == {0, 1, 2}, (off0, seen)                # no crossing, one and two quarters in a trip
        assert clamp, "lastc reached in the middle of a walk"


def test_a_stream_without_words_asks_for_its_states():
    rng = np.random.default_rng(78)
    st = Stream(rng, 0, 0)
    assert st.avail == 0 and st.lastc == 0
    new = New(st)
    # the first fill and every later request read the sixteen bytes in front of `words`, whatever offset is asked for
    for o in (0, 16, 384, 64 * 1000 + 48):
        assert np.array_equal(new.request(o), st.front)
    assert new.asked == []
