"""No GPU.  Integer models of the state update and of the output bookkeeping of the decode chain on packed rows of layout 2
(htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2, `finish` and the body of sixteen steps), executed as the
statements are written, in 32-bit arithmetic.

State update.  A row's field before its first symbol reads 1023, which stands for -1 (write_row_pk: L[j] = cum[j] - 1).
The masked form took prev = L[c] and cur = L[c + 1] out of the dword and computed
    np = ~prev;  fm1 = (cur + np) & 1023;  off = (m + np) & 1023;  x = umul24(fm1, xs) + xs + off
The mask-free form adds 1 to every field position of the rotated dword first, P = ((D << 11) | (D >> 22)) + 0x00400801, so
that the extract yields cum = cum[c] itself modulo 1024 (the carries land in bits 10, 21 and off the top, outside every
10-bit extract; bits 10 and 21 of P are zero because the guard bits of a stored dword are zero), and computes
    x = umul24(cur - cum, xs) + ((m + xs) - cum)
The pick returns the first field that is at least m, so cum <= m <= cur.

Bookkeeping.  Every step of a trip of sixteen shifts its byte into one of four accumulators with one v_alignbit_b32, and
every second step ors the flags of two rows into `bad` with one v_or3_b32, where the compiler used to gather sixteen kept
hdr words behind the body."""
import numpy as np

import test_dec_pivot_cpu as P

M32 = 0xffffffff
ONES = 0x00400801
u32 = np.uint32
u64 = np.uint64


def umul24(a, b):
    return ((a.astype(u64) & u64(0xffffff)) * (b.astype(u64) & u64(0xffffff))).astype(u32)


def masked(prev, cur, m, xs):
    """The parent's statements: (fm1, off, xn)."""
    np_ = ~prev
    fm1 = (cur + np_) & u32(1023)
    off = (m + np_) & u32(1023)
    return fm1, off, umul24(fm1, xs) + xs + off


def mask_free(cum, cur, m, xs):
    """The new statements: (fm1, off, xn); off is not computed on its own, (m + xs) - cum holds it."""
    mxs = m + xs
    fm1 = cur - cum
    return fm1, m - cum, umul24(fm1, xs) + (mxs - cum)


def test_mask_free_update_equals_the_masked_one_for_every_cum_and_cur():
    rng = np.random.default_rng(30)
    cum, cur = np.meshgrid(np.arange(1024, dtype=u32), np.arange(1024, dtype=u32), indexing="ij")
    keep = cum <= cur
    cum, cur = cum[keep], cur[keep]
    assert len(cum) == 1024 * 1025 // 2
    prev = (cum - u32(1)) & u32(1023)                      # the stored field: 1023 where cum == 0
    span = (cur - cum + u32(1)).astype(np.int64)
    ms = [cum, cur] + [(cum + (rng.integers(0, 1 << 30, size=len(cum)) % span).astype(u32)) for _ in range(3)]
    for m in ms:
        assert ((cum <= m) & (m <= cur)).all()
        for xs in (np.zeros(len(cum), u32), np.full(len(cum), (1 << 22) - 1, u32), rng.integers(0, 1 << 22, size=len(cum)).astype(u32)):
            a, b = masked(prev, cur, m, xs), mask_free(cum, cur, m, xs)
            for x, y, what in zip(a, b, ("fm1", "off", "xn")):
                assert (x == y).all(), what
            assert (a[0] <= 1023).all() and (a[1] <= a[0]).all()


def rot(D):
    return ((D << u32(11)) | (D >> u32(22))) + u32(ONES)


def dword(f0, f1, top):
    return (f0 | (f1 << u32(11)) | (top << u32(22))).astype(u32)


def test_fields_plus_one_without_carry_between_them():
    rng = np.random.default_rng(31)
    n = 200000
    f = [rng.integers(0, 1024, size=n).astype(u32) for _ in range(3)]
    for at in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):    # 1023 in each position, and in all three at once
        g = [x.copy() for x in f]
        for i in at:
            g[i][: n // 2] = 1023
        D = dword(*g)
        assert not (D & u32(P.GB)).any()                   # the guard bits of a stored dword are zero
        Pn = rot(D)
        # stride-11 order of the rotated dword: the top field, then the two low ones
        for r11, field in ((0, g[2]), (11, g[0]), (22, g[1])):
            assert (((Pn >> u32(r11)) & u32(1023)) == ((field + u32(1)) & u32(1023))).all(), (at, r11)
    # every value of one field beside 1023 in the other two
    v = np.arange(1024, dtype=u32)
    k = np.full(1024, 1023, u32)
    for D, r11 in ((dword(k, k, v), 0), (dword(v, k, k), 11), (dword(k, v, k), 22)):
        Pn = rot(D)
        assert (((Pn >> u32(r11)) & u32(1023)) == ((v + u32(1)) & u32(1023))).all()
        for other in {0, 11, 22} - {r11}:
            assert not ((Pn >> u32(other)) & u32(1023)).any()


def test_mask_free_step_on_every_slot_of_rows_as_the_front_end_builds_them():
    """The whole step on rows laid out as write_row_pk lays them out: symbol, frequency and m - start of every slot."""
    rng = np.random.default_rng(32)
    for n in P.ALPHABETS:
        for freqs in P.frequency_tables(n, rng):
            root, leaf, first, _ = P.build_row(freqs)
            cums = np.concatenate(([0], np.cumsum(freqs)))
            for m in range(1024):
                D, Dn, q, g, r, s, freq, off = P.lookup(root, leaf, first, m, P.pick2)
                r11 = 22 - 11 * (2 - r)
                Pn = ((((D << 11) | (D >> 22)) & M32) + ONES) & M32
                Cc = (D & 0x003fffff) | (Dn & 0xffc00000)
                cum, cur = (Pn >> r11) & 1023, (Cc >> r11) & 1023
                assert cum == cums[s] and cum <= m <= cur, (n, freqs, m)
                assert cur - cum == freq - 1 and m - cum == off, (n, freqs, m)
                xs = int(rng.integers(0, 1 << 22))
                assert ((cur - cum) * xs + ((m + xs) - cum)) & M32 == (freq * xs + off) & M32


def alignbit(hi, lo, sh):
    return (((hi << 32) | lo) >> sh) & M32


def test_bytes_and_flags_booked_step_by_step_equal_the_gather_behind_the_body():
    rng = np.random.default_rng(33)
    for _ in range(2000):
        hdr = [int(v) | 0x100 for v in rng.integers(0, 1 << 32, size=17)]      # hdr[u]: the row in use after step u of the trip
        t, count = int(rng.integers(0, 64)) * 16, int(rng.integers(0, 1200))
        b = [int(v) for v in rng.integers(0, 1 << 32, size=4)]                  # what the trip before left in the accumulators
        bad0 = int(rng.integers(0, 1 << 32))
        # the parent's gather: sixteen kept words, shifted in behind the body
        want = []
        for a in range(4):
            A = b[a]
            for u in range(4 * a + 1, 4 * a + 5):
                A = alignbit(hdr[u], A, 8)
            want.append(A)
        assert want == [sum((hdr[4 * a + 1 + j] & 0xff) << (8 * j) for j in range(4)) for a in range(4)]
        want_bad = bad0
        for u in range(1, 16):
            want_bad |= hdr[u]
        want_bad |= hdr[16] if t + 16 < count else 0
        # the new statements, step by step
        acc, bad, hdr_even = list(b), bad0, 0
        for u in range(1, 17):
            if u == 16:
                bad |= hdr_even | (hdr[u] if t + 16 < count else 0)
            elif u & 1:
                hdr_even = hdr[u]
            else:
                bad = bad | hdr[u] | hdr_even                                   # v_or3_b32
            a = 0 if u <= 4 else 1 if u <= 8 else 2 if u <= 12 else 3
            acc[a] = alignbit(hdr[u], acc[a], 8)                                # v_alignbit_b32
        assert acc == want and bad == want_bad
