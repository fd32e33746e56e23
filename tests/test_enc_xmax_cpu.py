"""x_max of the encode chain's short-index packed rows by one multiply (htscodecs_amd/csrc/r4x16_enc_chain.h,
chain_encode_o1_lds' topk and EncOutT::step_freq / trip_freq), in integer models.  No GPU.

A packed row holds cumulative frequencies in 11-bit fields; v_alignbit delivers the 32 bits p that begin at a symbol's
field: start in bits 0..10, next in bits 11..21, the row's following fields (or whatever lies beyond the row) above.
The step wants start and x_max = (next - start) << 21, the table read wants the byte address 8 (next - start):
    X = v_mul_i32_i24(p, 2^10 - 2^21) & 0xFFE00000 = x_max,    X >> 18 = 8 f."""
import numpy as np

K = 1024 - 2097152
MASK = 0xFFE00000


def s24(v):
    """the low 24 bits as a signed number (numpy int64 in, int64 out)"""
    v = v & 0xFFFFFF
    return v - ((v & 0x800000) << 1)


def mul_i24(a, b):
    """v_mul_i32_i24: both operands' low 24 bits as signed, the low 32 bits of the product"""
    return (s24(a) * s24(b)) & 0xFFFFFFFF


def xmax_of(p):
    return mul_i24(p, np.int64(K & 0xFFFFFFFF)) & MASK


def all_pairs():
    st, nx = np.meshgrid(np.arange(1025, dtype=np.int64), np.arange(1025, dtype=np.int64), indexing="ij")
    keep = st <= nx
    return st[keep], nx[keep]


def test_model_of_the_multiply():
    assert mul_i24(np.int64(3), np.int64(5)) == 15
    assert mul_i24(np.int64(0xFFFFFF), np.int64(2)) == 0xFFFFFFFE             # -1 * 2
    assert mul_i24(np.int64(0x7F000000 | 7), np.int64(0xFF000003)) == 21      # bits above 23 are not looked at
    assert mul_i24(np.int64(0x800000), np.int64(0x800000)) == (1 << 46) & 0xFFFFFFFF
    assert s24(np.int64(K & 0xFFFFFFFF)) == K                                 # the multiplier fits its 24 bits


def test_every_pair_without_upper_bits():
    st, nx = all_pairs()
    assert len(st) == 525825
    X = xmax_of(st | nx << 11)
    f = nx - st
    assert np.array_equal(X, (f << 21) & 0xFFFFFFFF)
    assert np.array_equal(X >> 18, 8 * f)
    assert X.max() == 1 << 31 and np.all(X[f == 1024] == 1 << 31)


def test_every_pair_with_any_upper_bits():
    """bits 22..31 of p belong to the fields behind the symbol's own - or to what lies beyond the row, for the last
    symbol of the last context; bit 23 is the sign of the multiply's operand"""
    st, nx = all_pairs()
    f = nx - st
    rng = np.random.default_rng(13)
    for sign in (0, 1):
        up = rng.integers(0, 1 << 10, size=len(st), dtype=np.int64)
        up = (up & ~np.int64(2)) | sign << 1                                  # bit 23 of p is bit 1 of the upper ten
        p = st | nx << 11 | up << 22
        assert np.all((p >> 23) & 1 == sign)
        X = xmax_of(p)
        assert np.array_equal(X, (f << 21) & 0xFFFFFFFF)
        assert np.array_equal(X >> 18, 8 * f)
    p = st | nx << 11 | np.int64(0x3FF) << 22
    assert np.array_equal(xmax_of(p), (f << 21) & 0xFFFFFFFF)


def test_the_neutral_pair():
    """start 0, next 1,024: frequency 1,024, x_max = 2^31, which no state reaches; its table entry is the last"""
    X = xmax_of(np.int64(1024 << 11))
    assert X == 1 << 31
    assert X >> 18 == 8 * 1024


# ---- the step ----------------------------------------------------------------------------------------------------------
def entry(f):
    """the frequency table's entry of f (r4x16_api.hip): the low word of ceil(2^(32 + s) / f), s = ceil(log2 f), and
    (1024 - f) | s << 24"""
    s = 0
    while f > (1 << s):
        s += 1
    return ((1 << (32 + s)) + f - 1) // f - (1 << 32), (1024 - f) | s << 24


def advance(xs, m, w, start):
    q = (((xs * m) >> 32) + xs) >> ((w >> 24) & 31)
    return ((q & 0xFFFFFF) * (w & 0xFFFFFF) + xs + start) & 0xFFFFFFFF


def step_with_f(x, m, w, start, f):
    """EncOutT::step_freq as it was: x_max = f << 21 made in the step; (new state, word emitted or -1)"""
    over = x >= ((f << 21) & 0xFFFFFFFF)
    xs = np.where(over, x >> 16, x)
    return advance(xs, m, w, start), np.where(over, x & 0xFFFF, -1)


def step_with_X(x, m, w, start, X):
    over = x >= X
    xs = np.where(over, x >> 16, x)
    return advance(xs, m, w, start), np.where(over, x & 0xFFFF, -1)


def test_the_step_with_x_max_is_the_step_with_f():
    rng = np.random.default_rng(17)
    n = 4096
    for f in range(1, 1025):
        m, w = entry(f)
        start = int(rng.integers(0, 1025 - f))
        nx = start + f
        x = rng.integers(0, 1 << 31, size=n, dtype=np.int64)
        x[:4] = [0, (1 << 31) - 1, (f << 21) - 1 if f < 1024 else 0, (f << 21) & 0x7FFFFFFF]      # both sides of x_max
        up = rng.integers(0, 1 << 10, size=n, dtype=np.int64)
        X = xmax_of(start | nx << 11 | up << 22)
        a, wa = step_with_f(x, m, w, start, f)
        b, wb = step_with_X(x, m, w, start, X)
        assert np.array_equal(a, b) and np.array_equal(wa, wb), f
        # ... and both are rANS_word.h's step: xs + start + (xs / f) * (1024 - f)
        xs = np.where(x >= (f << 21), x >> 16, x)
        assert np.array_equal(a, (xs + start + (xs // f) * (1024 - f)) & 0xFFFFFFFF), f


# ---- the trip, instruction by instruction ----------------------------------------------------------------------------
def trip_model(x, written, syms, nxt, ring):
    """EncOutT::trip_freq for one quad (lanes k = 0..3; the shift that brings the quad's bits down is 0 here): the
    statement's instructions in their order, with the registers they share.  x, written: per lane; syms: four
    (m, w, start, X) per lane; nxt: two raw pairs of the next trip per lane, whose starts the statement takes behind its
    first compare; ring: the list of (slot, word) written, without the dump slot's.  Returns (x, written, starts)."""
    above = [(0xE << kk) & 0xF for kk in range(4)]
    xa, xb = list(x), [0] * 4
    pj, wr = [0] * 4, list(written)

    def write(src):
        for l in range(4):
            if pj[l] != -1:                                                   # v_mad_i32_i24 + ds_write_b16
                ring.append((pj[l], src[l] & 0xFFFF))

    def step(xi, xo, n, prev):
        vcc = sum((xi[l] >= syms[l][n][3]) << l for l in range(4))            # v_cmp_ge_u32
        if prev is not None:
            write(prev)                                                       # the previous step's, in the compare's gap
        else:
            for l in range(4):
                nxt[l] = [p & 0x7FF for p in nxt[l]]                          # 2 x v_and_b32 0x7ff
        for l in range(4):
            m, w, start, _ = syms[l][n]
            em = vcc                                                          # v_lshrrev_b64
            emit = vcc >> l & 1
            xs = xi[l] >> 16 if emit else xi[l]                               # v_cndmask_b32_sdwa .. WORD_1
            t = above[l] & em
            q = (xs * m) >> 32                                                # v_mul_hi_u32
            em &= 15
            t = bin(t).count("1") + wr[l]                                     # v_bcnt_u32_b32 (the old count)
            q = (xs + q) & 0xFFFFFFFF
            wr[l] = bin(em).count("1") + wr[l]
            q >>= (w >> 24) & 31                                              # v_lshrrev_b32_sdwa .. BYTE_3
            t &= 63
            q = (q & 0xFFFFFF) * (w & 0xFFFFFF) & 0xFFFFFFFF                  # v_mul_u32_u24
            pj[l] = t if emit else -1                                         # v_cndmask_b32 -1, t, vcc
            xo[l] = (xs + start + q) & 0xFFFFFFFF                             # v_add3_u32

    step(xa, xb, 0, None)
    step(xb, xa, 1, list(xa))
    step(xa, xb, 2, list(xb))
    step(xb, xa, 3, list(xa))
    write(xb)
    return xa, wr, nxt


def trip_reference(x, written, syms, ring):
    """four times emit16q<true> + step_freq, as the C++ form has them"""
    x, wr = list(x), written
    for n in range(4):
        over = [x[l] >= syms[l][n][3] for l in range(4)]
        em = sum(o << l for l, o in enumerate(over))
        for l in range(4):
            j = wr + bin(em >> (l + 1)).count("1")
            if over[l]:
                ring.append((j & 63, x[l] & 0xFFFF))
        wr += bin(em).count("1")
        for l in range(4):
            m, w, start, _ = syms[l][n]
            xs = x[l] >> 16 if over[l] else x[l]
            x[l] = advance(xs, m, w, start)
    return x, wr


def test_the_trip_statement_against_four_steps():
    rng = np.random.default_rng(19)
    for case in range(3000):
        syms, x = [], []
        for l in range(4):
            row = []
            for n in range(4):
                f = int(rng.choice([1, 2, 3, 5, 100, 511, 512, 1023, 1024])) if case % 3 else int(rng.integers(1, 1025))
                start = int(rng.integers(0, 1025 - f))
                m, w = entry(f)
                row.append((m, w, start, int(xmax_of(np.int64(start | (start + f) << 11)))))
            syms.append(row)
            # states on both sides of the first symbol's x_max, inside the coder's interval [2^15, 2^31)
            X0 = row[0][3]
            x.append(int(rng.integers(1 << 15, 1 << 31)) if case % 2 else min(max(X0 + int(rng.integers(-2, 3)), 1 << 15), (1 << 31) - 1))
        written = int(rng.integers(0, 200))
        ra, rb = [], []
        nxt = [[int(v) for v in rng.integers(0, 1 << 32, size=2)] for _ in range(4)]
        xa, wa, st = trip_model(x, [written] * 4, syms, [list(v) for v in nxt], ra)
        assert st == [[v & 2047 for v in lane] for lane in nxt]
        xb, wb = trip_reference(x, written, syms, rb)
        assert xa == xb and wa == [wb] * 4, case
        # the same words at the same slots (no slot twice in a trip: at most sixteen words, a ring of 64), one step late
        assert sorted(ra) == sorted(rb) and len({s for s, _ in ra}) == len(ra), case
        assert len(ra) == wb - written, case
