"""The computed index words of the encode chain's affine body (htscodecs_amd/csrc/r4x16_enc_chain.h, chain_encode_o1_lds:
idx4 with AFF) as an integer model, without a GPU.

Packed rows look a (context, symbol) pair up through the WORD of a compact index j,
    word(j) = 11 j  |  (dword address of row j) << 16  =  j * wmul + wadd,     wmul = 11 | W << 16,  wadd = base << 16
(W = dwords per row, base = dword address of row 0 in LDS).  When the alphabet is a run of consecutive bytes, j = byte - c,
the loop computes the word from the byte with one 24-bit multiply-add and two constants of the lane,
    word = (byte * wmul + addend) mod 2^32,     addend = (wadd - c * wmul) mod 2^32,
and reads no idx_of[].  The addend's low half is -11 c mod 2^16: it borrows from the high half, and the sum gives the
borrow back - which holds because both halves of the RESULT are in range.  The model checks exactly that, for every
alphabet size of the packed rows, every offset c that keeps the run below byte 128 (the short-index kind) and LDS bases
up to the end of a CU's 160 KiB; then the rule by which k_enc_tables (r4x16_encode.hip) calls an alphabet affine."""
import numpy as np

M32 = (1 << 32) - 1
ENC_PK_MIN_NS, ENC_PK_MAX_NS = 20, 64
ENC_LFREQ_BYTES, ENC_IMG_IDX_SHORT = 8208, 128
LDS_BYTES = 163840


def row_dwords(ns):
    """enc_pk_row_dwords (r4x16_common.h): ns + 1 entries of 11 bits"""
    return (11 * (ns + 1) + 31) // 32


def umul24(a, b):
    """v_mul_u32_u24 / the multiply of v_mad_u32_u24: the low 24 bits of both operands, the low 32 of the product"""
    return ((a & 0xffffff) * (b & 0xffffff)) & M32


def word(j, wmul, wadd):
    return (umul24(j, wmul) + wadd) & M32


def bases(ns):
    """dword addresses of row 0 for a stream in the first, second and last seat of a workgroup, and the highest any class allows"""
    per = ENC_IMG_IDX_SHORT + 4 * ns * row_dwords(ns) + 4 + 144              # image + ring, before the class rounds it up
    seats = (LDS_BYTES - ENC_LFREQ_BYTES) // per
    first = ENC_LFREQ_BYTES + ENC_IMG_IDX_SHORT
    top = LDS_BYTES - 4 * ns * row_dwords(ns) - 4 - 144
    return sorted({first >> 2, (first + per) >> 2, (first + (seats - 1) * per) >> 2, top >> 2})


def test_word_from_byte_for_every_run():
    cases = 0
    for ns in range(ENC_PK_MIN_NS, ENC_PK_MAX_NS + 1):
        W = row_dwords(ns)
        wmul = 11 | W << 16
        assert wmul < 1 << 24                                               # an operand of a 24-bit multiply
        for base in bases(ns):
            wadd = base << 16
            for c in range(0, 128 - (ns - 1)):                              # bytes c + 1 .. c + ns - 1 stay below 128
                addend = (wadd - umul24(c, wmul)) & M32
                run = np.arange(c + 1, c + ns)                              # the bytes of the run; index j = byte - c
                if c == 0:
                    run = np.arange(0, ns)                                  # byte 0 is index 0 and may occur
                for byte in run.tolist():
                    j = byte - c
                    w = (umul24(byte, wmul) + addend) & M32
                    assert w == word(j, wmul, wadd), (ns, base, c, byte)
                    lo, hi = w & 0xffff, w >> 16
                    # both halves in range, no borrow between them: the bit offset of entry j, the dword address of row j
                    assert lo == 11 * j <= 11 * (ENC_PK_MAX_NS - 1) < 1 << 11, (ns, c, byte, lo)
                    assert hi == base + W * j and 4 * hi + 4 * W <= LDS_BYTES, (ns, base, c, byte, hi)
                    cases += 1
    assert cases > 100000


def test_constant_words_of_lanes_without_data():
    """A lane whose bytes are not its own data - no double trip: it reads the `safe` bytes - has multiplier 0: whatever
    byte it sees, its word is its addend, the word of index 0 of the image it holds: row 0, entry 0, a pair inside the
    image (the loop replaces the pair by the neutral one)."""
    for ns in (ENC_PK_MIN_NS, 46, ENC_PK_MAX_NS):
        for base in bases(ns):
            wadd = base << 16
            for byte in range(256):
                w = (umul24(byte, 0) + wadd) & M32
                assert w == word(0, 11 | row_dwords(ns) << 16, wadd)
                assert w >> 16 == base and w & 0xffff == 0


def affine_of(alpha, col0_nonzero):
    """k_enc_tables' rule.  alpha: the compact alphabet, ascending, alpha[0] == 0 (byte 0 is in every order-1 alphabet);
    col0_nonzero: byte 0 is coded somewhere (a pair counter in column 0).  c + 1, or 0."""
    ns = len(alpha)
    if ns < 2:
        return 0
    c = alpha[1] - 1
    if any(alpha[j] != j + c for j in range(1, ns)):
        return 0
    if c != 0 and col0_nonzero:
        return 0
    return c + 1


def alpha_of(data):
    return sorted(set(data) | {0})


def test_affinity_rule():
    run = bytes(range(33, 78))
    assert affine_of(alpha_of(run), False) == 33                            # quality values: c = 32
    assert affine_of(alpha_of(bytes(range(40, 60))), False) == 40
    for gap in (34, 50, 76):                                                # a byte missing from the middle
        assert affine_of(alpha_of(run.replace(bytes([gap]), b"")), False) == 0
    assert affine_of(alpha_of(run.replace(b"\x21", b"")), False) == 34      # ... from either end: still a run
    assert affine_of(alpha_of(run.replace(b"\x4d", b"")), False) == 33
    assert affine_of(alpha_of(run + b"\0"), True) == 0                      # byte 0 occurs: index 0 is not 0 - 32
    low = bytes(range(1, 46))
    assert affine_of(alpha_of(low), False) == 1                             # c == 0: index = byte
    assert affine_of(alpha_of(low + b"\0"), True) == 1                      # ... byte 0 included
    assert affine_of(alpha_of(bytes(range(2, 46))), False) == 2
    assert affine_of(alpha_of(bytes(range(2, 46)) + b"\0"), True) == 0
    assert affine_of([0], False) == 0
    # every byte of an affine block maps to the index the alphabet gives it
    for data, col0 in ((run, False), (low + b"\0", True), (bytes(range(40, 60)), False)):
        a = alpha_of(data)
        aff = affine_of(a, col0)
        assert aff and all(a.index(b) == b - (aff - 1) for b in data)
