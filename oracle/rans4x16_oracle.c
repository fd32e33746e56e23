/*
 * rans4x16_oracle.c — CPU ORACLE (test infrastructure only; see rans4x16_oracle.h).
 *
 * Scalar restatement of the CRAM 3.1 rANS 4x16 codec exactly as htscodecs 1.1 behaves.
 * Written from the bitstream description and the behaviour of the
 * reference; every function names the reference lines it follows.  It is organised
 * differently from the reference on purpose: bounded byte readers/writers, explicit
 * work buffers instead of in-place pointer juggling, division-form encoder steps, and a
 * single renormalisation rule.  None of this file ships in the product path.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <math.h>
#include <pthread.h>

#include "rans4x16_oracle.h"

/* Flag bits of the first stream byte: rANS_static4x16pr.c:38-43 */
enum { F_ORDER = 0x01, F_STRIPE = 0x08, F_NOSZ = 0x10, F_CAT = 0x20, F_RLE = 0x40, F_PACK = 0x80 };

#define RANS_LOW   (1u << 15)          /* rANS_word.h:63 */
#define O0_BITS    12                  /* rANS_static4x16pr.c:81  */
#define O1_BITS_HI 12                  /* rANS_static4x16pr.c:86-88 */
#define O1_BITS_LO 10                  /* rANS_static4x16pr.c:89-91 */

/* ------------------------------------------------------------------------------------
 * varints: 7 bits per byte, most significant group first, 0x80 = "more follows".
 * varint.h:85-104 (put), :131-160 (get).
 * ---------------------------------------------------------------------------------- */
int orc_var_put_u32(uint8_t *cp, uint32_t v)
{
    int groups = 1;
    for (uint32_t t = v >> 7; t; t >>= 7) groups++;
    for (int g = groups - 1; g >= 0; g--)
        *cp++ = (uint8_t)(((v >> (7 * g)) & 0x7f) | (g ? 0x80 : 0));
    return groups;
}

/* Bounded read.  Mirrors varint.h:131-160: returns 0 (value 0) when cp >= endp; otherwise
 * keeps consuming continuation bytes until endp, accumulating modulo 2^32. */
int orc_var_get_u32(const uint8_t *cp, const uint8_t *endp, uint32_t *v)
{
    const uint8_t *start = cp;
    uint32_t acc = 0;
    uint8_t c;
    if (cp >= endp) { *v = 0; return 0; }
    do {
        c = *cp++;
        acc = (acc << 7) | (c & 0x7f);
    } while ((c & 0x80) && cp < endp);
    *v = acc;
    return (int)(cp - start);
}

/* ------------------------------------------------------------------------------------
 * Frequency normalisation.
 * ---------------------------------------------------------------------------------- */
/* rANS_static4x16pr.c:105-114 */
static uint32_t pow2_ceil(uint32_t v)
{
    v--;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return v + 1;
}

/* rANS_static4x16pr.c:116-163.  Scale the 256 counts in F (current total `size`) to total
 * `tot` exactly.  The largest symbol (first maximum) absorbs the rounding error; if that is
 * not possible the scaling is retried once against the achieved sum, and as a last resort
 * the excess is taken from every entry >= 2 in symbol order.  Integer types follow the
 * reference (mixed int / uint32 arithmetic) because they decide corner cases. */
int orc_normalise_freq(uint32_t *F, int size, uint32_t tot)
{
    int retried = 0;
    if (!size) return 0;

    for (;;) {
        uint64_t scale = ((uint64_t)tot << 31) / size + (1 << 30) / size;
        uint32_t best = 0;
        int arg = 0, sum = 0;
        for (int j = 0; j < 256; j++) {
            if (!F[j]) continue;
            if (best < F[j]) { best = F[j]; arg = j; }
            F[j] = (uint32_t)((F[j] * scale) >> 31);
            if (F[j] == 0) F[j] = 1;
            sum += F[j];
        }
        int adjust = (int)(tot - (uint32_t)sum);
        if (adjust > 0) {
            F[arg] += adjust;
        } else if (adjust < 0) {
            uint32_t need = (uint32_t)(-adjust);
            if (F[arg] > need && (retried || F[arg] / 2 >= need)) {
                F[arg] -= need;
            } else if (!retried) {
                retried = 1;
                size = sum;            /* the reference reuses `size` as the running sum (:125) */
                continue;
            } else {
                adjust += (int)(F[arg] - 1);
                F[arg] = 1;
                for (int j = 0; adjust && j < 256; j++) {
                    if (F[j] < 2) continue;
                    int take = (F[j] > (uint32_t)(-adjust)) ? adjust : (int)(1 - F[j]);
                    F[j] += take;
                    adjust -= take;
                }
            }
        }
        return F[arg] > 0 ? 0 : -1;
    }
}

/* rANS_static4x16pr.c:168-179: a power-of-two total is brought up to max_tot by shifting. */
static void scale_up_pow2(uint32_t *F, uint32_t size, uint32_t max_tot)
{
    if (size == 0 || size == max_tot) return;
    int sh = 0;
    while (size < max_tot) { size *= 2; sh++; }
    for (int i = 0; i < 256; i++) F[i] <<= sh;
}

/* ------------------------------------------------------------------------------------
 * Table wire format.
 * ---------------------------------------------------------------------------------- */
/* rANS_static4x16pr.c:182-206.  Ascending symbols; a symbol whose predecessor is also
 * present is followed by the count of further consecutive symbols, which become implicit. */
static int put_alphabet(uint8_t *cp, const uint32_t *F)
{
    uint8_t *start = cp;
    int implicit = 0;
    for (int j = 0; j < 256; j++) {
        if (!F[j]) continue;
        if (implicit) { implicit--; continue; }
        *cp++ = (uint8_t)j;
        if (j && F[j - 1]) {
            int k = j + 1;
            while (k < 256 && F[k]) k++;
            implicit = k - (j + 1);
            *cp++ = (uint8_t)implicit;
        }
    }
    *cp++ = 0;
    return (int)(cp - start);
}

/* rANS_static4x16pr.c:208-255.  The reference has an unchecked fast loop followed by a
 * checked one.  The fast loop only runs where the checks cannot fire, so the checked body is
 * the behaviour — with one wrinkle: the fast loop is a do/while, so when at least three
 * bytes remain the FIRST symbol is accepted even if it is 0 (that is how an alphabet
 * containing symbol 0 is written: "00 .. 00").  Returns bytes consumed, 0 on failure. */
static int get_alphabet(const uint8_t *cp, const uint8_t *end, uint32_t *F)
{
    const uint8_t *start = cp;
    int implicit = 0;
    if (cp == end) return 0;
    int j = *cp++;
    int more = (cp + 2 < end) || j;
    while (more) {
        F[j] = 1;
        if (cp >= end) return 0;
        if (!implicit && j + 1 == *cp) {
            if (cp + 1 >= end) return 0;
            j = *cp++;
            implicit = *cp++;
        } else if (implicit) {
            implicit--;
            if (++j > 255) return 0;
        } else {
            j = *cp++;
        }
        more = j && cp < end;
    }
    return (int)(cp - start);
}

/* rANS_static4x16pr.c:257-269 */
static int put_freqs_o0(uint8_t *cp, const uint32_t *F)
{
    uint8_t *start = cp;
    cp += put_alphabet(cp, F);
    for (int j = 0; j < 256; j++)
        if (F[j]) cp += orc_var_put_u32(cp, F[j]);
    return (int)(cp - start);
}

/* rANS_static4x16pr.c:271-289.  NB: like the reference, a failed alphabet parse (0 bytes)
 * is not an error by itself — the frequencies of whatever symbols were marked are read
 * from the same position. */
static int get_freqs_o0(const uint8_t *cp, const uint8_t *end, uint32_t *F, uint32_t *total)
{
    const uint8_t *start = cp;
    if (cp == end) return 0;
    cp += get_alphabet(cp, end, F);
    uint32_t tot = 0;
    for (int j = 0; j < 256; j++) {
        if (!F[j]) continue;
        cp += orc_var_get_u32(cp, end, &F[j]);
        tot += F[j];
    }
    *total = tot;
    return (int)(cp - start);
}

/* rANS_static4x16pr.c:295-325.  One row of the order-1 table: a varint per symbol of the
 * order-0 alphabet; a zero is followed by one byte holding the number of further zeros. */
static int put_freqs_o1_row(uint8_t *cp, const uint32_t *F0, const uint32_t *F)
{
    uint8_t *start = cp;
    int zeros = 0;
    for (int j = 0; j < 256; j++) {
        if (!F0[j]) continue;
        if (F[j]) {
            if (zeros) { *cp++ = 0; *cp++ = (uint8_t)(zeros - 1); zeros = 0; }
            cp += orc_var_put_u32(cp, F[j]);
        } else {
            zeros++;
        }
    }
    if (zeros) { *cp++ = 0; *cp++ = (uint8_t)(zeros - 1); }
    return (int)(cp - start);
}

/* rANS_static4x16pr.c:327-358 */
static int get_freqs_o1_row(const uint8_t *cp, const uint8_t *end, const uint32_t *F0,
                            uint32_t *F, uint32_t *total)
{
    const uint8_t *start = cp;
    uint32_t tot = 0;
    int zeros = 0;
    if (cp == end) return 0;
    for (int j = 0; j < 256 && cp < end; j++) {
        if (!F0[j]) continue;
        uint32_t f;
        if (zeros) {
            f = 0; zeros--;
        } else {
            cp += orc_var_get_u32(cp, end, &f);
            if (f == 0) {
                if (cp >= end) return 0;
                zeros = *cp++;
            }
        }
        F[j] = f;
        tot += f;
    }
    *total = tot;
    return (int)(cp - start);
}

/* ------------------------------------------------------------------------------------
 * rANS primitives (rANS_word.h).  One rule covers the reference's fast and "safe"
 * renormalisation paths: a decoder state below 2^15 takes one 16-bit little-endian word
 * if two more bytes exist (rANS_word.h:356-410; the unchecked variant is only used where
 * the bytes are known to exist: rANS_static4x16pr.c:574, :1049).
 * ---------------------------------------------------------------------------------- */
typedef struct { uint8_t *base, *ptr; } back_writer;   /* grows downwards from the end */

static inline uint32_t enc_step(uint32_t x, back_writer *w, uint32_t start, uint32_t freq, int bits)
{
    /* rANS_word.h:281-321 via the equivalent division form noted at :95-101, :310-311 */
    uint32_t x_max = ((RANS_LOW >> bits) << 16) * freq;
    if (x >= x_max) {
        w->ptr -= 2;
        w->ptr[0] = (uint8_t)x; w->ptr[1] = (uint8_t)(x >> 8);
        x >>= 16;
    }
    return ((x / freq) << bits) + (x % freq) + start;
}

static inline void enc_flush(uint32_t x, back_writer *w)   /* rANS_word.h:104-116 */
{
    w->ptr -= 4;
    w->ptr[0] = (uint8_t)x; w->ptr[1] = (uint8_t)(x >> 8);
    w->ptr[2] = (uint8_t)(x >> 16); w->ptr[3] = (uint8_t)(x >> 24);
}

static inline uint32_t rd32le(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static inline uint32_t dec_renorm(uint32_t x, const uint8_t **pp, const uint8_t *end)
{
    if (x < RANS_LOW && *pp + 2 <= end) {
        x = (x << 16) | (uint32_t)((*pp)[0] | ((*pp)[1] << 8));
        *pp += 2;
    }
    return x;
}

/* ------------------------------------------------------------------------------------
 * Order-0 stream.  rANS_static4x16pr.c:378-494 (encode), :500-616 (decode).
 * ---------------------------------------------------------------------------------- */
static uint32_t o0_bound(uint32_t n)   /* bound(size,0)-20, rANS_static4x16pr.c:390 */
{
    return orc_rans_compress_bound_4x16(n, 0) - 20;
}

int orc_o0_encode(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *out_len)
{
    if (cap < o0_bound(n)) return -1;                    /* :396 */
    if (n == 0) { *out_len = 0; return 0; }              /* :405-406, :487-489 */

    uint32_t F[256] = {0};
    for (uint32_t i = 0; i < n; i++) F[in[i]]++;         /* hist8, utils.h:80-102 */

    uint32_t target = pow2_ceil(n);
    if (target > (1u << O0_BITS)) target = 1u << O0_BITS;
    if (orc_normalise_freq(F, (int)n, target) < 0) return -1;
    uint32_t tab = (uint32_t)put_freqs_o0(out, F);       /* stored at the smaller total :422 */
    if (orc_normalise_freq(F, (int)target, 1u << O0_BITS) < 0) return -1;   /* :426 */

    uint32_t C[256], acc = 0;
    for (int j = 0; j < 256; j++) { C[j] = acc; acc += F[j]; }

    uint8_t *scratch = malloc((size_t)2 * n + 32);
    if (!scratch) return -1;
    back_writer w = { scratch, scratch + (size_t)2 * n + 32 };
    uint8_t *top = w.ptr;

    /* byte i belongs to state i&3; bytes are taken last to first, so within a group of four
     * the emit order is state 3,2,1,0 (:442-459) */
    uint32_t R[4] = { RANS_LOW, RANS_LOW, RANS_LOW, RANS_LOW };
    for (uint32_t i = n; i-- > 0; ) {
        uint8_t s = in[i];
        R[i & 3] = enc_step(R[i & 3], &w, C[s], F[s], O0_BITS);
    }
    for (int k = 3; k >= 0; k--) enc_flush(R[k], &w);    /* :482-485 */

    uint32_t pay = (uint32_t)(top - w.ptr);
    memcpy(out + tab, w.ptr, pay);                       /* :491 */
    *out_len = tab + pay;
    free(scratch);
    return 0;
}

int orc_o0_decode(const uint8_t *in, uint32_t in_size, uint8_t *out, uint32_t out_sz)
{
    if (in_size < 16) return -1;                          /* :503 */
    if (out_sz >= INT_MAX) return -1;                     /* :506 */

    const uint8_t *cp = in, *end = in + in_size;
    const uint8_t *tab_end = end - 8;                     /* :516 */
    uint32_t F[256] = {0}, total;
    int used = get_freqs_o0(cp, tab_end, F, &total);
    if (!used) return -1;
    cp += used;
    scale_up_pow2(F, total, 1u << O0_BITS);               /* :535 */

    /* slot -> symbol, plus per-symbol (freq, start): :538-552 */
    static __thread uint8_t slot_sym[1 << O0_BITS];
    uint32_t C[256], x = 0;
    for (int j = 0; j < 256; j++) {
        C[j] = x;
        if (!F[j]) continue;
        if (F[j] > (1u << O0_BITS) - x) return -1;
        memset(slot_sym + x, j, F[j]);
        x += F[j];
    }
    if (x != (1u << O0_BITS)) return -1;
    if (cp + 16 > end) return -1;                         /* :554 */

    uint32_t R[4];
    for (int k = 0; k < 4; k++, cp += 4) {
        R[k] = rd32le(cp);
        if (R[k] < RANS_LOW) return -1;                   /* :558-561 */
    }
    const uint32_t mask = (1u << O0_BITS) - 1;
    for (uint32_t i = 0; i < out_sz; i++) {               /* :574-607 */
        uint32_t r = R[i & 3], m = r & mask;
        uint8_t s = slot_sym[m];
        out[i] = s;
        r = F[s] * (r >> O0_BITS) + m - C[s];
        R[i & 3] = dec_renorm(r, &cp, end);
    }
    return 0;
}

/* ------------------------------------------------------------------------------------
 * 10-bit vs 12-bit decision.  rANS_static4x16pr.c:620-691.  Floating point, order of
 * operations preserved (build with -ffp-contract=off).
 * ---------------------------------------------------------------------------------- */
static double approx_log(double a)            /* fast_log, :620-623 */
{
    union { double d; long long x; } u = { a };
    return (u.x - 4606921278410026770LL) * 1.539095918623324e-16;
}

/* `st` (may be NULL) receives what the decision was made from - for tests that have to know which side of a rule an input
 * is on, from this arithmetic and not from a second one. */
static int compute_shift(const uint32_t *F0, const uint32_t (*F)[256], const uint32_t *T, int *S, orc_shift_stats *st)
{
    double e10 = 0, e12 = 0;
    int max_tot = 0;
    if (st) memset(st, 0, sizeof(*st));
    for (int i = 0; i < 256; i++) {
        if (!F0[i]) continue;
        int target = (int)pow2_ceil(T[i]);
        int present = 0, tiny10 = 0, tiny12 = 0;
        for (int j = 0; j < 256; j++) {
            if (!F[i][j]) continue;
            if ((uint32_t)target / F[i][j] > (1u << O1_BITS_LO)) tiny10++;
            if ((uint32_t)target / F[i][j] > (1u << O1_BITS_HI)) tiny12++;
        }
        double l10 = log((1 << O1_BITS_LO) + tiny10);
        double l12 = log((1 << O1_BITS_HI) + tiny12);
        for (int j = 0; j < 256; j++) {
            if (!F[i][j]) continue;
            present++;
            int x = (int)((double)(1 << O1_BITS_LO) * F[i][j] / T[i]);
            if (st && x < 1) st->clamped10++;
            e10 -= F[i][j] * (approx_log(x > 1 ? x : 1) - l10);
            x = (int)((double)(1 << O1_BITS_HI) * F[i][j] / T[i]);
            if (st && x < 1) st->clamped12++;
            e12 -= F[i][j] * (approx_log(x > 1 ? x : 1) - l12);
            e10 += 4;
            e12 += 6;
        }
        if (st) { st->present[i] = present; st->tiny10[i] = tiny10; st->tiny12[i] = tiny12; st->target0[i] = target; }
        if (present < 64 && target > 128) target /= 2;    /* :678-681 */
        if (target > 1024) target /= 2;
        if (target > (1 << O1_BITS_HI)) target = 1 << O1_BITS_HI;
        S[i] = target;
        if (max_tot < target) max_tot = target;
    }
    if (st) { st->e10 = e10; st->e12 = e12; st->ratio = e10 / e12; st->max_tot = max_tot; }
    return (e10 / e12 < 1.01 || max_tot <= (1 << O1_BITS_LO)) ? O1_BITS_LO : O1_BITS_HI;
}

int orc_compute_shift(const uint32_t *F0, const uint32_t (*F)[256], const uint32_t *T, int *S)
{
    return compute_shift(F0, F, T, S, NULL);
}

int orc_compute_shift_stats(const uint32_t *F0, const uint32_t (*F)[256], const uint32_t *T, int *S, orc_shift_stats *st)
{
    return compute_shift(F0, F, T, S, st);
}

/* ------------------------------------------------------------------------------------
 * Order-1 stream.  rANS_static4x16pr.c:694-847 (encode), :869-1130 (decode).
 * ---------------------------------------------------------------------------------- */
static uint32_t o1_bound(uint32_t n) { return orc_rans_compress_bound_4x16(n, 1) - 20; }  /* :700 */

int orc_o1_encode(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *out_len)
{
    if (cap < o1_bound(n)) return -1;                     /* :706 */
    if (n < 4) return -1;      /* the reference is never entered below 8 bytes (:1322) */

    int rc = -1;
    uint32_t (*F)[256] = calloc(256, sizeof(*F));
    uint32_t (*C)[256] = malloc(256 * sizeof(*C));
    uint8_t *table = malloc(257 * 257 * 3 + 16);
    uint8_t *scratch = malloc((size_t)2 * n + 64);
    uint8_t *nested = NULL;
    if (!F || !C || !table || !scratch) goto done;

    uint32_t T[256] = {0}, F0[256] = {0};
    const uint32_t q = n >> 2;

    /* hist1_4 (utils.h:136-202): every adjacent pair, the first byte seen in context 0;
     * plus the three quarter starts coded in context 0 (:720-723). */
    {
        uint8_t prev = 0;
        for (uint32_t i = 0; i < n; i++) { F[prev][in[i]]++; T[prev]++; prev = in[i]; }
        for (int k = 1; k < 4; k++) F[0][in[k * q]]++;
        T[0] += 3;
    }
    for (uint32_t i = 0; i < n; i++) F0[in[i]] = 1;       /* present8, utils.h:108-131 */
    F0[0] = 1;                                            /* :731 */

    uint8_t *tp = table;
    tp += put_alphabet(tp, F0);                           /* :732 */

    int S[256] = {0};
    int bits = orc_compute_shift(F0, (const uint32_t (*)[256])F, T, S);   /* :737 */

    for (int i = 0; i < 256; i++) {                       /* :740-764 */
        if (!F0[i]) continue;
        int target = S[i];
        if (bits == O1_BITS_LO && target > (1 << O1_BITS_LO)) target = 1 << O1_BITS_LO;
        if (orc_normalise_freq(F[i], (int)T[i], (uint32_t)target) < 0) goto done;
        tp += put_freqs_o1_row(tp, F0, F[i]);
        scale_up_pow2(F[i], (uint32_t)target, 1u << bits);
        uint32_t acc = 0;
        for (int j = 0; j < 256; j++) { C[i][j] = acc; acc += F[i][j]; }
    }

    /* header byte + table, optionally order-0 compressed (:766-780).  The 1000-byte test and
     * the "6 bytes smaller" test both count the header byte. */
    uint32_t tlen = (uint32_t)(tp - table);
    uint8_t *op = out;
    *op++ = (uint8_t)(bits << 4);
    int stored = 0;
    if (1 + tlen > 1000) {
        uint32_t ncap = o0_bound(tlen), nlen = 0;
        nested = malloc(ncap);
        if (nested && orc_o0_encode(table, tlen, nested, ncap, &nlen) == 0 && nlen + 6 < 1 + tlen) {
            out[0] |= 1;
            op += orc_var_put_u32(op, tlen);
            op += orc_var_put_u32(op, nlen);
            memcpy(op, nested, nlen);
            op += nlen;
            stored = 1;
        }
    }
    if (!stored) { memcpy(op, table, tlen); op += tlen; }
    uint32_t tab = (uint32_t)(op - out);

    /* Four states over four contiguous quarters, state 3 also takes the tail.  Symbols are
     * consumed last to first; the first byte of each quarter is coded in context 0 (:794-834). */
    back_writer w = { scratch, scratch + (size_t)2 * n + 64 };
    uint8_t *top = w.ptr;
    uint32_t R[4] = { RANS_LOW, RANS_LOW, RANS_LOW, RANS_LOW };

    for (uint32_t p = n - 1; p >= 4 * q; p--)              /* tail on state 3 (:806-811) */
        R[3] = enc_step(R[3], &w, C[in[p - 1]][in[p]], F[in[p - 1]][in[p]], bits);
    for (uint32_t r = q; r-- > 1; ) {                      /* offsets q-1 .. 1 inside each quarter */
        for (int k = 3; k >= 0; k--) {
            uint32_t p = k * q + r;
            R[k] = enc_step(R[k], &w, C[in[p - 1]][in[p]], F[in[p - 1]][in[p]], bits);
        }
    }
    for (int k = 3; k >= 0; k--) {                        /* quarter starts in context 0 (:831-834) */
        uint8_t s = in[k * q];
        R[k] = enc_step(R[k], &w, C[0][s], F[0][s], bits);
    }
    for (int k = 3; k >= 0; k--) enc_flush(R[k], &w);     /* :836-839 */

    uint32_t pay = (uint32_t)(top - w.ptr);
    memcpy(out + tab, w.ptr, pay);                        /* :844 */
    *out_len = tab + pay;
    rc = 0;
done:
    free(F); free(C); free(table); free(scratch); free(nested);
    return rc;
}

/* The reference keeps slot->symbol rows in one big per-thread block whose row stride is
 * (1<<10)+179 unless the header says 12 bits, and it only ever looks up 10 or 12 bits
 * (:924-930, :1027-1114).  Streams written by the encoder always say 10 or 12, but the
 * decoder accepts any value 0..15 in the header; for 11, 13, 14, 15 the result is still
 * deterministic (rows overlap, yet the first 1024 slots of each row survive), so it is
 * reproduced here by using the same layout.  Below 10 the reference reads slots it never
 * wrote; the oracle rejects those. */
#define ROW_PAD 179                                       /* MAGIC2, :862 */

int orc_o1_decode(const uint8_t *in, uint32_t in_size, uint8_t *out, uint32_t out_sz)
{
    if (in_size < 16) return -1;                          /* :872 */
    if (out_sz >= INT_MAX) return -1;                     /* :875 */

    int rc = -1;
    const uint8_t *cp = in, *end = in + in_size;
    uint8_t *plain = NULL;                                /* nested-decoded table */
    uint8_t *slots = calloc(256 * ((1 << O1_BITS_HI) + ROW_PAD), 1);
    uint16_t (*fq)[256] = calloc(256, sizeof(*fq));       /* freq  per (ctx,sym) */
    uint16_t (*st)[256] = calloc(256, sizeof(*st));       /* start per (ctx,sym) */
    if (!slots || !fq || !st) goto done;

    const unsigned bits = *cp >> 4;                       /* :943 */
    const int compressed = *cp++ & 1;
    if (bits < O1_BITS_LO) goto done;                     /* see note above */
    const unsigned look = (bits == O1_BITS_HI) ? O1_BITS_HI : O1_BITS_LO;
    const size_t stride = (1u << look) + ROW_PAD;

    const uint8_t *tcp = cp, *tend = end, *after_table = NULL;
    if (compressed) {                                     /* :944-955 */
        uint32_t usz, csz;
        cp += orc_var_get_u32(cp, end, &usz);
        cp += orc_var_get_u32(cp, end, &csz);
        if ((long)csz >= (long)(end - cp) - 16) goto done;
        after_table = cp + csz;
        plain = malloc(usz ? usz : 1);
        if (!plain || orc_o0_decode(cp, csz, plain, usz) < 0) goto done;
        tcp = plain; tend = plain + usz;
    }

    uint32_t F0[256] = {0};
    int used = get_alphabet(tcp, tend, F0);               /* :959 */
    if (!used) goto done;
    tcp += used;
    if (tcp >= tend) goto done;                           /* :964 */

    for (int i = 0; i < 256; i++) {                       /* :967-998 */
        if (!F0[i]) continue;
        uint32_t F[256] = {0}, tot = 0;
        used = get_freqs_o1_row(tcp, tend, F0, F, &tot);
        if (!used) goto done;
        tcp += used;
        if (!tot) continue;
        scale_up_pow2(F, tot, 1u << bits);
        uint32_t x = 0;
        for (int j = 0; j < 256; j++) {
            if (!F[j]) continue;
            if (F[j] > (1u << bits) - x) goto done;
            memset(slots + i * stride + x, j, F[j]);
            fq[i][j] = (uint16_t)F[j];
            st[i][j] = (uint16_t)x;
            x += F[j];
        }
        if (x != (1u << bits)) goto done;
    }
    cp = compressed ? after_table : tcp;                  /* :1000-1001 */
    if (cp + 16 > end) goto done;                         /* :1005 */

    uint32_t R[4];
    for (int k = 0; k < 4; k++, cp += 4) {
        R[k] = rd32le(cp);
        if (R[k] < RANS_LOW) goto done;                   /* :1010-1013 */
    }

    const uint32_t q = out_sz >> 2, mask = (1u << look) - 1;
    uint8_t ctx[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < q; r++) {                    /* :1031-1060 / :1074-1103 */
        for (int k = 0; k < 4; k++) {
            uint32_t m = R[k] & mask;
            uint8_t s = slots[ctx[k] * stride + m];
            R[k] = (uint32_t)fq[ctx[k]][s] * (R[k] >> look) + m - st[ctx[k]][s];
            out[k * q + r] = ctx[k] = s;
        }
        for (int k = 0; k < 4; k++) R[k] = dec_renorm(R[k], &cp, end);
    }
    for (uint32_t p = 4 * q; p < out_sz; p++) {           /* tail on state 3 (:1063-1070) */
        uint32_t m = R[3] & mask;
        uint8_t s = slots[ctx[3] * stride + m];
        R[3] = (uint32_t)fq[ctx[3]][s] * (R[3] >> look) + m - st[ctx[3]][s];
        out[p] = ctx[3] = s;
        R[3] = dec_renorm(R[3], &cp, end);
    }
    rc = 0;
done:
    free(slots); free(fq); free(st); free(plain);
    return rc;
}

/* ------------------------------------------------------------------------------------
 * Bit packing.  pack.c:56-151 (pack), :165-198 (meta), :211-348 (unpack).
 * ---------------------------------------------------------------------------------- */
/* meta[0] = number of distinct symbols (256 wraps to 0), then the symbols — unless there are
 * more than 16, in which case meta is that single byte and the data is copied unchanged. */
int orc_pack(const uint8_t *in, uint64_t n, uint8_t *meta, int *meta_len, uint8_t *out, uint64_t *out_len)
{
    int code[256], seen[256] = {0}, nsym = 0;
    for (uint64_t i = 0; i < n; i++) seen[in[i]] = 1;
    for (int s = 0; s < 256; s++)
        if (seen[s]) { code[s] = nsym++; meta[nsym] = (uint8_t)s; }
    meta[0] = (uint8_t)nsym;

    if (nsym > 16) {
        *meta_len = 1;
        memcpy(out, in, n);
        *out_len = n;
        return 0;
    }
    *meta_len = nsym + 1;
    int per = nsym > 4 ? 2 : nsym > 2 ? 4 : nsym > 1 ? 8 : 0;   /* symbols per byte; 0 = constant */
    if (per == 0) { *out_len = 0; return 0; }
    int width = 8 / per;
    uint64_t nout = (n + per - 1) / per;
    for (uint64_t b = 0; b < nout; b++) {
        unsigned v = 0;
        for (int k = 0; k < per && b * per + k < n; k++)
            v |= (unsigned)code[in[b * per + k]] << (k * width);     /* first symbol in the low bits */
        out[b] = (uint8_t)v;
    }
    *out_len = nout;
    return 0;
}

/* pack.c:165-198.  Returns bytes of meta consumed (0 = failure); *per = symbols per byte. */
static unsigned unpack_meta(const uint8_t *data, uint32_t len, uint8_t *map, int *per)
{
    if (len == 0) return 0;
    unsigned n = data[0] ? data[0] : 256;
    if (n <= 1) *per = 0;
    else if (n <= 2) *per = 8;
    else if (n <= 4) *per = 4;
    else if (n <= 16) *per = 2;
    else { *per = 1; return 1; }
    if (len <= 1) return 0;
    unsigned j = 1, c = 0;
    do { map[c++] = data[j++]; } while (c < n && j < len);
    return c < n ? 0 : j;
}

/* pack.c:211-348 */
static int unpack(const uint8_t *data, int64_t len, uint8_t *out, uint64_t out_len, int per, const uint8_t *map)
{
    if (per == 1) { memcpy(out, data, (size_t)len); return 0; }
    if (per == 0) { memset(out, map[0], out_len); return 0; }
    if (per != 2 && per != 4 && per != 8) return -1;
    if ((int64_t)((out_len + per - 1) / per) > len) return -1;
    int width = 8 / per;
    unsigned mask = (1u << width) - 1;
    for (uint64_t i = 0; i < out_len; i++)
        out[i] = map[(data[i / per] >> ((i % per) * width)) & mask];
    return 0;
}

/* ------------------------------------------------------------------------------------
 * Run-length split.  rle.c:48-98 (symbol choice), :100-138 (encode), :142-187 (decode).
 * ---------------------------------------------------------------------------------- */
int orc_rle_encode(const uint8_t *in, uint64_t n, uint8_t *runs, uint64_t *runs_len,
                   uint8_t *syms, int *nsyms, uint8_t *lits, uint64_t *lits_len)
{
    /* a symbol is worth run-length coding if it repeats its predecessor more often than not */
    int64_t score[256] = {0};
    int last = -1;
    for (uint64_t i = 0; i < n; i++) {
        score[in[i]] += (in[i] == last) ? 1 : -1;
        last = in[i];
    }
    int ns = 0;
    for (int s = 0; s < 256; s++) if (score[s] > 0) syms[ns++] = (uint8_t)s;
    *nsyms = ns;

    uint64_t nl = 0, nr = 0;
    for (uint64_t i = 0; i < n; ) {
        uint8_t b = in[i];
        lits[nl++] = b;
        if (score[b] > 0) {
            uint64_t j = i + 1;
            while (j < n && in[j] == b) j++;
            nr += orc_var_put_u32(runs + nr, (uint32_t)(j - i - 1));
            i = j;
        } else {
            i++;
        }
    }
    *runs_len = nr;
    *lits_len = nl;
    return 0;
}

static int rle_expand(const uint8_t *lit, uint64_t lit_len, const uint8_t *run, uint64_t run_len,
                      const uint8_t *syms, int nsyms, uint8_t *out, uint64_t *out_len)
{
    uint8_t is_rle[256] = {0};
    for (int j = 0; j < nsyms; j++) is_rle[syms[j]] = 1;
    const uint8_t *run_end = run + run_len;
    uint8_t *op = out, *oend = out + *out_len;
    for (uint64_t i = 0; i < lit_len; i++) {
        if (op >= oend) return -1;
        uint8_t b = lit[i];
        uint32_t extra = 0;
        if (is_rle[b]) run += orc_var_get_u32(run, run_end, &extra);
        if (extra) {
            if ((uint64_t)(oend - op) <= extra) return -1;   /* rle.c:173 */
            memset(op, b, (size_t)extra + 1);
            op += (size_t)extra + 1;
        } else {
            *op++ = b;
        }
    }
    *out_len = (uint64_t)(op - out);
    return 0;
}

/* ------------------------------------------------------------------------------------
 * Container.  rANS_static4x16pr.c:360-372 (bound), :1138-1345 (encode), :1352-1636 (decode).
 * ---------------------------------------------------------------------------------- */
unsigned int orc_rans_compress_bound_4x16(unsigned int size, int order)
{
    int N = order >> 8;
    if (!N) N = 4;
    order &= 0xff;
    /* evaluated in double and truncated once, as in the reference */
    double d = (order == 0 ? 1.05 * size + 257 * 3 + 4
                           : 1.05 * size + 257 * 257 * 3 + 4 + 257 * 3 + 4)
             + ((order & F_PACK) ? 1 : 0)
             + ((order & F_RLE) ? 1 + 257 * 3 + 4 : 0) + 20
             + ((order & F_STRIPE) ? 1 + 5 * N : 0);
    int sz = (int)d;
    return (unsigned)(sz + (sz & 1) + 2);
}

static unsigned char *encode_striped(unsigned char *in, unsigned int n, unsigned char *out,
                                     unsigned int *out_size, int order);

unsigned char *orc_rans_compress_to_4x16(unsigned char *in, unsigned int in_size,
                                         unsigned char *out, unsigned int *out_size, int order)
{
    unsigned char *mine = NULL;
    if (!out) {
        *out_size = orc_rans_compress_bound_4x16(in_size, order);
        if (!(out = mine = malloc(*out_size))) return NULL;
    } else if (*out_size < orc_rans_compress_bound_4x16(in_size, order)) {
        /* The reference's inner coders refuse short buffers (:396, :706) but the wrapper does
         * not look at that; every in-tree caller passes a bound-sized buffer.  We refuse. */
        return NULL;
    }

    if (in_size <= 20) order &= ~F_STRIPE;                /* :1151 */
    if (order & F_STRIPE) {
        unsigned char *r = encode_striped(in, in_size, out, out_size, order);
        if (!r) free(mine);
        return r;
    }

    if (order & F_CAT) {                                  /* :1218-1225 */
        unsigned hdr = 1;
        out[0] = F_CAT;
        hdr += orc_var_put_u32(out + 1, in_size);
        memcpy(out + hdr, in, in_size);
        *out_size = hdr + in_size;
        return out;
    }

    int want_pack = order & F_PACK, want_rle = order & F_RLE, nosz = order & F_NOSZ;
    unsigned hdr = 1;
    uint8_t *packed = NULL, *lits = NULL, *rmeta = NULL, *tmp = NULL;
    unsigned char *ret = NULL;
    const uint8_t *data = in;
    unsigned int dlen = in_size;

    out[0] = (unsigned char)order;                        /* :1231 */
    if (!nosz) hdr += orc_var_put_u32(out + 1, in_size);
    order &= 0xf;

    if (want_pack && dlen) {                              /* :1244-1264 */
        int mlen; uint64_t plen;
        packed = malloc((size_t)dlen + 1);
        if (!packed) goto fail;
        orc_pack(data, dlen, out + hdr, &mlen, packed, &plen);
        if (mlen == 1 && out[hdr] > 16) {                 /* n==256 wraps to 0 and stays packed */
            out[0] &= ~F_PACK;
        } else {
            data = packed; dlen = (unsigned)plen;
            hdr += mlen;
            hdr += orc_var_put_u32(out + hdr, dlen);
        }
    } else if (want_pack) {
        out[0] &= ~F_PACK;                                /* :1265-1266 */
    }

    if (want_rle && dlen) {                               /* :1269-1316 */
        uint64_t runs_len, lits_len;
        uint8_t syms[256]; int nsyms = 0;
        rmeta = malloc((size_t)dlen * 5 + 257 + 8);
        lits = malloc((size_t)dlen + 8);
        if (!rmeta || !lits) goto fail;
        /* meta := nsyms (256 -> 0), syms, run varints (:1282-1285) */
        orc_rle_encode(data, dlen, rmeta + 257, &runs_len, syms, &nsyms, lits, &lits_len);
        uint8_t *m = rmeta + 257 - (1 + nsyms);
        m[0] = (uint8_t)nsyms;
        memcpy(m + 1, syms, nsyms);
        unsigned mlen = (unsigned)(runs_len + nsyms + 1);

        if ((double)(lits_len + mlen) >= .99 * dlen) {    /* :1287 */
            out[0] &= ~F_RLE;
        } else {
            uint32_t ccap = o0_bound(mlen), clen = 0;
            tmp = malloc(ccap);
            if (!tmp || orc_o0_encode(m, mlen, tmp, ccap, &clen) < 0) goto fail;
            if (clen < mlen) {                            /* :1299-1301 */
                hdr += orc_var_put_u32(out + hdr, mlen * 2);
                hdr += orc_var_put_u32(out + hdr, (uint32_t)lits_len);
                hdr += orc_var_put_u32(out + hdr, clen);
                memcpy(out + hdr, tmp, clen);
                hdr += clen;
            } else {                                      /* raw meta, odd marker (:1303-1307) */
                hdr += orc_var_put_u32(out + hdr, mlen * 2 + 1);
                hdr += orc_var_put_u32(out + hdr, (uint32_t)lits_len);
                memcpy(out + hdr, m, mlen);
                hdr += mlen;
            }
            data = lits; dlen = (unsigned)lits_len;
        }
    } else if (want_rle) {
        out[0] &= ~F_RLE;                                 /* :1317-1318 */
    }

    if (order && dlen < 8) { out[0] &= ~1; order &= ~1; } /* :1322-1325 */

    {
        uint32_t cap = (order == 1 ? o1_bound(dlen) : o0_bound(dlen)), plen = 0;
        uint8_t *pay = malloc(cap);
        if (!pay) goto fail;
        int rc = (order == 1) ? orc_o1_encode(data, dlen, pay, cap, &plen)
                              : orc_o0_encode(data, dlen, pay, cap, &plen);
        if (rc < 0) { free(pay); goto fail; }
        if (plen >= dlen) {                               /* :1332-1337: raw copy instead */
            out[0] &= ~3;
            out[0] |= F_CAT | nosz;
            memcpy(out + hdr, data, dlen);
            plen = dlen;
        } else {
            memcpy(out + hdr, pay, plen);
        }
        free(pay);
        *out_size = hdr + plen;
    }
    ret = out;
fail:
    if (!ret) free(mine);
    free(packed); free(lits); free(rmeta); free(tmp);
    return ret;
}

/* :1154-1216.  Byte i of the input goes to sub-stream i mod N; each sub-stream is coded on its
 * own (X_NOSZ) with whichever of {order1, RLE, PACK, plain} allowed by `order` is smallest. */
static unsigned char *encode_striped(unsigned char *in, unsigned int n, unsigned char *out,
                                     unsigned int *out_size, int order)
{
    int N = order >> 8;
    if (N == 0) N = 4;
    if (N > 255) return NULL;

    unsigned int part[256], first[256];
    unsigned char *planes = malloc(n ? n : 1);
    if (!planes) return NULL;
    for (int i = 0; i < N; i++) {
        part[i] = n / N + ((n % N) > (unsigned)i);
        first[i] = i ? first[i - 1] + part[i - 1] : 0;
    }
    for (unsigned int i = 0; i < n; i++) planes[first[i % N] + i / N] = in[i];

    unsigned hdr = 1;
    out[0] = (unsigned char)(order & ~F_NOSZ);
    hdr += orc_var_put_u32(out + hdr, n);
    out[hdr++] = (unsigned char)N;

    static const int methods[4] = { 1, 64, 128, 0 };
    unsigned char *body = malloc(*out_size), *bp = body, *trial = NULL;
    if (!body) { free(planes); return NULL; }
    for (int i = 0; i < N; i++) {
        unsigned int best_sz = n + 10, tsz;
        int best = 0;
        unsigned int tcap = orc_rans_compress_bound_4x16(part[i], 0xc1 | F_NOSZ);
        trial = malloc(tcap);
        if (!trial) { free(planes); free(body); return NULL; }
        for (int j = 0; j < 4; j++) {
            if ((order & methods[j]) != methods[j]) continue;
            tsz = tcap;
            if (!orc_rans_compress_to_4x16(planes + first[i], part[i], trial, &tsz, methods[j] | F_NOSZ))
                { free(planes); free(body); free(trial); return NULL; }
            if (best_sz > tsz) { best_sz = tsz; best = j; }
        }
        tsz = tcap;
        orc_rans_compress_to_4x16(planes + first[i], part[i], trial, &tsz, methods[best] | F_NOSZ);
        memcpy(bp, trial, tsz);
        bp += tsz;
        hdr += orc_var_put_u32(out + hdr, tsz);
        free(trial);
    }
    memcpy(out + hdr, body, (size_t)(bp - body));
    *out_size = hdr + (unsigned)(bp - body);
    free(planes); free(body);
    return out;
}

unsigned char *orc_rans_compress_4x16(unsigned char *in, unsigned int in_size,
                                      unsigned int *out_size, int order)
{
    return orc_rans_compress_to_4x16(in, in_size, NULL, out_size, order);
}

/* :1360-1433 */
static unsigned char *decode_striped(unsigned char *in, unsigned int in_size,
                                     unsigned char *out, unsigned int *out_size)
{
    const uint8_t *end = in + in_size;
    unsigned int ulen, hdr = 1;
    unsigned char *mine = NULL;
    hdr += orc_var_get_u32(in + hdr, end, &ulen);
    if (hdr >= in_size) return NULL;
    unsigned N = in[hdr++];
    unsigned int clen[256], plen[256], first[256];
    if (!out) {
        if (ulen >= INT_MAX) return NULL;
        if (!(out = mine = malloc(ulen ? ulen : 1))) return NULL;
        *out_size = ulen;
    }
    if (ulen != *out_size) { free(mine); return NULL; }

    uint64_t ctot = 0;
    for (unsigned i = 0; i < N; i++) {
        plen[i] = ulen / N + ((ulen % N) > i);
        first[i] = i ? first[i - 1] + plen[i - 1] : 0;
        hdr += orc_var_get_u32(in + hdr, end, &clen[i]);
        ctot += clen[i];
        if (hdr > in_size || clen[i] > in_size || clen[i] < 1) { free(mine); return NULL; }
    }
    if (hdr + ctot > in_size) { free(mine); return NULL; }
    in_size = (unsigned)(hdr + ctot);

    unsigned char *planes = malloc(ulen ? ulen : 1);
    if (!planes) { free(mine); return NULL; }
    for (unsigned i = 0; i < N; i++) {
        unsigned int got = plen[i];
        if (in_size < hdr ||
            !orc_rans_uncompress_to_4x16(in + hdr, in_size - hdr, planes + first[i], &got) ||
            got != plen[i]) {
            free(mine); free(planes); return NULL;
        }
        hdr += clen[i];
    }
    /* unstripe, utils.h:41-73: out[i] = plane (i mod N), element i / N.  (N == 0 with data
     * makes the reference spin forever; we fail instead.) */
    if (!N && ulen) { free(mine); free(planes); return NULL; }
    for (unsigned int i = 0; i < ulen; i++) out[i] = planes[first[i % N] + i / N];
    free(planes);
    *out_size = ulen;
    return out;
}

unsigned char *orc_rans_uncompress_to_4x16(unsigned char *in, unsigned int in_size,
                                           unsigned char *out, unsigned int *out_size)
{
    if (in_size == 0) return NULL;                        /* :1357 */
    if (in[0] & F_STRIPE) return decode_striped(in, in_size, out, out_size);

    const uint8_t *end = in + in_size;
    const uint8_t *cp = in;
    int flags = *cp++;
    unsigned int left = in_size - 1;
    const int do_pack = flags & F_PACK, do_rle = flags & F_RLE, do_cat = flags & F_CAT;
    const int nosz = flags & F_NOSZ, order = flags & 1;
    unsigned char *mine = NULL, *tmp = NULL, *meta_owned = NULL;
    unsigned char *ret = NULL;

    unsigned int osz;
    {
        int sz = 0;
        if (!nosz) sz = orc_var_get_u32(cp, end, &osz);
        else { if (!out) return NULL; osz = *out_size; }  /* :1444-1457 */
        cp += sz; left -= sz;
    }
    if (!out) {
        *out_size = osz;
        if (!(out = mine = malloc(osz ? osz : 1))) return NULL;
    } else {
        if (*out_size < osz) return NULL;                 /* :1464 */
        *out_size = osz;
    }

    /* stage buffers as in the reference's table (:1480-1520) */
    unsigned char *s1 = out, *s2 = out, *s3 = out;        /* rans -> s1, unrle -> s2, unpack -> s3 */
    unsigned int s1_size = osz;
    if (do_pack || do_rle) {
        if (!(tmp = malloc(osz ? osz : 1))) goto fail;
        if (do_pack && do_rle) { s1 = out; s2 = tmp; s3 = out; }
        else if (do_pack)      { s1 = tmp; s2 = tmp; s3 = out; }
        else                   { s1 = tmp; s2 = out; s3 = out; }
    }

    uint8_t map[16] = {0};
    int per = 0;
    uint64_t unpacked = 0;
    if (do_pack) {                                        /* :1527-1545 */
        unsigned used = unpack_meta(cp, left, map, &per);
        if (!used) goto fail;
        unpacked = osz;
        cp += used; left -= used;
        unsigned int psz;
        int sz = orc_var_get_u32(cp, end, &psz);
        cp += sz; left -= sz;
        if (psz > s1_size) goto fail;
        s1_size = psz;
    }

    const uint8_t *meta = NULL;
    uint32_t meta_len = 0;
    if (do_rle) {                                         /* :1549-1572 */
        uint32_t c_meta, lit_len, sz;
        sz  = orc_var_get_u32(cp, end, &meta_len);
        sz += orc_var_get_u32(cp + sz, end, &lit_len);
        if (lit_len > s1_size) goto fail;
        if (meta_len & 1) {
            meta = cp + sz;
            long avail = (long)(end - meta);
            meta_len = ((long)(meta_len / 2) > avail) ? (uint32_t)avail : meta_len / 2;
            c_meta = meta_len;
        } else {
            sz += orc_var_get_u32(cp + sz, end, &c_meta);
            meta_len /= 2;
            meta_owned = malloc(meta_len ? meta_len : 1);
            if (!meta_owned || orc_o0_decode(cp + sz, left - sz, meta_owned, meta_len) < 0) goto fail;
            meta = meta_owned;
        }
        if (c_meta + sz > left) goto fail;
        cp += c_meta + sz; left -= c_meta + sz;
        s1_size = lit_len;
    }

    if (left) {                                           /* :1577-1595 */
        if (do_cat) {
            if (s1_size > left || s1_size > *out_size) goto fail;
            memcpy(s1, cp, s1_size);
        } else {
            int rc = order ? orc_o1_decode(cp, left, s1, s1_size) : orc_o0_decode(cp, left, s1, s1_size);
            if (rc < 0) goto fail;
        }
    } else {
        s1 = NULL; s1_size = 0;
    }
    unsigned int s2_size = s1_size, s3_size = s1_size;

    if (do_rle) {                                         /* :1598-1613 */
        if (meta_len == 0) goto fail;
        int nsyms = meta[0] ? meta[0] : 256;
        if (meta_len < 1u + nsyms) goto fail;
        uint64_t n = *out_size;
        if (rle_expand(s1, s1_size, meta + 1 + nsyms, meta_len - (1 + nsyms), meta + 1, nsyms, s2, &n) < 0)
            goto fail;
        s2_size = s3_size = (unsigned)n;
    }
    if (do_pack) {                                        /* :1614-1623 */
        if (per == 1) unpacked = s2_size;
        if (unpack(s2, s2_size, s3, unpacked, per, map) < 0) goto fail;
        s3_size = (unsigned)unpacked;
    }
    *out_size = s3_size;
    ret = s3;
fail:
    free(tmp); free(meta_owned);
    if (!ret) free(mine);
    return ret;
}

unsigned char *orc_rans_uncompress_4x16(unsigned char *in, unsigned int in_size, unsigned int *out_size)
{
    return orc_rans_uncompress_to_4x16(in, in_size, NULL, out_size);
}

/* ------------------------------------------------------------------------------------
 * "All cores" helper for the CPU baseline (bench.py): static split of the block list over
 * pthreads.  The codec is re-entrant, as the reference is (SURVEY §8b threading).
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int lo, hi, order, decode, failed;
    unsigned char *const *in; const unsigned int *in_size;
    unsigned char *const *out; unsigned int *out_size;
} span_job;

static void *span_run(void *arg)
{
    span_job *j = arg;
    for (int i = j->lo; i < j->hi; i++) {
        unsigned char *r = j->decode
            ? orc_rans_uncompress_to_4x16(j->in[i], j->in_size[i], j->out[i], &j->out_size[i])
            : orc_rans_compress_to_4x16(j->in[i], j->in_size[i], j->out[i], &j->out_size[i], j->order);
        if (!r) j->failed++;
    }
    return NULL;
}

static int run_many(int n, unsigned char *const *in, const unsigned int *in_size,
                    unsigned char *const *out, unsigned int *out_size, int order, int nthreads, int decode)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > n) nthreads = n > 0 ? n : 1;
    pthread_t *th = calloc(nthreads, sizeof(*th));
    span_job *jobs = calloc(nthreads, sizeof(*jobs));
    int failed = 0;
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (span_job){ (int)((long)n * t / nthreads), (int)((long)n * (t + 1) / nthreads),
                              order, decode, 0, in, in_size, out, out_size };
        if (t == nthreads - 1) span_run(&jobs[t]);
        else pthread_create(&th[t], NULL, span_run, &jobs[t]);
    }
    for (int t = 0; t < nthreads - 1; t++) pthread_join(th[t], NULL);
    for (int t = 0; t < nthreads; t++) failed += jobs[t].failed;
    free(th); free(jobs);
    return failed;
}

int orc_compress_many(int n, unsigned char *const *in, const unsigned int *in_size,
                      unsigned char *const *out, unsigned int *out_size, int order, int nthreads)
{
    return run_many(n, in, in_size, out, out_size, order, nthreads, 0);
}

int orc_uncompress_many(int n, unsigned char *const *in, const unsigned int *in_size,
                        unsigned char *const *out, unsigned int *out_size, int nthreads)
{
    return run_many(n, in, in_size, out, out_size, 0, nthreads, 1);
}
