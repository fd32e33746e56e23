// r4x16_fqz_pick_dec.h - what the parameter choice of fqz_compress does once the statistics are counted: the decisions of
// fqz_qual_stats(.., -1) (fqzcomp_qual.c:560-690) on the entropy sums, fqz_pick_parameters' rules (:818-905), store_array
// (:106-148) and fqz_store_parameters (:696-752), written once for the host and the device.  r4x16_fqz_pick.h is the
// statement-by-statement restatement that the reference's streams pin; this is the same choice taken from the MARGINAL
// SUMS of the joint histogram J[dir][bin][x][q], as the kernels of r4x16_fqz_pick.hip count them and as
// tests/host/fqz_pick_dev_check.cpp counts them on the CPU.  No HIP type, no container, no local array: a plain C++
// compiler takes it, and hipcc compiles it for gfx950 without scratch memory.
//
// The exactness rule: a comparison of entropy sums is taken only where its two sides differ by more than a
// guard that bounds the host's error plus the device's; otherwise the answer is FQD_UNDECIDED and nothing is chosen.
// A comparison whose terms are all exact zeros has a guard of 0 and is exact.
//
// Loops: over tables of fixed size (2,560, 1,024, 256, 64 entries) and, in store_array, over the values of an ascending
// table (at most its size).
#pragma once
#include <stdint.h>
#include <math.h>

#ifndef FQD_HD
#if defined(__HIPCC__)
#define FQD_HD __host__ __device__ inline
#else
#define FQD_HD inline
#endif
#endif

enum { FQD_OK = 0, FQD_UNDECIDED = 10 };
enum { FQD_FREAD2 = 128, FQD_NP = 128, FQD_AVG = 2560, FQD_NSTRATS = 5 };
#define FQD_LN2 0.6931471805599453          // log(2) as a double
#define FQD_GUARD 9.5367431640625e-07       // 2^-20: of the sum of a comparison's |terms|
#define FQD_PSHIFT_EXACT_BELOW (1u << 22)   // first_len below this: the reference's double arithmetic and the integer rule agree

struct FqdParam {       // fqz_param's fields the pick uses
    int qbits, qshift, pbits, pshift, dbits, dshift, qloc, sloc, ploc, dloc, do_r2, do_qa;
    int do_sel, do_dedup, max_sym, nsym, store_qmap, fixed_len, use_ptab, use_dtab, pflags;
    int gflags;
};
// What the record pass and the byte pass know of a slice (after the length fix-ups)
struct FqdStats {
    int nrec;                   // the caller's records: num_rec
    uint32_t in_size;
    uint32_t first_len;         // L[0], or 0 without a record
    int fixed_len;              // every record as long as the first (no record at all: 0)
    int has_r2;                 // a READ2 flag in any record
    int caller_max_sel;         // the largest flags[rec] >> 16 as the caller left them
    uint32_t visited;           // `rec` when the loop over the bytes ends
    uint32_t dups;              // records equal to the visited record before them
    int nsym, max_sym;          // qualities that occur, the largest
};
// The sums of v * log(v / (double)c) of the two questions (each <= 0) and, beside each, the sum of |v * log(v / c)|
struct FqdSums {
    double e1, a1, e2, a2, e4, a4;      // average-quality bins: none, two, four
    double r1, ra1, r2, ra2;            // READ1 with READ2, and apart
};
struct FqdChoice { int way; int split; };       // way: 0, 2 or 4 average-quality bins as selectors; split: READ2 doubles the selector

FQD_HD void fqd_strat(int strat, FqdParam *pm)
{
    const int opts[FQD_NSTRATS][12] = {
        {10, 5, 4, -1, 2, 1, 0, 14, 10, 14, 0, -1},
        {8, 5, 7, 0, 0, 0, 0, 14, 8, 14, 1, -1},
        {12, 6, 2, 0, 2, 3, 0, 9, 12, 14, 0, 0},
        {12, 6, 0, 0, 0, 0, 0, 12, 0, 0, 0, 0},
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    };
    if (strat >= FQD_NSTRATS) strat = FQD_NSTRATS - 1;
    const int *o = opts[strat];
    pm->qbits = o[0]; pm->qshift = o[1]; pm->pbits = o[2]; pm->pshift = o[3]; pm->dbits = o[4]; pm->dshift = o[5];
    pm->qloc = o[6]; pm->sloc = o[7]; pm->ploc = o[8]; pm->dloc = o[9]; pm->do_r2 = o[10]; pm->do_qa = o[11];
    pm->do_sel = pm->do_dedup = pm->max_sym = pm->nsym = pm->store_qmap = pm->fixed_len = pm->use_ptab = pm->use_dtab = pm->pflags = 0;
    pm->gflags = 0;
}

// one term of an entropy sum: v of c, 0 < v <= c
FQD_HD double fqd_term(uint32_t v, uint64_t c) { return v * log(v / (double)c); }

// The average-quality thresholds (:567-580), in place: avg[0 .. 2560) holds the counts and gets the bins.  Each loop adds
// avg[i] again after the break of the loop before it, as the reference does.
FQD_HD void fqd_thresholds(uint32_t *avg, int num_rec, int nsym)
{
    const double qf0 = nsym > 8 ? 0.2 : 0.05, qf1 = nsym > 8 ? 0.5 : 0.22, qf2 = nsym > 8 ? 0.8 : 0.60;
    int total = 0, i = 0;
    while (i < FQD_AVG) { total += (int)avg[i]; if (total > qf0 * num_rec) break; avg[i++] = 0; }
    while (i < FQD_AVG) { total += (int)avg[i]; if (total > qf1 * num_rec) break; avg[i++] = 1; }
    while (i < FQD_AVG) { total += (int)avg[i]; if (total > qf2 * num_rec) break; avg[i++] = 2; }
    while (i < FQD_AVG) avg[i++] = 3;
}

// lhs < rhs, where lhs and rhs carry errors of at most `guard` together.  1 / 0, or -1: too close to call.
FQD_HD int fqd_less(double lhs, double rhs, double guard)
{
    const double d = lhs - rhs;
    if (guard > 0 && (d < 0 ? -d : d) <= guard) return -1;
    return lhs < rhs;
}

// The decisions of fqz_qual_stats on the sums: do_dedup, the average-quality selectors with the bit shuffle, the READ
// split.  guard_bits scales the guard by 2^guard_bits.  FQD_OK, or FQD_UNDECIDED with *pm and *ch of no meaning.
FQD_HD int fqd_decide(FqdParam *pm, const FqdStats *st, const FqdSums *s, int guard_bits, FqdChoice *ch)
{
    const double unit = FQD_LN2 / 8, g = ldexp(FQD_GUARD, guard_bits) / unit;
    const int nrec = st->nrec;
    ch->way = 0; ch->split = 0;
    pm->do_dedup = (((uint64_t)st->visited + 1) / ((uint64_t)st->dups + 1) < 500);
    pm->max_sym = st->max_sym; pm->nsym = st->nsym;
    if (pm->do_qa != 0) {
        const double e1 = s->e1 / -unit, e2 = s->e2 / -unit, e4 = s->e4 / -unit;
        const double qm = pm->do_qa > 0 ? 1 : 0.98;
        int four = 0, two = 0;
        if (pm->do_qa == -1 || pm->do_qa >= 4) {
            four = fqd_less(e4 + nrec / 4, e2 * qm + nrec / 8, g * (s->a4 + s->a2));
            if (four < 0) return FQD_UNDECIDED;
            if (four) {
                four = fqd_less(e4 + nrec / 4, e1 * qm, g * (s->a4 + s->a1));
                if (four < 0) return FQD_UNDECIDED;
            }
        }
        if (!four && (pm->do_qa == -1 || pm->do_qa >= 2)) {
            two = fqd_less(e2 + nrec / 8, e1 * qm, g * (s->a2 + s->a1));
            if (two < 0) return FQD_UNDECIDED;
        }
        ch->way = four ? 4 : two ? 2 : 0;
        if (ch->way) pm->do_sel = 1;
        if (pm->do_qa == -1) {
            if (pm->pbits > 0 && pm->dbits > 0) {
                pm->sloc = pm->dloc - 1;
                pm->pbits--;
                pm->dbits--;
                pm->dloc++;
            } else if (pm->dbits >= 2) {
                pm->sloc = pm->dloc;
                pm->dbits -= 2;
                pm->dloc += 2;
            } else if (pm->qbits >= 2) {
                pm->qbits -= 2;
                pm->ploc -= 2;
                pm->sloc = 16 - 2 - pm->do_r2;
                if (pm->qbits == 6 && pm->qshift == 5) pm->qbits--;
            }
            pm->do_qa = 4;
        }
    }
    if (st->has_r2 || pm->do_r2) {
        const double e1 = -s->r1 / (FQD_LN2 * 8), e2 = -s->r2 / (FQD_LN2 * 8);
        const double qm = pm->do_r2 > 0 ? 1 : 0.95;
        const int split = fqd_less(e2 + (8 + nrec / 8), e1 * qm, ldexp(FQD_GUARD, guard_bits) / (FQD_LN2 * 8) * (s->ra2 + s->ra1));
        if (split < 0) return FQD_UNDECIDED;
        ch->split = split;
    }
    return FQD_OK;
}

// The selector of a record as the choice leaves it in flags[rec]: bin is the record's average-quality bin 0..3
FQD_HD uint32_t fqd_flags(uint32_t flags, uint32_t bin, const FqdChoice *ch)
{
    if (ch->way == 4) flags |= bin << 16;
    else if (ch->way == 2) flags |= (bin >> 1) << 16;
    if (ch->split) {
        const uint32_t sel = flags >> 16;
        flags = (flags & 0xffff) | ((flags & FQD_FREAD2) ? ((sel * 2) + 1) << 16 : ((sel * 2) + 0) << 16);
    }
    return flags;
}

// floor(log2(first_len / 2^pbits) + .5), at least 0, in integers: k is the largest with 2^(2k-1) <= r^2.  first_len < 2^32.
FQD_HD int fqd_pshift(uint32_t first_len, int pbits)
{
    const uint64_t sq = (uint64_t)first_len * first_len;
    int k = 0;
    while (2 * (k + 1) - 1 + 2 * pbits < 64 && sq >= ((uint64_t)1 << (2 * (k + 1) - 1 + 2 * pbits))) k++;
    return k;
}

FQD_HD int fqd_dsqr(int i) { return (i >= 1) + (i >= 4) + (i >= 9) + (i >= 16) + (i >= 25) + (i >= 36) + (i >= 49); }
struct FqdZero { FQD_HD uint32_t operator()(int) const { return 0u; } };
struct FqdPtab {
    int pbits, pshift;
    FQD_HD uint32_t operator()(int i) const { const int top = (1 << pbits) - 1, v = i >> pshift; return (uint32_t)(top < v ? top : v); }
};
struct FqdDtab {
    int dbits, dshift;
    FQD_HD uint32_t operator()(int i) const
    {
        const int top = (1 << dbits) - 1, k = i >> dshift, d = fqd_dsqr(k < 63 ? k : 63);
        return (uint32_t)(d > top ? top : d);
    }
};
// where the parameter bytes go: the bytes up to cap are written, all are counted
struct FqdSink {
    uint8_t *p; uint32_t cap, n;
    FQD_HD void put(uint32_t v) { if (n < cap) p[n] = (uint8_t)v; n++; }
};
// store_array without its temporary: the run lengths go through the second stage one by one
struct FqdRuns {
    int last, counting; uint32_t cnt;
    FQD_HD void feed(FqdSink *out, int v)
    {
        if (counting) {
            if (v == last) { cnt++; return; }
            out->put(cnt);
            counting = 0;
        }
        out->put((uint32_t)v);
        if (v == last) { counting = 1; cnt = 0; }
        else last = v;
    }
    FQD_HD void end(FqdSink *out) { if (counting) out->put(cnt); }
};
template <class V>
FQD_HD void fqd_store_array(FqdSink *out, int size, const V &val)
{
    FqdRuns runs = {-1, 0, 0u};
    int i = 0;
    for (uint32_t j = 0; i < size; j++) {
        int run_len = i;
        while (i < size && val(i) == j) i++;
        run_len = i - run_len;
        int r;
        do {
            r = run_len < 255 ? run_len : 255;
            runs.feed(out, r);
            run_len -= r;
        } while (r == 255);
    }
    runs.end(out);
}

// fqz_pick_parameters behind the statistics, and fqz_store_parameters.  strat: as the caller gave it (>= 0).  final_max:
// the largest selector in the flags as fqd_flags leaves them.  qmask: bit q of word q / 32 set where quality q occurs.
// FQD_OK with the bytes in *out (out->n: their number, written up to out->cap), or FQD_UNDECIDED.
FQD_HD int fqd_store(FqdParam *pm, const FqdStats *st, const FqdChoice *ch, int vers, int strat, uint32_t final_max, const uint32_t *qmask, FqdSink *out)
{
    if (strat >= FQD_NSTRATS) strat = FQD_NSTRATS - 1;
    if (vers == 3) pm->gflags |= 4;
    // max_sel > 0 (:686-689): the caller's, 3 or 1 where the bins became selectors, the flags' largest after the split
    const uint32_t prev = ch->way == 4 ? 3u : ch->way == 2 ? 1u : (uint32_t)st->caller_max_sel;
    if (prev > 0 || (ch->split && final_max > 0)) pm->do_sel = 1;
    pm->store_qmap = (pm->nsym <= 8 && pm->nsym * 2 < pm->max_sym);
    pm->fixed_len = st->fixed_len;
    const uint32_t in_size = st->in_size;
    if (strat < FQD_NSTRATS - 1) {
        if (pm->pshift < 0) {
            if (st->first_len >= FQD_PSHIFT_EXACT_BELOW) return FQD_UNDECIDED;
            pm->pshift = fqd_pshift(st->first_len, pm->pbits);
        }
        if (pm->nsym <= 4) {
            pm->qshift = 2;
            if (in_size < 5000000) { pm->pbits = 2; pm->pshift = 5; }
        } else if (pm->nsym <= 8) {
            pm->qbits = pm->qbits < 9 ? pm->qbits : 9;
            pm->qshift = 3;
            if (in_size < 5000000) pm->qbits = 6;
        }
        if (in_size < 300000) { pm->qbits = pm->qshift; pm->dbits = 2; }
    }
    if (pm->store_qmap) pm->max_sym = pm->nsym;
    else pm->nsym = 255;
    pm->use_ptab = (pm->pbits > 0);
    pm->use_dtab = (pm->dbits > 0);
    pm->pflags = (pm->use_dtab ? 64 : 0) | (pm->use_ptab ? 32 : 0) | (pm->do_sel ? 8 : 0) | (pm->fixed_len ? 4 : 0) | (pm->do_dedup ? 2 : 0) |
                 (pm->store_qmap ? 16 : 0);
    if (pm->do_sel) pm->gflags |= 2;                                 // GFLAG_HAVE_STAB

    out->put(5);                                                     // FQZ_VERS
    out->put((uint32_t)pm->gflags);
    if (pm->gflags & 2) {
        out->put(final_max);
        fqd_store_array(out, 256, FqdZero());
    }
    out->put(0); out->put(0);                                        // the starting context
    out->put((uint32_t)pm->pflags);
    out->put((uint32_t)pm->max_sym);
    out->put((uint32_t)((pm->qbits << 4) | pm->qshift));
    out->put((uint32_t)((pm->qloc << 4) | pm->sloc));
    out->put((uint32_t)((pm->ploc << 4) | pm->dloc));
    if (pm->store_qmap)
        for (uint32_t q = 0; q < 256; q++)
            if (qmask[q >> 5] >> (q & 31) & 1u) out->put(q);
    if (pm->use_ptab) { const FqdPtab t = {pm->pbits, pm->pshift}; fqd_store_array(out, 1024, t); }
    if (pm->use_dtab) { const FqdDtab t = {pm->dbits, pm->dshift}; fqd_store_array(out, 256, t); }
    return FQD_OK;
}

// A bound on the bytes fqd_store writes.  store_array of `size` ascending values below `size`: its first
// stage makes one run-length byte per value up to the largest and one more per 255 of a run, at most
// size + size / 255 + 1 bytes; its second stage writes each of them or a count in its place, and a count only behind
// a byte it wrote: at most twice as many.  The rest: version and gflags, max_sel and the selector table (256 zeros), the
// starting context, five parameter bytes, a qmap of at most 8, ptab (1,024 values) and dtab (256).
FQD_HD uint32_t fqd_array_cap(uint32_t size) { return 2u * (size + size / 255u + 1u) + 2u; }
FQD_HD uint32_t fqd_cap() { return 2u + 1u + fqd_array_cap(256) + 2u + 5u + 8u + fqd_array_cap(1024) + fqd_array_cap(256); }
