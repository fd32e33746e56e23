// r4x16_fqz_pick.h - the parameter choice of htscodecs' quality encoder on the host: fqz_qual_stats with one_param = -1
// (fqzcomp_qual.c:418-693), fqz_pick_parameters (:757-945) with strat_opts (:199-206), store_array (:106-148) and
// fqz_store_parameters (:696-752), restated statement by statement.  The decisions are comparisons of sums of
// n * log(n / total) in doubles: the summation order and the arithmetic are the reference's (build without contraction
// of multiply-adds, as the library is).  Nothing here needs HIP: a plain C++ compiler takes it
// (rans4x16_hip_fqz_pick_parameters, the host-buffer batch, tests/host/fqz_pick_check.cpp).
//
// The result is the PARAMETER BYTES - what lies between the size varint and the range coder's bytes of a stream - and the
// slice as the reference's encode loop finds it: the lengths after the fix-ups of :806-816, the selector in
// flags[rec] >> 16.  Where the reference reads outside its arrays this restatement is defined: with no record at all it
// takes s->len[0] (:824, :836) as 0.
//
// Loops: every loop runs over the records (nrec), the bytes (in_size) or a table of fixed size.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>

enum { FQP_OK = 0, FQP_E_CAPACITY = 1, FQP_E_SIZE = 5, FQP_E_UNSUPPORTED = 6 };
enum { FQP_FREVERSE = 16, FQP_FREAD2 = 128 };
#define FQP_NP 128
#define FQP_NSTRATS 5
#define FQP_MIN(a, b) ((a) < (b) ? (a) : (b))
#define FQP_MAX(a, b) ((a) > (b) ? (a) : (b))

// store_array: array[0 .. size) of ascending values as run lengths per value, then runs of equal run lengths
static inline void fqp_store_array(std::vector<uint8_t> &out, const uint32_t *array, int size)
{
    std::vector<uint8_t> tmp;
    int i = 0;
    for (uint32_t j = 0; i < size; j++) {
        int run_len = i;
        while (i < size && array[i] == j) i++;
        run_len = i - run_len;
        int r;
        do {
            r = FQP_MIN(255, run_len);
            tmp.push_back((uint8_t)r);
            run_len -= r;
        } while (r == 255);
    }
    int last = -1;
    for (size_t j = 0; j < tmp.size();) {
        const uint8_t v = tmp[j++];
        out.push_back(v);
        if (v == last) {
            const size_t n = j;
            while (j < tmp.size() && tmp[j] == last) j++;
            out.push_back((uint8_t)(j - n));
        } else
            last = v;
    }
}

struct FqpParam {       // fqz_param's fields the pick uses
    int qbits, qshift, pbits, pshift, dbits, dshift, qloc, sloc, ploc, dloc, do_r2, do_qa;
    int do_sel, do_dedup, max_sym, nsym, store_qmap, fixed_len, use_qtab, use_ptab, use_dtab, pflags, max_sel;
};

// fqz_qual_stats(s, in, in_size, pm, qhist, -1).  flags: the working copy.
static inline void fqp_qual_stats(int nrec, const uint32_t *len, uint32_t *flags, const uint8_t *in, size_t in_size, FqpParam *pm,
                                  uint32_t *qhist)
{
    typedef uint32_t Row[256];
    std::vector<uint32_t> hist((size_t)3 * FQP_NP * 256, 0);
    Row *qhistb = (Row *)hist.data(), *qhist1 = qhistb + FQP_NP, *qhist2 = qhist1 + FQP_NP;
    uint64_t t1[FQP_NP] = {0}, t2[FQP_NP] = {0};
    std::vector<uint32_t> avg(2560, 0);
    int dir = 0, last_len = 0, do_dedup = 0, num_rec = 0;
    size_t rec, i, j;
    int max_sel = 0, has_r2 = 0;
    for (rec = 0; rec < (size_t)nrec; rec++) {
        num_rec++;
        if (max_sel < (int)(flags[rec] >> 16)) max_sel = (int)(flags[rec] >> 16);
        if (flags[rec] & FQP_FREAD2) has_r2 = 1;
    }
    std::vector<int> avg_qual((size_t)nrec + 1, 0);
    rec = i = j = 0;
    while (i < in_size) {
        if (rec < (size_t)nrec) {
            j = len[rec];
            dir = flags[rec] & FQP_FREAD2 ? 1 : 0;
            if (i > 0 && j == (size_t)last_len && !memcmp(in + i - last_len, in + i, j)) do_dedup++;
        } else {
            j = in_size - i;
            dir = 0;
        }
        last_len = (int)j;
        Row *qh = dir ? qhist2 : qhist1;
        uint64_t *th = dir ? t2 : t1;
        uint32_t tot = 0;
        for (; i < in_size && j > 0; i++, j--) {
            tot += in[i];
            qhist[in[i]]++;
            qhistb[j & (FQP_NP - 1)][in[i]]++;
            qh[j & (FQP_NP - 1)][in[i]]++;
            th[j & (FQP_NP - 1)]++;
        }
        tot = last_len ? (uint32_t)((tot * 10.0) / last_len + .5) : 0;
        if (rec <= (size_t)nrec) avg_qual[rec] = (int)tot;           // (past the last record: the remainder as one more)
        avg[FQP_MIN(2559u, tot)]++;
        rec++;
    }
    pm->do_dedup = ((rec + 1) / (size_t)(do_dedup + 1) < 500);
    last_len = 0;
    pm->max_sym = pm->nsym = 0;
    for (i = 0; i < 256; i++)
        if (qhist[i]) pm->max_sym = (int)i, pm->nsym++;

    // does the average quality help?
    if (pm->do_qa != 0) {
        const double qf0 = pm->nsym > 8 ? 0.2 : 0.05, qf1 = pm->nsym > 8 ? 0.5 : 0.22, qf2 = pm->nsym > 8 ? 0.8 : 0.60;
        int total = 0;
        i = 0;
        while (i < 2560) { total += avg[i]; if (total > qf0 * num_rec) break; avg[i++] = 0; }
        while (i < 2560) { total += avg[i]; if (total > qf1 * num_rec) break; avg[i++] = 1; }
        while (i < 2560) { total += avg[i]; if (total > qf2 * num_rec) break; avg[i++] = 2; }
        while (i < 2560) avg[i++] = 3;

        typedef int IRow[256];
        std::vector<int> bins((size_t)7 * FQP_NP * 256, 0);
        IRow *qbin4 = (IRow *)bins.data(), *qbin2 = qbin4 + 4 * FQP_NP, *qbin1 = qbin2 + 2 * FQP_NP;   // [4][NP], [2][NP], [NP]
        int qcnt4[4][FQP_NP] = {{0}}, qcnt2[4][FQP_NP] = {{0}}, qcnt1[FQP_NP] = {0};
        i = 0;
        rec = 0;
        while (i < in_size) {
            j = rec < (size_t)nrec ? len[rec] : in_size - i;
            last_len = (int)j;
            const uint32_t tot = rec <= (size_t)nrec ? (uint32_t)avg_qual[rec] : 0u;
            const int qb4 = (int)avg[FQP_MIN(2559u, tot)], qb2 = qb4 / 2;
            for (; i < in_size && j > 0; i++, j--) {
                const int x = (int)(j & (FQP_NP - 1));
                qbin4[qb4 * FQP_NP + x][in[i]]++; qcnt4[qb4][x]++;
                qbin2[qb2 * FQP_NP + x][in[i]]++; qcnt2[qb2][x]++;
                qbin1[x][in[i]]++;                qcnt1[x]++;
            }
            rec++;
        }
        double e1 = 0, e2 = 0, e4 = 0;
        for (j = 0; j < FQP_NP; j++)
            for (i = 0; i < 256; i++) {
                if (qbin1[j][i]) e1 += qbin1[j][i] * log(qbin1[j][i] / (double)qcnt1[j]);
                for (int b = 0; b < 2; b++) { const int v = qbin2[b * FQP_NP + j][i]; if (v) e2 += v * log(v / (double)qcnt2[b][j]); }
                for (int b = 0; b < 4; b++) { const int v = qbin4[b * FQP_NP + j][i]; if (v) e4 += v * log(v / (double)qcnt4[b][j]); }
            }
        e1 /= -log(2) / 8;
        e2 /= -log(2) / 8;
        e4 /= -log(2) / 8;
        const double qm = pm->do_qa > 0 ? 1 : 0.98;
        if ((pm->do_qa == -1 || pm->do_qa >= 4) && e4 + nrec / 4 < e2 * qm + nrec / 8 && e4 + nrec / 4 < e1 * qm) {
            for (i = 0; i < (size_t)nrec; i++) flags[i] |= avg[FQP_MIN(2559, avg_qual[i])] << 16;
            pm->do_sel = 1;
            max_sel = 3;
        } else if ((pm->do_qa == -1 || pm->do_qa >= 2) && e2 + nrec / 8 < e1 * qm) {
            for (i = 0; i < (size_t)nrec; i++) flags[i] |= (avg[FQP_MIN(2559, avg_qual[i])] >> 1) << 16;
            pm->do_sel = 1;
            max_sel = 1;
        }
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

    // does splitting READ1 from READ2 help?
    if (has_r2 || pm->do_r2) {
        double e1 = 0, e2 = 0;
        for (j = 0; j < FQP_NP; j++) {
            if (!t1[j] || !t2[j]) continue;
            for (i = 0; i < 256; i++) {
                if (!qhistb[j][i]) continue;
                e1 -= (qhistb[j][i]) * log(qhistb[j][i] / (double)(t1[j] + t2[j]));
                if (qhist1[j][i]) e2 -= qhist1[j][i] * log(qhist1[j][i] / (double)t1[j]);
                if (qhist2[j][i]) e2 -= qhist2[j][i] * log(qhist2[j][i] / (double)t2[j]);
            }
        }
        e1 /= log(2) * 8;
        e2 /= log(2) * 8;
        const double qm = pm->do_r2 > 0 ? 1 : 0.95;
        if (e2 + (8 + nrec / 8) < e1 * qm) {
            for (rec = 0; rec < (size_t)nrec; rec++) {
                const uint32_t sel = flags[rec] >> 16;
                flags[rec] = (flags[rec] & 0xffff) | ((flags[rec] & FQP_FREAD2) ? ((sel * 2) + 1) << 16 : ((sel * 2) + 0) << 16);
                if (max_sel < (int)(flags[rec] >> 16)) max_sel = (int)(flags[rec] >> 16);
            }
        }
    }
    if (max_sel > 0) {
        pm->do_sel = 1;
        pm->max_sel = max_sel;
    }
}

// pshift where the strategy leaves it to the first record's length (:840-841)
static inline int fqp_pshift(uint32_t first_len, int pbits)
{
    const double v = log((double)first_len / (1 << pbits)) / log(2) + .5;
    return (int)(0 > v ? 0 : v);
}

// fqz_pick_parameters + fqz_store_parameters.  len and flags are the caller's and are only read: L and F take the slice as
// the reference leaves it (on success), out the parameter bytes.
static inline int fqp_pick(int vers, int strat, int nrec, const uint32_t *len, const uint32_t *flags, const uint8_t *in, size_t in_size,
                           std::vector<uint8_t> &out, std::vector<uint32_t> &L, std::vector<uint32_t> &F)
{
    static const int strat_opts[FQP_NSTRATS][12] = {
        {10, 5, 4, -1, 2, 1, 0, 14, 10, 14, 0, -1},
        {8, 5, 7, 0, 0, 0, 0, 14, 8, 14, 1, -1},
        {12, 6, 2, 0, 2, 3, 0, 9, 12, 14, 0, 0},
        {12, 6, 0, 0, 0, 0, 0, 12, 0, 0, 0, 0},
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    };
    int dsqr[64] = {0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5,
                    5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7};
    if (strat < 0 || nrec < 0 || (nrec && (!len || !flags)) || (in_size && !in)) return FQP_E_UNSUPPORTED;
    if (in_size >= 0x80000000ull) return FQP_E_UNSUPPORTED;
    if (strat >= FQP_NSTRATS) strat = FQP_NSTRATS - 1;
    uint32_t qhist[256] = {0};
    int gflags = 0;
    if (vers == 3) gflags |= 4;                                      // GFLAG_DO_REV
    FqpParam P;
    memset(&P, 0, sizeof(P));
    FqpParam *pm = &P;
    pm->qbits = strat_opts[strat][0]; pm->qshift = strat_opts[strat][1];
    pm->pbits = strat_opts[strat][2]; pm->pshift = strat_opts[strat][3];
    pm->dbits = strat_opts[strat][4]; pm->dshift = strat_opts[strat][5];
    pm->qloc = strat_opts[strat][6]; pm->sloc = strat_opts[strat][7];
    pm->ploc = strat_opts[strat][8]; pm->dloc = strat_opts[strat][9];
    pm->do_r2 = strat_opts[strat][10]; pm->do_qa = strat_opts[strat][11];

    // the length fix-ups (:806-816), on the copies
    L.assign(len, len + nrec);
    F.assign(flags, flags + nrec);
    size_t tlen = 0, i;
    for (i = 0; i < (size_t)nrec; i++) {
        if (tlen + L[i] > in_size) L[i] = (uint32_t)(in_size - tlen);
        tlen += L[i];
    }
    if (nrec > 0 && tlen < in_size) L[nrec - 1] += (uint32_t)(in_size - tlen);

    fqp_qual_stats(nrec, L.data(), F.data(), in, in_size, pm, qhist);
    pm->store_qmap = (pm->nsym <= 8 && pm->nsym * 2 < pm->max_sym);
    const uint32_t first_len = nrec ? L[0] : 0u;
    for (i = 1; i < (size_t)nrec; i++)
        if (L[i] != first_len) break;
    pm->fixed_len = (i == (size_t)nrec);                             // (no record at all: 1 != 0, not fixed)
    pm->use_qtab = 0;
    if (strat < FQP_NSTRATS - 1) {
        if (pm->pshift < 0) pm->pshift = fqp_pshift(first_len, pm->pbits);
        if (pm->nsym <= 4) {
            pm->qshift = 2;
            if (in_size < 5000000) { pm->pbits = 2; pm->pshift = 5; }
        } else if (pm->nsym <= 8) {
            pm->qbits = FQP_MIN(pm->qbits, 9);
            pm->qshift = 3;
            if (in_size < 5000000) pm->qbits = 6;
        }
        if (in_size < 300000) { pm->qbits = pm->qshift; pm->dbits = 2; }
    }
    for (i = 0; i < 64; i++)
        if (dsqr[i] > (1 << pm->dbits) - 1) dsqr[i] = (1 << pm->dbits) - 1;
    uint32_t ptab[1024], dtab[256];
    if (pm->store_qmap) pm->max_sym = pm->nsym;
    else pm->nsym = 255;
    if (pm->pbits)
        for (i = 0; i < 1024; i++) ptab[i] = (uint32_t)FQP_MIN((1 << pm->pbits) - 1, (int)(i >> pm->pshift));
    if (pm->dbits)
        for (i = 0; i < 256; i++) dtab[i] = (uint32_t)dsqr[FQP_MIN((size_t)63, i >> pm->dshift)];
    pm->use_ptab = (pm->pbits > 0);
    pm->use_dtab = (pm->dbits > 0);
    pm->pflags = (pm->use_qtab ? 128 : 0) | (pm->use_dtab ? 64 : 0) | (pm->use_ptab ? 32 : 0) | (pm->do_sel ? 8 : 0) |
                 (pm->fixed_len ? 4 : 0) | (pm->do_dedup ? 2 : 0) | (pm->store_qmap ? 16 : 0);
    int g_max_sel = 0;
    if (pm->do_sel) {
        gflags |= 2;                                                 // GFLAG_HAVE_STAB: two selector values and more, one parameter block
        for (i = 0; i < (size_t)nrec; i++)
            if (g_max_sel < (int)(F[i] >> 16)) g_max_sel = (int)(F[i] >> 16);
    }

    // fqz_store_parameters
    out.clear();
    out.push_back(5);                                                // FQZ_VERS
    out.push_back((uint8_t)gflags);
    if (gflags & 2) {
        const uint32_t stab[256] = {0};
        out.push_back((uint8_t)g_max_sel);
        fqp_store_array(out, stab, 256);
    }
    out.push_back(0); out.push_back(0);                              // the starting context
    out.push_back((uint8_t)pm->pflags);
    out.push_back((uint8_t)pm->max_sym);
    out.push_back((uint8_t)((pm->qbits << 4) | pm->qshift));
    out.push_back((uint8_t)((pm->qloc << 4) | pm->sloc));
    out.push_back((uint8_t)((pm->ploc << 4) | pm->dloc));
    if (pm->store_qmap)
        for (i = 0; i < 256; i++)
            if (qhist[i]) out.push_back((uint8_t)i);
    if (pm->pbits && pm->use_ptab) fqp_store_array(out, ptab, 1024);
    if (pm->dbits && pm->use_dtab) fqp_store_array(out, dtab, 256);
    return FQP_OK;
}
