// fqz_best_check.cpp - the arithmetic of the best-of-several calls' shared statistics on the host, alone
// (htscodecs_amd/csrc/r4x16_fqz_best.hip): ONE joint histogram J[dir][bin][x][q] a slice, counted on the CPU the way the
// kernels of r4x16_fqz_pick.hip count it - with the average-quality bins computed where ANY candidate of the list asks for
// them -, its marginal sums taken once, and then per candidate the very decision and store code the kernel runs
// (r4x16_fqz_pick_dec.h).  Every candidate must come out as the host pick of its strategy alone (r4x16_fqz_pick.h:
// fqp_pick): status, parameter bytes, lengths, flags.  Built with g++ and -fsanitize=address,undefined, run as a program
// of its own (tests/test_fqz_best_cpu.py).
//
// Input (argv[1]): cases in fqz_pick_check.cpp's layout (the strategy word is not used).  Every case runs under the lists
// [0,1,2,3], [2,0], [3,1] and [4,0].
// Output: one line a case and list, "case list-index statuses-of-the-candidates bins-computed need-J", then
// "fqz_best_check: ok <cases> <candidates>"; any disagreement prints FAILED and exits 1.
#include "r4x16_fqz_pick.h"
#include "r4x16_fqz_pick_dec.h"

#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

// What the statistics pass leaves of a slice: everything the candidates read
struct Shared {
    FqdStats fs;
    FqdSums sm;
    uint32_t qmask[8];
    std::vector<uint32_t> wlen, cls;
    bool bins, need_j;
};

static void shared_stats(const std::vector<int> &list, int nrec, const uint32_t *len, const uint32_t *flags, const uint8_t *in, uint32_t size,
                         Shared *sh)
{
    // k_fqp_lens
    const uint32_t nw = nrec ? (uint32_t)nrec : size ? 1u : 0u;
    std::vector<uint32_t> wstart(nw + 1, 0), wavg(nw + 1, 0);
    sh->wlen.assign(nw + 1, 0); sh->cls.assign(nw + 1, 0);
    std::vector<uint32_t> &wlen = sh->wlen;
    FqdStats &fs = sh->fs;
    memset(&fs, 0, sizeof(fs));
    fs.nrec = nrec; fs.in_size = size; fs.fixed_len = nrec != 0; fs.visited = nrec || !size ? 0u : 1u;
    if (!nrec && size) wlen[0] = size;
    uint64_t pre = 0;
    for (int r = 0; r < nrec; r++) {
        const uint64_t start = pre;
        pre = std::min<uint64_t>(pre + std::min(len[r], size), size);
        if (r == nrec - 1) pre = size;
        wstart[r] = (uint32_t)start; wlen[r] = (uint32_t)(pre - start);
        if (flags[r] & FQD_FREAD2) fs.has_r2 = 1;
        fs.caller_max_sel = std::max(fs.caller_max_sel, (int)(flags[r] >> 16));
        if (start < size) fs.visited++;
    }
    if (nrec) fs.first_len = wlen[0];
    for (int r = 0; r < nrec; r++) if (wlen[r] != fs.first_len) fs.fixed_len = 0;
    // k_fqp_recs
    std::vector<uint32_t> avg(FQD_AVG, 0);
    memset(sh->qmask, 0, sizeof(sh->qmask));
    for (uint32_t r = 0; r < nw; r++) {
        const uint32_t l = wlen[r], s = wstart[r];
        if (s >= size) continue;
        bool dup = s > 0 && l == wlen[r - 1];
        uint32_t tot = 0;
        for (uint32_t t = 0; t < l; t++) {
            const uint32_t q = in[s + t];
            tot += q; sh->qmask[q >> 5] |= 1u << (q & 31);
            if (dup && in[s - l + t] != q) dup = false;
        }
        const uint32_t q10 = l ? (uint32_t)((tot * 10.0) / (int)l + .5) : 0u;
        avg[std::min<uint32_t>(q10, FQD_AVG - 1)]++;
        wavg[r] = q10;
        fs.dups += dup;
    }
    // k_fqp_bins: the bins where any candidate asks the average-quality question, J where any asks either question
    for (uint32_t q = 0; q < 256; q++) if (sh->qmask[q >> 5] >> (q & 31) & 1) { fs.nsym++; fs.max_sym = (int)q; }
    bool any_qa = false, any_r2 = false;
    for (int strat : list) {
        FqdParam pm;
        fqd_strat(strat, &pm);
        any_qa |= pm.do_qa != 0; any_r2 |= pm.do_r2 != 0;
    }
    sh->bins = any_qa;
    sh->need_j = any_qa || fs.has_r2 || any_r2;
    if (any_qa) fqd_thresholds(avg.data(), nrec, fs.nsym);
    for (uint32_t r = 0; r < nw; r++)
        sh->cls[r] = (nrec && (flags[r] & FQD_FREAD2) ? 4u : 0u) + (any_qa ? avg[std::min<uint32_t>(wavg[r], FQD_AVG - 1)] : 0u);
    // k_fqp_count, k_fqp_sums: the sums in table order
    FqdSums &sm = sh->sm;
    sm = FqdSums{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!sh->need_j) return;
    std::vector<uint32_t> J((size_t)8 * FQD_NP * 256, 0);
    for (uint32_t r = 0; r < nw; r++)
        if (wstart[r] < size)
            for (uint32_t t = 0; t < wlen[r]; t++) J[((size_t)sh->cls[r] * FQD_NP + ((wlen[r] - t) & (FQD_NP - 1))) * 256 + in[wstart[r] + t]]++;
    for (uint32_t x = 0; x < FQD_NP; x++) {
        uint32_t cnt[8] = {0};
        for (uint32_t c = 0; c < 8; c++) for (uint32_t q = 0; q < 256; q++) cnt[c] += J[((size_t)c * FQD_NP + x) * 256 + q];
        uint32_t c4[4];
        for (uint32_t c = 0; c < 4; c++) c4[c] = cnt[c] + cnt[c + 4];
        const uint32_t c20 = c4[0] + c4[1], c21 = c4[2] + c4[3], c1 = c20 + c21, t1 = cnt[0] + cnt[1] + cnt[2] + cnt[3], t2 = c1 - t1;
        for (uint32_t q = 0; q < 256; q++) {
            uint32_t v[8], v4[4];
            for (uint32_t c = 0; c < 8; c++) v[c] = J[((size_t)c * FQD_NP + x) * 256 + q];
            for (uint32_t c = 0; c < 4; c++) { v4[c] = v[c] + v[c + 4]; if (v4[c]) sm.e4 += fqd_term(v4[c], c4[c]); }
            const uint32_t v20 = v4[0] + v4[1], v21 = v4[2] + v4[3], v1 = v20 + v21, h1 = v[0] + v[1] + v[2] + v[3], h2 = v1 - h1;
            if (v20) sm.e2 += fqd_term(v20, c20);
            if (v21) sm.e2 += fqd_term(v21, c21);
            if (v1) sm.e1 += fqd_term(v1, c1);
            if (t1 && t2 && v1) {
                sm.r1 += fqd_term(v1, (uint64_t)t1 + t2);
                if (h1) sm.r2 += fqd_term(h1, t1);
                if (h2) sm.r2 += fqd_term(h2, t2);
            }
        }
    }
    sm.a1 = -sm.e1; sm.a2 = -sm.e2; sm.a4 = -sm.e4; sm.ra1 = -sm.r1; sm.ra2 = -sm.r2;
}

// k_fqb_store: one candidate's decisions and store from the shared statistics
static int candidate(const Shared &sh, int vers, int strat, int nrec, const uint32_t *flags, std::vector<uint8_t> &out, std::vector<uint32_t> &F)
{
    FqdParam pm;
    FqdChoice ch;
    FqdStats fs = sh.fs;
    fqd_strat(strat, &pm);
    int st = fqd_decide(&pm, &fs, &sh.sm, 0, &ch);
    if (st != FQD_OK) return st;
    F.resize(nrec);
    uint32_t fmax = 0;
    for (int r = 0; r < nrec; r++) { F[r] = fqd_flags(flags[r], sh.cls[r] & 3u, &ch); fmax = std::max(fmax, F[r] >> 16); }
    out.assign(fqd_cap(), 0);
    FqdSink sink = {out.data(), (uint32_t)out.size(), 0u};
    st = fqd_store(&pm, &fs, &ch, vers, strat, fmax, sh.qmask, &sink);
    if (st != FQD_OK) return st;
    if (sink.n > out.size()) { printf("FAILED: %u parameter bytes, above fqd_cap() = %zu\n", sink.n, out.size()); exit(1); }
    out.resize(sink.n);
    return FQD_OK;
}

static size_t cases = 0, candidates = 0;
static void one_case(int vers, const std::vector<uint32_t> &len, const std::vector<uint32_t> &flags, const std::vector<uint8_t> &in)
{
    static const std::vector<std::vector<int>> lists = {{0, 1, 2, 3}, {2, 0}, {3, 1}, {4, 0}};
    const int nrec = (int)len.size();
    // heap copies of exactly each array's size: a read beyond one stops the program
    uint32_t *l = (uint32_t *)malloc(len.size() * 4 + 1), *f = (uint32_t *)malloc(len.size() * 4 + 1);
    uint8_t *b = (uint8_t *)malloc(in.size() + 1);
    if (nrec) { memcpy(l, len.data(), len.size() * 4); memcpy(f, flags.data(), len.size() * 4); }
    if (in.size()) memcpy(b, in.data(), in.size());
    for (size_t k = 0; k < lists.size(); k++) {
        Shared sh;
        shared_stats(lists[k], nrec, l, f, b, (uint32_t)in.size(), &sh);
        printf("%zu %zu", cases, k);
        for (int strat : lists[k]) {
            std::vector<uint8_t> want, got;
            std::vector<uint32_t> L, F, F2;
            const int hst = fqp_pick(vers, strat, nrec, l, f, b, in.size(), want, L, F);
            const int st = candidate(sh, vers, strat, nrec, f, got, F2);
            if (hst != FQP_OK || st != FQD_OK) { printf("\nFAILED: case %zu list %zu strategy %d: host status %d, shared status %d\n", cases, k, strat, hst, st); exit(1); }
            if (got != want || F2 != F || !std::equal(L.begin(), L.end(), sh.wlen.begin())) {
                printf("\nFAILED: case %zu list %zu strategy %d differs from the host pick (%zu / %zu parameter bytes)\n", cases, k, strat, got.size(), want.size());
                exit(1);
            }
            printf(" %d", st);
            candidates++;
        }
        printf(" %d %d\n", (int)sh.bins, (int)sh.need_j);
    }
    free(l); free(f); free(b);
    cases++;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: fqz_best_check CASES\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5];
    while (fread(head, 4, 5, fp) == 5) {
        const uint32_t nrec = head[2], size = head[3];
        std::vector<uint32_t> len(nrec), flags(nrec);
        std::vector<uint8_t> in(size);
        if ((nrec && (fread(len.data(), 4, nrec, fp) != nrec || fread(flags.data(), 4, nrec, fp) != nrec)) ||
            (size && fread(in.data(), 1, size, fp) != size)) { printf("FAILED: short case file\n"); return 1; }
        one_case((int)head[0], len, flags, in);
    }
    fclose(fp);
    printf("fqz_best_check: ok %zu %zu\n", cases, candidates);
    return 0;
}
