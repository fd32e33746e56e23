// fqz_pick_dev_check.cpp - the device pick's arithmetic on the host, alone: the joint histogram J[dir][bin][x][q] counted
// on the CPU the way the kernels of htscodecs_amd/csrc/r4x16_fqz_pick.hip count it (the clamped prefix sum of the
// lengths, a record's tot and duplicate test, the thresholds, one count a byte, the marginal sums), then the very
// decision and store code the kernel runs (r4x16_fqz_pick_dec.h), against the host pick (r4x16_fqz_pick.h: fqp_pick).
// Built with g++ and -fsanitize=address,undefined, run as a program of its own (tests/test_fqz_pick_dev_cpu.py).
//
// Input (argv[1]): cases in fqz_pick_check.cpp's layout; the fifth word is 1 where the case must be decided at the
// default guard (the reference-made inputs), else 0.  argv[2]: how many seeded random slices follow them.  Behind those
// come the pshift cases: a first record on either side of every 2^(k + .5) * 2^pbits below the proven limit.
// Per case three picks from J:
//   plain      the sums in table order with the library's log, guard_bits 0: decided and equal to fqp_pick - parameter
//              bytes, lengths, flags - or undecided (not allowed where the fifth word is 1)
//   perturbed  every term's log one ULP up or down at random and the terms summed in a shuffled order: undecided, or equal
//   wide       guard_bits 40: undecided where any compared sum has a non-zero term, else equal
// and for every first_len 0 .. 2^16 the integer pshift rule against the host pick's expression.
// Output: one line a case "status plain perturbed wide way split size hex-of-fqp_pick's-bytes", plain / perturbed / wide
// 0 = equal, 10 = undecided, way / split what the plain pick chose (0 / 2 / 4 bins as selectors, the READ split); any
// disagreement prints FAILED and exits 1.
#include "r4x16_fqz_pick.h"
#include "r4x16_fqz_pick_dec.h"

#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

static FqdChoice chosen;      // what the last decided dev_pick chose
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

struct Terms {      // one entropy sum: its terms as (v, c)
    std::vector<std::pair<uint32_t, uint64_t>> t;
    void add(uint32_t v, uint64_t c) { if (v) t.push_back({v, c}); }
    double sum(bool perturb)
    {
        if (!perturb) { double s = 0; for (auto &p : t) s += fqd_term(p.first, p.second); return s; }
        std::vector<std::pair<uint32_t, uint64_t>> u = t;
        for (size_t i = u.size(); i > 1; i--) std::swap(u[i - 1], u[below((uint32_t)i)]);
        double s = 0;
        for (auto &p : u) {
            double l = log(p.first / (double)p.second);
            if (l != 0) l = nextafter(l, (rnd() & 1) ? 1.0 : -1e300);
            s += p.first * l;
        }
        return s;
    }
};

// The device pick from J.  FQD_OK with out / L / F, or FQD_UNDECIDED.  *zero: every compared sum is without a term.
static int dev_pick(int vers, int strat, int nrec, const uint32_t *len, const uint32_t *flags, const uint8_t *in, uint32_t size, int guard_bits,
                    bool perturb, std::vector<uint8_t> &out, std::vector<uint32_t> &L, std::vector<uint32_t> &F, bool *zero)
{
    // k_fqp_lens
    const uint32_t nw = nrec ? (uint32_t)nrec : size ? 1u : 0u;
    std::vector<uint32_t> wlen(nw + 1, 0), wstart(nw + 1, 0), wavg(nw + 1, 0), cls(nw + 1, 0);
    FqdStats fs;
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
    uint32_t qmask[8] = {0};
    for (uint32_t r = 0; r < nw; r++) {
        const uint32_t l = wlen[r], s = wstart[r];
        if (s >= size) continue;
        bool dup = s > 0 && l == wlen[r - 1];
        uint32_t tot = 0;
        for (uint32_t t = 0; t < l; t++) {
            const uint32_t q = in[s + t];
            tot += q; qmask[q >> 5] |= 1u << (q & 31);
            if (dup && in[s - l + t] != q) dup = false;
        }
        const uint32_t q10 = l ? (uint32_t)((tot * 10.0) / (int)l + .5) : 0u;
        avg[std::min<uint32_t>(q10, FQD_AVG - 1)]++;
        wavg[r] = q10;
        fs.dups += dup;
    }
    // k_fqp_bins
    for (uint32_t q = 0; q < 256; q++) if (qmask[q >> 5] >> (q & 31) & 1) { fs.nsym++; fs.max_sym = (int)q; }
    FqdParam pm;
    fqd_strat(strat, &pm);
    const bool qa = pm.do_qa != 0;
    if (qa) fqd_thresholds(avg.data(), nrec, fs.nsym);
    for (uint32_t r = 0; r < nw; r++)
        cls[r] = (nrec && (flags[r] & FQD_FREAD2) ? 4u : 0u) + (qa ? avg[std::min<uint32_t>(wavg[r], FQD_AVG - 1)] : 0u);
    // k_fqp_count
    std::vector<uint32_t> J((size_t)8 * FQD_NP * 256, 0);
    for (uint32_t r = 0; r < nw; r++)
        if (wstart[r] < size)
            for (uint32_t t = 0; t < wlen[r]; t++) J[((size_t)cls[r] * FQD_NP + ((wlen[r] - t) & (FQD_NP - 1))) * 256 + in[wstart[r] + t]]++;
    // k_fqp_sums
    Terms e1, e2, e4, r1, r2;
    for (uint32_t x = 0; x < FQD_NP; x++) {
        uint32_t cnt[8] = {0};
        for (uint32_t c = 0; c < 8; c++) for (uint32_t q = 0; q < 256; q++) cnt[c] += J[((size_t)c * FQD_NP + x) * 256 + q];
        uint32_t c4[4];
        for (uint32_t c = 0; c < 4; c++) c4[c] = cnt[c] + cnt[c + 4];
        const uint32_t c20 = c4[0] + c4[1], c21 = c4[2] + c4[3], c1 = c20 + c21, t1 = cnt[0] + cnt[1] + cnt[2] + cnt[3], t2 = c1 - t1;
        for (uint32_t q = 0; q < 256; q++) {
            uint32_t v[8], v4[4];
            for (uint32_t c = 0; c < 8; c++) v[c] = J[((size_t)c * FQD_NP + x) * 256 + q];
            for (uint32_t c = 0; c < 4; c++) { v4[c] = v[c] + v[c + 4]; e4.add(v4[c], c4[c]); }
            const uint32_t v20 = v4[0] + v4[1], v21 = v4[2] + v4[3], v1 = v20 + v21, h1 = v[0] + v[1] + v[2] + v[3];
            e2.add(v20, c20); e2.add(v21, c21); e1.add(v1, c1);
            if (t1 && t2 && v1) { r1.add(v1, (uint64_t)t1 + t2); r2.add(h1, t1); r2.add(v1 - h1, t2); }
        }
    }
    FqdSums sm;
    sm.e1 = e1.sum(perturb); sm.e2 = e2.sum(perturb); sm.e4 = e4.sum(perturb); sm.r1 = r1.sum(perturb); sm.r2 = r2.sum(perturb);
    sm.a1 = -sm.e1; sm.a2 = -sm.e2; sm.a4 = -sm.e4; sm.ra1 = -sm.r1; sm.ra2 = -sm.r2;
    *zero = (!qa || (sm.e1 == 0 && sm.e2 == 0 && sm.e4 == 0)) && (!(fs.has_r2 || pm.do_r2) || (sm.r1 == 0 && sm.r2 == 0));
    // k_fqp_store
    FqdChoice ch;
    int st = fqd_decide(&pm, &fs, &sm, guard_bits, &ch);
    if (st != FQD_OK) return st;
    chosen = ch;
    L.assign(wlen.begin(), wlen.begin() + nrec);
    F.resize(nrec);
    uint32_t fmax = 0;
    for (int r = 0; r < nrec; r++) { F[r] = fqd_flags(flags[r], cls[r] & 3u, &ch); fmax = std::max(fmax, F[r] >> 16); }
    out.assign(fqd_cap(), 0);
    FqdSink sink = {out.data(), (uint32_t)out.size(), 0u};
    st = fqd_store(&pm, &fs, &ch, vers, strat, fmax, qmask, &sink);
    if (st != FQD_OK) return st;
    if (sink.n > out.size()) { printf("FAILED: %u parameter bytes, above fqd_cap() = %zu\n", sink.n, out.size()); exit(1); }
    out.resize(sink.n);
    return FQD_OK;
}

static size_t cases = 0;
static void one_case(int vers, int strat, const std::vector<uint32_t> &len, const std::vector<uint32_t> &flags, const std::vector<uint8_t> &in, bool must)
{
    const int nrec = (int)len.size();
    std::vector<uint8_t> want, got;
    std::vector<uint32_t> L, F, L2, F2;
    // heap copies of exactly each array's size: a read beyond one stops the program
    uint32_t *l = (uint32_t *)malloc(len.size() * 4 + 1), *f = (uint32_t *)malloc(len.size() * 4 + 1);
    uint8_t *b = (uint8_t *)malloc(in.size() + 1);
    if (nrec) { memcpy(l, len.data(), len.size() * 4); memcpy(f, flags.data(), len.size() * 4); }
    if (in.size()) memcpy(b, in.data(), in.size());
    const int st = fqp_pick(vers, strat, nrec, l, f, b, in.size(), want, L, F);
    int res[3] = {0, 0, 0};
    FqdChoice plain = {0, 0};
    if (st == FQP_OK)
        for (int k = 0; k < 3; k++) {
            bool zero = false;
            res[k] = dev_pick(vers, strat, nrec, l, f, b, (uint32_t)in.size(), k == 2 ? 40 : 0, k == 1, got, L2, F2, &zero);
            if (res[k] == FQD_OK && (got != want || L2 != L || F2 != F)) {
                printf("FAILED: case %zu pick %d disagrees silently (%zu / %zu parameter bytes)\n", cases, k, got.size(), want.size());
                exit(1);
            }
            if (res[k] != FQD_OK && res[k] != FQD_UNDECIDED) { printf("FAILED: case %zu pick %d status %d\n", cases, k, res[k]); exit(1); }
            if (k == 0 && res[k] == FQD_OK) plain = chosen;
            if (k == 0 && must && res[k] != FQD_OK) { printf("FAILED: case %zu is undecided at the default guard\n", cases); exit(1); }
            if (k == 2 && (res[k] == FQD_OK) != zero && in.size() < FQD_PSHIFT_EXACT_BELOW) {
                printf("FAILED: case %zu under guard_bits 40: status %d, all-zero sums %d\n", cases, res[k], (int)zero);
                exit(1);
            }
        }
    printf("%d %d %d %d %d %d %zu ", st, res[0], res[1], res[2], plain.way, plain.split, want.size());
    for (uint8_t v : want) printf("%02x", v);
    printf("\n");
    free(l); free(f); free(b);
    cases++;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: fqz_pick_dev_check CASES RANDOM-COUNT\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5];
    while (fread(head, 4, 5, fp) == 5) {
        const uint32_t nrec = head[2], size = head[3];
        std::vector<uint32_t> len(nrec), flags(nrec);
        std::vector<uint8_t> in(size);
        if ((nrec && (fread(len.data(), 4, nrec, fp) != nrec || fread(flags.data(), 4, nrec, fp) != nrec)) ||
            (size && fread(in.data(), 1, size, fp) != size)) { printf("FAILED: short case file\n"); return 1; }
        one_case((int)head[0], (int)head[1], len, flags, in, head[4] == 1);
    }
    fclose(fp);
    // seeded random slices: 1 .. 300 records of 0 .. 300 bytes, 2 .. 60 symbols, READ2 and selector flags, lists that over- and under-run
    const int nrandom = atoi(argv[2]);
    for (int k = 0; k < nrandom; k++) {
        rng_state = 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1);      // a slice does not depend on what ran before it
        const uint32_t nrec = 1 + below(300), nsym = 2 + below(59), maxlen = k % 7 == 0 ? 300 : 1 + below(300);
        const bool fixed = below(3) == 0, r2 = below(2), sels = below(4) == 0, skew = below(2);
        std::vector<uint32_t> len(nrec), flags(nrec);
        uint64_t total = 0;
        const uint32_t fl = below(maxlen + 1);
        for (uint32_t r = 0; r < nrec; r++) {
            len[r] = fixed ? fl : below(maxlen + 1);
            flags[r] = (r2 && below(2) ? 128u : 0u) | (below(2) ? 16u : 0u) | (sels ? below(3) << 16 : 0u);
            total += len[r];
        }
        const uint32_t how = below(4);                               // exact, exact, the list over-runs, under-runs
        const uint64_t size = how == 2 ? total - std::min<uint64_t>(total, 1 + below(400)) : how == 3 ? total + 1 + below(400) : total;
        std::vector<uint8_t> in((size_t)size);
        uint64_t at = 0;
        for (uint32_t r = 0; at < size; r++) {
            // a record's level follows its READ2 flag and its number: the average-quality and the READ questions have something to find
            const uint32_t l = r < nrec ? len[r] : (uint32_t)(size - at), lvl = skew ? ((r < nrec && (flags[r] & 128u)) ? nsym / 2 : 0) + r % 3 : 0;
            const bool dup = r > 0 && r < nrec && len[r] == len[r - 1] && below(5) == 0 && at >= l;
            for (uint32_t t = 0; t < l && at < size; t++, at++)
                in[at] = dup ? in[at - l] : (uint8_t)std::min<uint32_t>(nsym - 1, (below(nsym) + lvl + (t > l / 2 ? 1 : 0)) % nsym + (skew ? lvl / 2 : 0));
        }
        one_case(k % 5 == 0 ? 3 : 4, (int)below(6), len, flags, in, false);
    }
    // pshift: the first record on either side of 2^(k + .5) * 2^pbits (strategy 0 after its bit shuffle: pbits = 3), nine symbols
    for (int k = 0; k < 64; k++) {
        const double edge = ldexp(sqrt(2.0), k + 3);
        if (edge + 1 >= FQD_PSHIFT_EXACT_BELOW) break;
        for (uint32_t first : {(uint32_t)edge, (uint32_t)edge + 1}) {
            std::vector<uint8_t> in((size_t)first + 1);
            for (size_t i = 0; i < in.size(); i++) in[i] = (uint8_t)((i * 7 + i / 5) % 9);
            one_case(4, 0, {first, 1}, {0, 0}, in, false);
        }
    }
    for (uint32_t first = 0; first <= 65536; first++)
        for (int pbits : {0, 2, 3, 4, 7})
            if (fqd_pshift(first, pbits) != fqp_pshift(first, pbits)) { printf("FAILED: pshift(%u, %d)\n", first, pbits); return 1; }
    for (int k = 0; k < 40; k++)
        for (int pbits : {0, 3, 4, 7}) {
            const double edge = ldexp(sqrt(2.0), k + pbits);
            if (edge + 2 >= FQD_PSHIFT_EXACT_BELOW) continue;
            for (uint32_t first = (uint32_t)edge - (edge >= 2 ? 2 : 0); first <= (uint32_t)edge + 2; first++)
                if (fqd_pshift(first, pbits) != fqp_pshift(first, pbits)) { printf("FAILED: pshift(%u, %d)\n", first, pbits); return 1; }
        }
    printf("fqz_pick_dev_check: ok %zu\n", cases);
    return 0;
}
