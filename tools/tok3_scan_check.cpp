// tok3_scan_check - rans4x16_hip_tok3_scan and rans4x16_hip_tok3_scan_any (htscodecs_amd/csrc/r4x16_tok3_scan.hip) over the
// containers given on the command line (either flavour) and over damaged variants of them, as a stand-alone host program: built with a sanitizer it checks that
// the walk reads nothing outside the buffer it was given, whatever the container says.  Every variant sits in a heap
// allocation of exactly its own size.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -x c++ htscodecs_amd/csrc/r4x16_tok3_scan.hip tools/tok3_scan_check.cpp -o build/tok3_scan_check
//   build/tok3_scan_check 100000 tests/golden/tok3/*
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/rans4x16_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int scan_exact(const std::vector<unsigned char> &v, uint32_t max_columns, uint32_t max_col_size, long *by_status)
{
    unsigned char *p = (unsigned char *)malloc(v.size() ? v.size() : 1);       // exactly the container: a read past it is seen
    if (v.size()) memcpy(p, v.data(), v.size());
    uint32_t ls, nr, nd, nc, lc, lst;
    uint64_t tot;
    const int rc = rans4x16_hip_tok3_scan(p, v.size(), max_columns, max_col_size, &ls, &nr, &nd, &nc, &tot, &lc, &lst);
    // the same bytes through the scan of either flavour: the same verdict where byte 8 is clear, else scan refuses at the
    // header and scan_any walks on
    uint32_t als, anr, and_, anc, alc, alst;
    uint64_t atot;
    int arith = -1;
    const int arc = rans4x16_hip_tok3_scan_any(p, v.size(), max_columns, max_col_size, &als, &anr, &and_, &anc, &atot, &alc, &alst, &arith);
    const bool flagged = v.size() > 8 && p[8] != 0;
    free(p);
    if (arith != (flagged ? 1 : 0)) { fprintf(stderr, "scan_any reports flavour %d\n", arith); exit(2); }
    if (!flagged && (arc != rc || als != ls || anr != nr || and_ != nd || anc != nc || atot != tot || alc != lc || alst != lst)) {
        fprintf(stderr, "scan_any differs from scan on a container without the flag\n"); exit(2);
    }
    if (flagged && (rc != R4X16_E_UNSUPPORTED || nd != 0)) { fprintf(stderr, "scan walks a container with use_arith set\n"); exit(2); }
    if (arc < 0 || arc > 9 || and_ > (max_columns ? max_columns : 2048u) || anc > 2u * and_ || alst > v.size()) { fprintf(stderr, "scan_any out of range\n"); exit(2); }
    if (flagged) { by_status[arc]++; return arc; }
    if (rc < 0 || rc > 9) { fprintf(stderr, "scan returned %d\n", rc); exit(2); }
    if (nd > (max_columns ? max_columns : 2048u) || nc > 2u * nd || lst > v.size()) { fprintf(stderr, "scan counts out of range\n"); exit(2); }
    by_status[rc]++;
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s variants container..\n", argv[0]); return 1; }
    const long variants = atol(argv[1]);
    std::vector<std::vector<unsigned char>> fx;
    for (int i = 2; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) { perror(argv[i]); return 1; }
        std::vector<unsigned char> v;
        unsigned char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        fclose(f);
        fx.push_back(v);
    }
    long by_status[10] = {};
    for (auto &v : fx)
        if (scan_exact(v, 0, 0, by_status) != 0) { fprintf(stderr, "a fixture does not scan\n"); return 2; }
    printf("%zu containers scan\n", fx.size());
    memset(by_status, 0, sizeof by_status);
    for (long r = 0; r < variants; r++) {
        std::vector<unsigned char> v = fx[rnd() % fx.size()];
        switch (r % 5) {
        case 0: for (int k = 1 + (int)(rnd() % 3); k; k--) v[rnd() % v.size()] = (unsigned char)rnd(); break;          // anywhere
        case 1: v[rnd() % (v.size() < 300 ? v.size() : 300)] ^= (unsigned char)(1u << (rnd() % 8)); break;              // header and first descriptors
        case 2: v.resize(rnd() % v.size()); break;                                                                        // cut
        case 3: v.resize(9 + rnd() % 40); for (size_t k = 9; k < v.size(); k++) v[k] = (unsigned char)rnd(); break;       // random descriptors
        default: for (size_t k = 9; k < v.size(); k += 1 + rnd() % 64) if (rnd() & 1) v[k] |= 0x80; break;                // continuation bits
        }
        scan_exact(v, r % 7 == 0 ? 1 + (uint32_t)(rnd() % 64) : 0, r % 11 == 0 ? (uint32_t)(rnd() % 5000) : 0, by_status);
    }
    printf("%ld damaged variants:", variants);
    for (int s = 0; s < 10; s++) if (by_status[s]) printf(" status %d x %ld", s, by_status[s]);
    printf("\n");
    return 0;
}
