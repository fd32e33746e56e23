// best_qual_check.cpp - checks htscodecs_amd/csrc/r4x16_best_qual.h on the host, alone: what the best-of calls across codecs
// (include/rans4x16_hip.h parts 2m and 2n) refuse of a method list before they ask for a device, with the reason they give,
// and the three sub-lists they make of a list they take.  Built with -fsanitize=address,undefined and run as a program of
// its own (tests/test_best_qual_cpu.py); prints one line per list under the quality calls' flavour, which admits all three
// tags - "<name>: <reason or ok>" and, for a list that is taken, the sub-lists - and the same again as "2m <name>: ..."
// under part 2m's, which admits no fqzcomp tag; then "best_qual_check: ok" and 0, or 1 where a check of its own failed.
#include "r4x16_best_qual.h"

#include <stdio.h>
#include <string.h>
#include <vector>

#define FQZ(s) (R4X16_CODEC_FQZ | (s))
#define ARITH(o) (R4X16_CODEC_ARITH | (o))

static int g_failed = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                             \
    } while (0)

// k may differ from the list's length (k = 0, k = 33 over a list that is long enough); a NULL list has no entries
static const char *run_as(const char *flavour, unsigned admit, const char *name, int k, const std::vector<int> &methods, bool null_list)
{
    BqSplit p;
    memset(&p, 0x5a, sizeof p);
    const char *why = bq_split(k, null_list ? nullptr : methods.data(), &p, admit);
    printf("%s%s: %s", flavour, name, why ? why : "ok");
    if (!why) {
        CHECK(p.pm.k == k && p.kr + p.ka + p.kf == k, "%s: %d + %d + %d of %d", name, p.kr, p.ka, p.kf, k);
        printf(" | rans");
        for (int j = 0; j < p.kr; j++) printf(" %d", p.rm[j]);
        printf(" | arith");
        for (int j = 0; j < p.ka; j++) printf(" %d", p.am[j]);
        printf(" | fqz");
        for (int j = 0; j < p.kf; j++) {
            printf(" %d@%d", p.sm[j], p.pm.fpos[j]);
            CHECK(p.pm.fpos[j] >= 0 && p.pm.fpos[j] < k && p.pm.m[p.pm.fpos[j]] == FQZ(p.sm[j]), "%s: strategy %d stands at %d", name, j, p.pm.fpos[j]);
        }
        for (int j = 0; j < k; j++) CHECK(p.pm.m[j] == methods[j], "%s: entry %d", name, j);
    }
    printf("\n");
    return why;
}

static void run(const char *name, int k, const std::vector<int> &methods, bool null_list = false)
{
    run_as("", BQ_RANS | BQ_ARITH | BQ_FQZ, name, k, methods, null_list);
    run_as("2m ", BQ_RANS | BQ_ARITH, name, k, methods, null_list);
}

int main()
{
    // the lists the calls take
    run("triple", 3, {0, ARITH(0), FQZ(0)});
    run("reversed", 3, {FQZ(0), ARITH(0), 0});
    run("eight", 8, {1, 65, ARITH(1), ARITH(65), FQZ(0), FQZ(1), FQZ(2), FQZ(3)});
    run("one strategy", 1, {FQZ(7)});
    run("no strategy", 2, {193, ARITH(193)});
    run("stripes of 255 planes", 2, {8 | (255 << 8), ARITH(9 | (255 << 8))});
    std::vector<int> sixteen(32, 1), seventeen(32, 1), thirty_three(33, 0);
    for (int j = 0; j < 16; j++) sixteen[2 * j] = FQZ(j);
    for (int j = 0; j < 17; j++) seventeen[j + 3] = FQZ(j & 3);
    run("sixteen strategies among 32", 32, sixteen);
    // the lists they refuse
    run("k = 0", 0, {0});
    run("k = 33", 33, thirty_three);
    run("a NULL list", 2, {}, true);
    run("the rANS 4x8 tag's place", 2, {0, (2 << 24) | 1});
    run("the tag behind fqzcomp's", 2, {FQZ(0), (4 << 24) | 1});
    run("the highest tag", 1, {0x0F000000});
    run("bits above the tag", 1, {FQZ(1) | (1 << 28)});
    run("a negative word", 1, {-1});
    run("a negative strategy", 2, {FQZ(0), (int)(R4X16_CODEC_FQZ | -2)});
    run("a rANS word with bit 16", 2, {1, 1 | (1 << 16)});
    run("an arith word with bit 23", 2, {1, ARITH(65 | (1 << 23))});
    run("a strategy with bit 16", 2, {1, FQZ(1 | (1 << 16))});
    run("a strategy with bit 23", 1, {FQZ(1 << 23)});
    run("a rANS stripe method of 256 planes", 2, {1, 8 | (256 << 8)});
    run("an arith stripe method of 256 planes", 2, {1, ARITH(9 | (256 << 8))});
    run("seventeen strategies", 32, seventeen);
    if (g_failed) { printf("best_qual_check: %d checks failed\n", g_failed); return 1; }
    printf("best_qual_check: ok\n");
    return 0;
}
