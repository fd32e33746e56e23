// names_plan_check.cpp - r4x16_cut_ranges (htscodecs_amd/csrc/r4x16_plan.h) against a brute-force scan: a stand-alone
// program, built with the address and undefined-behaviour sanitizers by tests/test_names_plan_cpu.py.
#include "r4x16_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static unsigned long long rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond) do { if (!(cond)) { printf("names_plan_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the end of the range that starts at i, by trying every end from the far one down
static size_t brute_end(const std::vector<size_t> &foot, size_t i, size_t cap, size_t limit)
{
    const size_t n = foot.size();
    size_t far = limit ? (i + limit < n ? i + limit : n) : n;
    for (size_t e = far; e > i + 1; e--) {
        unsigned __int128 sum = 0;
        for (size_t j = i; j < e; j++) sum += foot[j];
        if (sum <= cap) return e;
    }
    return i + 1;
}

static int check(const std::vector<size_t> &foot, size_t cap, size_t limit)
{
    const size_t n = foot.size();
    std::vector<size_t> ends(n + 1, (size_t)-1);
    const size_t ranges = r4x16_cut_ranges(foot.data(), n, cap, limit, ends.data());
    CHECK(ends[n] == (size_t)-1);                       // nothing behind the n entries it may use
    CHECK((n == 0) == (ranges == 0));
    CHECK(ranges <= n);
    size_t at = 0;
    for (size_t r = 0; r < ranges; r++) {
        CHECK(ends[r] > at && ends[r] <= n);             // contiguous, one block at least
        CHECK(limit == 0 || ends[r] - at <= limit);
        unsigned __int128 sum = 0;
        for (size_t j = at; j < ends[r]; j++) sum += foot[j];
        CHECK(sum <= cap || ends[r] - at == 1);          // fits, or holds one block
        CHECK(ends[r] == brute_end(foot, at, cap, limit));
        at = ends[r];
    }
    CHECK(at == n);                                      // covers 0 .. n
    return 0;
}

int main()
{
    if (check({}, 100, 0)) return 1;
    if (check({}, 0, 3)) return 1;
    if (check({(size_t)-1}, 100, 0)) return 1;          // one huge block
    if (check({5, (size_t)-1, (size_t)-1, 5}, (size_t)-1, 0)) return 1;
    if (check({(size_t)-1 / 2, (size_t)-1 / 2, 2, 1}, (size_t)-1, 2)) return 1;
    if (check({0, 0, 0, 0}, 0, 0)) return 1;
    if (check({1, 1, 1, 1, 1}, 0, 0)) return 1;
    for (int t = 0; t < 4000; t++) {
        const size_t n = rnd() % 40;
        std::vector<size_t> foot(n);
        const size_t scale = (size_t)1 << (rnd() % 40);
        for (auto &f : foot) f = rnd() % 16 == 0 ? (size_t)(rnd() % (scale * 64 + 1)) : (size_t)(rnd() % (scale + 1));
        const size_t cap = rnd() % (scale * 8 + 1), limit = rnd() % 3 == 0 ? 0 : rnd() % 9;
        if (check(foot, cap, limit)) return 1;
    }
    printf("names_plan_check: ok\n");
    return 0;
}
