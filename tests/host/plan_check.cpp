// plan_check.cpp - checks htscodecs_amd/csrc/r4x16_plan.h on the host, alone: the chunk search against its definition
// written as a plain loop, the gathered route's former division against the search, the carver's layouts, the back-off.
// Built with -fsanitize=address,undefined and run as a program of its own (tests/test_plan_cpu.py); prints one line
// per failed check and exits 1, or "plan_check: ok" and 0.
#include "r4x16_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                             \
    } while (0)

// the definition: lo = the largest value in [1, min(n, limit)] with bytes(lo) <= cap, 1 if none; equal rounds
template <class F>
static size_t scan_chunk(size_t n, size_t limit, size_t cap, F bytes)
{
    size_t lo = 1;
    for (size_t nb = 1; nb <= n && nb <= limit; nb++) if (bytes(nb) <= cap) lo = nb;
    const size_t rounds = (n + lo - 1) / lo;
    return (n + rounds - 1) / rounds;
}

template <class F>
static void search_against_scan(const char *what, size_t n, F bytes, size_t cap_lo, size_t cap_hi, size_t cap_step)
{
    const size_t limits[] = {1, 2, 3, n / 2 ? n / 2 : 1, n > 1 ? n - 1 : 1, n, n + 1, SIZE_MAX};
    for (size_t limit : limits)
        for (size_t cap = cap_lo; cap <= cap_hi; cap += cap_step) {
            const size_t got = r4x16_fit_chunk(n, limit, cap, bytes), want = scan_chunk(n, limit, cap, bytes);
            CHECK(got == want, "%s n %zu limit %zu cap %zu: %zu, the scan says %zu", what, n, limit, cap, got, want);
            CHECK(got >= 1 && got <= n, "%s n %zu limit %zu cap %zu: %zu outside the batch", what, n, limit, cap, got);
            if (limit >= n && bytes(n) <= cap) CHECK(got == n, "%s n %zu cap %zu: the whole batch fits, got %zu", what, n, cap, got);
        }
}

static void check_search()
{
    for (size_t n = 1; n <= 200; n++) {
        // every cap from below bytes(1) to above bytes(n)
        auto lin = [](size_t nb) { return (size_t)5 + nb * 3; };
        search_against_scan("linear", n, lin, lin(1) - 2, lin(n) + 2, 1);
        auto step = [](size_t nb) { return (size_t)7 + (nb + 7) / 8 * 11 + nb / 50 * 40; };      // flat stretches and jumps
        search_against_scan("step", n, step, step(1) - 2, step(n) + 2, 1);
        auto big = [](size_t nb) { return (size_t)4096 + nb * 4352; };
        search_against_scan("large stride", n, big, big(1) - 300, big(n) + 300, 149);
    }
}

// the packed calls' slot layout (r4x16_packed_carve): two arrays over the whole batch, then a chunk's slots
static size_t packed_bytes(size_t n, size_t nb, size_t stride)
{
    Carver cv(nullptr);
    cv.take<uint64_t>(n);
    cv.take<uint32_t>(n);
    cv.take<uint8_t>(nb * stride + 256);
    return cv.total();
}

// what the gathered route computed by division before it called the search
static size_t gathered_by_division(size_t n, size_t budget, size_t stride)
{
    const size_t fixed = packed_bytes(n, 0, stride);
    size_t chunk = budget > fixed + stride ? (budget - fixed) / stride : 1;
    if (chunk > n) chunk = n;
    const size_t rounds = (n + chunk - 1) / chunk;
    return (n + rounds - 1) / rounds;
}

static void check_gathered()
{
    const size_t strides[] = {256, 512, 4352, 1 << 20};
    for (size_t stride : strides)
        for (size_t n = 1; n <= 200; n += (n < 40 ? 1 : 7)) {
            auto bytes = [&](size_t nb) { return packed_bytes(n, nb, stride); };
            const size_t fixed = bytes(0);
            CHECK(bytes(3) == fixed + 3 * stride, "stride %zu n %zu: the slots are not fixed + nb * stride", stride, n);
            for (size_t nb = 0; nb <= n + 1; nb++)
                for (long d = -2; d <= 2; d++) {                       // budgets around every point where the answer changes
                    const size_t at = fixed + nb * stride;
                    if (d < 0 && at < (size_t)-d) continue;
                    const size_t budget = at + d;
                    const size_t got = r4x16_fit_chunk(n, SIZE_MAX, budget, bytes), want = gathered_by_division(n, budget, stride);
                    CHECK(got == want, "gathered stride %zu n %zu budget %zu: %zu, the division gave %zu", stride, n, budget, got, want);
                }
            for (size_t budget = 0; budget <= fixed + (n + 1) * stride; budget += stride / 3 + 37) {
                const size_t got = r4x16_fit_chunk(n, SIZE_MAX, budget, bytes), want = gathered_by_division(n, budget, stride);
                CHECK(got == want, "gathered stride %zu n %zu budget %zu: %zu, the division gave %zu", stride, n, budget, got, want);
            }
        }
}

struct Piece { size_t off, bytes; };

// one layout of mixed types, an explicit element size and empty pieces; dry (base == nullptr) or real
static size_t layout(uint8_t *base, size_t at, const size_t count[5], std::vector<Piece> *pieces)
{
    Carver cv(base, at);
    auto note = [&](void *p, size_t bytes) {
        if (base) pieces->push_back({(size_t)((uint8_t *)p - base), bytes});
        else CHECK(p == nullptr, "a dry run handed out a pointer");
    };
    note(cv.take<uint64_t>(count[0]), count[0] * 8);
    note(cv.take<uint32_t>(count[1]), count[1] * 4);
    note(cv.take<uint8_t>(count[2], 48), count[2] * 48);               // (records of 48 bytes)
    note(cv.take<uint8_t>(count[3], 0), 0);                            // (a table this batch does not need)
    note(cv.take<uint16_t>(count[4]), count[4] * 2);
    return cv.total();
}

static void check_carver()
{
    const size_t counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000};
    const size_t starts[] = {0, 256, 4096};
    const size_t nc = sizeof(counts) / sizeof(counts[0]);
    for (size_t at : starts)
        for (size_t i = 0; i < nc * nc * nc; i++) {
            const size_t count[5] = {counts[i % nc], counts[i / nc % nc], counts[i / nc / nc], counts[(i * 7) % nc], counts[(i * 3 + 1) % nc]};
            const size_t dry = layout(nullptr, at, count, nullptr);
            CHECK(dry % 256 == 0 && dry >= at, "at %zu: a total of %zu", at, dry);
            uint8_t *arena = (uint8_t *)malloc(dry ? dry : 1);          // exactly the dry run's size: a write beyond it is a finding
            std::vector<Piece> pieces;
            const size_t real = layout(arena, at, count, &pieces);
            CHECK(real == dry, "at %zu: the dry run says %zu, the real run ends at %zu", at, dry, real);
            CHECK(pieces[0].off == at, "at %zu: the first piece starts at %zu", at, pieces[0].off);
            for (size_t k = 0; k < pieces.size(); k++) {
                CHECK(pieces[k].off % 256 == 0, "piece %zu at %zu", k, pieces[k].off);
                const size_t next = k + 1 < pieces.size() ? pieces[k + 1].off : real;
                CHECK(pieces[k].off + pieces[k].bytes <= next, "piece %zu [%zu, +%zu) runs into %zu", k, pieces[k].off, pieces[k].bytes, next);
                memset(arena + pieces[k].off, (int)k, pieces[k].bytes);
            }
            free(arena);
        }
}

static void check_backoff()
{
    for (size_t start = 1; start <= 300; start++)
        for (size_t fits = 0; fits <= start; fits += (fits < 5 ? 1 : 13)) {        // fits == 0: nothing can be had
            size_t chunk = start, want = start, calls = 0, last = 0;
            while (want > fits && want > 1) want = (want + 1) / 2;
            const int rc = r4x16_backoff(chunk, [&](size_t nb) { calls++; last = nb; return nb <= fits ? 0 : -1; });
            CHECK(rc == (want <= fits ? 0 : -1), "back-off from %zu, %zu fit: rc %d", start, fits, rc);
            CHECK(chunk == want && last == want, "back-off from %zu, %zu fit: ends at %zu, asked last for %zu, expected %zu", start, fits, chunk, last, want);
            CHECK(calls <= 10, "back-off from %zu: %zu tries", start, calls);
        }
}

int main()
{
    check_search();
    check_gathered();
    check_carver();
    check_backoff();
    if (g_failed) { printf("plan_check: %d checks failed\n", g_failed); return 1; }
    printf("plan_check: ok\n");
    return 0;
}
