// r4x16_plan.h - the arithmetic every device call plans its arenas with: the carver that lays a layout out, the search
// for the largest chunk of blocks that fits a budget, the cut of a batch of unequal blocks into ranges, and the back-off when an allocation fails all the same.  Host
// only and pure: nothing here knows the context or the runtime, so a stand-alone program can check it
// (tests/host/plan_check.cpp).  The context's side - which arenas there are, how they grow, what a call may take - is
// r4x16_ensure / r4x16_room (r4x16_host.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Lays pieces out behind each other from `at`, every piece at a multiple of 256 bytes.  base == nullptr: a dry run that
// only sizes (every take returns nullptr).  A layout is one function that is run twice, dry for total() and then over
// the arena.
struct Carver {
    uint8_t *base; size_t off;
    explicit Carver(uint8_t *base_, size_t at = 0) : base(base_), off(at) {}
    // count elements of elem bytes each (elem: where the layout's stride is not the type's size)
    template <class T> T *take(size_t count, size_t elem = sizeof(T))
    {
        off = align_up(off, 256);
        T *r = base ? (T *)(base + off) : nullptr;
        off += count * elem;
        return r;
    }
    size_t total() const { return align_up(off, 256); }
};

// Blocks per chunk of a batch of n: lo = the largest value in [1, min(n, limit)] with bytes(lo) <= cap (1 if none fits:
// the allocation decides), then equal chunks rather than full ones and a rest: rounds = ceil(n / lo), ceil(n / rounds).
// bytes(nb) = what a chunk of nb blocks takes, monotone in nb.  n, limit >= 1.
template <class F>
static inline size_t r4x16_fit_chunk(size_t n, size_t limit, size_t cap, F bytes)
{
    size_t lo = 1, hi = (n < limit ? n : limit) + 1;           // bytes(lo) <= cap < bytes(hi), hi one past the range at first
    if (limit >= n) {
        if (bytes(n) <= cap) return n;
        hi = n;
    }
    while (lo + 1 < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (bytes(mid) <= cap) lo = mid; else hi = mid;
    }
    const size_t rounds = (n + lo - 1) / lo;
    return (n + rounds - 1) / rounds;
}

// Blocks whose footprints differ (the host-buffer names batches): contiguous ranges of whole blocks, cut greedily from the
// front.  A range takes blocks while the sum of their footprints stays within cap and their number within limit
// (limit 0: no limit), and one block at least - a block that exceeds cap alone is a range of its own, the allocation
// decides.  ends[r] = one past the last block of range r (ends has room for n); returns the number of ranges, 0 for n = 0.
static inline size_t r4x16_cut_ranges(const size_t *foot, size_t n, size_t cap, size_t limit, size_t *ends)
{
    size_t r = 0;
    for (size_t i = 0; i < n;) {
        size_t sum = foot[i], j = i + 1;
        while (j < n && (limit == 0 || j - i < limit) && sum <= cap && foot[j] <= cap - sum) sum += foot[j++];
        ends[r++] = i = j;
    }
    return r;
}

// Out of memory although the plan fitted (other contexts and processes share the card): walk the batch in smaller
// chunks.  grab(chunk) tries to get the chunk's arenas, 0 = it has them; the chunk halves, rounding up, until it does.
// -1: not even one block - the last failure's text stays in the context's err.
template <class F>
static inline int r4x16_backoff(size_t &chunk, F grab)
{
    for (;;) {
        if (grab(chunk) == 0) return 0;
        if (chunk == 1) return -1;
        chunk = (chunk + 1) / 2;
    }
}
