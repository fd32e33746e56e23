// r4x16_stage.h - how every host-buffer entry point lays a batch out in the staging arena: the slots of the blocks, and
// the one layout of payload regions and per-item arrays.  Host only and pure, like r4x16_plan.h whose Carver it builds
// on: nothing here knows the context or the runtime, so a stand-alone program can check it (tests/host/stage_check.cpp).
// The context's side - growing the arena, the arrays' way up and the verdicts' way back - is r4x16_stage_begin /
// r4x16_stage_verdicts (r4x16_host.h).
#pragma once
#include "r4x16_plan.h"

struct PackDesc { uint64_t src, dst; uint32_t len, pad; };      // one result to gather: slot offset, packed offset, bytes

// Slots behind each other from offset 0: block i owns k slots of align_up(size[i] + pad, align) bytes each, slot j of
// block i starts at off[i * k + j].  Returns the bytes of all slots.  The rANS calls take pad 16 and align 256, the arith
// batch pad 0 and align 16.  k > 1: the candidates of a best-of-k block.
static inline size_t r4x16_stage_slots(const uint32_t *size, size_t n, size_t pad, size_t align, uint64_t *off, size_t k = 1)
{
    size_t at = 0;
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < k; j++) { off[i * k + j] = at; at += align_up((size_t)size[i] + pad, align); }
    return at;
}

// One staged batch: the payload regions, then the per-item arrays, every piece of its own at a multiple of 256 bytes.
// (Region sizes that are multiples of 256, as the slot totals above are, leave no gap: the gathers of sparse results
// write from `in` on into `planes`.)
struct StageLayout {
    uint8_t *in, *planes, *out;              // input blocks; byte planes of X_STRIPE blocks (or nullptr); output slots
    uint64_t *in_off, *out_off;              // [items] each, and so are the five below
    uint32_t *in_size, *cap, *osz;
    int32_t *status, *order;                 // order: nullptr where the call takes one order for all
    PackDesc *pk;                            // [pk_count]: the gather of sparse results (or nullptr)
};

// base == nullptr: a dry run that only sizes.  Returns the arena's bytes.
static inline size_t r4x16_stage_layout(StageLayout *L, uint8_t *base, size_t items, size_t in_bytes, size_t plane_bytes,
                                        size_t out_bytes, bool has_order, size_t pk_count)
{
    Carver cv(base);
    L->in = cv.take<uint8_t>(in_bytes);
    L->planes = plane_bytes ? cv.take<uint8_t>(plane_bytes) : nullptr;
    L->out = cv.take<uint8_t>(out_bytes);
    L->in_off = cv.take<uint64_t>(items);
    L->out_off = cv.take<uint64_t>(items);
    L->in_size = cv.take<uint32_t>(items);
    L->cap = cv.take<uint32_t>(items);
    L->osz = cv.take<uint32_t>(items);
    L->status = cv.take<int32_t>(items);
    L->order = has_order ? cv.take<int32_t>(items) : nullptr;
    L->pk = pk_count ? cv.take<PackDesc>(pk_count) : nullptr;
    return cv.total();
}
