// r4x16_best_any.h - what the best-of-k units hand to the call that picks across codecs (r4x16_best_qual.hip,
// include/rans4x16_hip.h parts 2m and 2n): each codec's candidates of one chunk of blocks, encoded into that codec's own internal
// slots and reduced to one winner a block by that codec's own pick kernel - everything of its best-packed call but the
// scan and the gather -, the bytes such a chunk takes, and the reader of a stream's size field that both codecs share.
#pragma once
#include "r4x16_host.h"

// ---- arith_dynamic (r4x16_arith_enc.hip) ---------------------------------------------------------------------------
#define AB_MAX_K 32
struct AbMethods { int k; int m[AB_MAX_K]; };
struct AbWs {
    u64 *in_off, *slot_off /*[items + 1]*/; u32 *in_size, *need, *cap, *out_size; i32 *status, *order; u32 *win /*[nb]*/; u8 *slots; u64 slot_bytes;
};
// What the call plans before it enqueues: the methods, the planes a stripe candidate may have, the items an inner item
// reserves, the batch's bytes and the blocks per chunk
struct AbPlan { AbMethods pm; u32 planes; size_t per; u64 total; size_t chunk; };
// the methods alone: what a call refuses before it asks for the device (`who` names the call in err)
int r4x16_ab_methods(rans4x16_hip_ctx *c, const char *who, int k, const int *methods, AbPlan *p);
// per, total (chunk stays 0: the caller's fit)
void r4x16_ab_sizes(int n, uint32_t max_in_size, uint64_t total_in_size, AbPlan *p);
// a chunk of nb blocks: the candidate slots with their arrays (carved at `base`, nullptr: a dry run), and the inner call's arena
size_t r4x16_ab_carve(AbWs *w, u8 *base, const AbPlan &p, size_t nb, u32 max_in_size);
size_t r4x16_ab_inner_bytes(const AbPlan &p, size_t nb, u32 max_in_size);
// blocks [base, base + nb) as k items each into w's slots, then k_ab_pick: out_size / status / chosen (may be null) are
// the chunk's own, indexed like w.win by the block's place in the chunk.  `arena`: the bytes the caller holds beside
// the inner call's (its ceiling shrinks by as much).  Enqueues only; 0 or -1.
int r4x16_ab_candidates(rans4x16_hip_ctx *c, const AbPlan &p, const AbWs &w, size_t arena, size_t base, int nb, const u8 *d_in,
                        const u64 *d_in_off, const u32 *d_in_size, u32 *out_size, i32 *status, i32 *chosen, u32 max_in_size, hipStream_t s);

// ---- rANS 4x16 (r4x16_best.hip, r4x16_packed.hip) --------------------------------------------------------------------
// the candidate arena and the inner call's workspace of rans4x16_hip_compress_best_dev over a chunk of nb blocks
size_t r4x16_best_chunk_bytes(int k, const int *methods, size_t nb, uint32_t max_in_size, uint64_t total_in_size);
// k_pk_slots under a method list: block i of the n owns slot i % chunk, its capacity the largest bound over the methods
void r4x16_launch_packed_slots_best(const u32 *d_in_size, int k, const int *methods, const PackedSlots *p, int n, size_t chunk,
                                    u32 max_in_size, hipStream_t s);

// ---- the size field ----------------------------------------------------------------------------------------------------
#define PK_NO_SIZE 0xffffffffu
// First byte and stored uncompressed size of one stream (rANS_static4x16pr.c:1360-1366 for X_STRIPE, :1435-1448
// otherwise; arith_dynamic has both where rANS 4x16 has them): the varint at byte 1, absent (PK_NO_SIZE) for X_NOSZ
// streams that are no stripes.
static __device__ __forceinline__ i32 peek_one(const u8 *in, u32 in_size, u32 max_in, i32 *format, u32 *raw)
{
    *format = -1; *raw = PK_NO_SIZE;
    if (in_size == 0) return ST_EMPTY;                                                // :1357
    if (in_size > max_in) return ST_UNSUPPORTED;                                      // larger than the call was sized for
    ByteSrc src(in);
    const u32 flags = src.at(0);
    *format = (i32)flags;
    if (!(flags & X_STRIPE) && (flags & X_NOSZ)) return ST_OK;
    u32 v = 0;
    const u32 used = var_get(src, 1u, in_size, &v);
    if (used == 0 || (src.at(used) & 0x80)) return ST_TRUNCATED;                      // no byte left, or the last one still continues
    *raw = v;
    return ST_OK;
}
