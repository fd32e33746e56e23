// r4x16_fqz_best.h - what the three fqzcomp_qual encode units share on the device side: the pick's and the encoder's
// per-chunk work areas (r4x16_fqz_pick.hip, r4x16_fqz_enc.hip) and the stages of either that the best-of-several call
// (r4x16_fqz_best.hip, include/rans4x16_hip.h part 2l) runs on its own: the pick's statistics once per slice, the
// encoder's front and encode kernels over the candidates without its back end.  The best-of-several call's own chunk, in
// two halves, is declared at the end: the call that picks across codecs (r4x16_best_qual.hip, part 2n) runs them too.
#pragma once
#include "r4x16_host.h"
#include "r4x16_fqz_pick_dec.h"

// ---- the pick (r4x16_fqz_pick.hip) ----------------------------------------------------------------------------------
#define FQP_J_CELLS (2u * 4u * FQD_NP * 256u)
#define FQP_PARTS 8u                        // workgroups of k_fqp_sums per block
#define FQP_STAGE ((fqd_cap() + 15u) & ~15u)
#define FQP_REC_GROUPS 256u                 // workgroups per block of the record kernels, at most

struct FqpIn {
    const u32 *len, *flags; const u64 *rec_off; const u32 *nrec; const i32 *d_strat;
    int vers, strat, guard_bits;
    u32 *len_out, *flags_out; const u64 *out_rec_off;    // out_rec_off and the slot arrays: indexed from obase
    // best-of-several: a candidate beside the block's own strategy asks the average-quality question / the READ question -
    // the bins are computed and J is counted for it (the block's own decisions read the same marginals either way)
    int any_qa, any_r2;
};
struct FqpBlk {
    i32 status, strat;
    u32 size, nrec, nw;                     // nw: the records worked on - nrec, or 1 for bytes without a record
    u32 first_len, fixed_len, has_r2, caller_max_sel, visited, dups;
    u32 nsym, max_sym, need_j;
    u32 qmask[8];
};
struct FqpWs {
    FqpBlk *blk;                            // [nb]
    u32 *route;                             // [R4X16_FQZ_PICK_KINDS]; nullptr in the kernels' copy: option route_count is off
    u32 *wlen, *wstart, *wavg;              // [nb] x rec_stride: fixed length, first byte, avg_qual
    u8 *wcls;                               // [nb] x rec_stride: dir * 4 + bin
    u32 *avg;                               // [nb] x 2560
    u32 *J;                                 // [nb] x FQP_J_CELLS
    double *part;                           // [nb] x FQP_PARTS x 5
    u8 *par;                                // [nb] x FQP_STAGE
    u64 rec_stride;
};

__device__ __forceinline__ u32 fqp_wave_max(u32 v)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) { const u32 o = (u32)__shfl_xor((int)v, m); v = v > o ? v : o; }
    return v;
}
// what the decisions read of a block: the record pass's and the byte pass's results, the entropy sums of its parts
__device__ __forceinline__ void fqp_stats_of(const FqpBlk *bk, const double *part, FqdStats *fs, FqdSums *sm)
{
    fs->nrec = (int)bk->nrec; fs->in_size = bk->size; fs->first_len = bk->first_len; fs->fixed_len = (int)bk->fixed_len;
    fs->has_r2 = (int)bk->has_r2; fs->caller_max_sel = (int)bk->caller_max_sel; fs->visited = bk->visited; fs->dups = bk->dups;
    fs->nsym = (int)bk->nsym; fs->max_sym = (int)bk->max_sym;
    *sm = FqdSums{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (bk->need_j) {
        for (u32 k = 0; k < FQP_PARTS; k++) { sm->e1 += part[5 * k]; sm->e2 += part[5 * k + 1]; sm->e4 += part[5 * k + 2]; sm->r1 += part[5 * k + 3]; sm->r2 += part[5 * k + 4]; }
        // every term is <= 0: the sum of the |terms| is the sum's own magnitude
        sm->a1 = -sm->e1; sm->a2 = -sm->e2; sm->a4 = -sm->e4; sm->ra1 = -sm->r1; sm->ra2 = -sm->r2;
    }
}

// a chunk's layout at `base` (nullptr: sized only), the blocks a chunk holds at most, and the statistics of one chunk -
// k_fqp_lens, k_fqp_recs, k_fqp_bins, k_fqp_count, k_fqp_sums over blocks base .. base + nb of `a` and `in` into `w`
size_t r4x16_fqp_layout(u8 *base, size_t nb, u32 max_rec, FqpWs *w);
size_t r4x16_fqp_chunk_limit(u32 max_rec);
int r4x16_fqp_stats(rans4x16_hip_ctx *c, const BatchArgs &a, const FqpIn &in, const FqpWs &w, int base, int nb, u32 max_in, u32 max_rec,
                    hipStream_t s);

// ---- the encoder (r4x16_fqz_enc.hip) --------------------------------------------------------------------------------
struct FqeBlk {
    i32 status; u32 size, gflags, nparam;
    u32 max_sel, max_sym, home, nrec;
    u32 body, lim, uses_sel, dups;      // dups: records coded as duplicates (k_fqe_encode)
    u64 tab;                // in the stage arena: the selector table, then nparam x FQ_PARAM_BYTES
    u64 inv;                // nparam x 256: quality -> symbol
    u64 cod;                // the block in coder order (GFLAG_DO_REV only)
    u64 out;                // the coder's bytes: 16-byte aligned, lim + 48 rounded up to 16
};
struct FqeWs {
    FqeBlk *blk;            // [nb]
    u64 *cursor;            // bytes of the stage arena handed out (a chunk's)
    u32 *route;             // [R4X16_FQZ_ENC_KINDS]; nullptr in the kernels' copy: option route_count is off
    u8 *stage;
    u64 stage_bytes;
    u8 *rows;               // [slots] x slot_bytes
    u64 slot_bytes;
    u32 slots, max_sym;
};
__host__ __device__ static inline u32 fqe_var_len(u32 v)
{
    u32 groups = 1;
    for (u32 t = v >> 7; t; t >>= 7) groups++;
    return groups;
}
// One chunk's front and encode stages, as r4x16_fqe_chunk runs them, without its back end: *w is the chunk's work area
// with the kernels' route pointer, *d_route the counters for r4x16_route_end(c, R4X16_ROUTE_FQZ_ENC, ..), which the caller
// owes once its own back end is enqueued.
int r4x16_fqe_stages(rans4x16_hip_ctx *c, const BatchArgs &a, const FqeIn &in, u8 *at, int base, int nb, u32 max_in_size, u32 max_params_size,
                     u32 max_records, hipStream_t s, FqeWs *w, u32 **d_route);

// ---- best of several strategies (r4x16_fqz_best.hip) ------------------------------------------------------------------
// The call in two halves, for the call that picks across codecs (r4x16_best_qual.hip, part 2n) as r4x16_ab_candidates is
// for arith: the candidates stage - statistics, store, front, encode, k_fqb_win - leaves every block's winner known by its
// size, and the back pass assembles the winners that are wanted at their final place.
#define FQB_MAX_K 16
struct FqbStrats { int k; int s[FQB_MAX_K]; };
// a chunk's hand-over between the stages, every array indexed by item but win ([nb])
struct FqbHand {
    u8 *par; u32 *flags;
    u64 *par_off, *rec_off, *len_off, *in_off;
    u32 *par_size, *nrec, *in_size, *out_cap, *out_size;
    i32 *pick_status, *status, *win;
    u32 *route;                             // [R4X16_FQZ_BEST_KINDS]; nullptr in the kernels' copy: option route_count is off
};
// candidate sets picked elsewhere (the host): what k_fqb_store would have left, entry g * k + j of every array for
// candidate j of block g of the whole call
struct FqbSets {
    const u8 *par; const u64 *par_off; const u32 *par_size;        // par_size FQB_NO_PARAMS: the pick refused the candidate
    const u32 *len, *flags; const u64 *rec_off, *len_off; const u32 *nrec;
    u32 max_par;
};
// a chunk's work area between r4x16_fqb_candidates and r4x16_fqb_back: the layouts in the arena, the encoder's inputs,
// the route counters the back pass reads out
struct FqbWork { FqpWs pw; FqbHand h; FqeWs fw; FqeIn ein; u32 *d_best, *d_enc; };
// the strategies alone: what a call refuses before it asks for the device (`who` names the call in err)
int r4x16_fqb_strats(rans4x16_hip_ctx *c, const char *who, int k, const int *strats, FqbStrats *ks);
// the bytes a chunk of nb blocks under k strategies takes at `at`, and the blocks a chunk holds at most
size_t r4x16_fqb_chunk_bytes(rans4x16_hip_ctx *c, size_t nb, size_t k, u32 max_in, u32 max_rec, bool sets);
size_t r4x16_fqb_chunk_limit(int k, u32 max_rec);
int r4x16_fqb_candidates(rans4x16_hip_ctx *c, const BatchArgs &a, const u32 *d_len, const u32 *d_flags, const u64 *d_rec_off, const u32 *d_nrec,
                         int vers, const FqbStrats &ks, const FqbSets *sets, u8 *at, int base, int nb, u32 *out_size, i32 *status, i32 *chosen,
                         int obase, u32 max_in, u32 max_rec, hipStream_t s, FqbWork *w);
int r4x16_fqb_back(rans4x16_hip_ctx *c, const BatchArgs &a, const PackedOut *pk, const FqbWork &w, u32 *d_len_out, const u64 *d_rec_off,
                   const u32 *d_nrec, int base, int nb, const i32 *take, hipStream_t s);
