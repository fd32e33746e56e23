// r4x16_fqz_pick.hip - the parameter choice of htscodecs' quality encoder on the device: fqz_qual_stats(.., -1),
// fqz_pick_parameters and fqz_store_parameters (fqzcomp_qual.c:418-945) over slices in device memory:
// include/rans4x16_hip.h part 2k.  The host's restatement is r4x16_fqz_pick.h; the decisions and the store are
// r4x16_fqz_pick_dec.h, the same code on both sides.  The work areas and the statistics stages (r4x16_fqp_stats: the
// first five kernels) are declared in r4x16_fqz_best.h: the best-of-several call runs them once for all its candidates.
//
// Everything fqz_qual_stats counts is a marginal of one joint histogram J[dir][bin][x][q]: dir READ2 or not,
// bin the record's average-quality bin, x = j & 127 with j counting down from the record's length, q the quality.  A
// block's J is 2 * 4 * 128 rows of 256 plain u32 counters in the context's arena (1 MiB), counted through L2.  Stages:
//   k_fqp_lens    one wave per block: the length fix-ups as a clamped prefix sum, where each record starts, first_len,
//                 fixed_len, has_r2, the caller's max_sel, the records the reference's loop visits
//   k_fqp_recs    one wave per record: its `tot` and avg_qual, the duplicate test against the record before, the
//                 2,560-entry avg histogram, which qualities occur
//   k_fqp_bins    one wave per block: nsym and max_sym, the thresholds (avg -> bin map), each record's (dir, bin) class
//                 (the bins where the block's strategy - or, best of several, any candidate's: FqpIn.any_qa - asks)
//   k_fqp_count   one wave per record: J, one atomic a byte
//   k_fqp_sums    eight workgroups per block, sixteen x each: the row totals, then the entropy terms of the non-zero cells
//   k_fqp_store   one wave per block: the decisions, the flags' largest selector, the parameter bytes into the stage,
//                 then - the capacity tested - the bytes, lengths and flags to the caller, the verdict
//
// Loops: over the records (nrec <= max_records), the bytes of a record (its fixed length: the lengths sum to the size
// before a byte is read), tables of fixed size.  Stores: the work arrays are sized by max_records + 1 and max_in_size,
// tested in k_fqp_lens before anything is read; only k_fqp_store writes to the caller's memory, after it has tested
// the slot's capacity, and only for a block whose status is 0.  All stores are plain vector stores or vector atomics.
#include "r4x16_host.h"
#include "r4x16_fqz_best.h"

__device__ __forceinline__ double fqp_wave_dsum(double v)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- (a) the records ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqp_lens(BatchArgs a, FqpIn in, FqpWs w, int base, int nb, u32 max_in, u32 max_rec)
{
    const u32 lane = threadIdx.x & 63u;
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b;
    const u32 size = a.in_size[g], nrec = in.nrec[g];
    const i32 strat = in.d_strat ? in.d_strat[g] : in.strat;
    FqpBlk bk;
    bk.status = size > max_in || size >= 0x80000000u || nrec > max_rec || nrec >= 0x80000000u || strat < 0 ? (i32)R4X16_E_UNSUPPORTED : 0;
    bk.strat = strat; bk.size = size; bk.nrec = nrec; bk.nw = nrec ? nrec : size ? 1u : 0u;
    bk.first_len = 0; bk.fixed_len = nrec != 0; bk.has_r2 = 0; bk.caller_max_sel = 0; bk.visited = nrec || !size ? 0u : 1u; bk.dups = 0;
    bk.nsym = 0; bk.max_sym = 0; bk.need_j = 0;
    for (u32 k = 0; k < 8; k++) bk.qmask[k] = 0;
    u32 *const wlen = w.wlen + (u64)b * w.rec_stride, *const wstart = w.wstart + (u64)b * w.rec_stride;
    if (bk.status == 0) {
        if (nrec == 0 && size && lane == 0) { wlen[0] = size; wstart[0] = 0; }          // the remainder as one record of direction 0
        const u32 *len = in.len + in.rec_off[g], *fl = in.flags + in.rec_off[g];
        u32 carry = 0, r2 = 0, msel = 0, visited = 0, first = 0;
        bool fixed = true;
        for (u32 r0 = 0; r0 < nrec; r0 += WAVE) {
            const u32 r = r0 + lane;
            const u32 l = r < nrec ? len[r] : 0u, f = r < nrec ? fl[r] : 0u;
            const u32 v = l < size ? l : size;                       // tlen never passes the size: min(sum, size) term by term
            const u64 incl = (u64)carry + wave_incl_scan(v & 0xffffu, lane) + ((u64)wave_incl_scan(v >> 16, lane) << 16);
            u32 end = (u32)(incl < size ? incl : size);
            const u32 start = (u32)(incl - v < size ? incl - v : size);
            if (r == nrec - 1u) end = size;                          // the last record takes what is left (:814-816)
            const u32 L = end - start;
            if (r < nrec) { wlen[r] = L; wstart[r] = start; }
            if (r0 == 0) first = (u32)__builtin_amdgcn_readlane((int)L, 0);
            if (__ballot(r < nrec && L != first)) fixed = false;
            if (__ballot(r < nrec && (f & FQD_FREAD2))) r2 = 1;
            msel = max(msel, fqp_wave_max(r < nrec ? f >> 16 : 0u));
            visited += (u32)__popcll(__ballot(r < nrec && start < size));
            carry = (u32)__builtin_amdgcn_readlane((int)end, WAVE - 1);
        }
        if (nrec) { bk.first_len = first; bk.fixed_len = fixed; bk.has_r2 = r2; bk.caller_max_sel = msel; bk.visited = visited; }
    }
    if (lane == 0) w.blk[b] = bk;
}

// Which record a wave of the record kernels works on: workgroup `grp` of the block's `groups`, four waves each, striding
__device__ __forceinline__ void fqp_rec_place(u32 groups, int *b, u32 *first, u32 *step)
{
    *b = (int)(blockIdx.x / groups);
    *first = (blockIdx.x % groups) * 4u + (threadIdx.x >> 6);
    *step = groups * 4u;
}

__global__ __launch_bounds__(256) void k_fqp_recs(BatchArgs a, FqpWs w, int base, u32 groups)
{
    __shared__ u32 mask[4][8];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    int b; u32 r, step;
    fqp_rec_place(groups, &b, &r, &step);
    FqpBlk *bk = w.blk + b;
    if (bk->status != 0) return;
    const u32 nw = bk->nw, size = bk->size;
    if (r >= nw) return;
    const u8 *src = a.in + a.in_off[base + b];
    const u32 *wlen = w.wlen + (u64)b * w.rec_stride, *wstart = w.wstart + (u64)b * w.rec_stride;
    u32 *wavg = w.wavg + (u64)b * w.rec_stride, *avg = w.avg + (u64)b * FQD_AVG;
    if (lane < 8) mask[wv][lane] = 0;
    wsync();
    u32 dups = 0;
    for (; r < nw; r += step) {
        const u32 L = wlen[r], s = wstart[r];
        u32 q10 = 0;
        if (s < size) {                                              // the loop over the bytes visits it (a record of 0 bytes too)
            bool dup = s > 0 && L == wlen[r - 1];                    // (s > 0: r > 0)
            u32 tot = 0;
            for (u32 t0 = 0; t0 < L; t0 += WAVE) {
                const u32 t = t0 + lane;
                if (t < L) {
                    const u32 q = src[s + t];
                    tot += q;
                    atomicOr(&mask[wv][q >> 5], 1u << (q & 31u));
                    if (dup && src[s - L + t] != q) dup = false;
                }
            }
            dup = !__ballot(!dup);
            tot = wave_sum(tot & 0xffffu) + (wave_sum(tot >> 16) << 16);             // a 32-bit sum, as the reference's
            q10 = L ? (u32)((tot * 10.0) / (int)L + .5) : 0u;
            if (lane == 0) atomicAdd(&avg[q10 < FQD_AVG - 1u ? q10 : FQD_AVG - 1u], 1u);
            dups += dup;
        }
        if (lane == 0) wavg[r] = q10;
    }
    wsync();
    if (lane < 8 && mask[wv][lane]) atomicOr(&bk->qmask[lane], mask[wv][lane]);
    if (lane == 0 && dups) atomicAdd(&bk->dups, dups);
}

// ---- (b) the thresholds ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqp_bins(FqpIn in, FqpWs w, int base, int nb)
{
    __shared__ u32 bins[4][FQD_AVG];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const int b = (int)(blockIdx.x * 4u + wv);
    if (b >= nb) return;
    FqpBlk *bk = w.blk + b;
    if (bk->status != 0) return;
    const u32 m = lane < 8 ? bk->qmask[lane] : 0u;
    const u32 nsym = wave_sum((u32)__popc(m));
    const u32 max_sym = fqp_wave_max(m ? lane * 32u + 31u - (u32)__clz(m) : 0u);
    FqdParam pm;
    fqd_strat(bk->strat, &pm);
    const bool qa = pm.do_qa != 0 || in.any_qa;
    if (lane == 0) { bk->nsym = nsym; bk->max_sym = max_sym; bk->need_j = qa || bk->has_r2 || pm.do_r2 || in.any_r2; }
    if (qa) {
        const u32 *avg = w.avg + (u64)b * FQD_AVG;
        for (u32 k = lane; k < FQD_AVG; k += WAVE) bins[wv][k] = avg[k];
        wsync();
        if (lane == 0) fqd_thresholds(bins[wv], (int)bk->nrec, (int)nsym);
        wsync();
    }
    const u32 nw = bk->nw, nrec = bk->nrec;
    const u32 *fl = in.flags + in.rec_off[base + b];
    const u32 *wavg = w.wavg + (u64)b * w.rec_stride;
    u8 *cls = w.wcls + (u64)b * w.rec_stride;
    for (u32 r = lane; r < nw; r += WAVE) {
        const u32 q10 = wavg[r], dir = nrec && (fl[r] & FQD_FREAD2) ? 1u : 0u;
        cls[r] = (u8)(dir * 4u + (qa ? bins[wv][q10 < FQD_AVG - 1u ? q10 : FQD_AVG - 1u] : 0u));
    }
}

// ---- (c) one pass over the bytes ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqp_count(BatchArgs a, FqpWs w, int base, u32 groups)
{
    const u32 lane = threadIdx.x & 63u;
    int b; u32 r, step;
    fqp_rec_place(groups, &b, &r, &step);
    const FqpBlk *bk = w.blk + b;
    if (bk->status != 0 || !bk->need_j) return;
    const u32 nw = bk->nw, size = bk->size;
    const u8 *src = a.in + a.in_off[base + b];
    const u32 *wlen = w.wlen + (u64)b * w.rec_stride, *wstart = w.wstart + (u64)b * w.rec_stride;
    const u8 *cls = w.wcls + (u64)b * w.rec_stride;
    u32 *J = w.J + (u64)b * FQP_J_CELLS;
    for (; r < nw; r += step) {
        const u32 L = wlen[r], s = wstart[r];
        if (s >= size) continue;
        u32 *rows = J + (u32)cls[r] * FQD_NP * 256u;
        for (u32 t = lane; t < L; t += WAVE) atomicAdd(&rows[((L - t) & (FQD_NP - 1u)) * 256u + src[s + t]], 1u);
    }
}

// ---- (d) the entropy sums -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqp_sums(FqpWs w)
{
    __shared__ double red[4][5];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const int b = (int)(blockIdx.x / FQP_PARTS);
    const u32 part = blockIdx.x % FQP_PARTS;
    const FqpBlk *bk = w.blk + b;
    if (bk->status != 0 || !bk->need_j) return;
    const u32 *J = w.J + (u64)b * FQP_J_CELLS;
    double e1 = 0, e2 = 0, e4 = 0, r1 = 0, r2 = 0;
    for (u32 k = 0; k < 4; k++) {
        const u32 x = part * 16u + wv * 4u + k;
        u32 cnt[8];
#pragma unroll
        for (u32 c = 0; c < 8; c++) {
            const u32 *row = J + (c * FQD_NP + x) * 256u;
            cnt[c] = wave_sum(row[lane] + row[lane + 64] + row[lane + 128] + row[lane + 192]);      // a row's total: below 2^31, the size
        }
        u32 c4[4], c2[2];
#pragma unroll
        for (u32 c = 0; c < 4; c++) c4[c] = cnt[c] + cnt[c + 4];
        c2[0] = c4[0] + c4[1]; c2[1] = c4[2] + c4[3];
        const u32 c1 = c2[0] + c2[1];
        const u32 t1 = cnt[0] + cnt[1] + cnt[2] + cnt[3], t2 = c1 - t1;
        if (!c1) continue;
        for (u32 q = lane; q < 256u; q += WAVE) {
            u32 v[8];
#pragma unroll
            for (u32 c = 0; c < 8; c++) v[c] = J[(c * FQD_NP + x) * 256u + q];
            u32 v4[4];
#pragma unroll
            for (u32 c = 0; c < 4; c++) {
                v4[c] = v[c] + v[c + 4];
                if (v4[c]) e4 += fqd_term(v4[c], c4[c]);
            }
            const u32 v20 = v4[0] + v4[1], v21 = v4[2] + v4[3], v1 = v20 + v21;
            if (v20) e2 += fqd_term(v20, c2[0]);
            if (v21) e2 += fqd_term(v21, c2[1]);
            if (v1) e1 += fqd_term(v1, c1);
            if (t1 && t2 && v1) {
                const u32 h1 = v[0] + v[1] + v[2] + v[3], h2 = v1 - h1;
                r1 += fqd_term(v1, (u64)t1 + t2);
                if (h1) r2 += fqd_term(h1, t1);
                if (h2) r2 += fqd_term(h2, t2);
            }
        }
    }
    e1 = fqp_wave_dsum(e1); e2 = fqp_wave_dsum(e2); e4 = fqp_wave_dsum(e4); r1 = fqp_wave_dsum(r1); r2 = fqp_wave_dsum(r2);
    if (lane == 0) { red[wv][0] = e1; red[wv][1] = e2; red[wv][2] = e4; red[wv][3] = r1; red[wv][4] = r2; }
    __syncthreads();
    if (threadIdx.x < 5) w.part[((u64)b * FQP_PARTS + part) * 5u + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ---- the decisions and the store ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqp_store(BatchArgs a, FqpIn in, FqpWs w, int base, int obase, int nb)
{
    const u32 lane = threadIdx.x & 63u;
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b, go = obase + b;
    const FqpBlk *bk = w.blk + b;
    int st = bk->status;
    FqdParam pm;
    FqdChoice ch = {0, 0};
    FqdStats fs;
    u32 psize = 0;
    if (st == 0) {
        FqdSums sm;
        fqp_stats_of(bk, w.part + (u64)b * FQP_PARTS * 5u, &fs, &sm);
        fqd_strat(bk->strat, &pm);
        st = fqd_decide(&pm, &fs, &sm, in.guard_bits, &ch);
    }
    const u32 nrec = bk->nrec;
    const u32 *fl = in.flags + in.rec_off[g];
    const u8 *cls = w.wcls + (u64)b * w.rec_stride;
    u8 *stage = w.par + (u64)b * FQP_STAGE;
    if (st == 0) {
        u32 fmax = 0;
        for (u32 r = lane; r < nrec; r += WAVE) fmax = max(fmax, fqd_flags(fl[r], cls[r] & 3u, &ch) >> 16);
        fmax = fqp_wave_max(fmax);
        if (lane == 0) {
            FqdSink sink = {stage, FQP_STAGE, 0u};
            st = fqd_store(&pm, &fs, &ch, in.vers, bk->strat, fmax, bk->qmask, &sink);
            psize = sink.n;                                          // (<= fqd_cap() <= FQP_STAGE)
        }
        st = __builtin_amdgcn_readfirstlane(st);
        psize = (u32)__builtin_amdgcn_readfirstlane((int)psize);
        if (st == 0 && psize > a.out_cap[go]) st = R4X16_E_CAPACITY;
    }
    if (lane == 0) {
        a.status[go] = st;
        a.out_size[go] = st == 0 || st == R4X16_E_CAPACITY ? psize : 0u;
        if (w.route) {
            if (st == 0) {
                atomicAdd(&w.route[R4X16_FQZ_PICK_BLOCKS], 1u);
                if (stage[1] & 2u) atomicAdd(&w.route[R4X16_FQZ_PICK_SEL], 1u);      // GFLAG_HAVE_STAB: written where PFLAG_DO_SEL is
                if (ch.split) atomicAdd(&w.route[R4X16_FQZ_PICK_SPLIT], 1u);
                if (pm.do_dedup) atomicAdd(&w.route[R4X16_FQZ_PICK_DEDUP], 1u);
            } else if (st == R4X16_E_UNDECIDED) atomicAdd(&w.route[R4X16_FQZ_PICK_UNDECIDED], 1u);
        }
    }
    if (st != 0) return;
    wsync();
    wave_copy(a.out + a.out_off[go], stage, psize, lane);
    const u32 *wlen = w.wlen + (u64)b * w.rec_stride;
    u32 *lo = in.len_out + in.out_rec_off[go], *fo = in.flags_out + in.out_rec_off[go];
    for (u32 r = lane; r < nrec; r += WAVE) {
        const u32 f = fqd_flags(fl[r], cls[r] & 3u, &ch);            // (fo may be fl: this lane's own entry)
        lo[r] = wlen[r];
        fo[r] = f;
    }
}

// ---- the device calls -----------------------------------------------------------------------------------------------
static size_t fqp_layout(u8 *base, size_t nb, u32 max_rec, FqpWs *w)
{
    Carver cv(base);
    w->rec_stride = (u64)max_rec + 1u;
    w->blk = cv.take<FqpBlk>(nb);
    w->route = cv.take<u32>(R4X16_FQZ_PICK_KINDS);
    w->avg = cv.take<u32>(nb * FQD_AVG);
    w->J = cv.take<u32>(nb * (size_t)FQP_J_CELLS);                   // (avg and J lie behind each other: one memset)
    w->wlen = cv.take<u32>(nb * w->rec_stride);
    w->wstart = cv.take<u32>(nb * w->rec_stride);
    w->wavg = cv.take<u32>(nb * w->rec_stride);
    w->wcls = cv.take<u8>(nb * w->rec_stride);
    w->part = cv.take<double>(nb * FQP_PARTS * 5u);
    w->par = cv.take<u8>(nb * (size_t)FQP_STAGE);
    return cv.total();
}
static u32 fqp_groups(u32 max_rec) { return std::min<u32>(FQP_REC_GROUPS, (max_rec + 1u + 3u) / 4u); }
// a chunk holds at most this many blocks: the record kernels' grids are blocks x groups
static size_t fqp_chunk_limit(u32 max_rec) { return (size_t)INT_MAX / std::max<u32>(fqp_groups(max_rec), FQP_PARTS); }

size_t r4x16_fqp_layout(u8 *base, size_t nb, u32 max_rec, FqpWs *w) { return fqp_layout(base, nb, max_rec, w); }
size_t r4x16_fqp_chunk_limit(u32 max_rec) { return fqp_chunk_limit(max_rec); }
int r4x16_fqp_stats(rans4x16_hip_ctx *c, const BatchArgs &a, const FqpIn &in, const FqpWs &w, int base, int nb, u32 max_in, u32 max_rec, hipStream_t s)
{
    const u32 groups = fqp_groups(max_rec);
    HIPCHK(c, hipMemsetAsync(w.avg, 0, (size_t)((u8 *)(w.J + (size_t)nb * FQP_J_CELLS) - (u8 *)w.avg), s));
    hipLaunchKernelGGL(k_fqp_lens, dim3((nb + 3) / 4), dim3(256), 0, s, a, in, w, base, nb, max_in, max_rec);
    hipLaunchKernelGGL(k_fqp_recs, dim3((u32)nb * groups), dim3(256), 0, s, a, w, base, groups);
    hipLaunchKernelGGL(k_fqp_bins, dim3((nb + 3) / 4), dim3(256), 0, s, in, w, base, nb);
    hipLaunchKernelGGL(k_fqp_count, dim3((u32)nb * groups), dim3(256), 0, s, a, w, base, groups);
    hipLaunchKernelGGL(k_fqp_sums, dim3((u32)nb * FQP_PARTS), dim3(256), 0, s, w);
    return 0;
}

// one chunk's pick, laid out at `at`: blocks base .. base + nb of the inputs, results at obase .. of the outputs
static int fqp_chunk(rans4x16_hip_ctx *c, const BatchArgs &a, const FqpIn &in, u8 *at, int base, int obase, int nb, u32 max_in, u32 max_rec,
                     hipStream_t s)
{
    FqpWs w;
    fqp_layout(at, (size_t)nb, max_rec, &w);
    u32 *const d_route = w.route;
    if (r4x16_route_begin(c, &w.route, R4X16_FQZ_PICK_KINDS, s) != 0) return -1;
    if (r4x16_fqp_stats(c, a, in, w, base, nb, max_in, max_rec, s) != 0) return -1;
    hipLaunchKernelGGL(k_fqp_store, dim3((nb + 3) / 4), dim3(256), 0, s, a, in, w, base, obase, nb);
    return r4x16_route_end(c, R4X16_ROUTE_FQZ_PICK, d_route, R4X16_FQZ_PICK_KINDS, s);
}

extern "C" unsigned int rans4x16_hip_fqz_pick_cap(void) { return fqd_cap(); }

extern "C" int rans4x16_hip_set_fqz_pick(rans4x16_hip_ctx *c, int mode, int guard_bits)
{
    if (!c) return -1;
    if (mode < 0 || mode > 1 || guard_bits < 0 || guard_bits > 64) { c->err = "set_fqz_pick: out of range"; return -1; }
    c->fqz_pick = mode;
    c->fqz_guard_bits = guard_bits;
    return 0;
}

extern "C" int rans4x16_hip_fqz_pick_dev(rans4x16_hip_ctx *c, int n,
                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                         const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                         int vers, int strat, const int32_t *d_strat,
                                         unsigned char *d_params, const uint64_t *d_par_off, const uint32_t *d_par_cap, uint32_t *d_par_size,
                                         uint32_t *d_len_out, uint32_t *d_flags_out, int32_t *d_status,
                                         uint32_t max_in_size, uint32_t max_records, void *stream)
{
    BatchArgs a;
    const bool ok = n <= 0 || (d_rec_off && d_nrec && max_records < 0x7fffffffu && (max_records == 0 || (d_len && d_flags && d_len_out && d_flags_out)));
    const int go = r4x16_dev_call_args(c, "fqz_pick_dev: bad arguments", ok, &a, n, d_in, d_in_off, d_in_size, d_params, d_par_off, d_par_cap,
                                       d_par_size, d_status, 0, nullptr);
    if (go <= 0) return go;
    hipStream_t s = (hipStream_t)stream;
    const FqpIn in{d_len, d_flags, d_rec_off, d_nrec, d_strat, vers, strat, c->fqz_guard_bits, d_len_out, d_flags_out, d_rec_off};
    FqpWs w;
    auto bytes_for = [&](size_t nb) { return fqp_layout(nullptr, nb, max_records, &w); };
    const size_t chunk = r4x16_fit_chunk((size_t)n, fqp_chunk_limit(max_records), r4x16_room(c, A_BIT(A_AR)), bytes_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        return fqp_chunk(c, a, in, c->at(A_AR), (int)base, (int)base, nb, max_in_size, max_records, s);
    });
}

// ---- the pick and the encoder in one call ---------------------------------------------------------------------------
// Behind a chunk's pick lie, in the arena, what the encode stages read in the caller's place: the picked parameter bytes
// (the pick's own stage is its scratch; these are its slots), lengths and flags, and the chunk's own slot arrays - a
// refused block with a parameter size no call admits, so that the front end reads nothing of it.  k_fqp_hand fills
// them, k_fqp_verdict gives every block the pick's status or the encoder's.
struct FqpHand {
    u8 *par; u64 *par_off, *rec_off, *in_off, *out_off;
    u32 *par_cap, *par_size, *nrec, *in_size, *out_cap, *out_size, *len, *flags;
    i32 *pick_status, *status;
};
static size_t fqp_hand_layout(u8 *base, size_t at, size_t nb, u32 max_rec, FqpHand *h)
{
    Carver cv(base, at);
    h->par = cv.take<u8>(nb * (size_t)FQP_STAGE);
    h->par_off = cv.take<u64>(nb); h->rec_off = cv.take<u64>(nb); h->in_off = cv.take<u64>(nb); h->out_off = cv.take<u64>(nb);
    h->par_cap = cv.take<u32>(nb); h->par_size = cv.take<u32>(nb); h->nrec = cv.take<u32>(nb); h->in_size = cv.take<u32>(nb);
    h->out_cap = cv.take<u32>(nb); h->out_size = cv.take<u32>(nb);
    h->len = cv.take<u32>(nb * ((size_t)max_rec + 1u)); h->flags = cv.take<u32>(nb * ((size_t)max_rec + 1u));
    h->pick_status = cv.take<i32>(nb); h->status = cv.take<i32>(nb);
    return cv.total();
}
__global__ void k_fqp_hand_slots(FqpHand h, int nb, u32 max_rec)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= nb) return;
    h.par_off[b] = (u64)b * FQP_STAGE; h.par_cap[b] = FQP_STAGE; h.rec_off[b] = (u64)b * ((u64)max_rec + 1u);
}
__global__ void k_fqp_hand(BatchArgs a, const u32 *nrec, const FqpBlk *blk, FqpHand h, int base, int nb)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= nb) return;
    const int g = base + b;
    const bool ok = h.pick_status[b] == 0;
    h.in_off[b] = a.in_off[g]; h.out_off[b] = a.out_off[g]; h.out_cap[b] = a.out_cap[g];
    h.in_size[b] = ok ? a.in_size[g] : 0u;
    // the records the reference's encode loop reaches: those behind the last byte (an over-running list leaves them with
    // 0 bytes) are never coded, and the encoder takes no record of 0 bytes.  (No record at all: none is handed on.)
    h.nrec[b] = ok && nrec[g] ? blk[b].visited : 0u;
    if (!ok) h.par_size[b] = 0xffffffffu;
}
__global__ void k_fqp_verdict(BatchArgs a, FqpHand h, u32 *len_out, const u64 *rec_off, const u32 *nrec, int base, int nb)
{
    const int b = (int)blockIdx.x, g = base + b;
    const bool picked = h.pick_status[b] == 0;
    if (threadIdx.x == 0) {
        a.status[g] = picked ? h.status[b] : h.pick_status[b];
        a.out_size[g] = picked ? h.out_size[b] : 0u;
    }
    if (len_out && picked)
        for (u32 r = threadIdx.x; r < nrec[g]; r += blockDim.x) len_out[rec_off[g] + r] = h.len[h.rec_off[b] + r];
}

int r4x16_fqz_compress_pick_run(rans4x16_hip_ctx *c, int n, const u8 *d_in, const u64 *d_in_off, const u32 *d_in_size, const u32 *d_len,
                                const u32 *d_flags, const u64 *d_rec_off, const u32 *d_nrec, int vers, int strat, const i32 *d_strat,
                                u8 *d_out, const u64 *d_out_off, const u32 *d_out_cap, u32 *d_out_size, i32 *d_status, u32 *d_len_out,
                                u32 max_in_size, u32 max_records, hipStream_t s)
{
    BatchArgs a;
    const bool ok = n <= 0 || (d_rec_off && d_nrec && max_records < 0x7fffffffu && (max_records == 0 || (d_len && d_flags)));
    const int go = r4x16_dev_call_args(c, "fqz_compress_pick_dev: bad arguments", ok, &a, n, d_in, d_in_off, d_in_size, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, 0, nullptr);
    if (go <= 0) return go;
    FqpWs w;
    FqpHand h;
    auto bytes_for = [&](size_t nb) {
        const size_t pick = fqp_hand_layout(nullptr, fqp_layout(nullptr, nb, max_records, &w), nb, max_records, &h);
        return pick + r4x16_fqe_chunk_bytes(c, nb, max_in_size, max_records);
    };
    const size_t chunk = r4x16_fit_chunk((size_t)n, fqp_chunk_limit(max_records), r4x16_room(c, A_BIT(A_AR)), bytes_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        u8 *const at = c->at(A_AR);
        const size_t pick = fqp_hand_layout(at, fqp_layout(nullptr, (size_t)nb, max_records, &w), (size_t)nb, max_records, &h);
        hipLaunchKernelGGL(k_fqp_hand_slots, dim3((nb + 255) / 256), dim3(256), 0, s, h, nb, max_records);
        BatchArgs pa = a;                                            // the pick's slots: the arena's
        pa.out = h.par; pa.out_off = h.par_off; pa.out_cap = h.par_cap; pa.out_size = h.par_size; pa.status = h.pick_status;
        const FqpIn in{d_len, d_flags, d_rec_off, d_nrec, d_strat, vers, strat, c->fqz_guard_bits, h.len, h.flags, h.rec_off};
        if (fqp_chunk(c, pa, in, at, (int)base, 0, nb, max_in_size, max_records, s) != 0) return -1;
        FqpWs pw;
        fqp_layout(at, (size_t)nb, max_records, &pw);
        hipLaunchKernelGGL(k_fqp_hand, dim3((nb + 255) / 256), dim3(256), 0, s, a, d_nrec, (const FqpBlk *)pw.blk, h, (int)base, nb);
        BatchArgs ea = a;                                            // the encoder's arrays: the chunk's own, from 0
        ea.in_off = h.in_off; ea.in_size = h.in_size; ea.out_off = h.out_off; ea.out_cap = h.out_cap; ea.out_size = h.out_size; ea.status = h.status;
        const FqeIn ein{h.par, h.par_off, h.par_size, h.len, h.flags, h.rec_off, h.nrec};
        if (r4x16_fqe_chunk(c, ea, ein, at + pick, 0, nb, max_in_size, FQP_STAGE, max_records, s) != 0) return -1;
        hipLaunchKernelGGL(k_fqp_verdict, dim3(nb), dim3(256), 0, s, a, h, d_len_out, d_rec_off, d_nrec, (int)base, nb);
        return 0;
    });
}

extern "C" int rans4x16_hip_fqz_compress_pick_dev(rans4x16_hip_ctx *c, int n,
                                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                  const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                                  int vers, int strat, const int32_t *d_strat,
                                                  unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                                  uint32_t *d_out_size, int32_t *d_status,
                                                  uint32_t max_in_size, uint32_t max_records, void *stream)
{
    return r4x16_fqz_compress_pick_run(c, n, d_in, d_in_off, d_in_size, d_len, d_flags, d_rec_off, d_nrec, vers, strat, d_strat, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, nullptr, max_in_size, max_records, (hipStream_t)stream);
}
