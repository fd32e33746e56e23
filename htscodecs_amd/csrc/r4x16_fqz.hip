// r4x16_fqz.hip - decoding of htscodecs' quality codec (fqzcomp_qual.c, on c_simple_model.h and c_range_coder.h) on the
// device: include/rans4x16_hip.h part 2i.
//
// A stream is one serial chain: every base is one step of an adaptive model picked by a 16-bit context that the bases
// before it made.  The parallelism is the arith decoder's (r4x16_arith.hip) - the model's list across the wave, one wave
// per stream - and so is the step (r4x16_arith_step.h, on r4x16_arith_model.h).  What is new is the size of the state: up to 65,536 models a
// stream, held in a slot of the context's arena, and the per-record machinery around the step.  Stages:
//   k_fq_front   one wave per block: the header walk (r4x16_fqz_parse.h), the block's flat tables and, under
//                GFLAG_DO_REV, its record table claimed from the stage arena
//   k_fq_plan    one wave per chunk: the blocks in order against total_out_size, the routes, and the verdicts of the
//                blocks that decode nothing
//   k_fq_decode  one wave per model slot, striding over the chunk's blocks: fill the slot, decode, reverse, verdict
//
// Homes, slots, the reversal rule and the arithmetic behind the budgets: DESIGN 4.8, profiles/fqz.md.
//
// Loops: the decode loop writes at least one output byte a trip (a duplicate: `len` >= 1 bytes) and ends at the stored
// size, which k_fq_front checked against the slot's capacity and max_out_size; the reversal walks the records the loop
// counted, whose lengths sum to the stored size.  All stores are plain vector stores.
#include "r4x16_host.h"
#include "r4x16_fqz_parse.h"
#include "r4x16_arith_step.h"
#include "r4x16_fqz_model.h"

struct FqBlk {
    i32 status; u32 out_size, hdr, gflags;
    u32 nparam, max_sel, max_sym, home;
    u64 tab;                // in the stage arena: the selector table, then nparam x FQ_PARAM_BYTES
    u64 rec;                // in the stage arena: the record table, out_size entries (GFLAG_DO_REV only)
};
struct FqLens { u32 *len; const u64 *off; const u32 *cap; u32 *nrec; };     // the four nullable arguments
struct FqWs {
    FqBlk *blk;             // [nb]
    u64 *cursor;            // [0] bytes of the stage arena handed out (a chunk's); [1] bytes the call's blocks decode to so far
    u32 *route;             // [R4X16_FQZ_KINDS]; nullptr in the kernels' copy: option route_count is off
    u8 *stage;
    u64 stage_bytes;
    u64 out_total;          // total_out_size
    u8 *rows;               // [slots] x slot_bytes
    u64 slot_bytes;
    u32 slots, max_sym;     // model slots in flight; the largest max_sym a slot holds
};

// ---- front ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fq_front(BatchArgs a, FqWs w, int base, int nb, u32 max_in, u32 max_out)
{
    const u32 lane = threadIdx.x & 63u;
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b;
    const u32 size = a.in_size[g], cap = a.out_cap[g];
    FqTop top = {0, 0, 0, 0, 0, 0};
    int st;
    u64 at = 0, rec = 0;
    if (size > max_in) st = FQ_E_UNSUPPORTED;                       // larger than the call was sized for: not read
    else {
        // the walk twice: once for the verdict and the sizes, and - with its place in the arena known - for the tables
        ByteSrc src(a.in + a.in_off[g]);
        FqNoSink none;
        st = fq_parse(src, size, cap, &top, none);
        if (st == FQ_OK && (top.out_size > max_out || top.out_size >= FQ_REV_BIT || top.max_sym > w.max_sym)) st = FQ_E_UNSUPPORTED;
        if (st == FQ_OK && top.out_size) {
            const u64 rec_bytes = (top.gflags & FQ_GFLAG_DO_REV) ? ((u64)top.out_size * 4u + 15u) & ~15ull : 0ull;
            const u64 need = fq_tab_bytes(top.nparam) + rec_bytes;
            if (lane == 0) at = atomicAdd((unsigned long long *)w.cursor, (unsigned long long)need);
            at = wave_uniform(at);
            if (at + need > w.stage_bytes) st = FQ_E_UNSUPPORTED;    // the arena holds no more parameter blocks: DESIGN 4.8
            else {
                rec = at + fq_tab_bytes(top.nparam);
                FqDevSink sink{w.stage + at, lane == 0};
                FqTop again;
                (void)fq_parse(src, size, cap, &again, sink);
            }
        }
    }
    if (lane == 0) {
        FqBlk bk;
        bk.status = st; bk.out_size = st == FQ_OK ? top.out_size : 0u; bk.hdr = top.hdr; bk.gflags = top.gflags;
        bk.nparam = top.nparam; bk.max_sel = top.max_sel; bk.max_sym = top.max_sym;
        bk.home = st != FQ_OK || top.out_size == 0 ? FQ_HOME_NONE : top.nparam <= FQ_LDS_PARAMS ? FQ_HOME_LDS : FQ_HOME_GLOBAL;
        bk.tab = at; bk.rec = rec;
        w.blk[b] = bk;
    }
}

// The chunk's blocks in their order: a batch that decodes to more than it announced does not fit, and the blocks that
// find the total spent are refused (a refused block's claim on the total stays taken).  Blocks that decode nothing get
// their verdicts here; the others from the wave that decodes them.
__global__ __launch_bounds__(64) void k_fq_plan(BatchArgs a, FqWs w, FqLens ln, int base, int nb)
{
    __shared__ u32 sz[WAVE];
    __shared__ u32 ok[WAVE];
    const u32 lane = threadIdx.x;
    u64 sum = w.cursor[1];
    for (int b0 = 0; b0 < nb; b0 += WAVE) {
        const int b = b0 + (int)lane;
        FqBlk bk;
        bk.status = -1; bk.out_size = 0; bk.home = FQ_HOME_NONE;
        if (b < nb) bk = w.blk[b];
        sz[lane] = bk.status == FQ_OK ? bk.out_size : 0u;
        wsync();
        if (lane == 0)
            for (u32 k = 0; k < WAVE; k++) { sum += sz[k]; ok[k] = sum <= w.out_total; }
        wsync();
        sum = wave_uniform(sum);
        if (b < nb) {
            if (bk.status == FQ_OK && !ok[lane]) {
                bk.status = FQ_E_UNSUPPORTED; bk.home = FQ_HOME_NONE;
                w.blk[b].status = bk.status; w.blk[b].home = bk.home;
            }
            if (bk.home == FQ_HOME_NONE) {
                a.status[base + b] = bk.status; a.out_size[base + b] = 0;
                if (ln.nrec) ln.nrec[base + b] = 0;
            } else if (w.route) {
                atomicAdd(&w.route[R4X16_FQZ_STREAMS], 1u);
                atomicAdd(&w.route[bk.home == FQ_HOME_LDS ? R4X16_FQZ_TAB_LDS : R4X16_FQZ_TAB_GLOBAL], 1u);
                if (bk.gflags & FQ_GFLAG_DO_REV) atomicAdd(&w.route[R4X16_FQZ_DO_REV], 1u);
                if (bk.nparam > 1) atomicAdd(&w.route[R4X16_FQZ_MULTI_PARAM], 1u);
            }
        }
        wsync();
    }
    if (lane == 0) w.cursor[1] = sum;
}

// ---- the decode loop ----------------------------------------------------------------------------------------------
// One symbol of a two-entry model (SIMPLE_MODEL(2,_decodeSymbol)): both entries in every lane's registers
__device__ __forceinline__ u32 fq_bit_symbol(u32 &e0, u32 &e1, ArCoder &rc, u32 lane)
{
    const u32 c0 = e0 & 0xffffu, tot = c0 + (e1 & 0xffffu);
    const u32 freq = rc.get_freq(tot);
    if (freq > AR_MAX_FREQ || freq >= tot) return 0;
    const bool j = c0 <= freq;
    const u32 ent = j ? e1 : e0;
    rc.decode(j ? c0 : 0u, ent & 0xffffu, lane);
    u32 cur = ent + AR_STEP;
    if (j) e1 = cur; else e0 = cur;
    if (tot + AR_STEP > AR_MAX_FREQ) { e0 = ar_half(e0); e1 = ar_half(e1); cur = ar_half(cur); }
    if (j && (cur & 0xffffu) > (e0 & 0xffffu)) { e1 = e0; e0 = cur; }
    return ent >> 16;
}

// One symbol of a 256-entry model in LDS (the `len` and `sel` models)
__device__ __forceinline__ u32 fq_lds_symbol(u32 *model, u32 &tot, ArCoder &rc, u32 lane)
{
    u32x4 *row = (u32x4 *)model;
    u32x4 e = row[lane];
    bool dirty;
    const u32 c = ar_symbol(e, tot, rc, lane, &dirty);
    if (dirty) row[lane] = e;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return c;
}

// TAB_LDS: the parameter blocks' tables in LDS (FQ_HOME_LDS), else read from the stage arena (FQ_HOME_GLOBAL).  Wave
// blockIdx.x owns model slot blockIdx.x and strides over the chunk's blocks, passing over those of the other home.
template <bool TAB_LDS>
__global__ __launch_bounds__(64) void k_fq_decode(BatchArgs a, FqWs w, FqLens ln, int base, int nb)
{
    __shared__ __attribute__((aligned(16))) u32 lds[(FQ_LDS_MODELS + FQ_STAB_BYTES + (TAB_LDS ? FQ_LDS_PARAMS * FQ_PARAM_BYTES : 0u)) / 4];
    const u32 lane = threadIdx.x;
    if (blockIdx.x >= w.slots) return;
    u32 *const rows = (u32 *)(w.rows + (u64)blockIdx.x * w.slot_bytes);
    u32 *const m_sel = lds + 1024;
    const u16 *const stab = (const u16 *)(lds + FQ_LDS_MODELS / 4);
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
        const FqBlk bk = w.blk[b];
        if (bk.home != (TAB_LDS ? FQ_HOME_LDS : FQ_HOME_GLOBAL)) continue;
        const int g = base + b;
        const u8 *src = a.in + a.in_off[g];
        u8 *dst = a.out + a.out_off[g];
        const u32 n = bk.out_size;                                   // <= the slot's capacity (the walk's test)
        const u32 m = bk.max_sym + 1u, stride = ar_row_stride(m);    // stride <= the slot's (k_fq_front's test)
        u32 *tots = rows + FQ_CTX_ROWS * stride;
        // SIMPLE_MODEL_init for every model, before every stream: the slot holds what the stream before left
        for (u32 k = lane; k < FQ_CTX_ROWS * (stride / 4u); k += WAVE) {
            const u32 s = (4u * k) % stride;
            u32x4 v;
            v.x = s < m ? 1u | (s << 16) : 0u; v.y = s + 1 < m ? 1u | ((s + 1) << 16) : 0u;
            v.z = s + 2 < m ? 1u | ((s + 2) << 16) : 0u; v.w = s + 3 < m ? 1u | ((s + 3) << 16) : 0u;
            ((u32x4 *)rows)[k] = v;
        }
        for (u32 k = lane; k < FQ_CTX_ROWS; k += WAVE) tots[k] = m;
        for (u32 k = lane; k < 1024u; k += WAVE) lds[k] = 1u | ((k & 255u) << 16);                  // len[0..3]: 256 symbols
        for (u32 k = lane; k < 256u; k += WAVE) m_sel[k] = k <= bk.max_sel ? 1u | (k << 16) : 0u;   // sel: max_sel + 1
        const u32 *tab_g = (const u32 *)(w.stage + bk.tab);
        const u32 tab_words = (FQ_STAB_BYTES + (TAB_LDS ? bk.nparam * FQ_PARAM_BYTES : 0u)) / 4u;
        for (u32 k = lane; k < tab_words; k += WAVE) lds[FQ_LDS_MODELS / 4 + k] = tab_g[k];
        wsync();
        const u8 *const params = TAB_LDS ? (const u8 *)(lds + (FQ_LDS_MODELS + FQ_STAB_BYTES) / 4) : w.stage + bk.tab + FQ_STAB_BYTES;
        u32 *const rtab = (u32 *)(w.stage + bk.rec);
        u32 tot_len[4] = {256u, 256u, 256u, 256u}, tot_sel = bk.max_sel + 1u;
        u32 rev0 = 1u, rev1 = 1u | (1u << 16), dup0 = 1u, dup1 = 1u | (1u << 16);
        ArCoder rc(src + bk.hdr - 1u, a.in_size[g] - bk.hdr + 1u, lane);       // the coder's input starts at byte hdr (hdr >= 10)
        const bool have_stab = (bk.gflags & FQ_GFLAG_HAVE_STAB) != 0, do_rev = (bk.gflags & FQ_GFLAG_DO_REV) != 0;
        const u32 len_cap = ln.len ? ln.cap[g] : 0u;
        u32 *const lens = ln.len ? ln.len + ln.off[g] : nullptr;
        const u8 *pt = params;                                       // the parameter block in use: gp.p[0] at first
        FqParam pm = *(const FqParam *)pt;
        u32 i = 0, rec = 0, p = 0, sel = 0, delta = 0, prevq = 0, qctx = 0, last = 0, last_len = 0, dups = 0;
        bool first_len = true;
        int st = FQ_OK;
        while (i < n) {
            if (p == 0) {                                            // a record starts (:1370-1431)
                sel = (pm.pflags & FQ_PFLAG_DO_SEL) ? fq_lds_symbol(m_sel, tot_sel, rc, lane) : 0u;
                const u32 x = have_stab ? stab[sel < 255u ? sel : 255u] : sel;
                if (x >= bk.nparam) { st = FQ_E_CONTEXT; break; }
                pt = params + x * FQ_PARAM_BYTES;
                pm = *(const FqParam *)pt;
                u32 len = last_len;
                if (!(pm.pflags & FQ_PFLAG_DO_LEN) || first_len) {
                    len = 0;
#pragma unroll
                    for (u32 k = 0; k < 4; k++) len |= fq_lds_symbol(lds + 256u * k, tot_len[k], rc, lane) << (8u * k);
                    first_len = false;
                    last_len = len;
                }
                if (len > n - i || len == 0) { st = FQ_E_SIZE; break; }
                if (rec < len_cap && lane == 0) lens[rec] = len;
                if (do_rev) {
                    const u32 rev = fq_bit_symbol(rev0, rev1, rc, lane);
                    if (lane == 0) rtab[rec] = len | (rev ? FQ_REV_BIT : 0u);
                }
                if ((pm.pflags & FQ_PFLAG_DO_DEDUP) && fq_bit_symbol(dup0, dup1, rc, lane)) {
                    if (len > i) { st = FQ_E_SIZE; break; }
                    wsync();                                         // the bytes before i, as decoded
                    for (u32 k = lane; k < len; k += WAVE) dst[i + k] = dst[i - len + k];
                    wsync();
                    i += len;
                    rec++; dups++;
                    continue;                                        // p stays 0: the next record starts
                }
                rec++;
                p = len; delta = 0; prevq = 0; qctx = 0;
                last = pm.context;
            }
            // the quality: row `last` of the slot
            u32x4 *row = (u32x4 *)(rows + last * stride);
            const bool mine = 4u * lane < stride;
            u32x4 e = mine ? row[lane] : u32x4{0, 0, 0, 0};
            u32 tot = tots[last];
            bool dirty;
            const u32 Q = ar_symbol(e, tot, rc, lane, &dirty) & 0xffu;
            if (dirty && mine) row[lane] = e;
            if (lane == 0) { tots[last] = tot; dst[i] = pt[FQ_OFF_QMAP + Q]; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next step's row may be this one
            i++;
            // fqz_update_ctx (:367-411)
            qctx = (qctx << pm.qshift) + ((const u16 *)(pt + FQ_OFF_QTAB))[Q];
            last = (qctx & pm.qmask) << pm.qloc;
            last += ((const u16 *)(pt + FQ_OFF_PTAB))[p < 1023u ? p : 1023u];
            last += ((const u16 *)(pt + FQ_OFF_DTAB))[delta < 255u ? delta : 255u];
            last += sel << pm.sloc;
            last &= FQ_CTX_ROWS - 1u;
            delta += prevq != Q;
            prevq = Q;
            p--;
        }
        wsync();
        if (st == FQ_OK && do_rev) {
            // the records marked reversed, in place, now that no duplicate reads them any more (:1453-1467): 64 records a
            // trip, a short one by its lane, a long one by the wave
            u32 pos = 0;
            for (u32 r0 = 0; r0 < rec; r0 += WAVE) {
                const u32 v = r0 + lane < rec ? rtab[r0 + lane] : 0u;
                const u32 len = v & ~FQ_REV_BIT;
                const u32 incl = wave_incl_scan(len, lane);
                u8 *cp = dst + pos + (incl - len);
                const bool rev = (v & FQ_REV_BIT) != 0;
                if (rev && len <= 32u)
                    for (u32 I = 0, J = len - 1u; I < J; I++, J--) { const u8 t = cp[I]; cp[I] = cp[J]; cp[J] = t; }
                u64 big = __ballot(rev && len > 32u);
                while (big) {
                    const int L = (int)__builtin_ctzll(big);
                    big &= big - 1;
                    const u32 bl = (u32)__builtin_amdgcn_readlane((int)len, L);
                    u8 *bp = dst + pos + ((u32)__builtin_amdgcn_readlane((int)incl, L) - bl);
                    for (u32 I = lane; I < bl / 2u; I += WAVE) { const u8 t = bp[I]; bp[I] = bp[bl - 1u - I]; bp[bl - 1u - I] = t; }
                }
                pos += (u32)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
            }
        }
        if (lane == 0) {
            a.status[g] = st; a.out_size[g] = st == FQ_OK ? n : 0u;
            if (ln.nrec) ln.nrec[g] = st == FQ_OK ? rec : 0u;
            if (w.route && st == FQ_OK && dups) atomicAdd(&w.route[R4X16_FQZ_DUP], 1u);
        }
        wsync();                                                     // the next stream's models overwrite these
    }
}

// ---- the device call ----------------------------------------------------------------------------------------------
static size_t fq_layout(u8 *base, size_t nb, u64 stage_bytes, size_t slots, u64 slot_bytes, FqWs *w)
{
    Carver cv(base);
    w->cursor = cv.take<u64>(2);                                    // first: the call's count keeps its place from chunk to chunk
    w->blk = cv.take<FqBlk>(nb);
    w->route = cv.take<u32>(R4X16_FQZ_KINDS);
    w->stage = cv.take<u8>(stage_bytes);
    w->stage_bytes = stage_bytes;
    w->rows = cv.take<u8>(slots * slot_bytes);
    w->slot_bytes = slot_bytes;
    w->slots = (u32)slots;
    return cv.total();
}

extern "C" int rans4x16_hip_set_fqz_limits(rans4x16_hip_ctx *c, int max_slots, int max_sym)
{
    if (!c) return -1;
    if (max_slots < 0 || max_slots > FQ_MAX_SLOTS || max_sym < 0 || max_sym > 255) { c->err = "set_fqz_limits: out of range"; return -1; }
    c->fqz_slots = max_slots;
    c->fqz_max_sym = max_sym ? max_sym : 255;
    return 0;
}

extern "C" int rans4x16_hip_fqz_uncompress_dev(rans4x16_hip_ctx *c, int n,
                                               const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                               unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                               uint32_t *d_out_size, int32_t *d_status,
                                               uint32_t *d_len, const uint64_t *d_len_off, const uint32_t *d_len_cap, uint32_t *d_nrec,
                                               uint32_t max_in_size, uint32_t max_out_size, uint64_t total_out_size, void *stream)
{
    BatchArgs a;
    const int go = r4x16_dev_call_args(c, "fqz_uncompress_dev: bad arguments", !d_len || (d_len_off && d_len_cap), &a, n, d_in, d_in_off,
                                       d_in_size, d_out, d_out_off, d_out_cap, d_out_size, d_status, 0, nullptr);
    if (go <= 0) return go;
    hipStream_t s = (hipStream_t)stream;
    const u64 total = total_out_size ? total_out_size : (u64)n * max_out_size;
    const u64 slot_bytes = fq_slot_bytes((u32)c->fqz_max_sym);
    const size_t max_slots = c->fqz_slots > 0 ? (size_t)c->fqz_slots : (size_t)FQ_MAX_SLOTS;
    FqWs w;
    // the stage arena: a selector table a block and room for four parameter blocks a block (256, one stream's most, at
    // least), and a record table as long as the output for the blocks under GFLAG_DO_REV - which only the device knows
    auto layout = [&](u8 *at, size_t nb) {
        const u64 tot = std::min<u64>(total, (u64)nb * max_out_size);
        const u64 stage = (u64)nb * FQ_STAB_BYTES + (u64)std::max<size_t>(4 * nb, 256) * FQ_PARAM_BYTES + 4ull * tot + 16ull * nb;
        return fq_layout(at, nb, stage, std::min(nb, max_slots), slot_bytes, &w);
    };
    auto bytes_for = [&](size_t nb) { return layout(nullptr, nb); };
    const size_t chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX, r4x16_room(c, A_BIT(A_AR)), bytes_for);
    const FqLens ln{d_len, d_len_off, d_len_cap, d_nrec};
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        if (base == 0) HIPCHK(c, hipMemsetAsync(c->at(A_AR), 0, 2 * sizeof(u64), s));
        layout(c->at(A_AR), (size_t)nb);
        w.out_total = total;
        w.max_sym = (u32)c->fqz_max_sym;
        u32 *const d_route = w.route;
        HIPCHK(c, hipMemsetAsync(w.cursor, 0, sizeof(u64), s));
        if (r4x16_route_begin(c, &w.route, R4X16_FQZ_KINDS, s) != 0) return -1;
        hipLaunchKernelGGL(k_fq_front, dim3((nb + 3) / 4), dim3(256), 0, s, a, w, (int)base, nb, max_in_size, max_out_size);
        hipLaunchKernelGGL(k_fq_plan, dim3(1), dim3(64), 0, s, a, w, ln, (int)base, nb);
        hipLaunchKernelGGL(k_fq_decode<true>, dim3(w.slots), dim3(64), 0, s, a, w, ln, (int)base, nb);
        hipLaunchKernelGGL(k_fq_decode<false>, dim3(w.slots), dim3(64), 0, s, a, w, ln, (int)base, nb);
        return r4x16_route_end(c, R4X16_ROUTE_FQZ, d_route, R4X16_FQZ_KINDS, s);
    });
}

// the stored size of every block: the varint at byte 0 (there is no flag byte in this format)
__global__ __launch_bounds__(256) void k_fq_peek(int n, const u8 *in, const u64 *in_off, const u32 *in_size, u32 *raw, i32 *status, u32 max_in)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const u32 size = in_size[i];
    u32 v = 0;
    int st = FQ_OK;
    if (size == 0) st = FQ_E_EMPTY;
    else if (size > max_in) st = FQ_E_UNSUPPORTED;
    else {
        ByteSrc src(in + in_off[i]);
        const u32 used = ar_var_get(src, 0, size, &v);
        if (src.at(used - 1u) & 0x80u) { st = FQ_E_TRUNCATED; v = 0; }   // the varint runs past the block
    }
    raw[i] = v;
    status[i] = st;
}

extern "C" int rans4x16_hip_fqz_peek_dev(rans4x16_hip_ctx *c, int n,
                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                         uint32_t *d_raw_size, int32_t *d_status, uint32_t max_in_size, void *stream)
{
    if (!c) return -1;
    if (n < 0 || (n && (!d_in || !d_in_off || !d_in_size || !d_raw_size || !d_status))) { c->err = "fqz_peek_dev: bad arguments"; return -1; }
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_fq_peek, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_in, d_in_off, d_in_size, d_raw_size,
                       d_status, max_in_size);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- the walk on host memory --------------------------------------------------------------------------------------
extern "C" int rans4x16_hip_fqz_scan(const unsigned char *in, unsigned int in_size, uint32_t *stored_size, uint32_t *header_bytes,
                                     uint32_t *gflags, uint32_t *nparam, uint32_t *max_sel, uint32_t *max_sym)
{
    FqTop top = {0, 0, 0, 0, 0, 0};
    HostSrc src{in};
    FqNoSink none;
    const int st = in ? fq_parse(src, in_size, FQ_NO_CAP, &top, none) : (int)FQ_E_EMPTY;
    if (stored_size) *stored_size = top.out_size;
    if (header_bytes) *header_bytes = top.hdr;
    if (gflags) *gflags = top.gflags;
    if (nparam) *nparam = top.nparam;
    if (max_sel) *max_sel = top.max_sel;
    if (max_sym) *max_sym = top.max_sym;
    return st;
}

// ---- host buffers -------------------------------------------------------------------------------------------------
// One round trip (r4x16_host_trip): behind the streams go the places of the lengths, behind the outputs come the record
// counts and the lengths.  The model slots are sized for the batch's largest max_sym, which the host walk knows; the
// caller's limit is put back.
extern "C" int rans4x16_hip_fqz_uncompress_batch(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *const *in, const unsigned int *in_size,
                                                 unsigned char *const *out, unsigned int *out_size, int *status,
                                                 int *const *lengths, const int *nlengths, unsigned int *nrec)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !out || !out_size || !status)) || (lengths && !nlengths)) {
        c->err = "fqz_uncompress_batch: bad arguments";
        return -1;
    }
    if (n == 0) return 0;
    std::vector<u32> isz(n, 0), cap(n, 0);
    std::vector<u8> take(n, 0), places(12 * (size_t)n, 0), tail;     // places: [n] offsets (8 bytes), [n] capacities (4) of the lengths
    u64 *const len_off = (u64 *)places.data();
    u32 *const len_cap = (u32 *)(places.data() + 8 * (size_t)n);
    u32 max_in = 0, max_out = 0, max_sym = 0;
    u64 nlen = 0;
    for (int i = 0; i < n; i++) {
        HostSrc src{in[i]};
        FqTop top;
        FqNoSink none;
        status[i] = in[i] && out[i] ? fq_parse(src, in_size[i], out_size[i], &top, none) : R4X16_E_UNSUPPORTED;
        if (nrec) nrec[i] = 0;
        if (status[i] != FQ_OK) { out_size[i] = 0; continue; }
        take[i] = 1; isz[i] = in_size[i]; cap[i] = out_size[i];
        max_in = std::max(max_in, isz[i]); max_out = std::max(max_out, cap[i]); max_sym = std::max(max_sym, top.max_sym);
        if (lengths && lengths[i] && nlengths[i] > 0) { len_off[i] = nlen; len_cap[i] = (u32)nlengths[i]; nlen += len_cap[i]; }
    }
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), nullptr,
                           places.data(), places.size(), 4 * (size_t)n + 4 * (size_t)nlen, &tail};
    const int bad = r4x16_host_trip(c, n, trip, [&](const StageLayout &L, size_t in_total, size_t out_total, hipStream_t s) {
        Keep<int> limit(c->fqz_max_sym, (int)max_sym);
        u32 *const d_nrec = (u32 *)(L.out + out_total);
        return rans4x16_hip_fqz_uncompress_dev(c, n, L.in, L.in_off, L.in_size, L.out, L.out_off, L.cap, L.osz, L.status,
                                               d_nrec + n, (const u64 *)(L.in + in_total), (const u32 *)(L.in + in_total + 8 * (size_t)n), d_nrec,
                                               max_in, max_out, out_total, s);
    });
    if (bad < 0 || tail.empty()) return bad;                        // (empty: nothing was taken)
    const u32 *h_nrec = (const u32 *)tail.data();
    for (int i = 0; i < n; i++)
        if (take[i] && status[i] == 0) {
            if (nrec) nrec[i] = h_nrec[i];
            // the reference's lengths[rec] = len for rec < nlengths: the entries behind the last record stay as they were
            if (len_cap[i]) memcpy(lengths[i], h_nrec + n + len_off[i], 4 * (size_t)std::min(h_nrec[i], len_cap[i]));
        }
    return bad;
}

// ---- the reference's call (fqzcomp_qual.h), on the calling thread's context ---------------------------------------
extern "C" char *rans4x16_hip_fqz_decompress(char *in, size_t comp_size, size_t *uncomp_size, int *lengths, int nlengths)
{
    if (!in || !uncomp_size || comp_size > 0xffffffffull) return nullptr;
    HostSrc src{(const u8 *)in};
    FqTop top;
    FqNoSink none;
    const int st = fq_parse(src, (u32)comp_size, FQ_NO_CAP, &top, none);
    *uncomp_size = top.out_size;                                     // :1301: set before anything can fail
    if (st != FQ_OK) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    unsigned char *buf = (unsigned char *)malloc(top.out_size);      // (a stored size of 0: malloc(0), as the reference)
    if (!buf) return nullptr;
    if (top.out_size == 0) return (char *)buf;                       // the loop never runs: nothing is decoded
    const unsigned char *ins[1] = {(const unsigned char *)in};
    unsigned char *outs[1] = {buf};
    unsigned int isz[1] = {(unsigned int)comp_size}, osz[1] = {top.out_size};
    int sts[1] = {0};
    int *lens[1] = {lengths};
    const int nl[1] = {nlengths};
    const int rc = rans4x16_hip_fqz_uncompress_batch(c, 1, ins, isz, outs, osz, sts, lengths ? lens : nullptr, nl, nullptr);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || sts[0] != 0) { free(buf); return nullptr; }
    return (char *)buf;
}
