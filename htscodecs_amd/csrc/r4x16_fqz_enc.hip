// r4x16_fqz_enc.hip - encoding with htscodecs' quality codec (fqzcomp_qual.c:952-1154 compress_block_fqz2f, on
// c_simple_model.h and c_range_coder.h) on the device: include/rans4x16_hip.h part 2j.
//
// The mirror of r4x16_fqz.hip: the same serial chain, the same slots of 65,536 models, the same homes of the tables; the
// step is the arith encoder's (r4x16_arith_enc_step.h).  The parameters arrive as PARAMETER BYTES - what a stream holds
// between its size and the range coder's bytes - and the header walk (r4x16_fqz_parse.h) turns them into the flat tables,
// as it does for the decoder: what the device refuses in a stream it refuses in parameters.  The parameter choice
// (r4x16_fqz_pick.h) is the host's.  Stages:
//   k_fqe_front   one wave per block: the walk, the tables and the inverse quality maps in the stage arena, the records
//                 and every byte checked against its record's parameter block, under GFLAG_DO_REV the coder-order copy
//   k_fqe_encode  one wave per model slot, striding over the chunk's blocks: fill the slot, encode into the stage arena
//   k_fqe_back    a workgroup per block: size, parameter bytes and body into the caller's slot, the verdict
// (r4x16_fqe_stages is the first two for a caller with a back end of its own: r4x16_fqz_best.hip, which assembles only
// the smallest of a block's candidates; the work areas are declared in r4x16_fqz_best.h)
//
// Loops: the encode loop consumes at least one input byte a trip (a duplicate: `len` >= 1 bytes) and ends at the block's
// size; the front's loops run over the records (nrec <= max_records) and their bytes, whose lengths it has summed to
// the size before it reads one.  Stores: a block's stage bytes are claimed as a whole before anything is written; the
// body's room is the proven bound or the slot's capacity, whichever is smaller, plus 48, and the loop ends once the body
// has outgrown it for certain (16 bytes a trip at most, five to finish).  Only k_fqe_back writes into the caller's slot,
// after it has tested the capacity.  All stores are plain vector stores.
#include "r4x16_host.h"
#include "r4x16_fqz_best.h"
#include "r4x16_fqz_parse.h"
#include "r4x16_fqz_model.h"
#include "r4x16_fqz_pick.h"
#include "r4x16_arith_enc_step.h"

// The parameter bytes as the walk reads a stream: a size byte of 0 in front, and behind them the nine bytes a stream
// has at least (the coder's five, and the walk asks for ten behind the size).  The walk must end where the bytes end.
#define FQE_PAD 9u
struct FqeParSrc {
    const u8 *p; u32 n;
    AR_HD uint8_t at(uint32_t i) const { return i >= 1u && i - 1u < n ? p[i - 1u] : (uint8_t)0; }
};
template <class SINK>
AR_HD static inline int fqe_parse(const u8 *par, u32 psz, FqTop *top, SINK &sink)
{
    FqeParSrc src{par, psz};
    int st = fq_parse(src, psz + 1u + FQE_PAD, FQ_NO_CAP, top, sink);
    if (st == FQ_OK && top->hdr != psz + 1u) st = top->hdr > psz + 1u ? FQ_E_TRUNCATED : FQ_E_UNSUPPORTED;   // bytes missing / left over
    // several parameter blocks and no selector model: the loop would code selectors with a model never set up
    if (st == FQ_OK && (top->gflags & FQ_GFLAG_MULTI_PARAM) && top->max_sel == 0) st = FQ_E_TABLE;
    return st;
}

// the body's bound: a symbol shifts out two bytes at most, a record has seven symbols beside its qualities, five to finish
AR_HD static inline u64 fqe_body_bound(u32 size, u32 nrec) { return 2ull * ((u64)size + 7ull * nrec) + 5ull; }
AR_HD static inline u64 fqe_cap(u32 size, u32 nrec, u32 psz) { return 5ull + psz + fqe_body_bound(size, nrec); }

// ---- front ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqe_front(BatchArgs a, FqeIn in, FqeWs w, int base, int nb, u32 max_in, u32 max_par, u32 max_rec)
{
    const u32 lane = threadIdx.x & 63u;
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b;
    const u32 size = a.in_size[g], cap = a.out_cap[g], psz = in.par_size[g], nrec = in.nrec[g];
    FqTop top = {0, 0, 0, 0, 0, 0};
    int st = FQ_OK;
    u64 at = 0, inv_at = 0, cod_at = 0, out_at = 0;
    u32 lim = 0, uses_sel = 0;
    if (size > max_in || size >= FQ_REV_BIT || psz > max_par || nrec > max_rec) st = FQ_E_UNSUPPORTED;   // above what the call was sized for: not read
    else {
        const u8 *par = in.par + in.par_off[g];
        FqNoSink none;
        st = fqe_parse(par, psz, &top, none);
        if (st == FQ_OK && top.max_sym > w.max_sym) st = FQ_E_UNSUPPORTED;
        if (st == FQ_OK && size && nrec == 0) st = FQ_E_SIZE;
        if (st == FQ_OK && size) {
            const bool do_rev = (top.gflags & FQ_GFLAG_DO_REV) != 0, have_stab = (top.gflags & FQ_GFLAG_HAVE_STAB) != 0;
            const u32 hdr = fqe_var_len(size) + psz;
            const u64 room = cap > hdr ? cap - hdr : 0u, bound = fqe_body_bound(size, nrec);
            lim = (u32)(room < bound ? room : bound);                // (room <= cap: 32 bits)
            const u64 need = (u64)fq_tab_bytes(top.nparam) + 256ull * top.nparam + (do_rev ? (u64)ar_r16(size) : 0ull) + (((u64)lim + 48u + 15u) & ~15ull);
            if (lane == 0) at = atomicAdd((unsigned long long *)w.cursor, (unsigned long long)need);
            at = wave_uniform(at);
            if (at + need > w.stage_bytes) st = FQ_E_UNSUPPORTED;    // the arena holds no more parameter blocks: DESIGN 4.9
            else {
                inv_at = at + fq_tab_bytes(top.nparam);
                cod_at = inv_at + 256ull * top.nparam;
                out_at = cod_at + (do_rev ? (u64)ar_r16(size) : 0ull);
                u8 *const tab = w.stage + at;
                FqDevSink sink{tab, lane == 0};
                FqTop again;
                (void)fqe_parse(par, psz, &again, sink);
                wsync();
                // quality -> symbol of every parameter block: the stored map turned round (where it names a quality
                // twice the later symbol stands), else the identity
                for (u32 k = 0; k < top.nparam; k++) {
                    u8 *inv = w.stage + inv_at + 256ull * k;
                    const u8 *pt = tab + FQ_STAB_BYTES + k * FQ_PARAM_BYTES;
                    const FqParam pm = *(const FqParam *)pt;
                    const bool stored = (pm.pflags & FQ_PFLAG_HAVE_QMAP) != 0;
                    for (u32 q = lane; q < 256u; q += WAVE) inv[q] = stored ? (u8)0 : (u8)q;
                    wsync();
                    if (stored && lane == 0)
                        for (u32 i = 0; i < pm.max_sym; i++) inv[pt[FQ_OFF_QMAP + i]] = (u8)i;
                }
                wsync();
                uses_sel = (top.gflags & FQ_GFLAG_MULTI_PARAM) || (((const FqParam *)(tab + FQ_STAB_BYTES))->pflags & FQ_PFLAG_DO_SEL);
                const u16 *stab = (const u16 *)tab;
                const u32 *len = in.len + (in.len_off ? in.len_off : in.rec_off)[g], *fl = in.flags + in.rec_off[g];
                // the records: lengths that sum to the size, none of 0; selectors inside the model, with a parameter block
                u64 sum = 0;
                bool bad_len = false, bad_sel = false;
                for (u32 r0 = 0; r0 < nrec; r0 += WAVE) {
                    const u32 r = r0 + lane;
                    const u32 l = r < nrec ? len[r] : 0u, f = r < nrec ? fl[r] : 0u;
                    if (r < nrec) {
                        bad_len |= l == 0;
                        const u32 s = uses_sel ? f >> 16 : 0u;
                        if (s > top.max_sel && uses_sel) bad_sel = true;
                        else if ((have_stab ? (u32)stab[s < 255u ? s : 255u] : s) >= top.nparam) bad_sel = true;
                    }
                    sum += (u64)wave_sum(l & 0xffffu) + ((u64)wave_sum(l >> 16) << 16);
                }
                if (__ballot(bad_len) || sum != size) st = FQ_E_SIZE;
                else if (__ballot(bad_sel)) st = FQ_E_CONTEXT;
                if (st == FQ_OK) {
                    // every byte against its record's parameter block; the coder-order copy
                    const u8 *src = a.in + a.in_off[g];
                    u8 *cod = do_rev ? w.stage + cod_at : nullptr;
                    bool bad_q = false;
                    u32 pos = 0;
                    for (u32 r0 = 0; r0 < nrec; r0 += WAVE) {
                        const u32 r = r0 + lane;
                        const u32 l = r < nrec ? len[r] : 0u, f = r < nrec ? fl[r] : 0u;
                        const u32 s = uses_sel ? f >> 16 : 0u;
                        const u32 x = r < nrec ? (have_stab ? (u32)stab[s < 255u ? s : 255u] : s) : 0u;   // < nparam
                        const FqParam pm = *(const FqParam *)(tab + FQ_STAB_BYTES + x * FQ_PARAM_BYTES);
                        const u32 incl = wave_incl_scan(l, lane);
                        const u32 cnt = nrec - r0 < WAVE ? nrec - r0 : WAVE;
                        for (u32 k = 0; k < cnt; k++) {
                            const u32 L = (u32)__builtin_amdgcn_readlane((int)l, (int)k);
                            const u32 start = pos + (u32)__builtin_amdgcn_readlane((int)incl, (int)k) - L;
                            const u32 X = (u32)__builtin_amdgcn_readlane((int)x, (int)k);
                            const bool rev = do_rev && ((u32)__builtin_amdgcn_readlane((int)f, (int)k) & 16u);
                            const bool stored = ((u32)__builtin_amdgcn_readlane((int)pm.pflags, (int)k) & FQ_PFLAG_HAVE_QMAP) != 0;
                            const u32 pmax = (u32)__builtin_amdgcn_readlane((int)pm.max_sym, (int)k);
                            const u8 *inv = w.stage + inv_at + 256ull * X;
                            const u8 *fwd = tab + FQ_STAB_BYTES + X * FQ_PARAM_BYTES + FQ_OFF_QMAP;
                            for (u32 t = lane; t < L; t += WAVE) {
                                const u32 q = src[start + t];
                                const u32 sy = inv[q];
                                bad_q |= stored ? !(sy < pmax && fwd[sy] == q) : q > top.max_sym;
                                if (cod) cod[start + (rev ? L - 1u - t : t)] = (u8)q;
                            }
                        }
                        pos += (u32)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
                    }
                    if (__ballot(bad_q)) st = FQ_E_CONTEXT;
                }
            }
        }
    }
    if (lane == 0) {
        FqeBlk bk;
        bk.status = st; bk.size = size; bk.gflags = top.gflags; bk.nparam = top.nparam;
        bk.max_sel = top.max_sel; bk.max_sym = top.max_sym; bk.nrec = nrec;
        bk.home = st != FQ_OK || size == 0 ? FQ_HOME_NONE : top.nparam <= FQ_LDS_PARAMS ? FQ_HOME_LDS : FQ_HOME_GLOBAL;
        bk.body = 0; bk.lim = lim; bk.uses_sel = uses_sel; bk.dups = 0;
        bk.tab = at; bk.inv = inv_at; bk.cod = cod_at; bk.out = out_at;
        w.blk[b] = bk;
        if (w.route && bk.home != FQ_HOME_NONE) {
            atomicAdd(&w.route[R4X16_FQZ_ENC_STREAMS], 1u);
            atomicAdd(&w.route[bk.home == FQ_HOME_LDS ? R4X16_FQZ_ENC_TAB_LDS : R4X16_FQZ_ENC_TAB_GLOBAL], 1u);
            if (top.gflags & FQ_GFLAG_DO_REV) atomicAdd(&w.route[R4X16_FQZ_ENC_DO_REV], 1u);
            if (top.nparam > 1) atomicAdd(&w.route[R4X16_FQZ_ENC_MULTI_PARAM], 1u);
        }
    }
}

// ---- the encode loop ----------------------------------------------------------------------------------------------
// One symbol of a two-entry model (SIMPLE_MODEL(2,_encodeSymbol)): both entries in every lane's registers
__device__ __forceinline__ void fqe_bit_symbol(u32 &e0, u32 &e1, u32 bit, AreCoder &rc, u32 lane)
{
    const u32 c0 = e0 & 0xffffu, tot = c0 + (e1 & 0xffffu);
    const bool j = (e0 >> 16) != bit;
    const u32 ent = j ? e1 : e0;
    rc.encode(j ? c0 : 0u, ent & 0xffffu, tot, lane);
    u32 cur = ent + AR_STEP;
    if (j) e1 = cur; else e0 = cur;
    if (tot + AR_STEP > AR_MAX_FREQ) { e0 = ar_half(e0); e1 = ar_half(e1); cur = ar_half(cur); }
    if (j && (cur & 0xffffu) > (e0 & 0xffffu)) { e1 = e0; e0 = cur; }
}

// One symbol of a 256-entry model in LDS (the `len` and `sel` models)
__device__ __forceinline__ void fqe_lds_symbol(u32 *model, u32 &tot, u32 c, AreCoder &rc, u32 lane)
{
    u32x4 *row = (u32x4 *)model;
    u32x4 e = row[lane];
    bool dirty;
    are_symbol(e, tot, c, rc, lane, &dirty);
    if (dirty) row[lane] = e;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// TAB_LDS: the parameter blocks' tables in LDS (FQ_HOME_LDS), else read from the stage arena (FQ_HOME_GLOBAL); in LDS
// the place of a block's qmap holds its inverse.  Wave blockIdx.x owns model slot blockIdx.x and strides over the chunk's
// blocks, passing over those of the other home.
template <bool TAB_LDS>
__global__ __launch_bounds__(64) void k_fqe_encode(BatchArgs a, FqeIn in, FqeWs w, int base, int nb)
{
    __shared__ __attribute__((aligned(16))) u32 lds[(FQ_LDS_MODELS + FQ_STAB_BYTES + (TAB_LDS ? FQ_LDS_PARAMS * FQ_PARAM_BYTES : 0u)) / 4];
    const u32 lane = threadIdx.x;
    if (blockIdx.x >= w.slots) return;
    u32 *const rows = (u32 *)(w.rows + (u64)blockIdx.x * w.slot_bytes);
    u32 *const m_sel = lds + 1024;
    const u16 *const stab = (const u16 *)(lds + FQ_LDS_MODELS / 4);
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
        const FqeBlk bk = w.blk[b];
        if (bk.home != (TAB_LDS ? FQ_HOME_LDS : FQ_HOME_GLOBAL)) continue;
        const int g = base + b;
        const u32 n = bk.size;
        const u32 m = bk.max_sym + 1u, stride = ar_row_stride(m);    // stride <= the slot's (k_fqe_front's test)
        u32 *tots = rows + FQ_CTX_ROWS * stride;
        // SIMPLE_MODEL_init for every model, before every stream: the slot holds what the stream before left
        for (u32 k = lane; k < FQ_CTX_ROWS * (stride / 4u); k += WAVE) ((u32x4 *)rows)[k] = ar_fresh((4u * k) % stride, m);
        for (u32 k = lane; k < FQ_CTX_ROWS; k += WAVE) tots[k] = m;
        for (u32 k = lane; k < 1024u; k += WAVE) lds[k] = 1u | ((k & 255u) << 16);                  // len[0..3]: 256 symbols
        for (u32 k = lane; k < 256u; k += WAVE) m_sel[k] = k <= bk.max_sel ? 1u | (k << 16) : 0u;   // sel: max_sel + 1
        const u32 *tab_g = (const u32 *)(w.stage + bk.tab);
        const u32 *inv_g = (const u32 *)(w.stage + bk.inv);
        const u32 tab_words = (FQ_STAB_BYTES + (TAB_LDS ? bk.nparam * FQ_PARAM_BYTES : 0u)) / 4u;
        for (u32 k = lane; k < tab_words; k += WAVE) {
            u32 v = tab_g[k];
            if (4u * k >= FQ_STAB_BYTES) {                           // the qmap's place: the inverse
                const u32 x = (4u * k - FQ_STAB_BYTES) / FQ_PARAM_BYTES, o = (4u * k - FQ_STAB_BYTES) % FQ_PARAM_BYTES;
                if (o >= FQ_OFF_QMAP && o < FQ_OFF_QTAB) v = inv_g[x * 64u + (o - FQ_OFF_QMAP) / 4u];
            }
            lds[FQ_LDS_MODELS / 4 + k] = v;
        }
        wsync();
        const u8 *const params = TAB_LDS ? (const u8 *)(lds + (FQ_LDS_MODELS + FQ_STAB_BYTES) / 4) : w.stage + bk.tab + FQ_STAB_BYTES;
        const u8 *const data = (bk.gflags & FQ_GFLAG_DO_REV) ? w.stage + bk.cod : a.in + a.in_off[g];
        const u32 *const lens = in.len + (in.len_off ? in.len_off : in.rec_off)[g], *const fls = in.flags + in.rec_off[g];
        u32 tot_len[4] = {256u, 256u, 256u, 256u}, tot_sel = bk.max_sel + 1u;
        u32 rev0 = 1u, rev1 = 1u | (1u << 16), dup0 = 1u, dup1 = 1u | (1u << 16);
        ArWindow src(data, n);
        AreCoder rc((u32 *)(w.stage + bk.out), 0u);
        rc.out.n = 0;                                                // no alphabet byte in front of this coder's bytes
        const bool have_stab = (bk.gflags & FQ_GFLAG_HAVE_STAB) != 0, do_rev = (bk.gflags & FQ_GFLAG_DO_REV) != 0;
        const u8 *pt = params;                                       // the parameter block in use: gp.p[0] at first
        const u8 *inv = TAB_LDS ? pt + FQ_OFF_QMAP : w.stage + bk.inv;
        FqParam pm = *(const FqParam *)pt;
        u32 i = 0, rec = 0, p = 0, sel = 0, delta = 0, prevq = 0, qctx = 0, last = 0, last_len = 0, dups = 0;
        bool first_len = true, over = false;
        while (i < n) {
            if (rc.sure() > bk.lim) { over = true; break; }          // the body has outgrown the slot for certain
            if (p == 0) {                                            // a record starts (:1041-1104); rec < nrec: the lengths sum to n
                const u32 len = lens[rec], fl = fls[rec];
                sel = 0;
                if (bk.uses_sel) { sel = fl >> 16; fqe_lds_symbol(m_sel, tot_sel, sel, rc, lane); }
                const u32 x = have_stab ? stab[sel < 255u ? sel : 255u] : sel;      // < nparam (k_fqe_front's test)
                pt = params + x * FQ_PARAM_BYTES;
                inv = TAB_LDS ? pt + FQ_OFF_QMAP : w.stage + bk.inv + 256u * x;
                pm = *(const FqParam *)pt;
                if (!(pm.pflags & FQ_PFLAG_DO_LEN) || first_len) {
#pragma unroll
                    for (u32 k = 0; k < 4; k++) fqe_lds_symbol(lds + 256u * k, tot_len[k], (len >> (8u * k)) & 0xffu, rc, lane);
                    first_len = false;
                }
                if (do_rev) fqe_bit_symbol(rev0, rev1, (fl >> 4) & 1u, rc, lane);
                rec++;
                p = len; delta = 0; prevq = 0; qctx = 0;
                last = pm.context;
                if (pm.pflags & FQ_PFLAG_DO_DEDUP) {
                    bool dup = i != 0 && len == last_len && len <= i;
                    for (u32 k0 = 0; dup && k0 < len; k0 += WAVE) {
                        const u32 k = k0 + lane;
                        if (__ballot(k < len && data[i + k] != data[i - len + k])) dup = false;
                    }
                    fqe_bit_symbol(dup0, dup1, dup ? 1u : 0u, rc, lane);
                    if (dup) { i += len; p = 0; dups++; continue; }
                    last_len = len;
                }
            }
            // the quality: row `last` of the slot
            const u32 Q = inv[src.byte(i, lane)];
            u32x4 *row = (u32x4 *)(rows + last * stride);
            const bool mine = 4u * lane < stride;
            u32x4 e = mine ? row[lane] : u32x4{0, 0, 0, 0};
            u32 tot = tots[last];
            bool dirty;
            are_symbol(e, tot, Q, rc, lane, &dirty);
            if (dirty && mine) row[lane] = e;
            if (lane == 0) tots[last] = tot;
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
        if (!over) rc.finish(lane);
        if (lane == 0) {
            w.blk[b].body = rc.out.n;
            w.blk[b].dups = dups;
            if (over) w.blk[b].status = FQ_E_CAPACITY;
        }
        wsync();                                                     // the next stream's models overwrite these
    }
}

// ---- back -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqe_back(BatchArgs a, FqeIn in, FqeWs w, int base)
{
    const int b = (int)blockIdx.x, g = base + b;
    const u32 t = threadIdx.x;
    const FqeBlk bk = w.blk[b];
    const u32 psz = in.par_size[g], vl = fqe_var_len(bk.size);
    const u32 body = bk.size ? bk.body : 5u;                         // (nothing to code: RC_FinishEncode's five zero bytes)
    const u64 total = (u64)vl + psz + body;
    const int st = bk.status != FQ_OK ? bk.status : total > a.out_cap[g] ? (int)FQ_E_CAPACITY : (int)FQ_OK;
    if (t == 0) {
        a.status[g] = st; a.out_size[g] = st == FQ_OK ? (u32)total : 0u;
        // counted here, not by the wave: a stream whose closing bytes outgrow the slot is refused only now
        if (w.route && st == FQ_OK && bk.dups) atomicAdd(&w.route[R4X16_FQZ_ENC_DUP], 1u);
    }
    if (st != FQ_OK) return;
    u8 *dst = a.out + a.out_off[g];
    if (t < vl) dst[t] = (u8)(((bk.size >> (7u * (vl - 1u - t))) & 0x7fu) | (t + 1u < vl ? 0x80u : 0u));   // var_put_u32
    group_copy<256>(dst + vl, in.par + in.par_off[g], psz, t);
    if (bk.size) group_copy<256>(dst + vl + psz, w.stage + bk.out, body, t);
    else if (t < 5u) dst[vl + psz + t] = 0;
}

// ---- the device call ----------------------------------------------------------------------------------------------
static size_t fqe_layout(u8 *base, size_t nb, u64 stage_bytes, size_t slots, u64 slot_bytes, FqeWs *w)
{
    Carver cv(base);
    w->cursor = cv.take<u64>(1);
    w->blk = cv.take<FqeBlk>(nb);
    w->route = cv.take<u32>(R4X16_FQZ_ENC_KINDS);
    w->stage = cv.take<u8>(stage_bytes);
    w->stage_bytes = stage_bytes;
    w->rows = cv.take<u8>(slots * slot_bytes);
    w->slot_bytes = slot_bytes;
    w->slots = (u32)slots;
    return cv.total();
}

// One chunk of nb blocks, blocks base .. base + nb of the arrays in `a` and `in`, laid out at `at` (r4x16_host.h: the
// device call below, and the one-call form of r4x16_fqz_pick.hip behind its pick).  The stage arena: a selector table a
// block, room for four parameter blocks a block with their inverse maps (256, one block's most, at least), and a block's
// coder-order copy and its body at the bound.
static size_t fqe_chunk_layout(rans4x16_hip_ctx *c, u8 *at, size_t nb, u32 max_in_size, u32 max_records, FqeWs *w)
{
    const u64 slot_bytes = fq_slot_bytes((u32)c->fqz_max_sym);
    const size_t max_slots = c->fqz_slots > 0 ? (size_t)c->fqz_slots : (size_t)FQ_MAX_SLOTS;
    const u64 per_block = (u64)ar_r16(max_in_size) + ((fqe_body_bound(max_in_size, max_records) + 48u + 15u) & ~15ull) + 64u;
    const u64 stage = (u64)nb * FQ_STAB_BYTES + (u64)std::max<size_t>(4 * nb, 256) * (FQ_PARAM_BYTES + 256u) + (u64)nb * per_block;
    return fqe_layout(at, nb, stage, std::min(nb, max_slots), slot_bytes, w);
}
size_t r4x16_fqe_chunk_bytes(rans4x16_hip_ctx *c, size_t nb, u32 max_in_size, u32 max_records)
{
    FqeWs w;
    return fqe_chunk_layout(c, nullptr, nb, max_in_size, max_records, &w);
}
int r4x16_fqe_stages(rans4x16_hip_ctx *c, const BatchArgs &a, const FqeIn &in, u8 *at, int base, int nb, u32 max_in_size, u32 max_params_size,
                     u32 max_records, hipStream_t s, FqeWs *w, u32 **d_route)
{
    fqe_chunk_layout(c, at, (size_t)nb, max_in_size, max_records, w);
    w->max_sym = (u32)c->fqz_max_sym;
    *d_route = w->route;
    HIPCHK(c, hipMemsetAsync(w->cursor, 0, sizeof(u64), s));
    if (r4x16_route_begin(c, &w->route, R4X16_FQZ_ENC_KINDS, s) != 0) return -1;
    hipLaunchKernelGGL(k_fqe_front, dim3((nb + 3) / 4), dim3(256), 0, s, a, in, *w, base, nb, max_in_size, max_params_size, max_records);
    hipLaunchKernelGGL(k_fqe_encode<true>, dim3(w->slots), dim3(64), 0, s, a, in, *w, base, nb);
    hipLaunchKernelGGL(k_fqe_encode<false>, dim3(w->slots), dim3(64), 0, s, a, in, *w, base, nb);
    return 0;
}
int r4x16_fqe_chunk(rans4x16_hip_ctx *c, const BatchArgs &a, const FqeIn &in, u8 *at, int base, int nb, u32 max_in_size, u32 max_params_size,
                    u32 max_records, hipStream_t s)
{
    FqeWs w;
    u32 *d_route;
    if (r4x16_fqe_stages(c, a, in, at, base, nb, max_in_size, max_params_size, max_records, s, &w, &d_route) != 0) return -1;
    hipLaunchKernelGGL(k_fqe_back, dim3(nb), dim3(256), 0, s, a, in, w, base);
    return r4x16_route_end(c, R4X16_ROUTE_FQZ_ENC, d_route, R4X16_FQZ_ENC_KINDS, s);
}

extern "C" unsigned int rans4x16_hip_fqz_compress_cap(unsigned int size, unsigned int nrec, unsigned int params_size)
{
    const u64 v = fqe_cap(size, nrec, params_size);
    return v > 0xffffffffull ? 0xffffffffu : (unsigned int)v;
}

extern "C" int rans4x16_hip_fqz_compress_dev(rans4x16_hip_ctx *c, int n,
                                             const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                             const unsigned char *d_params, const uint64_t *d_par_off, const uint32_t *d_par_size,
                                             const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                             unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                             uint32_t *d_out_size, int32_t *d_status,
                                             uint32_t max_in_size, uint32_t max_params_size, uint32_t max_records, void *stream)
{
    BatchArgs a;
    const bool ok = n <= 0 || (d_params && d_par_off && d_par_size && d_rec_off && d_nrec && (max_records == 0 || (d_len && d_flags)));
    const int go = r4x16_dev_call_args(c, "fqz_compress_dev: bad arguments", ok, &a, n, d_in, d_in_off, d_in_size, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, 0, nullptr);
    if (go <= 0) return go;
    hipStream_t s = (hipStream_t)stream;
    const FqeIn in{d_params, d_par_off, d_par_size, d_len, d_flags, d_rec_off, d_nrec};
    auto bytes_for = [&](size_t nb) { return r4x16_fqe_chunk_bytes(c, nb, max_in_size, max_records); };
    const size_t chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX, r4x16_room(c, A_BIT(A_AR)), bytes_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        return r4x16_fqe_chunk(c, a, in, c->at(A_AR), (int)base, nb, max_in_size, max_params_size, max_records, s);
    });
}

// ---- the parameter choice on host memory --------------------------------------------------------------------------
extern "C" int rans4x16_hip_fqz_pick_parameters(int vers, int strat, int nrec, uint32_t *len, uint32_t *flags,
                                                const unsigned char *in, size_t in_size,
                                                unsigned char *params, unsigned int params_cap, unsigned int *params_size)
{
    if (params_size) *params_size = 0;
    // the caller's slice changes only with the bytes it gets
    std::vector<uint32_t> L, F;
    std::vector<uint8_t> out;
    const int st = fqp_pick(vers, strat, nrec, len, flags, in, in_size, out, L, F);
    if (st != FQP_OK) return st;
    if (params_size) *params_size = (unsigned int)out.size();
    if (out.size() > params_cap || !params) return R4X16_E_CAPACITY;
    memcpy(params, out.data(), out.size());
    for (int i = 0; i < nrec; i++) { len[i] = L[i]; flags[i] = F[i]; }
    return 0;
}

// ---- host buffers: the trip with the device pick (rans4x16_hip_set_fqz_pick mode 1) -------------------------------
// The blocks of `todo` in one round trip of their own: behind the inputs go the places of the records (8 bytes each),
// the record counts, the lengths and the flags (4 bytes each); behind the outputs come the lengths as the pick left
// them.  A block the device pick leaves undecided goes back into todo with its capacity, for the host; every other
// block of the trip is done, whatever its status.  The model slots are as rans4x16_hip_set_fqz_limits sized them: the
// pick's max_sym is not known here.
static int fqe_pick_trip(rans4x16_hip_ctx *c, int n, const unsigned char *const *in, const unsigned int *in_size, const unsigned int *nrec,
                         uint32_t *const *len, uint32_t *const *flags, int vers, int strat, unsigned char *const *out, unsigned int *out_size,
                         int *status, std::vector<int> &todo, std::vector<u8> &done)
{
    const size_t N = (size_t)n;
    std::vector<u32> isz(n, 0), cap(n, 0), nr(n, 0);
    std::vector<u8> take(n, 0);
    u32 max_in = 0, max_rec = 0;
    u64 nrecs = 0;
    for (int i : todo) {
        take[i] = 1; isz[i] = in_size[i]; cap[i] = out_size[i]; nr[i] = nrec[i];
        max_in = std::max(max_in, isz[i]); max_rec = std::max(max_rec, nr[i]);
        nrecs += nr[i];
    }
    std::vector<u8> tail(12 * N + 8 * (size_t)nrecs, 0), back;
    u64 *const t_rec_off = (u64 *)tail.data();
    u32 *const t_nrec = (u32 *)(t_rec_off + N), *const t_len = t_nrec + N, *const t_flags = t_len + nrecs;
    u64 at_rec = 0;
    for (int i = 0; i < n; i++) {
        t_rec_off[i] = at_rec;
        if (!take[i]) continue;
        t_nrec[i] = nr[i];
        if (nr[i]) { memcpy(t_len + at_rec, len[i], 4 * (size_t)nr[i]); memcpy(t_flags + at_rec, flags[i], 4 * (size_t)nr[i]); }
        at_rec += nr[i];
    }
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), nullptr, tail.data(), tail.size(), 4 * (size_t)nrecs, &back};
    const int rc = r4x16_host_trip(c, n, trip, [&](const StageLayout &L, size_t in_total, size_t out_total, hipStream_t s) {
        const u8 *d_tail = L.in + in_total;
        const u64 *d_rec_off = (const u64 *)d_tail;
        const u32 *d_nrec = (const u32 *)(d_rec_off + N), *d_len = d_nrec + N, *d_flags = d_len + nrecs;
        return r4x16_fqz_compress_pick_run(c, n, L.in, L.in_off, L.in_size, d_len, d_flags, d_rec_off, d_nrec, vers, strat, nullptr, L.out,
                                           L.out_off, L.cap, L.osz, L.status, (u32 *)(L.out + out_total), max_in, max_rec, s);
    });
    if (rc < 0) return -1;
    std::vector<int> host;
    for (int i : todo) {
        if (status[i] == R4X16_E_UNDECIDED) { status[i] = 0; out_size[i] = cap[i]; host.push_back(i); continue; }
        done[i] = 1;
        if (status[i] == 0 && nr[i] && back.size() >= 4 * (size_t)nrecs) memcpy(len[i], back.data() + 4 * t_rec_off[i], 4 * (size_t)nr[i]);
    }
    if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_FQZ_PICK][R4X16_FQZ_PICK_HOST] += (long)host.size();
    todo.swap(host);
    return 0;
}

// ---- host buffers -------------------------------------------------------------------------------------------------
// The blocks without parameter bytes are picked on the host first (a few threads: the picks do not depend on each
// other).  Then one round trip (r4x16_host_trip): behind the inputs go the places and sizes of the parameter bytes and
// the records, the lengths, the flags and the parameter bytes.  The model slots are sized for the batch's largest
// max_sym, which the host walk knows; the caller's limit is put back.
extern "C" int rans4x16_hip_fqz_compress_batch(rans4x16_hip_ctx *c, int n,
                                               const unsigned char *const *in, const unsigned int *in_size,
                                               const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags,
                                               int vers, int strat,
                                               const unsigned char *const *params, const unsigned int *params_size,
                                               unsigned char *const *out, unsigned int *out_size, int *status)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !nrec || !len || !flags || !out || !out_size || !status)) || (params && !params_size)) {
        c->err = "fqz_compress_batch: bad arguments";
        return -1;
    }
    if (n == 0) return 0;
    std::vector<std::vector<uint8_t>> picked(n);
    std::vector<const u8 *> par(n, nullptr);
    std::vector<u32> psz(n, 0);
    std::vector<u8> done(n, 0);                                      // coded by the trip with the device pick
    // the picks
    {
        std::vector<int> todo;
        for (int i = 0; i < n; i++) {
            status[i] = 0;
            if ((!in[i] && in_size[i]) || !out[i] || (nrec[i] && (!len[i] || !flags[i])) || nrec[i] > 0x7fffffffu) status[i] = R4X16_E_UNSUPPORTED;
            else if (params && params[i]) { par[i] = params[i]; psz[i] = params_size[i]; }
            else todo.push_back(i);
        }
        // rans4x16_hip_set_fqz_pick mode 1: one trip picks and codes them on the device; what it leaves undecided the host picks
        if (c->fqz_pick == 1 && !todo.empty() && fqe_pick_trip(c, n, in, in_size, nrec, len, flags, vers, strat, out, out_size, status, todo, done) != 0) return -1;
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (size_t k; (k = next.fetch_add(1)) < todo.size();) {
                const int i = todo[k];
                std::vector<uint32_t> L, F;
                status[i] = fqp_pick(vers, strat, (int)nrec[i], len[i], flags[i], in[i], in_size[i], picked[i], L, F);
                if (status[i] == FQP_OK) for (u32 r = 0; r < nrec[i]; r++) { len[i][r] = L[r]; flags[i][r] = F[r]; }
                par[i] = picked[i].data(); psz[i] = (u32)picked[i].size();
            }
        };
        const size_t nthreads = std::min<size_t>({todo.size(), (size_t)std::max(1u, std::thread::hardware_concurrency()), (size_t)8});
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nthreads; t++) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
    std::vector<u32> isz(n, 0), cap(n, 0), nr(n, 0);
    std::vector<u8> take(n, 0);
    u32 max_in = 0, max_par = 0, max_rec = 0, max_sym = 0;
    u64 nrecs = 0, par_bytes = 0;
    for (int i = 0; i < n; i++) {
        FqTop top;
        FqNoSink none;
        if (done[i]) continue;
        if (status[i] == 0) status[i] = fqe_parse(par[i], psz[i], &top, none);
        if (status[i] != 0) { out_size[i] = 0; continue; }
        take[i] = 1; isz[i] = in_size[i]; cap[i] = out_size[i];
        nr[i] = in_size[i] ? nrec[i] : 0u;                            // (nothing to code: the records are not read)
        max_in = std::max(max_in, isz[i]); max_par = std::max(max_par, psz[i]); max_rec = std::max(max_rec, nr[i]);
        max_sym = std::max(max_sym, top.max_sym);
        nrecs += nr[i]; par_bytes += psz[i];
    }
    // the tail: [n] places of the parameter bytes, [n] places of the records (8 bytes each), [n] sizes of the parameter
    // bytes, [n] record counts, the lengths, the flags (4 bytes each), the parameter bytes
    const size_t N = (size_t)n;
    std::vector<u8> tail(24 * N + 8 * (size_t)nrecs + (size_t)par_bytes, 0);
    u64 *const t_par_off = (u64 *)tail.data(), *const t_rec_off = t_par_off + N;
    u32 *const t_par_size = (u32 *)(t_rec_off + N), *const t_nrec = t_par_size + N, *const t_len = t_nrec + N, *const t_flags = t_len + nrecs;
    u8 *const t_par = (u8 *)(t_flags + nrecs);
    u64 at_rec = 0, at_par = 0;
    for (int i = 0; i < n; i++) {
        t_par_off[i] = at_par; t_rec_off[i] = at_rec;
        if (!take[i]) continue;
        t_par_size[i] = psz[i]; t_nrec[i] = nr[i];
        if (nr[i]) { memcpy(t_len + at_rec, len[i], 4 * (size_t)nr[i]); memcpy(t_flags + at_rec, flags[i], 4 * (size_t)nr[i]); }
        if (psz[i]) memcpy(t_par + at_par, par[i], psz[i]);
        at_rec += nr[i]; at_par += psz[i];
    }
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), nullptr, tail.data(), tail.size(), 0, nullptr};
    int bad = r4x16_host_trip(c, n, trip, [&](const StageLayout &L, size_t in_total, size_t, hipStream_t s) {
        Keep<int> limit(c->fqz_max_sym, (int)std::max(max_sym, 1u));
        const u8 *d_tail = L.in + in_total;                          // (in_total: a multiple of 16 in an arena aligned to 256)
        const u64 *d_par_off = (const u64 *)d_tail, *d_rec_off = d_par_off + N;
        const u32 *d_par_size = (const u32 *)(d_rec_off + N), *d_nrec = d_par_size + N, *d_len = d_nrec + N, *d_flags = d_len + nrecs;
        return rans4x16_hip_fqz_compress_dev(c, n, L.in, L.in_off, L.in_size, (const u8 *)(d_flags + nrecs), d_par_off, d_par_size,
                                             d_len, d_flags, d_rec_off, d_nrec, L.out, L.out_off, L.cap, L.osz, L.status,
                                             max_in, max_par, max_rec, s);
    });
    // the reference clears the selectors it kept in the flags (:1142-1144)
    for (int i = 0; i < n; i++)
        if (len[i] && flags[i]) for (u32 r = 0; r < nrec[i]; r++) flags[i][r] &= 0xffffu;
    if (bad >= 0 && std::find(done.begin(), done.end(), 1) != done.end()) bad = (int)(n - std::count(status, status + n, 0));
    return bad;
}

// ---- the reference's call (fqzcomp_qual.h), on the calling thread's context ---------------------------------------
extern "C" char *rans4x16_hip_fqz_compress(int vers, rans4x16_hip_fqz_slice *s, char *in, size_t in_size, size_t *out_size, int strat,
                                           struct rans4x16_hip_fqz_gparams *gp)
{
    if (gp || !s || !out_size || (!in && in_size) || in_size >= FQ_REV_BIT || s->num_records < 0) return nullptr;
    if (in_size && s->num_records == 0) return nullptr;              // (the reference reads s->len[0]: undefined)
    const unsigned int nrec = (unsigned int)s->num_records;
    unsigned int psz = 0;
    std::vector<unsigned char> par(4096);
    int st = rans4x16_hip_fqz_pick_parameters(vers, strat, s->num_records, s->len, s->flags, (const unsigned char *)in, in_size, par.data(),
                                              (unsigned int)par.size(), &psz);
    if (st == R4X16_E_CAPACITY) {
        par.resize(psz);
        st = rans4x16_hip_fqz_pick_parameters(vers, strat, s->num_records, s->len, s->flags, (const unsigned char *)in, in_size, par.data(), psz, &psz);
    }
    if (st != 0) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    const unsigned int cap = rans4x16_hip_fqz_compress_cap((unsigned int)in_size, nrec, psz);
    unsigned char *buf = (unsigned char *)malloc(cap);
    if (!buf) return nullptr;
    unsigned char none = 0;
    const unsigned char *ins[1] = {in ? (const unsigned char *)in : &none}, *pars[1] = {par.data()};
    unsigned char *outs[1] = {buf};
    unsigned int isz[1] = {(unsigned int)in_size}, nr[1] = {nrec}, ps[1] = {psz}, osz[1] = {cap};
    uint32_t *lens[1] = {s->len}, *fls[1] = {s->flags};
    int sts[1] = {0};
    const int rc = rans4x16_hip_fqz_compress_batch(c, 1, ins, isz, nr, lens, fls, vers, strat, pars, ps, outs, osz, sts);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || sts[0] != 0) { free(buf); return nullptr; }
    *out_size = osz[0];
    return (char *)buf;
}
