// r4x16_arith_enc.hip - encoding with htscodecs' adaptive arithmetic codec (arith_dynamic.c:621-863 arith_compress_to, the
// four core coders, c_simple_model.h, c_range_coder.h) on the device: include/rans4x16_hip.h part 2h.
//
// The mirror of r4x16_arith.hip.  The model layout, the three homes of the models, the input window and the byte writer
// are r4x16_arith_model.h's, shared with the decoder; the call's walk over chunks and the host round trip r4x16_host.h's.
// Stages:
//   k_are_front   one wave per block: what arith_compress_to decides before it codes - the flag rules, the items (one for
//                 a plain block; for an X_STRIPE block every candidate method of every plane), the transposition, hts_pack,
//                 the alphabet byte - and the items' places in the stage arena
//   k_are_encode  one wave per item: the models and the range coder (the hot loop); an item ends early once it cannot
//                 come out smaller than its input, which the reference stores (X_CAT)
//   k_are_back    a workgroup per block: the reference's bytes in the caller's slot - flag byte, sizes, pack map, body;
//                 for a stripe block the first smallest candidate of every plane
// Best of k (rans4x16_hip_arith_compress_best_packed_dev, the end of this file): a chunk's blocks go through these three
// kernels once, as k items each with the method as the item's order word, into slots of this unit's own; k_ab_pick takes
// the smallest, k_pk_scan lays the winners out and k_ab_gather copies each to its place.
// The step, the early end and the capacity rule: DESIGN 4.7.
//
// Loops: the encode loop consumes an input byte a trip, the run loop three bytes of a run a trip; the flush of pending 0xFF
// bytes runs over bytes counted before; the front's loops run over the block's bytes (size <= max_in_size) or its planes
// (<= 255).  Stores: an item's stage slots hold its length rounded up to 16, plus 16 for the coded body, and are claimed
// as a whole before anything is written; the coded body is cut off at the input's length (the early end), five closing
// bytes at most behind it.  All stores are plain vector stores.
#include "r4x16_host.h"
#include "r4x16_best_any.h"
#include "r4x16_arith_parse.h"
#include "r4x16_arith_enc_step.h"

enum { ARE_NONE = 0, ARE_CODE = 1, ARE_STORED = 2 };
#define ARE_CANDS 3u                             // candidate methods a plane has at most (arith_dynamic.c:690-693)
#define ARE_META 28u                             // size varint 5, pack map 17, packed length 5

struct AreItem {
    u64 src;                // the bytes to code: in d_in, or in the stage arena (src_stage)
    u64 out;                // the coded body in the stage arena: 16-byte aligned, n rounded up to 16, plus 16
    u32 n;                  // bytes to code (after packing)
    u32 body;               // bytes of the coded body, the alphabet byte included (k_are_encode)
    u8 flags;               // the flag byte as the front resolved it; the fall-back to X_CAT is the back's
    u8 state;               // ARE_*
    u8 home;                // R4X16_ARITH_ENC_O0 / _O1_LDS / _O1_GLOBAL
    u8 m;                   // the alphabet byte: the largest byte + 1 (0 means 256)
    u8 src_stage, nmeta, rle, pad;
    u8 meta[ARE_META];      // behind the flag byte: the size unless X_NOSZ, the pack map, the packed length
};
struct AreBlk { i32 status; u32 nplanes, flags, size; };          // nplanes 0: a plain block (item 0)
struct AreWs {
    AreItem *items;         // [nb * per]: block b's items from b * per, candidate c of plane j at j * ARE_CANDS + c
    AreBlk *blk;            // [nb]
    u64 *cursor;            // bytes of the stage arena handed out (a chunk's)
    u32 *route;             // [R4X16_ARITH_ENC_KINDS]; nullptr in the kernels' copy: option route_count is off
    u8 *stage;
    u64 stage_bytes;
    u8 *rows;               // [AR_GLOBAL_SLOTS] x AR_GLOBAL_ROW_BYTES
    u32 per;                // items a block reserves: 1, or ARE_CANDS x planes
    u32 planes;             // planes a stripe block may have (0: stripe blocks report UNSUPPORTED)
};

// candidate c of plane j (:690-693), -1 past the last
__host__ __device__ static inline int are_method(u32 j, u32 c)
{
    if (c == 0) return 1;
    if (j == 0) return c == 1 ? 64 : c == 2 ? 0 : -1;
    if (c > 1) return -1;
    return j == 1 ? 0 : 128;
}
// what of the order word decides before any byte is read: 0, or the status of a block that is refused
__host__ __device__ static inline int are_order_check(u32 size, int order, u32 *nplanes)
{
    *nplanes = 0;
    if ((order & AR_X_STRIPE) && size > 20) {
        const u32 N = (u32)order >> 8 ? (u32)order >> 8 : 4u;
        if (N > 255) return AR_E_UNSUPPORTED;                        // :648: the reference's NULL
        *nplanes = N;
        return AR_OK;
    }
    return (order & AR_X_EXT) ? AR_E_UNSUPPORTED : AR_OK;            // bzip2: a reference built without it
}
__host__ __device__ static inline u32 are_cap(u32 size, int order)
{
    u32 N;
    // a plain block: flag 1, size 5, pack map 17, packed length 5.  A stripe block: flag, size, N; a plane its length (5) and,
    // where method 1 is among its candidates (an odd order), at most the flag and the bytes themselves; under an even
    // order a plane from the third on has X_PACK alone and may carry the map and the packed length as well
    if (are_order_check(size, order, &N) == AR_OK && N) return size + 7u + ((order & 1) ? 6u : 28u) * N;
    return size + 28u;
}
// stage bytes of one plane of len bytes coded as candidates [0, nc): its copy (a stripe block's), its packed form, the bodies
__host__ __device__ static inline u64 are_plane_need(u32 len, bool copy, bool pack, u32 nc)
{
    return (copy ? (u64)ar_r16(len) : 0ull) + (pack ? (u64)ar_r16((len + 1u) / 2u) : 0ull) + (u64)nc * ((u64)ar_r16(len) + 16u);
}

// ---- front ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 wave_max(u32 v)
{
    for (int o = 32; o; o >>= 1) { const u32 x = (u32)__shfl_xor((int)v, o); v = x > v ? x : v; }
    return v;
}

struct ArePlane {           // wave-uniform
    const u8 *raw; u32 len, max_raw;
    u64 raw_at; bool raw_stage;
    u32 nsym;               // hts_pack's count (0: not looked at)
    u64 pk_at; u32 pk_len, max_pk;
    u8 map[16];
};

// The plane's bytes: read at in[x * stride], copied to `copy` (or nullptr), their maximum, and under `seen` the symbols
// that occur.  All lanes.
__device__ static u32 are_scan(const u8 *in, u32 stride, u32 len, u8 *copy, u32 *seen, u32 lane)
{
    u32 mx = 0;
    for (u32 x = lane; x < len; x += WAVE) {
        const u32 c = in[(size_t)x * stride];
        mx = c > mx ? c : mx;
        if (copy) copy[x] = (u8)c;
        if (seen) seen[c] = 1u;
    }
    return wave_max(mx);
}

// hts_pack (pack.c:56-151) of P.raw into dst: seen[] holds the symbols that occur and becomes symbol -> code
__device__ static void are_pack(ArePlane &P, u8 *dst, u32 *seen, u32 lane)
{
    u32 n = 0;
    for (u32 q = 0; q < 4; q++) {
        const u32 s = q * WAVE + lane;
        const bool p = seen[s] != 0;
        const u64 mask = __ballot(p);
        const u32 rank = n + (u32)__popcll(mask & ((1ull << lane) - 1ull));
        n += (u32)__popcll(mask);
        wsync();
        seen[s] = rank;
        // (the map's entries: lane-uniform registers, so each is read from the lane that found it)
        for (u32 k = 0; k < 16; k++) {
            const u64 at = __ballot(p && rank == k);
            if (at) P.map[k] = (u8)(q * WAVE + (u32)__builtin_ctzll(at));
        }
    }
    wsync();
    P.nsym = n;
    P.pk_len = 0; P.max_pk = 0;
    if (n > 16 || n <= 1) return;
    const u32 per = n > 4 ? 2u : n > 2 ? 4u : 8u, bits = 8u / per;
    P.pk_len = (P.len + per - 1) / per;
    u32 mx = 0;
    for (u32 k = lane; k < P.pk_len; k += WAVE) {
        u32 b = 0;
        for (u32 t = 0; t < per; t++) { const u32 x = k * per + t; if (x < P.len) b |= seen[P.raw[x]] << (bits * t); }
        dst[k] = (u8)b;
        mx = b > mx ? b : mx;
    }
    P.max_pk = wave_max(mx);
}

__device__ __forceinline__ u32 are_var_len(u32 v)
{
    u32 groups = 1;
    for (u32 t = v >> 7; t; t >>= 7) groups++;
    return groups;
}
__device__ __forceinline__ u32 are_var_put(u8 *cp, u32 v)
{
    const u32 groups = are_var_len(v);
    for (u32 g = groups; g-- > 0;) *cp++ = (u8)(((v >> (7u * g)) & 0x7fu) | (g ? 0x80u : 0u));
    return groups;
}

// One candidate: plane P under `order` (a plain block's order word, a plane's method | X_NOSZ), as :760-811 resolve it.
// Lane 0 writes the item; every lane gets its state.
__device__ static u32 are_item(AreItem *dst, const ArePlane &P, u32 order, u64 in_base, u64 out_at, u32 lane, u32 *route)
{
    AreItem it;
    u32 flags = order & 0xffu, ord = order & 3u, n = P.len, nm = 0;
    it.src = P.raw_stage ? P.raw_at : in_base; it.src_stage = P.raw_stage;
    u32 mx = P.max_raw;
    if (!(flags & AR_X_NOSZ)) nm += are_var_put(it.meta + nm, P.len);
    if ((flags & AR_X_PACK) && P.len) {
        if (P.nsym > 16 && P.nsym != 256) flags &= ~(u32)AR_X_PACK;
        else if (P.nsym == 256) { it.meta[nm++] = 0; nm += are_var_put(it.meta + nm, P.len); }   // the count byte wraps: the flag stays
        else {
            it.meta[nm++] = (u8)P.nsym;
            for (u32 k = 0; k < P.nsym; k++) it.meta[nm++] = P.map[k];
            n = P.pk_len; mx = P.max_pk;
            nm += are_var_put(it.meta + nm, n);
            it.src = P.pk_at; it.src_stage = 1;
        }
    } else flags &= ~(u32)AR_X_PACK;
    if ((flags & AR_X_RLE) && !n) flags &= ~(u32)AR_X_RLE;
    if (ord && n < 8) { flags &= ~3u; ord = 0; }
    it.n = n; it.body = 0; it.out = out_at;
    it.flags = (u8)flags; it.nmeta = (u8)nm; it.pad = 0;
    it.m = (u8)(n ? mx + 1u : 1u);
    it.rle = (flags & AR_X_RLE) != 0;
    const u32 m = it.m ? it.m : 256u;
    it.home = ord == 1 ? (ar_lds_home(m) ? R4X16_ARITH_ENC_O1_LDS : R4X16_ARITH_ENC_O1_GLOBAL) : R4X16_ARITH_ENC_O0;
    it.state = (flags & AR_X_CAT) ? ARE_STORED : ARE_CODE;          // an explicit X_CAT stores the bytes
    for (u32 k = nm; k < ARE_META; k++) it.meta[k] = 0;
    if (lane == 0) {
        *dst = it;
        if (route) {
            if (it.state == ARE_STORED) atomicAdd(&route[R4X16_ARITH_ENC_STORED], 1u);
            else {
                atomicAdd(&route[it.home], 1u);
                if (it.rle) atomicAdd(&route[R4X16_ARITH_ENC_RLE], 1u);
            }
        }
    }
    return it.state;
}

__global__ __launch_bounds__(256) void k_are_front(BatchArgs a, AreWs w, int base, int nb, u32 max_in)
{
    __shared__ u32 seen_all[4][256];
    const u32 lane = threadIdx.x & 63u;
    u32 *seen = seen_all[threadIdx.x >> 6];
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b;
    const u32 size = a.in_size[g], cap = a.out_cap[g];
    const int order = a.d_order ? a.d_order[g] : a.order;
    AreItem *items = w.items + (size_t)b * w.per;
    u32 N = 0;
    int st = size > max_in ? AR_E_UNSUPPORTED : are_order_check(size, order, &N);
    if (st == AR_OK && N > w.planes) st = AR_E_UNSUPPORTED;                          // more planes than the call reserved
    if (st == AR_OK && cap < are_cap(size, order)) st = AR_E_CAPACITY;
    // the block's stage bytes, from its size and its order word alone, claimed before anything is written
    const u32 even = (order & 3) == 0;
    u64 need = 0;
    if (st == AR_OK) {
        if (!N) need = are_plane_need(size, false, (order & AR_X_PACK) != 0, 1);
        else for (u32 j = 0; j < N; j++) {
            const u32 len = size / N + ((size % N) > j);
            u32 nc = 0;
            for (u32 c = 0; c < ARE_CANDS; c++) { const int mt = are_method(j, c); nc += mt >= 0 && !(even && (mt & 1)); }
            need += are_plane_need(len, true, j >= 2, nc);
        }
    }
    u64 at = 0;
    if (st == AR_OK && lane == 0) at = atomicAdd((unsigned long long *)w.cursor, (unsigned long long)need);
    at = wave_uniform(at);
    if (st == AR_OK && at + need > w.stage_bytes) st = AR_E_UNSUPPORTED;             // (the arena holds what the host sized it for)
    u32 live = 0;
    if (st == AR_OK) {
        const u8 *in = a.in + a.in_off[g];
        const u32 P_n = N ? N : 1u;
        live = N ? N * ARE_CANDS : 1u;
        for (u32 j = 0; j < P_n; j++) {
            ArePlane P;
            P.len = N ? size / N + ((size % N) > j) : size;
            P.nsym = 0; P.pk_at = 0; P.pk_len = 0; P.max_pk = 0;
            for (u32 k = 0; k < 16; k++) P.map[k] = 0;
            bool pack = false;
            if (!N) pack = (order & AR_X_PACK) != 0 && size != 0;
            else pack = j >= 2 && P.len != 0;
            if (pack) { for (u32 k = lane; k < 256; k += WAVE) seen[k] = 0; wsync(); }
            P.raw_stage = N != 0;
            P.raw_at = at;
            u8 *copy = N ? w.stage + at : nullptr;
            P.max_raw = are_scan(in + (N ? j : 0u), N ? N : 1u, P.len, copy, pack ? seen : nullptr, lane);
            if (N) at += ar_r16(P.len);
            wsync();                                                                 // the copy and the symbols seen, before they are read
            P.raw = N ? copy : in;
            if (!N ? (order & AR_X_PACK) != 0 : j >= 2) {
                P.pk_at = at;
                if (pack) are_pack(P, w.stage + at, seen, lane);
                at += ar_r16((P.len + 1u) / 2u);
                wsync();
            }
            if (!N) { are_item(items, P, (u32)order & ~(u32)AR_X_STRIPE, a.in_off[g], at, lane, w.route); break; }   // (:634: 20 bytes and fewer are not striped)
            for (u32 c = 0; c < ARE_CANDS; c++) {
                const int mt = are_method(j, c);
                AreItem *dst = items + (size_t)j * ARE_CANDS + c;
                if (mt < 0 || (even && (mt & 1))) { if (lane == 0) dst->state = ARE_NONE; continue; }
                are_item(dst, P, (u32)mt | AR_X_NOSZ, 0, at, lane, w.route);
                at += ar_r16(P.len) + 16u;
            }
        }
    }
    for (u32 j = live + lane; j < w.per; j += WAVE) items[j].state = ARE_NONE;
    if (lane == 0) {
        AreBlk bk;
        bk.status = st; bk.nplanes = st == AR_OK ? N : 0u; bk.flags = (u32)order & 0xffu & ~(u32)AR_X_NOSZ; bk.size = size;
        w.blk[b] = bk;
    }
}

// ---- the step ---------------------------------------------------------------------------------------------------
// The range coder and the symbol step: r4x16_arith_enc_step.h, shared with r4x16_fqz_enc.hip.

// One symbol of a run-length model (SIMPLE_MODEL(258,_encodeSymbol) after _init(.., 4)): four live entries, held by every
// lane alike
__device__ __forceinline__ void are_run_symbol(u32x4 &e, u32 part, AreCoder &rc, u32 lane)
{
    const u32 c0 = e.x & 0xffffu, c1 = c0 + (e.y & 0xffffu), c2 = c1 + (e.z & 0xffffu), c3 = c2 + (e.w & 0xffffu);
    const u32 j = (e.x >> 16) == part ? 0u : (e.y >> 16) == part ? 1u : (e.z >> 16) == part ? 2u : 3u;
    const u32 ent = ar_get(e, j);
    rc.encode(j == 0 ? 0u : j == 1 ? c0 : j == 2 ? c1 : c2, ent & 0xffffu, c3, lane);
    u32 cur = ent + AR_STEP;
    ar_set(e, j, cur, true);
    if (c3 + AR_STEP > AR_MAX_FREQ) {
        e.x = ar_half(e.x); e.y = ar_half(e.y); e.z = ar_half(e.z); e.w = ar_half(e.w);
        cur = ar_half(cur);
    }
    if (j) {
        const u32 prev = ar_get(e, j - 1);
        if ((cur & 0xffffu) > (prev & 0xffffu)) { ar_set(e, j, prev, true); ar_set(e, j - 1, cur, true); }
    }
}

// HOME: R4X16_ARITH_ENC_O0 / _O1_LDS / _O1_GLOBAL.  One wave per item, the items of other homes passed over; the global
// home's waves stride over the items, each with the row slot of its workgroup.
template <int HOME>
__global__ __launch_bounds__(64) void k_are_encode(const u8 *in, AreWs w, int nitems)
{
    __shared__ __attribute__((aligned(16))) u32 lds[(HOME == R4X16_ARITH_ENC_O1_LDS ? AR_LDS_BUDGET : AR_RUN_BYTES) / 4];
    const u32 lane = threadIdx.x;
    u32x4 *runs = (u32x4 *)lds;
    for (int it = (int)blockIdx.x; it < nitems; it += (int)gridDim.x) {
        AreItem *item = w.items + it;
        if (item->state != ARE_CODE || item->home != HOME) continue;
        const bool rle = item->rle != 0;
        const u32 n = item->n;
        const u32 m = item->m ? item->m : 256u;
        const u32 stride = ar_row_stride(m);
        const ArHome h = ar_home(HOME == R4X16_ARITH_ENC_O1_LDS, lds, w.rows, m, stride);
        if (rle) ar_runs_init(lds, lane);
        u32x4 e = {0, 0, 0, 0};
        u32 tot = m;
        if (HOME == R4X16_ARITH_ENC_O0) e = ar_fresh(4u * lane, m);
        else {
            for (u32 k = lane; k < m * stride; k += WAVE) { const u32 s = k % stride; h.rows[k] = s < m ? 1u | (s << 16) : 0u; }
            for (u32 k = lane; k < m; k += WAVE) h.tots[k] = m;
        }
        wsync();
        ArWindow src(item->src_stage ? w.stage + item->src : in + item->src, n);
        AreCoder rc((u32 *)(w.stage + item->out), m & 0xffu);
        u32 last = 0, i = 0;
        const bool mine = 4u * lane < stride;
        // the early end: the body only grows, and the reference stores the bytes once it is no smaller than they are (:850)
        bool stored = rc.sure() >= n;
        while (!stored && i < n) {
            bool dirty;
            const u32 c = src.byte(i++, lane);
            if (HOME == R4X16_ARITH_ENC_O0) are_symbol(e, tot, c, rc, lane, &dirty);
            else {
                u32x4 *row = (u32x4 *)(h.rows + last * stride);
                e = mine ? row[lane] : u32x4{0, 0, 0, 0};
                tot = h.tots[last];
                are_symbol(e, tot, c, rc, lane, &dirty);
                if (dirty && mine) row[lane] = e;
                if (lane == 0) h.tots[last] = tot;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next step's row may be this one
            }
            last = c;
            stored = rc.sure() >= n;
            if (rle && !stored) {
                u32 run = 0, rctx = last;
                while (i < n && src.byte(i, lane) == last) { run++; i++; }
                do {                                                               // arith_dynamic.c:432-443, :548-559
                    const u32 part = run < 4u ? run : 3u;
                    u32x4 re = runs[rctx];
                    are_run_symbol(re, part, rc, lane);
                    if (lane == 0) runs[rctx] = re;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    run -= part;
                    rctx = rctx == last ? 256u : rctx + (rctx < AR_NRUN - 1u);
                    if (part == 3u && run == 0) {                                  // the closing zero
                        re = runs[rctx];
                        are_run_symbol(re, 0u, rc, lane);
                        if (lane == 0) runs[rctx] = re;
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    }
                    stored = rc.sure() >= n;
                } while (run && !stored);
            }
        }
        if (!stored) { rc.finish(lane); stored = rc.out.n >= n; }
        if (lane == 0) {
            item->body = rc.out.n;
            if (stored) item->state = ARE_STORED;
            if (stored && w.route) atomicAdd(&w.route[R4X16_ARITH_ENC_STORED], 1u);
        }
        wsync();                                                                   // the next item's models overwrite these
    }
}

// ---- back -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 are_len(const AreItem &it) { return 1u + it.nmeta + (it.state == ARE_STORED ? it.n : it.body); }

// One stream at dst: the flag byte with the bits of :851-852, what the front put behind it, the body or the bytes themselves
__device__ __forceinline__ void are_put(u8 *dst, const AreItem &it, const u8 *in, const u8 *stage, u32 t)
{
    const bool cat = it.state == ARE_STORED;
    if (t == 0) dst[0] = cat ? (u8)((it.flags & ~7u) | AR_X_CAT) : it.flags;
    if (t < it.nmeta) dst[1 + t] = it.meta[t];
    const u8 *src = cat ? (it.src_stage ? stage + it.src : in + it.src) : stage + it.out;
    group_copy<256>(dst + 1 + it.nmeta, src, cat ? it.n : it.body, t);
}

__global__ __launch_bounds__(256) void k_are_back(BatchArgs a, AreWs w, int base)
{
    __shared__ u32 win[255], at[256];
    const int b = (int)blockIdx.x, g = base + b;
    const u32 t = threadIdx.x;
    const AreBlk bk = w.blk[b];
    if (bk.status != AR_OK) {
        if (t == 0) { a.status[g] = bk.status; a.out_size[g] = 0; }
        return;
    }
    const AreItem *items = w.items + (size_t)b * w.per;
    u8 *dst = a.out + a.out_off[g];
    const u32 cap = a.out_cap[g];                                    // (at least are_cap, the front's test: every result fits; tested all the same)
    if (!bk.nplanes) {
        const AreItem &it = items[0];
        const bool fits = are_len(it) <= cap;
        if (fits) are_put(dst, it, a.in, w.stage, t);
        if (t == 0) { a.status[g] = fits ? AR_OK : AR_E_CAPACITY; a.out_size[g] = fits ? are_len(it) : 0u; }
        return;
    }
    const u32 N = bk.nplanes;
    if (t < N) {                                                     // the smallest candidate, the first of them in table order
        u32 best = 0xffffffffu, bc = 0;
        for (u32 c = 0; c < ARE_CANDS; c++) {
            const AreItem &it = items[t * ARE_CANDS + c];
            if (it.state == ARE_NONE) continue;
            const u32 len = are_len(it);
            if (len < best) { best = len; bc = c; }
        }
        win[t] = bc; at[t] = best;
    }
    __syncthreads();
    if (t == 0) {                                                    // :672-677, :752: flags, size, N, the planes' lengths
        u64 all = 2u + are_var_len(bk.size);
        for (u32 j = 0; j < N; j++) all += (u64)are_var_len(at[j]) + at[j];
        const bool fits = all <= cap;
        if (fits) {
            u32 p = 0;
            dst[p++] = (u8)bk.flags;
            p += are_var_put(dst + p, bk.size);
            dst[p++] = (u8)N;
            for (u32 j = 0; j < N; j++) p += are_var_put(dst + p, at[j]);
            for (u32 j = 0; j < N; j++) { const u32 len = at[j]; at[j] = p; p += len; }
        }
        at[255] = fits;
        a.status[g] = fits ? AR_OK : AR_E_CAPACITY; a.out_size[g] = fits ? (u32)all : 0u;
    }
    __syncthreads();
    if (!at[255]) return;
    for (u32 j = 0; j < N; j++) are_put(dst + at[j], items[j * ARE_CANDS + win[j]], a.in, w.stage, t);
}

// ---- the device call ----------------------------------------------------------------------------------------------
static size_t are_layout(u8 *base, size_t nb, size_t per, u64 stage_bytes, AreWs *w)
{
    Carver cv(base);
    w->cursor = cv.take<u64>(1);
    w->items = cv.take<AreItem>(nb * per);
    w->blk = cv.take<AreBlk>(nb);
    w->route = cv.take<u32>(R4X16_ARITH_ENC_KINDS);
    w->stage = cv.take<u8>(stage_bytes);
    w->stage_bytes = stage_bytes;
    w->rows = cv.take<u8>((size_t)std::min<size_t>(nb * per, AR_GLOBAL_SLOTS) * AR_GLOBAL_ROW_BYTES);
    w->per = (u32)per;
    return cv.total();
}

// the stage arena of nb blocks of a call that holds `total` bytes in blocks of at most max_in
static u64 are_stage_bytes(size_t nb, size_t per, u32 planes, u64 total, u32 max_in)
{
    const u64 tot = std::min<u64>(total, (u64)nb * max_in);
    return tot * (planes ? 5u : 2u) + 64ull * nb * per + 64ull * nb;
}

extern "C" unsigned int rans4x16_hip_arith_compress_bound(unsigned int size, int order)
{
    // arith_dynamic.c:80-86, its expression in its order of evaluation (the sum is a double, converted at the end)
    return (unsigned int)((order == 0
        ? 1.05 * size + 257 * 3 + 4
        : 1.05 * size + 257 * 257 * 3 + 4 + 257 * 3 + 4) +
        ((order & AR_X_PACK) ? 1 : 0) +
        ((order & AR_X_RLE) ? 1 + 257 * 3 + 4 : 0) + 5);
}

extern "C" unsigned int rans4x16_hip_arith_compress_cap(unsigned int size, int order) { return are_cap(size, order); }

extern "C" int rans4x16_hip_arith_compress_dev(rans4x16_hip_ctx *c, int n,
                                               const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                               unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                               uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                               uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    BatchArgs a;
    const int go = r4x16_dev_call_args(c, "arith_compress_dev: bad arguments", true, &a, n, d_in, d_in_off, d_in_size, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, order, d_order);
    if (go <= 0) return go;
    hipStream_t s = (hipStream_t)stream;
    // the planes a stripe block may have: the one order's own, or what rans4x16_hip_set_dev_stripe_encode reserved
    u32 planes = 0;
    if (d_order) planes = (u32)c->dev_stripe_enc;
    else if (are_order_check(21u, order, &planes) != AR_OK) planes = 0;
    const size_t per = planes ? (size_t)planes * ARE_CANDS : 1;
    // the stage arena: a plain block's packed form and its body; a stripe block's planes, their packed forms and a body
    // a candidate (are_plane_need: 4.5 bytes a byte at most, and the roundings of every item)
    const u64 total = total_in_size ? total_in_size : (u64)n * max_in_size;
    AreWs w;
    auto layout = [&](u8 *at, size_t nb) { return are_layout(at, nb, per, are_stage_bytes(nb, per, planes, total, max_in_size), &w); };
    auto bytes_for = [&](size_t nb) { return layout(nullptr, nb); };
    const size_t chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX / per, r4x16_room(c, A_BIT(A_AR)), bytes_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        layout(c->at(A_AR), (size_t)nb);
        w.planes = planes;
        const int nitems = nb * (int)per;
        u32 *const d_route = w.route;
        HIPCHK(c, hipMemsetAsync(w.cursor, 0, sizeof(u64), s));
        if (r4x16_route_begin(c, &w.route, R4X16_ARITH_ENC_KINDS, s) != 0) return -1;
        hipLaunchKernelGGL(k_are_front, dim3((nb + 3) / 4), dim3(256), 0, s, a, w, (int)base, nb, max_in_size);
        hipLaunchKernelGGL(k_are_encode<R4X16_ARITH_ENC_O0>, dim3(nitems), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_are_encode<R4X16_ARITH_ENC_O1_LDS>, dim3(nitems), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_are_encode<R4X16_ARITH_ENC_O1_GLOBAL>, dim3(std::min(nitems, AR_GLOBAL_SLOTS)), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_are_back, dim3(nb), dim3(256), 0, s, a, w, (int)base);
        return r4x16_route_end(c, R4X16_ROUTE_ARITH_ENC, d_route, R4X16_ARITH_ENC_KINDS, s);
    });
}

// ---- best of k, results back to back --------------------------------------------------------------------------------
// Candidate j of block lb of a chunk is item lb * k + j of one rans4x16_hip_arith_compress_dev call with per-item orders.
// Its slot holds rans4x16_hip_arith_compress_cap of its size and method, rounded up to 16; the slots lie back to back
// (k_pk_scan over their sizes), so a chunk's arena is k times its input plus a constant an item.  A candidate that is
// not tried - a stripe method on a size that is no multiple of 4 (tokenise_name3.c:1270), a block above max_in_size, a
// slot beyond the arena (a batch that holds more than it announced) - has capacity 0: the front refuses it before it
// makes an item, so it is neither coded nor counted.
// (AbMethods, AbWs, AbPlan: r4x16_best_any.h - the call that picks across codecs runs this unit's candidates too)

static size_t ab_carve(AbWs *w, u8 *base, size_t nb, size_t k, u64 slot_bytes)
{
    const size_t items = nb * k;
    Carver cv(base);
    w->in_off = cv.take<u64>(items); w->slot_off = cv.take<u64>(items + 1);
    w->in_size = cv.take<u32>(items); w->need = cv.take<u32>(items); w->cap = cv.take<u32>(items); w->out_size = cv.take<u32>(items);
    w->status = cv.take<i32>(items); w->order = cv.take<i32>(items); w->win = cv.take<u32>(nb);
    w->slots = cv.take<u8>((size_t)slot_bytes + 256);
    w->slot_bytes = slot_bytes;
    return cv.total();
}

__device__ __forceinline__ bool ab_skipped(u32 size, int method) { return (method & AR_X_STRIPE) && (size & 3u); }

__global__ __launch_bounds__(256) void k_ab_expand(const u64 *in_off, const u32 *in_size, AbWs w, AbMethods pm, int base, u32 items, u32 max_in)
{
    const u32 q = blockIdx.x * 256u + threadIdx.x;
    if (q >= items) return;
    const int g = base + (int)(q / (u32)pm.k), m = pm.m[q % (u32)pm.k];
    const u32 sz = in_size[g];
    w.in_off[q] = in_off[g];
    w.in_size[q] = sz;
    w.order[q] = m;
    w.need[q] = (sz > max_in || ab_skipped(sz, m)) ? 0u : ar_r16(are_cap(sz, m));
}

__global__ __launch_bounds__(256) void k_ab_admit(AbWs w, u32 items)
{
    const u32 q = blockIdx.x * 256u + threadIdx.x;
    if (q >= items) return;
    w.cap[q] = w.slot_off[q + 1] <= w.slot_bytes ? w.need[q] : 0u;
}

// the smallest result, the first of them in list order; the status of a block without one is that of the first candidate
// that was tried, UNSUPPORTED if none was.  A tried candidate that failed although its size and its order word are
// acceptable found no room - no slot, or no stage bytes: the batch holds more than it announced - and fails the block as a
// whole (UNSUPPORTED): the smallest of the rest would not be the smallest of the list.
__global__ __launch_bounds__(256) void k_ab_pick(const u32 *in_size, AbWs w, AbMethods pm, u32 *out_size, i32 *status, i32 *chosen, int base, int nb,
                                                 u32 max_in)
{
    const int lb = (int)(blockIdx.x * 256u + threadIdx.x);
    if (lb >= nb) return;
    const int g = base + lb;
    const u32 sz = in_size[g];
    int win = -1, first = -1;
    u32 best = 0;
    bool no_room = false;
    for (int j = 0; j < pm.k; j++) {
        if (ab_skipped(sz, pm.m[j])) continue;
        const size_t q = (size_t)lb * pm.k + j;
        if (first < 0) first = j;
        u32 N;
        if (w.status[q] != AR_OK && sz <= max_in && are_order_check(sz, pm.m[j], &N) == AR_OK) no_room = true;
        if (w.status[q] == AR_OK && (win < 0 || w.out_size[q] < best)) { best = w.out_size[q]; win = j; }
    }
    i32 st = AR_OK;
    if (no_room) { win = -1; st = AR_E_UNSUPPORTED; }
    else if (win < 0) st = first >= 0 ? w.status[(size_t)lb * pm.k + first] : AR_E_UNSUPPORTED;
    w.win[lb] = win >= 0 ? (u32)win : 0u;
    status[lb] = st;                                                                  // (the chunk's arrays: the callers pass them from `base` on)
    out_size[lb] = win >= 0 ? best : 0u;
    if (chosen) chosen[lb] = win >= 0 ? pm.m[win] : -1;
}

__global__ __launch_bounds__(256) void k_ab_gather(PackedOut pk, AbWs w, int k, u32 *out_size, i32 *status, int base)
{
    const u32 tid = threadIdx.x;
    const int lb = (int)blockIdx.x, i = base + lb;
    const u32 sz = out_size[i];
    if (sz == 0) return;
    if (pk.off[i + 1] > pk.capacity) {
        if (tid == 0) { status[i] = AR_E_CAPACITY; out_size[i] = 0; }
        return;
    }
    group_copy<256>(pk.out + pk.off[i], w.slots + w.slot_off[(size_t)lb * k + w.win[lb]], sz, tid);
}

// What the call plans before it enqueues (AbPlan): the methods, the planes a stripe candidate may have, the items an inner
// item reserves, the batch's bytes and the blocks per chunk - this call's candidate slots (the packed arena) and the inner
// call's arena for k items a block fit the room together, so that the inner call takes the chunk in one pass.
static u64 ab_slot_bytes(const AbPlan &p, size_t nb, u32 max_in)
{
    return (u64)p.pm.k * (std::min<u64>(p.total, (u64)nb * max_in) + (u64)nb * (64u + 28u * p.planes));
}
static u64 ab_inner_total(const AbPlan &p, size_t nb, u32 max_in) { return (u64)p.pm.k * std::min<u64>(p.total, (u64)nb * max_in); }

int r4x16_ab_methods(rans4x16_hip_ctx *c, const char *who, int k, const int *methods, AbPlan *p)
{
    p->pm = AbMethods{};
    p->pm.k = k;
    p->planes = 0;
    for (int j = 0; j < k; j++) {
        u32 N = 0;
        if ((methods[j] & AR_X_STRIPE) && are_order_check(21u, methods[j], &N) != AR_OK) { c->err = std::string(who) + ": more than 255 stripes"; return -1; }
        p->planes = std::max(p->planes, N);
        p->pm.m[j] = methods[j];
    }
    return 0;
}

void r4x16_ab_sizes(int n, uint32_t max_in_size, uint64_t total_in_size, AbPlan *p)
{
    p->per = p->planes ? (size_t)p->planes * ARE_CANDS : 1;
    p->total = total_in_size ? total_in_size : (u64)n * max_in_size;
    p->chunk = 0;
}

size_t r4x16_ab_carve(AbWs *w, u8 *base, const AbPlan &p, size_t nb, u32 max_in_size)
{
    return ab_carve(w, base, nb, (size_t)p.pm.k, ab_slot_bytes(p, nb, max_in_size));
}

size_t r4x16_ab_inner_bytes(const AbPlan &p, size_t nb, u32 max_in_size)
{
    AreWs iw;
    const size_t items = nb * (size_t)p.pm.k;
    return are_layout(nullptr, items, p.per, are_stage_bytes(items, p.per, p.planes, ab_inner_total(p, nb, max_in_size), max_in_size), &iw);
}

// the rest, on the context's device
static void ab_fit(rans4x16_hip_ctx *c, int n, uint32_t max_in_size, uint64_t total_in_size, AbPlan *p)
{
    r4x16_ab_sizes(n, max_in_size, total_in_size, p);
    if (n == 0) return;
    AbWs w;
    auto bytes = [&](size_t nb) { return r4x16_ab_carve(&w, nullptr, *p, nb, max_in_size) + r4x16_ab_inner_bytes(*p, nb, max_in_size); };
    p->chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX / (p->per * p->pm.k), r4x16_room(c, A_BIT(A_PS) | A_BIT(A_AR)), bytes);
}

int r4x16_ab_candidates(rans4x16_hip_ctx *c, const AbPlan &p, const AbWs &w, size_t arena, size_t base, int nb, const u8 *d_in,
                        const u64 *d_in_off, const u32 *d_in_size, u32 *out_size, i32 *status, i32 *chosen, u32 max_in_size, hipStream_t s)
{
    const u32 items = (u32)nb * (u32)p.pm.k;
    const dim3 per_item((items + 255) / 256);
    hipLaunchKernelGGL(k_ab_expand, per_item, dim3(256), 0, s, d_in_off, d_in_size, w, p.pm, (int)base, items, max_in_size);
    r4x16_launch_packed_scan(w.need, w.slot_off, 0, (int)items, s);
    hipLaunchKernelGGL(k_ab_admit, per_item, dim3(256), 0, s, w, items);
    {
        // the inner call: what is left of the ceiling beside the caller's slots, and the planes the methods ask for
        Keep<size_t> ceiling(c->max_ws, c->max_ws > arena + ((size_t)1 << 20) ? c->max_ws - arena : (size_t)1 << 20);
        Keep<int> stripe(c->dev_stripe_enc, (int)p.planes);
        if (rans4x16_hip_arith_compress_dev(c, (int)items, d_in, w.in_off, w.in_size, w.slots, w.slot_off, w.cap, w.out_size, w.status, 0,
                                            w.order, max_in_size, ab_inner_total(p, (size_t)nb, max_in_size), s) != 0)
            return -1;
    }
    hipLaunchKernelGGL(k_ab_pick, dim3((u32)(nb + 255) / 256), dim3(256), 0, s, d_in_size, w, p.pm, out_size, status, chosen, (int)base, nb, max_in_size);
    return 0;
}

extern "C" int rans4x16_hip_arith_best_chunk_blocks(rans4x16_hip_ctx *c, int n, int k, const int *methods, uint32_t max_in_size,
                                                    uint64_t total_in_size)
{
    if (!c) return -1;
    if (n < 0 || k < 1 || k > AB_MAX_K || !methods) { c->err = "arith_best_chunk_blocks: bad arguments"; return -1; }
    AbPlan p;
    if (r4x16_ab_methods(c, "arith_compress_best_packed_dev", k, methods, &p) != 0) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    ab_fit(c, n, max_in_size, total_in_size, &p);
    return (int)p.chunk;
}

extern "C" int rans4x16_hip_arith_compress_best_packed_dev(rans4x16_hip_ctx *c, int n,
                                                           const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                           unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                           uint32_t *d_out_size, int32_t *d_status,
                                                           int k, const int *methods, int32_t *d_chosen,
                                                           uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    AbPlan p;
    BatchArgs a;                                   // (filled, not read: the items of the inner call are this call's own)
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "arith_compress_best_packed_dev: bad arguments", k >= 1 && k <= AB_MAX_K && methods, &a, &pk, n,
                                          d_in, d_in_off, d_in_size, d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s,
                                          [&] { return r4x16_ab_methods(c, "arith_compress_best_packed_dev", k, methods, &p); });
    if (go <= 0) return go;
    ab_fit(c, n, max_in_size, total_in_size, &p);
    AbWs w;
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_PS, r4x16_ab_carve(&w, nullptr, p, nb, max_in_size), false); };
    return r4x16_chunk_walk(c, n, p.chunk, s, grab, [&](size_t base, int nb) {
        const size_t arena = r4x16_ab_carve(&w, c->at(A_PS), p, (size_t)nb, max_in_size);
        if (r4x16_ab_candidates(c, p, w, arena, base, nb, d_in, d_in_off, d_in_size, d_out_size + base, d_status + base,
                                d_chosen ? d_chosen + base : nullptr, max_in_size, s) != 0)
            return -1;
        r4x16_launch_packed_scan(d_out_size, d_out_off, (int)base, nb, s);
        hipLaunchKernelGGL(k_ab_gather, dim3((u32)nb), dim3(256), 0, s, pk, w, k, d_out_size, d_status, (int)base);
        return 0;
    });
}

// ---- host buffers -------------------------------------------------------------------------------------------------
// One round trip (r4x16_host_trip) around the device call with per-block orders.  Stripe encoding is switched on for the
// call (rans4x16_hip_set_dev_stripe_encode with the most planes of the batch) and the caller's setting put back.
extern "C" int rans4x16_hip_arith_compress_batch(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *const *in, const unsigned int *in_size,
                                                 unsigned char *const *out, unsigned int *out_size, const int *order, int *status)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !out || !out_size || !order || !status))) { c->err = "arith_compress_batch: bad arguments"; return -1; }
    if (n == 0) return 0;
    // what the order word and the capacity refuse is refused here, before anything is uploaded; a refused block takes no
    // slot (its capacity 0 refuses it on the device as well)
    std::vector<u32> isz(n, 0), cap(n, 0);
    std::vector<i32> ord(n, 0);
    std::vector<u8> take(n, 0);
    u32 max_in = 0, planes = 0;
    for (int i = 0; i < n; i++) {
        u32 N = 0;
        status[i] = (in[i] || !in_size[i]) && out[i] ? are_order_check(in_size[i], order[i], &N) : R4X16_E_UNSUPPORTED;
        if (status[i] == AR_OK && out_size[i] < are_cap(in_size[i], order[i])) status[i] = AR_E_CAPACITY;
        if (status[i] != AR_OK) { out_size[i] = 0; continue; }
        take[i] = 1;
        isz[i] = in_size[i]; cap[i] = are_cap(in_size[i], order[i]); ord[i] = order[i];
        max_in = std::max(max_in, isz[i]); planes = std::max(planes, N);
    }
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), ord.data(), nullptr, 0, 0, nullptr};
    return r4x16_host_trip(c, n, trip, [&](const StageLayout &L, size_t in_total, size_t, hipStream_t s) {
        Keep<int> stripe(c->dev_stripe_enc, (int)planes);
        return rans4x16_hip_arith_compress_dev(c, n, L.in, L.in_off, L.in_size, L.out, L.out_off, L.cap, L.osz, L.status, 0, L.order, max_in,
                                               in_total, s);
    });
}

// ---- the reference's calls (arith_dynamic.h), on the calling thread's context -------------------------------------
extern "C" unsigned char *rans4x16_hip_arith_compress_to(unsigned char *in, unsigned int in_size,
                                                        unsigned char *out, unsigned int *out_size, int order)
{
    if (!out_size || (!in && in_size)) return nullptr;
    u32 N;
    if (are_order_check(in_size, order, &N) != AR_OK) return nullptr;            // before any device is asked for
    if (out && *out_size < are_cap(in_size, order)) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    unsigned int cap = out ? *out_size : rans4x16_hip_arith_compress_bound(in_size, order);
    unsigned char *buf = out ? out : (unsigned char *)malloc(cap);
    if (!buf) return nullptr;
    unsigned char none = 0;
    const unsigned char *ins[1] = {in ? in : &none};
    unsigned char *outs[1] = {buf};
    unsigned int osz[1] = {cap};
    int st[1] = {0};
    const int rc = rans4x16_hip_arith_compress_batch(c, 1, ins, &in_size, outs, osz, &order, st);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || st[0] != 0) { if (!out) free(buf); return nullptr; }
    *out_size = osz[0];
    return buf;
}

extern "C" unsigned char *rans4x16_hip_arith_compress(unsigned char *in, unsigned int in_size, unsigned int *out_size, int order)
{
    return rans4x16_hip_arith_compress_to(in, in_size, nullptr, out_size, order);
}
