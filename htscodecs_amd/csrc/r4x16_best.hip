// r4x16_best.hip - "try k methods, keep the smallest" for device-resident batches (tokenise_name3.c:1246-1300), and
// X_STRIPE under per-block orders (rans4x16_hip_set_dev_stripe_encode).
//
// Both are the same three steps on the caller's stream, without a read-back:
//   prepare : every block gets P internal items, laid out from host knowledge - a plain method is one item that reads
//             the caller's input in place, a stripe method is N x K items (plane, sub-method of {1, 64, 128, 0}) that
//             read the block's byte planes, transposed once per distinct N and shared by the stripe methods of that N.
//             Items that do not apply (X_STRIPE on a size that is no multiple of four, a candidate whose bound exceeds
//             the caller's capacity, unused planes) are idle: in_size 0, X_CAT | X_NOSZ.
//   encode  : the ordinary pipeline over the internal items with a per-item order (a recursive *_dev call).
//   pick    : per block, the arg-min over the sub-methods of every plane (first on ties, rANS_static4x16pr.c:1199), then
//             the arg-min over the methods (first on ties, tokenise_name3.c:1281); only the winner is moved into the
//             caller's slot - a stripe winner as header (:1185-1187, :1210) and the N chosen payloads behind it.
// Under per-block orders (k = 1) the one method of a block is d_order[b]: the kernels derive N and the sub-methods from
// it, every block reserves max_planes x 4 items, and a block that is no stripe is encoded straight into the caller's slot.
//
// Candidate slots are bound-sized, so a batch is walked in chunks of blocks: the candidate arena of a chunk and the
// workspace of its inner call together stay under the context's ceiling (option max_workspace_mb) and under three
// quarters of the free device memory.
//
// Loops: every trip count is a launch argument (k <= 32, N <= 255, K <= 4, P) or a block size that was checked against
// the host's max_in_size first.
#include "r4x16_host.h"
#include "r4x16_best_any.h"

#define BEST_MAX_K 32
#define BEST_IDLE (X_CAT | X_NOSZ)
enum { BK_PLAIN = 0, BK_STRIPE = 1, BK_SKIP = 2 };

struct BestMethod {
    i32 method;                    // as the caller gave it
    u32 N;                         // planes (stripe)
    u32 item0, items;              // the method's internal items within a block
    u32 slot, slot0, n0;           // bytes of one candidate output slot: slot0 for the first n0 items, slot for the rest
    u64 off;                       // first slot, from the start of the block's candidate region
    u8 stripe, K, set, pad;        // K sub-methods; set: which plane buffer of the block
    u8 sub[4];
};
struct BestArgs {
    int k, nsets, by_order;
    u32 P, max_in, max_planes;
    u64 blk_bytes, pl_stride;      // candidate region / one plane buffer, per block
    u8 setN[BEST_MAX_K];
    BestMethod m[BEST_MAX_K];
};
struct BestWs {                    // M = nb * P internal items; every pointer into the context's stripe arena
    u8 *planes;
    u64 *in_off, *out_off;
    u32 *in_size, *out_cap, *out_size;
    i32 *status, *order;
    u8 *out;
};

// N and the sub-methods that `method` allows (:1192-1195).  Sub-method 0 is always among them, and a plane coded with
// 0 | X_NOSZ never takes more than its own length + 1 (stored as X_CAT when rANS does not shrink it, :1332-1337): the
// reference's starting value best_sz = in_size + 10 (:1192) is always replaced, so the arg-min over the K candidates is
// the whole of its search.
static __host__ __device__ inline void bm_fill(BestMethod *M, int method)
{
    const int cand[4] = {1, 64, 128, 0};
    M->method = method;
    M->stripe = (method & X_STRIPE) ? 1 : 0;
    const u32 N = (u32)method >> 8;
    M->N = N ? N : 4;
    u32 K = 0;
    for (int q = 0; q < 4; q++) if ((method & cand[q]) == cand[q]) M->sub[K++] = (u8)cand[q];
    M->K = (u8)K;
}

static __device__ __forceinline__ BestMethod bm_of(const BestArgs &e, u32 j, const BatchArgs &a, int b)
{
    BestMethod M = e.m[e.by_order ? 0 : j];
    if (e.by_order) bm_fill(&M, a.d_order[b]);
    return M;
}

// what becomes of method M on a block of n bytes with `cap` bytes of room (*st != ST_OK: the candidate fails)
static __device__ __forceinline__ u32 bm_decide(const BestArgs &e, const BestMethod &M, u32 n, u32 cap, i32 *st)
{
    *st = ST_OK;
    if (M.stripe && !e.by_order && (n & 3u)) return BK_SKIP;                          // tokenise_name3.c:1270
    if (n > e.max_in) { *st = ST_UNSUPPORTED; return BK_PLAIN; }                      // larger than the call was sized for
    if (cap < r4x16_bound_hd(n, M.method)) { *st = ST_CAPACITY; return BK_PLAIN; }
    if (M.stripe && n > 20) {                                                         // :1151
        if (M.N > e.max_planes) *st = ST_UNSUPPORTED;
        return BK_STRIPE;
    }
    return BK_PLAIN;
}

__global__ __launch_bounds__(256) void k_best_prepare(BatchArgs a, BestWs w, BestArgs e, int base)
{
    __shared__ u32 s_kind[BEST_MAX_K], s_need[BEST_MAX_K];
    __shared__ i32 s_st[BEST_MAX_K];
    const u32 lb = blockIdx.x, tid = threadIdx.x;
    const int b = base + (int)lb;
    const u8 *src = a.in + a.in_off[b];
    const u32 n = a.in_size[b], cap = a.out_cap[b];
    u8 *pl = w.planes + (u64)lb * (u64)e.nsets * e.pl_stride;
    const u64 item0 = (u64)lb * e.P, cand0 = (u64)lb * e.blk_bytes;
    if (tid < BEST_MAX_K) s_need[tid] = 0;
    __syncthreads();
    if (tid < (u32)e.k) {
        const BestMethod M = bm_of(e, tid, a, b);
        i32 st;
        const u32 kind = bm_decide(e, M, n, cap, &st);
        s_kind[tid] = kind; s_st[tid] = st;
        if (kind == BK_STRIPE && st == ST_OK) s_need[M.set] = 1;
    }
    __syncthreads();
    for (u32 j = 0; j < (u32)e.k; j++) {
        const BestMethod M = bm_of(e, j, a, b);
        const bool live = s_st[j] == ST_OK && s_kind[j] != BK_SKIP;
        const bool stripe = live && s_kind[j] == BK_STRIPE;
        const u32 K = M.K, N = stripe ? M.N : 1u, part = n / N, extra = n % N;
        const u8 *pbase = pl + (u64)M.set * e.pl_stride;
        for (u32 t = tid; t < M.items; t += 256) {
            const u64 it = item0 + M.item0 + t;
            u64 ioff = 0, ooff = cand0 + M.off + (t < M.n0 ? (u64)t * M.slot0 : (u64)M.n0 * M.slot0 + (u64)(t - M.n0) * M.slot);
            u32 isz = 0, ocap = t < M.n0 ? M.slot0 : M.slot;
            i32 ord = BEST_IDLE;
            if (stripe) {
                const u32 p = t / K, q = t % K;
                if (p < N) {
                    ioff = (u64)(pbase - w.planes) + (u64)p * part + (p < extra ? p : extra);
                    isz = part + (extra > p ? 1u : 0u);
                    ord = (i32)M.sub[q] | X_NOSZ;                                     // :1197
                }
            } else if (live && t == 0) {
                ioff = (u64)(src - w.planes);
                isz = n;
                ord = M.stripe ? (M.method & 0xff & ~X_STRIPE) : M.method;            // :1151
                if (e.by_order) { ooff = (u64)((a.out + a.out_off[b]) - w.out); ocap = cap; }   // no second candidate: in place
            }
            w.in_off[it] = ioff; w.in_size[it] = isz; w.order[it] = ord;
            w.out_off[it] = ooff; w.out_cap[it] = ocap;
        }
    }
    for (u32 s = 0; s < (u32)e.nsets; s++) {                                          // :1168-1180, once per distinct N
        if (!s_need[s]) continue;
        const u32 N = e.by_order ? bm_of(e, 0, a, b).N : (u32)e.setN[s];
        const u32 part = n / N, extra = n % N;
        u8 *dst = pl + (u64)s * e.pl_stride;
        for (u32 i = tid; i < n; i += 256) {                                          // n <= max_in (bm_decide)
            const u32 p = i % N, x = i / N;
            dst[p * part + (p < extra ? p : extra) + x] = src[i];
        }
    }
}

// plane p of stripe method M: the smallest of its candidates, the first on ties (:1192-1208)
static __device__ __forceinline__ i32 plane_pick(const BestWs &w, const BestMethod &M, u64 mitem0, u32 p, u32 n, u32 *sz, u32 *item)
{
    const u32 K = M.K;
    u32 best_sz = n + 10u, best = K;
    for (u32 q = 0; q < K; q++) {
        const u64 it = mitem0 + (u64)p * K + q;
        if (w.status[it] != ST_OK) return w.status[it];
        if (best_sz > w.out_size[it]) { best_sz = w.out_size[it]; best = q; }
    }
    if (best == K) return ST_UNSUPPORTED;                                             // (never: see bm_fill)
    *sz = best_sz; *item = p * K + best;
    return ST_OK;
}

__global__ __launch_bounds__(256) void k_best_pick(BatchArgs a, BestWs w, BestArgs e, i32 *chosen, int base)
{
    __shared__ u32 s_kind[BEST_MAX_K], s_size[BEST_MAX_K];
    __shared__ i32 s_st[BEST_MAX_K];
    __shared__ u32 s_psz[256], s_pit[256], s_poff[256];
    __shared__ int s_win;
    __shared__ u32 s_hl;
    const u32 lb = blockIdx.x, tid = threadIdx.x;
    const int b = base + (int)lb;
    const u32 n = a.in_size[b], cap = a.out_cap[b];
    const u64 item0 = (u64)lb * e.P;
    u8 *out = a.out + a.out_off[b];

    if (tid < (u32)e.k) {                                                             // every method's verdict and size
        const BestMethod M = bm_of(e, tid, a, b);
        i32 st;
        const u32 kind = bm_decide(e, M, n, cap, &st);
        u32 size = 0;
        if (st == ST_OK && kind == BK_PLAIN) {
            st = w.status[item0 + M.item0];
            size = w.out_size[item0 + M.item0];
        } else if (st == ST_OK && kind == BK_STRIPE) {
            u64 total = 2u + var_len(n);                                              // flags, size, N (:1185-1187)
            for (u32 p = 0; p < M.N; p++) {
                u32 sz = 0, item = 0;
                st = plane_pick(w, M, item0 + M.item0, p, n, &sz, &item);
                if (st != ST_OK) break;
                total += (u64)var_len(sz) + sz;
            }
            if (st == ST_OK && total > cap) st = ST_CAPACITY;                         // (the bound rules it out)
            size = (u32)total;
        }
        s_kind[tid] = kind; s_st[tid] = st; s_size[tid] = size;
    }
    __syncthreads();
    if (tid == 0) {                                                                   // smallest wins, the first on ties
        int win = -1, first = -1;
        u32 best = 0;
        for (int j = 0; j < e.k; j++) {
            if (s_kind[j] == BK_SKIP) continue;
            if (first < 0) first = j;
            if (s_st[j] == ST_OK && (win < 0 || best > s_size[j])) { best = s_size[j]; win = j; }
        }
        s_win = win;
        a.status[b] = win >= 0 ? ST_OK : first >= 0 ? s_st[first] : ST_UNSUPPORTED;
        a.out_size[b] = win >= 0 ? best : 0u;
        if (chosen) chosen[b] = win >= 0 ? bm_of(e, (u32)win, a, b).method : -1;
    }
    __syncthreads();
    if (s_win < 0) return;
    const BestMethod M = bm_of(e, (u32)s_win, a, b);
    const u64 mitem0 = item0 + M.item0;
    if (s_kind[s_win] == BK_PLAIN) {
        if (!e.by_order) group_copy<256>(out, w.out + w.out_off[mitem0], s_size[s_win], tid);
        return;
    }
    if (tid < M.N) {
        u32 sz = 0, item = 0;
        (void)plane_pick(w, M, mitem0, tid, n, &sz, &item);
        s_psz[tid] = sz; s_pit[tid] = item;
    }
    __syncthreads();
    if (tid == 0) {
        u32 hl = 1, body = 0;
        out[0] = (u8)(M.method & ~X_NOSZ);                                            // :1185
        hl += var_put(out + hl, n);
        out[hl++] = (u8)M.N;
        for (u32 p = 0; p < M.N; p++) { hl += var_put(out + hl, s_psz[p]); s_poff[p] = body; body += s_psz[p]; }   // :1210
        s_hl = hl;
    }
    __syncthreads();
    for (u32 p = 0; p < M.N; p++)
        group_copy<256>(out + s_hl + s_poff[p], w.out + w.out_off[mitem0 + s_pit[p]], s_psz[p], tid);
}

// ---- host ----------------------------------------------------------------------------------------------------
static size_t best_carve(BestWs *w, u8 *base, size_t nb, const BestArgs &e)
{
    const size_t M = nb * e.P;
    Carver cv(base);
    w->planes = cv.take<u8>(nb * (size_t)e.nsets * e.pl_stride + 256);
    w->in_off = cv.take<u64>(M); w->out_off = cv.take<u64>(M);
    w->in_size = cv.take<u32>(M); w->out_cap = cv.take<u32>(M); w->out_size = cv.take<u32>(M);
    w->status = cv.take<i32>(M); w->order = cv.take<i32>(M);
    w->out = cv.take<u8>(nb * e.blk_bytes + 256);
    return cv.total();
}

// Lays the methods out (items, slots, plane sets) and runs the batch in chunks.  e->k, e->by_order, e->max_planes and
// e->m[j].method are set by the caller; `reserve` is the number of items a by_order block keeps.  `fan` bounds the bytes
// the inner call reads per input byte (every plain method once, every stripe method once per sub-method).
static u32 best_layout(BestArgs *e, u32 reserve, uint32_t max_in_size)
{
    e->max_in = max_in_size;
    e->pl_stride = align_up((size_t)max_in_size + 64, 256);
    e->nsets = 0;
    u32 P = 0, fan = 0;
    u64 off = 0;
    for (int j = 0; j < e->k; j++) {
        BestMethod *M = &e->m[j];
        bm_fill(M, M->method);
        M->item0 = P; M->off = off; M->set = 0;
        u32 item_max = max_in_size;
        M->n0 = 0; M->slot0 = 0;
        if (e->by_order) {
            // N is known to the device only.  Items 0..3 may be planes of N = 1, whole blocks; an item from 4 on belongs
            // to plane t / K >= 1 (K <= 4), so its block has N >= 2 and the plane at most half of it, rounded up.
            M->items = reserve;
            M->n0 = reserve < 4 ? reserve : 4;
            M->slot0 = (u32)align_up((size_t)r4x16_compress_bound(max_in_size, 0xc1) + 64, 256);
            const u32 half = max_in_size / 2 + 1;
            item_max = half > 20 ? half : 20;
            e->nsets = 1; e->setN[0] = 0;
            fan = 4;
        } else if (M->stripe) {
            M->items = M->N * M->K;
            int set = 0;
            while (set < e->nsets && e->setN[set] != M->N) set++;
            if (set == e->nsets) e->setN[e->nsets++] = (u8)M->N;
            M->set = (u8)set;
            const u32 part = (max_in_size + M->N - 1) / M->N;
            item_max = part > 20 ? part : 20;                                         // (a block of up to 20 bytes rides as item 0)
            fan += M->K;
        } else {
            M->items = 1;
            fan += 1;
        }
        const int slot_order = (e->by_order || M->stripe) ? 0xc1 : M->method;
        M->slot = (u32)align_up((size_t)r4x16_compress_bound(item_max, slot_order) + 64, 256);
        P += M->items;
        off += (u64)M->n0 * M->slot0 + (u64)(M->items - M->n0) * M->slot;
    }
    e->P = P;
    e->blk_bytes = off;
    return fan;
}

// what a chunk of nb blocks takes: the candidate arena and the inner call's workspace
static size_t best_chunk_bytes(const BestArgs &e, u32 fan, size_t nb, uint32_t max_in_size, u64 total_in)
{
    BestWs w;
    return best_carve(&w, nullptr, nb, e) + r4x16_enc_ws_bytes(nb * e.P, max_in_size, (u64)fan * std::min<u64>(total_in, (u64)nb * max_in_size));
}

size_t r4x16_best_chunk_bytes(int k, const int *methods, size_t nb, uint32_t max_in_size, uint64_t total_in_size)
{
    BestArgs e = {};
    e.k = k; e.by_order = 0; e.max_planes = 255;
    for (int j = 0; j < k; j++) e.m[j].method = methods[j];
    const u32 fan = best_layout(&e, 0, max_in_size);
    return best_chunk_bytes(e, fan, nb, max_in_size, total_in_size ? total_in_size : (u64)nb * max_in_size);
}

static int best_run(rans4x16_hip_ctx *c, int n, const BatchArgs &a, BestArgs *e, i32 *d_chosen, u32 reserve,
                    uint32_t max_in_size, uint64_t total_in_size, hipStream_t s)
{
    const u32 fan = best_layout(e, reserve, max_in_size);
    const u32 P = e->P;

    // blocks per chunk: candidate arena + the inner call's workspace under the ceiling, in equal chunks
    const u64 total_in = total_in_size ? total_in_size : (u64)n * max_in_size;
    auto inner_total = [&](size_t nb) { return (u64)fan * std::min<u64>(total_in, (u64)nb * max_in_size); };
    BestWs w;
    auto bytes = [&](size_t nb) { return best_chunk_bytes(*e, fan, nb, max_in_size, total_in); };
    // (INT_MAX / P: the inner call counts its items in an int)
    const size_t chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX / P, r4x16_room(c, A_BIT(A_WS) | A_BIT(A_XS)), bytes);
    // (no refusal above half of the free memory here, unlike r4x16_stripe.hip on the same arena: the chunk was planned
    //  under r4x16_room a moment ago, and a chunk that does not fit after all is halved, not refused)
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_XS, best_carve(&w, nullptr, nb, *e), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        if (base == 0) best_carve(&w, c->at(A_XS), (size_t)nb, *e);                   // the layout of the call: nb is the chunk size here
        hipLaunchKernelGGL(k_best_prepare, dim3((u32)nb), dim3(256), 0, s, a, w, *e, (int)base);
        {
            Keep<bool> inner(c->in_stripe, true);
            if (rans4x16_hip_compress_dev_sized(c, nb * (int)P, w.planes, w.in_off, w.in_size, w.out, w.out_off, w.out_cap, w.out_size,
                                                w.status, 0, w.order, max_in_size, inner_total((size_t)nb), s) != 0)
                return -1;
        }
        hipLaunchKernelGGL(k_best_pick, dim3((u32)nb), dim3(256), 0, s, a, w, *e, d_chosen, (int)base);
        return 0;
    });
}

int r4x16_orders_stripe_compress_dev(rans4x16_hip_ctx *c, int n, const BatchArgs &a, uint32_t max_in_size, uint64_t total_in_size,
                                     hipStream_t s)
{
    BestArgs e = {};
    e.k = 1; e.by_order = 1; e.max_planes = (u32)c->dev_stripe_enc;
    e.m[0].method = 0;
    return best_run(c, n, a, &e, nullptr, (u32)c->dev_stripe_enc * 4u, max_in_size, total_in_size, s);
}

extern "C" int rans4x16_hip_compress_best_dev(rans4x16_hip_ctx *c, int n,
                                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                              unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                              uint32_t *d_out_size, int32_t *d_status,
                                              int k, const int *methods, int32_t *d_chosen,
                                              uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    BestArgs e = {};
    e.k = k; e.by_order = 0; e.max_planes = 255;
    auto table = [&] {
        for (int j = 0; j < k; j++) {
            if ((methods[j] & X_STRIPE) && ((unsigned)methods[j] >> 8) > 255) { c->err = "compress_best_dev: more than 255 stripes"; return -1; }   // :1158
            e.m[j].method = methods[j];
        }
        return 0;
    };
    BatchArgs a;
    const int go = r4x16_dev_call_args(c, "compress_best_dev: bad arguments", k >= 1 && k <= BEST_MAX_K && methods, &a, n, d_in, d_in_off,
                                       d_in_size, d_out, d_out_off, d_out_cap, d_out_size, d_status, 0, nullptr, table);
    if (go <= 0) return go;
    if (c->opts.v[OPT_ROUTE_COUNT] && !c->in_packed) c->route[R4X16_ROUTE_RESULT][R4X16_RESULT_IN_SLOT] += n;
    return best_run(c, n, a, &e, d_chosen, 0, max_in_size, total_in_size, (hipStream_t)stream);
}
