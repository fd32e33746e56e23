// r4x16_packed.hip - the packed device-resident calls (include/rans4x16_hip.h: rans4x16_hip_compress_packed_dev,
// rans4x16_hip_compress_best_packed_dev, rans4x16_hip_peek_dev, rans4x16_hip_uncompress_packed_dev): results back to
// back in one dense arena, where they start written by the device, no bound-sized slot per block on the caller's side.
//
// Encode.  The pipeline still needs a bound-sized slot per block (the payload is written backwards from its end), so
// the slots move into an arena of the context (`ps`), a chunk of blocks at a time, and the caller holds dense bytes only:
//   dense    : front, tables and chain into the internal slots, then k_enc_size (the finish's length arithmetic, nothing
//              moved), k_pk_scan (sizes -> offsets, carried on from the previous chunk's last offset) and the dense
//              instantiation of k_enc_finish, which assembles every stream at its final place (r4x16_encode.hip;
//              r4x16_enc_run in r4x16_api.hip).  Every result byte moves once.
//   gathered : where the stripe machinery or best-of-k runs, the existing call encodes a chunk into the internal slots,
//              then k_pk_scan and k_pk_gather (one workgroup per block copies its result to its offset).
// Decode.  k_unpk_claim reads every stream's own size field (k_peek's reader), k_pk_scan lays the outputs out,
// k_unpk_admit withdraws the blocks that may not run (their input length becomes 0 for the inner call), the existing
// decode runs with capacity = claimed size, and k_unpk_verdict restores the withdrawn blocks' statuses.
//
//
// rANS 4x8 (include/rans4x8_hip.h, the five calls at the end of this file) has the same surface on the same kernels.
// Its encoder leaves the payload in workspace scratch and its finish only copies header, table and payload out, so the
// packed encode and best-of-two are all dense and hold no slots at all: a block runs as k <= 2 internal items over the
// same input, k8_enc_size picks the winner and sizes it, k_pk_scan lays the winners out and k8_enc_finish assembles
// each at its place (r4x16_encode.hip; r4x8_enc_run in r4x16_api.hip).  Its decode is the sequence above around
// rans4x8_hip_uncompress_dev, with peek_one8 reading the size field (bytes 5..8).
//
// Loops: every trip count is a launch argument (n, nb, k <= 32) or a block size checked against the host's max_in_size
// first (the size field's varint is read inside the block's in_size <= max_in_size bytes; rANS 4x8's is at a fixed place
// and read only from blocks of 9 bytes or more).
#include "r4x16_host.h"
#include "r4x16_best_any.h"            // peek_one, the reader of the size field, and the slots of a method list

#define PK_MAX_K 32
struct PkMethods { int k; int m[PK_MAX_K]; };      // k == 0: the call's order / d_order

// The internal slot of every block of the call: block i of a chunk of `chunk` blocks owns slot i % chunk.  Its capacity
// is the block's own bound (the largest over the methods of a best-of-k call); 0 marks a block the arena was not sized
// for - larger than max_in_size, or an order whose bound exceeds the slot - which the pipeline then refuses (CAPACITY,
// reported as UNSUPPORTED by k_enc_size / k_pk_gather).
__global__ __launch_bounds__(256) void k_pk_slots(const u32 *in_size, const i32 *d_order, int order, PkMethods pm, int n, u32 chunk,
                                                  u64 stride, u32 max_in, u64 *slot_off, u32 *slot_cap)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const u32 sz = in_size[i];
    u64 cap = 0;
    if (pm.k == 0) cap = r4x16_bound_hd(sz, d_order ? d_order[i] : order);
    else
        for (int j = 0; j < pm.k; j++) { const u32 bj = r4x16_bound_hd(sz, pm.m[j]); if (bj > cap) cap = bj; }
    if (sz > max_in || cap + 64u > stride) cap = 0;
    slot_off[i] = (u64)((u32)i % chunk) * stride;
    slot_cap[i] = (u32)cap;
}

// off[base + b + 1] = off[base] + size[base] + .. + size[base + b] for b < nb; off[0] = 0.  One workgroup: the running
// offset of a call lives in off[] itself, the last entry one chunk wrote is the seed of the next.  A thread sums
// PK_SCAN_PER consecutive sizes, the 1024 sums are scanned in LDS, and the thread writes its offsets from its own start:
// a chunk of 131,072 blocks is eight trips of twenty barriers (one size per thread and trip was 128 of them, 0.4 ms).
#define PK_SCAN_PER 16
__global__ __launch_bounds__(1024) void k_pk_scan(const u32 *size, u64 *off, int base, int nb)
{
    __shared__ u64 part[1024];
    __shared__ u64 carry;
    const u32 t = threadIdx.x;
    if (t == 0) {
        if (base == 0) off[0] = 0ull;
        carry = base == 0 ? 0ull : off[base];
    }
    __syncthreads();
    for (int at = 0; at < nb; at += 1024 * PK_SCAN_PER) {
        const int b0 = at + (int)t * PK_SCAN_PER;
        u32 v[PK_SCAN_PER];
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < PK_SCAN_PER; j++) { v[j] = b0 + j < nb ? size[base + b0 + j] : 0u; mine += v[j]; }
        part[t] = mine;
        __syncthreads();
        for (u32 d = 1; d < 1024u; d <<= 1) {
            const u64 add = t >= d ? part[t - d] : 0ull;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        u64 run = carry + part[t] - mine;                             // what lies before this thread's first block
#pragma unroll
        for (int j = 0; j < PK_SCAN_PER; j++) { run += v[j]; if (b0 + j < nb) off[base + b0 + j + 1] = run; }
        __syncthreads();
        if (t == 1023) carry += part[1023];
        __syncthreads();
    }
}

// gathered route: block i's result from its internal slot to out + off[i] (k_pack_results' loop, r4x16_host.hip, with
// the descriptor computed here), and the capacity rule
__global__ __launch_bounds__(256) void k_pk_gather(PackedOut pk, const u8 *slots, const u64 *slot_off, const u32 *slot_cap,
                                                   u32 *out_size, i32 *status, int base)
{
    const u32 tid = threadIdx.x;
    const int i = base + (int)blockIdx.x;
    const u32 sz = out_size[i];
    const u64 at = pk.off[i], end = pk.off[i + 1];
    if (sz == 0) {
        if (tid == 0 && status[i] == ST_CAPACITY && slot_cap[i] == 0) status[i] = ST_UNSUPPORTED;
        return;
    }
    if (end > pk.capacity) {
        if (tid == 0) { status[i] = ST_CAPACITY; out_size[i] = 0; }
        return;
    }
    group_copy<256>(pk.out + at, slots + slot_off[i], sz, tid);
}

// ---- peek ----------------------------------------------------------------------------------------------------
// (peek_one, the first byte and the stored uncompressed size of one rANS 4x16 stream: r4x16_best_any.h)
// The same for a rANS 4x8 stream (rANS_static.c:934-943): the order byte, and the uncompressed size in bytes 5..8; a
// stream of fewer than 9 bytes has none (:938).  Nothing else is judged here: the decoder does that.
static __device__ __forceinline__ i32 peek_one8(const u8 *in, u32 in_size, u32 max_in, i32 *format, u32 *raw)
{
    *format = -1; *raw = PK_NO_SIZE;
    if (in_size == 0) return ST_EMPTY;
    if (in_size > max_in) return ST_UNSUPPORTED;
    *format = (i32)in[0];
    if (in_size < 9) return ST_TRUNCATED;
    *raw = (u32)in[5] | ((u32)in[6] << 8) | ((u32)in[7] << 16) | ((u32)in[8] << 24);
    return ST_OK;
}

// X8: the blocks are rANS 4x8 streams
template <bool X8>
__global__ __launch_bounds__(256) void k_peek(const u8 *in, const u64 *in_off, const u32 *in_size, i32 *format, u32 *raw_size,
                                              i32 *status, int n, u32 max_in)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 f; u32 r;
    status[i] = X8 ? peek_one8(in + in_off[i], in_size[i], max_in, &f, &r) : peek_one(in + in_off[i], in_size[i], max_in, &f, &r);
    format[i] = f; raw_size[i] = r;
}

// ---- packed decode -------------------------------------------------------------------------------------------
struct UnpkWs { u32 *claim, *in_size; i32 *pre; };   // [n] each, in the context's packed arena

// what block i asks for: its stored size, or the caller's for an X_NOSZ stream; 0 and a status where it may not run
// (X8: a rANS 4x8 stream always carries its size)
template <bool X8>
__global__ __launch_bounds__(256) void k_unpk_claim(const u8 *in, const u64 *in_off, const u32 *in_size, const u32 *nosz_size,
                                                    UnpkWs w, int n, u32 max_in, u32 max_out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 f; u32 claim;
    i32 st = X8 ? peek_one8(in + in_off[i], in_size[i], max_in, &f, &claim) : peek_one(in + in_off[i], in_size[i], max_in, &f, &claim);
    if (!X8 && st == ST_OK && !(f & X_STRIPE) && (f & X_NOSZ)) {                            // the stream carries no size: the caller's
        if (nosz_size) claim = nosz_size[i]; else st = ST_SIZE;
    }
    if (st == ST_OK && claim > max_out) st = ST_UNSUPPORTED;                          // hostile, or larger than announced
    w.claim[i] = st == ST_OK ? claim : 0u;
    w.pre[i] = st;
}

// after the scan: a block whose range ends beyond the capacity is withdrawn too; withdrawn blocks reach the decoder
// with an empty input, so that nothing of them is read or written
__global__ __launch_bounds__(256) void k_unpk_admit(const u32 *in_size, UnpkWs w, PackedOut pk, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 st = w.pre[i];
    if (st == ST_OK && pk.off[i + 1] > pk.capacity) { st = ST_CAPACITY; w.pre[i] = st; }
    w.in_size[i] = st == ST_OK ? in_size[i] : 0u;
}

__global__ __launch_bounds__(256) void k_unpk_verdict(UnpkWs w, u32 *out_size, i32 *status, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    if (w.pre[i] != ST_OK) { status[i] = w.pre[i]; out_size[i] = 0; }
    else if (status[i] != ST_OK) out_size[i] = 0;
}

// ---- host ----------------------------------------------------------------------------------------------------
size_t r4x16_packed_carve(PackedSlots *p, u8 *base, size_t n, size_t chunk, u64 stride)
{
    Carver cv(base);
    p->slot_off = cv.take<u64>(n);
    p->slot_cap = cv.take<u32>(n);
    p->slots = cv.take<u8>(chunk * stride + 256);
    p->stride = stride;
    return cv.total();
}

u64 r4x16_packed_stride(u32 max_in_size, int order, bool any_order)
{
    // per-block orders: the largest bound any order byte and plane count up to 255 can ask for
    const int worst = any_order ? ((255 << 8) | X_STRIPE | X_PACK | X_RLE | 1) : order;
    return align_up((size_t)r4x16_bound_hd(max_in_size, worst) + 64, 256);
}

void r4x16_launch_packed_slots(const BatchArgs *a, const PackedSlots *p, int n, size_t chunk, u32 max_in_size, hipStream_t s)
{
    PkMethods pm = {};
    hipLaunchKernelGGL(k_pk_slots, dim3((n + 255) / 256), dim3(256), 0, s, a->in_size, a->d_order, a->order, pm, n, (u32)chunk,
                       p->stride, max_in_size, p->slot_off, p->slot_cap);
}

void r4x16_launch_packed_slots_best(const u32 *d_in_size, int k, const int *methods, const PackedSlots *p, int n, size_t chunk,
                                    u32 max_in_size, hipStream_t s)
{
    PkMethods pm = {};
    pm.k = k;
    for (int j = 0; j < k; j++) pm.m[j] = methods[j];
    hipLaunchKernelGGL(k_pk_slots, dim3((n + 255) / 256), dim3(256), 0, s, d_in_size, (const i32 *)nullptr, 0, pm, n, (u32)chunk, p->stride,
                       max_in_size, p->slot_off, p->slot_cap);
}

extern "C" void r4x16_launch_packed_scan(const u32 *size, u64 *off, int base, int nb, hipStream_t s)
{
    hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, s, size, off, base, nb);
}

// The gathered route: the existing slot call over a chunk of blocks into the internal slots, then scan and copy.
// pm.k > 0: best-of-k over pm.m[]; else the call's order / d_order.  The slot arena takes at most a quarter of what the
// call may hold; the inner call plans its own arenas (workspace, candidates, stripe items) under the rest.
static int gathered(rans4x16_hip_ctx *c, int n, const BatchArgs &a, const PackedOut &pk, const PkMethods &pm, i32 *d_chosen,
                    uint32_t max_in_size, uint64_t total_in_size, hipStream_t s)
{
    u64 stride = 0;
    if (pm.k == 0) stride = r4x16_packed_stride(max_in_size, a.order, a.d_order != nullptr);
    else
        for (int j = 0; j < pm.k; j++) stride = std::max(stride, r4x16_packed_stride(max_in_size, pm.m[j], false));
    PackedSlots p;
    size_t arena = 0;
    auto slots_for = [&](size_t nb) { return r4x16_packed_carve(&p, nullptr, (size_t)n, nb, stride); };
    const size_t room = r4x16_room(c, A_BIT(A_WS) | A_BIT(A_XS) | A_BIT(A_PS));
    const size_t chunk = r4x16_fit_chunk((size_t)n, SIZE_MAX, room / 4, slots_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_PS, slots_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        if (base == 0) {                               // the layout of the call: nb is the chunk size here
            arena = r4x16_packed_carve(&p, c->at(A_PS), (size_t)n, (size_t)nb, stride);
            hipLaunchKernelGGL(k_pk_slots, dim3((n + 255) / 256), dim3(256), 0, s, a.in_size, a.d_order, a.order, pm, n, (u32)nb, stride,
                               max_in_size, p.slot_off, p.slot_cap);
        }
        const u64 total = total_in_size ? std::min<u64>(total_in_size, (u64)nb * max_in_size) : 0;
        {
            // the inner call: what is left of the ceiling beside this call's slots
            Keep<size_t> ceiling(c->max_ws, c->max_ws > arena + ((size_t)1 << 20) ? c->max_ws - arena : (size_t)1 << 20);
            Keep<bool> inner(c->in_packed, true);
            const int rc = pm.k
                ? rans4x16_hip_compress_best_dev(c, nb, a.in, a.in_off + base, a.in_size + base, p.slots, p.slot_off + base, p.slot_cap + base,
                                                 a.out_size + base, a.status + base, pm.k, pm.m, d_chosen ? d_chosen + base : nullptr,
                                                 max_in_size, total, s)
                : rans4x16_hip_compress_dev_sized(c, nb, a.in, a.in_off + base, a.in_size + base, p.slots, p.slot_off + base, p.slot_cap + base,
                                                  a.out_size + base, a.status + base, a.order, a.d_order ? a.d_order + base : nullptr,
                                                  max_in_size, total, s);
            if (rc != 0) return -1;
        }
        hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, s, (const u32 *)a.out_size, pk.off, (int)base, nb);
        hipLaunchKernelGGL(k_pk_gather, dim3((u32)nb), dim3(256), 0, s, pk, (const u8 *)p.slots, (const u64 *)p.slot_off,
                           (const u32 *)p.slot_cap, a.out_size, a.status, (int)base);
        if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_RESULT][R4X16_RESULT_GATHERED] += nb;
        return 0;
    });
}

extern "C" int rans4x16_hip_compress_packed_dev(rans4x16_hip_ctx *c, int n,
                                                const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                                uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "compress_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size, d_out,
                                          out_capacity, d_out_off, d_out_size, d_status, order, d_order, s);
    if (go <= 0) return go;
    const bool stripes = d_order ? c->dev_stripe_enc > 0 : (order & X_STRIPE) != 0;
    if (!stripes) return r4x16_enc_run(c, a, max_in_size, total_in_size, s, &pk);
    if (!d_order && ((unsigned)order >> 8) > 255) { c->err = "compress_packed_dev: more than 255 stripes"; return -1; }
    PkMethods pm = {};
    return gathered(c, n, a, pk, pm, nullptr, max_in_size, total_in_size, s);
}

extern "C" int rans4x16_hip_compress_best_packed_dev(rans4x16_hip_ctx *c, int n,
                                                     const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                     unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                     uint32_t *d_out_size, int32_t *d_status,
                                                     int k, const int *methods, int32_t *d_chosen,
                                                     uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    PkMethods pm = {};
    auto table = [&] {
        pm.k = k;
        for (int j = 0; j < k; j++) {
            if ((methods[j] & X_STRIPE) && ((unsigned)methods[j] >> 8) > 255) { c->err = "compress_best_packed_dev: more than 255 stripes"; return -1; }
            pm.m[j] = methods[j];
        }
        return 0;
    };
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "compress_best_packed_dev: bad arguments", k >= 1 && k <= PK_MAX_K && methods, &a, &pk, n, d_in,
                                          d_in_off, d_in_size, d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s, table);
    if (go <= 0) return go;
    return gathered(c, n, a, pk, pm, d_chosen, max_in_size, total_in_size, s);
}

extern "C" int rans4x16_hip_peek_dev(rans4x16_hip_ctx *c, int n,
                                     const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                     int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status,
                                     uint32_t max_in_size, void *stream)
{
    if (!c) return -1;
    if (n < 0 || (n && (!d_in || !d_in_off || !d_in_size || !d_format || !d_raw_size || !d_status))) {
        c->err = "peek_dev: bad arguments";
        return -1;
    }
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_peek<false>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_in_off, d_in_size, d_format, d_raw_size,
                       d_status, n, max_in_size);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The packed decode of either codec: claims, offsets, admission, the slot call with capacity = claim, verdicts.
template <bool X8>
static int unpack_run(rans4x16_hip_ctx *c, const BatchArgs &a, const PackedOut &pk, const uint32_t *d_nosz_size, uint32_t max_in_size,
                      uint32_t max_out_size, hipStream_t s)
{
    const int n = a.n;
    // the layout's own arrays: 12 bytes per block in the packed arena (ordered between streams like the workspace)
    if (r4x16_ensure(c, A_PS, 3 * align_up((size_t)n * 4, 256), false) != 0) return -1;
    Carver cv(c->at(A_PS));
    UnpkWs w;
    w.claim = cv.take<u32>(n); w.in_size = cv.take<u32>(n); w.pre = cv.take<i32>(n);
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const dim3 grid((n + 255) / 256), wg(256);
    hipLaunchKernelGGL(k_unpk_claim<X8>, grid, wg, 0, s, a.in, a.in_off, a.in_size, d_nosz_size, w, n, max_in_size, max_out_size);
    hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, s, (const u32 *)w.claim, pk.off, 0, n);
    hipLaunchKernelGGL(k_unpk_admit, grid, wg, 0, s, a.in_size, w, pk, n);
    // every admitted block ends inside the capacity, so the capacities of the transformed blocks together do too
    const u64 total = std::max<u64>(std::min<u64>(pk.capacity, (u64)n * max_out_size), 1);
    // rANS 4x8's sizing pass (no arena, capacity 0): only blocks that claim 0 bytes are admitted and nothing is written,
    // but the slot call wants a pointer - the packed arena's own
    unsigned char *out8 = pk.out ? pk.out : c->at(A_PS);
    const int rc = X8 ? rans4x8_hip_uncompress_dev(c, n, a.in, a.in_off, w.in_size, out8, pk.off, w.claim, a.out_size, a.status, s)
                      : rans4x16_hip_uncompress_dev_sized(c, n, a.in, a.in_off, w.in_size, pk.out, pk.off, w.claim, a.out_size, a.status,
                                                          max_in_size, max_out_size, total, s);
    if (rc != 0) return -1;
    hipLaunchKernelGGL(k_unpk_verdict, grid, wg, 0, s, w, a.out_size, a.status, n);
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}

extern "C" int rans4x16_hip_uncompress_packed_dev(rans4x16_hip_ctx *c, int n,
                                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                  unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                  uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                                  uint32_t max_in_size, uint32_t max_out_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "uncompress_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size, d_out,
                                          out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    return unpack_run<false>(c, a, pk, d_nosz_size, max_in_size, max_out_size, s);
}

// ---- rANS 4x8 (include/rans4x8_hip.h) --------------------------------------------------------------------------
static int pick8_methods(rans4x16_hip_ctx *c, int k, const int *methods, Enc8Sel *sel, const char *who)
{
    if (k < 1 || k > 2 || !methods) { c->err = std::string(who) + ": k must be 1 or 2"; return -1; }
    sel->k = k;
    for (int j = 0; j < k; j++) {
        if (methods[j] != 0 && methods[j] != 1) { c->err = std::string(who) + ": a method must be 0 or 1"; return -1; }
        sel->m[j] = methods[j];
    }
    return 0;
}

extern "C" int rans4x8_hip_compress_packed_dev(rans4x16_hip_ctx *c, int n,
                                               const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                               unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                               uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                               uint32_t max_in_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "rans4x8 compress_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size, d_out,
                                          out_capacity, d_out_off, d_out_size, d_status, order, d_order, s);
    if (go <= 0) return go;
    return r4x8_enc_run(c, a, max_in_size, s, &pk, nullptr);
}

extern "C" int rans4x8_hip_compress_best_dev(rans4x16_hip_ctx *c, int n,
                                             const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                             unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                             uint32_t *d_out_size, int32_t *d_status,
                                             int k, const int *methods, int32_t *d_chosen, uint32_t max_in_size, void *stream)
{
    Enc8Sel sel = {};
    BatchArgs a;
    const int go = r4x16_dev_call_args(c, "rans4x8 compress_best_dev: bad arguments", true, &a, n, d_in, d_in_off, d_in_size, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, 0, nullptr,
                                       [&] { return pick8_methods(c, k, methods, &sel, "rans4x8 compress_best_dev"); });
    if (go <= 0) return go;
    sel.d_chosen = d_chosen;
    return r4x8_enc_run(c, a, max_in_size, (hipStream_t)stream, nullptr, &sel);
}

extern "C" int rans4x8_hip_compress_best_packed_dev(rans4x16_hip_ctx *c, int n,
                                                    const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                    unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                    uint32_t *d_out_size, int32_t *d_status,
                                                    int k, const int *methods, int32_t *d_chosen, uint32_t max_in_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    Enc8Sel sel = {};
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "rans4x8 compress_best_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size,
                                          d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s,
                                          [&] { return pick8_methods(c, k, methods, &sel, "rans4x8 compress_best_packed_dev"); });
    if (go <= 0) return go;
    sel.d_chosen = d_chosen;
    return r4x8_enc_run(c, a, max_in_size, s, &pk, &sel);
}

extern "C" int rans4x8_hip_peek_dev(rans4x16_hip_ctx *c, int n,
                                    const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                    int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status, uint32_t max_in_size, void *stream)
{
    if (!c) return -1;
    if (n < 0 || (n && (!d_in || !d_in_off || !d_in_size || !d_format || !d_raw_size || !d_status))) {
        c->err = "rans4x8 peek_dev: bad arguments";
        return -1;
    }
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_peek<true>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_in_off, d_in_size, d_format,
                       d_raw_size, d_status, n, max_in_size);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int rans4x8_hip_uncompress_packed_dev(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                 unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                 uint32_t *d_out_size, int32_t *d_status,
                                                 uint32_t max_in_size, uint32_t max_out_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "rans4x8 uncompress_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size,
                                          d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    return unpack_run<true>(c, a, pk, nullptr, max_in_size, max_out_size, s);
}
