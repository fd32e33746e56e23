// r4x16_arith.hip - decoding of htscodecs' adaptive arithmetic codec (arith_dynamic.c, c_simple_model.h, c_range_coder.h)
// on the device: include/rans4x16_hip.h part 2g.
//
// Nothing of this codec is tabled up front: a stream is one serial chain of dependent steps, each of which reads the
// model the step before it changed.  The parallelism is inside a step - the model's list, up to 256 entries, lies across
// the wave - and across streams: one wave per stream.  Three stages, as in the rANS decoder:
//   k_ar_front   one wave per block: the header walk (r4x16_arith_parse.h), the block's items - one per plain block, N per
//                X_STRIPE block - and their places in the stage arena
//   k_ar_decode  one wave per item: the range coder and the models (the hot loop)
//   k_ar_back    a workgroup per block: unpack X_PACK pieces, copy X_CAT pieces, un-stripe, sizes and statuses
//
// The step (ar_symbol: r4x16_arith_step.h), where the models live (order 0: registers; run-length models: LDS; order-1
// rows: LDS up to the budget, else a slot of the context's arena - the homes of r4x16_arith_model.h, which the encoder
// shares) and what was measured: DESIGN 4.6, profiles/arith.md.  The device call and the host round trip are built on
// r4x16_dev_call_args / r4x16_chunk_walk / r4x16_route_begin, _end / r4x16_host_trip (r4x16_host.h).
//
// Loops: every loop is bounded by the item's output size or input size (each trip writes an output byte or consumes an
// input byte, or adds 3 to a run that ends the loop at the output size), both checked against max_in_size /
// max_out_size by k_ar_front; an item that has no work enters none.  All stores are plain vector stores.
#include "r4x16_host.h"
#include "r4x16_arith_parse.h"
#include "r4x16_arith_step.h"

enum { AR_HOME_O0 = 0, AR_HOME_O1_LDS = 1, AR_HOME_O1_GLOBAL = 2, AR_HOME_NONE = 3 };

struct ArItem {
    u64 in;                 // the payload in d_in
    u64 stage;              // the decoded bytes in the stage arena
    u32 in_size, dec_size, out_size;
    u8 kind, nsym, home, pad;
    u8 map[16];
};
struct ArBlk { i32 status; u32 out_size, nplanes, pad; };
struct ArWs {
    ArItem *items;          // [nb * per]: block b's items from b * per
    ArBlk *blk;             // [nb]
    u64 *cursor;            // [0] bytes of the stage arena handed out (a chunk's); [1] bytes decoded into the caller's slots (the call's)
    u32 *route;             // [R4X16_ARITH_KINDS]; nullptr in the kernels' copy: option route_count is off
    u8 *stage;
    u64 stage_bytes;
    u64 out_total;          // total_out_size: what the call's blocks may decode to together
    u8 *rows;               // [AR_GLOBAL_SLOTS] x AR_GLOBAL_ROW_BYTES
    u32 per;                // items a block reserves: max(1, planes)
    u32 planes, stripe_out; // rans4x16_hip_set_dev_stripe_planes
};

// ---- front ------------------------------------------------------------------------------------------------------
struct ArDevSink {
    ArItem *items; u64 in_base; u32 lane; u32 need; const u8 *in;
    __device__ void put(u32 j, const ArPiece &pc)
    {
        if (lane != 0) return;
        ArItem it;
        it.in = in_base + pc.in_pos; it.stage = need;
        it.in_size = pc.in_size; it.dec_size = pc.dec_size; it.out_size = pc.out_size;
        it.kind = pc.kind; it.nsym = pc.nsym; it.pad = 0;
        it.home = AR_HOME_NONE;
        if (pc.kind == AR_K_O0 || pc.kind == AR_K_O0_RLE) it.home = AR_HOME_O0;
        else if (pc.kind == AR_K_O1 || pc.kind == AR_K_O1_RLE) {
            const u32 m = in[pc.in_pos] ? in[pc.in_pos] : 256u;
            it.home = ar_lds_home(m) ? AR_HOME_O1_LDS : AR_HOME_O1_GLOBAL;
        }
        for (int k = 0; k < 16; k++) it.map[k] = pc.map[k];
        items[j] = it;
        if (it.home != AR_HOME_NONE) need += ar_r16(pc.dec_size);
    }
};

__global__ __launch_bounds__(256) void k_ar_front(BatchArgs a, ArWs w, int base, int nb, u32 max_in, u32 max_out)
{
    const u32 lane = threadIdx.x & 63u;
    const int b = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nb) return;
    const int g = base + b;
    const u32 size = a.in_size[g], cap = a.out_cap[g];
    ArItem *items = w.items + (size_t)b * w.per;
    ArTop top = {0, 0, 0};
    int st;
    u32 need = 0;
    if (size > max_in) st = AR_E_UNSUPPORTED;                       // larger than the call was sized for: not read
    else {
        ByteSrc src(a.in + a.in_off[g]);
        ArDevSink sink{items, a.in_off[g], lane, 0u, a.in + a.in_off[g]};
        st = ar_parse(src, size, cap, w.planes, w.stripe_out, &top, sink);
        if (st == AR_OK && top.out_size > max_out) st = AR_E_UNSUPPORTED;
        need = sink.need;
    }
    wsync();                                                        // lane 0's items are written before any lane marks the rest
    u32 live = st == AR_OK ? ((top.flags & AR_X_STRIPE) ? top.nplanes : 1u) : 0u;
    if (lane == 0 && live) {
        // the block's share of the announced total and its place in the stage arena.  A batch that decodes to more than it
        // announced does not fit: the blocks that find the total spent are refused, whichever they are (a refused block's
        // claim on the total stays taken).  Only a block within the total takes a place in the arena, which holds the
        // total and 16 bytes an item: it finds one, and the test of the place is the bound of the decoders' stores
        const u64 sum = top.out_size ? atomicAdd((unsigned long long *)w.cursor + 1, (unsigned long long)top.out_size) : 0ull;
        const bool fits = sum + top.out_size <= w.out_total;
        const u64 at = fits && need ? atomicAdd((unsigned long long *)w.cursor, (unsigned long long)need) : 0ull;
        if (!fits || at + need > w.stage_bytes) { st = AR_E_UNSUPPORTED; live = 0; }
        else
            for (u32 j = 0; j < live; j++) {
                items[j].stage += at;
                if (w.route && items[j].home != AR_HOME_NONE) {
                    atomicAdd(&w.route[items[j].home], 1u);
                    if (items[j].kind == AR_K_O0_RLE || items[j].kind == AR_K_O1_RLE) atomicAdd(&w.route[R4X16_ARITH_RLE], 1u);
                }
            }
    }
    st = __builtin_amdgcn_readfirstlane(st);
    live = (u32)__builtin_amdgcn_readfirstlane((int)live);
    for (u32 j = live + lane; j < w.per; j += WAVE) { items[j].kind = AR_K_NONE; items[j].home = AR_HOME_NONE; }
    if (lane == 0) {
        ArBlk bk;
        bk.status = st; bk.out_size = st == AR_OK ? top.out_size : 0u; bk.nplanes = st == AR_OK ? top.nplanes : 0u; bk.pad = 0;
        w.blk[b] = bk;
    }
}

// One symbol of a run-length model (SIMPLE_MODEL(258,_decodeSymbol) after _init(.., 4)): four live entries, held by every
// lane alike
__device__ __forceinline__ u32 ar_run_symbol(u32x4 &e, ArCoder &rc, u32 lane)
{
    const u32 c0 = e.x & 0xffffu, c1 = c0 + (e.y & 0xffffu), c2 = c1 + (e.z & 0xffffu), c3 = c2 + (e.w & 0xffffu);
    const u32 freq = rc.get_freq(c3);
    if (freq > AR_MAX_FREQ || freq >= c3) return 0;
    const u32 j = (u32)(c0 <= freq) + (u32)(c1 <= freq) + (u32)(c2 <= freq);
    const u32 ent = ar_get(e, j);
    rc.decode(j == 0 ? 0u : j == 1 ? c0 : j == 2 ? c1 : c2, ent & 0xffffu, lane);
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
    return ent >> 16;
}

// HOME: AR_HOME_*.  One wave per item, the items of other homes passed over; the global home's waves stride over the items,
// each with the row slot of its workgroup.
template <int HOME>
__global__ __launch_bounds__(64) void k_ar_decode(const u8 *in, ArWs w, int nitems)
{
    __shared__ __attribute__((aligned(16))) u32 lds[(HOME == AR_HOME_O1_LDS ? AR_LDS_BUDGET : AR_RUN_BYTES) / 4];
    const u32 lane = threadIdx.x;
    u32x4 *runs = (u32x4 *)lds;
    for (int it = (int)blockIdx.x; it < nitems; it += (int)gridDim.x) {
        const ArItem *item = w.items + it;
        if (item->home != HOME) continue;
        const bool rle = item->kind == AR_K_O0_RLE || item->kind == AR_K_O1_RLE;
        const u8 *src = in + item->in;
        const u32 out_sz = item->dec_size;
        const u32 m = src[0] ? src[0] : 256u;                        // the alphabet byte: 0 means 256
        const u32 stride = ar_row_stride(m);
        const ArHome h = ar_home(HOME == AR_HOME_O1_LDS, lds, w.rows, m, stride);
        if (rle) ar_runs_init(lds, lane);
        u32x4 e = {0, 0, 0, 0};
        u32 tot = m;
        if (HOME == AR_HOME_O0) e = ar_fresh(4u * lane, m);
        else {
            for (u32 k = lane; k < m * stride; k += WAVE) { const u32 s = k % stride; h.rows[k] = s < m ? 1u | (s << 16) : 0u; }
            for (u32 k = lane; k < m; k += WAVE) h.tots[k] = m;
        }
        wsync();
        ArCoder rc(src, item->in_size, lane);
        ArBytes out{(u32 *)(w.stage + item->stage), 0u, 0u};
        u32 last = 0;
        const bool mine = 4u * lane < stride;
        while (out.n < out_sz) {
            bool dirty;
            u32 c;
            if (HOME == AR_HOME_O0) c = ar_symbol(e, tot, rc, lane, &dirty);
            else {
                u32x4 *row = (u32x4 *)(h.rows + last * stride);
                e = mine ? row[lane] : u32x4{0, 0, 0, 0};
                tot = h.tots[last];
                c = ar_symbol(e, tot, rc, lane, &dirty);
                if (dirty && mine) row[lane] = e;
                if (lane == 0) h.tots[last] = tot;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next step's row may be this one
            }
            out.put(c, lane);
            last = c;
            if (rle) {
                u32 run = 0, r, rctx = last;
                do {
                    u32x4 re = runs[rctx];
                    r = ar_run_symbol(re, rc, lane);
                    if (lane == 0) runs[rctx] = re;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    rctx = rctx == last ? 256u : rctx + (rctx < AR_NRUN - 1u);
                    run += r;
                } while (r == 3 && run < out_sz);                                  // arith_dynamic.c:491, :606
                while (run-- && out.n < out_sz) out.put(last, lane);               // :492, :607 (i + 1 < out_sz)
            }
        }
        out.flush(lane);
        wsync();                                                                   // the next item's models overwrite these
    }
}

// ---- back -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u8 ar_piece_byte(const ArItem &it, const u8 *src, u32 i)
{
    if (it.nsym == AR_NOT_PACKED || it.nsym == 1) return src[i];
    if (it.nsym == 0) return it.map[0];
    const u32 bits = 8u / it.nsym;
    return it.map[(src[i / it.nsym] >> (bits * (i % it.nsym))) & ((1u << bits) - 1u)];
}

__global__ __launch_bounds__(256) void k_ar_back(BatchArgs a, ArWs w, int base)
{
    __shared__ ArItem sh[255];
    const int b = (int)blockIdx.x, g = base + b;
    const u32 t = threadIdx.x;
    const ArBlk bk = w.blk[b];
    if (t == 0) { a.status[g] = bk.status; a.out_size[g] = bk.out_size; }
    if (bk.status != AR_OK || bk.out_size == 0) return;
    const u32 N = bk.nplanes ? bk.nplanes : 1u;
    const ArItem *items = w.items + (size_t)b * w.per;
    for (u32 j = t; j < N; j += 256) sh[j] = items[j];
    __syncthreads();
    u8 *dst = a.out + a.out_off[g];
    const u32 n = bk.out_size;                                       // <= the slot's capacity (the walk's test)
    if (N == 1) {
        const ArItem &it = sh[0];
        const u8 *src = it.kind == AR_K_CAT ? a.in + it.in : w.stage + it.stage;
        if (it.nsym == AR_NOT_PACKED || it.nsym == 1) group_copy<256>(dst, src, n, t);
        else for (u32 x = t; x < n; x += 256) dst[x] = ar_piece_byte(it, src, x);
        return;
    }
    for (u32 x = t; x < n; x += 256) {                                // utils.h unstripe: byte x is byte x / N of plane x % N
        const ArItem &it = sh[x % N];
        const u8 *src = it.kind == AR_K_CAT ? a.in + it.in : w.stage + it.stage;
        dst[x] = ar_piece_byte(it, src, x / N);
    }
}

// ---- the device call ----------------------------------------------------------------------------------------------
static size_t ar_layout(u8 *base, size_t nb, size_t per, u64 stage_bytes, ArWs *w)
{
    Carver cv(base);
    w->cursor = cv.take<u64>(2);                                    // first: the call's count keeps its place from chunk to chunk
    w->items = cv.take<ArItem>(nb * per);
    w->blk = cv.take<ArBlk>(nb);
    w->route = cv.take<u32>(R4X16_ARITH_KINDS);
    w->stage = cv.take<u8>(stage_bytes);
    w->stage_bytes = stage_bytes;
    w->rows = cv.take<u8>((size_t)std::min<size_t>(nb * per, AR_GLOBAL_SLOTS) * AR_GLOBAL_ROW_BYTES);
    w->per = (u32)per;
    return cv.total();
}

extern "C" int rans4x16_hip_arith_uncompress_dev(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                 unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                                 uint32_t *d_out_size, int32_t *d_status,
                                                 uint32_t max_in_size, uint32_t max_out_size, uint64_t total_out_size, void *stream)
{
    BatchArgs a;
    const int go = r4x16_dev_call_args(c, "arith_uncompress_dev: bad arguments", true, &a, n, d_in, d_in_off, d_in_size, d_out, d_out_off,
                                       d_out_cap, d_out_size, d_status, 0, nullptr);
    if (go <= 0) return go;
    hipStream_t s = (hipStream_t)stream;
    const size_t per = c->dev_stripe_planes > 0 ? (size_t)c->dev_stripe_planes : 1;
    // every item's decoded bytes wait in the stage arena, each rounded up to 16: the caller's total, or n x the largest
    const u64 total = total_out_size ? total_out_size : (u64)n * max_out_size;
    ArWs w;
    auto layout = [&](u8 *at, size_t nb) {
        const u64 tot = std::min<u64>(total, (u64)nb * max_out_size);
        return ar_layout(at, nb, per, tot + 16ull * nb * per, &w);
    };
    auto bytes_for = [&](size_t nb) { return layout(nullptr, nb); };
    const size_t chunk = r4x16_fit_chunk((size_t)n, (size_t)INT_MAX / per, r4x16_room(c, A_BIT(A_AR)), bytes_for);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, bytes_for(nb), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        if (base == 0) HIPCHK(c, hipMemsetAsync(c->at(A_AR), 0, 2 * sizeof(u64), s));
        layout(c->at(A_AR), (size_t)nb);
        w.out_total = total;
        w.planes = (u32)c->dev_stripe_planes; w.stripe_out = c->dev_stripe_out;
        const int nitems = nb * (int)per;
        u32 *const d_route = w.route;
        HIPCHK(c, hipMemsetAsync(w.cursor, 0, sizeof(u64), s));
        if (r4x16_route_begin(c, &w.route, R4X16_ARITH_KINDS, s) != 0) return -1;
        hipLaunchKernelGGL(k_ar_front, dim3((nb + 3) / 4), dim3(256), 0, s, a, w, (int)base, nb, max_in_size, max_out_size);
        hipLaunchKernelGGL(k_ar_decode<AR_HOME_O0>, dim3(nitems), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_ar_decode<AR_HOME_O1_LDS>, dim3(nitems), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_ar_decode<AR_HOME_O1_GLOBAL>, dim3(std::min(nitems, AR_GLOBAL_SLOTS)), dim3(64), 0, s, d_in, w, nitems);
        hipLaunchKernelGGL(k_ar_back, dim3(nb), dim3(256), 0, s, a, w, (int)base);
        return r4x16_route_end(c, R4X16_ROUTE_ARITH, d_route, R4X16_ARITH_KINDS, s);
    });
}

extern "C" int rans4x16_hip_arith_peek_dev(rans4x16_hip_ctx *c, int n,
                                           const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                           int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status,
                                           uint32_t max_in_size, void *stream)
{
    // the flag byte and the size varint lie where rANS 4x16 has them, with the same X_NOSZ and X_STRIPE bits: one reader
    return rans4x16_hip_peek_dev(c, n, d_in, d_in_off, d_in_size, d_format, d_raw_size, d_status, max_in_size, stream);
}

// ---- host buffers -------------------------------------------------------------------------------------------------
// One round trip (r4x16_host_trip).  X_STRIPE blocks are decoded as after rans4x16_hip_set_dev_stripe_planes(ctx, most
// planes of the batch, largest block); the caller's setting is put back.
struct ArNoSink { void put(u32, const ArPiece &) {} };

extern "C" int rans4x16_hip_arith_uncompress_batch(rans4x16_hip_ctx *c, int n,
                                                   const unsigned char *const *in, const unsigned int *in_size,
                                                   unsigned char *const *out, unsigned int *out_size, int *status)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !out || !out_size || !status))) { c->err = "arith_uncompress_batch: bad arguments"; return -1; }
    if (n == 0) return 0;
    // the host walk refuses what the device walk would refuse, before anything is uploaded, and gives the stripe limits
    std::vector<u32> isz(n, 0), cap(n, 0);
    std::vector<u8> take(n, 0);
    u32 max_in = 0, max_out = 0, planes = 0, stripe_out = 0;
    for (int i = 0; i < n; i++) {
        HostSrc src{in[i]};
        ArTop top;
        ArNoSink sink;
        status[i] = in[i] && out[i] ? ar_parse(src, in_size[i], out_size[i], 255u, 0xffffffffu, &top, sink) : R4X16_E_UNSUPPORTED;
        if (status[i] != AR_OK) { out_size[i] = 0; continue; }
        take[i] = 1; isz[i] = in_size[i]; cap[i] = out_size[i];
        max_in = std::max(max_in, isz[i]); max_out = std::max(max_out, cap[i]);
        if (top.nplanes) { planes = std::max(planes, top.nplanes); stripe_out = std::max(stripe_out, top.out_size); }
    }
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), nullptr, nullptr, 0, 0, nullptr};
    return r4x16_host_trip(c, n, trip, [&](const StageLayout &L, size_t, size_t out_total, hipStream_t s) {
        StripeLimits limits(c, (int)planes, stripe_out);
        return rans4x16_hip_arith_uncompress_dev(c, n, L.in, L.in_off, L.in_size, L.out, L.out_off, L.cap, L.osz, L.status, max_in, max_out,
                                                 out_total, s);
    });
}

// ---- the reference's two calls (arith_dynamic.h), on the calling thread's context ---------------------------------
extern "C" unsigned char *rans4x16_hip_arith_uncompress_to(unsigned char *in, unsigned int in_size,
                                                          unsigned char *out, unsigned int *out_size)
{
    if (!in || !out_size || in_size == 0) return nullptr;
    HostSrc src{in};
    ArTop top;
    ArNoSink sink;
    if (ar_parse(src, in_size, out ? *out_size : AR_NO_CAP, 255u, 0xffffffffu, &top, sink) != AR_OK) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    // out == NULL: the capacity is the size the stream stores (:893, :984) - the walk above refused a stream that stores none
    unsigned int cap = out ? *out_size : top.out_size;
    if (!out && !(top.flags & AR_X_STRIPE)) ar_var_get(src, 1u, in_size, &cap);
    unsigned char *buf = out ? out : (unsigned char *)malloc(cap ? cap : 1);
    if (!buf) return nullptr;
    const unsigned char *ins[1] = {in};
    unsigned char *outs[1] = {buf};
    unsigned int osz[1] = {cap};
    int st[1] = {0};
    const int rc = rans4x16_hip_arith_uncompress_batch(c, 1, ins, &in_size, outs, osz, st);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || st[0] != 0) { if (!out) free(buf); return nullptr; }
    *out_size = osz[0];
    return buf;
}

extern "C" unsigned char *rans4x16_hip_arith_uncompress(unsigned char *in, unsigned int in_size, unsigned int *out_size)
{
    return rans4x16_hip_arith_uncompress_to(in, in_size, nullptr, out_size);
}
