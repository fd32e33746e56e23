// r4x16_best_any.hip - "try k methods, keep the smallest" across codecs for device-resident batches, rANS 4x16 against
// arith_dynamic, and the decode of the mixed arena it leaves: include/rans4x16_hip.h part 2m.
//
// Encode, per chunk of blocks, on the caller's stream and without a read-back:
//   rANS    : the rANS sub-list through rans4x16_hip_compress_best_dev into bound-sized slots of this call (the packed
//             calls' gathered route without its scan and gather, r4x16_packed.hip): k_best_pick leaves a winner a block
//   arith   : the arith sub-list through r4x16_ab_candidates (r4x16_arith_enc.hip): k_ab_pick leaves a winner a block
//   k_any_pick   : a thread a block compares the two winners - size, then position in the caller's list - and writes the
//                  block's size, status and tagged method
//   k_pk_scan    : the winners' sizes to offsets, carried on from the chunk before
//   k_any_gather : a workgroup a block copies the winner from whichever arena holds it to its final place
// Both codecs' results wait in arrays of this call; neither writes the caller's arrays, so a sub-list of one codec gives
// what that codec's own best-packed call gives.  The packed arena holds this call's arrays, the rANS slots and the arith
// candidates' slots behind each other; the rANS call plans its candidate arena and workspace (A_XS, A_WS), the arith call
// its own (A_AR), each under what the others leave of the ceiling (Keep on max_ws): any_fit plans a chunk by their sum.
//
// Decode: k_any_claim reads every stream's size field (peek_one: both codecs keep it in the same place), k_pk_scan lays the
// outputs out, k_any_admit gives each slot decoder the lengths of its own codec's admitted blocks and 0 for every other,
// both decoders run over the same entries into status and size arrays of their own, and k_any_verdict takes each block's
// from its codec's (the pattern of k_t3_admit / k_t3_verdict, r4x16_tok3.hip).
//
// Loops: trip counts are launch arguments (k <= 32) or sizes the codecs' own kernels wrote for slots they sized.  Stores:
// k_any_gather writes [off[i], off[i + 1]) of blocks that end inside the capacity, nothing else of the caller's arena.
#include "r4x16_host.h"
#include "r4x16_best_any.h"

#define ANY_MAX_K 32
enum { ANY_NONE = 0, ANY_RANS = 1, ANY_ARITH = 2 };
struct AnyMethods { int k; int m[ANY_MAX_K]; };          // the caller's list, tags included
struct AnyWs {
    u32 *r_size, *a_size; i32 *r_status, *a_status, *r_chosen, *a_chosen;      // [nb]: each codec's winner, by the block's place in the chunk
    u8 *side;                                                                  // [nb]: ANY_* of the chunk's blocks
    u32 *route;                                                                // [R4X16_BEST_ANY_KINDS]; nullptr in the kernels' copy: route_count is off
};

// where `word` of codec `tag` stands first in the list (a method that stands twice gives the same stream twice)
static __device__ __forceinline__ int any_pos(const AnyMethods &pm, int tag, int word)
{
    for (int j = 0; j < pm.k; j++)
        if ((pm.m[j] & R4X16_CODEC_MASK) == tag && (pm.m[j] & ~R4X16_CODEC_MASK) == word) return j;
    return pm.k;
}

// has_r / has_a: the list has methods of that codec (the arrays of a codec without one are not read).  slot_cap: the rANS
// slots' capacities, 0 for a block the slots were not sized for, whose CAPACITY is UNSUPPORTED (k_pk_gather's rule).
__global__ __launch_bounds__(256) void k_any_pick(AnyMethods pm, AnyWs w, const u32 *slot_cap, int has_r, int has_a, u32 *out_size,
                                                  i32 *status, i32 *chosen, int base, int nb)
{
    const int lb = (int)(blockIdx.x * 256u + threadIdx.x);
    if (lb >= nb) return;
    const int g = base + lb;
    i32 rs = ST_UNSUPPORTED, as = ST_UNSUPPORTED;
    u32 rsz = 0, asz = 0;
    if (has_r) {
        rs = w.r_status[lb]; rsz = w.r_size[lb];
        if (rsz == 0 && rs == ST_CAPACITY && slot_cap[lb] == 0) rs = ST_UNSUPPORTED;
    }
    if (has_a) { as = w.a_status[lb]; asz = w.a_size[lb]; }
    const bool r_ok = has_r && rs == ST_OK, a_ok = has_a && as == ST_OK;
    int side = r_ok ? ANY_RANS : a_ok ? ANY_ARITH : ANY_NONE;
    bool tie = false;
    if (r_ok && a_ok) {
        if (rsz != asz) side = asz < rsz ? ANY_ARITH : ANY_RANS;
        else {                                                                        // tokenise_name3.c:1281-1284 over the whole list
            tie = true;
            side = any_pos(pm, R4X16_CODEC_ARITH, w.a_chosen[lb]) < any_pos(pm, R4X16_CODEC_RANS4X16, w.r_chosen[lb]) ? ANY_ARITH : ANY_RANS;
        }
    }
    const bool first_arith = (pm.m[0] & R4X16_CODEC_MASK) == R4X16_CODEC_ARITH;
    w.side[lb] = (u8)side;
    out_size[g] = side == ANY_RANS ? rsz : side == ANY_ARITH ? asz : 0u;
    status[g] = side != ANY_NONE ? ST_OK : first_arith ? as : rs;
    if (chosen) chosen[g] = side == ANY_RANS ? w.r_chosen[lb] : side == ANY_ARITH ? (w.a_chosen[lb] | R4X16_CODEC_ARITH) : -1;
    if (w.route) {
        atomicAdd(&w.route[side == ANY_RANS ? R4X16_BEST_ANY_RANS : side == ANY_ARITH ? R4X16_BEST_ANY_ARITH : R4X16_BEST_ANY_FAILED], 1u);
        if (tie) atomicAdd(&w.route[R4X16_BEST_ANY_TIE], 1u);
        if (lb == 0) atomicAdd(&w.route[R4X16_BEST_ANY_CHUNKS], 1u);
    }
}

// block i's winner from its codec's slot to out + off[i], and the capacity rule (k_pk_gather / k_ab_gather over both arenas)
__global__ __launch_bounds__(256) void k_any_gather(PackedOut pk, const u8 *side, const u8 *r_slots, const u64 *r_slot_off, AbWs aw, int ka,
                                                    u32 *out_size, i32 *status, int base)
{
    const u32 tid = threadIdx.x;
    const int lb = (int)blockIdx.x, i = base + lb;
    const u32 sz = out_size[i];
    if (sz == 0) return;
    if (pk.off[i + 1] > pk.capacity) {
        if (tid == 0) { status[i] = ST_CAPACITY; out_size[i] = 0; }
        return;
    }
    const u8 *src = side[lb] == ANY_ARITH ? aw.slots + aw.slot_off[(size_t)lb * ka + aw.win[lb]] : r_slots + r_slot_off[lb];
    group_copy<256>(pk.out + pk.off[i], src, sz, tid);
}

// ---- decode ----------------------------------------------------------------------------------------------------------
struct AnyDecWs { u32 *claim, *in_r, *in_a, *sz_r, *sz_a; i32 *pre, *st_r, *st_a; };       // [n] each, in the packed arena

static __device__ __forceinline__ int any_side(i32 method)
{
    const int tag = method & R4X16_CODEC_MASK;
    return method < 0 ? ANY_NONE : tag == R4X16_CODEC_RANS4X16 ? ANY_RANS : tag == R4X16_CODEC_ARITH ? ANY_ARITH : -1;
}

// what block i asks for (k_unpk_claim under a method array): its stored size, or the caller's for an X_NOSZ stream; 0 and a
// status where it may not run
__global__ __launch_bounds__(256) void k_any_claim(const u8 *in, const u64 *in_off, const u32 *in_size, const i32 *method,
                                                   const u32 *nosz_size, AnyDecWs w, int n, u32 max_in, u32 max_out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const int side = any_side(method[i]);
    i32 st, f = -1;
    u32 claim = 0;
    if (side == ANY_NONE) st = ST_EMPTY;                                              // never written
    else if (side < 0) st = ST_UNSUPPORTED;                                           // a codec that is no candidate here
    else {
        st = peek_one(in + in_off[i], in_size[i], max_in, &f, &claim);
        if (st == ST_OK && !(f & X_STRIPE) && (f & X_NOSZ)) {                         // the stream carries no size: the caller's
            if (nosz_size) claim = nosz_size[i]; else st = ST_SIZE;
        }
        if (st == ST_OK && claim > max_out) st = ST_UNSUPPORTED;                      // hostile, or larger than announced
    }
    w.claim[i] = st == ST_OK ? claim : 0u;
    w.pre[i] = st;
}

// after the scan: a block whose range ends beyond the capacity is withdrawn too; a decoder sees an empty input for every
// block that is withdrawn or the other codec's, so that nothing of them is read or written
__global__ __launch_bounds__(256) void k_any_admit(const u32 *in_size, const i32 *method, AnyDecWs w, PackedOut pk, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 st = w.pre[i];
    if (st == ST_OK && pk.off[i + 1] > pk.capacity) { st = ST_CAPACITY; w.pre[i] = st; }
    const int side = any_side(method[i]);
    w.in_r[i] = st == ST_OK && side == ANY_RANS ? in_size[i] : 0u;
    w.in_a[i] = st == ST_OK && side == ANY_ARITH ? in_size[i] : 0u;
}

__global__ __launch_bounds__(256) void k_any_verdict(const i32 *method, AnyDecWs w, u32 *out_size, i32 *status, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 st = w.pre[i];
    u32 sz = 0;
    if (st == ST_OK) {
        const bool arith = any_side(method[i]) == ANY_ARITH;
        st = arith ? w.st_a[i] : w.st_r[i];
        sz = arith ? w.sz_a[i] : w.sz_r[i];
    }
    status[i] = st;
    out_size[i] = st == ST_OK ? sz : 0u;
}

// ---- host --------------------------------------------------------------------------------------------------------------
// The list split by codec (each sub-list in list order, tags off), the arith side's plan and the rANS slots' stride.
struct AnyPlan {
    AnyMethods pm;
    int kr, ka, rm[ANY_MAX_K], am[ANY_MAX_K];
    AbPlan ab;
    u64 stride, total;
    size_t chunk;
};
struct AnyLayout { AnyWs w; PackedSlots ps; AbWs aw; };

// the methods alone: what a call refuses before it asks for the device
static int any_methods(rans4x16_hip_ctx *c, const char *who, int k, const int *methods, AnyPlan *p)
{
    *p = AnyPlan{};
    if (k < 1 || k > ANY_MAX_K || !methods) { c->err = std::string(who) + ": bad arguments"; return -1; }
    p->pm.k = k;
    for (int j = 0; j < k; j++) {
        const int m = methods[j], tag = m & R4X16_CODEC_MASK, word = m & ~R4X16_CODEC_MASK;
        if (m < 0 || (m >> 28) || (tag != R4X16_CODEC_RANS4X16 && tag != R4X16_CODEC_ARITH)) { c->err = std::string(who) + ": unknown codec tag"; return -1; }
        // the order word is bits 0..15: the flags and, for a stripe method, up to 255 planes (:1158; arith_dynamic.c:648)
        if (word >> 16) { c->err = std::string(who) + ((word & X_STRIPE) ? ": more than 255 stripes" : ": an order word above 16 bits"); return -1; }
        p->pm.m[j] = m;
        if (tag == R4X16_CODEC_ARITH) p->am[p->ka++] = word; else p->rm[p->kr++] = word;
    }
    return p->ka ? r4x16_ab_methods(c, who, p->ka, p->am, &p->ab) : 0;
}

static u64 any_chunk_total(const AnyPlan &p, size_t nb, u32 max_in) { return std::min<u64>(p.total, (u64)nb * max_in); }

// the packed arena of a chunk of nb blocks: this call's arrays, the rANS slots, the arith candidates' slots
static size_t any_carve(AnyLayout *L, u8 *base, const AnyPlan &p, size_t nb, u32 max_in)
{
    Carver cv(base);
    AnyWs &w = L->w;
    w.r_size = cv.take<u32>(nb); w.a_size = cv.take<u32>(nb);
    w.r_status = cv.take<i32>(nb); w.a_status = cv.take<i32>(nb); w.r_chosen = cv.take<i32>(nb); w.a_chosen = cv.take<i32>(nb);
    w.side = cv.take<u8>(nb);
    w.route = cv.take<u32>(R4X16_BEST_ANY_KINDS);
    size_t at = cv.total();
    if (p.kr) at += r4x16_packed_carve(&L->ps, base ? base + at : nullptr, nb, nb, p.stride);
    if (p.ka) at += r4x16_ab_carve(&L->aw, base ? base + at : nullptr, p.ab, nb, max_in);
    return at;
}
// what the codecs' own calls take for such a chunk beside it
static size_t any_rans_bytes(const AnyPlan &p, size_t nb, u32 max_in)
{
    return p.kr ? r4x16_best_chunk_bytes(p.kr, p.rm, nb, max_in, any_chunk_total(p, nb, max_in)) : 0;
}
static size_t any_arith_bytes(const AnyPlan &p, size_t nb, u32 max_in) { return p.ka ? r4x16_ab_inner_bytes(p.ab, nb, max_in) : 0; }

// the rest of the plan, on the context's device: both arenas and both workspaces of a chunk fit the room together
static void any_fit(rans4x16_hip_ctx *c, int n, uint32_t max_in_size, uint64_t total_in_size, AnyPlan *p)
{
    p->total = total_in_size ? total_in_size : (u64)n * max_in_size;
    p->stride = 0;
    for (int j = 0; j < p->kr; j++) p->stride = std::max(p->stride, r4x16_packed_stride(max_in_size, p->rm[j], false));
    if (p->ka) r4x16_ab_sizes(n, max_in_size, total_in_size, &p->ab);
    p->chunk = 0;
    if (n == 0) return;
    AnyLayout L = {};
    auto bytes = [&](size_t nb) {
        return any_carve(&L, nullptr, *p, nb, max_in_size) + any_rans_bytes(*p, nb, max_in_size) + any_arith_bytes(*p, nb, max_in_size);
    };
    // (the arith candidates of a chunk are counted in an int; the rANS call cuts a chunk further where its items ask for it)
    const size_t limit = p->ka ? (size_t)INT_MAX / (p->ab.per * p->ka) : SIZE_MAX;
    p->chunk = r4x16_fit_chunk((size_t)n, limit, r4x16_room(c, A_BIT(A_PS) | A_BIT(A_XS) | A_BIT(A_WS) | A_BIT(A_AR)), bytes);
}

extern "C" int rans4x16_hip_best_any_chunk_blocks(rans4x16_hip_ctx *c, int n, int k, const int *methods, uint32_t max_in_size,
                                                  uint64_t total_in_size)
{
    if (!c) return -1;
    AnyPlan p;
    if (any_methods(c, "best_any_chunk_blocks", k, methods, &p) != 0) return -1;
    if (n < 0) { c->err = "best_any_chunk_blocks: bad arguments"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    any_fit(c, n, max_in_size, total_in_size, &p);
    return (int)p.chunk;
}

extern "C" int rans4x16_hip_compress_best_any_packed_dev(rans4x16_hip_ctx *c, int n,
                                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                         unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                         uint32_t *d_out_size, int32_t *d_status,
                                                         int k, const int *methods, int32_t *d_chosen,
                                                         uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    if (!c) return -1;
    hipStream_t s = (hipStream_t)stream;
    AnyPlan p;
    if (any_methods(c, "compress_best_any_packed_dev", k, methods, &p) != 0) return -1;
    BatchArgs a;                                   // (filled, not read: the codecs' calls take this call's own slots)
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "compress_best_any_packed_dev: bad arguments", true, &a, &pk, n, d_in, d_in_off, d_in_size, d_out,
                                          out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    any_fit(c, n, max_in_size, total_in_size, &p);
    AnyLayout L = {};
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_PS, any_carve(&L, nullptr, p, nb, max_in_size), false); };
    return r4x16_chunk_walk(c, n, p.chunk, s, grab, [&](size_t base, int nb) {
        const size_t arena = any_carve(&L, c->at(A_PS), p, (size_t)nb, max_in_size);
        const size_t r_bytes = any_rans_bytes(p, (size_t)nb, max_in_size), a_bytes = any_arith_bytes(p, (size_t)nb, max_in_size);
        AnyWs w = L.w;
        u32 *const d_route = w.route;
        if (r4x16_route_begin(c, &w.route, R4X16_BEST_ANY_KINDS, s) != 0) return -1;
        if (p.kr) {
            r4x16_launch_packed_slots_best(d_in_size + base, p.kr, p.rm, &L.ps, nb, (size_t)nb, max_in_size, s);
            // the rANS call: what is left of the ceiling beside this call's arena and the arith call's
            const size_t held = arena + a_bytes;
            Keep<size_t> ceiling(c->max_ws, c->max_ws > held + ((size_t)1 << 20) ? c->max_ws - held : (size_t)1 << 20);
            Keep<bool> inner(c->in_packed, true);
            const u64 total = total_in_size ? any_chunk_total(p, (size_t)nb, max_in_size) : 0;
            if (rans4x16_hip_compress_best_dev(c, nb, d_in, d_in_off + base, d_in_size + base, L.ps.slots, L.ps.slot_off, L.ps.slot_cap,
                                               w.r_size, w.r_status, p.kr, p.rm, w.r_chosen, max_in_size, total, s) != 0)
                return -1;
        }
        if (p.ka && r4x16_ab_candidates(c, p.ab, L.aw, arena + r_bytes, base, nb, d_in, d_in_off, d_in_size, w.a_size, w.a_status, w.a_chosen,
                                        max_in_size, s) != 0)
            return -1;
        hipLaunchKernelGGL(k_any_pick, dim3((u32)(nb + 255) / 256), dim3(256), 0, s, p.pm, w, (const u32 *)L.ps.slot_cap, p.kr, p.ka, d_out_size,
                           d_status, d_chosen, (int)base, nb);
        r4x16_launch_packed_scan(d_out_size, d_out_off, (int)base, nb, s);
        hipLaunchKernelGGL(k_any_gather, dim3((u32)nb), dim3(256), 0, s, pk, (const u8 *)w.side, (const u8 *)L.ps.slots,
                           (const u64 *)L.ps.slot_off, L.aw, p.ka, d_out_size, d_status, (int)base);
        if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_RESULT][R4X16_RESULT_GATHERED] += nb;
        return r4x16_route_end(c, R4X16_ROUTE_BEST_ANY, d_route, R4X16_BEST_ANY_KINDS, s);
    });
}

extern "C" int rans4x16_hip_uncompress_any_packed_dev(rans4x16_hip_ctx *c, int n,
                                                      const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                      const int32_t *d_method,
                                                      unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                      uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                                      uint32_t max_in_size, uint32_t max_out_size, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    const int go = r4x16_packed_call_args(c, "uncompress_any_packed_dev: bad arguments", n == 0 || d_method, &a, &pk, n, d_in, d_in_off, d_in_size,
                                          d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    // the layout's own arrays: 32 bytes per block in the packed arena (ordered between streams like the workspace)
    if (r4x16_ensure(c, A_PS, 8 * align_up((size_t)n * 4, 256), false) != 0) return -1;
    Carver cv(c->at(A_PS));
    AnyDecWs w;
    w.claim = cv.take<u32>(n); w.in_r = cv.take<u32>(n); w.in_a = cv.take<u32>(n); w.sz_r = cv.take<u32>(n); w.sz_a = cv.take<u32>(n);
    w.pre = cv.take<i32>(n); w.st_r = cv.take<i32>(n); w.st_a = cv.take<i32>(n);
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const dim3 grid((n + 255) / 256), wg(256);
    hipLaunchKernelGGL(k_any_claim, grid, wg, 0, s, d_in, d_in_off, d_in_size, d_method, d_nosz_size, w, n, max_in_size, max_out_size);
    r4x16_launch_packed_scan(w.claim, pk.off, 0, n, s);
    hipLaunchKernelGGL(k_any_admit, grid, wg, 0, s, d_in_size, d_method, w, pk, n);
    // every admitted block ends inside the capacity, so the capacities of either decoder's blocks together do too
    const u64 total = std::max<u64>(std::min<u64>(pk.capacity, (u64)n * max_out_size), 1);
    // the sizing pass (no arena, capacity 0): only blocks that claim 0 bytes are admitted and nothing is written, but the
    // slot calls want a pointer - the packed arena's own
    unsigned char *out = pk.out ? pk.out : c->at(A_PS);
    if (rans4x16_hip_uncompress_dev_sized(c, n, d_in, d_in_off, w.in_r, out, pk.off, w.claim, w.sz_r, w.st_r, max_in_size, max_out_size, total, s) != 0)
        return -1;
    if (rans4x16_hip_arith_uncompress_dev(c, n, d_in, d_in_off, w.in_a, out, pk.off, w.claim, w.sz_a, w.st_a, max_in_size, max_out_size, total, s) != 0)
        return -1;
    hipLaunchKernelGGL(k_any_verdict, grid, wg, 0, s, d_method, w, d_out_size, d_status, n);
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}

// ---- host buffers ------------------------------------------------------------------------------------------------------
// Both calls walk the batch in ranges of blocks whose inputs and outputs together stay under ANY_HOST_CHUNK_BYTES of
// staging (r4x16_cut_ranges): the staging layout with one item more than blocks (the offsets' n + 1 entries lie in its
// out_off array, the methods in its order array), the arrays' upload, the packed device call on the staged arenas, the
// verdict read, then the offsets, the methods and the dense results in one download each.  Like r4x16_host_trip the copies
// go from and to pageable memory and are not pipelined; every range ends in a synchronise before its vectors go.
#define ANY_HOST_CHUNK_BYTES ((size_t)256 << 20)

// one range of rans4x16_hip_compress_best_any_batch: blocks [at, at + nb).  made: the buffers this call allocated.  0 or -1.
static int any_host_compress(rans4x16_hip_ctx *c, const AnyPlan &p, int at, int nb, const unsigned char *const *in, const unsigned int *in_size,
                             unsigned char **out, unsigned int *out_size, int k, const int *methods, int *chosen, int *status,
                             const std::vector<u32> &bound, std::vector<int> *made, int *failed)
{
    hipStream_t s = c->stream;
    std::vector<u64> in_off(nb + 1, 0), off(nb + 1, 0);
    std::vector<u32> isz(nb + 1, 0), cap(nb + 1, 0), osz(nb + 1);
    std::vector<i32> ord(nb + 1, 0), st(nb + 1), won(nb + 1);
    size_t out_total = 0;
    u32 max_in = 0;
    for (int i = 0; i < nb; i++) { isz[i] = in_size[at + i]; max_in = std::max(max_in, isz[i]); out_total += bound[at + i]; }
    const size_t in_total = r4x16_stage_slots(isz.data(), (size_t)nb, 16, 256, in_off.data());
    StageLayout L;
    if (r4x16_stage_begin(c, &L, (size_t)nb + 1, in_total + 256, 0, out_total + 256, 0, {in_off.data(), off.data(), isz.data(), cap.data(), ord.data()}, s) != 0)
        return -1;
    std::vector<u8> up(in_total + 1);
    for (int i = 0; i < nb; i++) if (isz[i]) memcpy(up.data() + in_off[i], in[at + i], isz[i]);
    if (in_total) HIPCHK(c, hipMemcpyAsync(L.in, up.data(), in_total, hipMemcpyHostToDevice, s));
    if (rans4x16_hip_compress_best_any_packed_dev(c, nb, L.in, L.in_off, L.in_size, L.out, out_total, L.out_off, L.osz, L.status, k, methods,
                                                  L.order, max_in, in_total, s) != 0) {
        (void)hipStreamSynchronize(s);                 // (the upload reads `up`)
        return -1;
    }
    HIPCHK(c, hipMemcpyAsync(off.data(), L.out_off, ((size_t)nb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(won.data(), L.order, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    if (r4x16_stage_verdicts(c, L, (size_t)nb, osz.data(), st.data(), s) != 0) return -1;
    std::vector<u8> down((size_t)off[nb] + 1);
    if (off[nb]) HIPCHK(c, hipMemcpy(down.data(), L.out, (size_t)off[nb], hipMemcpyDeviceToHost));
    for (int i = 0; i < nb; i++) {
        const int g = at + i;
        status[g] = st[i];
        if (chosen) chosen[g] = won[i];
        if (st[i] == 0 && out[g] && out_size[g] < osz[i]) status[g] = R4X16_E_CAPACITY;              // the caller's buffer is too short
        if (status[g] == 0 && !out[g]) {
            if ((out[g] = (unsigned char *)malloc(osz[i] ? osz[i] : 1))) made->push_back(g); else status[g] = R4X16_E_UNSUPPORTED;
        }
        if (status[g] != 0) { out_size[g] = 0; ++*failed; continue; }
        memcpy(out[g], down.data() + off[i], osz[i]);
        out_size[g] = osz[i];
    }
    return 0;
}

extern "C" int rans4x16_hip_compress_best_any_batch(rans4x16_hip_ctx *c, int n,
                                                    const unsigned char *const *in, const unsigned int *in_size,
                                                    unsigned char **out, unsigned int *out_size,
                                                    int k, const int *methods, int *chosen, int *status)
{
    if (!c) return -1;
    AnyPlan p;
    if (any_methods(c, "compress_best_any_batch", k, methods, &p) != 0) return -1;
    if (n < 0 || (n && (!in || !in_size || !out || !out_size || !status))) { c->err = "compress_best_any_batch: bad arguments"; return -1; }
    if (n == 0) return 0;
    for (int i = 0; i < n; i++) if (!in[i] && in_size[i]) { c->err = "compress_best_any_batch: bad arguments"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    // the room a block's winner may take: the largest bound over the list
    std::vector<u32> bound(n, 0);
    std::vector<size_t> foot(n), ends(n);
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < p.kr; j++) bound[i] = std::max(bound[i], r4x16_compress_bound(in_size[i], p.rm[j]));
        for (int j = 0; j < p.ka; j++) bound[i] = std::max(bound[i], rans4x16_hip_arith_compress_cap(in_size[i], p.am[j]));
        foot[i] = (size_t)in_size[i] + bound[i] + 512;
    }
    const size_t ranges = r4x16_cut_ranges(foot.data(), (size_t)n, ANY_HOST_CHUNK_BYTES, 0, ends.data());
    std::vector<int> made;
    int failed = 0;
    for (size_t r = 0, at = 0; r < ranges; at = ends[r++])
        if (any_host_compress(c, p, (int)at, (int)(ends[r] - at), in, in_size, out, out_size, k, methods, chosen, status, bound, &made, &failed) != 0) {
            // the call failed: what it allocated for earlier ranges is not left with the caller
            for (int g : made) { free(out[g]); out[g] = nullptr; out_size[g] = 0; }
            return -1;
        }
    return failed;
}

// The size a stream stores, read as k_any_claim reads it (peek_one's varint): false where the stream has none of its own
// (empty, X_NOSZ without X_STRIPE) or the field is cut off - the device says what such a block is.
static bool any_host_claim(const unsigned char *b, u32 size, u32 *claim)
{
    if (size == 0 || (!(b[0] & X_STRIPE) && (b[0] & X_NOSZ))) return false;
    u32 acc = 0, q = 1;
    unsigned char ch = 0;
    if (q >= size) return false;
    do { ch = b[q++]; acc = (acc << 7) | (ch & 0x7f); } while ((ch & 0x80) && q < size);
    if (ch & 0x80) return false;
    *claim = acc;
    return true;
}

// one range of rans4x16_hip_uncompress_any_batch
static int any_host_uncompress(rans4x16_hip_ctx *c, int at, int nb, const unsigned char *const *in, const unsigned int *in_size, const int *method,
                               unsigned char *const *out, unsigned int *out_size, int *status, int *failed)
{
    hipStream_t s = c->stream;
    std::vector<u64> in_off(nb + 1, 0), off(nb + 1, 0);
    std::vector<u32> isz(nb + 1, 0), cap(nb + 1, 0), osz(nb + 1);
    std::vector<i32> ord(nb + 1, 0), st(nb + 1);
    std::vector<u8> short_of(nb, 0);
    size_t out_total = 0;
    u32 max_in = 0, max_out = 0, planes = 0, stripe_out = 0;
    for (int i = 0; i < nb; i++) {
        const unsigned char *b = in[at + i];
        isz[i] = in_size[at + i]; cap[i] = out_size[at + i]; ord[i] = method[at + i];
        // A block fails alone, as in rans4x16_hip_uncompress_batch where it has a slot of its own: the dense arena is laid out
        // by the sizes the streams claim, so a stream that stores more than its caller's buffer holds is withdrawn here - the
        // device sees a block that was never written - and every block that runs ends inside the sum of the capacities.
        u32 claim = 0;
        if (ord[i] >= 0 && any_host_claim(b, isz[i], &claim) && claim > cap[i]) { short_of[i] = 1; ord[i] = -1; isz[i] = 0; continue; }
        max_in = std::max(max_in, isz[i]); max_out = std::max(max_out, cap[i]); out_total += cap[i];
        // an X_STRIPE stream of either codec: flags, the size's varint, N
        if (isz[i] < 3 || !(b[0] & X_STRIPE)) continue;
        u32 q = 1;
        while (q + 1 < isz[i] && (b[q] & 0x80)) q++;
        if (q + 1 >= isz[i]) continue;                                            // truncated: the decoder says so
        planes = std::max<u32>(planes, b[q + 1]);
        stripe_out = std::max(stripe_out, cap[i]);
    }
    const size_t in_total = r4x16_stage_slots(isz.data(), (size_t)nb, 16, 256, in_off.data());
    StageLayout L;
    if (r4x16_stage_begin(c, &L, (size_t)nb + 1, in_total + 256, 0, out_total + 256, 0, {in_off.data(), off.data(), isz.data(), cap.data(), ord.data()}, s) != 0)
        return -1;
    std::vector<u8> up(in_total + 1);
    for (int i = 0; i < nb; i++) if (isz[i]) memcpy(up.data() + in_off[i], in[at + i], isz[i]);
    if (in_total) HIPCHK(c, hipMemcpyAsync(L.in, up.data(), in_total, hipMemcpyHostToDevice, s));
    // X_STRIPE blocks as after rans4x16_hip_set_dev_stripe_planes(ctx, most planes of the range, largest such block); the
    // caller's setting is put back
    StripeLimits stripes(c, (int)planes, stripe_out);
    // L.cap: the callers' capacities, what an X_NOSZ stream decodes to
    if (rans4x16_hip_uncompress_any_packed_dev(c, nb, L.in, L.in_off, L.in_size, L.order, L.out, out_total, L.out_off, L.osz, L.status, L.cap,
                                               max_in, max_out, s) != 0) {
        (void)hipStreamSynchronize(s);                 // (the upload reads `up`)
        return -1;
    }
    HIPCHK(c, hipMemcpyAsync(off.data(), L.out_off, ((size_t)nb + 1) * 8, hipMemcpyDeviceToHost, s));
    if (r4x16_stage_verdicts(c, L, (size_t)nb, osz.data(), st.data(), s) != 0) return -1;
    const size_t got = (size_t)std::min<u64>(off[nb], out_total);
    std::vector<u8> down(got + 1);
    if (got) HIPCHK(c, hipMemcpy(down.data(), L.out, got, hipMemcpyDeviceToHost));
    for (int i = 0; i < nb; i++) {
        const int g = at + i;
        status[g] = short_of[i] ? R4X16_E_CAPACITY : st[i];                       // the stream stores more than the caller has room for
        if (status[g] == 0 && out_size[g] < osz[i]) status[g] = R4X16_E_CAPACITY; // (an admitted block claims no more than its capacity)
        if (status[g] != 0) { out_size[g] = 0; ++*failed; continue; }
        if (osz[i]) memcpy(out[g], down.data() + off[i], osz[i]);
        out_size[g] = osz[i];
    }
    return 0;
}

extern "C" int rans4x16_hip_uncompress_any_batch(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *const *in, const unsigned int *in_size, const int *method,
                                                 unsigned char *const *out, unsigned int *out_size, int *status)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !method || !out || !out_size || !status))) { c->err = "uncompress_any_batch: bad arguments"; return -1; }
    if (n == 0) return 0;
    for (int i = 0; i < n; i++) if ((!in[i] && in_size[i]) || (!out[i] && out_size[i])) { c->err = "uncompress_any_batch: bad arguments"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<size_t> foot(n), ends(n);
    for (int i = 0; i < n; i++) foot[i] = (size_t)in_size[i] + out_size[i] + 512;
    const size_t ranges = r4x16_cut_ranges(foot.data(), (size_t)n, ANY_HOST_CHUNK_BYTES, 0, ends.data());
    int failed = 0;
    for (size_t r = 0, at = 0; r < ranges; at = ends[r++])
        if (any_host_uncompress(c, (int)at, (int)(ends[r] - at), in, in_size, method, out, out_size, status, &failed) != 0) return -1;
    return failed;
}
