// r4x16_tok3.hip - the tok3 column container on the device (include/rans4x16_hip.h part 2c): what encode_names
// (htscodecs tokenise_name3.c:1431-1531) does with a name block's token columns once they are filled, and what
// decode_names (:1546-1669) does before it reads them (the names themselves: r4x16_tok3_names.hip).
//
// Pack.   rans4x16_hip_compress_best_packed_dev over all columns of the batch leaves the winners back to back in an
//         arena of the context (`t3`); then
//           k_t3_hash  : one wave per column, a 64-bit hash of the winner's bytes
//           k_t3_dup   : one wave per block - the block's verdict, per column the first earlier column with the same
//                        (length, hash) and, on such a hit only, the same bytes (:1461-1477), the column's place in the
//                        block and the block's size
//           k_pk_scan  : block sizes -> offsets (r4x16_packed.hip)
//           k_t3_frame : header, type bytes, varints, and every stream copied to its final place - one move more than
//                        the best-of-k call makes.
// Unpack. k_t3_walk    : one wave per container, one lane walks it (r4x16_tok3_walk.h, the text the host scan runs too)
//                        and writes a fixed-stride directory of max_columns entries per block: id, kind, claimed size
//           k_pk_scan  : the claims of all nblk x max_columns entries -> where every column goes
//           k_t3_admit : blocks refused by the walk or ending beyond the capacity are withdrawn; the plain columns of
//                        the others become the items of one rans4x16_hip_uncompress_dev_sized call, capacity = claim
//           k_t3_fill  : duplicate columns copied from the decoded original, type columns synthesised, 16 bytes a piece
//           k_t3_verdict: per block the first failing column's status, sizes, the caller's directory.
//         After rans4x16_hip_set_tok3_arith(ctx, R4X16_TOK3_ARITH_DECODE) the walk admits containers with use_arith set
//         and notes each block's flavour; k_t3_admit then fills two masked item lists over the same entries - an entry
//         has its length and capacity in its own flavour's list and 0 in the other (the arith list's length reaches to the
//         container's end, see k_t3_admit) - and rans4x16_hip_arith_uncompress_dev
//         runs over the second with statuses and sizes of its own, so that neither decoder touches what the other reports.
//         Pack writes use_arith = 1 and takes its winners from rans4x16_hip_arith_compress_best_packed_dev after
//         R4X16_TOK3_ARITH_ENCODE; hash, duplicates, scan and frame do not look at the streams' flavour.
//
// Loops: trip counts are launch arguments (nblk, n, max_columns) or sizes checked first - a column's stream is at most
// the bound of max_col_size (the inner call's guarantee), a block has at most T3_MAX_IDS columns (more cannot have
// ascending ids and are refused before any loop over them), a claimed size is checked against max_col_size by the walk.
#include "r4x16_host.h"
#include "r4x16_tok3_walk.h"

typedef u64 u64_unaligned __attribute__((aligned(1)));
#define T3_KIND_NONE 3u

// ---- unpack --------------------------------------------------------------------------------------------------
// [nblk * max_columns] each (off: one more), entry b * max_columns + d is descriptor d of block b; pre: [nblk].
// An entry claims lead + size bytes at off: the type column synthesised in front of it, then its own column at col_off.
struct T3Items {
    u64 *in_off; u32 *clen, *in_size, *claim, *size, *lead, *cap, *kind_a; u64 *off, *col_off; u32 *out_size; i32 *status; i32 *pre;
    // the arith flavour's masked list and results ([nitems]) and the blocks' flavours ([nblk]); nullptr: arith is not admitted
    u32 *in_size_a, *cap_a, *out_size_a; i32 *status_a; u8 *arith;
};

static size_t t3_items_carve(T3Items *w, u8 *base, size_t nitems, size_t nblk, bool arith)
{
    Carver cv(base);
    w->in_off = cv.take<u64>(nitems); w->clen = cv.take<u32>(nitems); w->in_size = cv.take<u32>(nitems);
    w->claim = cv.take<u32>(nitems); w->size = cv.take<u32>(nitems); w->lead = cv.take<u32>(nitems);
    w->cap = cv.take<u32>(nitems); w->kind_a = cv.take<u32>(nitems);
    w->off = cv.take<u64>(nitems + 1); w->col_off = cv.take<u64>(nitems); w->out_size = cv.take<u32>(nitems); w->status = cv.take<i32>(nitems);
    w->pre = cv.take<i32>(nblk);
    w->in_size_a = w->cap_a = w->out_size_a = nullptr; w->status_a = nullptr; w->arith = nullptr;
    if (arith) {
        w->in_size_a = cv.take<u32>(nitems); w->cap_a = cv.take<u32>(nitems); w->out_size_a = cv.take<u32>(nitems);
        w->status_a = cv.take<i32>(nitems); w->arith = cv.take<u8>(nblk);
    }
    return cv.total();
}

struct DevDir {
    T3Items w; i32 *id; u64 cbase; size_t base;
    __device__ void put(u32 c, int cid, int kind, u32 a, u32 b, u32 size, u32 lead)
    {
        const size_t i = base + c;
        id[i] = cid | (lead ? R4X16_TOK3_TYPE_COLUMN : 0);
        w.kind_a[i] = ((u32)kind << 16) | (kind == T3_PLAIN ? 0u : (a & 0xffffu));
        w.in_off[i] = cbase + (kind == T3_PLAIN ? a : 0u);
        w.clen[i] = kind == T3_PLAIN ? b : 0u;
        w.size[i] = size;
        w.lead[i] = lead;
        w.claim[i] = lead + size;              // (a sum beyond 32 bits fails the block: the walk's total)
    }
    __device__ int id_at(u32 c) const { return id[base + c] & (T3_MAX_IDS - 1); }
    __device__ int kind_at(u32 c) const { return (int)(w.kind_a[base + c] >> 16); }
    __device__ u32 a_at(u32 c) const { return w.kind_a[base + c] & 0xffffu; }
    __device__ u32 size_at(u32 c) const { return w.size[base + c]; }
};

__global__ __launch_bounds__(64) void k_t3_walk(const u8 *in, const u64 *in_off, const u32 *in_size, T3Items w, i32 *dir_id,
                                                u32 *ncol, u32 *last_start, u32 *nreads, u32 maxc, u32 max_in, u32 max_col)
{
    __shared__ u16 map[T3_MAX_IDS];
    __shared__ u32 wrote;
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)b * maxc;
    for (u32 i = lane; i < T3_MAX_IDS; i += 64) map[i] = T3_NONE;
    __syncthreads();
    if (lane == 0) {
        T3Sum sum = {};
        int st = T3_E_UNSUPPORTED;                                        // larger than the call was sized for: not read
        const u32 size = in_size[b];
        if (size <= max_in) {
            ByteSrc src(in + in_off[b]);
            DevDir dir = {w, dir_id, in_off[b], base};
            st = t3_walk(src, size, maxc, max_col, w.arith != nullptr, map, dir, &sum);
        }
        if (w.arith) w.arith[b] = (u8)sum.arith;
        w.pre[b] = st;
        ncol[b] = st == T3_OK ? sum.ndesc : 0u;
        last_start[b] = sum.last_start;
        nreads[b] = sum.nreads;
        if (st != T3_OK)                                                  // the block fails as a whole: it claims nothing
            for (u32 c = 0; c <= sum.ndesc && c < maxc; c++) { w.claim[base + c] = 0; w.size[base + c] = 0; w.lead[base + c] = 0; w.clen[base + c] = 0; w.kind_a[base + c] = T3_KIND_NONE << 16; dir_id[base + c] = -1; }
        wrote = st == T3_OK ? sum.ndesc : (sum.ndesc + 1 < maxc ? sum.ndesc + 1 : maxc);     // (the refused descriptor may have been put)
    }
    __syncthreads();
    for (u32 c = wrote + lane; c < maxc; c += 64) {
        const size_t i = base + c;
        w.claim[i] = 0; w.size[i] = 0; w.lead[i] = 0; w.clen[i] = 0; w.kind_a[i] = T3_KIND_NONE << 16; w.in_off[i] = 0; dir_id[i] = -1;
    }
}

__device__ __forceinline__ bool t3_admitted(const T3Items &w, size_t b, u32 maxc, u64 capacity)
{
    return w.pre[b] == ST_OK && w.off[(b + 1) * maxc] <= capacity;
}

// blk_off / blk_size: the containers, for the arith flavour's input length (below)
__global__ __launch_bounds__(256) void k_t3_admit(T3Items w, const u64 *blk_off, const u32 *blk_size, u64 *out_off, u64 capacity, u32 nblk,
                                                  u32 maxc, u64 nitems)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nitems) return;
    const size_t b = (size_t)(i / maxc);
    const bool run = t3_admitted(w, b, maxc, capacity) && (w.kind_a[i] >> 16) == T3_PLAIN;
    const bool ar = w.arith && w.arith[b];
    w.in_size[i] = run && !ar ? w.clen[i] : 0u;
    w.cap[i] = run && !ar ? w.size[i] : 0u;
    if (w.arith) {
        // The arith decoder is handed the rest of the container, as the reference hands it (tokenise_name3.c:1214), not
        // the clen bytes of the stream: c_range_coder.h:64 starts to decode only if more than five bytes lie in front of
        // in_end, and the reference's own writer gives a near-constant column a body of exactly five.  Such a column
        // decodes because another descriptor follows it (and to zeros where none does, here as there).
        w.in_size_a[i] = run && ar ? (u32)(blk_off[b] + blk_size[b] - w.in_off[i]) : 0u;
        w.cap_a[i] = run && ar ? w.size[i] : 0u;
    }
    w.col_off[i] = w.off[i] + w.lead[i];
    if (i == (u64)b * maxc) {
        out_off[b] = w.off[i];
        if (b == nblk - 1) out_off[nblk] = w.off[nitems];
    }
}

// `n` bytes of a type column at dst: the type, then N_MATCH (:1589-1590), by one wave
__device__ __forceinline__ void t3_type_column(u8 *dst, u32 n, u8 type, u32 lane)
{
    u32 head = (u32)((16 - ((u64)dst & 15)) & 15);
    if (head > n) head = n;
    for (u32 j = lane; j < head; j += 64) dst[j] = j ? (u8)T3_N_MATCH : type;
    const u32 body = (n - head) >> 4;
    const u32 tens = 0x01010101u * T3_N_MATCH;
    u32x4 *d16 = (u32x4 *)(dst + head);
    for (u32 j = lane; j < body; j += 64) {
        u32x4 v = {tens, tens, tens, tens};
        if (head == 0 && j == 0) v.x = (tens & 0xffffff00u) | type;
        d16[j] = v;
    }
    for (u32 j = head + body * 16 + lane; j < n; j += 64) dst[j] = j ? (u8)T3_N_MATCH : type;
}

// one wave per descriptor: the type column in front of it, and its own column where that is a copy - a duplicate reads
// the decoded original, a copy of a type column is written like one
__global__ __launch_bounds__(256) void k_t3_fill(T3Items w, const i32 *dir_id, u8 *out, u64 capacity, u32 maxc, u64 nitems)
{
    const u64 i = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63u;
    if (i >= nitems) return;
    const u32 ka = w.kind_a[i], kind = ka >> 16, n = w.size[i], lead = w.lead[i];
    if (kind == T3_KIND_NONE || (lead == 0 && (kind == T3_PLAIN || n == 0))) return;
    const size_t b = (size_t)(i / maxc);
    if (!t3_admitted(w, b, maxc, capacity)) return;
    if (lead) t3_type_column(out + w.off[i], lead, (u8)(dir_id[i] & 15), lane);
    if (kind == T3_DUP && n) wave_copy(out + w.col_off[i], out + w.col_off[b * maxc + (ka & 0xffffu)], n, lane);
    else if (kind == T3_SYNTH) t3_type_column(out + w.col_off[i], n, (u8)(ka & 15u), lane);
}

struct T3Out { u32 *out_size; i32 *status; u32 *ncol; u64 *col_off; u32 *col_size; };

__global__ __launch_bounds__(64) void k_t3_verdict(T3Items w, T3Out o, u64 capacity, u32 maxc)
{
    const size_t b = blockIdx.x, base = b * maxc;
    const u32 lane = threadIdx.x;
    i32 st = w.pre[b];
    const u64 start = w.off[base], end = w.off[base + maxc];
    if (st == ST_OK && end > capacity) st = ST_CAPACITY;
    const bool ar = w.arith && w.arith[b];                                // the block's columns were the arith decoder's
    const i32 *cst = ar ? w.status_a : w.status;
    const u32 *csz = ar ? w.out_size_a : w.out_size;
    if (st == ST_OK)
        for (u32 c0 = 0; c0 < maxc; c0 += 64) {                           // the first column that failed to decode
            const u32 c = c0 + lane;
            // (a stream may decode to fewer bytes than its size field says - X_PACK over an empty payload - where the
            //  reference trips its assert, :1655: the column would not be what the directory says)
            const bool bad = c < maxc && (w.kind_a[base + c] >> 16) == T3_PLAIN &&
                             (cst[base + c] != ST_OK || csz[base + c] != w.size[base + c]);
            const u64 m = __ballot(bad);
            if (m) {
                const size_t f = base + c0 + (u32)__builtin_ctzll(m);
                st = cst[f] != ST_OK ? cst[f] : ST_SIZE;
                break;
            }
        }
    for (u32 c = lane; c < maxc; c += 64) {
        o.col_off[base + c] = w.col_off[base + c];
        o.col_size[base + c] = st == ST_OK ? w.size[base + c] : 0u;
    }
    if (lane == 0) {
        o.status[b] = st;
        o.out_size[b] = st == ST_OK ? (u32)(end - start) : 0u;
        if (st != ST_OK) o.ncol[b] = 0;
    }
}

extern "C" int rans4x16_hip_tok3_unpack_dev(rans4x16_hip_ctx *c, int nblk,
                                            const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                            unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                            uint32_t *d_out_size, int32_t *d_status,
                                            uint32_t *d_ncol, uint32_t *d_last_start, uint32_t *d_nreads,
                                            int32_t *d_col_id, uint64_t *d_col_off, uint32_t *d_col_size,
                                            uint32_t max_columns, uint32_t max_in_size, uint32_t max_col_size, void *stream)
{
    if (!c) return -1;
    if (nblk < 0 || !d_out_off || max_columns < 1 || max_columns > T3_MAX_IDS ||
        (nblk && (!d_in || !d_in_off || !d_in_size || (!d_out && out_capacity) || !d_out_size || !d_status || !d_ncol || !d_last_start ||
                  !d_nreads || !d_col_id || !d_col_off || !d_col_size))) {
        c->err = "tok3_unpack_dev: bad arguments";
        return -1;
    }
    const u64 nitems = (u64)nblk * max_columns;
    if (nitems >= (u64)INT_MAX) { c->err = "tok3_unpack_dev: nblk x max_columns does not fit an int"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nblk == 0) { HIPCHK(c, hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s)); return 0; }
    T3Items w;
    const bool arith = (c->tok3_arith & R4X16_TOK3_ARITH_DECODE) != 0;
    if (r4x16_ensure(c, A_T3, t3_items_carve(&w, nullptr, (size_t)nitems, (size_t)nblk, arith), false) != 0) return -1;
    const size_t arena = t3_items_carve(&w, c->at(A_T3), (size_t)nitems, (size_t)nblk, arith);
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const dim3 per_item((u32)((nitems + 255) / 256));
    hipLaunchKernelGGL(k_t3_walk, dim3((u32)nblk), dim3(64), 0, s, d_in, d_in_off, d_in_size, w, d_col_id, d_ncol, d_last_start, d_nreads,
                       max_columns, max_in_size, max_col_size);
    r4x16_launch_packed_scan(w.claim, w.off, 0, (int)nitems, s);
    hipLaunchKernelGGL(k_t3_admit, per_item, dim3(256), 0, s, w, d_in_off, d_in_size, d_out_off, out_capacity, (u32)nblk, max_columns, nitems);
    const u64 total = std::max<u64>(std::min<u64>(out_capacity, nitems * (u64)max_col_size), 1);
    const size_t keep_ws = c->max_ws;
    c->max_ws = keep_ws > arena + ((size_t)1 << 20) ? keep_ws - arena : (size_t)1 << 20;
    // the sizing pass (no arena, capacity 0): only blocks that claim 0 bytes are admitted and nothing is written, but the
    // slot call wants a pointer - the tok3 arena's own
    unsigned char *out = d_out ? d_out : c->at(A_T3);
    int rc = rans4x16_hip_uncompress_dev_sized(c, (int)nitems, d_in, w.in_off, w.in_size, out, w.col_off, w.cap, w.out_size, w.status,
                                               max_in_size, max_col_size, total, s);
    if (rc == 0 && arith)
        rc = rans4x16_hip_arith_uncompress_dev(c, (int)nitems, d_in, w.in_off, w.in_size_a, out, w.col_off, w.cap_a, w.out_size_a, w.status_a,
                                               max_in_size, max_col_size, total, s);
    c->max_ws = keep_ws;
    if (rc != 0) return -1;
    hipLaunchKernelGGL(k_t3_fill, dim3((u32)((nitems + 3) / 4)), dim3(256), 0, s, w, (const i32 *)d_col_id, d_out, out_capacity, max_columns, nitems);
    const T3Out o = {d_out_size, d_status, d_ncol, d_col_off, d_col_size};
    hipLaunchKernelGGL(k_t3_verdict, dim3((u32)nblk), dim3(64), 0, s, w, o, out_capacity, max_columns);
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}

// ---- pack ----------------------------------------------------------------------------------------------------
// per column [n] (s_off: one more): the winners of the best-of-k call in `streams`, and what the framing adds
struct T3Cols {
    u64 *s_off; u32 *s_size; i32 *s_status; u64 *hash; u32 *rel; i32 *dup; u32 *pmax /*[nblk]*/; u8 *streams;
};

static size_t t3_cols_carve(T3Cols *w, u8 *base, size_t n, size_t nblk, u64 stream_bytes)
{
    Carver cv(base);
    w->s_off = cv.take<u64>(n + 1); w->s_size = cv.take<u32>(n); w->s_status = cv.take<i32>(n);
    w->hash = cv.take<u64>(n); w->rel = cv.take<u32>(n); w->dup = cv.take<i32>(n);
    w->pmax = cv.take<u32>(nblk);
    w->streams = cv.take<u8>((size_t)stream_bytes + 256);
    return cv.total();
}

__device__ __forceinline__ u64 t3_mix(u64 x)                              // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ u64 t3_tail_word(const u8 *p, u32 nbytes)     // nbytes < 8
{
    u64 v = 0;
    for (u32 t = 0; t < nbytes; t++) v |= (u64)p[t] << (8 * t);
    return v;
}

// one wave per column: the sum of the mixed 8-byte pieces, each with its position (a sum, so the lanes' order is free)
__global__ __launch_bounds__(256) void k_t3_hash(T3Cols w, int n)
{
    const int i = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    const u32 lane = threadIdx.x & 63u;
    if (i >= n) return;
    const u32 sz = w.s_size[i];
    const u8 *p = w.streams + w.s_off[i];
    const u32 words = sz >> 3;
    u64 h = 0;
    for (u32 k = lane; k < words; k += 64) h += t3_mix(*(const u64_unaligned *)(p + 8ull * k) + 0x9e3779b97f4a7c15ull * (k + 1));
    if (lane == 0) h += t3_mix(t3_tail_word(p + 8ull * words, sz & 7u) + 0x9e3779b97f4a7c15ull * (words + 1)) ^ sz;
    for (int d = 32; d; d >>= 1) h += __shfl_xor(h, d);
    if (lane == 0) w.hash[i] = sz ? h : 0ull;
}

__device__ __forceinline__ bool t3_wave_equal(const u8 *a, const u8 *b, u32 n, u32 lane)
{
    const u32 words = n >> 3;
    bool diff = false;
    for (u32 k = lane; k < words; k += 64) diff |= *(const u64_unaligned *)(a + 8ull * k) != *(const u64_unaligned *)(b + 8ull * k);
    if (lane == 0) diff |= t3_tail_word(a + 8ull * words, n & 7u) != t3_tail_word(b + 8ull * words, n & 7u);
    return __ballot(diff) == 0ull;
}

// pmax[b] = the largest of blk_first[0 .. b]: a block that starts below it shares columns with an earlier block.  One
// workgroup, k_pk_scan's scheme with max for plus.
__global__ __launch_bounds__(1024) void k_t3_first_max(const u32 *blk_first, u32 *pmax, int nblk)
{
    __shared__ u32 part[1024];
    __shared__ u32 carry;
    const u32 t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int at = 0; at < nblk; at += 1024) {
        const int b = at + (int)t;
        part[t] = b < nblk ? blk_first[b] : 0u;
        __syncthreads();
        for (u32 d = 1; d < 1024u; d <<= 1) {
            const u32 other = t >= d ? part[t - d] : 0u;
            __syncthreads();
            if (other > part[t]) part[t] = other;
            __syncthreads();
        }
        const u32 mine = part[t] > carry ? part[t] : carry;
        if (b < nblk) pmax[b] = mine;
        __syncthreads();
        if (t == 1023) carry = mine;
        __syncthreads();
    }
}

// pre: [nblk] or nullptr - a block with a non-zero entry reports that status and is not framed; n_dev: nullptr, or where
// the number of columns lies on the device (the directory of r4x16_tok3_enc.hip: the launch's n is then only its bound)
struct T3In { const u32 *blk_first; const u32 *size; const i32 *id; const u32 *last_start, *nreads; const i32 *pre; const u32 *n_dev; };

// one wave per block: the verdict, the duplicates, every column's place behind the header, the block's size
__global__ __launch_bounds__(64) void k_t3_dup(T3In in, T3Cols w, const u32 *pmax, u32 *out_size, i32 *status, int nblk, u32 n_bound, u32 max_col)
{
    const int b = (int)blockIdx.x;
    const u32 lane = threadIdx.x;
    const u32 first = in.blk_first[b], next = in.blk_first[b + 1];
    const u32 n = in.n_dev ? (*in.n_dev < n_bound ? *in.n_dev : n_bound) : n_bound;
    i32 st = in.pre ? in.pre[b] : ST_OK;
    if (st != ST_OK) { if (lane == 0) { status[b] = st; out_size[b] = 0; } return; }
    if ((b == 0 && first != 0) || (b == nblk - 1 && next != n) || first > next || next > n || next - first > T3_MAX_IDS || first < pmax[b]) st = ST_SIZE;
    const u32 cnt = st == ST_OK ? next - first : 0u;
    for (u32 c0 = 0; c0 < cnt && st == ST_OK; c0 += 64) {                 // the first column that cannot be written
        const u32 c = first + c0 + lane;
        i32 code = ST_OK;
        if (c < next) {
            const i32 id = in.id[c];
            const u32 sz = in.size[c];
            if (sz == 0 || id < 0 || id >= T3_MAX_IDS || (c > first && in.id[c - 1] >= id)) code = ST_SIZE;
            else if (sz > max_col) code = ST_UNSUPPORTED;
            else if (w.s_status[c] != ST_OK) code = w.s_status[c] == ST_CAPACITY ? ST_UNSUPPORTED : w.s_status[c];   // (more than announced)
            else if (w.s_size[c] == 0) code = ST_UNSUPPORTED;
        }
        const u64 m = __ballot(code != ST_OK);
        if (m) st = __shfl(code, (int)__builtin_ctzll(m));
    }
    u64 run = T3_HEADER;
    if (st == ST_OK)
        for (u32 i = 0; i < cnt; i++) {
            const u32 ci = first + i, szi = w.s_size[ci];
            const u64 hi = w.hash[ci];
            const u8 *pi = w.streams + w.s_off[ci];
            int found = -1;
            if (var_len(szi) + szi > 4)                                   // :1466
                for (u32 j0 = 0; j0 < i && found < 0; j0 += 64) {
                    const u32 j = j0 + lane;
                    u64 m = __ballot(j < i && w.s_size[first + j] == szi && w.hash[first + j] == hi);
                    while (m) {
                        const u32 jj = j0 + (u32)__builtin_ctzll(m);
                        m &= m - 1;
                        if (t3_wave_equal(pi, w.streams + w.s_off[first + jj], szi, lane)) { found = (int)jj; break; }
                    }
                }
            // :1472, :1521: dup_from is the id, and an id of 0 reads as "none" - such a column is written in full
            const i32 from = found >= 0 ? in.id[first + found] : 0;
            if (lane == 0) { w.rel[ci] = (u32)run; w.dup[ci] = from; }
            run += from ? 3u : 1u + var_len(szi) + szi;
            if (run > 0xffffffffull) { st = ST_UNSUPPORTED; break; }      // a block's size is reported in 32 bits
        }
    if (lane == 0) { status[b] = st; out_size[b] = st == ST_OK ? (u32)run : 0u; }
}

__global__ __launch_bounds__(256) void k_t3_frame(T3In in, T3Cols w, PackedOut pk, u32 *out_size, i32 *status, u32 use_arith)
{
    const int b = (int)blockIdx.x;
    const u32 tid = threadIdx.x, lane = tid & 63u;
    if (status[b] != ST_OK) return;
    if (pk.off[b + 1] > pk.capacity) {
        __syncthreads();                                                  // (every thread has read the status)
        if (tid == 0) { status[b] = ST_CAPACITY; out_size[b] = 0; }
        return;
    }
    u8 *dst = pk.out + pk.off[b];
    if (tid == 0) {
        const u32 ls = in.last_start[b], nr = in.nreads[b];
        for (int k = 0; k < 4; k++) { dst[k] = (u8)(ls >> (8 * k)); dst[4 + k] = (u8)(nr >> (8 * k)); }
        dst[8] = (u8)use_arith;
    }
    const u32 first = in.blk_first[b], next = in.blk_first[b + 1];
    for (u32 c = first + (tid >> 6); c < next; c += 4) {
        const i32 id = in.id[c], from = w.dup[c];
        const u32 t = (u32)(id & 15) | ((c == first || (in.id[c - 1] >> 4) != (id >> 4)) ? 128u : 0u);     // :1517
        u8 *p = dst + w.rel[c];
        if (from) {
            if (lane == 0) { p[0] = (u8)(t | 64u); p[1] = (u8)(from >> 4); p[2] = (u8)(from & 15); }
            continue;
        }
        const u32 sz = w.s_size[c], nb = var_len(sz);
        if (lane == 0) { p[0] = (u8)t; var_put(p + 1, sz); }
        wave_copy(p + 1 + nb, w.streams + w.s_off[c], sz, lane);
    }
}

extern "C" int rans4x16_hip_tok3_pack_dev(rans4x16_hip_ctx *c, int nblk, int n, const uint32_t *d_blk_first,
                                          const unsigned char *d_in, const uint64_t *d_col_off, const uint32_t *d_col_size,
                                          const int32_t *d_col_id, const uint32_t *d_last_start, const uint32_t *d_nreads,
                                          unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                          uint32_t *d_out_size, int32_t *d_status,
                                          int k, const int *methods, int32_t *d_chosen,
                                          uint32_t max_col_size, uint64_t total_col_size, void *stream)
{
    if (!c) return -1;
    return r4x16_tok3_pack_run(c, nblk, n, d_blk_first, d_in, d_col_off, d_col_size, d_col_id, d_last_start, d_nreads, d_out, out_capacity,
                               d_out_off, d_out_size, d_status, k, methods, d_chosen, max_col_size, total_col_size, nullptr, false,
                               (hipStream_t)stream);
}

// The call above, and the second half of rans4x16_hip_tok3_encode_names_dev (r4x16_tok3_enc.hip).  n_on_device: n is the
// directory's room - the number of columns lies at d_blk_first[nblk], the entries behind it are idle (size 0) and belong
// to no block; d_pre: the blocks an earlier stage refused.
int r4x16_tok3_pack_run(rans4x16_hip_ctx *c, int nblk, int n, const uint32_t *d_blk_first,
                        const unsigned char *d_in, const uint64_t *d_col_off, const uint32_t *d_col_size,
                        const int32_t *d_col_id, const uint32_t *d_last_start, const uint32_t *d_nreads,
                        unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                        uint32_t *d_out_size, int32_t *d_status,
                        int k, const int *methods, int32_t *d_chosen,
                        uint32_t max_col_size, uint64_t total_col_size, const int32_t *d_pre, bool n_on_device, hipStream_t stream)
{
    if (nblk < 0 || n < 0 || (nblk == 0 && n) || k < 1 || k > 32 || !methods || !d_out_off ||
        (nblk && (!d_blk_first || !d_last_start || !d_nreads || (!d_out && out_capacity) || !d_out_size || !d_status)) ||
        (n && (!d_in || !d_col_off || !d_col_size || !d_col_id))) {
        c->err = "tok3_pack_dev: bad arguments";
        return -1;
    }
    // What the winners of n columns take together at most: the candidate that is always tried (a method without X_STRIPE
    // where the list has one: the others are skipped for sizes that are no multiple of 4) and has the smallest bound
    // succeeds within its bound, and the winner is no larger.  The bounds are 1.05 x size + a constant, rounded.
    const bool arith = (c->tok3_arith & R4X16_TOK3_ARITH_ENCODE) != 0;
    auto bound = [&](u32 size, int m) { return arith ? rans4x16_hip_arith_compress_cap(size, m) : r4x16_bound_hd(size, m); };
    int lean = -1;
    bool plain = false;
    for (int j = 0; j < k; j++) plain |= !(methods[j] & X_STRIPE);
    for (int j = 0; j < k; j++) {
        if ((methods[j] & X_STRIPE) && ((unsigned)methods[j] >> 8) > 255) { c->err = "tok3_pack_dev: more than 255 stripes"; return -1; }
        if (plain && (methods[j] & X_STRIPE)) continue;
        if (lean < 0 || bound(max_col_size, methods[j]) < bound(max_col_size, lean)) lean = methods[j];
    }
    // (arith: rans4x16_hip_arith_compress_cap is the size plus a constant of the method's - one for blocks of up to 20
    //  bytes, which are never striped, and one for larger blocks)
    const u64 per_col = arith ? std::max<u64>(bound(0, lean), bound(21, lean) - 21u) : bound(0, lean);
    u64 stream_bytes = (u64)n * bound(max_col_size, lean);
    if (total_col_size) stream_bytes = std::min<u64>(stream_bytes, (u64)(1.05 * (double)total_col_size) + 1 + (u64)n * (per_col + 4ull));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream;
    if (nblk == 0) { HIPCHK(c, hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s)); return 0; }
    T3Cols w;
    const size_t need = t3_cols_carve(&w, nullptr, (size_t)n, (size_t)nblk, stream_bytes);
    if (need > r4x16_room(c, A_BIT(A_WS) | A_BIT(A_XS) | A_BIT(A_T3)) / 2) {
        // (the winners of the whole batch wait in one arena until their blocks are framed; the best-of-k call in front of
        //  it walks the columns in chunks of its own)
        c->err = "tok3_pack_dev: the winners of this batch (" + std::to_string(need >> 20) + " MiB) do not fit half of max_workspace_mb: split the batch";
        return -1;
    }
    if (r4x16_ensure(c, A_T3, need, false) != 0) return -1;
    const size_t arena = t3_cols_carve(&w, c->at(A_T3), (size_t)n, (size_t)nblk, stream_bytes);
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    if (n) {
        const size_t keep_ws = c->max_ws;
        c->max_ws = keep_ws > arena + ((size_t)1 << 20) ? keep_ws - arena : (size_t)1 << 20;
        const int rc = arith
            ? rans4x16_hip_arith_compress_best_packed_dev(c, n, d_in, d_col_off, d_col_size, w.streams, stream_bytes, w.s_off, w.s_size,
                                                          w.s_status, k, methods, d_chosen, max_col_size, total_col_size, s)
            : rans4x16_hip_compress_best_packed_dev(c, n, d_in, d_col_off, d_col_size, w.streams, stream_bytes, w.s_off, w.s_size,
                                                    w.s_status, k, methods, d_chosen, max_col_size, total_col_size, s);
        c->max_ws = keep_ws;
        if (rc != 0) return -1;
        hipLaunchKernelGGL(k_t3_hash, dim3((u32)((n + 3) / 4)), dim3(256), 0, s, w, n);
    }
    const T3In in = {d_blk_first, d_col_size, d_col_id, d_last_start, d_nreads, d_pre, n_on_device ? d_blk_first + nblk : nullptr};
    const PackedOut pk = {d_out, d_out_off, out_capacity};
    hipLaunchKernelGGL(k_t3_first_max, dim3(1), dim3(1024), 0, s, d_blk_first, w.pmax, nblk);
    hipLaunchKernelGGL(k_t3_dup, dim3((u32)nblk), dim3(64), 0, s, in, w, (const u32 *)w.pmax, d_out_size, d_status, nblk, (u32)n, max_col_size);
    r4x16_launch_packed_scan(d_out_size, d_out_off, 0, nblk, s);
    hipLaunchKernelGGL(k_t3_frame, dim3((u32)nblk), dim3(256), 0, s, in, w, pk, d_out_size, d_status, arith ? 1u : 0u);
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}
