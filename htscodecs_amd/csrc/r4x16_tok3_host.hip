// r4x16_tok3_host.hip - tok3 names with host buffers (include/rans4x16_hip.h part 2f): encode_names / decode_names of
// htscodecs tokenise_name3.c behind the reference's own signatures, and their batch forms.  Orchestration over the device
// calls of parts 2c to 2e - this unit finds the limits those calls ask of their caller, cuts a batch into chunks whose
// arenas fit, and moves the bytes - and one kernel:
//
//   k_te_measure : one wave per block, 64 bytes a step, ballots of "byte <= '\n'" as k_te_frame takes them
//                  (r4x16_tok3_enc.hip): the names of the block and its longest name; the maxima over the chunk go into
//                  a 16-byte record, the only limits the host reads back.  The host never walks name bytes to find them.
//
// Encode, per chunk: the blocks gathered into the staging arena -> k_te_measure -> rans4x16_hip_tok3_tokenise_dev into the
// staging arena -> the column count and sizes read back -> the pack stages over exactly those columns, into an arena
// sized from the winners' bound plus framing (the names arena: the tokeniser is done with it) -> sizes and offsets read
// once, the dense arena copied down once and scattered.
// Decode, per chunk: rans4x16_hip_tok3_scan per container on the host (descriptors only) gives the limits; the accepted
// containers gathered -> rans4x16_hip_tok3_decode_names_dev -> sizes read, the dense arena copied down and scattered.
//
// The arith flavour (rans4x16_hip_set_tok3_arith): with ENCODE the pack stages write use_arith = 1 and the bounds below
// are the arith coder's; with DECODE the scan admits either flavour and the device calls decode each block by its own.
// rans4x16_hip_tok3_arith_encode_names / _decode_names set the mode for their one call and put the caller's back.
//
// Arenas: A_STAGE is this unit's (layouts below, dry for the plan and over the arena for the run); A_TN, A_T3, A_WS and
// A_XS are those of the device calls.  Everything runs on the context's own stream.
#include "r4x16_host.h"
#include "r4x16_tok3_walk.h"

#define NH_MAX_IN (65535u * 256u)        // rans4x16_hip_tok3_tokenise_dev's hard limits (part 2e)
#define NH_MAX_NAMES 0xffffffu
#define NH_MAX_NAME_LEN 16384u
#define NH_PAD 64u                       // between gathered blocks: the kernels load aligned words that hold a block's last byte
#define NH_REUSE (A_BIT(A_STAGE) | A_BIT(A_WS) | A_BIT(A_XS) | A_BIT(A_T3) | A_BIT(A_TN))

// rec[0] names of the block with most, rec[1] longest name, rec[2] blocks measured
__global__ __launch_bounds__(64) void k_te_measure(const u8 *in, const u64 *off, const u32 *size, u32 max_in, u32 *rec)
{
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const u32 sz = size[b];
    if (sz > max_in) return;                                              // not uploaded: the tokeniser refuses it unread
    const u8 *src = in + off[b];
    u32 count = 0, cur = 0, maxlen = 0;
    for (u32 i0 = 0; i0 < sz; i0 += 64) {                                 // sz <= max_in
        const u32 i = i0 + lane;
        const u32 c = i < sz ? src[i] : 0x40u;
        const bool term = c <= '\n';
        const u64 m = __ballot(term);
        if (term) {
            const u64 below = m & ((1ull << lane) - 1ull);
            const u32 s = below ? i0 + 64u - (u32)__builtin_clzll(below) : cur;
            if (i - s > maxlen) maxlen = i - s;
        }
        if (m) { count += (u32)__builtin_popcountll(m); cur = i0 + 64u - (u32)__builtin_clzll(m); }
    }
    for (int d = 32; d; d >>= 1) { const u32 o = (u32)__shfl_xor((int)maxlen, d); maxlen = o > maxlen ? o : maxlen; }
    if (lane == 0) { atomicMax(rec, count); atomicMax(rec + 1, maxlen); atomicAdd(rec + 2, 1u); }
}

// ---- layouts of the staging arena -------------------------------------------------------------------------------
struct NhEnc {
    u8 *in; u64 *in_off; u32 *in_size; u32 *rec;
    u8 *cols; u64 *cols_off; u32 *cols_size; i32 *tok_status; u32 *blk_first, *last_start, *nreads;
    i32 *col_id; u64 *col_off; u32 *col_size;
};
static size_t nh_enc_carve(NhEnc *e, u8 *base, size_t nblk, size_t in_bytes)
{
    Carver cv(base);
    const size_t items = nblk * (size_t)T3_MAX_IDS;
    e->in = cv.take<u8>(in_bytes + NH_PAD); e->in_off = cv.take<u64>(nblk); e->in_size = cv.take<u32>(nblk); e->rec = cv.take<u32>(4);
    e->cols = cv.take<u8>(6 * in_bytes + NH_PAD); e->cols_off = cv.take<u64>(nblk + 1); e->cols_size = cv.take<u32>(nblk);
    e->tok_status = cv.take<i32>(nblk); e->blk_first = cv.take<u32>(nblk + 1); e->last_start = cv.take<u32>(nblk); e->nreads = cv.take<u32>(nblk);
    e->col_id = cv.take<i32>(items); e->col_off = cv.take<u64>(items); e->col_size = cv.take<u32>(items);
    return cv.total();
}
// the results of either direction: a dense arena and its per-block arrays (encode: in the names arena, behind the tokeniser)
struct NhOut { u8 *out; u64 *off; u32 *size; i32 *status; u32 *nnames; };
static size_t nh_out_carve(NhOut *o, u8 *base, size_t at, size_t nblk, size_t out_bytes)
{
    Carver cv(base, at);
    o->out = cv.take<u8>(out_bytes + NH_PAD); o->off = cv.take<u64>(nblk + 1); o->size = cv.take<u32>(nblk); o->status = cv.take<i32>(nblk);
    o->nnames = cv.take<u32>(nblk);
    return cv.total();
}
struct NhDec { u8 *in; u64 *in_off; u32 *in_size; NhOut o; };
static size_t nh_dec_carve(NhDec *d, u8 *base, size_t nblk, size_t in_bytes, size_t out_bytes)
{
    Carver cv(base);
    d->in = cv.take<u8>(in_bytes + NH_PAD); d->in_off = cv.take<u64>(nblk); d->in_size = cv.take<u32>(nblk);
    return nh_out_carve(&d->o, base, cv.total(), nblk, out_bytes);
}

static size_t nh_slot(size_t bytes) { return align_up(bytes + NH_PAD, 64); }

// the largest bound of the list for a column of `size` bytes: the winner is no larger than its own
static u64 nh_col_bound(u32 size, int k, const int *methods, bool arith)
{
    u32 best = 0;
    for (int j = 0; j < k; j++) best = std::max(best, arith ? rans4x16_hip_arith_compress_cap(size, methods[j]) : r4x16_compress_bound(size, methods[j]));
    return (u64)best + 6;                                                 // the type byte and var_put_u32(clen)
}

// What a block of `size` bytes adds to an encode chunk at most, before anything of it is known: this unit's staging, the
// tokeniser's arena under the limits the largest block of the batch allows, the winners (r4x16_tok3.hip)
static size_t nh_enc_foot(u32 size, u32 batch_max_in)
{
    NhEnc e;
    if (size > NH_MAX_IN) return 256;                                     // refused before upload
    const u32 mi = std::max(batch_max_in, 1u);
    return nh_enc_carve(&e, nullptr, 1, nh_slot(size)) +
           r4x16_tok3_tokenise_need(1, mi, std::min(mi, NH_MAX_NAMES), std::min(mi, NH_MAX_NAME_LEN), std::max(size, 1u)) +
           2 * (6 * (size_t)size) + ((size_t)256 << 10);
}

static void nh_count(rans4x16_hip_ctx *c, int kind, long by)
{
    if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_NAMES][kind] += by;
}

// a block's result into the caller's buffer, or one of exactly its size; 0 or the status
static int nh_deliver(const u8 *src, u32 size, unsigned char **out, unsigned int *out_size)
{
    if (*out) {
        if (*out_size < size) return R4X16_E_CAPACITY;
        memcpy(*out, src, size);
    } else {
        unsigned char *p = (unsigned char *)malloc(size ? size : 1);
        if (!p) return R4X16_E_CAPACITY;
        memcpy(p, src, size);
        *out = p;
    }
    *out_size = size;
    return R4X16_OK;
}

// ---- encode ------------------------------------------------------------------------------------------------------
// blocks [lo, lo + nb): 0 = their results are with the caller; -1 = nothing was delivered (err set), the caller may try fewer
static int nh_enc_chunk(rans4x16_hip_ctx *c, size_t lo, size_t nb, const unsigned char *const *in, const unsigned int *in_size,
                        unsigned char **out, unsigned int *out_size, int k, const int *methods, unsigned int *last_start,
                        unsigned int *nreads, int *status, int *failed)
{
    hipStream_t s = c->stream;
    std::vector<u64> in_off(nb, 0);
    std::vector<u32> isz(nb);
    size_t in_bytes = 0, uploaded = 0;
    u32 max_in = 1;
    for (size_t i = 0; i < nb; i++) {
        isz[i] = in_size[lo + i];
        if (isz[i] > NH_MAX_IN) continue;
        in_off[i] = in_bytes; in_bytes += nh_slot(isz[i]);
        max_in = std::max(max_in, isz[i]);
        uploaded++;
    }
    NhEnc e;
    if (r4x16_ensure(c, A_STAGE, nh_enc_carve(&e, nullptr, nb, in_bytes), false) != 0) return -1;
    nh_enc_carve(&e, c->at(A_STAGE), nb, in_bytes);
    // gather: one host copy per block into one buffer, one transfer
    std::vector<u8> host(in_bytes + NH_PAD, 0);
    for (size_t i = 0; i < nb; i++)
        if (isz[i] && isz[i] <= NH_MAX_IN) memcpy(host.data() + in_off[i], in[lo + i], isz[i]);
    HIPCHK(c, hipMemcpyAsync(e.in, host.data(), host.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(e.in_off, in_off.data(), nb * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(e.in_size, isz.data(), nb * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(e.rec, 0, 16, s));
    hipLaunchKernelGGL(k_te_measure, dim3((u32)nb), dim3(64), 0, s, (const u8 *)e.in, (const u64 *)e.in_off, (const u32 *)e.in_size, max_in, e.rec);
    HIPCHK(c, hipGetLastError());
    u32 rec[4];
    HIPCHK(c, hipMemcpyAsync(rec, e.rec, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // the limits: what the chunk holds, clamped to what the tokeniser takes - a block beyond them is refused alone
    const u32 max_names = std::min(std::max(rec[0], 1u), NH_MAX_NAMES), max_name_len = std::min(rec[1], NH_MAX_NAME_LEN);
    const u64 col_cap = 6ull * in_bytes;
    if (rans4x16_hip_tok3_tokenise_dev(c, (int)nb, e.in, e.in_off, e.in_size, e.cols, col_cap, e.cols_off, e.cols_size, e.tok_status,
                                       e.blk_first, e.col_id, e.col_off, e.col_size, e.last_start, e.nreads, max_in, max_names,
                                       max_name_len, T3_MAX_TOKENS, T3_MAX_IDS, (u64)std::max(in_bytes, (size_t)1), 0, s) != 0) return -1;
    // how many columns there are, and how large: the pack runs over exactly these
    std::vector<u32> first(nb + 1), csz;
    HIPCHK(c, hipMemcpyAsync(first.data(), e.blk_first, (nb + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const size_t n = first[nb];
    if (n > nb * (size_t)T3_MAX_IDS) { c->err = "tok3_encode_names_batch: the tokeniser's directory is inconsistent"; return -1; }
    csz.resize(n);
    if (n) HIPCHK(c, hipMemcpyAsync(csz.data(), e.col_size, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    u64 out_bound = (u64)nb * T3_HEADER, total_col = 0;
    u32 max_col = 1;
    const bool arith = (c->tok3_arith & R4X16_TOK3_ARITH_ENCODE) != 0;
    for (size_t i = 0; i < n; i++) { out_bound += nh_col_bound(csz[i], k, methods, arith); total_col += csz[i]; max_col = std::max(max_col, csz[i]); }
    NhOut o;
    if (r4x16_ensure(c, A_TN, nh_out_carve(&o, nullptr, 0, nb, (size_t)out_bound), false) != 0) return -1;
    nh_out_carve(&o, c->at(A_TN), 0, nb, (size_t)out_bound);
    if (r4x16_tok3_pack_run(c, (int)nb, (int)n, e.blk_first, e.cols, e.col_off, e.col_size, e.col_id, e.last_start, e.nreads, o.out, out_bound,
                            o.off, o.size, o.status, k, methods, nullptr, max_col, total_col, e.tok_status, false, s) != 0) return -1;
    std::vector<u64> off(nb + 1);
    std::vector<u32> size(nb), ls(nb), nr(nb);
    std::vector<i32> st(nb);
    HIPCHK(c, hipMemcpyAsync(off.data(), o.off, (nb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(size.data(), o.size, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(st.data(), o.status, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(ls.data(), e.last_start, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(nr.data(), e.nreads, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (off[nb] > out_bound) { c->err = "tok3_encode_names_batch: the results exceed their bound"; return -1; }
    std::vector<u8> arena((size_t)off[nb]);
    if (off[nb]) HIPCHK(c, hipMemcpyAsync(arena.data(), o.out, (size_t)off[nb], hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < nb; i++) {
        int rc = st[i];
        if (rc == R4X16_OK && (off[i] + size[i] > off[nb] || size[i] == 0)) rc = R4X16_E_SIZE;
        if (rc == R4X16_OK) rc = nh_deliver(arena.data() + off[i], size[i], &out[lo + i], &out_size[lo + i]);
        if (rc != R4X16_OK) { out_size[lo + i] = 0; (*failed)++; }
        if (status) status[lo + i] = rc;
        if (last_start) last_start[lo + i] = ls[i];
        if (nreads) nreads[lo + i] = nr[i];
    }
    nh_count(c, R4X16_NAMES_ENC_CHUNKS, 1);
    nh_count(c, R4X16_NAMES_UPLOADED, (long)uploaded);
    nh_count(c, R4X16_NAMES_REFUSED, (long)(nb - uploaded));
    return 0;
}

// the ranges of a batch: the cut of r4x16_plan.h over the footprints, every range run through r4x16_backoff
template <class F>
static int nh_walk(rans4x16_hip_ctx *c, const std::vector<size_t> &foot, F run)
{
    const size_t n = foot.size();
    std::vector<size_t> ends(n);
    const size_t cap = r4x16_room(c, NH_REUSE) / 2;
    const size_t ranges = r4x16_cut_ranges(foot.data(), n, cap, (size_t)c->names_chunk_blocks, ends.data());
    size_t at = 0;
    for (size_t r = 0; r < ranges; r++)
        while (at < ends[r]) {
            size_t chunk = ends[r] - at;
            if (r4x16_backoff(chunk, [&](size_t nb) { return run(at, nb); }) != 0) return -1;
            at += chunk;
        }
    return 0;
}

extern "C" int rans4x16_hip_tok3_encode_names_batch(rans4x16_hip_ctx *c, int nblk,
                                                    const unsigned char *const *in, const unsigned int *in_size,
                                                    unsigned char **out, unsigned int *out_size,
                                                    int k, const int *methods, unsigned int *last_start, unsigned int *nreads, int *status)
{
    if (!c) return -1;
    if (nblk < 0 || k < 1 || k > 32 || !methods || (nblk && (!in || !in_size || !out || !out_size))) {
        c->err = "tok3_encode_names_batch: bad arguments";
        return -1;
    }
    for (int i = 0; i < nblk; i++)
        if (!in[i] && in_size[i]) { c->err = "tok3_encode_names_batch: a block without a buffer"; return -1; }
    if (nblk == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    u32 batch_max = 1;
    for (int i = 0; i < nblk; i++) if (in_size[i] <= NH_MAX_IN) batch_max = std::max(batch_max, in_size[i]);
    std::vector<size_t> foot((size_t)nblk);
    for (int i = 0; i < nblk; i++) foot[i] = nh_enc_foot(in_size[i], batch_max);
    int failed = 0;
    if (nh_walk(c, foot, [&](size_t at, size_t nb) {
            return nh_enc_chunk(c, at, nb, in, in_size, out, out_size, k, methods, last_start, nreads, status, &failed);
        }) != 0) return -1;
    return failed;
}

// ---- decode ------------------------------------------------------------------------------------------------------
struct NhScan { int rc; u32 last_start, nreads, ndesc, largest_col; u64 total; };

// names a container can decode to at most: the header's count, a name per byte of column 0, a byte (its NUL) per name
static u32 nh_names(const NhScan &sc) { return std::max(std::min(std::min(sc.nreads, sc.largest_col), sc.last_start), 1u); }

// the accepted containers which[lo .. lo + nb) of the batch
static int nh_dec_chunk(rans4x16_hip_ctx *c, const std::vector<int> &which, const std::vector<NhScan> &scan, size_t lo, size_t nb,
                        const unsigned char *const *in, const unsigned int *in_size, unsigned char **out, unsigned int *out_size,
                        unsigned int *nnames, int *status, int *failed)
{
    hipStream_t s = c->stream;
    std::vector<u64> in_off(nb);
    std::vector<u32> isz(nb);
    size_t in_bytes = 0;
    u64 out_bytes = 0, total_col = 0;
    u32 max_in = 1, max_columns = 1, max_names = 1, max_col = 1;
    for (size_t i = 0; i < nb; i++) {
        const int b = which[lo + i];
        const NhScan &sc = scan[b];
        isz[i] = in_size[b];
        in_off[i] = in_bytes; in_bytes += nh_slot(isz[i]);
        out_bytes += sc.last_start; total_col += sc.total;
        max_in = std::max(max_in, isz[i]); max_columns = std::max(max_columns, sc.ndesc);
        max_names = std::max(max_names, nh_names(sc));
        max_col = std::max(max_col, sc.largest_col);
    }
    NhDec d;
    if (r4x16_ensure(c, A_STAGE, nh_dec_carve(&d, nullptr, nb, in_bytes, (size_t)out_bytes), true) != 0) return -1;
    nh_dec_carve(&d, c->at(A_STAGE), nb, in_bytes, (size_t)out_bytes);
    std::vector<u8> host(in_bytes + NH_PAD, 0);
    for (size_t i = 0; i < nb; i++) memcpy(host.data() + in_off[i], in[which[lo + i]], isz[i]);
    HIPCHK(c, hipMemcpyAsync(d.in, host.data(), host.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d.in_off, in_off.data(), nb * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d.in_size, isz.data(), nb * 4, hipMemcpyHostToDevice, s));
    // X_STRIPE columns (levels 3 and up): what rans4x16_hip_set_dev_stripe_planes arranges, for this call alone
    int rc;
    {
        StripeLimits limits(c, 4, max_col);
        rc = rans4x16_hip_tok3_decode_names_dev(c, (int)nb, d.in, d.in_off, d.in_size, d.o.out, out_bytes, d.o.off, d.o.size, d.o.nnames,
                                                d.o.status, nullptr, max_columns, max_in, max_col, max_names, T3_MAX_TOKENS,
                                                std::max<u64>(total_col, 1), s);
    }
    if (rc != 0) return -1;
    std::vector<u64> off(nb + 1);
    std::vector<u32> size(nb), nn(nb);
    std::vector<i32> st(nb);
    HIPCHK(c, hipMemcpyAsync(off.data(), d.o.off, (nb + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(size.data(), d.o.size, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(st.data(), d.o.status, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(nn.data(), d.o.nnames, nb * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // the dense arena comes down once, up to the last block that decoded (a failed block keeps its range, and a hostile
    // header may have claimed a large one: what lies behind the last good block is not fetched)
    size_t down = 0;
    for (size_t i = 0; i < nb; i++) {
        if (st[i] == R4X16_OK && (off[i] > out_bytes || size[i] > out_bytes - off[i])) st[i] = R4X16_E_SIZE;
        if (st[i] == R4X16_OK) down = (size_t)(off[i] + size[i]);
    }
    std::vector<u8> arena(down);
    if (down) HIPCHK(c, hipMemcpyAsync(arena.data(), d.o.out, down, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < nb; i++) {
        const int b = which[lo + i];
        int r = st[i];
        if (r == R4X16_OK) r = nh_deliver(arena.data() + off[i], size[i], &out[b], &out_size[b]);
        if (r != R4X16_OK) { out_size[b] = 0; (*failed)++; }
        if (status) status[b] = r;
        if (nnames) nnames[b] = r == R4X16_OK ? nn[i] : 0;
    }
    nh_count(c, R4X16_NAMES_DEC_CHUNKS, 1);
    nh_count(c, R4X16_NAMES_UPLOADED, (long)nb);
    return 0;
}

extern "C" int rans4x16_hip_tok3_decode_names_batch(rans4x16_hip_ctx *c, int nblk,
                                                    const unsigned char *const *in, const unsigned int *in_size,
                                                    unsigned char **out, unsigned int *out_size, unsigned int *nnames, int *status)
{
    if (!c) return -1;
    if (nblk < 0 || (nblk && (!in || !in_size || !out || !out_size))) { c->err = "tok3_decode_names_batch: bad arguments"; return -1; }
    for (int i = 0; i < nblk; i++)
        if (!in[i] && in_size[i]) { c->err = "tok3_decode_names_batch: a block without a buffer"; return -1; }
    if (nblk == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    // the descriptors of every container, on the host: its limits, or the status it is refused with
    std::vector<NhScan> scan((size_t)nblk);
    std::vector<int> which;
    u32 max_columns = 1, max_names = 1;
    int failed = 0;
    const size_t cap = r4x16_room(c, NH_REUSE) / 2;
    for (int i = 0; i < nblk; i++) {
        NhScan &sc = scan[i];
        sc.rc = (c->tok3_arith & R4X16_TOK3_ARITH_DECODE)
            ? rans4x16_hip_tok3_scan_any(in[i], in_size[i], 0, 0, &sc.last_start, &sc.nreads, &sc.ndesc, nullptr, &sc.total, &sc.largest_col, nullptr, nullptr)
            : rans4x16_hip_tok3_scan(in[i], in_size[i], 0, 0, &sc.last_start, &sc.nreads, &sc.ndesc, nullptr, &sc.total, &sc.largest_col, nullptr);
        if (sc.rc < 0) { c->err = "tok3_decode_names_batch: bad arguments"; return -1; }
        if (sc.rc == R4X16_OK) {
            // a container that claims more than the context may take, alone: hostile or too large for this card
            NhDec d;
            const u32 names = nh_names(sc);
            const u64 units = (u64)names + ((u64)names * T3_MAX_TOKENS * 8u + 15u) / 16u;
            if (units > 0xffffffffull || sc.total > cap || sc.last_start > cap ||
                nh_dec_carve(&d, nullptr, 1, nh_slot(in_size[i]), sc.last_start) +
                r4x16_tok3_decode_names_need(1, std::max(sc.ndesc, 1u), names, T3_MAX_TOKENS, std::max<u64>(sc.total, 1)) > cap)
                sc.rc = R4X16_E_UNSUPPORTED;
        }
        if (sc.rc != R4X16_OK) {
            out_size[i] = 0;
            if (status) status[i] = sc.rc;
            if (nnames) nnames[i] = 0;
            failed++;
            nh_count(c, R4X16_NAMES_REFUSED, 1);
            continue;
        }
        which.push_back(i);
        max_columns = std::max(max_columns, sc.ndesc);
        max_names = std::max(max_names, nh_names(sc));
    }
    // a block's footprint under the limits of the whole batch: a chunk's arenas are laid out for its largest
    std::vector<size_t> foot(which.size());
    for (size_t j = 0; j < which.size(); j++) {
        const NhScan &sc = scan[which[j]];
        NhDec d;
        foot[j] = nh_dec_carve(&d, nullptr, 1, nh_slot(in_size[which[j]]), sc.last_start) +
                  r4x16_tok3_decode_names_need(1, max_columns, max_names, T3_MAX_TOKENS, std::max<u64>(sc.total, 1));
    }
    if (nh_walk(c, foot, [&](size_t at, size_t nb) {
            return nh_dec_chunk(c, which, scan, at, nb, in, in_size, out, out_size, nnames, status, &failed);
        }) != 0) return -1;
    return failed;
}

// ---- the reference's two functions ----------------------------------------------------------------------------------
extern "C" int rans4x16_hip_tok3_level_methods(int level, int *methods)
{
    static const int rows[5][10] = {                                      // tokenise_name3.c:1254-1260: count, methods
        {2, 0, 128},
        {2, 0, 192 + 8},
        {3, 0, 128, 193 + 8},
        {6, 0, 1, 129, 65, 193, 193 + 8},
        {9, 0, 1, 128, 129, 64, 65, 192, 193, 193 + 8},
    };
    if (!methods) return -1;
    level = (level - 1) / 2;
    level = level < 0 ? 0 : level > 4 ? 4 : level;
    for (int j = 0; j < rows[level][0]; j++) methods[j] = rows[level][1 + j];
    return rows[level][0];
}

// the mode a caller set on the thread's context (rans4x16_hip_thread_ctx), put back when the single-block call ends
struct Tok3ArithMode {
    rans4x16_hip_ctx *c;
    int was;
    Tok3ArithMode(rans4x16_hip_ctx *c_, int mode) : c(c_), was(c_->tok3_arith) { c->tok3_arith = mode; }
    ~Tok3ArithMode() { c->tok3_arith = was; }
    Tok3ArithMode(const Tok3ArithMode &) = delete;
    Tok3ArithMode &operator=(const Tok3ArithMode &) = delete;
};

static unsigned char *nh_encode_one(char *blk, int len, int level, int mode, int *out_len, int *last_start_p)
{
    if (!blk || len < 0 || !out_len) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    Tok3ArithMode flavour(c, mode);
    int methods[9];
    const int k = rans4x16_hip_tok3_level_methods(level, methods);
    const unsigned char *ins[1] = {(const unsigned char *)blk};
    unsigned char *outs[1] = {nullptr};
    unsigned int isz[1] = {(unsigned int)len}, osz[1] = {0}, ls[1] = {0};
    const int rc = rans4x16_hip_tok3_encode_names_batch(c, 1, ins, isz, outs, osz, k, methods, ls, nullptr, nullptr);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || !outs[0]) return nullptr;
    // the caller's buffer, as the reference leaves it (:1374): the separators in front of last_start become NULs.  It is
    // host memory that only the host can write; the limits and the tokens never come from a host walk.
    for (unsigned int i = 0; i < ls[0]; i++) if ((unsigned char)blk[i] <= '\n') blk[i] = '\0';
    *out_len = (int)osz[0];
    if (last_start_p) *last_start_p = (int)ls[0];
    return outs[0];
}

extern "C" unsigned char *rans4x16_hip_tok3_encode_names(char *blk, int len, int level, int use_arith, int *out_len, int *last_start_p)
{
    if (use_arith) {
        static std::once_flag once;
        std::call_once(once, [] { fprintf(stderr, "rans4x16_hip: encode_names with use_arith != 0 is the arithmetic flavour: call rans4x16_hip_tok3_arith_encode_names (include/tok3_names_hip.h forwards there)\n"); });
        return nullptr;
    }
    return nh_encode_one(blk, len, level, 0, out_len, last_start_p);
}

extern "C" unsigned char *rans4x16_hip_tok3_arith_encode_names(char *blk, int len, int level, int *out_len, int *last_start_p)
{
    return nh_encode_one(blk, len, level, R4X16_TOK3_ARITH_ENCODE, out_len, last_start_p);
}

static unsigned char *nh_decode_one(unsigned char *in, uint32_t sz, int mode, uint32_t *out_len)
{
    if (!in || !out_len) return nullptr;
    rans4x16_hip_ctx *c = r4x16_thread_ctx();
    if (!c) return nullptr;
    Tok3ArithMode flavour(c, mode);
    const unsigned char *ins[1] = {in};
    unsigned char *outs[1] = {nullptr};
    unsigned int isz[1] = {sz}, osz[1] = {0};
    const int rc = rans4x16_hip_tok3_decode_names_batch(c, 1, ins, isz, outs, osz, nullptr, nullptr);
    r4x16_trim(c, SINGLE_CALL_KEEP);
    if (rc != 0 || !outs[0]) return nullptr;
    *out_len = osz[0];
    return outs[0];
}

extern "C" unsigned char *rans4x16_hip_tok3_decode_names(unsigned char *in, uint32_t sz, uint32_t *out_len)
{
    return nh_decode_one(in, sz, 0, out_len);
}

extern "C" unsigned char *rans4x16_hip_tok3_arith_decode_names(unsigned char *in, uint32_t sz, uint32_t *out_len)
{
    return nh_decode_one(in, sz, R4X16_TOK3_ARITH_DECODE, out_len);
}
