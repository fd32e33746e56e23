// r4x16_tok3_names.hip - tok3 name decoding on the device (include/rans4x16_hip.h part 2d): what decode_name
// (htscodecs tokenise_name3.c:1018-1189) and the loop around it (:1671-1689) do with the token columns of a name block.
//
//   k_tn_claim  : one wave per block - the names it holds (bytes of column id 0), its token positions, the verdict of the
//                 framing rules, what it claims of the output arena (last_start) and of the history arena
//   k_pk_scan   : twice - history claims -> offsets, output claims -> d_out_off (r4x16_packed.hip)
//   k_tn_decode : one wave per block, lane t owns token position t (positions 64..127: a second pass of the same wave,
//                 entered only by blocks that have them).  Names depend on earlier names, so the loop over names is
//                 serial; inside a name every step is wave-wide:
//                   position 0 (type, distance) is read by all lanes alike;
//                   every lane reads its next type byte speculatively, one ballot of "this is an end" gives the end
//                   position e, and lanes 1..e commit their type cursors;
//                   lanes below e turn their token into an entry (type, value, aux) from their value columns or from
//                   the entry the earlier name has at their position, and the entry into a length and either up to ten
//                   immediate bytes or a source in the position's N_ALPHA column;
//                   a wave scan of the lengths places the bytes; every lane puts its own into a copy of the name in
//                   LDS, which leaves in whole-wave stores (a name above 1,024 bytes: every lane writes its own).
//                 A N_DUP name is the earlier name's entries rendered again: it reads no column but its distance.
//
// History.  An entry is 8 bytes: value | aux << 32 | type << 60; aux is the width of a N_DIGITS0 token or where a
// N_ALPHA string starts in its column (28 bits: a column of 2^28 bytes or more is refused).  A string is always copied
// from its column, never from an earlier name, so the kernel only ever writes the output arena.  Entries lie
// position-major, ent[t * count + name], behind one 16-byte record per name (start, length, state, end position);
// `state` is the name whose entries a name has - its own, or for a N_DUP name those of the name it repeats, which are
// not copied.  The entries of the state last used stay in registers (distance 1 is three quarters of real names).
// Lane t alone writes and reads ent[t * ..], lane 0 alone the records: no lane reads what another lane wrote, so the
// kernel needs no fence.
//
// Loops: the name loop runs count <= max_names trips (k_tn_claim refuses more); directory loops run ncol <= max_columns
// trips; a string is searched inside what is left of its column (c_rem, from the directory, checked against
// col_capacity when the map is built) and copied in len <= that many bytes; everything else is unrolled.  Lanes that
// have no token hold length 0 and enter no data-dependent loop.
#include "r4x16_host.h"
#include "r4x16_tok3_walk.h"

enum { TN_ALPHA = 1, TN_CHAR = 2, TN_DIGITS0 = 3, TN_DZLEN = 4, TN_DUP = 5, TN_DIFF = 6, TN_DIGITS = 7, TN_DDELTA = 8,
       TN_DDELTA0 = 9, TN_MATCH = 10, TN_NOP = 11, TN_END = 12, TN_REPLAY = 16 /* not a token: a N_DUP name's positions */ };
#define TN_TOKENS 0x0f8eu               // the types decode_name's switch knows (:1063-1173); any other value ends the name (:1175)
#define TN_MAX_COLUMN (1u << 28)
#define TN_NONE 0xffffffffu

// what rans4x16_hip_tok3_unpack_dev wrote
struct TnIn {
    const u8 *cols; u64 col_capacity;
    const i32 *col_id; const u64 *col_off; const u32 *col_size;
    const u32 *ncol, *last_start, *nreads; const i32 *blk_status;
    u32 maxc, max_names, max_tokens;
};
// per block [nblk] (hoff: one more); hist: the histories back to back, block b's at hist + 16 * hoff[b]
struct TnWs { u32 *hclaim; u64 *hoff; u32 *oclaim, *count, *npos; i32 *pre; u8 *hist; u64 hist_bytes; };
struct TnOut { u8 *out; u64 capacity; const u64 *off; u32 *out_size, *nnames; i32 *status; u32 *name_start; };

static size_t tn_carve(TnWs *w, u8 *base, size_t at, size_t nblk, size_t hist_bytes)
{
    Carver cv(base, at);
    w->hclaim = cv.take<u32>(nblk); w->hoff = cv.take<u64>(nblk + 1); w->oclaim = cv.take<u32>(nblk);
    w->count = cv.take<u32>(nblk); w->npos = cv.take<u32>(nblk); w->pre = cv.take<i32>(nblk);
    w->hist = cv.take<u8>(hist_bytes + 16);
    w->hist_bytes = hist_bytes;
    return cv.total();
}

__device__ __forceinline__ u32 tn_wave_max(u32 v)
{
    for (int d = 32; d; d >>= 1) { const u32 o = (u32)__shfl_xor((int)v, d); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(64) void k_tn_claim(TnIn in, TnWs w)
{
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)b * in.maxc;
    const bool skipped = in.blk_status && in.blk_status[b] != ST_OK;
    const u32 nc = skipped ? 0u : (in.ncol[b] < in.maxc ? in.ncol[b] : in.maxc);
    const u32 nreads = in.nreads[b], last_start = in.last_start[b];
    u32 cnt = 0, top = 0;
    for (u32 c0 = 0; c0 < nc; c0 += 64) {                                 // nc <= max_columns
        const u32 c = c0 + lane;
        const i32 id = c < nc ? in.col_id[base + c] : -1;
        if (id < 0) continue;
        const u32 cid = (u32)id & (T3_MAX_IDS - 1u);
        if ((cid >> 4) + 1 > top) top = (cid >> 4) + 1;
        if (cid == 0) cnt = in.col_size[base + c];
        else if ((cid >> 4) == 0 && (id & R4X16_TOK3_TYPE_COLUMN)) cnt = nreads;
    }
    cnt = tn_wave_max(cnt);
    top = tn_wave_max(top);
    if (lane) return;
    i32 st = skipped ? in.blk_status[b] : ST_OK;
    if (st == ST_OK) {
        if (nreads == 0 || cnt > nreads || last_start >= 0x7fffffffu - 1024u) st = ST_SIZE;     // create_context, :1023, :1555
        else if (top > in.max_tokens || cnt > in.max_names) st = ST_UNSUPPORTED;
    }
    w.pre[b] = st;
    w.count[b] = st == ST_OK ? cnt : 0u;
    w.npos[b] = top;
    w.oclaim[b] = skipped ? 0u : last_start;
    // (cnt <= max_names, top <= max_tokens: the host checked that this fits 32 bits)
    w.hclaim[b] = st == ST_OK ? (u32)(cnt + ((u64)cnt * top * 8u + 15u) / 16u) : 0u;
}

// ---- bytes ---------------------------------------------------------------------------------------------------
// n <= 8 bytes at p, by aligned 8-byte loads that hold at least one of them
__device__ __forceinline__ u64 tn_load8(const u8 *p, u32 n)
{
    const u64 a = (u64)p, al = a & ~7ull;
    const u32 sh = (u32)(a & 7u) * 8u;
    u64 v = *(const u64 *)al >> sh;
    if ((u32)(a & 7u) + n > 8u) v |= *(const u64 *)(al + 8) << (64u - sh);                   // (then sh != 0)
    return v;
}

// the length of the string at p inside [p, p + rem), rem if no NUL lies there.  rem / 8 + 2 trips at most.
__device__ __forceinline__ u32 tn_strlen(const u8 *p, u32 rem)
{
    const u64 a = (u64)p, stop = a + rem;
    u64 at = a & ~7ull;
    u64 v = *(const u64 *)at | ((1ull << ((u32)(a & 7u) * 8u)) - 1ull);                       // bytes in front of p count as non-zero
    for (;;) {
        const u64 z = (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;              // its lowest set bit: the first zero byte
        if (z) {
            const u64 where = at + ((u32)__builtin_ctzll(z) >> 3);
            return where < stop ? (u32)(where - a) : rem;
        }
        at += 8;
        if (at >= stop) return rem;
        v = *(const u64 *)at;
    }
}

__device__ __forceinline__ void tn_put(u8 *dst, u64 lo, u32 hi, u32 n)    // n <= 10 bytes
{
#pragma unroll
    for (u32 i = 0; i < 8; i++) if (i < n) dst[i] = (u8)(lo >> (8 * i));
    if (n > 8) dst[8] = (u8)hi;
    if (n > 9) dst[9] = (u8)(hi >> 8);
}

// v in decimal as append_uint32_var (width == TN_NONE: no leading zeros, and no byte at all for 0, :279-315) or as
// append_uint32_fixed writes it in `width` <= 9 characters (:263-277: a value that needs more leaves the whole quotient
// in the first character, truncated to 8 bits).  Returns the length; the characters in *lo (0..7) and *hi (8, 9).
__device__ __forceinline__ u32 tn_decimal(u32 v, u32 width, u64 *lo, u32 *hi)
{
    unsigned __int128 s = 0;                   // all ten digits, the most significant in byte 0
    u32 r = v, ndig = 0, q = v;
#pragma unroll
    for (u32 j = 0; j < 10; j++) {
        if (j + 1 == width) q = r;             // v / 10^(width - 1)
        if (r) ndig = j + 1;
        s |= (unsigned __int128)(r % 10u + '0') << (8 * (9 - j));
        r /= 10u;
    }
    const u32 n = width == TN_NONE ? ndig : width;
    s >>= 8 * (10 - n);
    *lo = (u64)s;
    *hi = (u32)(s >> 64);
    if (width != TN_NONE && n) *lo = (*lo & ~0xffull) | ((q + '0') & 0xffu);
    return n;
}

// ---- one block ---------------------------------------------------------------------------------------------------
// the map of a block's columns in LDS: where the next unread byte of column id is, and how many are left.  Lane t only
// touches ids t << 4 | type, so the map is laid out type-major: the lanes of one access fall on consecutive banks.
#define TN_SLOT(cid) ((((cid) & 15u) << 7) | ((cid) >> 4))
struct TnMap {
    u64 *addr; u32 *rem;
    // n bytes (1 or 4) of column cid as a little-endian value; false if the column runs out
    __device__ __forceinline__ bool take(u32 cid, u32 n, u32 *v)
    {
        const u32 s = TN_SLOT(cid);
        if (rem[s] < n) return false;
        const u8 *p = (const u8 *)addr[s];
        *v = (u32)tn_load8(p, n) & (n == 4 ? 0xffffffffu : 0xffu);
        addr[s] = (u64)(p + n);
        rem[s] -= n;
        return true;
    }
};

// a lane's cursor in the type column of its position, with the 8 bytes around it held in registers
struct TnType {
    u64 addr, win, wbase; u32 rem;
    __device__ __forceinline__ void open(u64 a, u32 r) { addr = a; rem = r; win = 0; wbase = ~0ull; }
    __device__ __forceinline__ u32 peek()                                  // TN_END where the column is missing or exhausted
    {
        if (rem == 0) return TN_END;
        const u64 al = addr & ~7ull;
        if (al != wbase) { wbase = al; win = *(const u64 *)al; }
        return (u32)(win >> ((u32)(addr & 7u) * 8u)) & 0xffu;
    }
    __device__ __forceinline__ void consume() { if (rem) { addr++; rem--; } }
};

#define TN_ENTRY(type, val, aux) ((u64)(val) | ((u64)(aux) << 32) | ((u64)(type) << 60))
#define TN_E_TYPE(e) ((u32)((e) >> 60))
#define TN_E_VAL(e) ((u32)(e))
#define TN_E_AUX(e) ((u32)((e) >> 32) & 0x0fffffffu)

struct TnTok { u64 ent; u64 lo; const u8 *src; u32 hi, len; i32 err; };

// position t < e of a name: `ty` is its token (TN_REPLAY: the earlier name's entry as it is), pe the entry the earlier
// name has here - valid if t < pend -, alpha where the position's N_ALPHA column starts
__device__ __forceinline__ TnTok tn_token(u32 t, u32 ty, u64 pe, u32 pend, TnMap &m, const u8 *alpha, u32 alpha_size)
{
    TnTok k = {0, 0, nullptr, 0, 0, ST_OK};
    u32 v = 0, vl = 0;
    const u32 cid = t << 4;
    switch (ty) {
    case TN_REPLAY:
        k.ent = pe;
        break;
    case TN_CHAR:
        if (!m.take(cid | TN_CHAR, 1, &v)) k.err = ST_TRUNCATED;
        k.ent = TN_ENTRY(TN_CHAR, v, 0);
        break;
    case TN_ALPHA: {
        const u32 s = TN_SLOT(cid | TN_ALPHA), rem = m.rem[s];
        const u8 *p = (const u8 *)m.addr[s];
        const u32 n = rem ? tn_strlen(p, rem) : 0u;
        if (n >= rem) { k.err = ST_TRUNCATED; break; }                    // nothing left, or no NUL inside the column
        k.ent = TN_ENTRY(TN_ALPHA, n, alpha_size - rem);
        m.addr[s] = (u64)(p + n + 1);
        m.rem[s] = rem - n - 1;
        break;
    }
    case TN_DIGITS0:
        if (!m.take(cid | TN_DZLEN, 1, &vl) || !m.take(cid | TN_DIGITS0, 4, &v)) k.err = ST_TRUNCATED;
        else if (vl > 9) k.err = ST_SIZE;
        k.ent = TN_ENTRY(TN_DIGITS0, v, vl);
        break;
    case TN_DIGITS:
        if (!m.take(cid | TN_DIGITS, 4, &v)) k.err = ST_TRUNCATED;
        k.ent = TN_ENTRY(TN_DIGITS, v, 0);
        break;
    case TN_DDELTA:
    case TN_DDELTA0: {
        const u32 kind = ty == TN_DDELTA ? TN_DIGITS : TN_DIGITS0;
        if (t >= pend) k.err = ST_SIZE;
        else if (!m.take(cid | ty, 1, &v)) k.err = ST_TRUNCATED;
        else if (TN_E_TYPE(pe) != kind) k.err = ST_SIZE;
        k.ent = TN_ENTRY(kind, TN_E_VAL(pe) + v, TN_E_AUX(pe));
        break;
    }
    case TN_MATCH:
        if (t >= pend || TN_E_TYPE(pe) == TN_NOP) k.err = ST_SIZE;
        k.ent = pe;
        break;
    default:                                                              // TN_NOP
        k.ent = TN_ENTRY(TN_NOP, 0, 0);
        break;
    }
    if (k.err != ST_OK) return k;
    switch (TN_E_TYPE(k.ent)) {
    case TN_CHAR: k.lo = TN_E_VAL(k.ent) & 0xffu; k.len = 1; break;
    case TN_ALPHA: k.src = alpha + TN_E_AUX(k.ent); k.len = TN_E_VAL(k.ent); break;
    case TN_DIGITS:
    case TN_DIGITS0: k.len = tn_decimal(TN_E_VAL(k.ent), TN_E_TYPE(k.ent) == TN_DIGITS ? TN_NONE : TN_E_AUX(k.ent), &k.lo, &k.hi); break;
    default: break;
    }
    return k;
}

// a lane's bytes at dst: the immediate ones, or the string from its column in pieces of 8 (len / 8 + 1 trips; len is
// what tn_strlen found inside the column)
__device__ __forceinline__ void tn_write(u8 *dst, const TnTok &k)
{
    if (!k.src) { tn_put(dst, k.lo, k.hi, k.len); return; }
    for (u32 at = 0; at < k.len; at += 8) {
        const u32 n = k.len - at < 8u ? k.len - at : 8u;
        tn_put(dst + at, tn_load8(k.src + at, n), 0, n);
    }
}

// A name of up to TN_STAGE bytes is put together in LDS and leaves in whole-wave stores: one or two store instructions a
// name instead of up to ten predicated ones per pass, and far fewer stores for the next name's loads to wait behind
// (loads and stores share vmcnt).  The accesses are volatile - the compiler keeps their order and merges none - and the
// LDS runs one wave's instructions in order, so what one lane wrote another lane reads.
#define TN_STAGE 1024u
typedef LAS volatile u8 lvu8;

// a lane's immediate bytes at p, all ten of them whatever its length, the last first: a byte beyond the lane's length
// falls on a lower byte of a later lane, which is written after it, or behind the name, where the buffer has room
__device__ __forceinline__ void tn_stage_put(lvu8 *p, u64 lo, u32 hi)
{
    p[9] = (u8)(hi >> 8);
    p[8] = (u8)hi;
#pragma unroll
    for (int i = 7; i >= 0; i--) p[i] = (u8)(lo >> (8 * i));
}

// a lane's string from its column, in pieces of 8 (len / 8 + 1 trips; len is what tn_strlen found inside the column)
__device__ __forceinline__ void tn_stage_copy(lvu8 *p, const u8 *src, u32 len)
{
    for (u32 at = 0; at < len; at += 8) {
        const u32 n = len - at < 8u ? len - at : 8u;
        const u64 v = tn_load8(src + at, n);
#pragma unroll
        for (u32 i = 0; i < 8; i++) if (i < n) p[at + i] = (u8)(v >> (8 * i));
    }
}

__global__ __launch_bounds__(64) void k_tn_decode(TnIn in, TnWs w, TnOut o)
{
    __shared__ u8 stage[TN_STAGE + 16];
    __shared__ u64 c_addr[T3_MAX_IDS];
    __shared__ u32 c_rem[T3_MAX_IDS];
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const u32 count = w.count[b], npos = w.npos[b], last_start = in.last_start[b], nreads = in.nreads[b];
    const u64 start = o.off[b], hstart = w.hoff[b] * 16ull;
    i32 st = w.pre[b];                                                    // (wave-uniform, like every value it is set from)
    if (st == ST_OK && w.hoff[b + 1] * 16ull > w.hist_bytes) st = ST_UNSUPPORTED;
    if (st == ST_OK && o.off[b + 1] > o.capacity) st = ST_CAPACITY;
    u32 total = 0;
    if (st == ST_OK) {
        for (u32 i = lane; i < T3_MAX_IDS; i += 64) { c_addr[i] = 0; c_rem[i] = 0; }
        __syncthreads();
        const size_t base = (size_t)b * in.maxc;
        const u32 nc = in.ncol[b] < in.maxc ? in.ncol[b] : in.maxc;
        i32 bad = ST_OK;
        for (u32 c0 = 0; c0 < nc; c0 += 64) {                             // nc <= max_columns
            const u32 c = c0 + lane;
            const i32 id = c < nc ? in.col_id[base + c] : -1;
            if (id < 0) continue;
            const u32 cid = (u32)id & (T3_MAX_IDS - 1u), sz = in.col_size[base + c];
            const u64 off = in.col_off[base + c];
            const u32 lead = (id & R4X16_TOK3_TYPE_COLUMN) ? nreads : 0u;
            if (sz >= TN_MAX_COLUMN || lead >= TN_MAX_COLUMN) bad = ST_UNSUPPORTED;
            else if (off > in.col_capacity || sz > in.col_capacity - off || off < lead) { if (bad == ST_OK) bad = ST_SIZE; }
            else {
                c_addr[TN_SLOT(cid)] = (u64)(in.cols + off); c_rem[TN_SLOT(cid)] = sz;
                if (lead) { c_addr[TN_SLOT(cid & ~15u)] = (u64)(in.cols + off - lead); c_rem[TN_SLOT(cid & ~15u)] = lead; }
            }
        }
        __syncthreads();
        if (__ballot(bad == ST_UNSUPPORTED)) st = ST_UNSUPPORTED;
        else if (__ballot(bad != ST_OK)) st = ST_SIZE;
    }
    if (st == ST_OK && count) {
        TnMap m = {c_addr, c_rem};
        // position 0, the same in every lane: the type column and the two distance columns
        ByteSrc type0((const u8 *)c_addr[TN_SLOT(0u)]);
        u64 dup_addr = c_addr[TN_SLOT((u32)TN_DUP)], diff_addr = c_addr[TN_SLOT((u32)TN_DIFF)];
        u32 dup_rem = c_rem[TN_SLOT((u32)TN_DUP)], diff_rem = c_rem[TN_SLOT((u32)TN_DIFF)];
        // this lane's positions
        const u32 t0 = lane, t1 = lane + 64u;
        const bool has0 = t0 >= 1 && t0 < npos, has1 = t1 < npos;
        TnType ty0, ty1;
        ty0.open(has0 ? c_addr[TN_SLOT(t0 << 4)] : 0ull, has0 ? c_rem[TN_SLOT(t0 << 4)] : 0u);
        ty1.open(has1 ? c_addr[TN_SLOT(t1 << 4)] : 0ull, has1 ? c_rem[TN_SLOT(t1 << 4)] : 0u);
        const u8 *alpha0 = (const u8 *)c_addr[TN_SLOT(t0 << 4 | TN_ALPHA)], *alpha1 = (const u8 *)c_addr[TN_SLOT(t1 << 4 | TN_ALPHA)];
        const u32 asize0 = c_rem[TN_SLOT(t0 << 4 | TN_ALPHA)], asize1 = c_rem[TN_SLOT(t1 << 4 | TN_ALPHA)];
        u32x4 *rec = (u32x4 *)(w.hist + hstart);
        u64 *ent = (u64 *)(w.hist + hstart + 16ull * count);
        u8 *out = o.out + start;
        u32 *name_start = o.name_start ? o.name_start + (size_t)b * in.max_names : nullptr;
        u64 pe0 = 0, pe1 = 0;                                             // the entries of state `held`, positions below its end
        u32 held = TN_NONE, last_state = 0, last_e = 0;
        const u32 top = npos < (u32)T3_MAX_TOKENS ? npos : (u32)T3_MAX_TOKENS;
        for (u32 cnum = 0; cnum < count; cnum++) {                        // count <= max_names
            const u32 first = type0.at(cnum);
            if (first != TN_DUP && first != TN_DIFF) { st = ST_SIZE; break; }
            if ((first == TN_DUP ? dup_rem : diff_rem) < 4) { st = ST_TRUNCATED; break; }
            const u32 dist = (u32)tn_load8((const u8 *)(first == TN_DUP ? dup_addr : diff_addr), 4);
            if (first == TN_DUP) { dup_addr += 4; dup_rem -= 4; } else { diff_addr += 4; diff_rem -= 4; }
            if (dist > cnum || (first == TN_DUP && dist == 0)) { st = ST_SIZE; break; }
            // the earlier name's state and end position (dist == 0: none, :1061)
            u32 ps = TN_NONE, pend = 0;
            if (dist == 1) { ps = last_state; pend = last_e; }
            else if (dist) {
                u32x4 r = {0, 0, 0, 0};
                if (lane == 0) r = rec[cnum - dist];
                ps = (u32)__builtin_amdgcn_readfirstlane((int)r.z);
                pend = (u32)__builtin_amdgcn_readfirstlane((int)r.w);
            }
            if (dist && ps != held) {
                pe0 = t0 >= 1 && t0 < pend ? ent[(size_t)t0 * count + ps] : 0ull;
                pe1 = t1 < pend ? ent[(size_t)t1 * count + ps] : 0ull;
                held = ps;
            }
            // the end position
            u32 e = top;
            bool ended = first == TN_DUP;
            u32 tok0 = TN_REPLAY, tok1 = TN_REPLAY;
            if (first == TN_DUP) e = pend;
            else {
                tok0 = ty0.peek(); tok1 = TN_END;
                u64 ends = __ballot(has0 && !(tok0 < 16u && ((TN_TOKENS >> tok0) & 1u)));
                if (ends) { e = (u32)__builtin_ctzll(ends); ended = true; }
                else if (npos > 64) {
                    tok1 = ty1.peek();
                    ends = __ballot(has1 && !(tok1 < 16u && ((TN_TOKENS >> tok1) & 1u)));
                    if (ends) { e = 64u + (u32)__builtin_ctzll(ends); ended = true; }
                }
                if (t0 >= 1 && t0 <= e) ty0.consume();
                if (t1 <= e) ty1.consume();
            }
            // the tokens below e (a name without an end: all of them, for the first failure among them comes first)
            TnTok k0 = {0, 0, nullptr, 0, 0, ST_OK}, k1 = k0;
            if (t0 >= 1 && t0 < e) k0 = tn_token(t0, tok0, pe0, pend, m, alpha0, asize0);
            else if (t0 == e && ended) k0.len = 1;                        // the NUL
            u64 failed = __ballot(k0.err != ST_OK);
            if (failed) st = __shfl(k0.err, (int)__builtin_ctzll(failed));
            else if (e >= 64) {
                if (t1 < e) k1 = tn_token(t1, tok1, pe1, pend, m, alpha1, asize1);
                else if (t1 == e && ended) k1.len = 1;
                failed = __ballot(k1.err != ST_OK);
                if (failed) st = __shfl(k1.err, (int)__builtin_ctzll(failed));
            }
            if (st == ST_OK && !ended) st = ST_SIZE;
            if (st != ST_OK) break;
            // lengths -> places.  The sum is tested in two halves: 128 lengths below 2^28 overflow 32 bits.
            const u32 high = wave_sum(k0.len >> 8) + (e >= 64 ? wave_sum(k1.len >> 8) : 0u);
            if (high >= (1u << 23)) { st = ST_SIZE; break; }              // 2^31 bytes or more: beyond any last_start
            const u32 inc0 = wave_incl_scan(k0.len, lane);
            const u32 sum0 = (u32)__builtin_amdgcn_readlane((int)inc0, 63);
            u32 inc1 = 0, sum1 = 0;
            if (e >= 64) { inc1 = wave_incl_scan(k1.len, lane); sum1 = (u32)__builtin_amdgcn_readlane((int)inc1, 63); }
            const u32 len = sum0 + sum1;
            if ((u64)total + len > last_start) { st = ST_SIZE; break; }   // (also: nothing is written beyond the block's claim)
            const u32 at0 = inc0 - k0.len, at1 = sum0 + inc1 - k1.len;
            if (len <= TN_STAGE) {
                lvu8 *sp = (lvu8 *)stage;
                if (k0.len && !k0.src) tn_stage_put(sp + at0, k0.lo, k0.hi);
                if (k1.len && !k1.src) tn_stage_put(sp + at1, k1.lo, k1.hi);                  // (behind every byte of the first pass)
                if (k0.src) tn_stage_copy(sp + at0, k0.src, k0.len);                          // strings last: no stray byte falls on them
                if (k1.src) tn_stage_copy(sp + at1, k1.src, k1.len);
                __builtin_amdgcn_wave_barrier();
                for (u32 i = lane; i < len; i += 64) out[total + i] = sp[i];                 // len <= TN_STAGE
                __builtin_amdgcn_wave_barrier();
            } else {
                if (k0.len) tn_write(out + total + at0, k0);
                if (k1.len) tn_write(out + total + at1, k1);
            }
            const u32 state = first == TN_DUP ? ps : cnum;
            if (first == TN_DIFF) {
                if (t0 >= 1 && t0 < e) ent[(size_t)t0 * count + cnum] = k0.ent;
                if (t1 < e) ent[(size_t)t1 * count + cnum] = k1.ent;
                pe0 = t0 < e ? k0.ent : 0ull; pe1 = t1 < e ? k1.ent : 0ull;
                held = cnum;
            }
            if (lane == 0) {
                rec[cnum] = u32x4{total, len, state, e};
                if (name_start) name_start[cnum] = total;
            }
            last_state = state; last_e = e;
            total += len;
        }
    }
    if (st == ST_OK && total != last_start) st = ST_SIZE;
    if (lane == 0) {
        o.status[b] = st;
        o.out_size[b] = st == ST_OK ? total : 0u;
        o.nnames[b] = st == ST_OK ? count : 0u;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------
// the arenas a names call may fill: its own, the unpack's in front of it, and what the unpack's inner call reuses
#define TN_REUSE (A_BIT(A_WS) | A_BIT(A_XS) | A_BIT(A_T3) | A_BIT(A_TN))
// 16-byte units of history a block of max_names names and max_tokens positions takes at most
static u64 tn_units(u32 max_names, u32 max_tokens) { return (u64)max_names + ((u64)max_names * max_tokens * 8u + 15u) / 16u; }

// the stage over a prepared TnIn; `front`: bytes at the start of the context's names arena that the caller holds
static int tn_stage(rans4x16_hip_ctx *c, int nblk, const TnIn &in, TnOut o, u64 *d_out_off, u64 hist_bytes, size_t front, hipStream_t s)
{
    TnWs w;
    tn_carve(&w, c->at(A_TN), front, (size_t)nblk, (size_t)hist_bytes);
    o.off = d_out_off;
    hipLaunchKernelGGL(k_tn_claim, dim3((u32)nblk), dim3(64), 0, s, in, w);
    r4x16_launch_packed_scan(w.hclaim, w.hoff, 0, nblk, s);
    r4x16_launch_packed_scan(w.oclaim, d_out_off, 0, nblk, s);
    hipLaunchKernelGGL(k_tn_decode, dim3((u32)nblk), dim3(64), 0, s, in, w, o);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static bool tn_limits_ok(uint32_t max_names, uint32_t max_tokens)
{
    return max_names >= 1 && max_tokens >= 1 && max_tokens <= T3_MAX_TOKENS && tn_units(max_names, max_tokens) <= 0xffffffffull;
}

extern "C" int rans4x16_hip_tok3_names_dev(rans4x16_hip_ctx *c, int nblk,
                                           const unsigned char *d_cols, uint64_t col_capacity,
                                           const int32_t *d_col_id, const uint64_t *d_col_off, const uint32_t *d_col_size,
                                           const uint32_t *d_ncol, const uint32_t *d_last_start, const uint32_t *d_nreads,
                                           const int32_t *d_blk_status,
                                           unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                           uint32_t *d_out_size, uint32_t *d_nnames, int32_t *d_status, uint32_t *d_name_start,
                                           uint32_t max_columns, uint32_t max_names, uint32_t max_tokens, void *stream)
{
    if (!c) return -1;
    if (nblk < 0 || !d_out_off || max_columns < 1 || max_columns > T3_MAX_IDS || !tn_limits_ok(max_names, max_tokens) ||
        (nblk && ((!d_cols && col_capacity) || !d_col_id || !d_col_off || !d_col_size || !d_ncol || !d_last_start || !d_nreads ||
                  (!d_out && out_capacity) || !d_out_size || !d_nnames || !d_status))) {
        c->err = "tok3_names_dev: bad arguments";
        return -1;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nblk == 0) { HIPCHK(c, hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s)); return 0; }
    // the histories of the batch: what its limits allow, under half of what the context may hold; a block whose history
    // ends beyond that reports UNSUPPORTED
    const u64 full = (u64)nblk * tn_units(max_names, max_tokens) * 16ull;
    // (the tok3 arena counts as room although this call does not use it: the set of the one-call form below, kept)
    const u64 hist_bytes = std::min<u64>(full, r4x16_room(c, TN_REUSE) / 2);
    TnWs w;
    if (r4x16_ensure(c, A_TN, tn_carve(&w, nullptr, 0, (size_t)nblk, (size_t)hist_bytes), false) != 0) return -1;
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const TnIn in = {d_cols, col_capacity, d_col_id, d_col_off, d_col_size, d_ncol, d_last_start, d_nreads, d_blk_status,
                     max_columns, max_names, max_tokens};
    const TnOut o = {d_out, out_capacity, nullptr, d_out_size, d_nnames, d_status, d_name_start};
    if (tn_stage(c, nblk, in, o, d_out_off, hist_bytes, 0, s) != 0) return -1;
    return r4x16_ws_order_end(c, s);
}

// what the unpack writes for the stage, in front of the stage's own arrays
struct TnDir { u64 *off; u32 *size; i32 *status; u32 *ncol, *last_start, *nreads; i32 *col_id; u64 *col_off; u32 *col_size; u8 *cols; };

static size_t tn_dir_carve(TnDir *d, u8 *base, size_t nblk, size_t nitems, u64 col_bytes)
{
    Carver cv(base);
    d->off = cv.take<u64>(nblk + 1); d->size = cv.take<u32>(nblk); d->status = cv.take<i32>(nblk);
    d->ncol = cv.take<u32>(nblk); d->last_start = cv.take<u32>(nblk); d->nreads = cv.take<u32>(nblk);
    d->col_id = cv.take<i32>(nitems); d->col_off = cv.take<u64>(nitems); d->col_size = cv.take<u32>(nitems);
    d->cols = cv.take<u8>((size_t)col_bytes + 16);
    return cv.total();
}

// what rans4x16_hip_tok3_decode_names_dev takes of the names arena with these limits: the host-buffer calls plan their chunks with it
size_t r4x16_tok3_decode_names_need(int nblk, u32 max_columns, u32 max_names, u32 max_tokens, u64 col_bytes)
{
    TnDir d;
    TnWs w;
    const size_t front = tn_dir_carve(&d, nullptr, (size_t)nblk, (size_t)nblk * max_columns, col_bytes);
    return tn_carve(&w, nullptr, front, (size_t)nblk, (size_t)((u64)nblk * tn_units(max_names, max_tokens) * 16ull));
}

extern "C" int rans4x16_hip_tok3_decode_names_dev(rans4x16_hip_ctx *c, int nblk,
                                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                  unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                  uint32_t *d_out_size, uint32_t *d_nnames, int32_t *d_status, uint32_t *d_name_start,
                                                  uint32_t max_columns, uint32_t max_in_size, uint32_t max_col_size,
                                                  uint32_t max_names, uint32_t max_tokens, uint64_t total_col_size, void *stream)
{
    if (!c) return -1;
    if (nblk < 0 || !d_out_off || max_columns < 1 || max_columns > T3_MAX_IDS || !tn_limits_ok(max_names, max_tokens) ||
        (nblk && (!d_in || !d_in_off || !d_in_size || (!d_out && out_capacity) || !d_out_size || !d_nnames || !d_status))) {
        c->err = "tok3_decode_names_dev: bad arguments";
        return -1;
    }
    const u64 nitems = (u64)nblk * max_columns;
    if (nitems >= (u64)INT_MAX) { c->err = "tok3_decode_names_dev: nblk x max_columns does not fit an int"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nblk == 0) { HIPCHK(c, hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s)); return 0; }
    // the columns of the whole batch wait in an arena of the context until their names are written: what the caller
    // announced, or what the limits allow (a descriptor gives its column and at most one type column)
    const u64 col_bytes = total_col_size ? total_col_size : nitems * 2ull * max_col_size;
    const u64 hist_bytes = (u64)nblk * tn_units(max_names, max_tokens) * 16ull;
    TnDir d;
    TnWs w;
    const size_t front = tn_dir_carve(&d, nullptr, (size_t)nblk, (size_t)nitems, col_bytes);
    const size_t need = tn_carve(&w, nullptr, front, (size_t)nblk, (size_t)hist_bytes);
    if (need > r4x16_room(c, TN_REUSE) / 2) {
        c->err = "tok3_decode_names_dev: the columns and histories of this batch (" + std::to_string(need >> 20) +
                 " MiB) do not fit half of max_workspace_mb: split the batch";
        return -1;
    }
    if (r4x16_ensure(c, A_TN, need, false) != 0) return -1;
    tn_dir_carve(&d, c->at(A_TN), (size_t)nblk, (size_t)nitems, col_bytes);
    // (the unpack orders itself on the context's arenas, and so does the stage behind it)
    if (rans4x16_hip_tok3_unpack_dev(c, nblk, d_in, d_in_off, d_in_size, d.cols, col_bytes, d.off, d.size, d.status, d.ncol, d.last_start,
                                     d.nreads, d.col_id, d.col_off, d.col_size, max_columns, max_in_size, max_col_size, s) != 0) return -1;
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const TnIn in = {d.cols, col_bytes, d.col_id, d.col_off, d.col_size, d.ncol, d.last_start, d.nreads, d.status,
                     max_columns, max_names, max_tokens};
    const TnOut o = {d_out, out_capacity, nullptr, d_out_size, d_nnames, d_status, d_name_start};
    if (tn_stage(c, nblk, in, o, d_out_off, hist_bytes, front, s) != 0) return -1;
    return r4x16_ws_order_end(c, s);
}
