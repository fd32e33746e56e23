// r4x16_tok3_enc.hip - tok3 name encoding on the device (include/rans4x16_hip.h part 2e): what encode_names
// (htscodecs tokenise_name3.c:1334-1429) does before it compresses - build_trie / search_trie (:507-712), encode_name
// (:729-1013) and the drop rule (:1406-1429) - from a block of read names to its token columns.
//
//   k_te_claim    : a block's claim of the call's arenas (its bytes; 0 above max_in_size)
//   k_pk_scan     : claims -> where a block's slots lie (r4x16_packed.hip)
//   k_te_frame    : one wave per block, 64 bytes a step - the names (a name ends at any byte <= '\n'), nreads,
//                   last_start, the verdict of the limits, per name its start, length and what the prefix rule says of it
//                   (:632-670), and the set of depths at which some name of the block asks for an earlier name
//   k_te_tokenise : one wave per block, serial over names (a name is coded against an earlier one).  Per name:
//                   the earlier name - prefix hashes of the name by a wave scan; the lanes whose depth is in the block's
//                     set insert the name there into a hash table of the block (key: depth and prefix hash, value: the last
//                     name that passed), the lanes at the name's own length and at its prefix length keep what was there.
//                     Every name is inserted at every depth of the set, so a miss says that no earlier name has the prefix;
//                     a hit is compared byte for byte, and one that differs (two prefixes, one key), like a table that is
//                     full, falls to the exact search: the earlier names newest first, a lane each.  From a full table on
//                     the block stays there;
//                   its token boundaries, which depend on the name alone - classes of the bytes, ballots, and from those
//                     every lane's own verdict "a token starts here", 64 bytes a pass with three carried values;
//                   its tokens - lane t owns token position t (64..127: a second pass of the same wave, entered only by
//                     names that long): the earlier name's entry at t, match / delta / literal, the entry of its own, and
//                     what it appends to the columns of its position: a record per token (type, where in the type column,
//                     where in the value column), for the bytes are placed only when every column's size is known.
//   k_pk_scan     : column bytes per block -> d_cols_off;  k_te_admit : the capacity rule;  k_pk_scan : columns per
//                   block -> d_blk_first
//   k_te_place    : one wave per block - the sizes of its 2,048 possible columns -> where each starts, the directory
//   k_te_write    : one thread per token record and per name: the bytes.
//
// Arenas.  A name of len bytes has at most len tokens and one N_END, and len + 1 bytes of its block with its separator:
// token t of a name lies in slot (name's start) + t - 1 of its block, so the slots of a batch are its bytes - entry
// (8 bytes, r4x16_tok3_names.hip's format; a N_ALPHA entry holds where the string starts in the BLOCK), record, and two
// offsets, 20 bytes a slot.  Lane t alone writes and reads the entries of position t, lane 0 alone a name's state and
// end; the table (8 bytes a slot: key and name) is read and written with atomics only (they meet in L2); what k_te_frame
// wrote is a launch away.
//
// Loops: bytes of a block (size <= max_in_size, checked first), names (<= max_names, checked by k_te_frame), bytes of
// a name (<= max_name_len, likewise), a probe sequence (TE_PROBES), everything else is unrolled or a launch argument.
#include "r4x16_host.h"
#include "r4x16_tok3_walk.h"

enum { TE_ALPHA = 1, TE_CHAR = 2, TE_DIGITS0 = 3, TE_DZLEN = 4, TE_DUP = 5, TE_DIFF = 6, TE_DIGITS = 7, TE_DDELTA = 8,
       TE_DDELTA0 = 9, TE_MATCH = 10, TE_END = 12 };
#define TE_NONE 0xffffffffu
#define TE_MAX_NAME_LEN 16384u          // the depth set is a bitmap in LDS
#define TE_MAX_IN (65535u * 256u)       // a string's place in its block takes 24 bits, k_te_write's grid 65,535 rows of 256 slots
#define TE_WORDS (TE_MAX_NAME_LEN / 32u + 1u)
#define TE_PROBES 64u
#define TE_B 0x9e3779b97f4a7c15ull

#define TE_ENTRY(type, val, aux) ((u64)(val) | ((u64)(aux) << 32) | ((u64)(type) << 60))
#define TE_E_TYPE(e) ((u32)((e) >> 60))
#define TE_E_VAL(e) ((u32)(e))
#define TE_E_AUX(e) ((u32)((e) >> 32) & 0x0fffffffu)

struct TeIn { const u8 *in; const u64 *off; const u32 *size; u32 max_in, max_names, max_name_len, max_tokens, maxc; };
// per block [nblk] (boff, first64: one more); colsz: [nblk x T3_MAX_IDS] sizes, then starts; bitmap: [nblk x words];
// per name [nblk x max_names]; per slot [slots]; the tables [nblk x tslots]
struct TeWs {
    u32 *claim; u64 *boff; i32 *pre; u32 *csize, *ncol; u64 *first64; u32 *colsz, *bitmap;
    u32 *nstart, *nlen, *npfx, *nfix, *nstate, *nend, *nfirst, *nrank;
    u64 *ent; u32 *emit, *toff, *voff;
    u64 *keys;
    u64 slots; u32 tslots, words;
};
struct TeOut {
    u8 *cols; u64 capacity; u64 *cols_off; u32 *cols_size; i32 *status; u32 *blk_first; i32 *col_id; u64 *col_off; u32 *col_size;
    u32 *last_start, *nreads;
};

static size_t te_carve(TeWs *w, u8 *base, size_t at, size_t nblk, size_t max_names, u64 slots, u32 tslots, u32 words)
{
    Carver cv(base, at);
    const size_t names = nblk * max_names;
    w->claim = cv.take<u32>(nblk); w->boff = cv.take<u64>(nblk + 1); w->pre = cv.take<i32>(nblk);
    w->csize = cv.take<u32>(nblk); w->ncol = cv.take<u32>(nblk); w->first64 = cv.take<u64>(nblk + 1);
    w->colsz = cv.take<u32>(nblk * (size_t)T3_MAX_IDS); w->bitmap = cv.take<u32>(nblk * (size_t)words);
    w->nstart = cv.take<u32>(names); w->nlen = cv.take<u32>(names); w->npfx = cv.take<u32>(names); w->nfix = cv.take<u32>(names);
    w->nstate = cv.take<u32>(names); w->nend = cv.take<u32>(names); w->nfirst = cv.take<u32>(names); w->nrank = cv.take<u32>(names);
    w->ent = cv.take<u64>((size_t)slots); w->emit = cv.take<u32>((size_t)slots); w->toff = cv.take<u32>((size_t)slots);
    w->voff = cv.take<u32>((size_t)slots);
    w->keys = cv.take<u64>(nblk * (size_t)tslots);
    w->slots = slots; w->tslots = tslots; w->words = words;
    return cv.total();
}

__global__ __launch_bounds__(256) void k_te_claim(TeIn in, TeWs w, u32 nblk)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b < nblk) w.claim[b] = in.size[b] <= in.max_in ? in.size[b] : 0u;
}

__device__ __forceinline__ u32 te_wave_max(u32 v)
{
    for (int d = 32; d; d >>= 1) { const u32 o = (u32)__shfl_xor((int)v, d); v = o > v ? o : v; }
    return v;
}

// :632-670 over a name of len bytes: its prefix length (TE_NONE: none) and, for a fixed prefix, that length in *fix
__device__ __forceinline__ u32 te_prefix(const u8 *nm, u32 len, u32 *fix)
{
    *fix = 0;
    if (len == 0) return TE_NONE;
    const u32 at = nm[0] == '@' ? 1u : 0u, f = nm[0] == '>' ? 1u : 0u;
    const u8 *d = nm + at;
    const u32 l = len - at;
    if (l > 70 && d[f] == 'm' && d[7] == '_' && d[f + 14] == '_' && d[f + 61] == '/') return 60u;             // PacBio
    if (l == 17 && d[f + 5] == ':' && d[f + 11] == ':') { *fix = 6; return 6u; }                            // IonTorrent
    if (l > 37 && d[f + 8] == '-' && d[f + 13] == '-' && d[f + 18] == '-' && d[f + 23] == '-') {           // ONT
        const u32 a = d[f], z = d[f + 35];
        if (((a - '0') < 10u || (a - 'a') < 6u) && ((z - '0') < 10u || (z - 'a') < 6u)) { *fix = 37; return 37u; }
    }
    u32 i = 0, colons = 0;                                                // Illumina: lane:tile:x:y in front of the first blank
    while (i < len && nm[i] > ' ' && nm[i] < 0x80u) i++;                  // len <= max_name_len
    while (i > 0 && colons < 4) if (nm[--i] == ':') colons++;
    if (colons == 4) { *fix = i + 1; return i + 1; }
    return TE_NONE;
}

__global__ __launch_bounds__(64) void k_te_frame(TeIn in, TeWs w, TeOut o)
{
    __shared__ u32 bits[TE_WORDS];
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const u32 size = in.size[b];
    for (u32 i = lane; i < TE_WORDS; i += 64) bits[i] = 0;
    __syncthreads();
    i32 st = ST_OK;
    if (size > in.max_in || w.boff[b + 1] > w.slots) st = ST_UNSUPPORTED;    // larger than the call was sized for: not read
    u32 count = 0, cur = 0, maxlen = 0, first_high = TE_NONE;
    if (st == ST_OK) {
        const u8 *src = in.in + in.off[b];
        const size_t nb = (size_t)b * in.max_names;
        for (u32 i0 = 0; i0 < size; i0 += 64) {                           // size <= max_in_size
            const u32 i = i0 + lane;
            const u32 c = i < size ? src[i] : 0x40u;
            const bool term = c <= '\n';
            const u64 m = __ballot(term), hm = __ballot(c >= 0x80u);
            if (hm && first_high == TE_NONE) first_high = i0 + (u32)__builtin_ctzll(hm);
            if (term) {
                const u64 below = m & ((1ull << lane) - 1ull);
                const u32 idx = count + (u32)__builtin_popcountll(below);
                const u32 s = below ? i0 + 64u - (u32)__builtin_clzll(below) : cur;
                const u32 len = i - s;
                if (len > maxlen) maxlen = len;
                if (idx < in.max_names && len <= in.max_name_len) {       // (the others fail their block below)
                    u32 fix;
                    const u32 pfx = te_prefix(src + s, len, &fix);
                    w.nstart[nb + idx] = s; w.nlen[nb + idx] = len; w.npfx[nb + idx] = pfx; w.nfix[nb + idx] = fix;
                    if (len) atomicOr(&bits[len >> 5], 1u << (len & 31u));
                    if (pfx <= len) atomicOr(&bits[pfx >> 5], 1u << (pfx & 31u));
                }
            }
            if (m) { count += (u32)__builtin_popcountll(m); cur = i0 + 64u - (u32)__builtin_clzll(m); }
        }
        maxlen = te_wave_max(maxlen);
        if (count == 0) st = ST_SIZE;                                     // create_context fails
        else if (first_high < cur || count > in.max_names || maxlen > in.max_name_len) st = ST_UNSUPPORTED;
    }
    __syncthreads();
    for (u32 i = lane; i < w.words; i += 64) w.bitmap[(size_t)b * w.words + i] = bits[i];
    if (lane == 0) { w.pre[b] = st; o.last_start[b] = cur; o.nreads[b] = count; }
}

// ---- bytes ---------------------------------------------------------------------------------------------------
// n <= 8 bytes at p, by aligned 8-byte loads that hold at least one of them; bytes behind the n-th are unspecified
__device__ __forceinline__ u64 te_load8(const u8 *p, u32 n)
{
    const u64 a = (u64)p, al = a & ~7ull;
    const u32 sh = (u32)(a & 7u) * 8u;
    u64 v = *(const u64 *)al >> sh;
    if ((u32)(a & 7u) + n > 8u) v |= *(const u64 *)(al + 8) << (64u - sh);
    return v;
}

__device__ __forceinline__ bool te_equal(const u8 *a, const u8 *b, u32 n)      // n / 8 + 1 trips
{
    for (u32 i = 0; i < n; i += 8) {
        const u32 k = n - i < 8u ? n - i : 8u;
        const u64 mask = k == 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
        if ((te_load8(a + i, k) ^ te_load8(b + i, k)) & mask) return false;
    }
    return true;
}

__device__ __forceinline__ bool te_isalpha(u32 c) { return ((c | 0x20u) - 'a') < 26u; }
__device__ __forceinline__ bool te_isdigit(u32 c) { return (c - '0') < 10u; }

__device__ __forceinline__ u64 te_mix(u64 x)                              // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ u64 te_scan64(u64 v, u32 lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u64 o = __shfl_up(v, d); if (lane >= (u32)d) v += o; }
    return v;
}

// the first d bytes of names x and y (block offsets) are the same: by the wave, 64 bytes a trip (d <= max_name_len)
__device__ __forceinline__ bool te_wave_same(const u8 *blk, u32 x, u32 y, u32 d, u32 lane)
{
    for (u32 i0 = 0; i0 < d; i0 += 64) {
        const u32 i = i0 + lane;
        if (__ballot(i < d && blk[x + i] != blk[y + i])) return false;
    }
    return true;
}

// the exact search: the most recent name m < cnum of at least d bytes whose first d bytes are those of the name at
// `start`; cnum if there is none.  A lane per candidate, newest first.
__device__ u32 te_search(const u8 *blk, const u32 *nstart, const u32 *nlen, u32 cnum, u32 start, u32 d, u32 lane)
{
    for (u32 top = cnum; top > 0; top = top > 64u ? top - 64u : 0u) {     // <= max_names / 64 + 1 trips
        bool hit = false;
        if (lane < top) {
            const u32 m = top - 1u - lane;
            if (nlen[m] >= d) {
                const u8 *a = blk + nstart[m], *q = blk + start;
                hit = te_equal(a, q, d);
            }
        }
        const u64 hm = __ballot(hit);
        if (hm) return top - 1u - (u32)__builtin_ctzll(hm);
    }
    return cnum;
}

// what a lane keeps for one token position: bytes so far in its type column and in its value columns, :934's two
// counts, and whether a type behind the column's first is anything but N_MATCH
struct TePos { u32 toff, va, vc, vz, vd, vdd, vdz, dcount, icount; bool varied; };

__device__ __forceinline__ u32 te_type(TePos &p, u32 ty)
{
    if (p.toff && ty != TE_MATCH) p.varied = true;
    return p.toff++;
}

// the token [at, at + n) of the name, a fixed prefix or not, against the earlier name's entry pe (pty 0: there is none):
// its own entry; *emit = type | delta << 12, *voff = where its value goes in its column
__device__ __forceinline__ u64 te_token(const u8 *blk, u32 at, u32 n, bool fixedtok, u64 pe, bool pvalid, TePos &p, u32 *emit, u32 *voff)
{
    const u32 c0 = blk[at];
    const u32 pty = pvalid ? TE_E_TYPE(pe) : 0u;
    u32 ty, delta = 0;
    u64 ent;
    *voff = 0;
    if (fixedtok || (te_isalpha(c0) && n > 1)) {
        const bool same = pty == TE_ALPHA && TE_E_VAL(pe) == n && te_equal(blk + TE_E_AUX(pe), blk + at, n);
        ty = same ? TE_MATCH : TE_ALPHA;
        ent = TE_ENTRY(TE_ALPHA, n, at);
        if (!same) { *voff = p.va; p.va += n + 1; }
    } else if (te_isdigit(c0)) {
        const u64 lo = te_load8(blk + at, n < 8u ? n : 8u);
        const u32 hi = n > 8 ? blk[at + 8] : 0u;
        u32 v = 0;
#pragma unroll
        for (u32 j = 0; j < 9; j++) if (j < n) v = v * 10u + ((j < 8 ? (u32)(lo >> (8 * j)) & 0xffu : hi) - '0');
        const bool fixedw = pty == TE_DIGITS0 && TE_E_AUX(pe) == n;
        if (c0 == '0' || fixedw) {                                        // :842, and :916-919
            ty = TE_DIGITS0;
            ent = TE_ENTRY(TE_DIGITS0, v, n);
            if (fixedw) {
                const u32 d = v - TE_E_VAL(pe);
                if (d == 0) ty = TE_MATCH;
                else if (d < 256u) { ty = TE_DDELTA0; delta = d; }
            }
            if (ty == TE_DIGITS0) { *voff = p.vz; p.vz += 4; }
            else if (ty == TE_DDELTA0) { *voff = p.vdz; p.vdz += 1; }
        } else {
            ty = TE_DIGITS;
            ent = TE_ENTRY(TE_DIGITS, v, 0);
            if (pty == TE_DIGITS) {
                const u32 d = v - TE_E_VAL(pe);
                if (d == 0) ty = TE_MATCH;
                else if (d < 256u && 5u + p.dcount > p.icount) { ty = TE_DDELTA; delta = d; p.dcount++; }
                else p.icount++;
            }
            if (ty == TE_DIGITS) { *voff = p.vd; p.vd += 4; }
            else if (ty == TE_DDELTA) { *voff = p.vdd; p.vdd += 1; }
        }
    } else {
        ty = pty == TE_CHAR && TE_E_VAL(pe) == c0 ? TE_MATCH : TE_CHAR;
        ent = TE_ENTRY(TE_CHAR, c0, 0);
        if (ty == TE_CHAR) { *voff = p.vc; p.vc += 1; }
    }
    *emit = ty | (delta << 12);
    return ent;
}

// the sizes of a position's sixteen columns, the type column dropped where the reference drops it (:1406-1429)
__device__ __forceinline__ void te_sizes(const TePos &p, u32 *cs, u32 t, u32 *ncol, u32 *bytes)
{
    u32 sz[16] = {p.toff, p.va, p.vc, p.vz, p.vz / 4u, 0, 0, p.vd, p.vdd, p.vdz, 0, 0, 0, 0, 0, 0};
    const u32 others = p.va | p.vc | p.vz | p.vd | p.vdd | p.vdz;
    if (!p.varied && others) sz[0] = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) { cs[(t << 4) | k] = sz[k]; *ncol += sz[k] != 0; *bytes += sz[k]; }
}

__global__ __launch_bounds__(64) void k_te_tokenise(TeIn in, TeWs w, const u32 *nreads)
{
    __shared__ u32 bits[TE_WORDS];
    __shared__ u32 tokstart[T3_MAX_TOKENS + 2];
    const u32 b = blockIdx.x, lane = threadIdx.x;
    i32 st = w.pre[b];                                                    // (wave-uniform, like every value it is set from)
    u32 *cs = w.colsz + (size_t)b * T3_MAX_IDS;
    TePos p0 = {}, p1 = {};
    u32 ndup = 0, ndiff = 0;
    const u32 count = st == ST_OK ? nreads[b] : 0u;
    if (st == ST_OK) {
        for (u32 i = lane; i < TE_WORDS; i += 64) bits[i] = i < w.words ? w.bitmap[(size_t)b * w.words + i] : 0u;
        __syncthreads();
        const u8 *blk = in.in + in.off[b];
        const size_t nb = (size_t)b * in.max_names;
        const u64 sb = w.boff[b];
        const u32 *nstart = w.nstart + nb, *nlen = w.nlen + nb;
        u32 *nstate = w.nstate + nb, *nend = w.nend + nb;
        u64 *keys = w.keys + (size_t)b * w.tslots;
        const u32 tmask = w.tslots - 1u, probes = w.tslots < TE_PROBES ? w.tslots : TE_PROBES;
        // B^lane and B^64
        u64 pw_lane = 1, pw64 = 1;
#pragma unroll 1
        for (u32 i = 0; i < 64; i++) { if (i < lane) pw_lane *= TE_B; pw64 *= TE_B; }
        const u32 t0 = lane, t1 = lane + 64u;
        u64 pe0 = 0, pe1 = 0;                                             // the entries of state `held`
        u32 held = TE_NONE, last_state = 0, last_e = 0;
        bool slow = w.tslots < 2u;
        for (u32 cnum = 0; cnum < count; cnum++) {                        // count <= max_names
            const u32 start = nstart[cnum], len = nlen[cnum], pfx = w.npfx[nb + cnum], fix = w.nfix[nb + cnum];
            // ---- the earlier name
            u32 from = cnum, p3 = TE_NONE;                                // p3 TE_NONE: none (-1)
            const bool want3 = pfx <= len;
            if (len) {
                bool full = slow;
                u32 f_hit = TE_NONE, p_hit = TE_NONE;                     // what the table held at the two depths
                if (!slow) {
                    u64 carry = 0, pw = pw_lane;
                    for (u32 i0 = 0; i0 < len; i0 += 64) {                // len <= max_name_len
                        const u32 i = i0 + lane, d = i + 1u;
                        const u64 term = i < len ? (u64)(blk[start + i] + 1u) * pw : 0ull;
                        const u64 h = carry + te_scan64(term, lane);
                        carry = __shfl(h, 63);
                        pw *= pw64;
                        const bool act = d <= len && ((bits[d >> 5] >> (d & 31u)) & 1u);
                        u32 found = TE_NONE;
                        bool done = !act;
                        if (act) {
                            // a slot: 40 bits of key (never 0) over 24 bits of name.  An empty slot is claimed by the
                            // compare-and-swap itself; a slot of the same key gives its name and takes this one by a
                            // swap nobody waits for (the wave's atomics on one address run in the order it issued them)
                            const u64 mixed = te_mix(h + (u64)d * 0xd6e8feb86659fd93ull);
                            const u64 key = (mixed >> 24) | 1ull, mine = (key << 24) | cnum;
                            u32 at = (u32)mixed & tmask;
                            for (u32 pr = 0; pr < probes; pr++) {
                                const u64 old = atomicCAS((unsigned long long *)&keys[at], 0ull, (unsigned long long)mine);
                                if (old == 0ull) { done = true; break; }
                                if ((old >> 24) == key) {
                                    found = (u32)old & 0xffffffu;
                                    (void)atomicExch((unsigned long long *)&keys[at], (unsigned long long)mine);
                                    done = true;
                                    break;
                                }
                                at = (at + 1u) & tmask;
                            }
                        }
                        if (__ballot(!done)) full = true;
                        const u64 mf = __ballot(act && d == len), mp = __ballot(act && d == pfx && want3);
                        if (mf) f_hit = (u32)__shfl((int)found, (int)__builtin_ctzll(mf));
                        if (mp) p_hit = (u32)__shfl((int)found, (int)__builtin_ctzll(mp));
                    }
                }
                if (full) {
                    slow = true;
                    from = te_search(blk, nstart, nlen, cnum, start, len, lane);
                    if (want3 && from == cnum) p3 = te_search(blk, nstart, nlen, cnum, start, pfx, lane);
                } else {
                    // a hit is the most recent name with the same key: if its bytes are the name's, it is the answer
                    if (f_hit != TE_NONE) {
                        if (f_hit < cnum && nlen[f_hit] >= len && te_wave_same(blk, nstart[f_hit], start, len, lane)) from = f_hit;
                        else from = te_search(blk, nstart, nlen, cnum, start, len, lane);
                    }
                    if (want3 && from == cnum) {                          // (an exact hit decides alone, :711)
                        p3 = cnum;
                        if (p_hit != TE_NONE) {
                            if (p_hit < cnum && nlen[p_hit] >= pfx && te_wave_same(blk, nstart[p_hit], start, pfx, lane)) p3 = p_hit;
                            else p3 = te_search(blk, nstart, nlen, cnum, start, pfx, lane);
                        }
                    }
                }
            }
            const bool exact = from != cnum && len;
            u32 pnum = exact ? from : p3;
            if (pnum == TE_NONE) pnum = cnum ? cnum - 1u : 0u;            // :735
            const bool dup = exact && nlen[pnum] == len;                  // :745
            // the earlier name's state and end position
            u32 ps = TE_NONE, pend = 0;
            if (pnum < cnum) {
                if (pnum + 1u == cnum) { ps = last_state; pend = last_e; }
                else {
                    u32 r0 = 0, r1 = 0;
                    if (lane == 0) { r0 = nstate[pnum]; r1 = nend[pnum]; }
                    ps = (u32)__builtin_amdgcn_readfirstlane((int)r0);
                    pend = (u32)__builtin_amdgcn_readfirstlane((int)r1);
                }
            }
            if (lane == 0) {
                w.nfirst[nb + cnum] = ((cnum - pnum) << 1) | (dup ? 1u : 0u);
                w.nrank[nb + cnum] = dup ? ndup : ndiff;
            }
            if (dup) {
                ndup++;
                if (lane == 0) { nstate[cnum] = ps; nend[cnum] = pend; }
                last_state = ps; last_e = pend;
                continue;
            }
            ndiff++;
            if (ps != TE_NONE && ps != held) {
                const u64 ps_start = sb + nstart[ps];
                pe0 = t0 >= 1 && t0 < pend ? w.ent[ps_start + t0 - 1u] : 0ull;
                pe1 = t1 < pend ? w.ent[ps_start + t1 - 1u] : 0ull;
                held = ps;
            }
            // ---- token boundaries
            u32 ntok = 0;
            {
                bool ap_run = false, ap_seen = false, d_run = false;
                u32 d_cnt = 0;
                for (u32 i0 = 0; i0 < len; i0 += 64) {                    // len <= max_name_len
                    const u32 i = i0 + lane;
                    const bool inside = i < len && i >= fix;
                    const u32 c = i < len ? blk[start + i] : 0u;
                    const bool isA = inside && te_isalpha(c), isD = inside && te_isdigit(c);
                    const bool isP = inside && !isA && !isD && c > 32u && c < 127u;
                    const u64 A = __ballot(isA), D = __ballot(isD), AP = A | __ballot(isP);
                    const u64 below = (1ull << lane) - 1ull;
                    const u64 nb_ap = ~AP & below, nb_d = ~D & below;
                    const u32 rs = nb_ap ? 64u - (u32)__builtin_clzll(nb_ap) : 0u;
                    const bool seen = (((A & below) >> rs) != 0ull) || (nb_ap == 0ull && ap_run && ap_seen);
                    const u32 rd = nb_d ? 64u - (u32)__builtin_clzll(nb_d) : 0u;
                    const u32 offs = lane - rd + (nb_d == 0ull && d_run ? d_cnt : 0u);
                    bool begins;
                    if (isA || isP) begins = !seen;
                    else if (isD) begins = offs % 9u == 0u;
                    else begins = inside || (i == 0 && fix);
                    const u64 S = __ballot(begins);
                    const u32 t = 1u + ntok + (u32)__builtin_popcountll(S & below);
                    if (begins && t <= (u32)T3_MAX_TOKENS) tokstart[t] = i;
                    ntok += (u32)__builtin_popcountll(S);
                    ap_run = (AP >> 63) & 1ull;
                    ap_seen = __shfl((int)(seen || isA), 63) != 0;
                    d_run = (D >> 63) & 1ull;
                    d_cnt = ((u32)__shfl((int)offs, 63) + 1u) % 9u;
                }
            }
            const u32 e = ntok + 1u;                                      // the position of N_END
            if (e >= in.max_tokens) { st = ST_UNSUPPORTED; break; }
            if (lane == 0) tokstart[e] = len;
            __syncthreads();
            // ---- tokens
            const u64 slot0 = sb + start;
            if (t0 >= 1 && t0 <= e) {
                u32 emit = TE_END, voff = 0;
                u64 ent = 0;
                if (t0 < e) ent = te_token(blk, start + tokstart[t0], tokstart[t0 + 1] - tokstart[t0], t0 == 1 && fix, pe0, t0 < pend, p0, &emit, &voff);
                const u32 to = te_type(p0, emit & 15u);
                const u64 sl = slot0 + t0 - 1u;
                w.ent[sl] = ent; w.emit[sl] = emit | (t0 << 4); w.toff[sl] = to; w.voff[sl] = voff;
                pe0 = ent;
            }
            if (e >= 64 && t1 <= e) {
                u32 emit = TE_END, voff = 0;
                u64 ent = 0;
                if (t1 < e) ent = te_token(blk, start + tokstart[t1], tokstart[t1 + 1] - tokstart[t1], false, pe1, t1 < pend, p1, &emit, &voff);
                const u32 to = te_type(p1, emit & 15u);
                const u64 sl = slot0 + t1 - 1u;
                w.ent[sl] = ent; w.emit[sl] = emit | (t1 << 4); w.toff[sl] = to; w.voff[sl] = voff;
                pe1 = ent;
            }
            __syncthreads();                                              // (tokstart is written again by the next name)
            held = cnum;
            if (lane == 0) { nstate[cnum] = cnum; nend[cnum] = e; }
            last_state = cnum; last_e = e;
        }
    }
    // ---- the block's columns
    u32 ncol = 0, bytes = 0;
    if (st == ST_OK) {
        if (lane == 0) p0 = TePos{};
        te_sizes(p0, cs, lane, &ncol, &bytes);
        te_sizes(p1, cs, lane + 64u, &ncol, &bytes);
        if (lane == 0) {                                                  // position 0: the switch - dropped where it is one byte - and the two distances
            cs[0] = count > 1 ? count : 0u; cs[TE_DUP] = 4u * ndup; cs[TE_DIFF] = 4u * ndiff;
            ncol += (count > 1) + (ndup != 0) + (ndiff != 0);              // (its own position 64 is counted already)
            bytes += (count > 1 ? count : 0u) + 4u * (ndup + ndiff);
        }
        ncol = wave_sum(ncol);
        bytes = wave_sum(bytes);
        if (ncol > in.maxc) st = ST_UNSUPPORTED;
    }
    if (lane == 0) { w.pre[b] = st; w.csize[b] = st == ST_OK ? bytes : 0u; w.ncol[b] = st == ST_OK ? ncol : 0u; }
}

__global__ __launch_bounds__(256) void k_te_admit(TeWs w, TeOut o, u32 nblk)
{
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblk) return;
    i32 st = w.pre[b];
    if (st == ST_OK && o.cols_off[b + 1] > o.capacity) st = ST_CAPACITY;
    o.status[b] = st;
    o.cols_size[b] = st == ST_OK ? w.csize[b] : 0u;
    if (st != ST_OK) w.ncol[b] = 0;                                       // a refused block has no columns
}

// one wave per block: sizes -> starts (TE_NONE: no such column), and the block's part of the directory
__global__ __launch_bounds__(64) void k_te_place(TeWs w, TeOut o, u32 nblk)
{
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const u32 first = (u32)w.first64[b];
    if (lane == 0) {
        o.blk_first[b] = first;
        if (b == nblk - 1u) o.blk_first[nblk] = (u32)w.first64[nblk];
    }
    u32 *cs = w.colsz + (size_t)b * T3_MAX_IDS;
    if (o.status[b] != ST_OK) return;
    const u64 base = o.cols_off[b];
    u32 run = 0, rank = 0;
#pragma unroll 1
    for (u32 i0 = 0; i0 < (u32)T3_MAX_IDS; i0 += 64) {
        const u32 id = i0 + lane, sz = cs[id];
        const u32 inc = wave_incl_scan(sz, lane);
        const u64 m = __ballot(sz != 0);
        if (sz) {
            const size_t at = (size_t)first + rank + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            o.col_id[at] = (i32)id; o.col_off[at] = base + run + inc - sz; o.col_size[at] = sz;
        }
        cs[id] = sz ? run + inc - sz : TE_NONE;
        run += (u32)__builtin_amdgcn_readlane((int)inc, 63);
        rank += (u32)__builtin_popcountll(m);
    }
}

// the directory behind the batch's last column: entries that belong to no block (for a stage that runs over all of it)
__global__ __launch_bounds__(256) void k_te_idle(const u64 *count, TeOut o, u64 nitems)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nitems || i < *count) return;
    o.col_id[i] = -1; o.col_off[i] = 0; o.col_size[i] = 0;
}

__device__ __forceinline__ void te_put32(u8 *p, u32 v) { p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24); }

// a thread per slot of a block: the name of that index (position 0), and the token record of that slot
__global__ __launch_bounds__(256) void k_te_write(TeIn in, TeWs w, TeOut o)
{
    const u32 b = blockIdx.x, s = blockIdx.y * 256u + threadIdx.x;
    if (o.status[b] != ST_OK || s >= in.size[b]) return;
    const u32 *cb = w.colsz + (size_t)b * T3_MAX_IDS;
    u8 *dst = o.cols + o.cols_off[b];
    const u8 *blk = in.in + in.off[b];
    if (s < o.nreads[b]) {
        const size_t n = (size_t)b * in.max_names + s;
        const u32 f = w.nfirst[n], ty = (f & 1u) ? (u32)TE_DUP : (u32)TE_DIFF;
        if (cb[0] != TE_NONE) dst[cb[0] + s] = (u8)ty;
        te_put32(dst + cb[ty] + 4ull * w.nrank[n], f >> 1);
    }
    const u64 sl = w.boff[b] + s;
    const u32 e = w.emit[sl];
    if (!e) return;
    const u32 ty = e & 15u, t = (e >> 4) & 127u, vo = w.voff[sl];
    const u64 ent = w.ent[sl];
    if (cb[t << 4] != TE_NONE) dst[cb[t << 4] + w.toff[sl]] = (u8)ty;
    u8 *v = dst + cb[(t << 4) | (ty & 15u)] + vo;                          // (not used where the type has no column)
    switch (ty) {
    case TE_ALPHA: {
        const u32 n = TE_E_VAL(ent);
        const u8 *src = blk + TE_E_AUX(ent);
        for (u32 i = 0; i < n; i++) v[i] = src[i];                        // n <= max_name_len
        v[n] = 0;
        break;
    }
    case TE_CHAR: v[0] = (u8)TE_E_VAL(ent); break;
    case TE_DIGITS0:
        te_put32(v, TE_E_VAL(ent));
        dst[cb[(t << 4) | TE_DZLEN] + vo / 4u] = (u8)TE_E_AUX(ent);
        break;
    case TE_DIGITS: te_put32(v, TE_E_VAL(ent)); break;
    case TE_DDELTA:
    case TE_DDELTA0: v[0] = (u8)(e >> 12); break;
    default: break;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------
#define TE_REUSE (A_BIT(A_WS) | A_BIT(A_XS) | A_BIT(A_T3) | A_BIT(A_TN))

struct TeLimits { u32 max_in_size, max_names, max_name_len, max_tokens, max_columns; u64 total_in_size; u32 search_slots; };

static bool te_limits_ok(const TeLimits &l)
{
    return l.max_in_size >= 1 && l.max_in_size <= TE_MAX_IN && l.max_names >= 1 && l.max_names <= 0xffffffu && l.max_name_len <= TE_MAX_NAME_LEN &&
           l.max_tokens >= 1 && l.max_tokens <= T3_MAX_TOKENS && l.max_columns >= 1 && l.max_columns <= T3_MAX_IDS &&
           l.search_slots <= (1u << 28);
}

// slots of a block's table: what the caller says, or sixteen per name the call is sized for, at most two per byte
static u32 te_table_slots(const TeLimits &l)
{
    const u64 want = l.search_slots ? l.search_slots : std::min<u64>(16ull * l.max_names, 2ull * l.max_in_size);
    u32 slots = 1;
    while (slots < want && slots < (1u << 28)) slots <<= 1;
    return slots;
}

static size_t te_need(TeWs *w, u8 *base, size_t front, int nblk, const TeLimits &l)
{
    const u64 slots = l.total_in_size ? l.total_in_size : (u64)nblk * l.max_in_size;
    return te_carve(w, base, front, (size_t)nblk, l.max_names, slots, te_table_slots(l), l.max_name_len / 32u + 1u);
}

// what rans4x16_hip_tok3_tokenise_dev takes of the names arena with these limits: the host-buffer calls plan their chunks with it
size_t r4x16_tok3_tokenise_need(int nblk, u32 max_in_size, u32 max_names, u32 max_name_len, u64 total_in_size)
{
    TeWs w;
    const TeLimits l = {max_in_size, max_names, max_name_len, T3_MAX_TOKENS, T3_MAX_IDS, total_in_size, 0};
    return te_need(&w, nullptr, 0, nblk, l);
}

// the stage; `front`: bytes at the start of the context's names arena that the caller holds
static int te_stage(rans4x16_hip_ctx *c, int nblk, const TeIn &in, const TeOut &o, const TeLimits &l, size_t front, bool idle, hipStream_t s)
{
    TeWs w;
    te_need(&w, c->at(A_TN), front, nblk, l);
    const dim3 per_blk((u32)((nblk + 255) / 256));
    HIPCHK(c, hipMemsetAsync(w.emit, 0, (size_t)w.slots * sizeof(u32), s));
    HIPCHK(c, hipMemsetAsync(w.keys, 0, (size_t)nblk * w.tslots * sizeof(u64), s));
    hipLaunchKernelGGL(k_te_claim, per_blk, dim3(256), 0, s, in, w, (u32)nblk);
    r4x16_launch_packed_scan(w.claim, w.boff, 0, nblk, s);
    hipLaunchKernelGGL(k_te_frame, dim3((u32)nblk), dim3(64), 0, s, in, w, o);
    hipLaunchKernelGGL(k_te_tokenise, dim3((u32)nblk), dim3(64), 0, s, in, w, (const u32 *)o.nreads);
    r4x16_launch_packed_scan(w.csize, o.cols_off, 0, nblk, s);
    hipLaunchKernelGGL(k_te_admit, per_blk, dim3(256), 0, s, w, o, (u32)nblk);
    r4x16_launch_packed_scan(w.ncol, w.first64, 0, nblk, s);
    hipLaunchKernelGGL(k_te_place, dim3((u32)nblk), dim3(64), 0, s, w, o, (u32)nblk);
    hipLaunchKernelGGL(k_te_write, dim3((u32)nblk, (in.max_in + 255u) / 256u), dim3(256), 0, s, in, w, o);
    if (idle) {
        const u64 nitems = (u64)nblk * in.maxc;
        hipLaunchKernelGGL(k_te_idle, dim3((u32)((nitems + 255) / 256)), dim3(256), 0, s, (const u64 *)(w.first64 + nblk), o, nitems);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int rans4x16_hip_tok3_tokenise_dev(rans4x16_hip_ctx *c, int nblk,
                                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                              unsigned char *d_cols, uint64_t col_capacity, uint64_t *d_cols_off,
                                              uint32_t *d_cols_size, int32_t *d_status,
                                              uint32_t *d_blk_first, int32_t *d_col_id, uint64_t *d_col_off, uint32_t *d_col_size,
                                              uint32_t *d_last_start, uint32_t *d_nreads,
                                              uint32_t max_in_size, uint32_t max_names, uint32_t max_name_len,
                                              uint32_t max_tokens, uint32_t max_columns, uint64_t total_in_size,
                                              uint32_t search_slots, void *stream)
{
    if (!c) return -1;
    const TeLimits l = {max_in_size, max_names, max_name_len, max_tokens, max_columns, total_in_size, search_slots};
    if (nblk < 0 || !d_cols_off || !d_blk_first || !te_limits_ok(l) ||
        (nblk && (!d_in || !d_in_off || !d_in_size || (!d_cols && col_capacity) || !d_cols_size || !d_status || !d_col_id || !d_col_off ||
                  !d_col_size || !d_last_start || !d_nreads))) {
        c->err = "tok3_tokenise_dev: bad arguments";
        return -1;
    }
    if ((u64)nblk * max_columns >= (u64)INT_MAX) { c->err = "tok3_tokenise_dev: nblk x max_columns does not fit an int"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nblk == 0) {
        HIPCHK(c, hipMemsetAsync(d_cols_off, 0, sizeof(uint64_t), s));
        HIPCHK(c, hipMemsetAsync(d_blk_first, 0, sizeof(uint32_t), s));
        return 0;
    }
    TeWs w;
    const size_t need = te_need(&w, nullptr, 0, nblk, l);
    if (need > r4x16_room(c, TE_REUSE) / 2) {
        c->err = "tok3_tokenise_dev: the names, token records and tables of this batch (" + std::to_string(need >> 20) +
                 " MiB) do not fit half of max_workspace_mb: split the batch";
        return -1;
    }
    if (r4x16_ensure(c, A_TN, need, false) != 0) return -1;
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const TeIn in = {d_in, d_in_off, d_in_size, max_in_size, max_names, max_name_len, max_tokens, max_columns};
    const TeOut o = {d_cols, col_capacity, d_cols_off, d_cols_size, d_status, d_blk_first, d_col_id, d_col_off, d_col_size,
                     d_last_start, d_nreads};
    if (te_stage(c, nblk, in, o, l, 0, false, s) != 0) return -1;
    return r4x16_ws_order_end(c, s);
}

// what the tokeniser writes for the pack, in front of its own arrays in the context's names arena
struct TeDir { u64 *cols_off; u32 *cols_size; i32 *status; u32 *blk_first, *last_start, *nreads; i32 *col_id; u64 *col_off; u32 *col_size; u8 *cols; };

static size_t te_dir_carve(TeDir *d, u8 *base, size_t nblk, size_t nitems, u64 col_bytes)
{
    Carver cv(base);
    d->cols_off = cv.take<u64>(nblk + 1); d->cols_size = cv.take<u32>(nblk); d->status = cv.take<i32>(nblk);
    d->blk_first = cv.take<u32>(nblk + 1); d->last_start = cv.take<u32>(nblk); d->nreads = cv.take<u32>(nblk);
    d->col_id = cv.take<i32>(nitems); d->col_off = cv.take<u64>(nitems); d->col_size = cv.take<u32>(nitems);
    d->cols = cv.take<u8>((size_t)col_bytes + 16);
    return cv.total();
}

__global__ __launch_bounds__(256) void k_te_first_out(const u32 *first, u32 *out, u32 n)
{
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = first[i];
}

extern "C" int rans4x16_hip_tok3_encode_names_dev(rans4x16_hip_ctx *c, int nblk,
                                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                  unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                  uint32_t *d_out_size, int32_t *d_status,
                                                  int k, const int *methods, int32_t *d_chosen, uint32_t *d_blk_first,
                                                  uint32_t max_in_size, uint32_t max_names, uint32_t max_name_len,
                                                  uint32_t max_tokens, uint32_t max_columns, uint32_t max_col_size,
                                                  uint64_t total_in_size, uint32_t search_slots, void *stream)
{
    if (!c) return -1;
    const TeLimits l = {max_in_size, max_names, max_name_len, max_tokens, max_columns, total_in_size, search_slots};
    if (nblk < 0 || !d_out_off || !te_limits_ok(l) || k < 1 || k > 32 || !methods ||
        (nblk && (!d_in || !d_in_off || !d_in_size || (!d_out && out_capacity) || !d_out_size || !d_status))) {
        c->err = "tok3_encode_names_dev: bad arguments";
        return -1;
    }
    const u64 nitems = (u64)nblk * max_columns;
    if (nitems >= (u64)INT_MAX) { c->err = "tok3_encode_names_dev: nblk x max_columns does not fit an int"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nblk == 0) {
        HIPCHK(c, hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s));
        if (d_blk_first) HIPCHK(c, hipMemsetAsync(d_blk_first, 0, sizeof(uint32_t), s));
        return 0;
    }
    // the columns of the whole batch wait in an arena of the context until they are packed: six bytes per byte of names
    // at most (include/rans4x16_hip.h part 2e); a column is a value per name at most, so four bytes per byte of its block
    const u64 in_bytes = total_in_size ? total_in_size : (u64)nblk * max_in_size;
    const u64 col_bytes = 6ull * in_bytes;
    const u32 max_col = max_col_size ? max_col_size : (u32)std::min<u64>(4ull * max_in_size, 0xffffffffull);
    TeDir d;
    TeWs w;
    const size_t front = te_dir_carve(&d, nullptr, (size_t)nblk, (size_t)nitems, col_bytes);
    const size_t need = te_need(&w, nullptr, front, nblk, l);
    if (need > r4x16_room(c, TE_REUSE) / 2) {
        c->err = "tok3_encode_names_dev: the columns, token records and tables of this batch (" + std::to_string(need >> 20) +
                 " MiB) do not fit half of max_workspace_mb: split the batch";
        return -1;
    }
    if (r4x16_ensure(c, A_TN, need, false) != 0) return -1;
    te_dir_carve(&d, c->at(A_TN), (size_t)nblk, (size_t)nitems, col_bytes);
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const TeIn in = {d_in, d_in_off, d_in_size, max_in_size, max_names, max_name_len, max_tokens, max_columns};
    const TeOut o = {d.cols, col_bytes, d.cols_off, d.cols_size, d.status, d.blk_first, d.col_id, d.col_off, d.col_size, d.last_start, d.nreads};
    if (te_stage(c, nblk, in, o, l, front, true, s) != 0) return -1;
    if (d_blk_first) hipLaunchKernelGGL(k_te_first_out, dim3((u32)(nblk / 256 + 1)), dim3(256), 0, s, (const u32 *)d.blk_first, d_blk_first, (u32)nblk + 1u);
    if (r4x16_ws_order_end(c, s) != 0) return -1;
    // (the pack orders itself on the context's arenas; its own are others than this one)
    return r4x16_tok3_pack_run(c, nblk, (int)nitems, d.blk_first, d.cols, d.col_off, d.col_size, d.col_id, d.last_start, d.nreads,
                               d_out, out_capacity, d_out_off, d_out_size, d_status, k, methods, d_chosen, max_col, col_bytes,
                               d.status, true, s);
}
