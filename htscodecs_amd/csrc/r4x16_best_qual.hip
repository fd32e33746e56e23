// r4x16_best_qual.hip - "try k methods, keep the smallest" across codecs for device-resident batches, and the decode of the
// mixed arena it leaves: include/rans4x16_hip.h part 2m (rANS 4x16 against arith_dynamic) and part 2n (quality blocks: the
// same two and fqzcomp_qual).  One implementation serves both parts: a flavour (BqFlavour) says which codec tags a call
// admits, which route it counts into and what it is called in err, and part 2m's calls are the ones that admit no
// fqzcomp tag and pass no records.
//
// Encode, per chunk of blocks, on the caller's stream and without a read-back:
//   rANS    : the rANS sub-list through rans4x16_hip_compress_best_dev into bound-sized slots of this call (the packed
//             calls' gathered route without its scan and gather, r4x16_packed.hip): k_best_pick leaves a winner a block
//   arith   : the arith sub-list through r4x16_ab_candidates (r4x16_arith_enc.hip): k_ab_pick leaves a winner a block
//   fqzcomp : the strategies through r4x16_fqb_candidates (r4x16_fqz_best.hip) - the statistics once per slice, store,
//             front and encode over the candidates, k_fqb_win: the winner's size is known, its stream lies in the
//             encoder's stage and is not assembled yet
//   k_bq_pick    : a thread a block compares up to three winners - size, then position in the caller's list - and writes
//                  the block's size, status and tagged method
//   k_pk_scan    : the winners' sizes to offsets, carried on from the chunk before
//   k_bq_gather  : a workgroup a block copies a rANS or arith winner from whichever arena holds it to its final place
//   k_fqb_back   : part 2l's back pass over the blocks fqzcomp won overall (take): varint, parameter bytes and body from
//                  the stage to the final place; a fqzcomp stream that lost is never assembled
// The codecs' results wait in arrays of this call; none writes the caller's arrays, so a sub-list of one codec gives what
// that codec's own best-packed call gives.  The packed arena (A_PS) holds this call's arrays, the rANS slots and the arith
// candidates' slots behind each other; the rANS call plans its candidate arena and workspace (A_XS, A_WS) under what the
// others leave of the ceiling (Keep on max_ws); the adaptive coders' arena (A_AR) holds the arith call's items while it
// runs and then the fqzcomp chunk - the arith winners lie in their slots by then, and the stream orders the two.  bq_fit
// plans a chunk by the sum of all of them.
//
// Decode: k_bq_claim reads every stream's size field (the varint at byte 1 - peek_one: rANS 4x16 and arith_dynamic keep it
// in the same place -, at byte 0 for fqzcomp), k_pk_scan lays the outputs out, k_bq_admit gives each slot decoder the
// lengths of its own codec's admitted blocks and 0 for every other, the admitted codecs' decoders run over the same entries
// into status and size arrays of their own, and k_bq_verdict takes each block's from its codec's (the pattern of
// k_t3_admit / k_t3_verdict, r4x16_tok3.hip).
//
// Loops: trip counts are launch arguments (k <= 32) or sizes the codecs' own kernels wrote for slots they sized.  Stores:
// k_bq_gather writes [off[i], off[i + 1]) of blocks that end inside the capacity, nothing else of the caller's arena;
// k_fqb_back the same for its blocks.  All stores are plain vector stores or vector atomics.
#include "r4x16_host.h"
#include "r4x16_best_any.h"
#include "r4x16_fqz_best.h"
#include "r4x16_best_qual.h"               // BQ_*, BqMethods, BqSplit, bq_split: the list's own refusals, host C++ alone

static_assert(BQ_MAX_FQZ == FQB_MAX_K && BQ_MAX_K == AB_MAX_K && X_STRIPE == 8, "the sub-lists' limits");
// where each of k_bq_pick's counts - part 2n's kinds, in their order - goes in the call's route array; -1: not counted
struct BqRouteMap { signed char at[R4X16_BEST_QUAL_KINDS]; };
// the five calls of a part, as err names them
struct BqNames { const char *enc_dev, *fit, *dec_dev, *enc_batch, *dec_batch; };
struct BqFlavour { unsigned admit; int route; u32 kinds; BqRouteMap map; BqNames who; };
static const BqFlavour BQ_ANY = {BQ_RANS | BQ_ARITH, R4X16_ROUTE_BEST_ANY, R4X16_BEST_ANY_KINDS,
                                 {{-1, R4X16_BEST_ANY_CHUNKS, R4X16_BEST_ANY_RANS, R4X16_BEST_ANY_ARITH, -1, R4X16_BEST_ANY_TIE, R4X16_BEST_ANY_FAILED, -1}},
                                 {"compress_best_any_packed_dev", "best_any_chunk_blocks", "uncompress_any_packed_dev", "compress_best_any_batch",
                                  "uncompress_any_batch"}};
static const BqFlavour BQ_QUAL = {BQ_RANS | BQ_ARITH | BQ_FQZ, R4X16_ROUTE_BEST_QUAL, R4X16_BEST_QUAL_KINDS, {{0, 1, 2, 3, 4, 5, 6, 7}},
                                  {"compress_best_qual_packed_dev", "best_qual_chunk_blocks", "uncompress_qual_packed_dev", "compress_best_qual_batch",
                                   "uncompress_qual_batch"}};
static_assert(R4X16_BEST_ANY_RANS == 0 && R4X16_BEST_ANY_ARITH == 1 && R4X16_BEST_ANY_TIE == 2 && R4X16_BEST_ANY_FAILED == 3 &&
              R4X16_BEST_ANY_CHUNKS == 4 && R4X16_BEST_QUAL_BLOCKS == 0 && R4X16_BEST_QUAL_UNDECIDED == 7, "the routes' kinds");

// (the fqzcomp arrays and take: nullptr where the call admits no fqzcomp tag)
struct BqWs {
    u32 *r_size, *a_size, *f_size; i32 *r_status, *a_status, *f_status, *r_chosen, *a_chosen, *f_chosen;   // [nb]: each codec's winner
    i32 *take;                                                                 // [nb]: 1 where fqzcomp won overall
    u8 *side;                                                                  // [nb]: BQ_* of the chunk's blocks
    u32 *route;                                                                // [the flavour's kinds]; nullptr in the kernels' copy: route_count is off
};

// where `word` of codec `tag` stands first in the list (a method that stands twice gives the same stream twice)
static __device__ __forceinline__ int bq_pos(const BqMethods &pm, int tag, int word)
{
    for (int j = 0; j < pm.k; j++)
        if ((pm.m[j] & R4X16_CODEC_MASK) == tag && (pm.m[j] & ~R4X16_CODEC_MASK) == word) return j;
    return pm.k;
}

// has_r / has_a / has_f: the list has methods of that codec (the arrays of a codec without one are not read).  slot_cap:
// the rANS slots' capacities, 0 for a block the slots were not sized for, whose CAPACITY is UNSUPPORTED (k_pk_gather's rule).
__global__ __launch_bounds__(256) void k_bq_pick(BqMethods pm, BqWs w, BqRouteMap map, const u32 *slot_cap, int has_r, int has_a, int has_f,
                                                 u32 *out_size, i32 *status, i32 *chosen, int base, int nb)
{
    const int lb = (int)(blockIdx.x * 256u + threadIdx.x);
    if (lb >= nb) return;
    const int g = base + lb;
    enum { R, A, F, SIDES };                                                           // BQ_RANS, BQ_ARITH, BQ_FQZ are 1 << these
    i32 st[SIDES] = {ST_UNSUPPORTED, ST_UNSUPPORTED, ST_UNSUPPORTED};
    u32 sz[SIDES] = {0, 0, 0};
    int pos[SIDES] = {pm.k, pm.k, pm.k}, word[SIDES] = {-1, -1, -1};
    if (has_r) {
        st[R] = w.r_status[lb]; sz[R] = w.r_size[lb];
        if (sz[R] == 0 && st[R] == ST_CAPACITY && slot_cap[lb] == 0) st[R] = ST_UNSUPPORTED;
        if (st[R] == ST_OK) { word[R] = w.r_chosen[lb]; pos[R] = bq_pos(pm, R4X16_CODEC_RANS4X16, word[R]); }
    }
    if (has_a) {
        st[A] = w.a_status[lb]; sz[A] = w.a_size[lb];
        if (st[A] == ST_OK) { word[A] = w.a_chosen[lb] | R4X16_CODEC_ARITH; pos[A] = bq_pos(pm, R4X16_CODEC_ARITH, w.a_chosen[lb]); }
    }
    bool undecided = false;
    if (has_f) {
        st[F] = w.f_status[lb]; sz[F] = w.f_size[lb];
        undecided = st[F] == R4X16_E_UNDECIDED;
        const int j = w.f_chosen[lb];
        if (st[F] == ST_OK && j >= 0 && j < FQB_MAX_K) { pos[F] = pm.fpos[j]; word[F] = pm.m[pos[F]]; }
        else if (st[F] == ST_OK) st[F] = ST_UNSUPPORTED;                                // (k_fqb_win names a winner wherever it says 0)
    }
    int win = -1;
    bool tie = false;
    if (!undecided)
        for (int s = 0; s < SIDES; s++) {
            if (st[s] != ST_OK) continue;
            if (win < 0) { win = s; continue; }
            // the reference loop's tie rule (tokenise_name3.c:1281-1284) over the whole list
            if (sz[s] == sz[win]) { tie = true; if (pos[s] < pos[win]) win = s; }
            else if (sz[s] < sz[win]) { win = s; tie = false; }
        }
    // a tie among losers is none: the smallest size is shared by two codecs' winners
    if (tie) {
        int shared = 0;
        for (int s = 0; s < SIDES; s++) shared += st[s] == ST_OK && sz[s] == sz[win];
        tie = shared > 1;
    }
    const int first_tag = pm.m[0] & R4X16_CODEC_MASK;
    const int first = first_tag == R4X16_CODEC_ARITH ? A : first_tag == R4X16_CODEC_FQZ ? F : R;
    w.side[lb] = (u8)(win < 0 ? BQ_NONE : 1 << win);
    if (w.take) w.take[lb] = win == F;
    out_size[g] = win >= 0 ? sz[win] : 0u;
    status[g] = undecided ? R4X16_E_UNDECIDED : win >= 0 ? ST_OK : st[first];
    if (chosen) chosen[g] = win >= 0 ? word[win] : -1;
    if (w.route) {
        auto count = [&](int kind) { if (map.at[kind] >= 0) atomicAdd(&w.route[map.at[kind]], 1u); };
        count(R4X16_BEST_QUAL_BLOCKS);
        count(undecided ? R4X16_BEST_QUAL_UNDECIDED : win == R ? R4X16_BEST_QUAL_RANS : win == A ? R4X16_BEST_QUAL_ARITH :
              win == F ? R4X16_BEST_QUAL_FQZ : R4X16_BEST_QUAL_FAILED);
        if (tie) count(R4X16_BEST_QUAL_TIE);
        if (lb == 0) count(R4X16_BEST_QUAL_CHUNKS);
    }
}

// block i's rANS or arith winner from its codec's slot to out + off[i], and the capacity rule (k_pk_gather / k_ab_gather
// over both arenas); a block fqzcomp won is the back pass's, with the same rule
__global__ __launch_bounds__(256) void k_bq_gather(PackedOut pk, const u8 *side, const u8 *r_slots, const u64 *r_slot_off, AbWs aw, int ka,
                                                   u32 *out_size, i32 *status, int base)
{
    const u32 tid = threadIdx.x;
    const int lb = (int)blockIdx.x, i = base + lb;
    const int sd = side[lb];
    const u32 sz = out_size[i];
    if (sz == 0 || (sd != BQ_RANS && sd != BQ_ARITH)) return;
    if (pk.off[i + 1] > pk.capacity) {
        if (tid == 0) { status[i] = ST_CAPACITY; out_size[i] = 0; }
        return;
    }
    const u8 *src = sd == BQ_ARITH ? aw.slots + aw.slot_off[(size_t)lb * ka + aw.win[lb]] : r_slots + r_slot_off[lb];
    group_copy<256>(pk.out + pk.off[i], src, sz, tid);
}

// ---- decode ----------------------------------------------------------------------------------------------------------
// [n] each, in the packed arena (in_f, sz_f, st_f: nullptr where the call admits no fqzcomp tag)
struct BqDecWs { u32 *claim, *in_r, *in_a, *in_f, *sz_r, *sz_a, *sz_f; i32 *pre, *st_r, *st_a, *st_f; };

// admit: the flavour's.  -1: the tag of a codec that is no candidate of this call
static __device__ __forceinline__ int bq_side(i32 method, unsigned admit)
{
    const int side = bq_tag_side(method & R4X16_CODEC_MASK);
    return method < 0 ? BQ_NONE : (side & admit) ? side : -1;
}

// what block i asks for (k_unpk_claim under a method array): its stored size - rans4x16_hip_fqz_peek_dev's rule for an
// fqzcomp block; for the others peek_one's, or the caller's for an X_NOSZ stream -, 0 and a status where it may not run
__global__ __launch_bounds__(256) void k_bq_claim(const u8 *in, const u64 *in_off, const u32 *in_size, const i32 *method,
                                                  const u32 *nosz_size, BqDecWs w, unsigned admit, int n, u32 max_in, u32 max_out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const int side = bq_side(method[i], admit);
    i32 st, f = -1;
    u32 claim = 0;
    if (side == BQ_NONE) st = ST_EMPTY;                                               // never written
    else if (side < 0) st = ST_UNSUPPORTED;                                           // a codec that is no candidate here
    else if (side == BQ_FQZ) {
        const u32 size = in_size[i];
        if (size == 0) st = ST_EMPTY;
        else if (size > max_in) st = ST_UNSUPPORTED;
        else {
            ByteSrc src(in + in_off[i]);
            const u32 used = var_get(src, 0u, size, &claim);
            st = (src.at(used - 1u) & 0x80u) ? ST_TRUNCATED : ST_OK;                  // the varint runs past the block
        }
        if (st == ST_OK && claim > max_out) st = ST_UNSUPPORTED;
    } else {
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
// block that is withdrawn or another codec's, so that nothing of them is read or written
__global__ __launch_bounds__(256) void k_bq_admit(const u32 *in_size, const i32 *method, BqDecWs w, unsigned admit, PackedOut pk, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 st = w.pre[i];
    if (st == ST_OK && pk.off[i + 1] > pk.capacity) { st = ST_CAPACITY; w.pre[i] = st; }
    const int side = bq_side(method[i], admit);
    w.in_r[i] = st == ST_OK && side == BQ_RANS ? in_size[i] : 0u;
    w.in_a[i] = st == ST_OK && side == BQ_ARITH ? in_size[i] : 0u;
    if (w.in_f) w.in_f[i] = st == ST_OK && side == BQ_FQZ ? in_size[i] : 0u;
}

__global__ __launch_bounds__(256) void k_bq_verdict(const i32 *method, BqDecWs w, unsigned admit, u32 *out_size, i32 *status, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    i32 st = w.pre[i];
    u32 sz = 0;
    if (st == ST_OK) {
        const int side = bq_side(method[i], admit);
        st = side == BQ_FQZ ? w.st_f[i] : side == BQ_ARITH ? w.st_a[i] : w.st_r[i];
        sz = side == BQ_FQZ ? w.sz_f[i] : side == BQ_ARITH ? w.sz_a[i] : w.sz_r[i];
    }
    status[i] = st;
    out_size[i] = st == ST_OK ? sz : 0u;
}

// ---- host --------------------------------------------------------------------------------------------------------------
// The call's flavour, the list split by codec (BqSplit), the fqzcomp and arith sides' plans, the rANS slots' stride.
struct BqPlan : BqSplit {
    const BqFlavour *f;
    FqbStrats fs;
    AbPlan ab;
    u64 stride, total;
    size_t chunk;
};
struct BqLayout { BqWs w; PackedSlots ps; AbWs aw; };

static int bq_bad(rans4x16_hip_ctx *c, const char *who)
{
    c->err = std::string(who) + ": bad arguments";
    return -1;
}

// the methods alone: what a call refuses before it asks for the device
static int bq_methods(rans4x16_hip_ctx *c, const BqFlavour &f, const char *who, int k, const int *methods, BqPlan *p)
{
    *p = BqPlan{};
    p->f = &f;
    if (const char *why = bq_split(k, methods, p, f.admit)) { c->err = std::string(who) + ": " + why; return -1; }
    if (p->kf && r4x16_fqb_strats(c, who, p->kf, p->sm, &p->fs) != 0) return -1;
    return p->ka ? r4x16_ab_methods(c, who, p->ka, p->am, &p->ab) : 0;
}

static u64 bq_chunk_total(const BqPlan &p, size_t nb, u32 max_in) { return std::min<u64>(p.total, (u64)nb * max_in); }

// the packed arena of a chunk of nb blocks: this call's arrays, the rANS slots, the arith candidates' slots
static size_t bq_carve(BqLayout *L, u8 *base, const BqPlan &p, size_t nb, u32 max_in)
{
    Carver cv(base);
    BqWs &w = L->w;
    w.r_size = cv.take<u32>(nb); w.a_size = cv.take<u32>(nb);
    w.r_status = cv.take<i32>(nb); w.a_status = cv.take<i32>(nb);
    w.r_chosen = cv.take<i32>(nb); w.a_chosen = cv.take<i32>(nb);
    if (p.f->admit & BQ_FQZ) { w.f_size = cv.take<u32>(nb); w.f_status = cv.take<i32>(nb); w.f_chosen = cv.take<i32>(nb); w.take = cv.take<i32>(nb); }
    w.side = cv.take<u8>(nb);
    w.route = cv.take<u32>(p.f->kinds);
    size_t at = cv.total();
    if (p.kr) at += r4x16_packed_carve(&L->ps, base ? base + at : nullptr, nb, nb, p.stride);
    if (p.ka) at += r4x16_ab_carve(&L->aw, base ? base + at : nullptr, p.ab, nb, max_in);
    return at;
}
// what the codecs' own calls take for such a chunk beside it
static size_t bq_rans_bytes(const BqPlan &p, size_t nb, u32 max_in)
{
    return p.kr ? r4x16_best_chunk_bytes(p.kr, p.rm, nb, max_in, bq_chunk_total(p, nb, max_in)) : 0;
}
static size_t bq_arith_bytes(const BqPlan &p, size_t nb, u32 max_in) { return p.ka ? r4x16_ab_inner_bytes(p.ab, nb, max_in) : 0; }
static size_t bq_fqz_bytes(rans4x16_hip_ctx *c, const BqPlan &p, size_t nb, u32 max_in, u32 max_rec)
{
    return p.kf ? r4x16_fqb_chunk_bytes(c, nb, (size_t)p.kf, max_in, max_rec, false) : 0;
}

// the rest of the plan, on the context's device: the codecs' arenas and workspaces of a chunk fit the room together
// (the arith items and the fqzcomp chunk share an arena one after the other; the plan counts both)
static void bq_fit(rans4x16_hip_ctx *c, int n, uint32_t max_in_size, uint32_t max_records, uint64_t total_in_size, BqPlan *p)
{
    p->total = total_in_size ? total_in_size : (u64)n * max_in_size;
    p->stride = 0;
    for (int j = 0; j < p->kr; j++) p->stride = std::max(p->stride, r4x16_packed_stride(max_in_size, p->rm[j], false));
    if (p->ka) r4x16_ab_sizes(n, max_in_size, total_in_size, &p->ab);
    p->chunk = 0;
    if (n == 0) return;
    BqLayout L = {};
    auto bytes = [&](size_t nb) {
        return bq_carve(&L, nullptr, *p, nb, max_in_size) + bq_rans_bytes(*p, nb, max_in_size) + bq_arith_bytes(*p, nb, max_in_size) +
               bq_fqz_bytes(c, *p, nb, max_in_size, max_records);
    };
    // (the arith candidates and the fqzcomp items of a chunk are counted in an int; the rANS call cuts a chunk further
    // where its items ask for it)
    size_t limit = p->ka ? (size_t)INT_MAX / (p->ab.per * p->ka) : SIZE_MAX;
    if (p->kf) limit = std::min(limit, r4x16_fqb_chunk_limit(p->kf, max_records));
    p->chunk = r4x16_fit_chunk((size_t)n, limit, r4x16_room(c, A_BIT(A_PS) | A_BIT(A_XS) | A_BIT(A_WS) | A_BIT(A_AR)), bytes);
}

static int bq_chunk_blocks(rans4x16_hip_ctx *c, const BqFlavour &f, int n, int k, const int *methods, uint32_t max_in_size,
                           uint32_t max_records, uint64_t total_in_size)
{
    if (!c) return -1;
    BqPlan p;
    if (bq_methods(c, f, f.who.fit, k, methods, &p) != 0) return -1;
    if (n < 0 || max_records >= 0x7fffffffu) return bq_bad(c, f.who.fit);
    HIPCHK(c, hipSetDevice(c->device));
    bq_fit(c, n, max_in_size, max_records, total_in_size, &p);
    return (int)p.chunk;
}

// the device encode call of either part: part 2m's passes no records, no vers and no d_len_out
static int bq_compress_dev(rans4x16_hip_ctx *c, const BqFlavour &f, int n, const unsigned char *d_in, const uint64_t *d_in_off,
                           const uint32_t *d_in_size, const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off,
                           const uint32_t *d_nrec, int vers, int k, const int *methods, unsigned char *d_out, uint64_t out_capacity,
                           uint64_t *d_out_off, uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                           uint32_t max_in_size, uint32_t max_records, uint64_t total_in_size, hipStream_t s)
{
    if (!c) return -1;
    BqPlan p;
    if (bq_methods(c, f, f.who.enc_dev, k, methods, &p) != 0) return -1;
    // the records are the fqzcomp sub-list's: a list without one does not look at them
    const bool recs_ok = !p.kf || n <= 0 ||
                         (d_rec_off && d_nrec && max_records < 0x7fffffffu && (max_records == 0 || (d_len && d_flags)));
    // (a: in, in_off, in_size for the fqzcomp stages, out_size and status for its back pass; the rANS and arith calls take
    // this call's own slots)
    BatchArgs a;
    PackedOut pk;
    const std::string bad = std::string(f.who.enc_dev) + ": bad arguments";
    const int go = r4x16_packed_call_args(c, bad.c_str(), recs_ok, &a, &pk, n, d_in, d_in_off, d_in_size, d_out, out_capacity, d_out_off,
                                          d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    bq_fit(c, n, max_in_size, max_records, total_in_size, &p);
    BqLayout L = {};
    auto grab = [&](size_t nb) {
        // the adaptive coders' arena holds the arith call's items, then the fqzcomp chunk: the larger of the two, so that
        // neither grows it while the other's results wait
        const size_t ar = std::max(bq_arith_bytes(p, nb, max_in_size), bq_fqz_bytes(c, p, nb, max_in_size, max_records));
        return r4x16_ensure(c, A_PS, bq_carve(&L, nullptr, p, nb, max_in_size), false) == 0 && (!p.kf || r4x16_ensure(c, A_AR, ar, false) == 0) ? 0 : -1;
    };
    return r4x16_chunk_walk(c, n, p.chunk, s, grab, [&](size_t base, int nb) {
        const size_t arena = bq_carve(&L, c->at(A_PS), p, (size_t)nb, max_in_size);
        const size_t r_bytes = bq_rans_bytes(p, (size_t)nb, max_in_size), a_bytes = bq_arith_bytes(p, (size_t)nb, max_in_size);
        const size_t f_bytes = bq_fqz_bytes(c, p, (size_t)nb, max_in_size, max_records);
        BqWs w = L.w;
        u32 *const d_route = w.route;
        if (r4x16_route_begin(c, &w.route, f.kinds, s) != 0) return -1;
        if (p.kr) {
            r4x16_launch_packed_slots_best(d_in_size + base, p.kr, p.rm, &L.ps, nb, (size_t)nb, max_in_size, s);
            // the rANS call: what is left of the ceiling beside this call's arena and the other codecs'
            const size_t held = arena + a_bytes + f_bytes;
            Keep<size_t> ceiling(c->max_ws, c->max_ws > held + ((size_t)1 << 20) ? c->max_ws - held : (size_t)1 << 20);
            Keep<bool> inner(c->in_packed, true);
            const u64 total = total_in_size ? bq_chunk_total(p, (size_t)nb, max_in_size) : 0;
            if (rans4x16_hip_compress_best_dev(c, nb, d_in, d_in_off + base, d_in_size + base, L.ps.slots, L.ps.slot_off, L.ps.slot_cap,
                                               w.r_size, w.r_status, p.kr, p.rm, w.r_chosen, max_in_size, total, s) != 0)
                return -1;
        }
        if (p.ka && r4x16_ab_candidates(c, p.ab, L.aw, arena + r_bytes + f_bytes, base, nb, d_in, d_in_off, d_in_size, w.a_size, w.a_status,
                                        w.a_chosen, max_in_size, s) != 0)
            return -1;
        FqbWork fw;
        if (p.kf && r4x16_fqb_candidates(c, a, d_len, d_flags, d_rec_off, d_nrec, vers, p.fs, nullptr, c->at(A_AR), (int)base, nb, w.f_size,
                                         w.f_status, w.f_chosen, 0, max_in_size, max_records, s, &fw) != 0)
            return -1;
        hipLaunchKernelGGL(k_bq_pick, dim3((u32)(nb + 255) / 256), dim3(256), 0, s, p.pm, w, f.map, (const u32 *)L.ps.slot_cap, p.kr, p.ka, p.kf,
                           d_out_size, d_status, d_chosen, (int)base, nb);
        r4x16_launch_packed_scan(d_out_size, d_out_off, (int)base, nb, s);
        if (p.kr || p.ka) {
            hipLaunchKernelGGL(k_bq_gather, dim3((u32)nb), dim3(256), 0, s, pk, (const u8 *)w.side, (const u8 *)L.ps.slots,
                               (const u64 *)L.ps.slot_off, L.aw, p.ka, d_out_size, d_status, (int)base);
            if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_RESULT][R4X16_RESULT_GATHERED] += nb;
        }
        if (p.kf && r4x16_fqb_back(c, a, &pk, fw, d_len_out, d_rec_off, d_nrec, (int)base, nb, w.take, s) != 0) return -1;
        return r4x16_route_end(c, f.route, d_route, f.kinds, s);
    });
}

// the device decode call of either part: part 2m's has no arrays for the lengths, and does not reach the fqzcomp decoder -
// no arena of its own is grown, its route is not counted, its limits are not looked at
static int bq_uncompress_dev(rans4x16_hip_ctx *c, const BqFlavour &f, int n, const unsigned char *d_in, const uint64_t *d_in_off,
                             const uint32_t *d_in_size, const int32_t *d_method, unsigned char *d_out, uint64_t out_capacity,
                             uint64_t *d_out_off, uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size, uint32_t *d_len,
                             const uint64_t *d_len_off, const uint32_t *d_len_cap, uint32_t *d_nrec, uint32_t max_in_size,
                             uint32_t max_out_size, hipStream_t s)
{
    BatchArgs a;
    PackedOut pk;
    const std::string bad = std::string(f.who.dec_dev) + ": bad arguments";
    const int go = r4x16_packed_call_args(c, bad.c_str(), (n == 0 || d_method) && (!d_len || (d_len_off && d_len_cap)), &a, &pk, n, d_in, d_in_off,
                                          d_in_size, d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s);
    if (go <= 0) return go;
    // the layout's own arrays: 32 bytes per block in the packed arena, 44 with fqzcomp's (ordered between streams like the
    // workspace)
    const bool fqz = f.admit & BQ_FQZ;
    if (r4x16_ensure(c, A_PS, (fqz ? 11 : 8) * align_up((size_t)n * 4, 256), false) != 0) return -1;
    Carver cv(c->at(A_PS));
    BqDecWs w = {};
    w.claim = cv.take<u32>(n); w.in_r = cv.take<u32>(n); w.in_a = cv.take<u32>(n); w.sz_r = cv.take<u32>(n); w.sz_a = cv.take<u32>(n);
    w.pre = cv.take<i32>(n); w.st_r = cv.take<i32>(n); w.st_a = cv.take<i32>(n);
    if (fqz) { w.in_f = cv.take<u32>(n); w.sz_f = cv.take<u32>(n); w.st_f = cv.take<i32>(n); }
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    const dim3 grid((n + 255) / 256), wg(256);
    hipLaunchKernelGGL(k_bq_claim, grid, wg, 0, s, d_in, d_in_off, d_in_size, d_method, d_nosz_size, w, f.admit, n, max_in_size, max_out_size);
    r4x16_launch_packed_scan(w.claim, pk.off, 0, n, s);
    hipLaunchKernelGGL(k_bq_admit, grid, wg, 0, s, d_in_size, d_method, w, f.admit, pk, n);
    // every admitted block ends inside the capacity, so the capacities of any decoder's blocks together do too
    const u64 total = std::max<u64>(std::min<u64>(pk.capacity, (u64)n * max_out_size), 1);
    // the sizing pass (no arena, capacity 0): only blocks that claim 0 bytes are admitted and nothing is written, but the
    // slot calls want a pointer - the packed arena's own
    unsigned char *out = pk.out ? pk.out : c->at(A_PS);
    if (rans4x16_hip_uncompress_dev_sized(c, n, d_in, d_in_off, w.in_r, out, pk.off, w.claim, w.sz_r, w.st_r, max_in_size, max_out_size, total, s) != 0)
        return -1;
    if (rans4x16_hip_arith_uncompress_dev(c, n, d_in, d_in_off, w.in_a, out, pk.off, w.claim, w.sz_a, w.st_a, max_in_size, max_out_size, total, s) != 0)
        return -1;
    if (fqz && rans4x16_hip_fqz_uncompress_dev(c, n, d_in, d_in_off, w.in_f, out, pk.off, w.claim, w.sz_f, w.st_f, d_len, d_len_off, d_len_cap, d_nrec,
                                               max_in_size, max_out_size, total, s) != 0)
        return -1;
    hipLaunchKernelGGL(k_bq_verdict, grid, wg, 0, s, d_method, w, f.admit, d_out_size, d_status, n);
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}

// ---- host buffers ------------------------------------------------------------------------------------------------------
// Both calls walk the batch in ranges of blocks whose inputs and outputs together stay under BQ_HOST_CHUNK_BYTES of staging
// (r4x16_cut_ranges): the staging layout with one item more than blocks (the offsets' n + 1 entries lie in its out_off
// array, the methods in its order array), the arrays' upload, the packed device call on the staged arenas, the verdict
// read, then the offsets, the methods and the dense results in one download each.  Where the call admits fqzcomp, behind
// the inputs go the records (compress: their places, counts, lengths and flags; uncompress: the places and capacities of
// the lengths), behind the outputs come the lengths (and, uncompress, the record counts).  Like r4x16_host_trip the copies
// go from and to pageable memory and are not pipelined; every range ends in a synchronise before its vectors go.
#define BQ_HOST_CHUNK_BYTES ((size_t)256 << 20)

// (nrec, len, flags, vers: the fqzcomp sub-list's - a list without one does not look at them)
struct BqHostArgs {
    const unsigned char *const *in; const unsigned int *in_size; const unsigned int *nrec; uint32_t *const *len, *const *flags;
    int vers; unsigned char **out; unsigned int *out_size; int k; const int *methods; int *chosen, *status;
};

// a block's result to the caller's buffer, or one the call allocates (made)
static void bq_deliver(const BqHostArgs &h, int g, const u8 *bytes, u32 size, std::vector<int> *made)
{
    if (h.out[g] && h.out_size[g] < size) h.status[g] = R4X16_E_CAPACITY;                        // the caller's buffer is too short
    if (h.status[g] == 0 && !h.out[g]) {
        if ((h.out[g] = (unsigned char *)malloc(size ? size : 1))) made->push_back(g); else h.status[g] = R4X16_E_UNSUPPORTED;
    }
    if (h.status[g] != 0) { h.out_size[g] = 0; return; }
    memcpy(h.out[g], bytes, size);
    h.out_size[g] = size;
}

// one range of the compress batch: blocks [at, at + nb).  made: the buffers this call allocated.  undecided: the blocks
// the device left so.  0 or -1.
static int bq_host_compress(rans4x16_hip_ctx *c, const BqPlan &p, int at, int nb, const BqHostArgs &h, const std::vector<u32> &bound,
                            std::vector<int> *made, std::vector<int> *undecided)
{
    hipStream_t s = c->stream;
    std::vector<u64> in_off(nb + 1, 0), off(nb + 1, 0);
    std::vector<u32> isz(nb + 1, 0), cap(nb + 1, 0), osz(nb + 1);
    std::vector<i32> ord(nb + 1, 0), st(nb + 1), won(nb + 1);
    size_t out_total = 0;
    u32 max_in = 0, max_rec = 0;
    u64 nrecs = 0;
    for (int i = 0; i < nb; i++) {
        isz[i] = h.in_size[at + i]; max_in = std::max(max_in, isz[i]); out_total += bound[at + i];
        if (p.kf) { max_rec = std::max(max_rec, h.nrec[at + i]); nrecs += h.nrec[at + i]; }
    }
    if (p.f->admit & BQ_FQZ) out_total = align_up(out_total, 256);    // (the lengths come behind the outputs)
    const size_t in_total = r4x16_stage_slots(isz.data(), (size_t)nb, 16, 256, in_off.data());
    const size_t N = (size_t)nb;
    std::vector<u8> tail(p.kf ? 12 * N + 8 * (size_t)nrecs : 0, 0);
    if (p.kf) {
        u64 *const t_rec_off = (u64 *)tail.data();
        u32 *const t_nrec = (u32 *)(t_rec_off + N), *const t_len = t_nrec + N, *const t_flags = t_len + nrecs;
        u64 at_rec = 0;
        for (int i = 0; i < nb; i++) {
            const u32 nr = h.nrec[at + i];
            t_rec_off[i] = at_rec; t_nrec[i] = nr;
            if (nr) { memcpy(t_len + at_rec, h.len[at + i], 4 * (size_t)nr); memcpy(t_flags + at_rec, h.flags[at + i], 4 * (size_t)nr); }
            at_rec += nr;
        }
    }
    StageLayout L;
    if (r4x16_stage_begin(c, &L, N + 1, in_total + tail.size() + 256, 0, out_total + 4 * (size_t)nrecs + 256, 0,
                          {in_off.data(), off.data(), isz.data(), cap.data(), ord.data()}, s) != 0)
        return -1;
    std::vector<u8> up(in_total + tail.size() + 1);
    for (int i = 0; i < nb; i++) if (isz[i]) memcpy(up.data() + in_off[i], h.in[at + i], isz[i]);
    if (!tail.empty()) memcpy(up.data() + in_total, tail.data(), tail.size());
    if (in_total + tail.size()) HIPCHK(c, hipMemcpyAsync(L.in, up.data(), in_total + tail.size(), hipMemcpyHostToDevice, s));
    const u64 *d_rec_off = p.kf ? (const u64 *)(L.in + in_total) : nullptr;                  // (in_total, out_total: multiples of 256)
    const u32 *d_nrec = p.kf ? (const u32 *)(d_rec_off + N) : nullptr, *d_len = p.kf ? d_nrec + N : nullptr, *d_flags = p.kf ? d_len + nrecs : nullptr;
    u32 *d_len_out = p.kf ? (u32 *)(L.out + out_total) : nullptr;
    if (bq_compress_dev(c, *p.f, nb, L.in, L.in_off, L.in_size, d_len, d_flags, d_rec_off, d_nrec, h.vers, h.k, h.methods, L.out, out_total,
                        L.out_off, L.osz, L.status, L.order, d_len_out, max_in, max_rec, in_total, s) != 0) {
        (void)hipStreamSynchronize(s);                 // (the upload reads `up`)
        return -1;
    }
    HIPCHK(c, hipMemcpyAsync(off.data(), L.out_off, (N + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(won.data(), L.order, N * 4, hipMemcpyDeviceToHost, s));
    if (r4x16_stage_verdicts(c, L, N, osz.data(), st.data(), s) != 0) return -1;
    std::vector<u8> down((size_t)off[nb] + 1);
    std::vector<u32> lens_out((size_t)nrecs + 1);
    if (off[nb]) HIPCHK(c, hipMemcpy(down.data(), L.out, (size_t)off[nb], hipMemcpyDeviceToHost));
    if (nrecs) HIPCHK(c, hipMemcpy(lens_out.data(), d_len_out, 4 * (size_t)nrecs, hipMemcpyDeviceToHost));
    u64 at_rec = 0;
    for (int i = 0; i < nb; i++) {
        const int g = at + i;
        const u32 nr = p.kf ? h.nrec[g] : 0;
        h.status[g] = st[i];
        if (h.chosen) h.chosen[g] = won[i];
        if (st[i] == R4X16_E_UNDECIDED) undecided->push_back(g);
        if (st[i] == 0) bq_deliver(h, g, down.data() + off[i], osz[i], made); else h.out_size[g] = 0;
        // fqzcomp won: the lengths as the fix-ups leave them, the flags as the reference leaves them (part 2l's batch)
        if (h.status[g] == 0 && (won[i] & R4X16_CODEC_MASK) == R4X16_CODEC_FQZ && nr) {
            memcpy(h.len[g], lens_out.data() + at_rec, 4 * (size_t)nr);
            for (u32 r = 0; r < nr; r++) h.flags[g][r] &= 0xffffu;
        }
        at_rec += nr;
    }
    return 0;
}

// The second trip: the blocks the device pick left undecided, those alone.  Their fqzcomp candidates are picked on the host
// and coded by rans4x16_hip_fqz_compress_batch under the parameter bytes, their rANS and arith methods - in list order -
// run through part 2m's batch, and the host compares the two results by k_bq_pick's rule.
static int bq_host_undecided(rans4x16_hip_ctx *c, const BqPlan &p, const BqHostArgs &h, const std::vector<int> &todo, const std::vector<u32> &caps,
                             std::vector<int> *made)
{
    const size_t U = todo.size(), K = (size_t)p.kf;
    if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_FQZ_PICK][R4X16_FQZ_PICK_HOST] += (long)U;
    // fqzcomp: item u * K + j is candidate j of block todo[u]
    std::vector<std::vector<u8>> par(U * K), fout(U * K);
    std::vector<std::vector<u32>> FL(U * K), FF(U * K);
    std::vector<int> fst(U * K, R4X16_E_UNSUPPORTED);
    std::vector<const unsigned char *> f_in, f_par;
    std::vector<unsigned char *> f_out;
    std::vector<unsigned int> f_isz, f_nrec, f_psz, f_osz;
    std::vector<uint32_t *> f_len, f_flags;
    std::vector<size_t> f_item;
    const unsigned int par_cap = rans4x16_hip_fqz_pick_cap();
    for (size_t u = 0; u < U; u++)
        for (size_t j = 0; j < K; j++) {
            const int g = todo[u];
            const size_t q = u * K + j;
            const u32 nr = h.nrec[g];
            FL[q].assign(h.len[g], h.len[g] + nr); FF[q].assign(h.flags[g], h.flags[g] + nr);
            FL[q].push_back(0); FF[q].push_back(0);                                          // (never empty: the pick wants arrays)
            par[q].resize(par_cap);
            unsigned int psz = 0;
            fst[q] = rans4x16_hip_fqz_pick_parameters(h.vers, p.sm[j], (int)nr, FL[q].data(), FF[q].data(), h.in[g], h.in_size[g], par[q].data(),
                                                      par_cap, &psz);
            if (fst[q] != 0) continue;
            fout[q].resize(rans4x16_hip_fqz_compress_cap(h.in_size[g], nr, psz));
            // the records the reference's encode loop reaches (a list that over-runs leaves the rest with 0 bytes)
            u32 reached = 0;
            for (u64 pos = 0; reached < nr && pos < h.in_size[g];) pos += FL[q][reached++];
            f_item.push_back(q);
            f_in.push_back(h.in[g]); f_isz.push_back(h.in_size[g]); f_nrec.push_back(reached); f_len.push_back(FL[q].data()); f_flags.push_back(FF[q].data());
            f_par.push_back(par[q].data()); f_psz.push_back(psz); f_out.push_back(fout[q].data()); f_osz.push_back((unsigned int)fout[q].size());
        }
    if (!f_item.empty()) {
        std::vector<int> st(f_item.size(), 0);
        if (rans4x16_hip_fqz_compress_batch(c, (int)f_item.size(), f_in.data(), f_isz.data(), f_nrec.data(), f_len.data(), f_flags.data(), h.vers, 0,
                                            f_par.data(), f_psz.data(), f_out.data(), f_osz.data(), st.data()) < 0)
            return -1;
        for (size_t e = 0; e < f_item.size(); e++) { fst[f_item[e]] = st[e]; fout[f_item[e]].resize(st[e] == 0 ? f_osz[e] : 0); }
    }
    // rANS and arith: their methods of the list, in list order
    std::vector<int> ram, ra_chosen(U, -1), ra_st(U, R4X16_E_UNSUPPORTED);
    std::vector<unsigned char *> ra_out(U, nullptr);
    std::vector<unsigned int> ra_osz(U, 0);
    for (int j = 0; j < p.pm.k; j++) if ((p.pm.m[j] & R4X16_CODEC_MASK) != R4X16_CODEC_FQZ) ram.push_back(p.pm.m[j]);
    auto release = [&] { for (auto *b : ra_out) free(b); };
    if (!ram.empty()) {
        std::vector<const unsigned char *> in(U);
        std::vector<unsigned int> isz(U);
        for (size_t u = 0; u < U; u++) { in[u] = h.in[todo[u]]; isz[u] = h.in_size[todo[u]]; }
        if (rans4x16_hip_compress_best_any_batch(c, (int)U, in.data(), isz.data(), ra_out.data(), ra_osz.data(), (int)ram.size(), ram.data(),
                                                 ra_chosen.data(), ra_st.data()) < 0)
            return -1;                                                                       // (it freed what it allocated)
    }
    const bool first_fqz = (p.pm.m[0] & R4X16_CODEC_MASK) == R4X16_CODEC_FQZ;
    for (size_t u = 0; u < U; u++) {
        const int g = todo[u];
        // the fqzcomp sub-list by k_fqb_win's rule
        int fw = -1, f_status = 0;
        bool no_room = false;
        for (size_t j = 0; j < K; j++) {
            const size_t q = u * K + j;
            if (fst[q] == R4X16_E_UNSUPPORTED) no_room = true;
            if (fst[q] == 0 && (fw < 0 || fout[q].size() < fout[u * K + fw].size())) fw = (int)j;
        }
        if (no_room) { fw = -1; f_status = R4X16_E_UNSUPPORTED; }
        else if (fw < 0) f_status = fst[u * K];
        // across: size, then the place in the caller's list
        int ra_pos = p.pm.k;
        if (ra_st[u] == 0) for (int j = p.pm.k - 1; j >= 0; j--) if (p.pm.m[j] == ra_chosen[u]) ra_pos = j;
        const bool ra_ok = !ram.empty() && ra_st[u] == 0, f_ok = fw >= 0;
        const size_t fsz = f_ok ? fout[u * K + fw].size() : 0;
        const bool take_f = f_ok && (!ra_ok || fsz < ra_osz[u] || (fsz == ra_osz[u] && p.pm.fpos[fw] < ra_pos));
        h.out_size[g] = caps[g];
        if (take_f) {
            h.status[g] = 0;
            bq_deliver(h, g, fout[u * K + fw].data(), (u32)fsz, made);
            if (h.chosen) h.chosen[g] = p.pm.m[p.pm.fpos[fw]];
            if (h.status[g] == 0 && h.nrec[g]) {
                memcpy(h.len[g], FL[u * K + fw].data(), 4 * (size_t)h.nrec[g]);
                for (u32 r = 0; r < h.nrec[g]; r++) h.flags[g][r] &= 0xffffu;
            }
        } else if (ra_ok) {
            h.status[g] = 0;
            bq_deliver(h, g, ra_out[u], ra_osz[u], made);
            if (h.chosen) h.chosen[g] = ra_chosen[u];
        } else {
            h.status[g] = first_fqz || ram.empty() ? f_status : ra_st[u];
            h.out_size[g] = 0;
            if (h.chosen) h.chosen[g] = -1;
        }
    }
    release();
    return 0;
}

// the compress batch of either part: part 2m's passes no records and no vers, and has no undecided trip
static int bq_compress_batch(rans4x16_hip_ctx *c, const BqFlavour &f, int n, const unsigned char *const *in, const unsigned int *in_size,
                             const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags, int vers, unsigned char **out,
                             unsigned int *out_size, int k, const int *methods, int *chosen, int *status)
{
    if (!c) return -1;
    BqPlan p;
    if (bq_methods(c, f, f.who.enc_batch, k, methods, &p) != 0) return -1;
    bool ok = n >= 0 && (n == 0 || (in && in_size && out && out_size && status && (!p.kf || (nrec && len && flags))));
    for (int i = 0; ok && i < n; i++) ok = (in[i] || !in_size[i]) && (!p.kf || (nrec[i] < 0x7fffffffu && (!nrec[i] || (len[i] && flags[i]))));
    if (!ok) return bq_bad(c, f.who.enc_batch);
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    // the room a block's winner may take: the largest bound over the list
    std::vector<u32> bound(n, 0), caps(out_size, out_size + n);
    std::vector<size_t> foot(n), ends(n);
    const unsigned int par_cap = rans4x16_hip_fqz_pick_cap();
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < p.kr; j++) bound[i] = std::max(bound[i], r4x16_compress_bound(in_size[i], p.rm[j]));
        for (int j = 0; j < p.ka; j++) bound[i] = std::max(bound[i], rans4x16_hip_arith_compress_cap(in_size[i], p.am[j]));
        if (p.kf) bound[i] = std::max(bound[i], rans4x16_hip_fqz_compress_cap(in_size[i], nrec[i], par_cap));
        foot[i] = (size_t)in_size[i] + bound[i] + 512 + (p.kf ? 12 * (size_t)nrec[i] + 12 : 0);
    }
    const size_t ranges = r4x16_cut_ranges(foot.data(), (size_t)n, BQ_HOST_CHUNK_BYTES, 0, ends.data());
    const BqHostArgs h{in, in_size, nrec, len, flags, vers, out, out_size, k, methods, chosen, status};
    std::vector<int> made, undecided;
    auto give_up = [&] {
        // the call failed: what it allocated, for earlier ranges too, is not left with the caller
        for (int g : made) { free(out[g]); out[g] = nullptr; out_size[g] = 0; }
        return -1;
    };
    for (size_t r = 0, at = 0; r < ranges; at = ends[r++])
        if (bq_host_compress(c, p, (int)at, (int)(ends[r] - at), h, bound, &made, &undecided) != 0) return give_up();
    if (!undecided.empty() && bq_host_undecided(c, p, h, undecided, caps, &made) != 0) return give_up();
    return (int)(n - std::count(status, status + n, 0));
}

// The size a stream stores, read as k_bq_claim reads it: fqzcomp's varint at byte 0, a rANS 4x16 or arith_dynamic
// stream's at byte 1 (peek_one's).  false where the stream has none of its own (empty, X_NOSZ without X_STRIPE) or the
// field is cut off - the device says what such a block is.
static bool bq_host_claim(const unsigned char *b, u32 size, bool fqz, u32 *claim)
{
    if (!fqz && (size == 0 || (!(b[0] & X_STRIPE) && (b[0] & X_NOSZ)))) return false;
    u32 acc = 0, q = fqz ? 0 : 1;
    unsigned char ch = 0x80;
    while ((ch & 0x80) && q < size) { ch = b[q++]; acc = (acc << 7) | (ch & 0x7f); }
    if (ch & 0x80) return false;
    *claim = acc;
    return true;
}

// one range of the uncompress batch.  lengths, nlengths, nrec: the quality calls' (nullptr otherwise); a call that admits
// no fqzcomp tag reads such a block's size field like any other's and lets the device say what the block is.
static int bq_host_uncompress(rans4x16_hip_ctx *c, const BqFlavour &f, int at, int nb, const unsigned char *const *in, const unsigned int *in_size,
                              const int *method, unsigned char *const *out, unsigned int *out_size, int *status, int *const *lengths,
                              const int *nlengths, unsigned int *nrec)
{
    hipStream_t s = c->stream;
    const size_t N = (size_t)nb;
    const bool quals = f.admit & BQ_FQZ;
    std::vector<u64> in_off(nb + 1, 0), off(nb + 1, 0);
    std::vector<u32> isz(nb + 1, 0), cap(nb + 1, 0), osz(nb + 1);
    std::vector<i32> ord(nb + 1, 0), st(nb + 1);
    std::vector<u8> short_of(nb, 0), places(quals ? 12 * N : 0, 0);   // places: [nb] offsets (8 bytes), [nb] capacities (4) of the lengths
    u64 *const len_off = (u64 *)places.data();
    u32 *const len_cap = quals ? (u32 *)(places.data() + 8 * N) : nullptr;
    size_t out_total = 0;
    u32 max_in = 0, max_out = 0, planes = 0, stripe_out = 0, max_sym = 1;
    u64 nlen = 0;
    for (int i = 0; i < nb; i++) {
        const unsigned char *b = in[at + i];
        isz[i] = in_size[at + i]; cap[i] = out_size[at + i]; ord[i] = method[at + i];
        const bool fqz = quals && ord[i] >= 0 && (ord[i] & R4X16_CODEC_MASK) == R4X16_CODEC_FQZ;
        // A block fails alone, as in rans4x16_hip_uncompress_batch where it has a slot of its own: the dense arena is laid out
        // by the sizes the streams claim, so a stream that stores more than its caller's buffer holds is withdrawn here - the
        // device sees a block that was never written - and every block that runs ends inside the sum of the capacities.
        u32 claim = 0;
        if (ord[i] >= 0 && bq_host_claim(b, isz[i], fqz, &claim) && claim > cap[i]) { short_of[i] = 1; ord[i] = -1; isz[i] = 0; continue; }
        max_in = std::max(max_in, isz[i]); max_out = std::max(max_out, cap[i]); out_total += cap[i];
        if (fqz) {
            // the model slots: sized for the largest max_sym of the range's streams, which the host walk knows
            u32 sym = 0;
            if (rans4x16_hip_fqz_scan(b, isz[i], nullptr, nullptr, nullptr, nullptr, nullptr, &sym) == 0) max_sym = std::max(max_sym, sym);
            if (lengths && lengths[at + i] && nlengths[at + i] > 0) { len_off[i] = nlen; len_cap[i] = (u32)nlengths[at + i]; nlen += len_cap[i]; }
            continue;
        }
        // an X_STRIPE stream of rANS 4x16 or arith: flags, the size's varint, N
        if (isz[i] < 3 || !(b[0] & X_STRIPE)) continue;
        u32 q = 1;
        while (q + 1 < isz[i] && (b[q] & 0x80)) q++;
        if (q + 1 >= isz[i]) continue;                                            // truncated: the decoder says so
        planes = std::max<u32>(planes, b[q + 1]);
        stripe_out = std::max(stripe_out, cap[i]);
    }
    if (quals) out_total = align_up(out_total, 256);                  // (the record counts come behind the outputs)
    const size_t in_total = r4x16_stage_slots(isz.data(), N, 16, 256, in_off.data());
    const size_t recs_words = quals ? N + (size_t)nlen : 0;                       // behind the outputs: [nb] record counts, the lengths
    StageLayout L;
    if (r4x16_stage_begin(c, &L, N + 1, in_total + places.size() + 256, 0, out_total + 4 * recs_words + 256, 0,
                          {in_off.data(), off.data(), isz.data(), cap.data(), ord.data()}, s) != 0)
        return -1;
    std::vector<u8> up(in_total + places.size() + 1);
    for (int i = 0; i < nb; i++) if (isz[i]) memcpy(up.data() + in_off[i], in[at + i], isz[i]);
    if (quals) memcpy(up.data() + in_total, places.data(), places.size());
    if (in_total + places.size()) HIPCHK(c, hipMemcpyAsync(L.in, up.data(), in_total + places.size(), hipMemcpyHostToDevice, s));
    // X_STRIPE blocks as after rans4x16_hip_set_dev_stripe_planes(ctx, most planes of the range, largest such block); the
    // caller's setting is put back
    StripeLimits stripes(c, (int)planes, stripe_out);
    Keep<int> limit(c->fqz_max_sym, quals ? (int)max_sym : c->fqz_max_sym);
    u32 *const d_nrec = quals ? (u32 *)(L.out + out_total) : nullptr;
    // L.cap: the callers' capacities, what an X_NOSZ stream decodes to
    if (bq_uncompress_dev(c, f, nb, L.in, L.in_off, L.in_size, L.order, L.out, out_total, L.out_off, L.osz, L.status, L.cap,
                          quals ? d_nrec + N : nullptr, quals ? (const u64 *)(L.in + in_total) : nullptr,
                          quals ? (const u32 *)(L.in + in_total + 8 * N) : nullptr, d_nrec, max_in, max_out, s) != 0) {
        (void)hipStreamSynchronize(s);                 // (the upload reads `up`)
        return -1;
    }
    HIPCHK(c, hipMemcpyAsync(off.data(), L.out_off, (N + 1) * 8, hipMemcpyDeviceToHost, s));
    if (r4x16_stage_verdicts(c, L, N, osz.data(), st.data(), s) != 0) return -1;
    const size_t got = (size_t)std::min<u64>(off[nb], out_total);
    std::vector<u8> down(got + 1);
    std::vector<u32> recs(recs_words + 1);
    if (got) HIPCHK(c, hipMemcpy(down.data(), L.out, got, hipMemcpyDeviceToHost));
    if (recs_words) HIPCHK(c, hipMemcpy(recs.data(), d_nrec, 4 * recs_words, hipMemcpyDeviceToHost));
    for (int i = 0; i < nb; i++) {
        const int g = at + i;
        status[g] = short_of[i] ? R4X16_E_CAPACITY : st[i];                       // the stream stores more than the caller has room for
        if (status[g] == 0 && out_size[g] < osz[i]) status[g] = R4X16_E_CAPACITY; // (an admitted block claims no more than its capacity)
        if (nrec) nrec[g] = status[g] == 0 ? recs[i] : 0;
        if (status[g] != 0) { out_size[g] = 0; continue; }
        if (osz[i]) memcpy(out[g], down.data() + off[i], osz[i]);
        out_size[g] = osz[i];
        // the reference's lengths[rec] = len for rec < nlengths: the entries behind the last record stay as they were
        if (quals && len_cap[i]) memcpy(lengths[g], recs.data() + N + len_off[i], 4 * (size_t)std::min(recs[i], len_cap[i]));
    }
    return 0;
}

static int bq_uncompress_batch(rans4x16_hip_ctx *c, const BqFlavour &f, int n, const unsigned char *const *in, const unsigned int *in_size,
                               const int *method, unsigned char *const *out, unsigned int *out_size, int *status, int *const *lengths,
                               const int *nlengths, unsigned int *nrec)
{
    if (!c) return -1;
    if (n < 0 || (n && (!in || !in_size || !method || !out || !out_size || !status)) || (lengths && !nlengths)) return bq_bad(c, f.who.dec_batch);
    if (n == 0) return 0;
    for (int i = 0; i < n; i++) if ((!in[i] && in_size[i]) || (!out[i] && out_size[i])) return bq_bad(c, f.who.dec_batch);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<size_t> foot(n), ends(n);
    for (int i = 0; i < n; i++) foot[i] = (size_t)in_size[i] + out_size[i] + 512 + (lengths && lengths[i] && nlengths[i] > 0 ? 4 * (size_t)nlengths[i] : 0);
    const size_t ranges = r4x16_cut_ranges(foot.data(), (size_t)n, BQ_HOST_CHUNK_BYTES, 0, ends.data());
    for (size_t r = 0, at = 0; r < ranges; at = ends[r++])
        if (bq_host_uncompress(c, f, (int)at, (int)(ends[r] - at), in, in_size, method, out, out_size, status, lengths, nlengths, nrec) != 0) return -1;
    return (int)(n - std::count(status, status + n, 0));
}

// ---- the public calls: part 2m's and part 2n's five, each the shared routine under its flavour ----------------------------
extern "C" int rans4x16_hip_best_any_chunk_blocks(rans4x16_hip_ctx *c, int n, int k, const int *methods, uint32_t max_in_size,
                                                  uint64_t total_in_size)
{
    return bq_chunk_blocks(c, BQ_ANY, n, k, methods, max_in_size, 0, total_in_size);
}

extern "C" int rans4x16_hip_best_qual_chunk_blocks(rans4x16_hip_ctx *c, int n, int k, const int *methods, uint32_t max_in_size,
                                                   uint32_t max_records, uint64_t total_in_size)
{
    return bq_chunk_blocks(c, BQ_QUAL, n, k, methods, max_in_size, max_records, total_in_size);
}

extern "C" int rans4x16_hip_compress_best_any_packed_dev(rans4x16_hip_ctx *c, int n,
                                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                         unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                         uint32_t *d_out_size, int32_t *d_status,
                                                         int k, const int *methods, int32_t *d_chosen,
                                                         uint32_t max_in_size, uint64_t total_in_size, void *stream)
{
    return bq_compress_dev(c, BQ_ANY, n, d_in, d_in_off, d_in_size, nullptr, nullptr, nullptr, nullptr, 0, k, methods, d_out, out_capacity, d_out_off,
                           d_out_size, d_status, d_chosen, nullptr, max_in_size, 0, total_in_size, (hipStream_t)stream);
}

extern "C" int rans4x16_hip_compress_best_qual_packed_dev(rans4x16_hip_ctx *c, int n,
                                                          const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                          const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off,
                                                          const uint32_t *d_nrec, int vers, int k, const int *methods,
                                                          unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                          uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                                          uint32_t max_in_size, uint32_t max_records, uint64_t total_in_size, void *stream)
{
    return bq_compress_dev(c, BQ_QUAL, n, d_in, d_in_off, d_in_size, d_len, d_flags, d_rec_off, d_nrec, vers, k, methods, d_out, out_capacity,
                           d_out_off, d_out_size, d_status, d_chosen, d_len_out, max_in_size, max_records, total_in_size, (hipStream_t)stream);
}

extern "C" int rans4x16_hip_uncompress_any_packed_dev(rans4x16_hip_ctx *c, int n,
                                                      const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                      const int32_t *d_method,
                                                      unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                      uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                                      uint32_t max_in_size, uint32_t max_out_size, void *stream)
{
    return bq_uncompress_dev(c, BQ_ANY, n, d_in, d_in_off, d_in_size, d_method, d_out, out_capacity, d_out_off, d_out_size, d_status, d_nosz_size,
                             nullptr, nullptr, nullptr, nullptr, max_in_size, max_out_size, (hipStream_t)stream);
}

extern "C" int rans4x16_hip_uncompress_qual_packed_dev(rans4x16_hip_ctx *c, int n,
                                                       const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                       const int32_t *d_method,
                                                       unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                       uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                                       uint32_t *d_len, const uint64_t *d_len_off, const uint32_t *d_len_cap, uint32_t *d_nrec,
                                                       uint32_t max_in_size, uint32_t max_out_size, void *stream)
{
    return bq_uncompress_dev(c, BQ_QUAL, n, d_in, d_in_off, d_in_size, d_method, d_out, out_capacity, d_out_off, d_out_size, d_status, d_nosz_size,
                             d_len, d_len_off, d_len_cap, d_nrec, max_in_size, max_out_size, (hipStream_t)stream);
}

extern "C" int rans4x16_hip_compress_best_any_batch(rans4x16_hip_ctx *c, int n,
                                                    const unsigned char *const *in, const unsigned int *in_size,
                                                    unsigned char **out, unsigned int *out_size,
                                                    int k, const int *methods, int *chosen, int *status)
{
    return bq_compress_batch(c, BQ_ANY, n, in, in_size, nullptr, nullptr, nullptr, 0, out, out_size, k, methods, chosen, status);
}

extern "C" int rans4x16_hip_compress_best_qual_batch(rans4x16_hip_ctx *c, int n,
                                                     const unsigned char *const *in, const unsigned int *in_size,
                                                     const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags, int vers,
                                                     unsigned char **out, unsigned int *out_size,
                                                     int k, const int *methods, int *chosen, int *status)
{
    return bq_compress_batch(c, BQ_QUAL, n, in, in_size, nrec, len, flags, vers, out, out_size, k, methods, chosen, status);
}

extern "C" int rans4x16_hip_uncompress_any_batch(rans4x16_hip_ctx *c, int n,
                                                 const unsigned char *const *in, const unsigned int *in_size, const int *method,
                                                 unsigned char *const *out, unsigned int *out_size, int *status)
{
    return bq_uncompress_batch(c, BQ_ANY, n, in, in_size, method, out, out_size, status, nullptr, nullptr, nullptr);
}

extern "C" int rans4x16_hip_uncompress_qual_batch(rans4x16_hip_ctx *c, int n,
                                                  const unsigned char *const *in, const unsigned int *in_size, const int *method,
                                                  unsigned char *const *out, unsigned int *out_size, int *status,
                                                  int *const *lengths, const int *nlengths, unsigned int *nrec)
{
    return bq_uncompress_batch(c, BQ_QUAL, n, in, in_size, method, out, out_size, status, lengths, nlengths, nrec);
}
