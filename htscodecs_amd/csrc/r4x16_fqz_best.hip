// r4x16_fqz_best.hip - best of several strategies for fqzcomp_qual encoding on the device: include/rans4x16_hip.h part 2l.
// A caller of the reference offers the rows of strat_opts (fqzcomp_qual.c:199-206) as so many methods and keeps the
// smallest block; here that loop is one enqueue.  Block lb of a chunk of nb blocks under k strategies is k items,
// candidate j being item j * nb + lb: an encode wave strides over the items by the number of model slots, and with the
// candidates of one strategy side by side it meets every strategy in turn - the strategies' streams take different
// times, and a wave that coded one strategy alone would set the pace of the chunk.  Stages:
//   the pick's statistics (r4x16_fqz_pick.hip: k_fqp_lens .. k_fqp_sums) once per SLICE: the fix-ups, first_len, the
//                 duplicates and the quality mask do not depend on the strategy; the average-quality bins are computed
//                 where any candidate asks for them, and the sums a candidate reads are marginals over those bins of the
//                 same integer histogram, summed in the same order
//   k_fqb_store   one wave per item: the decisions, the flags' largest selector and the store of r4x16_fqz_pick_dec.h -
//                 the item's parameter bytes and flags into the hand-over, its slot arrays; the lengths stay the slice's
//   the encoder's front and encode kernels (r4x16_fqz_enc.hip) once over the chunk's nb * k items, every item with room
//                 for its body at the bound: no candidate is cut short by the caller's capacity
//   k_fqb_win     one thread per block: the smallest vl + psz + body among the accepted candidates, the first of equals
//   k_fqb_back    a workgroup per block: the winner alone - varint, parameter bytes, body - at its final place, the
//                 caller's slot or the packed offset (k_pk_scan over the winners' sizes in between)
// The host-buffer batch enters behind the first two stages with candidate sets it picked on the host (FqbSets).
// The chunk is offered in two halves (r4x16_fqz_best.h): r4x16_fqb_candidates, everything up to and including k_fqb_win,
// and r4x16_fqb_back.  This unit's calls run one behind the other; the call that picks across codecs
// (r4x16_best_qual.hip, part 2n) puts its own pick, scan and gather between them and hands the back pass the blocks
// fqzcomp won overall.
//
// Loops: over k <= 16 candidates, the records of a block (nrec <= max_records, tested by k_fqp_lens before a record is
// read), tables of fixed size.  Stores: the hand-over is sized by the chunk's items, max_records + 1 and FQP_STAGE; only
// k_fqb_back writes payload to the caller's memory, after the capacity test, and only for a block with a winner.  All
// stores are plain vector stores or vector atomics.
#include "r4x16_host.h"
#include "r4x16_fqz_best.h"
#include "r4x16_fqz_pick.h"

// (FQB_MAX_K, FqbStrats, FqbHand, FqbSets, FqbWork: r4x16_fqz_best.h - the call that picks across codecs runs these stages too)
#define FQB_NO_PARAMS 0xffffffffu           // a parameter size no call admits: the front end reads nothing of the item
static size_t fqb_hand_layout(u8 *base, size_t at, size_t nb, size_t k, u32 max_rec, bool sets, FqbHand *h)
{
    const size_t items = nb * k;
    Carver cv(base, at);
    h->par = cv.take<u8>(sets ? 0 : items * (size_t)FQP_STAGE);
    h->flags = cv.take<u32>(sets ? 0 : items * ((size_t)max_rec + 1u));
    h->par_off = cv.take<u64>(items); h->rec_off = cv.take<u64>(items); h->len_off = cv.take<u64>(items); h->in_off = cv.take<u64>(items);
    h->par_size = cv.take<u32>(items); h->nrec = cv.take<u32>(items); h->in_size = cv.take<u32>(items);
    h->out_cap = cv.take<u32>(items); h->out_size = cv.take<u32>(items);
    h->pick_status = cv.take<i32>(items); h->status = cv.take<i32>(items); h->win = cv.take<i32>(nb);
    h->route = cv.take<u32>(R4X16_FQZ_BEST_KINDS);
    return cv.total();
}

// ---- stage 1: a candidate's decisions and store -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fqb_store(BatchArgs a, FqpIn in, FqpWs w, FqbHand h, FqbStrats ks, int base, int nb)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= (u32)nb * (u32)ks.k) return;
    const int b = (int)(q % (u32)nb), j = (int)(q / (u32)nb), g = base + b;
    const int strat = ks.s[j];
    const FqpBlk *bk = w.blk + b;
    int st = bk->status;
    FqdParam pm;
    FqdChoice ch = {0, 0};
    FqdStats fs;
    u32 psize = 0;
    if (st == 0) {
        FqdSums sm;
        fqp_stats_of(bk, w.part + (u64)b * FQP_PARTS * 5u, &fs, &sm);
        fqd_strat(strat, &pm);
        st = fqd_decide(&pm, &fs, &sm, in.guard_bits, &ch);
    }
    const u32 nrec = bk->nrec;
    u8 *stage = h.par + (u64)q * FQP_STAGE;
    if (st == 0) {
        const u32 *fl = in.flags + in.rec_off[g];
        const u8 *cls = w.wcls + (u64)b * w.rec_stride;
        u32 *fo = h.flags + (u64)q * w.rec_stride;
        u32 fmax = 0;
        for (u32 r = lane; r < nrec; r += WAVE) {
            const u32 f = fqd_flags(fl[r], cls[r] & 3u, &ch);
            fo[r] = f;
            fmax = max(fmax, f >> 16);
        }
        fmax = fqp_wave_max(fmax);
        if (lane == 0) {
            FqdSink sink = {stage, FQP_STAGE, 0u};
            st = fqd_store(&pm, &fs, &ch, in.vers, strat, fmax, bk->qmask, &sink);
            psize = sink.n;                                          // (<= fqd_cap() <= FQP_STAGE)
        }
        st = __builtin_amdgcn_readfirstlane(st);
        psize = (u32)__builtin_amdgcn_readfirstlane((int)psize);
    }
    if (lane != 0) return;
    const bool ok = st == 0;
    h.par_off[q] = (u64)q * FQP_STAGE; h.rec_off[q] = (u64)q * w.rec_stride; h.len_off[q] = (u64)b * w.rec_stride;
    h.in_off[q] = a.in_off[g]; h.out_cap[q] = 0xffffffffu;
    h.in_size[q] = ok ? a.in_size[g] : 0u;
    // the records the reference's encode loop reaches, as in the one-call form (k_fqp_hand)
    h.nrec[q] = ok && nrec ? bk->visited : 0u;
    h.par_size[q] = ok ? psize : FQB_NO_PARAMS;
    h.pick_status[q] = st;
    if (h.route && j == 0 && bk->status == 0 && bk->need_j) atomicAdd(&h.route[R4X16_FQZ_BEST_COUNTED], 1u);
    if (w.route) {
        if (ok) {
            atomicAdd(&w.route[R4X16_FQZ_PICK_BLOCKS], 1u);
            if (stage[1] & 2u) atomicAdd(&w.route[R4X16_FQZ_PICK_SEL], 1u);          // GFLAG_HAVE_STAB: written where PFLAG_DO_SEL is
            if (ch.split) atomicAdd(&w.route[R4X16_FQZ_PICK_SPLIT], 1u);
            if (pm.do_dedup) atomicAdd(&w.route[R4X16_FQZ_PICK_DEDUP], 1u);
        } else if (st == R4X16_E_UNDECIDED) atomicAdd(&w.route[R4X16_FQZ_PICK_UNDECIDED], 1u);
    }
}

// the same arrays for candidate sets that came picked (candidate j of block g of the call: entry g * k + j of the sets'
// arrays): the items of blocks base .. base + nb read their parameter bytes and records from the sets themselves
__global__ __launch_bounds__(256) void k_fqb_items(BatchArgs a, FqbSets sets, FqbHand h, int k, int base, int nb)
{
    const u32 q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (u32)nb * (u32)k) return;
    const int g = base + (int)(q % (u32)nb);
    const size_t e = (size_t)g * k + q / (u32)nb;
    h.in_off[q] = a.in_off[g]; h.in_size[q] = a.in_size[g]; h.out_cap[q] = 0xffffffffu; h.pick_status[q] = 0;
    h.par_off[q] = sets.par_off[e]; h.par_size[q] = sets.par_size[e]; h.rec_off[q] = sets.rec_off[e]; h.len_off[q] = sets.len_off[e];
    h.nrec[q] = sets.nrec[e];
}

// ---- stage 2: the winner ----------------------------------------------------------------------------------------------
// The smallest stream among the candidates the encoder accepted, the first of them in list order.  A candidate the device
// pick cannot decide leaves the block undecided, and one that found no room in the arena - or a slice above the call's
// limits, which refuses every candidate alike - fails the block as a whole (UNSUPPORTED): the smallest of the rest would
// not be the smallest of the list.  A candidate refused otherwise (its parameter bytes, the slice's records) is out of the
// running; with none left the block has the status of the first.
// out_size / status / chosen: entry obase + lb is block lb's (the call's own arrays from the chunk's base, or a chunk's from 0).
__global__ __launch_bounds__(256) void k_fqb_win(FqeIn ein, FqbHand h, FqeWs fw, int k, u32 *out_size, i32 *status, i32 *chosen, int obase, int nb)
{
    const int lb = (int)(blockIdx.x * 256u + threadIdx.x);
    if (lb >= nb) return;
    const int g = obase + lb;
    int win = -1;
    i32 first = 0;
    u64 best = 0;
    u32 coded = 0, refused = 0;
    bool undecided = false, no_room = false;
    for (int j = 0; j < k; j++) {
        const size_t q = (size_t)j * nb + lb;
        const FqeBlk *bk = fw.blk + q;
        const i32 ps = h.pick_status[q], st = ps != 0 ? ps : bk->status;
        if (j == 0) first = st;
        if (st == R4X16_E_UNDECIDED) undecided = true;
        if (st == R4X16_E_UNSUPPORTED) no_room = true;
        if (st != 0) { refused++; continue; }
        coded++;
        const u64 total = (u64)fqe_var_len(bk->size) + ein.par_size[q] + (bk->size ? bk->body : 5u);
        if (win < 0 || total < best) { best = total; win = j; }
        if (fw.route && bk->dups) atomicAdd(&fw.route[R4X16_FQZ_ENC_DUP], 1u);
    }
    i32 st = 0;
    if (undecided) { win = -1; st = R4X16_E_UNDECIDED; }
    else if (no_room) { win = -1; st = R4X16_E_UNSUPPORTED; }
    else if (win < 0) st = first;
    else if (best > 0xffffffffull) { win = -1; st = R4X16_E_CAPACITY; }          // no 32-bit size holds it, and no slot
    h.win[lb] = win;
    status[g] = st;
    out_size[g] = win >= 0 ? (u32)best : 0u;
    if (chosen) chosen[g] = win;
    if (h.route) {
        if (undecided) atomicAdd(&h.route[R4X16_FQZ_BEST_UNDECIDED], 1u);
        else if (!no_room) {
            if (coded) atomicAdd(&h.route[R4X16_FQZ_BEST_CANDIDATES], coded);
            if (refused) atomicAdd(&h.route[R4X16_FQZ_BEST_REFUSED], refused);
        }
    }
}

// pk.off == nullptr: the slot form.  The capacity is tested here, on the winner alone.  take (may be null): [nb], 0 for a
// block whose winner is not wanted - another codec's stream is smaller (r4x16_best_qual.hip); a.out_size[g] is the size of
// the stream that is.
__global__ __launch_bounds__(256) void k_fqb_back(BatchArgs a, PackedOut pk, FqeIn ein, FqbHand h, FqeWs fw, const u32 *wlen, u64 wlen_stride,
                                                  u32 *len_out, const u64 *rec_off, const u32 *nrec, const i32 *take, int base, int nb)
{
    const int lb = (int)blockIdx.x, g = base + lb;
    const u32 t = threadIdx.x;
    const int win = h.win[lb];
    if (win < 0 || (take && take[lb] == 0)) return;
    if (len_out)
        for (u32 r = t; r < nrec[g]; r += 256u) len_out[rec_off[g] + r] = wlen[(u64)lb * wlen_stride + r];
    const size_t q = (size_t)win * nb + lb;
    const FqeBlk bk = fw.blk[q];
    const u32 total = a.out_size[g];
    const bool fits = pk.off ? pk.off[g + 1] <= pk.capacity : total <= a.out_cap[g];
    __syncthreads();                                                 // (every thread has read the size)
    if (t == 0) {
        if (!fits) { a.status[g] = R4X16_E_CAPACITY; a.out_size[g] = 0u; }
        else if (h.route) atomicAdd(&h.route[R4X16_FQZ_BEST_BLOCKS], 1u);
    }
    if (!fits) return;
    const u32 psz = ein.par_size[q], vl = fqe_var_len(bk.size);
    u8 *dst = pk.off ? pk.out + pk.off[g] : a.out + a.out_off[g];
    if (t < vl) dst[t] = (u8)(((bk.size >> (7u * (vl - 1u - t))) & 0x7fu) | (t + 1u < vl ? 0x80u : 0u));   // var_put_u32
    group_copy<256>(dst + vl, ein.par + ein.par_off[q], psz, t);
    if (bk.size) group_copy<256>(dst + vl + psz, fw.stage + bk.out, total - vl - psz, t);
    else if (t < 5u) dst[vl + psz + t] = 0;                          // (nothing to code: RC_FinishEncode's five zero bytes)
}

// ---- the call ---------------------------------------------------------------------------------------------------------
int r4x16_fqb_strats(rans4x16_hip_ctx *c, const char *who, int k, const int *strats, FqbStrats *ks)
{
    bool ok = k >= 1 && k <= FQB_MAX_K && strats;
    for (int j = 0; ok && j < k; j++) ok = strats[j] >= 0;
    if (!ok) { c->err = std::string(who) + ": 1 <= k <= 16 strategies, none negative"; return -1; }
    *ks = FqbStrats{};
    ks->k = k;
    for (int j = 0; j < k; j++) ks->s[j] = strats[j];
    return 0;
}

// what a chunk of nb blocks takes in the adaptive coders' arena: the pick's layout, the hand-over, the encoder's layout
// for nb * k items
size_t r4x16_fqb_chunk_bytes(rans4x16_hip_ctx *c, size_t nb, size_t k, u32 max_in, u32 max_rec, bool sets)
{
    FqpWs w;
    FqbHand h;
    const size_t pick = fqb_hand_layout(nullptr, sets ? 0 : r4x16_fqp_layout(nullptr, nb, max_rec, &w), nb, k, max_rec, sets, &h);
    return pick + r4x16_fqe_chunk_bytes(c, nb * k, max_in, max_rec);
}
size_t r4x16_fqb_chunk_limit(int k, u32 max_rec)
{
    return std::max<size_t>(1, std::min<size_t>(r4x16_fqp_chunk_limit(max_rec), (size_t)INT_MAX) / (size_t)k);
}
static size_t fqb_fit(rans4x16_hip_ctx *c, int n, int k, u32 max_in, u32 max_rec, bool sets)
{
    return r4x16_fit_chunk((size_t)n, r4x16_fqb_chunk_limit(k, max_rec), r4x16_room(c, A_BIT(A_AR)),
                           [&](size_t nb) { return r4x16_fqb_chunk_bytes(c, nb, (size_t)k, max_in, max_rec, sets); });
}

// One chunk up to and including k_fqb_win, laid out at `at`: block lb's winner - size, status, index into the strategies -
// in out_size / status / chosen (may be null) at entry obase + lb, and *w for r4x16_fqb_back, which the caller owes: it
// reads out the encoder's and this unit's route counters.  sets == nullptr: both stages.  Enqueues only; 0 or -1.
int r4x16_fqb_candidates(rans4x16_hip_ctx *c, const BatchArgs &a, const u32 *d_len, const u32 *d_flags, const u64 *d_rec_off, const u32 *d_nrec,
                         int vers, const FqbStrats &ks, const FqbSets *sets, u8 *at, int base, int nb, u32 *out_size, i32 *status, i32 *chosen,
                         int obase, u32 max_in, u32 max_rec, hipStream_t s, FqbWork *w)
{
    const int k = ks.k, items = nb * k;
    *w = FqbWork{};
    FqpWs &pw = w->pw;
    FqbHand &h = w->h;
    const size_t pick = fqb_hand_layout(at, sets ? 0 : r4x16_fqp_layout(at, (size_t)nb, max_rec, &pw), (size_t)nb, (size_t)k, max_rec,
                                        sets != nullptr, &h);
    w->d_best = h.route;
    if (r4x16_route_begin(c, &h.route, R4X16_FQZ_BEST_KINDS, s) != 0) return -1;
    FqeIn &ein = w->ein;
    u32 max_par = FQP_STAGE;
    if (sets) {
        hipLaunchKernelGGL(k_fqb_items, dim3((items + 255) / 256), dim3(256), 0, s, a, *sets, h, k, base, nb);
        ein = FqeIn{sets->par, h.par_off, h.par_size, sets->len, sets->flags, h.rec_off, h.nrec, h.len_off};
        max_par = sets->max_par;
    } else {
        int any_qa = 0, any_r2 = 0;
        for (int j = 0; j < k; j++) {
            FqdParam pm;
            fqd_strat(ks.s[j], &pm);
            any_qa |= pm.do_qa != 0; any_r2 |= pm.do_r2 != 0;
        }
        u32 *const d_pick = pw.route;
        if (r4x16_route_begin(c, &pw.route, R4X16_FQZ_PICK_KINDS, s) != 0) return -1;
        const FqpIn in{d_len, d_flags, d_rec_off, d_nrec, nullptr, vers, ks.s[0], c->fqz_guard_bits, nullptr, nullptr, nullptr, any_qa, any_r2};
        if (r4x16_fqp_stats(c, a, in, pw, base, nb, max_in, max_rec, s) != 0) return -1;
        hipLaunchKernelGGL(k_fqb_store, dim3((items + 3) / 4), dim3(256), 0, s, a, in, pw, h, ks, base, nb);
        if (r4x16_route_end(c, R4X16_ROUTE_FQZ_PICK, d_pick, R4X16_FQZ_PICK_KINDS, s) != 0) return -1;
        ein = FqeIn{h.par, h.par_off, h.par_size, pw.wlen, h.flags, h.rec_off, h.nrec, h.len_off};
    }
    BatchArgs ea = a;                                                // the encoder's arrays: the chunk's items, from 0
    ea.in_off = h.in_off; ea.in_size = h.in_size; ea.out = nullptr; ea.out_off = nullptr; ea.out_cap = h.out_cap; ea.out_size = h.out_size;
    ea.status = h.status;
    if (r4x16_fqe_stages(c, ea, ein, at + pick, 0, items, max_in, max_par, max_rec, s, &w->fw, &w->d_enc) != 0) return -1;
    hipLaunchKernelGGL(k_fqb_win, dim3((nb + 255) / 256), dim3(256), 0, s, ein, h, w->fw, k, out_size, status, chosen, obase, nb);
    return 0;
}

// The back pass over the chunk: the winners of the blocks with take[lb] != 0 (take == nullptr: every winner) assembled
// at a.out + a.out_off[g] or, pk given, at pk->out + pk->off[g], where a.out_size[g] is the size of the stream that goes
// there; d_len_out (may be null) for the same blocks.
int r4x16_fqb_back(rans4x16_hip_ctx *c, const BatchArgs &a, const PackedOut *pk, const FqbWork &w, u32 *d_len_out, const u64 *d_rec_off,
                   const u32 *d_nrec, int base, int nb, const i32 *take, hipStream_t s)
{
    const PackedOut pko = pk ? *pk : PackedOut{nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_fqb_back, dim3(nb), dim3(256), 0, s, a, pko, w.ein, w.h, w.fw, (const u32 *)w.pw.wlen, w.pw.rec_stride, d_len_out,
                       d_rec_off, d_nrec, take, base, nb);
    if (r4x16_route_end(c, R4X16_ROUTE_FQZ_ENC, w.d_enc, R4X16_FQZ_ENC_KINDS, s) != 0) return -1;
    return r4x16_route_end(c, R4X16_ROUTE_FQZ_BEST, w.d_best, R4X16_FQZ_BEST_KINDS, s);
}

// `a`: the call's arrays (the packed form: out, out_off, out_cap null and *pk given).  sets == nullptr: both stages.
static int fqb_run(rans4x16_hip_ctx *c, int n, const BatchArgs &a, const PackedOut *pk, const u32 *d_len, const u32 *d_flags, const u64 *d_rec_off,
                   const u32 *d_nrec, int vers, const FqbStrats &ks, i32 *d_chosen, u32 *d_len_out, u32 max_in, u32 max_rec, const FqbSets *sets,
                   hipStream_t s)
{
    const int k = ks.k;
    const size_t chunk = fqb_fit(c, n, k, max_in, max_rec, sets != nullptr);
    auto grab = [&](size_t nb) { return r4x16_ensure(c, A_AR, r4x16_fqb_chunk_bytes(c, nb, (size_t)k, max_in, max_rec, sets != nullptr), false); };
    return r4x16_chunk_walk(c, n, chunk, s, grab, [&](size_t base, int nb) {
        FqbWork w;
        if (r4x16_fqb_candidates(c, a, d_len, d_flags, d_rec_off, d_nrec, vers, ks, sets, c->at(A_AR), (int)base, nb, a.out_size, a.status, d_chosen,
                                 (int)base, max_in, max_rec, s, &w) != 0)
            return -1;
        if (pk) r4x16_launch_packed_scan(a.out_size, pk->off, (int)base, nb, s);
        return r4x16_fqb_back(c, a, pk, w, sets ? nullptr : d_len_out, d_rec_off, d_nrec, (int)base, nb, nullptr, s);
    });
}

static bool fqb_records_ok(int n, const u32 *d_len, const u32 *d_flags, const u64 *d_rec_off, const u32 *d_nrec, u32 max_records)
{
    return n <= 0 || (d_rec_off && d_nrec && max_records < 0x7fffffffu && (max_records == 0 || (d_len && d_flags)));
}

extern "C" int rans4x16_hip_fqz_best_chunk_blocks(rans4x16_hip_ctx *c, int n, int k, uint32_t max_in_size, uint32_t max_records)
{
    if (!c) return -1;
    if (n < 0 || k < 1 || k > FQB_MAX_K || max_records >= 0x7fffffffu) { c->err = "fqz_best_chunk_blocks: bad arguments"; return -1; }
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    return (int)fqb_fit(c, n, k, max_in_size, max_records, false);
}

extern "C" int rans4x16_hip_fqz_compress_best_dev(rans4x16_hip_ctx *c, int n,
                                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                  const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                                  int vers, int k, const int *strats,
                                                  unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                                  uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                                  uint32_t max_in_size, uint32_t max_records, void *stream)
{
    BatchArgs a;
    FqbStrats ks;
    const int go = r4x16_dev_call_args(c, "fqz_compress_best_dev: bad arguments", fqb_records_ok(n, d_len, d_flags, d_rec_off, d_nrec, max_records), &a,
                                       n, d_in, d_in_off, d_in_size, d_out, d_out_off, d_out_cap, d_out_size, d_status, 0, nullptr,
                                       [&] { return r4x16_fqb_strats(c, "fqz_compress_best_dev", k, strats, &ks); });
    if (go <= 0) return go;
    return fqb_run(c, n, a, nullptr, d_len, d_flags, d_rec_off, d_nrec, vers, ks, d_chosen, d_len_out, max_in_size, max_records, nullptr,
                   (hipStream_t)stream);
}

extern "C" int rans4x16_hip_fqz_compress_best_packed_dev(rans4x16_hip_ctx *c, int n,
                                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                         const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off,
                                                         const uint32_t *d_nrec, int vers, int k, const int *strats,
                                                         unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                         uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                                         uint32_t max_in_size, uint32_t max_records, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    BatchArgs a;
    PackedOut pk;
    FqbStrats ks;
    const int go = r4x16_packed_call_args(c, "fqz_compress_best_packed_dev: bad arguments", fqb_records_ok(n, d_len, d_flags, d_rec_off, d_nrec, max_records),
                                          &a, &pk, n, d_in, d_in_off, d_in_size, d_out, out_capacity, d_out_off, d_out_size, d_status, 0, nullptr, s,
                                          [&] { return r4x16_fqb_strats(c, "fqz_compress_best_packed_dev", k, strats, &ks); });
    if (go <= 0) return go;
    return fqb_run(c, n, a, &pk, d_len, d_flags, d_rec_off, d_nrec, vers, ks, d_chosen, d_len_out, max_in_size, max_records, nullptr, s);
}

// ---- host buffers -----------------------------------------------------------------------------------------------------
// One round trip (r4x16_host_trip): behind the inputs go the places of the records (8 bytes each), the record counts, the
// lengths and the flags (4 bytes each); behind the outputs come the lengths as the fix-ups left them and the winners'
// indices.  The blocks the device leaves undecided have all their candidates picked on the host and go through a second
// trip of their own, which enters behind the device pick: behind their inputs go the items' arrays (FqbSets) - places of
// the parameter bytes, of the flags and of the lengths (8 bytes each), parameter sizes and record counts (4 bytes
// each) -, one list of lengths a block, the flags of every candidate, the parameter bytes.
static int fqb_host_trip(rans4x16_hip_ctx *c, int n, const unsigned char *const *in, const unsigned int *in_size, const unsigned int *nrec,
                         uint32_t *const *len, uint32_t *const *flags, int vers, const FqbStrats &ks, unsigned char *const *out,
                         unsigned int *out_size, int *chosen, int *status, const std::vector<int> &todo, bool on_host)
{
    const size_t N = (size_t)n, K = (size_t)ks.k;
    std::vector<u32> isz(n, 0), cap(n, 0), nr(n, 0);
    std::vector<u8> take(n, 0);
    u32 max_in = 0, max_rec = 0, max_par = 0;
    u64 nrecs = 0;
    for (int i : todo) {
        take[i] = 1; isz[i] = in_size[i]; cap[i] = out_size[i]; nr[i] = nrec[i];
        max_in = std::max(max_in, isz[i]); max_rec = std::max(max_rec, nr[i]);
        nrecs += nr[i];
    }
    std::vector<u8> tail, back;
    std::vector<std::vector<u32>> L(n);
    if (!on_host) {
        tail.assign(12 * N + 8 * (size_t)nrecs, 0);
        u64 *const t_rec_off = (u64 *)tail.data();
        u32 *const t_nrec = (u32 *)(t_rec_off + N), *const t_len = t_nrec + N, *const t_flags = t_len + nrecs;
        u64 at_rec = 0;
        for (int i = 0; i < n; i++) {
            t_rec_off[i] = at_rec;
            if (!take[i]) continue;
            t_nrec[i] = nr[i];
            if (nr[i]) { memcpy(t_len + at_rec, len[i], 4 * (size_t)nr[i]); memcpy(t_flags + at_rec, flags[i], 4 * (size_t)nr[i]); }
            at_rec += nr[i];
        }
    } else {
        // the host's picks: every candidate of every block of the trip
        std::vector<std::vector<u8>> par(N * K);
        std::vector<std::vector<u32>> F(N * K);
        for (int i : todo)
            for (size_t j = 0; j < K; j++) {
                std::vector<u32> Lj;
                if (fqp_pick(vers, ks.s[j], (int)nr[i], len[i], flags[i], in[i], in_size[i], par[i * K + j], Lj, F[i * K + j]) != FQP_OK) {
                    par[i * K + j].clear(); F[i * K + j].assign(nr[i], 0); Lj.assign(nr[i], 0);
                    par[i * K + j].push_back(0xff);                  // (no version byte: the header walk refuses it)
                }
                if (j == 0) L[i] = Lj;                               // (the fix-ups do not depend on the strategy)
                max_par = std::max(max_par, (u32)par[i * K + j].size());
            }
        u64 par_bytes = 0;
        for (auto &p : par) par_bytes += p.size();
        const size_t items = N * K;
        tail.assign(32 * items + 4 * (size_t)nrecs * (1 + K) + (size_t)par_bytes, 0);
        u64 *const t_par_off = (u64 *)tail.data(), *const t_rec_off = t_par_off + items, *const t_len_off = t_rec_off + items;
        u32 *const t_par_size = (u32 *)(t_len_off + items), *const t_nrec = t_par_size + items, *const t_len = t_nrec + items;
        u32 *const t_flags = t_len + nrecs;
        u8 *const t_par = (u8 *)(t_flags + nrecs * K);
        u64 at_len = 0, at_fl = 0, at_par = 0;
        for (int i = 0; i < n; i++) {
            // the records the reference's encode loop reaches (a list that over-runs leaves the rest with 0 bytes)
            u32 reached = 0;
            if (take[i]) {
                u64 pos = 0;
                while (reached < nr[i] && pos < isz[i]) pos += L[i][reached++];
                if (nr[i]) memcpy(t_len + at_len, L[i].data(), 4 * (size_t)nr[i]);
            }
            for (size_t j = 0; j < K; j++) {
                const size_t q = i * K + j;
                t_par_off[q] = at_par; t_rec_off[q] = at_fl; t_len_off[q] = at_len;
                t_par_size[q] = take[i] ? (u32)par[q].size() : FQB_NO_PARAMS;
                t_nrec[q] = reached;
                if (!take[i]) continue;
                if (nr[i]) memcpy(t_flags + at_fl, F[q].data(), 4 * (size_t)nr[i]);
                memcpy(t_par + at_par, par[q].data(), par[q].size());
                at_fl += nr[i]; at_par += par[q].size();
            }
            if (take[i]) at_len += nr[i];
        }
    }
    const size_t down = on_host ? 4 * N : 4 * (size_t)nrecs + 4 * N;
    const HostTrip trip = {in, out, out_size, status, take.data(), isz.data(), cap.data(), nullptr, tail.data(), tail.size(), down, &back};
    const int rc = r4x16_host_trip(c, n, trip, [&](const StageLayout &Ly, size_t in_total, size_t out_total, hipStream_t s) {
        const u8 *d_tail = Ly.in + in_total;                         // (in_total, out_total: multiples of 16 in arenas aligned to 256)
        BatchArgs a;
        const int go = r4x16_dev_call_args(c, "fqz_compress_best_batch: bad arguments", true, &a, n, Ly.in, Ly.in_off, Ly.in_size, Ly.out, Ly.out_off,
                                           Ly.cap, Ly.osz, Ly.status, 0, nullptr);
        if (go <= 0) return go;
        if (!on_host) {
            const u64 *d_rec_off = (const u64 *)d_tail;
            const u32 *d_nrec = (const u32 *)(d_rec_off + N), *d_len = d_nrec + N, *d_flags = d_len + nrecs;
            u32 *d_len_out = (u32 *)(Ly.out + out_total);
            return fqb_run(c, n, a, nullptr, d_len, d_flags, d_rec_off, d_nrec, vers, ks, (i32 *)(d_len_out + nrecs), d_len_out, max_in, max_rec, nullptr, s);
        }
        const size_t items = N * K;
        const u64 *d_par_off = (const u64 *)d_tail, *d_rec_off = d_par_off + items, *d_len_off = d_rec_off + items;
        const u32 *d_par_size = (const u32 *)(d_len_off + items), *d_nrec = d_par_size + items, *d_len = d_nrec + items, *d_flags = d_len + nrecs;
        const FqbSets sets{(const u8 *)(d_flags + nrecs * K), d_par_off, d_par_size, d_len, d_flags, d_rec_off, d_len_off, d_nrec, max_par};
        return fqb_run(c, n, a, nullptr, nullptr, nullptr, nullptr, nullptr, vers, ks, (i32 *)(Ly.out + out_total), nullptr, max_in, max_rec, &sets, s);
    });
    if (rc < 0) return -1;
    if (back.size() < down) { c->err = "fqz_compress_best_batch: the trip's tail is missing"; return -1; }
    const u32 *b_len = (const u32 *)back.data();
    const i32 *b_chosen = (const i32 *)(back.data() + (on_host ? 0 : 4 * (size_t)nrecs));
    u64 at_rec = 0;
    for (int i = 0; i < n; i++) {
        if (!take[i]) continue;
        if (chosen) chosen[i] = status[i] == 0 ? b_chosen[i] : -1;
        if (status[i] == 0 && nr[i]) memcpy(len[i], on_host ? L[i].data() : b_len + at_rec, 4 * (size_t)nr[i]);
        at_rec += nr[i];
    }
    return 0;
}

extern "C" int rans4x16_hip_fqz_compress_best_batch(rans4x16_hip_ctx *c, int n,
                                                    const unsigned char *const *in, const unsigned int *in_size,
                                                    const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags,
                                                    int vers, int k, const int *strats,
                                                    unsigned char *const *out, unsigned int *out_size, int *chosen, int *status)
{
    if (!c) return -1;
    FqbStrats ks;
    if (n < 0 || (n && (!in || !in_size || !nrec || !len || !flags || !out || !out_size || !status))) {
        c->err = "fqz_compress_best_batch: bad arguments";
        return -1;
    }
    if (r4x16_fqb_strats(c, "fqz_compress_best_batch", k, strats, &ks) != 0) return -1;
    if (n == 0) return 0;
    std::vector<int> todo, host;
    std::vector<u32> cap(out_size, out_size + n);
    for (int i = 0; i < n; i++) {
        status[i] = 0;
        if (chosen) chosen[i] = -1;
        if ((!in[i] && in_size[i]) || !out[i] || (nrec[i] && (!len[i] || !flags[i])) || nrec[i] > 0x7fffffffu) { status[i] = R4X16_E_UNSUPPORTED; out_size[i] = 0; }
        else todo.push_back(i);
    }
    if (!todo.empty() && fqb_host_trip(c, n, in, in_size, nrec, len, flags, vers, ks, out, out_size, chosen, status, todo, false) != 0) return -1;
    for (int i : todo)
        if (status[i] == R4X16_E_UNDECIDED) { status[i] = 0; out_size[i] = cap[i]; host.push_back(i); }
    if (!host.empty()) {
        if (c->opts.v[OPT_ROUTE_COUNT]) c->route[R4X16_ROUTE_FQZ_PICK][R4X16_FQZ_PICK_HOST] += (long)host.size();
        if (fqb_host_trip(c, n, in, in_size, nrec, len, flags, vers, ks, out, out_size, chosen, status, host, true) != 0) return -1;
    }
    // the reference clears the selectors it kept in the flags (:1142-1144)
    for (int i = 0; i < n; i++)
        if (len[i] && flags[i]) for (u32 r = 0; r < nrec[i]; r++) flags[i][r] &= 0xffffu;
    return (int)(n - std::count(status, status + n, 0));
}
