// =============================================================================================
// r4x16_enc_chain.hip - the encoder's LDS size classes, their classify kernel and the table of launches that
// r4x16_launch_enc_chain hands to the class launcher (sched_launch_classes, r4x16_sched.hip); the residency and route
// queries over the same tables; the instantiations of k_enc_chain (r4x16_enc_chain.h) for u16 images, and the rANS 4x8
// chain kernel.  The packed-row instantiation lives in r4x16_enc_chain_pk.hip, the record kernel in
// r4x16_enc_chain_rec.hip: their kernels are reached through the accessors declared below.
// =============================================================================================
#include "r4x16_enc_chain.h"
#include "r4x16_host.h"

// r4x16_enc_chain_pk.hip: k_enc_chain<true, true> / k_enc_chain<true, true, true>; r4x16_enc_chain_rec.hip: k_enc_chain_rec
extern "C" void r4x16_enc_chain_pk_lds_limit(int bytes);
extern "C" const void *r4x16_enc_chain_pk_kernel(int freq_table);
extern "C" void r4x16_enc_chain_rec_lds_limit(int bytes);
extern "C" const void *r4x16_enc_chain_rec_kernel(void);

// ---- host-callable launcher ----------------------------------------------------------------------
// {LDS bytes per stream, streams per wave}; LDS is allocated in 1,280-byte granules.
// q4/q8 images are ~0.4 KB, an order-0 row 0.8 KB, q40 4.6 KB (16 x 4,800 = 60 granules: 2 waves, 32 streams per CU — fuller waves measured faster than more waves)
// LDS size classes: bytes per stream (image + word ring).  A workgroup takes as many streams as
// fit beside the shared reciprocal table, up to 64 (four waves); 1,280-byte allocation granules.
// (sizes are 16 mod 128: consecutive streams start four LDS banks apart, so that the eight streams of a
// 32-lane access group do not all hit the same bank when they touch the same offset)
// (round 3: the steps above 12,816 were 33,296 and 73,616 - the 13 KB image of a 79-symbol alphabet, what X_PACK|X_RLE
//  makes of four-letter quality values, sat in the 33 KB class at four streams per CU: 11.8 ms for 4,096 such streams.
//  Now every count of streams per CU from nine to one has its class: 147,344 bytes beside the reciprocal table / k.)
// {LDS bytes per stream, streams per wave - rows: 0, as many streams per workgroup as fit (enc_class_qpw)}
struct EncClass { u32 bytes; int qpw; };
static constexpr EncClass ENC_CLASSES[] = {{656}, {1296}, {2576}, {4752}, {6416}, {12816}, {16272}, {24464}, {36752}, {49040}, {73616}, {147344}};
// packed rows (20..64 symbols, 10-bit tables): 46 symbols need 3,532 bytes -> 45 streams per CU beside the small
// reciprocal table (3,536 is 80 mod 128: consecutive streams start 20 banks apart)
static constexpr EncClass ENC_PK_CLASSES[] = {{1168}, {2064}, {2832}, {3536}, {3728}, {4752}, {6416}};
// the short-index kind of the packed rows (r4x16_common.h: highest byte below 128): class k is packed class k less the
// half of the index its images leave out - 46 symbols: 3,408 bytes, 45 streams per CU beside the 8,208-byte frequency
// table (80 mod 128 like 3,536)
#define ENC_PKS_LESS (ENC_IMG_IDX - ENC_IMG_IDX_SHORT)
// symbol records (r4x16_enc_chain_rec.hip; only batches that leave LDS to spare make such images): one wave
// per workgroup; four workgroups per CU, then fewer
static constexpr EncClass ENC_REC_CLASSES[] = {
    {2576, 15}, {4112, 9}, {8080, 5}, {13584, 3}, {20368, 2}, {32000, 1}, {40960, 1}, {53760, 1}, {81920, 1}, {163840, 1},
};
// the order-0 streams of the u16 rows (a 770-byte image and the ring) and of the records (a 4,352-byte image and the
// ring) have a class of their own each: the kernels run a wave's order-1 streams, then its order-0 streams, and a class
// that holds both - small order-1 alphabets make images as small as a one-row image - would pay both latencies
static constexpr EncClass ENC_O0_ROWS[] = {{1296}}, ENC_O0_REC[] = {{8080, 5}};
// The classes, group by group in the order of their ids: the kind the classifier matches (r4x16_common.h ENC_KIND_*),
// the group's table (less: taken off every entry), what the route read-out counts its streams as (R4X16_ENC_*; freq: as
// R4X16_ENC_PACKED_FREQ too).  Behind them the catch-all of images too large for LDS.
struct EncGroup { u32 kind; const EncClass *cls; u32 n, less; int route; bool freq; };
template <u32 N> static constexpr EncGroup enc_group(u32 kind, const EncClass (&cls)[N], u32 less, int route, bool freq = false) { return {kind, cls, N, less, route, freq}; }
static constexpr EncGroup ENC_GROUPS[] = {
    enc_group(ENC_KIND_U16, ENC_CLASSES, 0u, R4X16_ENC_U16),
    enc_group(ENC_KIND_PACKED, ENC_PK_CLASSES, 0u, R4X16_ENC_PACKED),
    enc_group(ENC_KIND_PK_SHORT, ENC_PK_CLASSES, ENC_PKS_LESS, R4X16_ENC_PACKED, true),
    enc_group(ENC_KIND_RECORDS, ENC_REC_CLASSES, 0u, R4X16_ENC_RECORDS),
    enc_group(ENC_KIND_U16_O0, ENC_O0_ROWS, 0u, R4X16_ENC_U16),
    enc_group(ENC_KIND_RECORDS_O0, ENC_O0_REC, 0u, R4X16_ENC_RECORDS),
};
static constexpr u32 enc_ncls() { u32 n = 0; for (const EncGroup &g : ENC_GROUPS) n += g.n; return n; }
static u32 enc_table_bytes(u32 kind) { return kind == ENC_KIND_PK_SHORT ? ENC_LFREQ_BYTES : kind == ENC_KIND_PACKED ? ENC_LRCP_PK_BYTES : ENC_LRCP_BYTES; }
static int enc_class_qpw(u32 bytes, u32 kind, const R4Opts *o)
{
    const u32 room = 163840u - enc_table_bytes(kind);
    const u32 fit = room / bytes;
    const int cap = (int)o->v[OPT_ENC_QPW_CAP];                  // tuning aid (default 64)
    return (int)(fit > (u32)cap ? (u32)cap : fit);
}
struct EncClassTab { u32 n; u32 sort; u32 bytes[CLS_MAX]; u32 pk[CLS_MAX]; };     // classes: u16 images, then packed ones, then records
__global__ __launch_bounds__(256) void k_enc_classify(const EncItem *items, int nitems, EncClassTab tab, SchedWs sw)
{
    __shared__ u32 local[CLS_MAX];
    __shared__ u64 lwork[2 * CLS_MAX];
    if (threadIdx.x < CLS_MAX) { local[threadIdx.x] = 0; lwork[threadIdx.x] = 0ull; lwork[CLS_MAX + threadIdx.x] = 0ull; }
    __syncthreads();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    u32 c = CLS_NONE, len = 0;
    if (i < nitems && items[i].active) {
        // the kind of the image; the order-0 streams of the u16 rows and of the records have classes of their own (ENC_GROUPS)
        const u32 need = items[i].img_bytes + ENC_RING_BYTES, raw = items[i].packed,
                  pk = items[i].order != 0 ? raw : raw == ENC_KIND_U16 ? ENC_KIND_U16_O0 : raw == ENC_KIND_RECORDS ? ENC_KIND_RECORDS_O0 : raw;
        c = tab.n;                                         // images too large for LDS (never a packed one)
        for (u32 k = 0; k < tab.n; k++) if (tab.pk[k] == pk && need <= tab.bytes[k]) { c = k; break; }
        len = items[i].n;
    }
    sched_classify(sw, i, i < nitems, c, len, tab.sort != 0, local, lwork);
    __syncthreads();
    sched_classify_flush(sw, local, lwork);
}
// the shape of a class's launch: streams per workgroup, waves, streams per wave, LDS bytes
struct EncShape { int qpw, waves, spw; size_t ldsb; u32 bytes; };
// (kind: u16 rows of either order, packed rows, their short-index kind)
static EncShape enc_rows_shape(u32 kind, u32 bytes, int nitems, const R4Opts *o)
{
    const u32 tuned = kind == ENC_KIND_PACKED ? 3536u : kind == ENC_KIND_PK_SHORT ? 3536u - ENC_PKS_LESS : 4752u;    // the class of the 46-symbol quality tables
    const int force_qpw = (int)o->v[OPT_ENC_QPW], force_waves = (int)o->v[OPT_ENC_WAVES];   // tuning aids
    int qpw = (force_qpw && bytes == tuned) ? force_qpw : enc_class_qpw(bytes, kind, o);
    // One workgroup per CU is the best shape (measured: 30 streams per CU as 1 x 32 beat 2 x 16 by a
    // third and half-filled 64s by a fifth), so a batch that cannot fill the class's workgroups on
    // every CU gets smaller ones (items [0, n/3) are the payload streams).
    {
        const int cus = r4x16_cu_count();
        int want = (((nitems + 2) / 3 + cus - 1) / cus + 3) & ~3;
        if (want < 8) want = 8;
        if (qpw > want) qpw = want;
    }
    int waves = (qpw + 7) / 8;                         // about eight streams per wave measured best (fewer
    if (waves > 4) waves = 4;                          // lanes per LDS access, one wave per SIMD)
    if (force_waves && bytes == tuned) waves = force_waves;
    EncShape sh;
    sh.qpw = qpw; sh.waves = waves; sh.spw = (qpw + waves - 1) / waves; sh.bytes = bytes;
    sh.ldsb = (size_t)enc_table_bytes(kind) + (size_t)qpw * bytes;
    return sh;
}
static EncShape enc_rec_shape(const EncClass &c, const R4Opts *o)
{
    const int force_rec = (int)o->v[OPT_ENC_QPW_REC];     // tuning aid
    EncShape sh;
    sh.qpw = (force_rec > 0 && c.qpw > force_rec) ? force_rec : c.qpw;
    sh.waves = 1; sh.spw = sh.qpw; sh.bytes = c.bytes;
    sh.ldsb = (size_t)sh.qpw * c.bytes;
    return sh;
}
extern "C" void r4x16_launch_enc_chain(const EncWs *ws, int nitems, hipStream_t s0, const R4Fork *fk, const R4Opts *o, SchedHint *hint)
{
    // the classes go out side by side or in stream order: sched_launch_classes (r4x16_sched.hip); class index ci =
    // position in the classify table: ENC_GROUPS' classes, group by group
    SchedLaunch todo[CLS_MAX];
    int ntodo = 0;
    EncClassTab tab;
    tab.n = 0;
    tab.sort = o->v[OPT_SCHED_SORT] != 0;
    SchedPlan plan;
    sched_plan_init(plan, fk ? fk->n + 1 : 1, o);
    const int cus = r4x16_cu_count();
    // (kern == nullptr: the class keeps its id and its plan entry, and gets no launch)
    auto add = [&](u32 pk, u32 bytes, const EncShape &sh, const void *kern) {
        const u32 ci = tab.n++;
        tab.pk[ci] = pk; tab.bytes[ci] = bytes;
        const int wgs = sched_resident_per_cu(sh.ldsb, sh.waves);
        plan.qpw[ci] = (u16)sh.qpw; plan.wgs_full[ci] = (u16)(cus * wgs);
        plan.rate[ci] = sched_rate(sh.qpw, sh.waves, wgs, cus);
        if (!kern) return;
        todo[ntodo++] = SchedLaunch{kern, r4x16_resident_grid(sh.ldsb, sh.waves, (nitems + sh.qpw - 1) / sh.qpw), WAVE * sh.waves, sh.ldsb, ci, sh.qpw, sh.spw, sh.bytes};
    };
    for (const EncGroup &g : ENC_GROUPS) {
        const bool rec = g.route == R4X16_ENC_RECORDS;       // (record classes: only batches that leave LDS to spare make such images)
        const void *kern = rec ? (ws->direct_budget ? r4x16_enc_chain_rec_kernel() : nullptr) :
                           g.route == R4X16_ENC_PACKED ? r4x16_enc_chain_pk_kernel(g.freq) : (const void *)k_enc_chain<true, false>;
        for (u32 k = 0; k < g.n; k++)
            add(g.kind, g.cls[k].bytes - g.less, rec ? enc_rec_shape(g.cls[k], o) : enc_rows_shape(g.kind, g.cls[k].bytes - g.less, nitems, o), kern);
    }
    plan.ncls = tab.n;
    if (r4x16_first_on_device(FIRST_ENC_CHAIN)) {
        sched_lds_limit((const void *)k_enc_chain<true, false>, 163840);
        r4x16_enc_chain_pk_lds_limit(163840);
        r4x16_enc_chain_rec_lds_limit(163840);
    }
    // images too large for LDS
    const SchedLaunch tail = {(const void *)k_enc_chain<false, false>, (nitems + 15) / 16, WAVE, 0, tab.n, 16, 16, 0u};
    EncItem *items = ws->items;
    const u32 *rcptab = ws->rcptab;
    u8 *dump = ws->dump;
    const u32 *list = ws->sched.list;
    u32 *cnt, bytes;
    int qpw, spw, dyn = o->v[OPT_SCHED_CLAIM] != 0, aff_on = o->v[OPT_ENC_AFFINE] != 0;
    // the streams coded by the affine body are counted in the last word of the per-class counts, which no class uses: it
    // travels to the host with them (r4x16_route_snap)
    static_assert(enc_ncls() + 1u <= ENC_ROUTE_AFF_WORD, "a free word behind the counts of the classes and the catch-all");
    u32 *aff_count = o->v[OPT_ROUTE_COUNT] ? ws->sched.cnt + SCHED_COUNT + ENC_ROUTE_AFF_WORD : nullptr;
    void *args[] = {(void *)&items, (void *)&rcptab, (void *)&dump, (void *)&list, (void *)&cnt, (void *)&qpw, (void *)&spw, (void *)&bytes, (void *)&dyn,
                    (void *)&aff_on, (void *)&aff_count};
    sched_launch_classes(plan, SchedBatch{&ws->sched, nitems, s0, fk, o, hint, 1u, "encode"}, todo, ntodo, &tail, 1,
        [&] { hipLaunchKernelGGL(k_enc_classify, dim3((nitems + 255) / 256), dim3(256), 0, s0, (const EncItem *)ws->items, nitems, tab, ws->sched); },
        [&](const SchedLaunch &L) { cnt = ws->sched.cnt + L.ci; qpw = L.qpw; spw = L.spw; bytes = L.bytes; return args; });
}
// LDS bytes a stream may spend on symbol records when `nblk` streams are to be resident at once: the largest record
// class that still holds the batch in one round of the chip (0: none).  R4X16_ENC_DIRECT=0 never; =N up to N rounds.
extern "C" u32 r4x16_enc_direct_budget(int nblk, const R4Opts *o)
{
    const int rounds = (int)o->v[OPT_ENC_DIRECT];
    if (rounds <= 0 || nblk <= 0) return 0u;
    const long cus = r4x16_cu_count();
    const long per_cu = (nblk + cus * rounds - 1) / (cus * rounds);
    u32 best = 0;
    for (const auto &c : ENC_REC_CLASSES)       // (one wave per workgroup)
        if ((long)sched_resident_per_cu((size_t)c.qpw * c.bytes, 1) * c.qpw >= per_cu && c.bytes > best) best = c.bytes;
    return best;
}
// The row kind of a class id of r4x16_launch_enc_chain's table (ENC_GROUPS' classes, then the catch-all of images too
// large for LDS: u16 rows) as the route read-out counts it (include/rans4x16_hip.h R4X16_ENC_*); -1 beyond the table.
// *freq_table: the class is of the short-index kind (counted as R4X16_ENC_PACKED_FREQ as well).
extern "C" int r4x16_enc_route_kind(u32 ci, int *freq_table)
{
    *freq_table = 0;
    for (const EncGroup &g : ENC_GROUPS) {
        if (ci < g.n) { *freq_table = g.freq; return g.route; }
        ci -= g.n;
    }
    return ci == 0 ? R4X16_ENC_U16 : -1;
}
// Streams per CU of the record class a stream lands in when the batch's budget admits records (r4x16_enc_direct_budget and
// the front's choice, r4x16_encode.hip); -1 where its image can never be records.
extern "C" int r4x16_enc_residency_records(u32 nsym, int order, int *streams_per_wave, int *waves_per_cu)
{
    if (nsym == 0 || nsym > 256) return -1;
    const u32 img = order ? enc_rec_img_bytes(nsym, nsym) : enc_rec_img_bytes(256u, 1u);
    if (img > ENC_IMG_MAIN) return -1;
    for (const auto &c : ENC_REC_CLASSES) {
        if (img + ENC_RING_BYTES > c.bytes) continue;
        const int wgs = sched_resident_per_cu((size_t)c.qpw * c.bytes, 1);      // (one wave per workgroup)
        *streams_per_wave = c.qpw;
        *waves_per_cu = wgs;
        return wgs * c.qpw;
    }
    return -1;
}
extern "C" int r4x16_enc_residency(u32 nsym, int order, int *streams_per_wave, int *waves_per_cu)
{
    if (nsym == 0 || nsym > 256) return -1;
    // (the packed rows need a 10-bit table: what every BASELINE text chooses; a 12-bit stream keeps the u16 rows)
    // (of the packed rows' two kinds the full index: what any alphabet of that size can take; the short-index classes
    //  hold as many streams or more)
    const bool pk = order && nsym >= ENC_PK_MIN_NS && nsym <= ENC_PK_MAX_NS;
    const u32 need = (pk ? enc_pk_img_bytes(nsym) : order ? ENC_IMG_IDX + 2u * nsym * (nsym + 1) : ENC_IMG_IDX + 2u * 257u) + ENC_RING_BYTES;
    const EncGroup &g = ENC_GROUPS[pk ? 1 : 0];
    static_assert(ENC_GROUPS[0].kind == ENC_KIND_U16 && ENC_GROUPS[1].kind == ENC_KIND_PACKED, "the groups of order-1 rows come first");
    for (u32 k = 0; k < g.n; k++) {
        const EncClass &c = g.cls[k];
        if (need > c.bytes) continue;
        const int qpw = enc_class_qpw(c.bytes, g.kind, r4x16_opts_defaults());
        int waves = (qpw + 7) / 8;
        if (waves > 4) waves = 4;
        *streams_per_wave = (qpw + waves - 1) / waves;
        *waves_per_cu = waves;                               // one workgroup per CU
        return qpw;
    }
    *streams_per_wave = 16; *waves_per_cu = 8;
    return 128;
}

// ---------------------------------------------------------------------------------------------
// rANS 4x8 (include/rans4x8_hip.h): the chain kernel for images that fit LDS.  Round 4: the 4x16 encoder's software
// pipeline (chain_encode_o1_lds / chain_encode_o0_pipe: input pieces, compact indices, cumulative pairs and reciprocals
// fetched trips ahead, emitted bytes through the LDS ring, 16-byte stores) with rANS 4x8's byte renormalisation
// (EncOutT<true>: up to two bytes per chain and step, rANS_byte.h:320-402) instead of round 2's step-at-a-time loop -
// the streams, the quarter maps and the u16 cumulative image are the same for both codecs.  A workgroup of up to four
// waves shares one LDS copy of the reciprocal table; qpw streams per workgroup, spw per wave.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k8_enc_chain_pipe(EncItem *items, const u32 *rcptab_, u8 *dump_, const u32 *list, const u32 *count,
                                                         u32 slot_bytes, int qpw, int spw)
{
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    const u32 tid = threadIdx.x, lane = tid & (WAVE - 1), wq = lane >> 2;
    const u32 quad = (tid >> 6) * (u32)spw + wq;                 // stream slot inside the workgroup
    const int nmine = (int)count[0];
    list += count[CLS_MAX];
    if ((int)blockIdx.x * qpw >= nmine) return;
    const int slot = (int)blockIdx.x * qpw + (int)quad;
    const bool mine = wq < (u32)spw && quad < (u32)qpw && slot < nmine;
    EncItem *I = &items[list[mine ? slot : (int)blockIdx.x * qpw]];
    const bool active = mine && I->active;
    gcu32 *rcptab = to_global(rcptab_);
    gcu8 *data = (gcu8 *)I->data;
    gu8 *send = (gu8 *)I->scratch_end;
    const u32 n = I->n, ns = I->ns, order = active ? I->order : 2u;
    u32 *lrcp = (u32 *)lds;
    u8 *slots = lds + ENC_LRCP_BYTES;
    for (u32 j = tid; j < RCPTAB_ENTRIES; j += blockDim.x) lrcp[j] = rcptab[j];
    // each wave copies the images of its own quads (16-byte pieces)
    const u64 my_img = active ? I->image : 0ull;
    const u32 nbytes = active ? ENC_IMG_IDX + (order ? 2u * ns * (ns + 1u) : 2u * 257u) : 0u;
    const u32 wq0 = (tid >> 6) * (u32)spw;
    for (int qd = 0; qd < 16; qd++) {
        const u64 src = __shfl(my_img, qd * 4);
        const u32 nb = __shfl(nbytes, qd * 4);
        if (!src) continue;
        gcu32x4 *sp = (gcu32x4 *)src;
        u32x4 *dd = (u32x4 *)(slots + (u64)(wq0 + qd) * slot_bytes);
        for (u32 j = lane; j < ((nb + 15) >> 4); j += WAVE) dd[j] = sp[j];
    }
    __syncthreads();
    const u32 sl = active ? quad : 0u;                         // (lanes without a stream read and write the LDS of stream 0)
    const u8 *im = slots + (u64)sl * slot_bytes;
    u8 *ring = slots + (u64)sl * slot_bytes + (slot_bytes - ENC_RING_BYTES);
    gu8 *dump = to_global(dump_) + 16u * ((blockIdx.x * blockDim.x + tid) & (ENC_DUMP_BYTES / 16u - 1u));
    u32 pay = chain_encode_o1_lds<false, true>(im, ring, lrcp, data, n, ns, 12u, (gcu8 *)rcptab, send, dump, order == 1, lane);
    pay |= chain_encode_o0_pipe<true>(im, ring, lrcp, data, n, 12u, (gcu8 *)rcptab, send, dump, order == 0, lane);
    if (active && (lane & 3) == 0) I->pay_len = pay;
}
extern "C" void r4x8_enc_chain_launch(EncItem *items, const u32 *rcptab, u8 *dump, const u32 *list, const u32 *count, int nblk, u32 slot_bytes,
                                      int qpw, int spw, hipStream_t s)
{
    if (r4x16_first_on_device(FIRST_ENC8_CHAIN)) sched_lds_limit((const void *)k8_enc_chain_pipe, 163840);
    const int waves = (qpw + spw - 1) / spw;
    hipLaunchKernelGGL(k8_enc_chain_pipe, dim3((nblk + qpw - 1) / qpw), dim3(WAVE * waves), ENC_LRCP_BYTES + (size_t)qpw * slot_bytes, s,
                       items, rcptab, dump, list, count, slot_bytes, qpw, spw);
}
