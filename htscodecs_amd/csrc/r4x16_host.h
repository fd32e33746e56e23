// r4x16_host.h - what the host-side translation units of librans4x16_hip.so share: the context, the error
// macro and the entry points of the host-buffer batch machinery (r4x16_host.hip) used by the C ABI (r4x16_api.hip).
// It is also the one place that declares the launchers and queries the kernel units define: those units include it,
// so that a definition that drifts from its declaration does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <string>
#include <vector>
#include <mutex>
#include <atomic>
#include <thread>
#include <chrono>
#include <algorithm>
#include <functional>

#include "../../include/rans4x16_hip.h"
#include "../../include/rans4x8_hip.h"
#include "r4x16_dev.h"
#include "r4x16_sched.h"
#include "r4x16_plan.h"
#include "r4x16_stage.h"

extern "C" {
void r4x16_launch_dec_front(const BatchArgs *, const DecWs *, int, int, hipStream_t, const R4Opts *);
void r4x16_launch_dec_chain(const DecWs *, int, hipStream_t, const R4Fork *, const R4Opts *, SchedHint *);
int  r4x16_launch_dec_back(const BatchArgs *, const DecWs *, int, int, hipStream_t, const R4Opts *);
void r4x16_launch_enc_front(const BatchArgs *, const EncWs *, int, int, hipStream_t, const R4Opts *);
void r4x16_launch_enc_tables(const BatchArgs *, const EncWs *, int, int, hipStream_t);
void r4x16_launch_enc_chain(const EncWs *, int, hipStream_t, const R4Fork *, const R4Opts *, SchedHint *);
void r4x16_launch_enc_finish(const BatchArgs *, const EncWs *, int, int, hipStream_t);
// the packed calls' finish: sizes, offsets, then every stream assembled at out + off[i] (r4x16_encode.hip, r4x16_packed.hip)
void r4x16_launch_enc_finish_dense(const BatchArgs *, const EncWs *, int, int, const PackedOut *, hipStream_t);
void r4x16_launch_packed_scan(const u32 *size, u64 *off, int base, int nb, hipStream_t);
u32  r4x16_compress_bound(u32 size, int order);
u32  r4x16_dec_direct_budget(int nblk, const R4Opts *);
u32  r4x16_dec_mid_budget(int nblk, const R4Opts *);
u32  r4x16_enc_direct_budget(int nblk, const R4Opts *);
void r4x16_launch_stripe(const u8 *, u8 *, u32, u32, int, hipStream_t);
// streams per CU of the chain kernels, by host arithmetic on the class tables (rans4x16_hip_residency), and the row kind
// of a class id as the route read-out counts it
int  r4x16_dec_residency(u32 nsym, int order, u32 bits, int *streams_per_wave, int *waves_per_cu, int short_ring);
int  r4x16_dec_residency_kind(u32 nsym, int order, u32 bits, bool short_step, int *streams_per_wave, int *waves_per_cu);
int  r4x16_enc_residency(u32 nsym, int order, int *streams_per_wave, int *waves_per_cu);
int  r4x16_enc_residency_records(u32 nsym, int order, int *streams_per_wave, int *waves_per_cu);
int  r4x16_dec_route_kind(u32 ci);
int  r4x16_enc_route_kind(u32 ci, int *freq_table);
// rANS 4x8
size_t r4x8_dec_ws_bytes(size_t nblk);
void r4x8_launch_decode(const BatchArgs *, u8 *ws, int base, int nblk, hipStream_t);
void r4x8_launch_encode(const BatchArgs *, const EncWs *, int base, int nblk, hipStream_t);
// the same in its two halves (front end, classes and chains over nblk items; the finish into the callers' slots), and
// what the packed and best-of-two calls put around the first half: a block as k items, then verdicts / sizes / winners,
// offsets and the winners at their final place (r4x16_encode.hip)
void r4x8_launch_enc_front(const BatchArgs *, const EncWs *, int base, int nblk, hipStream_t);
void r4x8_launch_enc_finish(const BatchArgs *, const EncWs *, int base, int nblk, hipStream_t);
void r4x8_launch_enc_items(const BatchArgs *, int base, int nb, int k, const int *m, u32 max_in_size, const Enc8Items *, hipStream_t);
void r4x8_launch_enc_finish_pick(const BatchArgs *, const EncWs *, int base, int nblk, int k, const Pick8Out *, hipStream_t);
void r4x8_enc_chain_launch(EncItem *items, const u32 *rcptab, u8 *dump, const u32 *list, const u32 *count, int nblk, u32 slot_bytes,
                           int qpw, int spw, hipStream_t);
u32  r4x8_compress_bound(u32 size);
}

struct TimedLaunch { hipEvent_t a, b; };
// route read-out (option route_count): a copy of one chain launch's per-class stream counts, on its way to pinned memory
struct RouteSnap { int which; u32 *cnt; hipEvent_t ev; };
#define ROUTE_WHICH 15
// R4X16_ROUTE_ENCODE_BODY rides on the encode chain's copy: the word of the per-class counts that k_enc_chain's affine
// waves count their streams in (no launch has that many classes; r4x16_enc_chain.hip)
#define ENC_ROUTE_AFF_WORD (CLS_MAX - 1u)
#define ROUTE_KINDS 8
struct HostPipe;
void r4x16_pipe_destroy(HostPipe *);
// the lane contexts of a context's host pipeline (nullptr past the last)
struct rans4x16_hip_ctx *r4x16_pipe_lane(HostPipe *, int i);
// The context's device arenas, each growing on demand and kept between calls (r4x16_api.hip).  One routine grows them,
// one says what a call may take, and the layouts inside them are Carver's (r4x16_plan.h).
enum R4Arena {
    A_WS,        // the workspace of the slot calls' pipelines
    A_STAGE,     // staging for the host-buffer entry points
    A_XS,        // the internal items of X_STRIPE blocks (r4x16_stripe.hip) and of best-of-k candidates (r4x16_best.hip)
    A_PS,        // the packed calls' internal bound-sized slots and layout arrays (r4x16_packed.hip)
    A_T3,        // tok3 containers: the winners waiting to be framed / the directory of the columns to decode (r4x16_tok3.hip)
    A_TN,        // tok3 names: the names' histories; for the one-call form the columns in front of them (r4x16_tok3_names.hip)
    A_AR,        // the adaptive coders: arith_dynamic, either direction - items, stage arena, the order-1 rows that do not fit LDS
                 // (r4x16_arith.hip, r4x16_arith_enc.hip); fqzcomp_qual, either direction - blocks, tables, record tables, model slots (r4x16_fqz.hip, r4x16_fqz_enc.hip)
    A_COUNT
};
#define A_BIT(a) (1u << (a))
// At least `bytes` in arena `which`: growing synchronizes the device, frees and allocates anew (contents are not kept).
// refuse_above_half_free: for sizes that come from a caller's arrays or a stream's own size fields - never more than
// half of what the card has free.  -1 with err set; an allocation failure is not sticky, the caller may ask for less.
int r4x16_ensure(rans4x16_hip_ctx *c, R4Arena which, size_t bytes, bool refuse_above_half_free);
// What the arenas of one call may take together: the context's ceiling (max_ws), and three quarters of the card's free
// memory plus the arenas in reuse_mask - those the call is about to reuse are not free, but they are the call's to fill.
size_t r4x16_room(rans4x16_hip_ctx *c, unsigned reuse_mask);
void r4x16_trim(rans4x16_hip_ctx *c, size_t keep);
// stream ordering of a context's arenas (workspace, stripe arena) between calls on different streams: r4x16_api.hip
int r4x16_ws_order_begin(rans4x16_hip_ctx *c, hipStream_t s);
int r4x16_ws_order_end(rans4x16_hip_ctx *c, hipStream_t s);
// route read-out: a copy of `words` device counters of list `which` behind what `s` holds, folded when the route is read
int r4x16_route_snap(rans4x16_hip_ctx *c, int which, const u32 *d_cnt, u32 words, hipStream_t s);
int r4x16_stripe_compress_dev(rans4x16_hip_ctx *c, int n, const BatchArgs &a, int order, uint32_t max_in_size, hipStream_t s);
// best-of-k and X_STRIPE under per-block orders (r4x16_best.hip); what they ask of r4x16_api.hip
int r4x16_orders_stripe_compress_dev(rans4x16_hip_ctx *c, int n, const BatchArgs &a, uint32_t max_in_size, uint64_t total_in_size,
                                     hipStream_t s);
size_t r4x16_enc_ws_bytes(size_t nitems, u32 max_in_size, u64 total_in);
int r4x16_stripe_uncompress_dev(rans4x16_hip_ctx *c, int n, const BatchArgs &a, uint32_t max_in_size, uint32_t max_out_cap,
                                uint32_t max_stripe_out, hipStream_t s);
// the packed calls (r4x16_packed.hip): the internal bound-sized slots of a chunk of blocks in the context's packed arena,
// and the plain encode pipeline of r4x16_api.hip with either finish (pk == nullptr: into the caller's slots)
struct PackedSlots { u64 *slot_off; u32 *slot_cap; u8 *slots; u64 stride; };     // slot_off / slot_cap: [n], block i in slot i % chunk
size_t r4x16_packed_carve(PackedSlots *p, u8 *base, size_t n, size_t chunk, u64 stride);
u64 r4x16_packed_stride(u32 max_in_size, int order, bool any_order);
void r4x16_launch_packed_slots(const BatchArgs *a, const PackedSlots *p, int n, size_t chunk, u32 max_in_size, hipStream_t s);
int r4x16_enc_run(rans4x16_hip_ctx *c, BatchArgs a, uint32_t max_in_size, uint64_t total_in_size, hipStream_t s, const PackedOut *pk);
// rans4x16_hip_tok3_pack_dev's body (r4x16_tok3.hip), with what rans4x16_hip_tok3_encode_names_dev adds: the blocks its
// tokeniser refused (d_pre, [nblk] or nullptr), and a column count that lies on the device at d_blk_first[nblk]
// (n_on_device: n is the room of the directory, the entries behind the count have size 0)
int r4x16_tok3_pack_run(rans4x16_hip_ctx *c, int nblk, int n, const uint32_t *d_blk_first,
                        const unsigned char *d_in, const uint64_t *d_col_off, const uint32_t *d_col_size,
                        const int32_t *d_col_id, const uint32_t *d_last_start, const uint32_t *d_nreads,
                        unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                        uint32_t *d_out_size, int32_t *d_status,
                        int k, const int *methods, int32_t *d_chosen,
                        uint32_t max_col_size, uint64_t total_col_size, const int32_t *d_pre, bool n_on_device, hipStream_t stream);
// the names arena of the two one-call tok3 forms under given limits (r4x16_tok3_enc.hip, r4x16_tok3_names.hip), and the
// context behind the drop-in symbols of the calling thread (r4x16_api.hip): what the host-buffer names calls
// (r4x16_tok3_host.hip) plan and run with
size_t r4x16_tok3_tokenise_need(int nblk, u32 max_in_size, u32 max_names, u32 max_name_len, u64 total_in_size);
size_t r4x16_tok3_decode_names_need(int nblk, u32 max_columns, u32 max_names, u32 max_tokens, u64 col_bytes);
rans4x16_hip_ctx *r4x16_thread_ctx();
// device memory a thread's context keeps between single-block calls; a call that needed more gives it back
#define SINGLE_CALL_KEEP ((size_t)1 << 30)
// rANS 4x8: the encode pipeline of r4x16_api.hip over a batch in chunks.  pk == nullptr && sel == nullptr: the slot call.
// pk: results back to back at pk->out + pk->off[i].  sel: best-of-k, k <= 2 candidates per block (sel->k == 0: one, the
// call's order / d_order), the winner into the caller's slot (pk == nullptr) or the dense arena.
struct Enc8Sel { int k; int m[2]; i32 *d_chosen; };
int r4x8_enc_run(rans4x16_hip_ctx *c, BatchArgs a, uint32_t max_in_size, hipStream_t s, const PackedOut *pk, const Enc8Sel *sel);
int r4x16_run_host_batch(rans4x16_hip_ctx *c, int n, bool decode,
                          const unsigned char *const *in, const unsigned int *in_size,
                          unsigned char *const *out, unsigned int *out_size, const int *order, int *status);
// The host-buffer calls' staging arena (A_STAGE, laid out by r4x16_stage.h; r4x16_host.hip).  begin: the arena for a batch
// of `items`, and the host arrays on their way up on `s` in this order (order == nullptr: the layout has no order array).
// verdicts: the result sizes and statuses back in osz / status, and `s` waited for.  Payload moves at each site's own.
struct StageArrays { const u64 *in_off, *out_off; const u32 *in_size, *cap; const i32 *order; };
int r4x16_stage_begin(rans4x16_hip_ctx *c, StageLayout *L, size_t items, size_t in_bytes, size_t plane_bytes, size_t out_bytes,
                      size_t pk_count, const StageArrays &h, hipStream_t s);
int r4x16_stage_verdicts(rans4x16_hip_ctx *c, const StageLayout &L, size_t items, u32 *osz, i32 *status, hipStream_t s);
// How every codec's device calls start and walk their batch (the tok3 calls and the single-shot stripe calls apart), and
// what rides on them.
// args: the start of a slot call - the context and the eight slot arguments tested (`ok`: what else the call requires),
// `check` run where the call has one (its method table: check leaves its own text in err), n == 0 answered, the device
// set, BatchArgs filled.  -1: refused, err = `bad` or check's; 0: n == 0, nothing to do; 1: go on.
int r4x16_dev_call_args(rans4x16_hip_ctx *c, const char *bad, bool ok, BatchArgs *a, int n, const u8 *d_in, const u64 *d_in_off,
                        const u32 *d_in_size, u8 *d_out, const u64 *d_out_off, const u32 *d_out_cap, u32 *d_out_size, i32 *d_status,
                        int order, const i32 *d_order, const std::function<int()> &check = {});
// The same for a packed call, whose results lie back to back at d_out + d_out_off[i]: d_out_off is required whatever n
// is, d_out may be null with capacity 0 (the sizing pass).  check, then the device set; n == 0 zeroes d_out_off[0] on `s`.
// BatchArgs filled but for out / out_off / out_cap (null: the route sets them), and *pk.
int r4x16_packed_call_args(rans4x16_hip_ctx *c, const char *bad, bool ok, BatchArgs *a, PackedOut *pk, int n, const u8 *d_in,
                           const u64 *d_in_off, const u32 *d_in_size, u8 *d_out, u64 out_capacity, u64 *d_out_off, u32 *d_out_size,
                           i32 *d_status, int order, const i32 *d_order, hipStream_t s, const std::function<int()> &check = {});
// walk: n blocks in chunks of `chunk` (what the caller's plan fitted), fewer where grab(nb) - r4x16_ensure on every arena a
// chunk of nb blocks takes, 0 or -1 - cannot have them for as many, ordered on the context's arenas before and behind:
// run(base, nb) enqueues one chunk, 0 or -1 (the walk ends there, the order left open).  The first chunk is a full one:
// a call that lays its arenas out once does so in run at base == 0, where nb is the chunk size the back-off ended on, and
// enqueues its once-per-call work there.
// r4x16_chunk_walk is a template over its two callables and needs the context's members: it stands at the end of this file.
// The route counters of one chunk of launches.  begin: zeroed on `s` - or, option route_count off, *kernels = nullptr: the
// kernels count nothing.  end (d_cnt: the counters, not the kernels' copy): read out into list `which`, the chunk counted
// as launched in order.
int r4x16_route_begin(rans4x16_hip_ctx *c, u32 **kernels, u32 words, hipStream_t s);
int r4x16_route_end(rans4x16_hip_ctx *c, int which, const u32 *d_cnt, u32 words, hipStream_t s);
// fqzcomp_qual encoding (r4x16_fqz_enc.hip): what the call takes beside the slot arguments, the arena bytes of a chunk of nb
// blocks, and one chunk's front / encode / back stages laid out at `at` - the device call's, and what the one-call form
// with the pick in front (r4x16_fqz_pick.hip) runs behind its pick.  (r4x16_fqz_best.h: the same without the back end.)
struct FqeIn {
    const u8 *par; const u64 *par_off; const u32 *par_size;
    const u32 *len, *flags; const u64 *rec_off; const u32 *nrec;
    const u64 *len_off;     // where a block's lengths start, if not at rec_off (nullptr): several blocks may share one list
};
size_t r4x16_fqe_chunk_bytes(rans4x16_hip_ctx *c, size_t nb, u32 max_in_size, u32 max_records);
int r4x16_fqe_chunk(rans4x16_hip_ctx *c, const BatchArgs &a, const FqeIn &in, u8 *at, int base, int nb, u32 max_in_size, u32 max_params_size,
                    u32 max_records, hipStream_t s);
// the device pick with the lengths' way back (r4x16_fqz_pick.hip): rans4x16_hip_fqz_compress_pick_dev, and d_len_out
// (may be null) for the host-buffer batch
int r4x16_fqz_compress_pick_run(rans4x16_hip_ctx *c, int n, const u8 *d_in, const u64 *d_in_off, const u32 *d_in_size, const u32 *d_len,
                                const u32 *d_flags, const u64 *d_rec_off, const u32 *d_nrec, int vers, int strat, const i32 *d_strat,
                                u8 *d_out, const u64 *d_out_off, const u32 *d_out_cap, u32 *d_out_size, i32 *d_status, u32 *d_len_out,
                                u32 max_in_size, u32 max_records, hipStream_t s);
// One round trip of a host-buffer batch of these coders: the taken blocks' bytes in one upload (slots of the size rounded
// up to 16 - a block that is not taken has size and capacity 0 and takes none - and up_tail behind them), the device
// call on the staged layout, one download (the outputs, and down_tail bytes behind them, handed back in *down_tail), the
// verdicts, and every taken block's status, size and bytes to the caller's arrays.  What the caller's walk said of a block
// it did not take stays, and that block's buffer is not written.  Returns the blocks whose status is not 0: n without
// touching the device where none is taken; -1 where the call itself failed.
struct HostTrip {
    const unsigned char *const *in; unsigned char *const *out;
    unsigned int *out_size; int *status;
    const u8 *take; const u32 *isz, *cap; const i32 *order;         // [n]; order: nullptr where the call takes none
    const void *up_tail; size_t up_tail_bytes;
    size_t down_tail_bytes; std::vector<u8> *down_tail;
};
// call(L, in_total, out_total, s): the device call; the tails lie at L.in + in_total and L.out + out_total
typedef std::function<int(const StageLayout &, size_t, size_t, hipStream_t)> HostTripCall;
int r4x16_host_trip(rans4x16_hip_ctx *c, int n, const HostTrip &t, const HostTripCall &call);
// one staging pass (copy in, the device calls, sizes back, copy out) on the context's stream; x8: the rANS 4x8 calls
int r4x16_run_slab(rans4x16_hip_ctx *c, int n, bool decode, bool x8,
                   const unsigned char *const *in, const unsigned int *in_size,
                   unsigned char *const *out, unsigned int *out_size, const int *order, int *status);

struct rans4x16_hip_ctx {
    int device = 0;
    std::string err;
    R4Opts opts = {};                       // rans4x16_hip_set_option; defaults from the environment, read once per process
    struct { u8 *p = nullptr; size_t bytes = 0; } arena[A_COUNT];
    u8 *at(R4Arena a) const { return arena[a].p; }
    double *logtab = nullptr;
    u32 *rcptab = nullptr;
    // timing hook
    int timing = 0;
    std::vector<TimedLaunch> timed[2];
    size_t max_ws = (size_t)160 << 30;       // ceiling for one chunk of blocks (r4x16_room also looks at free memory)
    // X_STRIPE in the device-resident calls (r4x16_stripe.hip): how many planes a device-resident decode batch reserves
    // per block (0: stripe blocks report UNSUPPORTED there)
    int dev_stripe_planes = 0;
    unsigned int dev_stripe_out = 0;        // largest uncompressed stripe block such a batch may hold
    int dev_stripe_enc = 0;                 // encode with per-block orders: planes a block reserves (rans4x16_hip_set_dev_stripe_encode)
    bool in_stripe = false;                 // inside the recursive call over the internal items
    bool in_packed = false;                 // inside a packed call's slot call over its internal slots (r4x16_packed.hip)
    int tok3_arith = 0;                     // tok3 calls: R4X16_TOK3_ARITH_* (rans4x16_hip_set_tok3_arith); 0: the rANS flavour alone
    int fqz_pick = 0, fqz_guard_bits = 0;   // fqzcomp_qual encoding: 1: host batches pick on the device; the guard times 2^guard_bits (rans4x16_hip_set_fqz_pick)
    int fqz_slots = 0, fqz_max_sym = 255;   // fqzcomp_qual: model slots in flight at most (0: 1024), the largest max_sym a slot holds (rans4x16_hip_set_fqz_limits)
    int names_chunk_blocks = 0;             // host-buffer names batches: blocks per chunk at most (rans4x16_hip_set_names_chunk_blocks)
    // calls on different streams are ordered on the one workspace through this event
    hipEvent_t ws_done = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_busy = false;
    // side streams for the class launches of small batches (created at first use)
    R4Fork fork = {};
    bool fork_made = false;
    SchedHint hint[2] = {};    // [0] encode, [1] decode: the last batch's work per class (pinned; r4x16_sched.h)
    bool no_fork = false;                   // a lane of the host pipeline: the lanes are its concurrency (one priority each)
    // host-buffer batches: this context's own stream, and the lane contexts large batches are pipelined over
    hipStream_t stream = nullptr;
    struct HostPipe *pipe = nullptr;
    // route read-out (rans4x16_hip_route_read): counts folded so far, and the launches' copies not yet folded
    long route[ROUTE_WHICH][ROUTE_KINDS] = {};
    std::vector<RouteSnap> route_pending;
};

// a host buffer as the header walks read it (r4x16_arith_parse.h, r4x16_fqz_parse.h).  (r4x16_tok3_scan.hip has one of its
// own in an anonymous namespace: that unit compiles without any HIP header and cannot include this one.)
struct HostSrc { const u8 *p; u8 at(u32 i) const { return p[i]; } };

// A setting of the context for one call made on the caller's behalf: set here, and the caller's own put back when the
// scope ends, whichever way it ends.
template <class T> struct Keep {
    T &field; T was;
    Keep(T &f, T v) : field(f), was(f) { f = v; }
    ~Keep() { field = was; }
    Keep(const Keep &) = delete;
    Keep &operator=(const Keep &) = delete;
};
// the X_STRIPE limits of the device-resident decode calls (rans4x16_hip_set_dev_stripe_planes)
struct StripeLimits {
    Keep<int> planes; Keep<unsigned int> out;
    StripeLimits(rans4x16_hip_ctx *c, int planes_, unsigned int out_) : planes(c->dev_stripe_planes, planes_), out(c->dev_stripe_out, out_) {}
};

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return -1;                                                                      \
        }                                                                                   \
    } while (0)

template <class Grab, class Run>
static inline int r4x16_chunk_walk(rans4x16_hip_ctx *c, int n, size_t chunk, hipStream_t s, Grab grab, Run run)
{
    if (r4x16_ws_order_begin(c, s) != 0) return -1;
    if (r4x16_backoff(chunk, grab) != 0) return -1;
    for (size_t base = 0; base < (size_t)n; base += chunk)
        if (run(base, (int)std::min(chunk, (size_t)n - base)) != 0) return -1;
    HIPCHK(c, hipGetLastError());
    return r4x16_ws_order_end(c, s);
}
