/*
 * rans4x16_hip.h — C ABI of librans4x16_hip.so: the MI355X (gfx950) implementation of the
 * CRAM 3.1 rANS 4x16 codec, bit-exact with htscodecs 1.1.
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 *  1. The five entry points of htscodecs/rANS_static4x16.h:41-50, same names, same argument
 *     meaning, same ownership and error rules.  A program linked against
 *     libhtscodecs can be re-linked against this library for this codec without source changes.
 *     Buffers are HOST memory; each call stages through the GPU as a batch of one.
 *
 *  2. Batch entry points — the shape of the reference's own benchmark loop
 *     (tests/rANS_static4x16pr_test.c:191-206: a serial loop of rans_compress_to_4x16 /
 *     rans_uncompress_to_4x16 over independent blocks), which is what a GPU needs to be fed.
 *     *_batch take host buffers; *_dev take device-resident buffers (no PCIe in the call),
 *     enqueue on a caller-supplied HIP stream and do not synchronise.
 *
 * All GPU work is done by hand-written HIP kernels; there is no CPU fallback.  If no usable
 * GPU is present every entry point fails (NULL / negative return) and says why on stderr once.
 */
#ifndef RANS4X16_HIP_H
#define RANS4X16_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#pragma GCC visibility push(default)

/* ---- 1. drop-in replacements (htscodecs/rANS_static4x16.h:41-50) ------------------------- */

/* rANS_static4x16pr.c:360-372.  Pure host arithmetic. */
unsigned int rans_compress_bound_4x16(unsigned int size, int order);

/* rANS_static4x16pr.c:1138-1345.  out==NULL: malloc'd result (caller frees); else *out_size is
 * the capacity on entry (must be >= rans_compress_bound_4x16(in_size, order), otherwise NULL)
 * and the produced size on return.  order: bit0 order-1, 0x80 PACK, 0x40 RLE, 0x20 CAT,
 * 0x10 NOSZ, 0x08 STRIPE, bits 8..15 stripe count. */
unsigned char *rans_compress_to_4x16(unsigned char *in, unsigned int in_size,
                                     unsigned char *out, unsigned int *out_size, int order);
/* rANS_static4x16pr.c:1347-1350 */
unsigned char *rans_compress_4x16(unsigned char *in, unsigned int in_size,
                                  unsigned int *out_size, int order);
/* rANS_static4x16pr.c:1352-1636.  NULL on any malformed input. */
unsigned char *rans_uncompress_to_4x16(unsigned char *in, unsigned int in_size,
                                       unsigned char *out, unsigned int *out_size);
/* rANS_static4x16pr.c:1638-1641 */
unsigned char *rans_uncompress_4x16(unsigned char *in, unsigned int in_size,
                                    unsigned int *out_size);

/* ---- 2. batch interface ------------------------------------------------------------------ */

typedef struct rans4x16_hip_ctx rans4x16_hip_ctx;

/* Per-block status codes written to the status arrays (0 = success). */
enum {
    R4X16_OK            = 0,
    R4X16_E_CAPACITY    = 1,   /* output capacity too small (encode: < bound; decode: < stored size) */
    R4X16_E_TRUNCATED   = 2,   /* input ends inside a header, table or state words               */
    R4X16_E_TABLE       = 3,   /* frequency table does not sum to a power of two / overflows      */
    R4X16_E_STATE       = 4,   /* initial rANS state below 2^15                                   */
    R4X16_E_SIZE        = 5,   /* inconsistent size fields (pack / rle / cat)                     */
    R4X16_E_UNSUPPORTED = 6,   /* valid-looking stream this build does not handle */
    R4X16_E_CONTEXT     = 7,   /* order-1 stream used a context that has no table row             */
    R4X16_E_RLE         = 8,   /* run-length expansion overran the output                         */
    R4X16_E_EMPTY       = 9,   /* zero-length compressed input                                    */
    R4X16_E_UNDECIDED   = 10   /* fqz pick on the device: a decision too close to call (part 2k)  */
};

/* One context per (host thread, device).  device < 0 selects the current HIP device.
 * Returns NULL if the device or the code object is unusable. */
rans4x16_hip_ctx *rans4x16_hip_create(int device);
void              rans4x16_hip_destroy(rans4x16_hip_ctx *ctx);
const char       *rans4x16_hip_last_error(const rans4x16_hip_ctx *ctx);

/* Host-buffer batches: n independent blocks, semantics of n calls of the functions in part 1
 * with caller-provided output buffers (out[i] != NULL, out_size[i] = capacity in / size out).
 * Returns the number of failed blocks (their out_size[i] is set to 0 and status[i] != 0 if
 * status is not NULL), or -1 if the batch could not be run at all.
 * An X_STRIPE block that fails on decode reports what rans4x16_hip_uncompress_dev reports for it: CAPACITY where the
 * stored size is not out_size[i] (:1379), SIZE for an inconsistent header, else the status of its first failing plane
 * (UNSUPPORTED for a plane that is itself a stripe stream; CONTEXT / RLE in the stricter cases above). */
int rans4x16_hip_compress_batch(rans4x16_hip_ctx *ctx, int n,
                                const unsigned char *const *in, const unsigned int *in_size,
                                unsigned char *const *out, unsigned int *out_size,
                                const int *order, int *status);
int rans4x16_hip_uncompress_batch(rans4x16_hip_ctx *ctx, int n,
                                  const unsigned char *const *in, const unsigned int *in_size,
                                  unsigned char *const *out, unsigned int *out_size,
                                  int *status);

/* "Try k methods, keep the smallest": the caller-side pattern of htscodecs/tokenise_name3.c:1246-1300
 * (compress(): up to nine `order` values per token column, smallest kept) and of CRAM block writers, as one
 * call.  Block i is encoded with every methods[j]; out[i] receives the smallest result, chosen[i] the
 * method that produced it (the first wins ties, tokenise_name3.c:1283-1286; -1 if every candidate
 * failed).  Methods with X_STRIPE (0x08) are skipped for blocks whose size is not a multiple of 4
 * (:1271-1272).  out_size[i] is the capacity on entry (at least the largest
 * rans_compress_bound_4x16(in_size[i], methods[j])) and the winner's size on return.
 * The candidates share one upload of the block; only the winner is copied back.
 * Returns the number of blocks without any successful candidate, or -1. */
int rans4x16_hip_compress_best_batch(rans4x16_hip_ctx *ctx, int n,
                                     const unsigned char *const *in, const unsigned int *in_size,
                                     unsigned char *const *out, unsigned int *out_size,
                                     int k, const int *methods, int *chosen, int *status);

/* Device-resident batches.  Every pointer below is a DEVICE pointer.
 *   d_in  + d_in_off[i]   : block i input,  d_in_size[i] bytes
 *   d_out + d_out_off[i]  : block i output slot, d_out_cap[i] bytes available
 *   d_out_size[i]         : bytes produced (0 on failure);  d_status[i]: code above
 * `order` applies to all blocks unless d_order != NULL (device array of n ints).
 * max_in_size / max_out_cap are host-side upper bounds on the per-block sizes, used only to
 * size the workspace (no device->host read-back happens inside these calls).  For decode, max_out_cap sizes
 * the stage buffers of X_PACK / X_RLE blocks only: it may be the largest output of THOSE blocks, 0 if the batch
 * has none (a transformed block larger than that reports UNSUPPORTED).
 * `stream` is a hipStream_t (NULL = default stream).  The call only enqueues work.
 * X_STRIPE (0x08), device-resident: encode accepts it when all blocks share one `order` (d_order == NULL): the
 * planes, the N x K candidate encodings, the choice of the smallest per plane and the header are all produced on the
 * device (rANS_static4x16pr.c:1154-1216); with per-block orders a stripe block is encoded the same way after
 * rans4x16_hip_set_dev_stripe_encode (below) and reports UNSUPPORTED without it.  Decode accepts
 * stripe blocks after rans4x16_hip_set_dev_stripe_planes (below); without it they report UNSUPPORTED.  The host
 * entry points handle stripes in every case.
 * Returns 0 if enqueued, -1 on argument / allocation / launch errors. */
int rans4x16_hip_compress_dev(rans4x16_hip_ctx *ctx, int n,
                              const unsigned char *d_in, const uint64_t *d_in_off,
                              const uint32_t *d_in_size,
                              unsigned char *d_out, const uint64_t *d_out_off,
                              const uint32_t *d_out_cap, uint32_t *d_out_size,
                              int32_t *d_status, int order, const int32_t *d_order,
                              uint32_t max_in_size, void *stream);
int rans4x16_hip_uncompress_dev(rans4x16_hip_ctx *ctx, int n,
                                const unsigned char *d_in, const uint64_t *d_in_off,
                                const uint32_t *d_in_size,
                                unsigned char *d_out, const uint64_t *d_out_off,
                                const uint32_t *d_out_cap, uint32_t *d_out_size,
                                int32_t *d_status, uint32_t max_in_size, uint32_t max_out_cap,
                                void *stream);

/* The same calls with one more host-side figure, the SUM of the blocks' sizes: the workspace a block needs for
 * X_PACK / X_RLE depends on its own length, the device lays those regions out itself, and the host only has to bound
 * their total - total_in_size (encode: sum of d_in_size) / total_out_cap (decode: sum of d_out_cap over the blocks
 * that carry X_PACK or X_RLE; the sum over all blocks is a valid bound) instead of n x the largest block.  A batch of
 * 22,729 blocks of 4 KiB .. 1 MiB (4 GiB) then takes 29 GB of workspace instead of 62.  0 = unknown
 * (the plain calls above).  A batch that holds more than it announced fails the blocks that do not fit (UNSUPPORTED). */
int rans4x16_hip_compress_dev_sized(rans4x16_hip_ctx *ctx, int n,
                                    const unsigned char *d_in, const uint64_t *d_in_off,
                                    const uint32_t *d_in_size,
                                    unsigned char *d_out, const uint64_t *d_out_off,
                                    const uint32_t *d_out_cap, uint32_t *d_out_size,
                                    int32_t *d_status, int order, const int32_t *d_order,
                                    uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_uncompress_dev_sized(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *d_in, const uint64_t *d_in_off,
                                      const uint32_t *d_in_size,
                                      unsigned char *d_out, const uint64_t *d_out_off,
                                      const uint32_t *d_out_cap, uint32_t *d_out_size,
                                      int32_t *d_status, uint32_t max_in_size, uint32_t max_out_cap,
                                      uint64_t total_out_cap, void *stream);

/* Device-resident decode of X_STRIPE blocks: the flag and the plane count N live in the stream, so the host cannot
 * size the workspace per block; this sets what every block of later rans4x16_hip_uncompress_dev calls reserves:
 * `planes` internal sub-blocks (the default N is 4) and a plane buffer of `max_block_size` bytes.  A stripe block
 * with more planes, or larger than that, reports UNSUPPORTED; like the reference (:1379) a stripe block must be given
 * an output capacity equal to its stored size.  planes == 0 (the default) switches it off.  Returns 0, -1 on bad arguments. */
int rans4x16_hip_set_dev_stripe_planes(rans4x16_hip_ctx *ctx, int planes, unsigned int max_block_size);

/* Device-resident encode of X_STRIPE blocks under per-block orders (d_order != NULL): N and the candidate methods of a
 * block are then known to the device only, so every block of such a call reserves max_planes x 4 internal items.
 * A stripe block with N <= max_planes is encoded byte for byte like rans_compress_to_4x16(.., d_order[b]); one with more
 * planes reports UNSUPPORTED and leaves its neighbours alone; blocks without the flag, and blocks of at most 20 bytes,
 * are encoded with their own order as before.  max_planes 0..255; 0 (the default) switches it off: a stripe block under
 * d_order reports UNSUPPORTED.  Calls with one `order` for all blocks are not affected.
 * Cost: the plane count of a block is not known to the host, so the reservation is made for the worst case - per block
 * four output slots of a whole block's bound and max_planes x 4 - 4 slots of half a block's bound (each at least the
 * 198 KB of an order-1 table), and as many items of workspace.  Set max_planes to the largest N the batches really
 * use (4 for the default N), not to 255.  Returns 0, -1 on bad arguments. */
int rans4x16_hip_set_dev_stripe_encode(rans4x16_hip_ctx *ctx, int max_planes);

/* rans4x16_hip_compress_best_batch for device-resident blocks: the arrays of rans4x16_hip_compress_dev_sized, the
 * semantics of the host call.  Block i is encoded with methods[0..k) (a HOST array, 1 <= k <= 32) in that order and
 * d_out + d_out_off[i] receives exactly the bytes of rans_compress_to_4x16(in, size, .., methods[j]) for the smallest
 * result; of equal sizes the earlier method wins (tokenise_name3.c:1281-1284).  d_chosen[i] (device, may be NULL) is that
 * methods[j] as given, -1 if no candidate succeeded.
 *   - A method with X_STRIPE (0x08) is skipped for a block whose size is no multiple of 4 (:1270-1271); on a block of at
 *     most 20 bytes it is a plain encode with the flag dropped (rANS_static4x16pr.c:1151).
 *   - A candidate that fails is skipped: one whose own rans_compress_bound_4x16(size, methods[j]) exceeds d_out_cap[i]
 *     (CAPACITY).  The block fails only if no candidate succeeded: d_out_size[i] = 0, d_chosen[i] = -1 and
 *     d_status[i] is the status of the first candidate that was tried, UNSUPPORTED if none was.  Other blocks are not affected.
 *   - A stripe method with more than 255 planes (methods[j] >> 8) makes the call return -1.
 * The choice is made on the device: the call only enqueues on `stream`, reads nothing back and does not synchronise; it
 * is ordered against the context's other calls like every *_dev call.  Every candidate is encoded in full into a
 * bound-sized slot of an internal arena (a stripe method as N x K plane encodings, the planes transposed once per
 * distinct N); the batch is walked in chunks of blocks so that this arena and the workspace together stay under the
 * option max_workspace_mb.  max_in_size / total_in_size (0 = unknown) as in rans4x16_hip_compress_dev_sized.
 * As with the workspace of every *_dev call, the arena grows on demand and is kept: a call that has to enlarge it (the
 * first one, or a larger batch) waits for the device once while it reallocates, and what a large call allocated stays
 * with the context until it is destroyed - max_workspace_mb bounds what one call plans for, not what earlier calls left.
 * Returns 0 if enqueued, -1 on argument / allocation / launch errors. */
int rans4x16_hip_compress_best_dev(rans4x16_hip_ctx *ctx, int n,
                                   const unsigned char *d_in, const uint64_t *d_in_off,
                                   const uint32_t *d_in_size,
                                   unsigned char *d_out, const uint64_t *d_out_off,
                                   const uint32_t *d_out_cap, uint32_t *d_out_size,
                                   int32_t *d_status, int k, const int *methods, int32_t *d_chosen,
                                   uint32_t max_in_size, uint64_t total_in_size, void *stream);

/* ---- 2a. packed device-resident calls -------------------------------------------------------
 * The calls above give every block a slot of its bound (an order-1 bound is 198 KB plus the data: 262,144 blocks of 4 KiB
 * need 53 GB of slots for 1 GiB of input) and need the output sizes of a decode on the host.  The packed calls produce
 * and consume ONE dense byte arena: block i's bytes at d_out + d_out_off[i], the next block right behind them.
 * d_out_off is a device array of n + 1 entries that the call WRITES; out_capacity (host) is what d_out holds.
 * All of them only enqueue on `stream`, read nothing back, are ordered against the context's other calls like every *_dev
 * call, and walk the batch in chunks under max_workspace_mb and three quarters of the free device memory.  The
 * bound-sized slots the encoder works in are the context's own (an arena of a chunk's worth, kept like the workspace).
 *
 * rans4x16_hip_compress_packed_dev: the arguments of rans4x16_hip_compress_dev_sized, with out_capacity and the written
 * d_out_off in place of the slot arrays.
 *   - The bytes of block i, d_out_size[i] and d_status[i] are what the slot call gives for a slot of exactly
 *     rans_compress_bound_4x16(d_in_size[i], order of block i) bytes: d_order, X_STRIPE with one `order`, and X_STRIPE
 *     under d_order after rans4x16_hip_set_dev_stripe_encode included.  (A block larger than max_in_size, or one whose
 *     bound exceeds that of the largest order byte with 255 planes, reports UNSUPPORTED.)
 *   - d_out_off[0] = 0 and d_out_off[i + 1] = d_out_off[i] + the size of block i, a block that failed to encode counting
 *     0.  The sums are taken BEFORE the capacity rule: d_out_off[n] is the capacity the batch needs even if it did not fit.
 *   - Capacity rule: a block with d_out_off[i + 1] > out_capacity reports R4X16_E_CAPACITY with size 0 and nothing of it
 *     is written; its neighbours are not affected.  No byte at or beyond out_capacity and no byte outside the blocks'
 *     ranges is written.
 *   - Routes (R4X16_ROUTE_RESULT below): without stripe machinery - one `order` without X_STRIPE, or d_order with
 *     rans4x16_hip_set_dev_stripe_encode off - every stream is assembled at its final place (dense: each result byte
 *     moves once); where the stripe routes run, the blocks are encoded into the internal slots and copied out (gathered).
 *
 * rans4x16_hip_compress_best_packed_dev: rans4x16_hip_compress_best_dev with the same substitution.  A candidate is
 * tried when its own bound fits the internal slot, which holds the largest bound of the methods - every candidate the
 * slot call tries with full capacity; skip rules, tie rule and d_chosen as there.  Gathered route.
 *
 * rans4x16_hip_peek_dev: per block d_format[i] = the first byte of the stream (-1 if there is none) and d_raw_size[i] =
 * the stored uncompressed size - the varint at byte 1, present for X_STRIPE streams and for streams without X_NOSZ
 * (rANS_static4x16pr.c:1360-1366, :1435-1448) - or 0xFFFFFFFF where the stream carries none.  d_status[i]: R4X16_E_EMPTY
 * for a zero-length block, R4X16_E_TRUNCATED where the varint runs past the block, R4X16_E_UNSUPPORTED for a block
 * larger than max_in_size (it is not read).
 *
 * rans4x16_hip_uncompress_packed_dev: the input arrays of rans4x16_hip_uncompress_dev; the output sizes come from the
 * streams themselves.
 *   - Every block claims its stored size (as peek reads it); an X_NOSZ block claims d_nosz_size[i] (device array, may be
 *     NULL: such a block then reports R4X16_E_SIZE and takes 0 bytes).  A claim above max_out_size is hostile or
 *     unannounced: the block reports R4X16_E_UNSUPPORTED and takes 0 bytes; so does what peek refuses, with its status.
 *   - d_out_off is the exclusive scan of the claimed sizes, d_out_off[n] their total.  A block whose range ends beyond
 *     out_capacity reports R4X16_E_CAPACITY and is not decoded.
 *   - The other blocks are decoded with a capacity of exactly the claimed size - what X_STRIPE blocks need (:1379; they
 *     are decoded after rans4x16_hip_set_dev_stripe_planes, as in the slot call).  A block that fails while decoding keeps
 *     its range, reports size 0, and the bytes inside its own range are unspecified.  Nothing outside the ranges is written.
 *   - max_out_size also sizes the stage buffers of X_PACK / X_RLE blocks (max_out_cap of the slot call).
 * Returns 0 if enqueued, -1 on argument / allocation / launch errors. */
int rans4x16_hip_compress_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                     const unsigned char *d_in, const uint64_t *d_in_off,
                                     const uint32_t *d_in_size,
                                     unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                     uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                     uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_compress_best_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                          const unsigned char *d_in, const uint64_t *d_in_off,
                                          const uint32_t *d_in_size,
                                          unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                          uint32_t *d_out_size, int32_t *d_status,
                                          int k, const int *methods, int32_t *d_chosen,
                                          uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_peek_dev(rans4x16_hip_ctx *ctx, int n,
                          const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                          int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status,
                          uint32_t max_in_size, void *stream);
int rans4x16_hip_uncompress_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                       const unsigned char *d_in, const uint64_t *d_in_off,
                                       const uint32_t *d_in_size,
                                       unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                       uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                       uint32_t max_in_size, uint32_t max_out_size, void *stream);

/* ---- 2c. tok3 column containers ---------------------------------------------------------------
 * The CRAM 3.1 name tokeniser (htscodecs tokenise_name3.c) turns a block of read names into token columns, compresses
 * each with the best of a method list and frames them into one container (encode_names, :1431-1531); decode_names
 * (:1546-1669) walks the container and decodes the columns before it rebuilds the names.  These calls do the column
 * half of both on the device - the rANS flavour (use_arith = 0), and the arith flavour (use_arith = 1, the streams are
 * arith_dynamic's, parts 2g and 2h) after rans4x16_hip_set_tok3_arith, below; part 2d turns the decoded columns into names
 * (decode_name), part 2e the names into the columns this part packs (the encoding tokeniser: trie, encode_name).
 *
 * A container: last_start (4 bytes, little endian), nreads (4), use_arith (1), then per column a type byte
 * (type | 128 on the first column of a token position, | 64 for a duplicate) followed by var_put_u32(clen) and the
 * rANS 4x16 stream, or - duplicate - by id >> 4, id & 15 of the earlier column it repeats.  A column's id is
 * tnum << 4 | type, tnum below 128.
 *
 * rans4x16_hip_tok3_scan: walks one container in HOST memory.  Pure host arithmetic, usable without a GPU, like
 * rans4x16_hip_partition.  Reports the header's last_start and nreads, the number of descriptors, the number of columns
 * they give (descriptors plus synthesised type columns, below), the total and the largest column size and the largest
 * stream (any of the pointers may be NULL), and returns 0 or the R4X16_E_* status the walk of
 * rans4x16_hip_tok3_unpack_dev gives with the same max_columns / max_col_size (0 = no limit: 2048 / 2^32 - 1); -1 on bad
 * arguments.  After a failure the counts and sizes are those of the columns accepted before it.
 * rans4x16_hip_tok3_scan_any: the same walk, which accepts either flavour - use_arith != 0 is not refused - and reports
 * byte 8 != 0 in *use_arith (may be NULL; 0 where the container has no byte 8).  Pure host arithmetic too.
 *
 * rans4x16_hip_set_tok3_arith(ctx, mode): the arith flavour (tokenise_name3.c with use_arith = 1: :1246-1300 swaps
 * rans_compress_to_4x16 for arith_compress_to, :1314-1321 the decoder, :1511 writes the flag) for the tok3 calls of parts
 * 2c to 2f on this context.  mode is 0 (the default) or a sum of
 *   R4X16_TOK3_ARITH_DECODE  unpack_dev, decode_names_dev, decode_names_batch: a container with use_arith != 0 is walked
 *                            by the same rules and its plain columns are decoded by rans4x16_hip_arith_uncompress_dev
 *                            with the claim as capacity.  The flavour is per block: one batch may mix both, and each
 *                            block's result is what it would be alone.  Nested X_STRIPE columns need
 *                            rans4x16_hip_set_dev_stripe_planes as the rANS ones do (decode_names_batch arranges it).
 *                            The decoder's in_size is the rest of the container from the stream's first byte, as the
 *                            reference hands it (:1214), not clen: the range coder starts only if more than five bytes
 *                            lie in front of its input's end (c_range_coder.h:64), and the reference's writer gives a
 *                            near-constant column a body of exactly five - such a column decodes because a descriptor
 *                            follows it (to zeros where none does, here as there).  The walk's own rule stays stricter:
 *                            a clen that reaches beyond the container is TRUNCATED.
 *   R4X16_TOK3_ARITH_ENCODE  pack_dev, encode_names_dev, encode_names_batch: byte 8 is 1 and every column's winner comes
 *                            from rans4x16_hip_arith_compress_best_packed_dev (part 2h) with the given method list; the
 *                            duplicate rule and the framing are unchanged.
 * Returns the previous mode, -1 for a NULL context or a mode outside 0..3.  A setter like
 * rans4x16_hip_set_dev_stripe_planes, not a named option.  In mode 0 the calls take the rANS path alone: no arith kernel
 * runs and R4X16_ROUTE_ARITH* stay untouched; what the text below says about use_arith != 0 being refused holds there.
 *
 * rans4x16_hip_tok3_pack_dev: nblk name blocks with n columns in all.  Every array is a DEVICE array.
 *   d_blk_first[nblk + 1]       first column of each block; d_blk_first[0] = 0, d_blk_first[nblk] = n
 *   d_in + d_col_off[i]         column i, d_col_size[i] bytes
 *   d_col_id[i]                 tnum << 4 | type; strictly ascending inside a block
 *   d_last_start, d_nreads      [nblk], the header values
 *   k, methods, d_chosen        as in rans4x16_hip_compress_best_dev, per column; a column written as a duplicate still
 *                               reports its method
 *   max_col_size, total_col_size  largest column / sum of the columns (0 = unknown), host
 *   d_out, out_capacity, d_out_off[nblk + 1], d_out_size, d_status: one dense arena as in
 *   rans4x16_hip_compress_packed_dev - offsets written by the call, sums before the capacity rule, d_out == NULL with
 *   out_capacity 0 as a sizing pass; a block that ends beyond out_capacity reports R4X16_E_CAPACITY and size 0.
 * Block b's bytes are what :1498-1531 writes: the header with use_arith = 0 (1 under R4X16_TOK3_ARITH_ENCODE), then per column the type byte and either
 * var_put_u32(clen) and the winner's stream - the winner of rans4x16_hip_compress_best_dev's rules, X_STRIPE skip and
 * first-listed-wins included - or the three bytes of a duplicate.  A column is a duplicate of the first earlier column
 * of its block whose varint + stream has the same length, more than 4 bytes, and the same bytes (:1461-1477); columns
 * that were themselves written as duplicates are candidates too; if that first match has id 0 the column is written in
 * full (the reference tests `if (dup_from)`).  d_out_size is the bytes really written (the reference's own figure comes
 * out too small after a duplicate).
 * A block with a zero-length column, with ids that do not ascend or are outside 0 .. 2047, or with an inconsistent
 * d_blk_first (first > next, next > n, a start below the start of an earlier block, d_blk_first[0] != 0 for block 0,
 * d_blk_first[nblk] != n for the last) reports
 * R4X16_E_SIZE and size 0; one with a column above max_col_size (or more bytes than total_col_size announced)
 * R4X16_E_UNSUPPORTED; one with a column that no method could encode that column's status.  Its neighbours are not
 * affected.  The call only enqueues and reads nothing back.  The columns are encoded in chunks under max_workspace_mb like
 * the packed calls; the winners of the whole batch wait in an arena of the context until their blocks are framed (about
 * 1.05 x the columns plus 800 bytes per column where the list has an order-0 method), so no block's columns are ever
 * split; a batch whose winners do not fit half of max_workspace_mb is refused with -1: split it.
 *
 * rans4x16_hip_tok3_unpack_dev: nblk containers at d_in + d_in_off[b], d_in_size[b] bytes (at most max_in_size).
 *   max_columns (1..2048)  descriptors per block the directory holds; nblk x max_columns sizes the internal decode batch
 *   max_col_size           largest column
 *   d_out, out_capacity, d_out_off[nblk + 1]: the dense arena; a block's columns lie back to back in descriptor order,
 *   a synthesised type column (below) right in front of the column whose descriptor opened its position.
 *   d_col_id / d_col_off / d_col_size [nblk x max_columns]: entry b * max_columns + c is the column of descriptor c of
 *   block b - its id, where it starts in d_out, its size (id -1, size 0 past the block's last descriptor).  An id with
 *   R4X16_TOK3_TYPE_COLUMN set says that the type column of its position (id & ~15 & 2047, nreads bytes) lies at
 *   d_col_off - nreads.
 *   d_ncol (descriptors), d_last_start, d_nreads, d_out_size (bytes of all columns), d_status [nblk].
 * The walk (the statuses are those of rans4x16_hip_tok3_scan):
 *   - fewer than 9 bytes: TRUNCATED; use_arith != 0: UNSUPPORTED unless rans4x16_hip_set_tok3_arith; last_start negative as an int or above
 *     INT_MAX - 1024: SIZE (:1555); a container above max_in_size: UNSUPPORTED, not read.
 *   - a | 128 descriptor opens the next tnum; the 128th: SIZE.  If its type is not 0 the position's type column (id
 *     tnum << 4) is synthesised first: nreads bytes, the type and then N_MATCH (10) repeated (:1581-1591, :1619-1629);
 *     nreads == 0: SIZE, nreads > max_col_size: UNSUPPORTED.  A descriptor before the first | 128: SIZE.
 *   - a duplicate needs its two bytes and one more inside the container (the reference's own test, :1570, which refuses
 *     a duplicate that is the last descriptor): else TRUNCATED; its j must be below its own id: else SIZE.  It is a
 *     copy of column j; a j that never appeared gives a column of 0 bytes.
 *   - a plain descriptor reads clen, then the stored size at the stream's byte 1 as rans4x16_hip_peek_dev does, claims
 *     that many bytes and is decoded, with in_size = clen, exactly as rans4x16_hip_uncompress_packed_dev decodes a block
 *     with that claim; a claim above max_col_size: UNSUPPORTED.
 *   Stricter than the reference, never reached by encoder output: ids that do not strictly ascend: UNSUPPORTED (this
 *   bounds the walk at 2048 descriptors); more descriptors than max_columns: UNSUPPORTED; a stream with X_NOSZ (and
 *   without X_STRIPE): SIZE; a clen that does not end, or reaches beyond the container: TRUNCATED; clen == 0: EMPTY.
 * A block fails as a whole, as the reference returns NULL: d_status is the walk's status, else R4X16_E_CAPACITY if its
 * range ends beyond out_capacity (it is not decoded), else the status of its first column that failed to decode (SIZE
 * for one that decoded to another size than it claimed, where the reference trips its assert at :1655);
 * d_ncol = 0, d_out_size = 0, its directory sizes are 0, the bytes inside its own range are unspecified (a block the walk
 * refuses has no range).  Nothing outside the ranges is written.  The call only enqueues and reads nothing back. */
#define R4X16_TOK3_TYPE_COLUMN 0x10000   /* d_col_id flag of rans4x16_hip_tok3_unpack_dev, above */
#define R4X16_TOK3_ARITH_DECODE 1
#define R4X16_TOK3_ARITH_ENCODE 2
int rans4x16_hip_set_tok3_arith(rans4x16_hip_ctx *ctx, int mode);
int rans4x16_hip_tok3_scan_any(const unsigned char *in, size_t size, uint32_t max_columns, uint32_t max_col_size,
                               uint32_t *last_start, uint32_t *nreads, uint32_t *ndesc, uint32_t *ncol,
                               uint64_t *total_col_size, uint32_t *largest_col, uint32_t *largest_stream, int *use_arith);
int rans4x16_hip_tok3_scan(const unsigned char *in, size_t size, uint32_t max_columns, uint32_t max_col_size,
                           uint32_t *last_start, uint32_t *nreads, uint32_t *ndesc, uint32_t *ncol,
                           uint64_t *total_col_size, uint32_t *largest_col, uint32_t *largest_stream);
int rans4x16_hip_tok3_pack_dev(rans4x16_hip_ctx *ctx, int nblk, int n, const uint32_t *d_blk_first,
                               const unsigned char *d_in, const uint64_t *d_col_off, const uint32_t *d_col_size,
                               const int32_t *d_col_id, const uint32_t *d_last_start, const uint32_t *d_nreads,
                               unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                               uint32_t *d_out_size, int32_t *d_status,
                               int k, const int *methods, int32_t *d_chosen,
                               uint32_t max_col_size, uint64_t total_col_size, void *stream);
int rans4x16_hip_tok3_unpack_dev(rans4x16_hip_ctx *ctx, int nblk,
                                 const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                 unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                 uint32_t *d_out_size, int32_t *d_status,
                                 uint32_t *d_ncol, uint32_t *d_last_start, uint32_t *d_nreads,
                                 int32_t *d_col_id, uint64_t *d_col_off, uint32_t *d_col_size,
                                 uint32_t max_columns, uint32_t max_in_size, uint32_t max_col_size, void *stream);

/* ---- 2d. tok3 name decoding ---------------------------------------------------------------------
 * The second half of decode_names (htscodecs tokenise_name3.c:1546-1694): the token columns of a name block become its
 * read names, NUL-separated, on the device - decode_name (:1018-1189) and the loop around it (:1671-1689).  rANS flavour
 * (use_arith = 0) unless rans4x16_hip_set_tok3_arith (part 2c); the encoding direction is part 2e.
 *
 * rans4x16_hip_tok3_names_dev: the stage.  Its inputs are what rans4x16_hip_tok3_unpack_dev wrote, DEVICE arrays all:
 *   d_cols, col_capacity         the column arena and its size in bytes; a column that does not lie inside it fails its
 *                                block with R4X16_E_SIZE, nothing outside it is read
 *   d_col_id / d_col_off / d_col_size  [nblk x max_columns], the directory, R4X16_TOK3_TYPE_COLUMN flags included
 *   d_ncol, d_last_start, d_nreads     [nblk]
 *   d_blk_status                 [nblk] or NULL (all good): a block with a non-zero entry is skipped, reports that status
 *                                and claims nothing
 *   max_names                    names per block the call is sized for (host)
 *   max_tokens                   token positions per block, 1..128 (host)
 * Its outputs are one dense arena as in the packed calls:
 *   d_out, out_capacity, d_out_off[nblk + 1]  block b's names at d_out + d_out_off[b]; the offsets are written by the call
 *                                as sums before the capacity rule; d_out == NULL with out_capacity 0 is a sizing pass.
 *                                A block's claim is its last_start (0 for a skipped block); a block that ends beyond
 *                                out_capacity reports R4X16_E_CAPACITY and size 0
 *   d_out_size, d_nnames, d_status [nblk]     bytes written (= last_start), names written, R4X16_OK or the failure
 *   d_name_start                 [nblk x max_names] or NULL: where name i of block b starts, relative to d_out_off[b];
 *                                entries [0, d_nnames[b]) of a block are written
 * Encoder output decodes byte for byte as the reference decodes it.  The rules, with the reference's lines:
 *   Framing.  A block holds as many names as its column id 0 has bytes (the reference stops when that column runs out,
 *   :1019-1027).  nreads == 0, more names than nreads, or last_start above INT_MAX - 1024: SIZE.  More token positions
 *   (largest id >> 4, plus 1) than max_tokens, or more names than max_names: UNSUPPORTED.  A column of 2^28 bytes or more:
 *   UNSUPPORTED.  A name that ends beyond last_start, or a decoded size other than last_start: SIZE (the reference uses
 *   the field as a capacity with 1,024 bytes of slack; encoder output satisfies equality, and it is what lets the arena be
 *   dense without a sizing decode).
 *   Position 0.  The type must be N_DUP (5) or N_DIFF (6): else SIZE (the reference reads a distance out of whatever
 *   column that number names).  dist: 4 bytes, little endian, of column id 5 / 6; a column that runs out: TRUNCATED;
 *   dist above the name's index, or N_DUP with dist 0: SIZE.  A N_DUP name is the bytes of name index - dist and takes
 *   its token state; it may itself be repeated and matched against.
 *   Positions 1 and up.  The type comes from column position << 4; a missing or exhausted type column, and every value
 *   outside {1, 2, 3, 7, 8, 9, 10, 11}, is N_END (:1175); no end before position min(128, positions of the block): SIZE.
 *   N_CHAR one byte; N_ALPHA the bytes up to a NUL; N_DIGITS0 the N_DZLEN byte vl and a 32-bit value written as
 *   append_uint32_fixed does; N_DIGITS a 32-bit value written as append_uint32_var does - 0 writes no byte at all
 *   (:284-302); N_DDELTA / N_DDELTA0 one byte added to the earlier name's value at that position, modulo 2^32; N_NOP
 *   nothing; N_MATCH repeats the earlier name's token of that position.  N_MATCH, N_DDELTA, N_DDELTA0 at or beyond the
 *   earlier name's end position (0 for dist 0, :1061), and N_MATCH of a N_NOP: SIZE.  A value column that runs out:
 *   TRUNCATED.  Of several failing positions of one name the lowest decides.
 *   Kept from the reference: a fixed-width value that needs more digits than vl has the byte v / 10^(vl - 1) + '0',
 *   truncated to 8 bits, in front.
 *   Stricter than the reference, never reached by encoder output: N_DDELTA on a token that is not N_DIGITS, N_DDELTA0 on
 *   one that is not N_DIGITS0: SIZE (the reference adds to whatever integer sits there); vl above 9: SIZE (the reference
 *   advances over bytes it never wrote); a N_ALPHA string without its NUL inside the column: TRUNCATED (the reference drops
 *   its last byte).  A N_CHAR of 0 or a truncated fixed-width byte of 0 stays a byte of the name, also where the name is
 *   repeated (the reference's strcpy would cut it there).
 * A block fails as a whole, as the reference returns NULL: its status, size 0, d_nnames 0; the bytes inside its own range
 * are unspecified; its neighbours are not affected.  Nothing outside the blocks' ranges is written.
 * Every name keeps 8 bytes per token position and 16 bytes of its own in a history arena of the context, laid out on the
 * device from each block's own names x positions (rounded up to 16 bytes, in batch order) and bounded on the host by
 * nblk x max_names x (8 x max_tokens + 16) and by half of max_workspace_mb; a block whose history ends beyond that
 * reports R4X16_E_UNSUPPORTED (before the capacity rule).  One wave decodes one block: a batch of few blocks leaves the chip idle.
 *
 * rans4x16_hip_tok3_decode_names_dev: decode_names as one call - rans4x16_hip_tok3_unpack_dev into a column arena of the
 * context, then the stage.  It takes the unpack's arguments and limits, the stage's outputs and limits, and
 * total_col_size: the bytes of all columns of the batch, synthesised type columns included (rans4x16_hip_tok3_scan's
 * total_col_size, summed), 0 for unknown (then nblk x max_columns x 2 x max_col_size is reserved).  A block the unpack
 * refuses - a block that ends beyond total_col_size is one, with R4X16_E_CAPACITY - reports the unpack's status.  A batch
 * whose column arena plus histories do not fit half of max_workspace_mb is refused with -1: split it.
 * Both calls only enqueue and read nothing back; -1 on bad arguments (a NULL context included). */
int rans4x16_hip_tok3_names_dev(rans4x16_hip_ctx *ctx, int nblk,
                                const unsigned char *d_cols, uint64_t col_capacity,
                                const int32_t *d_col_id, const uint64_t *d_col_off, const uint32_t *d_col_size,
                                const uint32_t *d_ncol, const uint32_t *d_last_start, const uint32_t *d_nreads,
                                const int32_t *d_blk_status,
                                unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                uint32_t *d_out_size, uint32_t *d_nnames, int32_t *d_status, uint32_t *d_name_start,
                                uint32_t max_columns, uint32_t max_names, uint32_t max_tokens, void *stream);
int rans4x16_hip_tok3_decode_names_dev(rans4x16_hip_ctx *ctx, int nblk,
                                       const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                       unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                       uint32_t *d_out_size, uint32_t *d_nnames, int32_t *d_status, uint32_t *d_name_start,
                                       uint32_t max_columns, uint32_t max_in_size, uint32_t max_col_size,
                                       uint32_t max_names, uint32_t max_tokens, uint64_t total_col_size, void *stream);

/* ---- 2e. tok3 name encoding ---------------------------------------------------------------------
 * The first half of encode_names (htscodecs tokenise_name3.c:1334-1429): a block of read names becomes the token columns
 * that rans4x16_hip_tok3_pack_dev compresses and frames - build_trie / search_trie (:507-712), encode_name (:729-1013,
 * mode 1) and the drop rule (:1406-1429), on the device.  rANS flavour (use_arith = 0) unless
 * rans4x16_hip_set_tok3_arith (part 2c).
 *
 * rans4x16_hip_tok3_tokenise_dev: nblk name blocks at d_in + d_in_off[b], d_in_size[b] bytes.  Every array is a DEVICE
 * array; the call only enqueues and reads nothing back.
 *   d_cols, col_capacity, d_cols_off[nblk + 1], d_cols_size[nblk]  one dense arena as in the packed calls: block b's columns
 *                                back to back, ids ascending, at d_cols + d_cols_off[b]; the offsets are sums before the
 *                                capacity rule; d_cols == NULL with col_capacity 0 is a sizing pass; a block that ends beyond
 *                                col_capacity reports R4X16_E_CAPACITY and size 0.  A block's columns take at most 6 x its
 *                                bytes (a lone '0' costs six: type, width, value; a name's own six - its N_DUP / N_DIFF byte,
 *                                the distance, its N_END - are paid for by its separator), so 6 x the bytes of the batch is
 *                                a capacity that needs no sizing pass
 *   d_blk_first[nblk + 1], d_col_id / d_col_off / d_col_size  what rans4x16_hip_tok3_pack_dev takes, d_col_off relative to
 *                                d_cols: the directory is dense, n = d_blk_first[nblk] entries, and needs room for
 *                                nblk x max_columns; ids ascend inside a block, no column is empty, a refused block has none
 *   d_last_start, d_nreads, d_status  [nblk]
 *   max_in_size (1 .. 16,776,960), max_names (1 .. 2^24 - 1), max_name_len (<= 16384), max_tokens (1..128), max_columns (1..2048): host limits
 *   total_in_size                the bytes of all blocks (0 = unknown: nblk x max_in_size is reserved), host
 *   search_slots                 slots of a block's table of name prefixes, rounded up to a power of two (host); 0 = sized by
 *                                the library (16 x max_names, at most 2 x max_in_size).  A block whose table fills up, and
 *                                every block with search_slots = 1, finds its earlier names by the exact search alone,
 *                                which costs names x names; the columns are the same
 * The rules, with the reference's lines:
 *   Framing (:1334-1380).  A name ends at any byte <= '\n'; nreads is the number of such bytes, last_start the offset
 *   behind the last of them; what follows it is ignored; names may be empty.
 *   The earlier name (:507-554, :621-712).  For name n of len bytes: `from` is the most recent earlier name of at least len
 *   bytes that starts with all of n, else n; p3 the same for n's first prefix_len bytes, none if n is shorter.
 *   exact = from != n && len; pnum = exact ? from : p3, and without either n - 1 (0 for the first name).  pnum == n happens:
 *   distance 0, nothing to match against.  The name is N_DUP only if exact and pnum has len bytes; an exact hit on a
 *   longer name is N_DIFF against that name.  prefix_len, is_fixed and fixed_len are :632-670's four formats, quirks kept.
 *   Tokens (:729-1013).  A fixed prefix is one N_ALPHA.  Behind it: in a maximal stretch of letters and punctuation the
 *   bytes before the first letter are N_CHAR each and the rest is one token, N_CHAR if it is one byte, else N_ALPHA; a
 *   stretch of digits is cut into pieces of nine from its start, N_DIGITS0 if the piece starts with '0' or the earlier
 *   name has a N_DIGITS0 of the same width there (:916-919), else N_DIGITS; any other byte is a N_CHAR.  Against the
 *   earlier name's token at the same position: N_MATCH, N_DDELTA / N_DDELTA0 for a difference of 1..255 (N_DDELTA only
 *   while 5 + deltas so far > literals so far at that position, :934), else the literal.
 *   Columns (:342-500).  As encode_token_* writes them; N_DZLEN has no type byte.  A type column that is N_MATCH behind
 *   its first byte is dropped if its position has another column (:1406-1429).
 * Statuses, for input the reference cannot encode: nreads == 0: SIZE (create_context fails); a byte >= 0x80 inside a name:
 * UNSUPPORTED (the reference aborts); a name whose N_END would lie at position max_tokens or beyond: UNSUPPORTED (the
 * reference runs over its arrays at 128); more names than max_names, a name above max_name_len, a block above max_in_size
 * (not read), a block that ends beyond total_in_size, more columns than max_columns: UNSUPPORTED.  A block fails as a whole:
 * its status, size 0, no columns; d_last_start / d_nreads are what the framing found (0 for a block that was not read); its
 * neighbours are not affected.  Nothing outside the blocks' ranges is written.
 * The names, token records (20 bytes per byte of input) and tables wait in an arena of the context; a batch whose arena
 * does not fit half of max_workspace_mb is refused with -1: split it.  One wave tokenises one block.
 *
 * rans4x16_hip_tok3_encode_names_dev: encode_names as one call, names in and containers out - the tokeniser into a column
 * arena of the context (6 x total_in_size bytes; total_in_size 0: 6 x nblk x max_in_size), then the stages of
 * rans4x16_hip_tok3_pack_dev over its directory.  It takes the tokeniser's input and limits and the pack's k, methods
 * and dense output arena (d_out, out_capacity, d_out_off, d_out_size, d_status: as there, the sizing pass included).
 * The number of columns stays on the device: the pack's stages run over all nblk x max_columns entries of the directory,
 * those behind the last column as empty items, so max_columns should not be far above what the blocks have.
 *   d_chosen       [nblk x max_columns] or NULL: the method of column i of the dense directory
 *   d_blk_first    [nblk + 1] or NULL: receives the directory's block starts, which say whose column i is
 *   max_col_size   largest column (host), 0: 4 x max_in_size, which no column exceeds; it sizes the encoder's internal slots
 * A block the tokeniser refuses reports that status and size 0; every other block what rans4x16_hip_tok3_pack_dev
 * reports for its columns, byte for byte what encode_names returns for the block with the same method list.  A batch whose
 * arenas do not fit half of max_workspace_mb is refused with -1: split it.
 * Both calls only enqueue and read nothing back; -1 on bad arguments (a NULL context included). */
int rans4x16_hip_tok3_tokenise_dev(rans4x16_hip_ctx *ctx, int nblk,
                                   const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                   unsigned char *d_cols, uint64_t col_capacity, uint64_t *d_cols_off,
                                   uint32_t *d_cols_size, int32_t *d_status,
                                   uint32_t *d_blk_first, int32_t *d_col_id, uint64_t *d_col_off, uint32_t *d_col_size,
                                   uint32_t *d_last_start, uint32_t *d_nreads,
                                   uint32_t max_in_size, uint32_t max_names, uint32_t max_name_len,
                                   uint32_t max_tokens, uint32_t max_columns, uint64_t total_in_size,
                                   uint32_t search_slots, void *stream);
int rans4x16_hip_tok3_encode_names_dev(rans4x16_hip_ctx *ctx, int nblk,
                                       const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                       unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                       uint32_t *d_out_size, int32_t *d_status,
                                       int k, const int *methods, int32_t *d_chosen, uint32_t *d_blk_first,
                                       uint32_t max_in_size, uint32_t max_names, uint32_t max_name_len,
                                       uint32_t max_tokens, uint32_t max_columns, uint32_t max_col_size,
                                       uint64_t total_in_size, uint32_t search_slots, void *stream);

/* ---- 2f. tok3 names with host buffers -------------------------------------------------------------
 * encode_names / decode_names of htscodecs tokenise_name3.c (:1334-1531, :1546-1694) with HOST buffers in and out, rANS
 * flavour (use_arith = 0) unless rans4x16_hip_set_tok3_arith or the two _arith_ functions below: the boundary of parts 2c to 2e for a caller that holds a `char *blk` and knows none of their
 * limits.  include/tok3_names_hip.h gives the two functions their reference names.
 *
 * rans4x16_hip_tok3_level_methods: the row of tokenise_name3.c:1254-1260 that `level` selects ((level - 1) / 2, clamped to
 * 0..4), written to methods[0..k-1]; returns k (<= 9).  Pure host, usable without a GPU.
 *
 * rans4x16_hip_tok3_encode_names / rans4x16_hip_tok3_decode_names: the reference's two functions with the reference's
 * ownership - a malloc'ed result the caller free()s, NULL on failure.  They are the batch calls below with nblk = 1, on the
 * context the five rANS symbols of part 1 use for the calling thread.  encode: the method list is that of `level`;
 * use_arith != 0 returns NULL (the reason on stderr, once per process); last_start_p may be NULL; after success every byte
 * <= '\n' in front of last_start has been overwritten with NUL in the caller's buffer, as the reference does (:1374), and
 * the bytes from last_start on are left alone.  decode: *out_len = last_start bytes of NUL-separated names.
 * These two keep to the rANS flavour whatever mode a context has: decode_names returns NULL for use_arith != 0.
 *
 * rans4x16_hip_tok3_arith_encode_names(blk, len, level, out_len, last_start_p) / rans4x16_hip_tok3_arith_decode_names: the
 * same two functions for the arith flavour - the thread's context with rans4x16_hip_set_tok3_arith's mode set for the
 * call and put back; ownership and NUL-writing as above.  The container's byte 8 is 1; `level` is the reference's inner
 * level 1..9 (the reference's command line writes -17 for level 7 with use_arith = 1).  arith_decode_names takes the flavour
 * from the container and reads rANS ones too.  include/tok3_names_hip.h forwards encode_names(.., use_arith != 0, ..) and
 * decode_names of a container with byte 8 set to them.
 *
 * rans4x16_hip_thread_ctx: the context of the CALLING thread on which the single-block functions of this part and of parts
 * 2g and 2h run (made at first use, NULL without a usable GPU).  It is the library's: it ends with its thread and must
 * not be destroyed.  A caller may read its routes and its last error and set its options and setters; the four functions
 * above set the tok3 mode they need for their one call and leave rans4x16_hip_set_tok3_arith's value as the caller had it.
 *
 * rans4x16_hip_tok3_encode_names_batch / rans4x16_hip_tok3_decode_names_batch: nblk independent blocks in host memory.
 *   in[i], in_size[i]   block i: names (encode) / a container (decode); never written
 *   out[i], out_size[i] out[i] == NULL on entry: the library malloc()s exactly the result and the caller free()s it;
 *                       else out_size[i] is the capacity on entry.  out_size[i] is the size on return.  A result that does
 *                       not fit reports R4X16_E_CAPACITY and nothing is written; a failed block has out_size[i] = 0 and an
 *                       out[i] that was NULL stays NULL; its neighbours are not affected
 *   k, methods          encode: the method list of every column, as in rans4x16_hip_tok3_pack_dev
 *   last_start, nreads (encode), nnames (decode), status: [nblk] each, any of them may be NULL
 * Returns the number of failed blocks, -1 if the batch could not be run (no GPU, bad arguments, no memory for a single
 * block); nblk == 0 returns 0.
 * Block i's bytes and status are those of rans4x16_hip_tok3_encode_names_dev / rans4x16_hip_tok3_decode_names_dev with
 * the same method list and limits that admit the block: the library finds the limits itself.  Encode: a kernel measures
 * the names and the longest name of every block and the host reads the maxima back (max_tokens is 128, max_columns 2048);
 * what exceeds the device calls' hard limits (a block above 16,776,960 bytes - it is not uploaded -, a name above 16,384
 * bytes, 2^24 names or more) is clamped, so that the device refuses that block alone with R4X16_E_UNSUPPORTED.  Decode:
 * rans4x16_hip_tok3_scan gives each container's limits; one it refuses reports the scan's status and is not uploaded
 * (use_arith != 0 is R4X16_E_UNSUPPORTED there; under R4X16_TOK3_ARITH_DECODE rans4x16_hip_tok3_scan_any is the scan); X_STRIPE columns (levels 3 and up) are decoded as after
 * rans4x16_hip_set_dev_stripe_planes(ctx, 4, largest column), and the context's own setting is left as the caller had
 * it.  A container whose columns and histories alone do not fit half of what the context may take (a hostile size
 * field, as a rule) reports R4X16_E_UNSUPPORTED and is not uploaded.
 * The batch is walked in chunks of whole blocks whose arenas fit half of max_workspace_mb and of the free memory;
 * rans4x16_hip_set_names_chunk_blocks(ctx, n) bounds a chunk to n blocks (0, the default: by room alone) - a setter like
 * rans4x16_hip_set_dev_stripe_planes rather than a named option.  The calls synchronise. */
int rans4x16_hip_tok3_level_methods(int level, int *methods);
unsigned char *rans4x16_hip_tok3_encode_names(char *blk, int len, int level, int use_arith,
                                              int *out_len, int *last_start_p);
unsigned char *rans4x16_hip_tok3_decode_names(unsigned char *in, uint32_t sz, uint32_t *out_len);
unsigned char *rans4x16_hip_tok3_arith_encode_names(char *blk, int len, int level, int *out_len, int *last_start_p);
unsigned char *rans4x16_hip_tok3_arith_decode_names(unsigned char *in, uint32_t sz, uint32_t *out_len);
rans4x16_hip_ctx *rans4x16_hip_thread_ctx(void);
int rans4x16_hip_tok3_encode_names_batch(rans4x16_hip_ctx *ctx, int nblk,
                                         const unsigned char *const *in, const unsigned int *in_size,
                                         unsigned char **out, unsigned int *out_size,
                                         int k, const int *methods, unsigned int *last_start, unsigned int *nreads, int *status);
int rans4x16_hip_tok3_decode_names_batch(rans4x16_hip_ctx *ctx, int nblk,
                                         const unsigned char *const *in, const unsigned int *in_size,
                                         unsigned char **out, unsigned int *out_size, unsigned int *nnames, int *status);
int rans4x16_hip_set_names_chunk_blocks(rans4x16_hip_ctx *ctx, int blocks);

/* ---- 2g. arith_dynamic decoding (the CRAM 3.1 adaptive arithmetic coder) ---------------------------------------
 * htscodecs/arith_dynamic.c's decoder on the device: one carry-less range coder and adaptive models per stream (order 0,
 * order 1, with or without the coder's own run lengths), inside the containers of rANS 4x16 (X_PACK, X_CAT, X_NOSZ,
 * X_STRIPE).  The encoder is part 2h.  tok3 containers with use_arith = 1 are R4X16_E_UNSUPPORTED (parts 2c-2f) unless
 * rans4x16_hip_set_tok3_arith.
 * A stream is one serial chain of dependent steps: one wave decodes it, so a
 * batch wants many streams.
 *
 * rans4x16_hip_arith_uncompress_dev has the arguments and the contract of rans4x16_hip_uncompress_dev_sized: it only
 * enqueues on `stream`, reads nothing back, writes d_out_size / d_status per block and nothing outside a block's slot
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]).  d_out_cap[i] is the capacity the reference's arith_uncompress_to is
 * given (and the size of a bare X_NOSZ stream).  Statuses, as the reference returns NULL:
 *   R4X16_E_EMPTY        a zero-length block
 *   R4X16_E_TRUNCATED    the input ends inside the header, the X_PACK map or an X_CAT payload; stripe lengths beyond it
 *   R4X16_E_SIZE         a size of INT_MAX or more; a plane length of 0; a plane that gives another size than its share;
 *                        packed bytes that cannot fill the stored size
 *   R4X16_E_CAPACITY     the stored size is above the capacity; for an X_STRIPE block, not equal to it (as for rANS);
 *                        a packed size above the stored size
 *   R4X16_E_UNSUPPORTED  X_EXT (bzip2), as a reference built without libbz2; a block above max_in_size (not read) or a
 *                        size above max_out_size; in a batch that decodes to more than total_out_size (0: n x max_out_size)
 *                        the blocks that no longer fit - several, and not necessarily the last ones
 * Deviations from the reference, on malformed input only: a plane that is itself an X_STRIPE stream, and a stripe block
 * with more planes or a larger size than rans4x16_hip_set_dev_stripe_planes reserved (0 planes, the default: every
 * stripe block), report R4X16_E_UNSUPPORTED; N = 0 with a size above 0 reports R4X16_E_SIZE (the reference does not
 * return from it).  An accepted damaged stream decodes to the reference's bytes: the core decoders never refuse.
 * Returns 0 if enqueued, -1 on argument / allocation errors.
 *
 * rans4x16_hip_arith_peek_dev: flag byte and stored size per block; the two lie where rANS 4x16 has them, so this is
 * rans4x16_hip_peek_dev's reader with its statuses.
 *
 * rans4x16_hip_arith_uncompress_batch: host buffers - out_size[i] holds the capacity of out[i] on entry and the size on
 * return, status[i] the code.  One upload, the device call on the context's own stream, one download; it is not
 * pipelined, and it synchronises.  Stripe blocks are decoded whatever the context's stripe setting, which is put back.
 * Returns the number of blocks refused, -1 on errors.
 *
 * rans4x16_hip_arith_uncompress_to / rans4x16_hip_arith_uncompress: the arguments and the ownership of the reference's
 * arith_uncompress_to / arith_uncompress (out == NULL: a malloc'd buffer of the stream's stored size, the caller's to
 * free; NULL on failure), on the calling thread's context.  include/arith_dynamic_hip.h gives them the reference's names.
 *
 * Route read-out: R4X16_ROUTE_ARITH counts the entropy-coded streams (a stripe block's planes each) by where their models
 * live: R4X16_ARITH_O0, R4X16_ARITH_O1_LDS, R4X16_ARITH_O1_GLOBAL; those with run lengths count under R4X16_ARITH_RLE too.
 * A batch above the workspace ceiling (option max_workspace_mb) is walked in chunks, and every chunk counts one
 * R4X16_LAUNCH_IN_ORDER under R4X16_ROUTE_LAUNCH. */
int rans4x16_hip_arith_uncompress_dev(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                      unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                      uint32_t *d_out_size, int32_t *d_status,
                                      uint32_t max_in_size, uint32_t max_out_size, uint64_t total_out_size, void *stream);
int rans4x16_hip_arith_peek_dev(rans4x16_hip_ctx *ctx, int n,
                                const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status,
                                uint32_t max_in_size, void *stream);
int rans4x16_hip_arith_uncompress_batch(rans4x16_hip_ctx *ctx, int n,
                                        const unsigned char *const *in, const unsigned int *in_size,
                                        unsigned char *const *out, unsigned int *out_size, int *status);
unsigned char *rans4x16_hip_arith_uncompress_to(unsigned char *in, unsigned int in_size,
                                                unsigned char *out, unsigned int *out_size);
unsigned char *rans4x16_hip_arith_uncompress(unsigned char *in, unsigned int in_size, unsigned int *out_size);

/* ---- 2h. arith_dynamic encoding -------------------------------------------------------------------------------
 * htscodecs/arith_dynamic.c's arith_compress_to on the device: the bytes the reference writes, for every order word it
 * takes - order 0 / 1, X_RLE, X_PACK, X_CAT, X_NOSZ and X_STRIPE with its candidate methods per plane, the smallest
 * kept, the first smallest where several tie.  One wave encodes a stream, so a batch wants many.
 *
 * rans4x16_hip_arith_compress_bound: the reference's arith_compress_bound, host arithmetic.
 *
 * rans4x16_hip_arith_compress_dev has the arguments and the contract of rans4x16_hip_compress_dev_sized: it only enqueues
 * on `stream`, reads nothing back, writes d_out_size / d_status per block and nothing outside a block's slot
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]).  `order` applies to all blocks unless d_order is given; total_in_size 0
 * means n x max_in_size.  X_STRIPE blocks are encoded when one `order` serves all blocks; under d_order only after
 * rans4x16_hip_set_dev_stripe_encode(ctx, max_planes), which reserves max_planes x 3 items a block.  Statuses:
 *   R4X16_E_UNSUPPORTED  X_EXT (bzip2), as a reference built without libbz2; X_STRIPE with more than 255 planes (the
 *                        reference's NULL), with more planes than reserved, or under d_order without the setting; a block
 *                        above max_in_size (not read); in a batch larger than total_in_size the blocks that no longer fit
 *   R4X16_E_CAPACITY     d_out_cap[i] below rans4x16_hip_arith_compress_cap(size, order): nothing is written
 * Capacity.  The reference's behaviour with a buffer below arith_compress_bound is undefined (its core coders return NULL
 * unnoticed, and the fall-back compares against a size nobody wrote).  The result here is defined as what
 * arith_compress(in, size, &n, order) returns, and any capacity is accepted that holds the worst case of that result:
 * size + 28 for a plain block (flag 1, size 5, pack map 17, packed length 5); size + 7 + 6 x N for a stripe block of N
 * planes under an odd order (every plane has method 1 among its candidates: its length, a flag and at most its bytes),
 * size + 7 + 28 x N under an even one (a plane from the third on is tried with X_PACK alone and may carry the map and
 * the packed length besides).  rans4x16_hip_arith_compress_cap returns that value; it is never above the bound.  This
 * deviation is confined to buffers the reference would have mishandled.
 * Returns 0 if enqueued, -1 on argument / allocation errors.
 *
 * rans4x16_hip_arith_compress_batch: host buffers - out_size[i] holds the capacity of out[i] on entry and the size on
 * return, status[i] the code, order[i] the block's order word.  One upload, the device call on the context's own stream,
 * one download; it is not pipelined, and it synchronises.  Stripe blocks are encoded whatever the context's stripe
 * setting, which is put back.  Returns the number of blocks refused, -1 on errors.
 *
 * rans4x16_hip_arith_compress_to / rans4x16_hip_arith_compress: the arguments and the ownership of the reference's
 * arith_compress_to / arith_compress (out == NULL: a malloc'd buffer of the bound, the caller's to free; *out_size the
 * capacity on entry and the size on return; NULL on failure), on the calling thread's context.
 * include/arith_dynamic_hip.h gives them the reference's names.
 *
 * rans4x16_hip_arith_compress_best_packed_dev: rans4x16_hip_compress_best_packed_dev for this coder - its arguments, its
 * dense arena (offsets written by the call and summed before the capacity rule, d_out == NULL with out_capacity 0 as a
 * sizing pass, R4X16_E_CAPACITY and size 0 for a block that ends beyond out_capacity), and the rules of
 * rans4x16_hip_compress_best_dev: block i gets exactly the bytes of arith_compress_to(in, size, .., methods[j]) for the
 * smallest result, the earlier method on ties; d_chosen[i] (may be NULL) is that methods[j] as given, -1 if no candidate
 * succeeded; an X_STRIPE method is skipped when size % 4 != 0 (tokenise_name3.c:1270); a block whose every method was
 * skipped, or that lies above max_in_size, reports R4X16_E_UNSUPPORTED; more than 255 planes in a method make the call
 * return -1.  A batch that holds more than total_in_size announced runs out of room for some candidates: a block of which
 * any tried candidate found no room reports R4X16_E_UNSUPPORTED as a whole, whatever its other candidates gave - a
 * winner is always the smallest of ALL the methods that apply.  rans4x16_hip_arith_best_chunk_blocks(ctx, n, k, methods,
 * max_in_size, total_in_size) returns the blocks per chunk the call plans for these arguments under the context's
 * max_workspace_mb and the free memory of the moment (n where the batch is one chunk; -1 on bad arguments): host
 * arithmetic, nothing is enqueued.  The k candidates of a chunk of blocks go through the coder's kernels in one pass, as
 * k times as many items with per-item order words (no rans4x16_hip_set_dev_stripe_encode is needed, the context's setting
 * is left alone), into slots of rans4x16_hip_arith_compress_cap bytes each in an arena of the context; the batch is walked
 * in chunks under max_workspace_mb.  The call only enqueues, reads nothing back and writes nothing outside the blocks'
 * ranges.  R4X16_ROUTE_ARITH_ENC counts every candidate stream that was tried.
 *
 * Route read-out: R4X16_ROUTE_ARITH_ENC counts the candidate streams (a stripe block's planes under each method) that
 * reached the coder by the home of their models, those with run lengths under R4X16_ARITH_ENC_RLE too, and under
 * R4X16_ARITH_ENC_STORED every candidate that came out as X_CAT: an explicit X_CAT, and a coded one that ended no smaller
 * than its input (it is counted under its home as well).  Chunks count as in part 2g. */
unsigned int rans4x16_hip_arith_compress_bound(unsigned int size, int order);
unsigned int rans4x16_hip_arith_compress_cap(unsigned int size, int order);
int rans4x16_hip_arith_compress_dev(rans4x16_hip_ctx *ctx, int n,
                                    const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                    unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                    uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                    uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_arith_compress_best_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                                const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                                unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                                uint32_t *d_out_size, int32_t *d_status,
                                                int k, const int *methods, int32_t *d_chosen,
                                                uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_arith_best_chunk_blocks(rans4x16_hip_ctx *ctx, int n, int k, const int *methods,
                                         uint32_t max_in_size, uint64_t total_in_size);
int rans4x16_hip_arith_compress_batch(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *const *in, const unsigned int *in_size,
                                      unsigned char *const *out, unsigned int *out_size, const int *order, int *status);
unsigned char *rans4x16_hip_arith_compress_to(unsigned char *in, unsigned int in_size,
                                              unsigned char *out, unsigned int *out_size, int order);
unsigned char *rans4x16_hip_arith_compress(unsigned char *in, unsigned int in_size, unsigned int *out_size, int order);

/* ---- 2i. fqzcomp_qual decoding (the CRAM 3.1 quality codec) ------------------------------------------------------
 * htscodecs/fqzcomp_qual.c's decoder on the device: the range coder and the adaptive models of parts 2g and 2h, with a
 * 16-bit context - up to 65,536 models a stream, in a slot of the context's arena - and the per-record machinery
 * (selector, lengths, reverse flag, duplicates, parameter blocks and their tables).  The encoder is part 2j.
 * DESIGN.md 4.8.
 *
 * rans4x16_hip_fqz_scan: walks the header of one stream in HOST memory.  Pure host arithmetic, usable without a GPU.
 * Reports the stored size, the bytes in front of the range coder's input, gflags, nparam, max_sel and max_sym (the
 * largest of the parameter blocks'; any of the pointers may be NULL) and returns 0 or the R4X16_E_* status the device
 * gives the stream before it decodes a symbol:
 *   R4X16_E_EMPTY        a zero-length block
 *   R4X16_E_TRUNCATED    fewer than 10 bytes behind the size; a parameter block of fewer than 7 bytes; a qmap beyond the end
 *   R4X16_E_UNSUPPORTED  a version other than 5
 *   R4X16_E_SIZE         nparam = 0
 *   R4X16_E_TABLE        where the reference is undefined: a table whose run lengths do not fill it
 *                        (read_array returns -1, which the reference adds to its index unchecked - a table that starts
 *                        at the end of the stream is one such), and PFLAG_DO_SEL in a parameter block with max_sel = 0
 *
 * rans4x16_hip_fqz_uncompress_dev has the arguments and the contract of rans4x16_hip_arith_uncompress_dev: it only
 * enqueues on `stream`, reads no device list back, and writes nothing outside [d_out_off[i], d_out_off[i] + d_out_cap[i])
 * and the lengths slots below.  Block i decodes to exactly the bytes of fqz_decompress, d_out_size[i] its stored size.
 * Besides the scan's statuses, d_status[i] is
 *   R4X16_E_CAPACITY     d_out_cap[i] below the stored size: nothing is written
 *   R4X16_E_CONTEXT      a record's selector names a parameter block the stream does not have (the reference's NULL)
 *   R4X16_E_SIZE         a record longer than the bytes that remain, or of length 0; a duplicate longer than the bytes
 *                        decoded so far (the reference's NULL)
 *   R4X16_E_UNSUPPORTED  a block above max_in_size (not read), a stored size above max_out_size or of 2^31 or more, a
 *                        max_sym above rans4x16_hip_set_fqz_limits's, a block that finds total_out_size spent - the
 *                        blocks are taken in their order - or no room for its parameter blocks (the arena holds four a
 *                        block of the chunk and 256 at least: one stream always fits)
 * On a refused block the bytes inside its slot may be anything.  Everything else is the reference's, bug for bug: a
 * frequency above MAX_FREQ decodes symbol 0, a coder that runs dry goes on, a symbol beyond a stored qmap gives 255.
 * The four arguments in front of max_in_size may be NULL (d_len_off and d_len_cap must be given with d_len):
 *   d_len      record lengths: block i's record r at d_len[d_len_off[i] + r] for r < d_len_cap[i] - offsets and
 *              capacities count ENTRIES; the reference's `lengths[rec] = len` for rec < nlengths
 *   d_nrec     d_nrec[i] = the records of block i (0 for a refused one)
 *
 * rans4x16_hip_set_fqz_limits(ctx, max_slots, max_sym): max_slots caps the model slots - the streams decoded side by
 * side; the others wait for a slot - at 1..1024 (0: 1024, four a compute unit).  max_sym (1..255; 0: 255) is the
 * largest max_sym a slot holds: a slot is 65,536 x (4 x (max_sym + 1 rounded up to 4) + 4) bytes, 12.8 MB for the 45
 * symbols of q40 data against 67.4 MB for 256, and the slots of a chunk count against max_workspace_mb.  Not named
 * options: like rans4x16_hip_set_dev_stripe_planes they describe the batches to come, not the library.
 *
 * rans4x16_hip_fqz_peek_dev: the stored size per block - the varint at byte 0; this format has no flag byte.
 * d_status[i]: R4X16_E_EMPTY, R4X16_E_UNSUPPORTED above max_in_size, R4X16_E_TRUNCATED where the varint runs past the block.
 *
 * rans4x16_hip_fqz_uncompress_batch: host buffers - out_size[i] holds the capacity of out[i] on entry and the size on
 * return; lengths (NULL, or per block NULL or an array of nlengths[i] entries) and nrec (NULL or [n]) as above.  One
 * upload, the device call with the slots sized for the batch's largest max_sym, one download.  Returns the number of
 * failed blocks, -1 on a call error.
 *
 * rans4x16_hip_fqz_decompress: the arguments and the ownership of the reference's fqz_decompress (a malloc'd buffer of
 * the stored size, the caller's to free; *uncomp_size is the stored size even on failure; NULL on failure), on the
 * calling thread's context.  include/fqzcomp_qual_hip.h gives it the reference's name.
 *
 * Route read-out: R4X16_ROUTE_FQZ counts the streams that were decoded (R4X16_FQZ_*); each chunk of a call counts once
 * as R4X16_LAUNCH_IN_ORDER under R4X16_ROUTE_LAUNCH. */
int rans4x16_hip_fqz_scan(const unsigned char *in, unsigned int in_size, uint32_t *stored_size, uint32_t *header_bytes,
                          uint32_t *gflags, uint32_t *nparam, uint32_t *max_sel, uint32_t *max_sym);
int rans4x16_hip_set_fqz_limits(rans4x16_hip_ctx *ctx, int max_slots, int max_sym);
int rans4x16_hip_fqz_uncompress_dev(rans4x16_hip_ctx *ctx, int n,
                                    const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                    unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                    uint32_t *d_out_size, int32_t *d_status,
                                    uint32_t *d_len, const uint64_t *d_len_off, const uint32_t *d_len_cap, uint32_t *d_nrec,
                                    uint32_t max_in_size, uint32_t max_out_size, uint64_t total_out_size, void *stream);
int rans4x16_hip_fqz_peek_dev(rans4x16_hip_ctx *ctx, int n,
                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                              uint32_t *d_raw_size, int32_t *d_status, uint32_t max_in_size, void *stream);
int rans4x16_hip_fqz_uncompress_batch(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *const *in, const unsigned int *in_size,
                                      unsigned char *const *out, unsigned int *out_size, int *status,
                                      int *const *lengths, const int *nlengths, unsigned int *nrec);
char *rans4x16_hip_fqz_decompress(char *in, size_t comp_size, size_t *uncomp_size, int *lengths, int nlengths);

/* ---- 2j. fqzcomp_qual encoding (fqz_compress) ---------------------------------------------------------------------
 * htscodecs/fqzcomp_qual.c's encoder: the parameter choice on the host (on the device: part 2k), the encode loop on the
 * device.  DESIGN.md 4.9.
 *
 * PARAMETER BYTES are the parameter format of every call here: what fqz_store_parameters writes and a stream holds
 * between its size varint and the range coder's bytes - the version byte (5), gflags, [nparam], [max_sel, the selector
 * table], the parameter blocks.  They go into the stream verbatim, and the device reads them with the header walk of
 * part 2i: parameter bytes it would refuse in a stream it refuses here, with the scan's statuses.
 *
 * rans4x16_hip_fqz_pick_parameters: fqz_pick_parameters and fqz_qual_stats(.., one_param = -1) in HOST memory.  Pure host
 * arithmetic, usable without a GPU.  vers 3 sets GFLAG_DO_REV; strat 0..3 are the reference's strategies, 4 and above its
 * all-zero row.  flags[rec] holds FQZ_FREVERSE (16), FQZ_FREAD2 (128) and, from bit 16 up, a selector of the caller's.
 * On success (0) `params` holds *params_size parameter bytes, len[] is as the reference's fix-ups leave it (a list that
 * overruns in_size is cut, the last record takes what is left over) and flags[rec] >> 16 holds the selector the
 * statistics chose (the average-quality split, the READ1/READ2 split): the slice the encode calls take.
 * R4X16_E_CAPACITY: params_cap is too small (or params NULL); *params_size is the size needed, len and flags are
 * unchanged.  R4X16_E_UNSUPPORTED: a negative strat or nrec, a missing array, 2^31 bytes or more.  With nrec = 0 the
 * reference reads len[0]; here that length counts as 0.
 *
 * rans4x16_hip_fqz_compress_dev has the contract of rans4x16_hip_arith_compress_dev: it only enqueues on `stream`, reads
 * nothing back and writes nothing outside [d_out_off[i], d_out_off[i] + d_out_cap[i]).  Per block: the qualities
 * (d_in, d_in_off, d_in_size), the parameter bytes (d_params, d_par_off, d_par_size), the records - d_nrec[i] lengths
 * and flags as 32-bit entries from d_len[d_rec_off[i]] and d_flags[d_rec_off[i]] (the offset counts ENTRIES), flags
 * with bit 4 = reversed and bits 16 and up = selector, the slice as the pick leaves it - and the slot.  Block i comes
 * out as compress_block_fqz2f writes it under those parameters: varint(size), the parameter bytes, the coder's bytes.
 * The caller's input is never modified.  d_status[i], besides the scan's statuses for the parameter bytes:
 *   R4X16_E_CAPACITY     the stream is longer than d_out_cap[i]: nothing is written.  A slot of any size is accepted;
 *                        one of rans4x16_hip_fqz_compress_cap(size, nrec, params_size) bytes never overflows
 *   R4X16_E_SIZE         record lengths that do not sum to the size, a record of 0 bytes, no record for a block that
 *                        has bytes (a block of size 0 reads no record)
 *   R4X16_E_CONTEXT      where the reference is undefined: a selector above max_sel where selectors are
 *                        coded, or one whose parameter block the bytes do not have; a quality that a stored qmap does
 *                        not list, or - without a stored qmap - above max_sym
 *   R4X16_E_TABLE        also: several parameter blocks with max_sel = 0 (no selector model to code with)
 *   R4X16_E_TRUNCATED / R4X16_E_UNSUPPORTED  also: parameter bytes that end before / go on behind the walk's end
 *   R4X16_E_UNSUPPORTED  a block above max_in_size, max_params_size or max_records, or of 2^31 bytes or more (not read),
 *                        a max_sym above rans4x16_hip_set_fqz_limits's, no room for its parameter blocks (the arena holds
 *                        four a block of the chunk and 256 at least)
 * The model slots and rans4x16_hip_set_fqz_limits are part 2i's.
 *
 * rans4x16_hip_fqz_compress_batch: host buffers.  nrec[i], len[i], flags[i] describe block i's records; params may be
 * NULL, and a block with params[i] == NULL is picked on the host with (vers, strat) - its len[i] and flags[i] change as
 * the pick changes them.  out_size[i] holds the capacity of out[i] on entry and the size on return.  One upload, the
 * device call with the slots sized for the batch's largest max_sym, one download.  On return flags[i][rec] &= 0xffff,
 * as the reference leaves them.  Returns the number of failed blocks, -1 on a call error.
 *
 * rans4x16_hip_fqz_compress: the arguments and the ownership of the reference's fqz_compress (a malloc'd buffer, the
 * caller's to free; NULL on failure; s->len and s->flags as the reference leaves them; `in` unchanged), on the calling
 * thread's context.  gp != NULL returns NULL: the parameter struct is not taken - a caller with parameters of its own
 * uses the batch call with parameter bytes.  include/fqzcomp_qual_enc_hip.h gives it the reference's name.
 *
 * Route read-out: R4X16_ROUTE_FQZ_ENC counts the streams that were encoded (R4X16_FQZ_ENC_*); each chunk of a call counts
 * once as R4X16_LAUNCH_IN_ORDER under R4X16_ROUTE_LAUNCH. */
typedef struct rans4x16_hip_fqz_slice { int num_records; uint32_t *len; uint32_t *flags; } rans4x16_hip_fqz_slice;
struct rans4x16_hip_fqz_gparams;   /* opaque: never looked into */
int rans4x16_hip_fqz_pick_parameters(int vers, int strat, int nrec, uint32_t *len, uint32_t *flags,
                                     const unsigned char *in, size_t in_size,
                                     unsigned char *params, unsigned int params_cap, unsigned int *params_size);
unsigned int rans4x16_hip_fqz_compress_cap(unsigned int size, unsigned int nrec, unsigned int params_size);
int rans4x16_hip_fqz_compress_dev(rans4x16_hip_ctx *ctx, int n,
                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                  const unsigned char *d_params, const uint64_t *d_par_off, const uint32_t *d_par_size,
                                  const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                  unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                  uint32_t *d_out_size, int32_t *d_status,
                                  uint32_t max_in_size, uint32_t max_params_size, uint32_t max_records, void *stream);
int rans4x16_hip_fqz_compress_batch(rans4x16_hip_ctx *ctx, int n,
                                    const unsigned char *const *in, const unsigned int *in_size,
                                    const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags,
                                    int vers, int strat,
                                    const unsigned char *const *params, const unsigned int *params_size,
                                    unsigned char *const *out, unsigned int *out_size, int *status);
char *rans4x16_hip_fqz_compress(int vers, rans4x16_hip_fqz_slice *s, char *in, size_t in_size, size_t *out_size, int strat,
                                struct rans4x16_hip_fqz_gparams *gp);

/* ---- 2k. fqzcomp_qual encoding: the parameter choice on the device ---------------------------------------------------
 * fqz_qual_stats(.., one_param = -1), fqz_pick_parameters and fqz_store_parameters over slices in DEVICE memory: what
 * rans4x16_hip_fqz_pick_parameters computes, byte for byte - the parameter bytes, the lengths after the fix-ups, the
 * selector in flags[rec] >> 16 - or no answer at all.  DESIGN.md 4.9 and 5.
 *
 * The choice compares sums of v * log(v / c) in doubles.  The device's log and its order of summation are not the
 * host's, so the device takes a comparison only where its two sides differ by more than a guard that bounds both
 * errors (2^-20 of the sum of the terms' magnitudes; a comparison of exact zeros is exact), and `pshift` of strategy 0
 * only for a first record below 2^22 bytes.  Otherwise the block's status is R4X16_E_UNDECIDED, nothing is written for
 * it, and the caller picks that block with rans4x16_hip_fqz_pick_parameters.
 *
 * rans4x16_hip_fqz_pick_dev only enqueues on `stream` and reads nothing back.  Inputs and records as in
 * rans4x16_hip_fqz_compress_dev, flags as the caller has them (a selector of the caller's from bit 16 up is kept and
 * OR-ed onto, as the reference does).  vers, strat as in rans4x16_hip_fqz_pick_parameters; d_strat (may be NULL) gives
 * block i the strategy d_strat[i] - one call can hold the same slice under several.  Block i gets its parameter bytes in
 * [d_par_off[i], + d_par_cap[i]) of d_params and their size in d_par_size[i], and its slice as the pick leaves it in
 * d_len_out / d_flags_out at the entries d_rec_off[i] .. + d_nrec[i].  d_len_out / d_flags_out may be the very pointers
 * d_len / d_flags; they may not overlap the inputs otherwise.  d_status[i]:
 *   R4X16_E_CAPACITY     d_par_cap[i] is too small: d_par_size[i] is the size needed, nothing else is written.
 *                        rans4x16_hip_fqz_pick_cap() bytes always do
 *   R4X16_E_UNSUPPORTED  a block above max_in_size or max_records, of 2^31 bytes or more, a negative strategy (not read)
 *   R4X16_E_UNDECIDED    see above
 * On any status but 0 the block's d_len_out / d_flags_out entries and its parameter slot are untouched, and
 * d_par_size[i] is 0 (the size needed under R4X16_E_CAPACITY).
 *
 * rans4x16_hip_fqz_compress_pick_dev: the pick and rans4x16_hip_fqz_compress_dev in one enqueue-only call.  The picked
 * parameter bytes, lengths and flags stay in the context's arena; the caller's input and records are never written.
 * d_out, d_out_off, d_out_cap, d_out_size, d_status as in rans4x16_hip_fqz_compress_dev; a block the pick refuses keeps
 * the pick's status (R4X16_E_UNSUPPORTED, R4X16_E_UNDECIDED) and codes nothing.  The encoder gets the records the
 * reference's encode loop reaches: those that the fix-ups leave behind the last byte (a list that over-runs) are never
 * coded, and the stream is the reference's.  A record of 0 bytes in front of the last byte, and bytes without a record,
 * are R4X16_E_SIZE as in part 2j.  The model slots are sized by rans4x16_hip_set_fqz_limits.
 *
 * rans4x16_hip_set_fqz_pick(ctx, mode, guard_bits): mode 0 (the default) changes nothing anywhere.  mode 1 makes
 * rans4x16_hip_fqz_compress_batch pick and code the blocks that come without parameter bytes in one round trip on the
 * device (the blocks that come with parameter bytes take the trip of mode 0 behind it); blocks the device leaves
 * R4X16_E_UNDECIDED are then picked on the host and coded in a second trip of those blocks alone.  The results are those
 * of mode 0: the streams, len[i] as the fix-ups leave them, flags[i][rec] &= 0xffff (an over-running list apart: mode 0
 * refuses its records of 0 bytes with R4X16_E_SIZE, the device trip codes it as the reference does).  The device trip's model slots are
 * as rans4x16_hip_set_fqz_limits sized them (mode 0 sizes them for the batch's largest max_sym, which the host pick
 * knows).  guard_bits (0 .. 64, default 0)
 * multiplies the guard by 2^guard_bits in every call of part 2k on this context: a test reaches the undecided path with
 * it.  Returns 0, -1 out of range.
 *
 * Route read-out: R4X16_ROUTE_FQZ_PICK (R4X16_FQZ_PICK_*); each chunk of a call counts once as R4X16_LAUNCH_IN_ORDER
 * under R4X16_ROUTE_LAUNCH (the one-call form: once for its pick, once for its encoder). */
unsigned int rans4x16_hip_fqz_pick_cap(void);
int rans4x16_hip_set_fqz_pick(rans4x16_hip_ctx *ctx, int mode, int guard_bits);
int rans4x16_hip_fqz_pick_dev(rans4x16_hip_ctx *ctx, int n,
                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                              const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                              int vers, int strat, const int32_t *d_strat,
                              unsigned char *d_params, const uint64_t *d_par_off, const uint32_t *d_par_cap, uint32_t *d_par_size,
                              uint32_t *d_len_out, uint32_t *d_flags_out, int32_t *d_status,
                              uint32_t max_in_size, uint32_t max_records, void *stream);
int rans4x16_hip_fqz_compress_pick_dev(rans4x16_hip_ctx *ctx, int n,
                                       const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                       const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                       int vers, int strat, const int32_t *d_strat,
                                       unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                       uint32_t *d_out_size, int32_t *d_status,
                                       uint32_t max_in_size, uint32_t max_records, void *stream);

/* ---- 2l. fqzcomp_qual encoding: best of several strategies ---------------------------------------------------------
 * The rows of strat_opts are alternatives for different instruments, and a CRAM writer offers them as so many methods and
 * keeps the smallest block.  These calls are that loop in one enqueue: block i is coded under each of the k strategies
 * strats[0 .. k) (a HOST array; 1 <= k <= 16, an entry >= 0, entries of 4 and above the all-zero row, entries may repeat;
 * anything else returns -1) and comes out as rans4x16_hip_fqz_compress_pick_dev(.., vers, strats[j], ..) writes it for the
 * j whose stream is smallest, the earlier j on a tie - the bytes and d_out_size[i] are that call's.  The statistics of part
 * 2k are counted once per slice, whatever k is; only the decisions and the store run per candidate.  DESIGN.md 4.9.
 *
 * Inputs and records as in rans4x16_hip_fqz_compress_pick_dev; the caller's input, lengths and flags are never written.
 * d_chosen (may be NULL): d_chosen[i] = the winner's index j into strats, -1 where the block has no winner (a winner that
 * the capacity refuses keeps its index).  d_len_out (may be NULL): for a block with a winner the entries d_rec_off[i] ..
 * + d_nrec[i] get the lengths as the fix-ups leave them.  d_status[i]:
 *   R4X16_E_UNDECIDED    the device pick cannot decide one of the candidates (part 2k): nothing is written for the block -
 *                        the smallest of the others would not be the smallest of the list
 *   R4X16_E_UNSUPPORTED  a block above max_in_size or max_records, of 2^31 bytes or more, a max_sym above
 *                        rans4x16_hip_set_fqz_limits's, or a candidate that found no room in the arena
 *   R4X16_E_CAPACITY     the WINNER is longer than d_out_cap[i] (it is tested alone: a loser that would fit is not taken),
 *                        or ends beyond the packed arena: nothing is written
 *   a candidate whose parameter bytes the encoder's front end refuses (R4X16_E_TABLE for a pshift the header walk cannot
 *   read back, ..) is out of the running; where no candidate is left - the records' own refusals, R4X16_E_SIZE and
 *   R4X16_E_CONTEXT, are every candidate's - the block has the status of the first candidate in list order.
 *
 * rans4x16_hip_fqz_compress_best_dev writes the winner into the caller's slot [d_out_off[i], + d_out_cap[i]).
 * rans4x16_hip_fqz_compress_best_packed_dev has the contract of rans4x16_hip_arith_compress_best_packed_dev: the winners lie
 * back to back in d_out, d_out_off ([n + 1]) is written on the device, a block that would end beyond out_capacity is
 * R4X16_E_CAPACITY with size 0 (its offsets stand), and nothing is written at or beyond d_out_off[n].  Both only enqueue on
 * `stream`, read nothing back and write nothing outside the results' ranges.  No candidate stream is copied twice and no
 * loser is copied at all: the winner is assembled at its final place from the encoder's stage.
 *
 * rans4x16_hip_fqz_best_chunk_blocks: the blocks per chunk these calls plan for n blocks under k strategies (n: one
 * chunk) - the pick's layout, the candidates' hand-over and the encoder's layout for k items a block fit
 * max_workspace_mb together.  Host arithmetic; -1 on bad arguments.
 *
 * rans4x16_hip_fqz_compress_best_batch: host buffers, as rans4x16_hip_fqz_compress_batch without parameter bytes: one
 * upload, the device call, one download of the winners.  chosen (may be NULL) as d_chosen.  len[i] comes back as the fix-ups
 * leave it (status 0) and flags[i][rec] &= 0xffff.  A block the device leaves R4X16_E_UNDECIDED has all its k candidates
 * picked on the host (rans4x16_hip_fqz_pick_parameters) and is coded in a second trip of those blocks alone, counted
 * under R4X16_FQZ_PICK_HOST.  Returns the number of failed blocks, -1 on a call error.
 *
 * Route read-out: R4X16_ROUTE_FQZ_BEST (R4X16_FQZ_BEST_*); R4X16_ROUTE_FQZ_PICK and R4X16_ROUTE_FQZ_ENC count what they
 * count, per candidate. */
int rans4x16_hip_fqz_compress_best_dev(rans4x16_hip_ctx *ctx, int n,
                                       const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                       const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                       int vers, int k, const int *strats,
                                       unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                       uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                       uint32_t max_in_size, uint32_t max_records, void *stream);
int rans4x16_hip_fqz_compress_best_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                              const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                              int vers, int k, const int *strats,
                                              unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                              uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                              uint32_t max_in_size, uint32_t max_records, void *stream);
int rans4x16_hip_fqz_best_chunk_blocks(rans4x16_hip_ctx *ctx, int n, int k, uint32_t max_in_size, uint32_t max_records);
int rans4x16_hip_fqz_compress_best_batch(rans4x16_hip_ctx *ctx, int n,
                                         const unsigned char *const *in, const unsigned int *in_size,
                                         const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags,
                                         int vers, int k, const int *strats,
                                         unsigned char *const *out, unsigned int *out_size, int *chosen, int *status);

/* ---- 2m. best of several methods ACROSS codecs: rANS 4x16 against arith_dynamic ------------------------------------
 * A CRAM 3.1 writer at its `small` and `archive` settings tries rANS 4x16 order words and arith_dynamic order words side
 * by side for an ordinary block, keeps the smallest stream and records the codec that won.  These calls are that loop
 * for blocks in device memory: one enqueue, one dense arena, no read-back; and the reader's one decode call for such a
 * mixed arena.
 *
 * A method is an int: a codec tag in bits 24..27 OR-ed with that codec's order word in bits 0..15.  An untagged word is a
 * rANS 4x16 method, as in every list of parts 2 and 2a.  Any other tag value makes a call return -1 (the tag space is
 * reserved for rANS 4x8 and fqzcomp_qual, which are no candidates here), and so does a word with a bit set in 16..23 or
 * above the tag: nothing but the tag and the order word is carried.
 *
 * rans4x16_hip_compress_best_any_packed_dev takes the arguments of rans4x16_hip_compress_best_packed_dev; `methods` is a
 * HOST array of 1..32 tagged words.  The list is split into its rANS sub-list and its arith sub-list, each in list order.
 * For each sub-list block i has the result that codec's own best-packed call gives under it
 * (rans4x16_hip_compress_best_packed_dev, rans4x16_hip_arith_compress_best_packed_dev: the X_STRIPE skip for sizes that
 * are no multiple of 4, the at-most-20-bytes rule, max_in_size, more than 255 planes returning -1, X_EXT refused by
 * arith).  Of the sub-lists whose result is status 0 block i gets the smaller stream; on equal sizes the one whose
 * winning method stands EARLIER in `methods` (the reference loop's tie rule, tokenise_name3.c:1281-1284, over the whole
 * list).  The bytes written are exactly that codec's stream.  A list of one codec gives byte for byte what that codec's
 * call gives.
 *   d_chosen[i] (may be NULL)  the winning methods[j] as given, tag included; -1 if no candidate succeeded: the block then
 *                              has size 0 and the status of the sub-list whose first method stands first in the list.
 *                              (An arith sub-list one of whose candidates found no room is R4X16_E_UNSUPPORTED as a
 *                              whole, as in part 2h; the rANS sub-list's result, if it has one, still stands.)
 *   output                     one dense arena with the rules of part 2a: d_out_off has n + 1 entries written by the call,
 *                              the sums are taken before the capacity rule, a block that ends beyond out_capacity is
 *                              R4X16_E_CAPACITY with size 0, d_out == NULL with out_capacity 0 is a sizing pass, and
 *                              nothing is written outside the blocks' ranges.
 * The call only enqueues on `stream`, reads nothing back and does not synchronise.  Per chunk of blocks both codecs'
 * candidates are encoded into internal slots by the kernels of parts 2 and 2h and reduced to a winner a codec by their own
 * pick kernels; one pick kernel compares the two winners (size, list position, status), the scan of part 2a runs over the
 * winners' sizes and one gather copies each winner from whichever arena holds it to its final place: a result byte is
 * copied once, a loser never leaves its slot.  The chunks are planned so that both codecs' slots and workspaces together
 * stay under max_workspace_mb and three quarters of the free device memory.
 *
 * rans4x16_hip_best_any_chunk_blocks: the blocks per chunk the call plans for these arguments.  Host arithmetic, nothing
 * is enqueued; -1 on bad arguments.
 *
 * rans4x16_hip_uncompress_any_packed_dev takes the arguments of rans4x16_hip_uncompress_packed_dev and d_method, a DEVICE
 * int32 array of which only `& R4X16_CODEC_MASK` is looked at: the encoder's d_chosen can be passed as it is.  A negative
 * entry is a block that was never written: it takes 0 bytes and reports R4X16_E_EMPTY.  An entry with any other tag than
 * the two above is R4X16_E_UNSUPPORTED with 0 bytes.  Every other block claims the size its stream stores (both codecs
 * keep it in the same place), or d_nosz_size[i] for an X_NOSZ stream (R4X16_E_SIZE where d_nosz_size is NULL); a claim
 * above max_out_size is refused (R4X16_E_UNSUPPORTED), d_out_off is the exclusive scan of the claims, a block that ends
 * beyond out_capacity is R4X16_E_CAPACITY with size 0, and nothing is written outside the ranges.  Then the two slot
 * decoders (rans4x16_hip_uncompress_dev_sized, rans4x16_hip_arith_uncompress_dev) run over the same entries, each seeing
 * length 0 for the other codec's blocks and reporting into arrays of its own.  X_STRIPE blocks of either codec decode
 * after rans4x16_hip_set_dev_stripe_planes.
 *
 * rans4x16_hip_compress_best_any_batch / rans4x16_hip_uncompress_any_batch: host buffers, through the staging arena of
 * the other host-buffer calls, in chunks of blocks.  Compress: out[i] == NULL - the library allocates exactly the result
 * (malloc; the caller frees); otherwise out_size[i] is the capacity on entry and a result that does not fit is
 * R4X16_E_CAPACITY for that block alone.  chosen (may be NULL) as d_chosen.  Uncompress: as rans4x16_hip_uncompress_batch
 * - out_size[i] is the capacity on entry (also what an X_NOSZ stream decodes to), method[i] as d_method; every block has a
 * buffer of its own and fails alone: a stream that stores more than out_size[i] is R4X16_E_CAPACITY and takes nothing from
 * its neighbours.  Both return the number of failed blocks, -1 on a call error; where the compress call returns -1 it has
 * freed every buffer it allocated and set those out[i] back to NULL (their out_size[i] to 0): nothing is left to free.
 *
 * Route read-out: R4X16_ROUTE_BEST_ANY (R4X16_BEST_ANY_*); the encode routes and R4X16_ROUTE_ARITH_ENC count their own
 * candidate streams as before. */
#define R4X16_CODEC_RANS4X16 0
#define R4X16_CODEC_ARITH    (1 << 24)
#define R4X16_CODEC_MASK     0x0F000000
int rans4x16_hip_compress_best_any_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                              const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                              unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                              uint32_t *d_out_size, int32_t *d_status,
                                              int k, const int *methods, int32_t *d_chosen,
                                              uint32_t max_in_size, uint64_t total_in_size, void *stream);
int rans4x16_hip_best_any_chunk_blocks(rans4x16_hip_ctx *ctx, int n, int k, const int *methods, uint32_t max_in_size,
                                       uint64_t total_in_size);
int rans4x16_hip_uncompress_any_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                           const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                           const int32_t *d_method,
                                           unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                           uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                           uint32_t max_in_size, uint32_t max_out_size, void *stream);
int rans4x16_hip_compress_best_any_batch(rans4x16_hip_ctx *ctx, int n,
                                         const unsigned char *const *in, const unsigned int *in_size,
                                         unsigned char **out, unsigned int *out_size,
                                         int k, const int *methods, int *chosen, int *status);
int rans4x16_hip_uncompress_any_batch(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *const *in, const unsigned int *in_size, const int *method,
                                      unsigned char *const *out, unsigned int *out_size, int *status);

/* ---- 2n. quality blocks: best of several methods across rANS 4x16, arith_dynamic and fqzcomp_qual -------------------
 * For a slice's quality series a CRAM 3.1 writer at `small` / `archive` tries rANS 4x16 order words, arith_dynamic order
 * words AND the fqzcomp_qual strategies, keeps the smallest stream and records the codec.  These calls are that loop for
 * slices in device memory, and the reader's one decode call for the arena it leaves.  Part 2m's calls keep their contract:
 * they still refuse the tag below.
 *
 * A method is a tagged int as in part 2m, with one tag more: R4X16_CODEC_FQZ | strat is a fqzcomp_qual strategy under part
 * 2l's rule for strat (>= 0; 4 and above the all-zero row).  `methods` is a HOST array of 1..32 words, at most 16 of them
 * with the FQZ tag.  Any other tag, a bit in 16..23 or above the tag, or a sub-list its own call refuses outright (more
 * than 255 stripe planes) makes a call return -1 before it touches the device.
 *
 * rans4x16_hip_compress_best_qual_packed_dev takes the arguments of rans4x16_hip_fqz_compress_best_packed_dev with
 * `k, methods` in place of `k, strats`, and total_in_size as in part 2m.  The list is split into its three sub-lists, each
 * in list order; for each, block i has exactly what that codec's own best-packed call gives under it
 * (rans4x16_hip_compress_best_packed_dev, rans4x16_hip_arith_compress_best_packed_dev,
 * rans4x16_hip_fqz_compress_best_packed_dev: their skips, limits and statuses).  Of the sub-lists whose result is status 0
 * the block gets the smaller stream, on equal sizes the one whose winning method stands EARLIER in `methods`; the bytes are
 * that codec's stream, unchanged.  A list of one codec gives byte for byte what that codec's call gives; a list without an
 * FQZ entry gives what part 2m's call gives and does not look at the record arrays (they may be NULL).
 *   R4X16_E_UNDECIDED   the fqzcomp sub-list cannot decide the block (part 2l): the whole block is undecided - size 0,
 *                       d_chosen -1, nothing written; the smallest of the others need not be the smallest of the list
 *   any other failure of the fqzcomp sub-list (the records' R4X16_E_SIZE / R4X16_E_CONTEXT, R4X16_E_UNSUPPORTED,
 *   R4X16_E_TABLE) takes only that codec out of the running, as a writer goes on when fqz_compress returns NULL.  With no
 *   sub-list left the block has size 0, d_chosen -1 and the status of the sub-list whose first method stands first.
 *   d_chosen[i] (may be NULL)  the winning methods[j] as given, tag included
 *   d_len_out (may be NULL)    written only for the blocks the fqzcomp sub-list won: the lengths as its fix-ups leave them
 *   output                     one dense arena with the rules of part 2a (sums before the capacity rule, R4X16_E_CAPACITY
 *                              with size 0 beyond out_capacity, d_out == NULL: a sizing pass)
 * The caller's input, lengths and flags are never written.  The call only enqueues on `stream`, reads nothing back and
 * writes nothing outside the winners' ranges.  Per chunk the rANS and arith candidates are encoded and reduced as in part
 * 2m; the fqzcomp candidates run part 2l's stages until the winner's size is known; one pick kernel compares up to three
 * winners (size, list position, status); after the scan one gather copies the rANS and arith winners, and part 2l's back
 * pass assembles, from the encoder's stage, the streams of the blocks fqzcomp won overall: a result byte moves once, a
 * loser never leaves its slot, and a fqzcomp stream that lost is never assembled.  DESIGN.md 4.10.
 *
 * rans4x16_hip_best_qual_chunk_blocks: the blocks per chunk the call plans - the largest for which the rANS slots and
 * workspace, the arith slots and inner arena and the fqzcomp pick layout, hand-over and encoder layout (model slots:
 * rans4x16_hip_set_fqz_limits) stay under max_workspace_mb and three quarters of the free memory.  Host arithmetic; -1 on
 * bad arguments.
 *
 * rans4x16_hip_uncompress_qual_packed_dev takes the arguments of rans4x16_hip_uncompress_any_packed_dev and the four
 * length arguments of rans4x16_hip_fqz_uncompress_dev (all may be NULL).  d_method[i] & R4X16_CODEC_MASK selects the
 * decoder; a negative entry is R4X16_E_EMPTY with 0 bytes, an unknown tag R4X16_E_UNSUPPORTED.  An FQZ block claims the
 * varint at byte 0 (rans4x16_hip_fqz_peek_dev), the others claim as in part 2m; scan, capacity rule and confinement are
 * part 2m's.  The three slot decoders run over the same entries, each seeing length 0 for the other codecs' blocks.
 * d_nrec[i] and the lengths are written for FQZ blocks; d_nrec[i] is 0 for every other.
 *
 * rans4x16_hip_compress_best_qual_batch / rans4x16_hip_uncompress_qual_batch: host buffers, through the staging arena of
 * the other host-buffer calls, in chunks of blocks, with the ownership rules of part 2m's batch calls (out[i] == NULL: the
 * library allocates exactly the result; where the compress call returns -1 it has freed what it allocated).  nrec, len,
 * flags as in rans4x16_hip_fqz_compress_best_batch (not looked at by a list without an FQZ entry: they may be NULL).  A
 * block the device leaves R4X16_E_UNDECIDED goes into a second trip of those blocks alone, counted under
 * R4X16_FQZ_PICK_HOST: its fqzcomp candidates are picked on the host (rans4x16_hip_fqz_pick_parameters) and coded under
 * their parameter bytes (rans4x16_hip_fqz_compress_batch, which runs rans4x16_hip_fqz_compress_dev), its rANS and arith
 * methods run through part 2m's batch call, and the host compares the results by the same rule.  len[i] comes back as the
 * fix-ups leave it and flags[i][rec] &= 0xffff where fqzcomp won; otherwise both are untouched.  Uncompress: method[i] as
 * d_method, out_size[i] the capacity on entry; lengths / nlengths / nrec as in rans4x16_hip_fqz_uncompress_batch, written
 * for the FQZ blocks (nrec[i] = 0 for every other); the model slots are sized for the largest max_sym of the FQZ streams.
 * Both return the number of failed blocks, -1 on a call error.
 *
 * Route read-out: R4X16_ROUTE_BEST_QUAL (R4X16_BEST_QUAL_*); the per-codec routes count their own candidates as before. */
#define R4X16_CODEC_FQZ      (3 << 24)
int rans4x16_hip_compress_best_qual_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                               const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                               const uint32_t *d_len, const uint32_t *d_flags, const uint64_t *d_rec_off, const uint32_t *d_nrec,
                                               int vers, int k, const int *methods,
                                               unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                               uint32_t *d_out_size, int32_t *d_status, int32_t *d_chosen, uint32_t *d_len_out,
                                               uint32_t max_in_size, uint32_t max_records, uint64_t total_in_size, void *stream);
int rans4x16_hip_best_qual_chunk_blocks(rans4x16_hip_ctx *ctx, int n, int k, const int *methods, uint32_t max_in_size,
                                        uint32_t max_records, uint64_t total_in_size);
int rans4x16_hip_uncompress_qual_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                            const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                            const int32_t *d_method,
                                            unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                            uint32_t *d_out_size, int32_t *d_status, const uint32_t *d_nosz_size,
                                            uint32_t *d_len, const uint64_t *d_len_off, const uint32_t *d_len_cap, uint32_t *d_nrec,
                                            uint32_t max_in_size, uint32_t max_out_size, void *stream);
int rans4x16_hip_compress_best_qual_batch(rans4x16_hip_ctx *ctx, int n,
                                          const unsigned char *const *in, const unsigned int *in_size,
                                          const unsigned int *nrec, uint32_t *const *len, uint32_t *const *flags, int vers,
                                          unsigned char **out, unsigned int *out_size,
                                          int k, const int *methods, int *chosen, int *status);
int rans4x16_hip_uncompress_qual_batch(rans4x16_hip_ctx *ctx, int n,
                                       const unsigned char *const *in, const unsigned int *in_size, const int *method,
                                       unsigned char *const *out, unsigned int *out_size, int *status,
                                       int *const *lengths, const int *nlengths, unsigned int *nrec);

/* ---- 2b. options ---------------------------------------------------------------------------
 * Everything that can be tuned or switched is an option of the context, set by name; the value is a long.
 * The R4X16_* environment variables named below only provide the DEFAULTS: they are read once per process, when the
 * first context is created (or the first option is asked for); no call path reads the environment.
 * ctx == NULL addresses the process-wide defaults: what contexts created from now on start with, and the
 * process-wide options at the end of the list.  Returns 0, or -1 for an unknown name.
 *
 *   name               default  environment default     meaning
 *   dec_direct            1     R4X16_DEC_DIRECT         decode: direct (short-step) rows for batches of up to N rounds of
 *                                                        resident direct streams; 0 = never
 *   enc_direct            1     R4X16_ENC_DIRECT         encode: the same for symbol records
 *   back_wg_per_cu        0     R4X16_BACK_WG_PER_CU     decode: run-length expansion by a workgroup per block up to N
 *                                                        blocks per compute unit (0: always one wave per block)
 *   dec_mid               0     R4X16_DEC_MID            decode: mid rows (bucket index + one 16-byte window of cumulative values) for
 *                                                        batches of up to N rounds of sixteen streams per compute unit; 0 = never
 *                                                        (built and measured in round 4, slower than the packed rows on quality data: off)
 *   dec_short_ring        0     R4X16_DEC_SHORT_RING     decode: packed rows of 43..44 symbols with a 128-byte word ring and four-step trips,
 *                                                        sixteen streams per wave instead of fifteen (measured slower per round: off)
 *   sched_sort            1     R4X16_SCHED_SORT         chain kernels: streams of a class ordered by length, longest first
 *   sched_claim           1     R4X16_SCHED_CLAIM        chain kernels: shares claimed from a counter (0: fixed stride)
 *   sched_concurrent      1     R4X16_SCHED_CONCURRENT   chain kernels: the classes of a batch side by side on six streams,
 *                                                        each with its share of the chip (0: one after the other)
 *   sched_trace           0     R4X16_SCHED_TRACE        the last batch's classes, and how this one's launches are dealt out, on stderr
 *   sched_learn           2     R4X16_SCHED_LEARN        bit 0 / bit 1: the encoder's / decoder's shares follow what the classes' launches of
 *                                                        the context's earlier batches really took (measured: the decoder gains 10 % on a
 *                                                        heterogeneous batch, the encoder's shares start to swing - so 2)
 *   max_workspace_mb  163840    R4X16_MAX_WS_MB          ceiling of the device workspace; larger batches are walked in chunks
 *   host_pipe_mb         64     R4X16_HOST_PIPE_MB       host batches of at least this many MiB (or 32 blocks) are pipelined
 *   host_threads          8     R4X16_HOST_THREADS       copier threads of the host pipeline
 *   host_lanes            2     R4X16_HOST_LANES         slabs of a host batch in flight at once
 *   host_slab_min_mb     32     R4X16_HOST_SLAB_MIN_MB   smallest slab
 *   host_dec_slabs / host_enc_slabs  0                   slabs per lane and round; 0 = by size (about 2.3 GB of input + capacity each)
 *   host_pack             1     R4X16_HOST_PACK          encode results gathered on the device before they cross PCIe
 *   host_stripe_dev       1     R4X16_HOST_STRIPE_DEV    X_STRIPE blocks of host batches through the device stripe kernels
 *   host_trace            0     R4X16_HOST_TRACE         timeline of a pipelined host batch on stderr
 *   dec_qpw, dec_qpw_small, dec_qpw_pk, dec_qpw_dir, enc_qpw, enc_waves, enc_qpw_rec, enc_qpw_cap, front_lds
 *                                                        tuning aids: streams per wave / workgroup of single classes
 *   route_count           0     R4X16_ROUTE_COUNT        1: keep the route read-out of rans4x16_hip_route_read (below); 0: nothing is
 *                                                        copied or recorded for it
 *   process-wide (ctx == NULL, before the first single-block or multi-device call):
 *   combine               1     R4X16_COMBINE            the five drop-in symbols go through the combiner
 *   combine_window_us    -1     R4X16_COMBINE_WINDOW_US  fixed gathering window (-1: adaptive)
 *   combine_max         256     R4X16_COMBINE_MAX        blocks per combined batch
 *   combine_workers       1     R4X16_COMBINE_WORKERS    worker threads per direction
 *   combine_max_mb     2048     R4X16_COMBINE_MAX_MB     buffer bytes per combined batch
 *   numa                  1     R4X16_NUMA               multi-device calls bind each device's worker to its NUMA node
 *   switches for A/B runs inside one library and for the tests (per context; set and read by name like the others, range
 *   0..1, but not in the list that rans4x16_hip_option_name walks - nothing to tune, the streams are the same either way):
 *   enc_affine            1     R4X16_ENC_AFFINE         encode: packed rows of the short-index kind whose alphabet is a run of consecutive
 *                                                        bytes compute their index words from the bytes (0: every wave looks them up)
 *
 * Every option has a range (0 keeps its meaning of "auto" / "never" where it has one; host_threads 1..32, host_lanes
 * 1..16, the dec_qpw* and enc_qpw_rec knobs 0..16, enc_qpw 0..31, enc_waves 0..4, enc_qpw_cap 1..64, switches 0..1,
 * sched_learn 0..3, combine_window_us -1..10^6, combine_workers 0..4; the counts and sizes 0 .. a large bound): a value
 * outside it is refused with -1 and the option keeps its value.  An environment default outside it is ignored.
 *
 * Contexts the library makes for itself follow the options of the context they work for: the lane contexts of the
 * host-batch pipeline take their parent's options (max_workspace_mb included) at every pipelined call, and the contexts
 * behind the five drop-in symbols (the combiner's, the per-thread ones) take the process-wide options at every batch.
 * The contexts of a rans4x16_hip_multi are the exception: they are made with the process-wide options of the moment of
 * rans4x16_hip_multi_create and keep them (there is no call to change them).
 */
int rans4x16_hip_set_option(rans4x16_hip_ctx *ctx, const char *name, long value);
int rans4x16_hip_get_option(const rans4x16_hip_ctx *ctx, const char *name, long *value);
/* Name of option number `index` (0, 1, ..), NULL past the last: lets a caller list what this build knows (the A/B switches
 * at the end of the table above excepted). */
const char *rans4x16_hip_option_name(int index);

/* Bytes of device workspace the context currently holds (grows on demand, never shrinks). */
size_t rans4x16_hip_workspace_bytes(const rans4x16_hip_ctx *ctx);

/* Timing hook for bench.py / rocprof cross-checks: when enabled, the *_dev calls bracket their
 * dominant ("chain") kernel with HIP events on the same stream; after synchronising, this
 * returns the accumulated milliseconds and launch count since the last reset. */
void rans4x16_hip_timing(rans4x16_hip_ctx *ctx, int enable);
int  rans4x16_hip_timing_read(rans4x16_hip_ctx *ctx, int which /*0 enc chain, 1 dec chain*/,
                              double *ms_total, int *launches, int reset);

/* Which routes a context's calls took (option route_count = 1; off, nothing is recorded).  The count of streams, blocks
 * or calls of each kind since the last reset, over the context's own *_dev calls and everything its host batches ran -
 * on the context itself or on its pipeline lanes.  `which` selects the list: */
enum {
    R4X16_ROUTE_ENCODE = 0,   /* encode chain: streams per row kind (R4X16_ENC_*)                                    */
    R4X16_ROUTE_DECODE = 1,   /* decode chain: streams per row kind (R4X16_DEC_*)                                    */
    R4X16_ROUTE_EXPAND = 2,   /* run-length expansion: blocks of the calls whose expansion kernel was that kind       */
    R4X16_ROUTE_LAUNCH = 3,   /* chain launches (encode and decode): in stream order, or classes side by side; the    */
                              /* arith call's chunks, in stream order                                                */
    R4X16_ROUTE_RESULT = 4,   /* encode results: blocks per way they reached the caller's memory (R4X16_RESULT_*)     */
    R4X16_ROUTE_NAMES = 5,    /* host-buffer names batches (part 2f): chunks and blocks (R4X16_NAMES_*)                */
    R4X16_ROUTE_ARITH = 6,    /* arith_dynamic decoding (part 2g): streams per home of their models (R4X16_ARITH_*)    */
    R4X16_ROUTE_ARITH_ENC = 7,/* arith_dynamic encoding (part 2h): candidate streams (R4X16_ARITH_ENC_*)               */
    R4X16_ROUTE_FQZ = 8,      /* fqzcomp_qual decoding (part 2i): decoded streams (R4X16_FQZ_*)                        */
    R4X16_ROUTE_ENCODE_BODY = 9,/* encode chain: streams per body of the pipelined loop (R4X16_ENC_BODY_*)               */
    R4X16_ROUTE_FQZ_ENC = 10, /* fqzcomp_qual encoding (part 2j): encoded streams (R4X16_FQZ_ENC_*)                    */
    R4X16_ROUTE_FQZ_PICK = 11,/* fqzcomp_qual's parameter choice on the device (part 2k): blocks (R4X16_FQZ_PICK_*)    */
    R4X16_ROUTE_FQZ_BEST = 12,/* fqzcomp_qual's best of several strategies (part 2l): R4X16_FQZ_BEST_*                  */
    R4X16_ROUTE_BEST_ANY = 13,/* best of several methods across codecs (part 2m): blocks and chunks (R4X16_BEST_ANY_*)  */
    R4X16_ROUTE_BEST_QUAL = 14/* quality blocks, best across three codecs (part 2n): R4X16_BEST_QUAL_*                  */
};
enum {   /* R4X16_ROUTE_DECODE: the decoder's row kinds (r4x16_common.h levels) */
    R4X16_DEC_L1 = 0,         /* packed 10-bit rows, 13..48 symbols                                                   */
    R4X16_DEC_L2 = 1,         /* u16 rows, two reads (up to 50 symbols; order-0 streams of such alphabets included)    */
    R4X16_DEC_L3 = 2,         /* u16 rows, three reads                                                                */
    R4X16_DEC_L4 = 3,         /* u16 rows, four reads                                                                 */
    R4X16_DEC_L5 = 4,         /* wide packed rows, 49..96 symbols                                                     */
    R4X16_DEC_DIRECT = 5,     /* level 6: the short-step rows (order-0 streams of them included)                      */
    R4X16_DEC_MID = 6,        /* level 10: mid rows                                                                   */
    R4X16_DEC_SHORT_RING = 7, /* packed rows with the short word ring                                                 */
    R4X16_DEC_KINDS = 8
};
enum {   /* R4X16_ROUTE_ENCODE: the encoder's row kinds */
    R4X16_ENC_U16 = 0, R4X16_ENC_PACKED = 1, R4X16_ENC_RECORDS = 2,
    R4X16_ENC_PACKED_FREQ = 3,/* those of the packed streams (counted there too) whose highest byte is below 128: the image  */
                              /* with the 128-byte index, coded from the 8-byte frequency table                              */
    R4X16_ENC_KINDS = 4
};
enum {   /* R4X16_ROUTE_ENCODE_BODY */
    R4X16_ENC_BODY_PACKED_AFFINE = 0, /* packed streams of the short-index kind (counted under R4X16_ROUTE_ENCODE too) in waves that  */
                                      /* took the affine body: every stream of the wave has a run of consecutive bytes for its       */
                                      /* alphabet, and option enc_affine is on                                                      */
    R4X16_ENC_BODY_KINDS = 1
};
enum { R4X16_EXPAND_WAVE = 0, R4X16_EXPAND_WORKGROUP = 1, R4X16_EXPAND_KINDS = 2 };               /* R4X16_ROUTE_EXPAND */
enum { R4X16_LAUNCH_IN_ORDER = 0, R4X16_LAUNCH_SIDE_BY_SIDE = 1, R4X16_LAUNCH_KINDS = 2 };        /* R4X16_ROUTE_LAUNCH */
enum {   /* R4X16_ROUTE_RESULT: device-resident encode calls, counted in blocks */
    R4X16_RESULT_IN_SLOT = 0, /* the slot calls (a host batch's own included): assembled in the bound-sized slot given       */
    R4X16_RESULT_DENSE = 1,   /* packed call, dense finish: assembled at its final offset, every byte moved once              */
    R4X16_RESULT_GATHERED = 2,/* packed call over the stripe / best-of-k routes: encoded into an internal slot, then copied    */
    R4X16_RESULT_KINDS = 3
};
enum {   /* R4X16_ROUTE_NAMES */
    R4X16_NAMES_ENC_CHUNKS = 0, /* chunks run by rans4x16_hip_tok3_encode_names_batch                                   */
    R4X16_NAMES_DEC_CHUNKS = 1, /* chunks run by rans4x16_hip_tok3_decode_names_batch                                   */
    R4X16_NAMES_UPLOADED = 2,   /* blocks uploaded, either direction                                                   */
    R4X16_NAMES_REFUSED = 3,    /* blocks refused before upload (above the size limit, refused by the scan)            */
    R4X16_NAMES_KINDS = 4
};
enum {   /* R4X16_ROUTE_ARITH: entropy-coded streams of rans4x16_hip_arith_uncompress_dev */
    R4X16_ARITH_O0 = 0,         /* order 0: the model in registers                                                     */
    R4X16_ARITH_O1_LDS = 1,     /* order 1, the rows in LDS                                                            */
    R4X16_ARITH_O1_GLOBAL = 2,  /* order 1, the rows in the context's arena in global memory                           */
    R4X16_ARITH_RLE = 3,        /* those of the three above that carry run lengths (counted there too)                 */
    R4X16_ARITH_KINDS = 4
};
enum {   /* R4X16_ROUTE_ARITH_ENC: candidate streams of rans4x16_hip_arith_compress_dev */
    R4X16_ARITH_ENC_O0 = 0,        /* coded with order 0: the model in registers                                        */
    R4X16_ARITH_ENC_O1_LDS = 1,    /* coded with order 1, the rows in LDS                                               */
    R4X16_ARITH_ENC_O1_GLOBAL = 2, /* coded with order 1, the rows in the context's arena in global memory              */
    R4X16_ARITH_ENC_RLE = 3,       /* those of the three above that carry run lengths (counted there too)               */
    R4X16_ARITH_ENC_STORED = 4,    /* candidates that came out as X_CAT: asked for, or ended no smaller than their input */
    R4X16_ARITH_ENC_KINDS = 5
};
enum {   /* R4X16_ROUTE_FQZ: streams rans4x16_hip_fqz_uncompress_dev sent to a decode wave */
    R4X16_FQZ_STREAMS = 0,      /* all of them                                                                         */
    R4X16_FQZ_TAB_LDS = 1,      /* the parameter blocks' tables in LDS (up to eight parameter blocks)                  */
    R4X16_FQZ_TAB_GLOBAL = 2,   /* the tables read from the context's arena                                            */
    R4X16_FQZ_DO_REV = 3,       /* with GFLAG_DO_REV: a record table and the reversal pass                             */
    R4X16_FQZ_MULTI_PARAM = 4,  /* with more than one parameter block                                                  */
    R4X16_FQZ_DUP = 5,          /* accepted streams in which a duplicate record was copied                             */
    R4X16_FQZ_KINDS = 6
};
enum {   /* R4X16_ROUTE_FQZ_ENC: streams rans4x16_hip_fqz_compress_dev sent to an encode wave */
    R4X16_FQZ_ENC_STREAMS = 0,      /* all of them                                                                     */
    R4X16_FQZ_ENC_TAB_LDS = 1,      /* the parameter blocks' tables in LDS (up to eight parameter blocks)              */
    R4X16_FQZ_ENC_TAB_GLOBAL = 2,   /* the tables read from the context's arena                                        */
    R4X16_FQZ_ENC_DO_REV = 3,       /* with GFLAG_DO_REV: coded from the coder-order copy                              */
    R4X16_FQZ_ENC_MULTI_PARAM = 4,  /* with more than one parameter block                                              */
    R4X16_FQZ_ENC_DUP = 5,          /* accepted streams (status 0) in which a record was coded as a duplicate          */
    R4X16_FQZ_ENC_KINDS = 6
};
enum {   /* R4X16_ROUTE_FQZ_PICK: blocks of rans4x16_hip_fqz_pick_dev / _compress_pick_dev */
    R4X16_FQZ_PICK_BLOCKS = 0,      /* picked (status 0)                                                               */
    R4X16_FQZ_PICK_SEL = 1,         /* picked with selectors coded (PFLAG_DO_SEL): the bins, the split or the caller's  */
    R4X16_FQZ_PICK_SPLIT = 2,       /* picked with the READ1 / READ2 split taken                                       */
    R4X16_FQZ_PICK_DEDUP = 3,       /* picked with PFLAG_DO_DEDUP                                                      */
    R4X16_FQZ_PICK_UNDECIDED = 4,   /* left to the host: R4X16_E_UNDECIDED                                             */
    R4X16_FQZ_PICK_HOST = 5,        /* blocks of a host-buffer batch picked on the host behind an undecided device pick */
    R4X16_FQZ_PICK_KINDS = 6
};
enum {   /* R4X16_ROUTE_FQZ_BEST: rans4x16_hip_fqz_compress_best_dev / _best_packed_dev / _best_batch */
    R4X16_FQZ_BEST_BLOCKS = 0,      /* blocks whose winner was written (status 0)                                      */
    R4X16_FQZ_BEST_CANDIDATES = 1,  /* candidate streams the encoder accepted, of the blocks that were decided          */
    R4X16_FQZ_BEST_COUNTED = 2,     /* slices whose histogram was counted: once each, whatever k is                     */
    R4X16_FQZ_BEST_UNDECIDED = 3,   /* blocks left R4X16_E_UNDECIDED by one of their candidates                         */
    R4X16_FQZ_BEST_REFUSED = 4,     /* candidates out of the running, of the blocks that were decided                   */
    R4X16_FQZ_BEST_KINDS = 5
};
enum {   /* R4X16_ROUTE_BEST_ANY: rans4x16_hip_compress_best_any_packed_dev / _best_any_batch */
    R4X16_BEST_ANY_RANS = 0,        /* blocks a rANS 4x16 method won (before the arena's capacity rule), ties included     */
    R4X16_BEST_ANY_ARITH = 1,       /* blocks an arith_dynamic method won, ties included                                 */
    R4X16_BEST_ANY_TIE = 2,         /* of those: both codecs' winners had the same size, the list position decided        */
    R4X16_BEST_ANY_FAILED = 3,      /* blocks without a winner (d_chosen -1)                                              */
    R4X16_BEST_ANY_CHUNKS = 4,      /* chunks the calls walked                                                            */
    R4X16_BEST_ANY_KINDS = 5
};
enum {   /* R4X16_ROUTE_BEST_QUAL: rans4x16_hip_compress_best_qual_packed_dev */
    R4X16_BEST_QUAL_BLOCKS = 0,     /* blocks the call compared                                                           */
    R4X16_BEST_QUAL_CHUNKS = 1,     /* chunks the call walked                                                             */
    R4X16_BEST_QUAL_RANS = 2,       /* blocks a rANS 4x16 method won (before the arena's capacity rule), ties included     */
    R4X16_BEST_QUAL_ARITH = 3,      /* blocks an arith_dynamic method won, ties included                                 */
    R4X16_BEST_QUAL_FQZ = 4,        /* blocks a fqzcomp_qual strategy won, ties included                                  */
    R4X16_BEST_QUAL_TIE = 5,        /* of the three above: two codecs' winners shared the smallest size, the list decided */
    R4X16_BEST_QUAL_FAILED = 6,     /* blocks without a winner (d_chosen -1) that were decided                            */
    R4X16_BEST_QUAL_UNDECIDED = 7,  /* blocks left R4X16_E_UNDECIDED by the fqzcomp sub-list                              */
    R4X16_BEST_QUAL_KINDS = 8
};
/* counts[k] = the count of kind k, for k < n; reset != 0 starts the counts of `which` afresh.  Waits for the work it counts (call
 * it after the calls, not while another thread uses the context).  Returns the number of kinds of `which`, -1 on error. */
int rans4x16_hip_route_read(rans4x16_hip_ctx *ctx, int which, long *counts, int n, int reset);

/* How many streams of one kind the chain kernel of this build keeps resident per compute unit (the unit of
 * parallelism is the stream): `nsym` symbols in the alphabet, order 0 / 1, table precision `shift`
 * (10 or 12; ignored for order 0).  Host arithmetic on the kernels' LDS size classes; bench.py reports it next
 * to the measured step latency, and sizes its batch in whole rounds of it.
 * `decode` may carry one of the flags below: the residency of the kind a stream takes in a batch that leaves LDS to
 * spare instead of the full chip's - R4X16_RES_SHORT: the short-step kind (decode: direct rows, encode: symbol records),
 * R4X16_RES_MID: the decoder's mid rows.  A batch of n blocks gives such a stream its kind while
 * ceil(n / (compute_units x dec_direct (enc_direct, dec_mid))) <= streams_per_cu.  Returns -1 if the stream can never
 * take that kind (alphabet, table precision or image size). */
#define R4X16_RES_SHORT 2
#define R4X16_RES_MID   4
int rans4x16_hip_residency(rans4x16_hip_ctx *ctx, int decode, unsigned int nsym, int order, unsigned int shift,
                           int *streams_per_cu, int *lanes_live_per_wave, int *compute_units);

/* Peak shader clock of the context's device in kHz (for cycles-per-step figures), -1 on error. */
int rans4x16_hip_device_clock_khz(rans4x16_hip_ctx *ctx);

/* Library/ABI version and the gfx target the code object was built for. */
const char *rans4x16_hip_version(void);

/* ---- 3. several GPUs of one node ---------------------------------------------------------------
 * Blocks are independent (every table travels in-band), so a batch is cut into contiguous ranges, one
 * per device, and each device runs the single-GPU pipeline on its range: no collective, no peer
 * traffic.  The split is the library's, not the caller's. */

/* Contiguous partition of n blocks into `parts` ranges of near-equal total weight (greedy on the
 * cumulative sum; a block goes to the range in which its midpoint falls).  Range r is
 * [bounds[r], bounds[r+1]); bounds has parts + 1 entries, bounds[0] = 0, bounds[parts] = n; ranges may
 * be empty.  weight == NULL means equal weights.  Pure host arithmetic, usable without a GPU (a
 * multi-process launcher calls it to find its rank's share).  Returns 0, or -1 on bad arguments. */
int rans4x16_hip_partition(int n, const unsigned int *weight, int parts, int *bounds);

typedef struct rans4x16_hip_multi rans4x16_hip_multi;

/* One context per listed device.  devices == NULL: devices 0 .. ndev-1; ndev <= 0: every visible device.
 * A device may be listed more than once (two pipelines on one card: how a one-GPU box rehearses the
 * multi-device path).  NULL if any context cannot be created. */
rans4x16_hip_multi *rans4x16_hip_multi_create(int ndev, const int *devices);
void                rans4x16_hip_multi_destroy(rans4x16_hip_multi *m);
int                 rans4x16_hip_multi_devices(const rans4x16_hip_multi *m);
const char         *rans4x16_hip_multi_last_error(const rans4x16_hip_multi *m);

/* rans4x16_hip_{compress,uncompress}_batch over all devices of `m`: the batch is partitioned by
 * uncompressed bytes (in_size for encode, the out_size capacities for decode), one host thread per
 * device runs its range through the host-buffer pipeline, and sizes / statuses land in the caller's
 * arrays in block order.  Same return value as the single-device calls. */
int rans4x16_hip_compress_batch_multi(rans4x16_hip_multi *m, int n,
                                      const unsigned char *const *in, const unsigned int *in_size,
                                      unsigned char *const *out, unsigned int *out_size,
                                      const int *order, int *status);
int rans4x16_hip_uncompress_batch_multi(rans4x16_hip_multi *m, int n,
                                        const unsigned char *const *in, const unsigned int *in_size,
                                        unsigned char *const *out, unsigned int *out_size,
                                        int *status);

/* Host feed of a multi-GPU node.  With eight devices the limiter is the host side: each device's
 * pipeline has eight copier threads moving the caller's buffers through pinned bounce buffers, and on a two-socket
 * node a copier on the wrong socket pushes every byte over the inter-socket link first.  The multi-device calls
 * therefore run each device's worker - and with it the copier threads it starts and the bounce buffers it
 * allocates - on the CPUs of the NUMA node the device hangs off (PCI bus id -> /sys/bus/pci/devices/<id>/numa_node
 * -> /sys/devices/system/node/node<N>/cpulist); the calling thread's own mask is restored afterwards.
 * R4X16_NUMA=0 switches it off; nothing happens where the node is unknown (-1) or the machine has one node. */

/* Parse a kernel "cpulist" ("0-15,32-47", "3", "0-3,8") into a bit mask of mask_bytes bytes (CPU c = bit c & 7 of byte
 * c >> 3).  Returns the number of CPUs set, or -1 on a malformed list or a CPU beyond the mask.  Pure text work,
 * usable (and tested) without a GPU. */
int rans4x16_hip_cpulist_parse(const char *list, unsigned char *mask, int mask_bytes);

/* NUMA node of a device of `m` (index into its device list) as the kernel reports it, -1 if unknown. */
int rans4x16_hip_multi_numa_node(const rans4x16_hip_multi *m, int index);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* RANS4X16_HIP_H */
