/*
 * rans4x8_hip.h — rANS 4x8 (CRAM 3.0's codec) in librans4x16_hip.so, bit-exact with htscodecs 1.1's
 * rANS_static.c.  Same two layers as rans4x16_hip.h and the same context type (rans4x16_hip_create):
 *
 *  1. The two entry points of htscodecs/rANS_static.h:41-44, same names and ownership (results are malloc'd,
 *     the caller frees; NULL on failure).  Host buffers, a batch of one per call.
 *  2. Batch calls on host buffers and on device-resident buffers, with the argument meaning of the 4x16 ones.
 *
 * order: 0 / non-zero = order-1.  No CPU path: without a GPU every call fails.
 * On damaged input the device refuses a few streams the reference lets through with undefined results
 * (DESIGN.md 11); valid encoder output is never affected.
 */
#ifndef RANS4X8_HIP_H
#define RANS4X8_HIP_H

#include "rans4x16_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- 1. drop-in replacements (htscodecs/rANS_static.h:41-44) ---------------------------------- */
/* rANS_static.c:927-932.  in_size == 0 returns NULL (the reference divides by zero there). */
unsigned char *rans_compress(unsigned char *in, unsigned int in_size, unsigned int *out_size, int order);
/* rANS_static.c:934-943 */
unsigned char *rans_uncompress(unsigned char *in, unsigned int in_size, unsigned int *out_size);

/* ---- 2. batches -------------------------------------------------------------------------------- */
/* Capacity an output slot needs: what the reference allocates, (int)(1.05 * size) + 257*257*3 + 9
 * (rANS_static.c:87, :448). */
unsigned int rans4x8_hip_compress_bound(unsigned int size);

/* Host buffers; out_size[i] is the capacity on entry (encode: at least rans4x8_hip_compress_bound(in_size[i]);
 * decode: at least the uncompressed size stored in bytes 5..8 of the stream) and the size produced on return.
 * Returns the number of failed blocks (out_size 0, status != 0), -1 if the batch could not be run. */
int rans4x8_hip_compress_batch(rans4x16_hip_ctx *ctx, int n,
                               const unsigned char *const *in, const unsigned int *in_size,
                               unsigned char *const *out, unsigned int *out_size,
                               const int *order, int *status);
int rans4x8_hip_uncompress_batch(rans4x16_hip_ctx *ctx, int n,
                                 const unsigned char *const *in, const unsigned int *in_size,
                                 unsigned char *const *out, unsigned int *out_size, int *status);

/* Device-resident buffers (every pointer a DEVICE pointer; see rans4x16_hip_compress_dev for the layout).
 * The calls only enqueue work on `stream`.
 * PADDING: the decoder fetches a stream in aligned 16-byte pieces, so up to 15 bytes before a block's first byte and
 * after its last one are READ (never used): d_in must stay readable for 16 bytes beyond the end of its last block, and
 * a block must not start within 15 bytes of the start of the allocation unless that start is 16-byte aligned (any
 * hipMalloc'ed arena is).  The host-buffer calls above pad their own staging. */
int rans4x8_hip_compress_dev(rans4x16_hip_ctx *ctx, int n,
                             const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                             unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                             uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                             uint32_t max_in_size, void *stream);
int rans4x8_hip_uncompress_dev(rans4x16_hip_ctx *ctx, int n,
                               const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                               unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                               uint32_t *d_out_size, int32_t *d_status, void *stream);

/* ---- 2a. packed and best-of-two device-resident calls --------------------------------------------
 * The surface of rans4x16_hip.h part 2a for CRAM 3.0's codec: results back to back in ONE dense arena (a slot of the
 * bound is 1.05 x size + 198,156 bytes: 262,144 blocks of 4 KiB would want 53 GB of slots for 1 GiB of input), a decode
 * that takes the output sizes from the streams, and the writer's "try both orders, keep the smaller" as one call.
 * d_out_off is a device array of n + 1 entries that the call WRITES; out_capacity (host) is what d_out holds.  All five
 * only enqueue on `stream`, read nothing back, are ordered against the context's other calls like every *_dev call,
 * and walk the batch in chunks under max_workspace_mb and three quarters of the free device memory.  Statuses are the
 * R4X16_E_* codes.  They hold no output slots: the encoder's payload waits in the workspace and every result byte
 * moves once, to its final place.  Every loop of their kernels runs a launch argument's trips, or a size checked
 * against max_in_size / max_out_size first.
 *
 * rans4x8_hip_compress_packed_dev:
 *   - The bytes of block i, d_out_size[i] and d_status[i] are what rans4x8_hip_compress_dev gives for a slot of exactly
 *     rans4x8_hip_compress_bound(d_in_size[i]) bytes with the same order / d_order - the reference's fall to order 0 for
 *     in_size < 4 (rANS_static.c:438) and the refusal of in_size == 0 (R4X16_E_EMPTY) included.
 *   - d_out_off[0] = 0 and d_out_off[i + 1] = d_out_off[i] + the size of block i, a failed block counting 0.  The sums
 *     are taken BEFORE the capacity rule: d_out_off[n] is what the batch needs even if it did not fit.
 *   - Capacity rule: a block with d_out_off[i + 1] > out_capacity reports R4X16_E_CAPACITY with size 0 and nothing of it
 *     is written; its neighbours are not affected.  No byte at or beyond out_capacity and no byte outside the blocks'
 *     ranges is written.
 *   - A block larger than max_in_size reports R4X16_E_UNSUPPORTED and is not read.
 *
 * rans4x8_hip_compress_best_dev / rans4x8_hip_compress_best_packed_dev: every block with each of methods[0..k),
 * 1 <= k <= 2, each method 0 or 1 (a repeated method is allowed; anything else returns -1 and enqueues nothing).
 *   - Each candidate is what the slot call gives for that order in a slot of the bound.  The two run as 2 x n internal
 *     items over the same input; the chunks are planned for that.
 *   - The winner is the smallest candidate, the first in `methods` on a tie - blocks of fewer than 4 bytes always tie.
 *     Failed candidates are passed over; a block fails only if none is left, with the status of the first tried.
 *   - d_chosen[i] (device array, may be NULL) is the winner's INDEX into `methods`, -1 for a block that reports a status.
 *   - The slot form writes the winner to d_out + d_out_off[i] and obeys d_out_cap[i]: a winner that does not fit reports
 *     R4X16_E_CAPACITY (the slot need not hold the bound).  The packed form obeys the capacity rule above.
 *
 * rans4x8_hip_peek_dev: d_format[i] = byte 0 of the stream (-1 if there is none), d_raw_size[i] = bytes 5..8, little
 * endian.  d_status[i]: R4X16_E_EMPTY for a zero-length block; R4X16_E_TRUNCATED for fewer than 9 bytes
 * (rANS_static.c:938), d_raw_size then 0xFFFFFFFF; R4X16_E_UNSUPPORTED for a block above max_in_size, which is not read.
 * Nothing else is judged here: the decoder judges the rest.
 *
 * rans4x8_hip_uncompress_packed_dev:
 *   - Every block claims what peek reads.  A claim above max_out_size reports R4X16_E_UNSUPPORTED and takes 0 bytes;
 *     what peek refuses takes 0 bytes and keeps peek's status.
 *   - d_out_off is the exclusive scan of the claims, d_out_off[n] their total.  A block whose range ends beyond
 *     out_capacity reports R4X16_E_CAPACITY and is not decoded.
 *   - The other blocks are decoded exactly as rans4x8_hip_uncompress_dev decodes them with a capacity equal to the
 *     claim.  A block that fails while decoding keeps its range and reports size 0 (the bytes inside its own range are
 *     unspecified).  Nothing outside the ranges is written.  The PADDING rule above applies to d_in unchanged.
 * Sizing pass: the three packed calls take d_out == NULL with out_capacity == 0.  Nothing is written to an arena, every
 * block that needs room reports R4X16_E_CAPACITY, and d_out_off[n] is what the batch needs.
 * Route read-out (option route_count): the packed encodes count their blocks under R4X16_ROUTE_RESULT /
 * R4X16_RESULT_DENSE - best-of-two too, its winner is assembled in place -, rans4x8_hip_compress_best_dev under
 * R4X16_RESULT_IN_SLOT.
 * Return 0 if enqueued, -1 on argument / allocation / launch errors. */
int rans4x8_hip_compress_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                    const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                    unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                    uint32_t *d_out_size, int32_t *d_status, int order, const int32_t *d_order,
                                    uint32_t max_in_size, void *stream);
int rans4x8_hip_compress_best_dev(rans4x16_hip_ctx *ctx, int n,
                                  const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                  unsigned char *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap,
                                  uint32_t *d_out_size, int32_t *d_status,
                                  int k, const int *methods, int32_t *d_chosen, uint32_t max_in_size, void *stream);
int rans4x8_hip_compress_best_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                         unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                         uint32_t *d_out_size, int32_t *d_status,
                                         int k, const int *methods, int32_t *d_chosen, uint32_t max_in_size, void *stream);
int rans4x8_hip_peek_dev(rans4x16_hip_ctx *ctx, int n,
                         const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                         int32_t *d_format, uint32_t *d_raw_size, int32_t *d_status, uint32_t max_in_size, void *stream);
int rans4x8_hip_uncompress_packed_dev(rans4x16_hip_ctx *ctx, int n,
                                      const unsigned char *d_in, const uint64_t *d_in_off, const uint32_t *d_in_size,
                                      unsigned char *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                      uint32_t *d_out_size, int32_t *d_status,
                                      uint32_t max_in_size, uint32_t max_out_size, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RANS4X8_HIP_H */
