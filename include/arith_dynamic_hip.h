/*
 * arith_dynamic_hip.h - the five functions of htscodecs/arith_dynamic.h under their own names - arith_compress_bound,
 * arith_compress_to, arith_compress, arith_uncompress_to, arith_uncompress -, served by librans4x16_hip.so
 * (include/rans4x16_hip.h parts 2g and 2h).  A program that uses the reference's adaptive arithmetic coder includes this
 * header in place of htscodecs/arith_dynamic.h and links the library; the call sites stay as they are.
 *
 * The functions are static inline: the library exports rans4x16_hip_* names only, so a program that links libhtscodecs
 * as well gets no duplicate symbols.  Ownership and failure are the reference's: out == NULL gives a malloc'ed buffer
 * (decoding: of the stream's stored size; encoding: of arith_compress_bound) that the caller free()s, *out_size holds the
 * capacity of a given buffer on entry and the size on return, NULL on failure.  One deviation, on buffers the reference
 * itself mishandles: arith_compress_to with a buffer below rans4x16_hip_arith_compress_cap(in_size, order) returns NULL
 * and writes nothing; every larger buffer, the bound's included, gets the bytes of arith_compress.
 */
#ifndef ARITH_DYNAMIC_HIP_H
#define ARITH_DYNAMIC_HIP_H

#include "rans4x16_hip.h"

static inline unsigned char *arith_uncompress_to(unsigned char *in, unsigned int in_size,
                                                 unsigned char *out, unsigned int *out_size)
{
    return rans4x16_hip_arith_uncompress_to(in, in_size, out, out_size);
}

static inline unsigned char *arith_uncompress(unsigned char *in, unsigned int in_size, unsigned int *out_size)
{
    return rans4x16_hip_arith_uncompress(in, in_size, out_size);
}

static inline unsigned int arith_compress_bound(unsigned int size, int order)
{
    return rans4x16_hip_arith_compress_bound(size, order);
}

static inline unsigned char *arith_compress_to(unsigned char *in, unsigned int in_size,
                                               unsigned char *out, unsigned int *out_size, int order)
{
    return rans4x16_hip_arith_compress_to(in, in_size, out, out_size, order);
}

static inline unsigned char *arith_compress(unsigned char *in, unsigned int in_size, unsigned int *out_size, int order)
{
    return rans4x16_hip_arith_compress(in, in_size, out_size, order);
}

#endif /* ARITH_DYNAMIC_HIP_H */
