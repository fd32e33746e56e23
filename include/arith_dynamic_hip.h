/*
 * arith_dynamic_hip.h - arith_uncompress / arith_uncompress_to of htscodecs/arith_dynamic.h under their own names, served
 * by librans4x16_hip.so (include/rans4x16_hip.h part 2g).  A program that decodes with the reference's adaptive
 * arithmetic coder includes this header in place of htscodecs/arith_dynamic.h and links the library; the call sites
 * stay as they are.
 *
 * Decoding only: arith_compress, arith_compress_to and arith_compress_bound are not here, and a program that needs them
 * keeps libhtscodecs for them.  That is why the two functions are static inline: the library exports rans4x16_hip_*
 * names only, so linking both gives no duplicate symbols and this header promises no encoder.  Ownership and failure are
 * the reference's: out == NULL gives a malloc'ed buffer of the stream's stored size that the caller free()s, *out_size
 * holds the capacity of a given buffer on entry and the size on return, NULL on failure.
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

#endif /* ARITH_DYNAMIC_HIP_H */
