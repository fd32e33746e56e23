/*
 * tok3_names_hip.h - encode_names / decode_names of htscodecs/tokenise_name3.h under their own names, served by
 * librans4x16_hip.so (include/rans4x16_hip.h part 2f).  A program that calls the reference's name tokeniser includes
 * this header in place of htscodecs/tokenise_name3.h and links the library; the call sites stay as they are.
 *
 * The two functions are static inline on purpose: the library exports rans4x16_hip_* names only, so a program that
 * also links libhtscodecs for its other codecs has no duplicate symbols.  Ownership and failure are the reference's:
 * a malloc'ed result the caller free()s, NULL on failure.  Both flavours are served: encode_names with use_arith != 0 and
 * decode_names of a container whose byte 8 (use_arith) is set go to the library's functions for the adaptive arithmetic
 * coder (rans4x16_hip_tok3_arith_encode_names / _decode_names), everything else to the rANS ones.
 */
#ifndef TOK3_NAMES_HIP_H
#define TOK3_NAMES_HIP_H

#include "rans4x16_hip.h"

static inline unsigned char *encode_names(char *blk, int len, int level, int use_arith,
                                          int *out_len, int *last_start_p)
{
    if (use_arith) return rans4x16_hip_tok3_arith_encode_names(blk, len, level, out_len, last_start_p);
    return rans4x16_hip_tok3_encode_names(blk, len, level, 0, out_len, last_start_p);
}

static inline unsigned char *decode_names(unsigned char *in, uint32_t sz, uint32_t *out_len)
{
    if (in && sz > 8 && in[8]) return rans4x16_hip_tok3_arith_decode_names(in, sz, out_len);
    return rans4x16_hip_tok3_decode_names(in, sz, out_len);
}

#endif /* TOK3_NAMES_HIP_H */
