/*
 * fqzcomp_qual_hip.h - fqz_decompress of htscodecs/fqzcomp_qual.h under its own name, served by librans4x16_hip.so
 * (include/rans4x16_hip.h part 2i).  A program that reads CRAM 3.1 quality blocks with the reference includes this
 * header in place of htscodecs/fqzcomp_qual.h and links the library; the call sites stay as they are.
 *
 * The function is static inline: the library exports rans4x16_hip_* names only, so a program that links libhtscodecs
 * as well gets no duplicate symbols.  Ownership and failure are the reference's: a malloc'ed buffer of the stream's
 * stored size that the caller free()s, *out_size the stored size, lengths[rec] the length of record rec for
 * rec < nlengths (lengths may be NULL), NULL on failure.
 *
 * This header is the reader's: it declares the decoder alone.  A program that writes quality blocks includes
 * fqzcomp_qual_enc_hip.h, which includes this header and adds the reference's encode call with fqz_slice, the FQZ_F*
 * flags and FQZ_MAX_STRAT (include/rans4x16_hip.h part 2j).  fqz_qual_stats as a call of its own is not built (the pick runs it: part 2j on the host, part 2k on the device).
 */
#ifndef FQZCOMP_QUAL_HIP_H
#define FQZCOMP_QUAL_HIP_H

#include <stddef.h>
#include "rans4x16_hip.h"

static inline char *fqz_decompress(char *in, size_t in_size, size_t *out_size, int *lengths, int nlengths)
{
    return rans4x16_hip_fqz_decompress(in, in_size, out_size, lengths, nlengths);
}

#endif /* FQZCOMP_QUAL_HIP_H */
