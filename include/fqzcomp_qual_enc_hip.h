/*
 * fqzcomp_qual_enc_hip.h - fqz_compress of htscodecs/fqzcomp_qual.h under its own name, beside fqz_decompress
 * (fqzcomp_qual_hip.h, which this header includes), served by librans4x16_hip.so (include/rans4x16_hip.h parts 2i and
 * 2j).  A program that writes CRAM 3.1 quality blocks with the reference includes this header in place of
 * htscodecs/fqzcomp_qual.h and links the library; the call sites stay as they are.  (The encoder has a header of its own
 * because fqzcomp_qual_hip.h is the reader's and declares the decoder alone.)
 *
 * The function is static inline: the library exports rans4x16_hip_* names only, so a program that links libhtscodecs
 * as well gets no duplicate symbols.  Ownership and failure are the reference's: a malloc'ed buffer that the caller
 * free()s, *out_size its bytes, NULL on failure.  The stream is the reference's, byte for byte: its parameter choice
 * (strat 0 .. FQZ_MAX_STRAT, vers 3 for CRAM 3.0's orientation) and its encode loop.  s->len and s->flags are left as the
 * reference leaves them (lengths that overrun the buffer cut, the last record extended to its end, flags & 0xffff);
 * `in` is not modified.
 * gp must be NULL, as htslib passes it: fqz_gparams is opaque here, and a non-NULL gp returns NULL.  A caller with
 * parameters of its own hands them to rans4x16_hip_fqz_compress_batch as parameter bytes.
 * fqz_qual_stats as a call of its own and the test program's fqz_manual_parameters are not built; the parameter choice
 * alone is rans4x16_hip_fqz_pick_parameters, and over slices in device memory rans4x16_hip_fqz_pick_dev
 * (include/rans4x16_hip.h part 2k).  This call picks on the host whatever rans4x16_hip_set_fqz_pick says.
 */
#ifndef FQZCOMP_QUAL_ENC_HIP_H
#define FQZCOMP_QUAL_ENC_HIP_H

#include "fqzcomp_qual_hip.h"

/* Bit flags of fqz_slice.flags (bits 16 and up: a selector of the caller's) */
#define FQZ_FREVERSE 16
#define FQZ_FREAD2 128
/* The highest strategy fqz_compress takes from a CRAM writer */
#define FQZ_MAX_STRAT 3

/* Minimal per-record information of a slice: num_records, len[num_records], flags[num_records] */
typedef rans4x16_hip_fqz_slice fqz_slice;
typedef struct rans4x16_hip_fqz_gparams fqz_gparams;

static inline char *fqz_compress(int vers, fqz_slice *s, char *in, size_t in_size, size_t *out_size, int strat, fqz_gparams *gp)
{
    return rans4x16_hip_fqz_compress(vers, s, in, in_size, out_size, strat, gp);
}

#endif /* FQZCOMP_QUAL_ENC_HIP_H */
