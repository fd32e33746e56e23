/* tok3_ref_driver: the reference's encode_names and decode_names over a file of name blocks.
 *
 * A stand-alone host program of this project's own; oracle/Makefile links it with the reference's unchanged sources
 * into oracle/_ref/tok3_ref (sanitizers on, nothing preloaded).  Test infrastructure only.
 *
 *   tok3_ref IN OUT
 *
 * IN,  all numbers 32-bit little endian: a count, then per block: level, use_arith, length, the bytes.
 * OUT: the count, then per block: made (1, or 0 where encode_names returned NULL), last_start, the container's length,
 *      the container, and back: 1 where decode_names gave the block's first last_start bytes with every byte <= '\n' a
 *      NUL, else 0.
 *
 * Every block is handed over as a heap copy of exactly its length, the container likewise, so that a read beyond
 * either is the sanitizer's to report.  Exit status: 0, 2 for a bad command line or file; the sanitizers end the run
 * themselves (-fno-sanitize-recover=all).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tokenise_name3.h"

static int get32(FILE *f, uint32_t *v)
{
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return -1;
    *v = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
    return 0;
}

static void put32(FILE *f, uint32_t v)
{
    unsigned char b[4] = {v & 0xff, v >> 8 & 0xff, v >> 16 & 0xff, v >> 24 & 0xff};
    fwrite(b, 1, 4, f);
}

int main(int argc, char **argv)
{
    FILE *in, *out;
    uint32_t n, k;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: tok3_ref IN OUT\n");
        return 2;
    }
    if (get32(in, &n) < 0) return 2;
    put32(out, n);
    for (k = 0; k < n; k++) {
        uint32_t level, use_arith, len, i;
        char *blk, *work;
        uint8_t *comp;
        int comp_len = 0, last_start = 0, back = 0;
        if (get32(in, &level) < 0 || get32(in, &use_arith) < 0 || get32(in, &len) < 0) return 2;
        blk = malloc(len ? len : 1);
        work = malloc(len ? len : 1);
        if (!blk || !work || fread(blk, 1, len, in) != len) return 2;
        memcpy(work, blk, len);                              /* encode_names writes NULs into its input */
        comp = encode_names(work, (int)len, (int)level, (int)use_arith, &comp_len, &last_start);
        if (comp) {
            uint8_t *exact = malloc(comp_len ? comp_len : 1), *names;
            uint32_t names_len = 0;
            if (!exact) return 2;
            memcpy(exact, comp, comp_len);
            names = decode_names(exact, (uint32_t)comp_len, &names_len);
            if (names && names_len == (uint32_t)last_start) {
                back = 1;
                for (i = 0; i < names_len; i++)
                    if (names[i] != ((unsigned char)blk[i] <= '\n' ? 0 : (unsigned char)blk[i])) back = 0;
            }
            free(names);
            put32(out, 1);
            put32(out, (uint32_t)last_start);
            put32(out, (uint32_t)comp_len);
            fwrite(exact, 1, comp_len, out);
            put32(out, (uint32_t)back);
            free(exact);
            free(comp);
        } else {
            put32(out, 0);
            put32(out, (uint32_t)last_start);
            put32(out, 0);
            put32(out, 0);
        }
        free(blk);
        free(work);
    }
    if (fclose(out) != 0) return 2;
    fclose(in);
    return 0;
}
