/*
 * tok3_hip - read names through the name tokeniser of librans4x16_hip.so (include/rans4x16_hip.h part 2f).
 *
 *   tok3_hip [-a] [-<level>] [-r] [in [out]]   names, one per line -> containers
 *   tok3_hip -d [-r] [in [out]]                containers -> names, one per line
 *
 * Without -r the input is cut into blocks of 1 MiB that end behind a line end (a partial last line is carried into the
 * next block, as a caller does with encode_names' last_start) and every container is written behind its 4-byte size,
 * little endian.  All blocks of a file go to the GPU in ONE batch call: a block alone is one wave on the chip.
 * -r: the whole input is one naked block (encode) or one naked container (decode), through the two single-block
 * functions.  Levels 1..9 select the method list as in the reference.  -a writes the arith flavour (use_arith = 1: the
 * columns go through the adaptive arithmetic coder), what the reference's command line spells as level + 10; levels from
 * 11 are refused here with a pointer to -a.  -d takes the flavour from the data, container by container: it always
 * asks for R4X16_TOK3_ARITH_DECODE, so a file of rANS containers alone also pays for the arith decoder's launches over
 * fully masked lists (under a millisecond a call, profiles/tok3_arith.md).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "../include/tok3_names_hip.h"

#define BLK_SIZE (1u << 20)

static unsigned char *load(FILE *fp, size_t *size)
{
    size_t cap = 1u << 20, n = 0, got;
    unsigned char *p = (unsigned char *)malloc(cap);
    if (!p) return NULL;
    while ((got = fread(p + n, 1, cap - n, fp)) > 0) {
        n += got;
        if (n == cap) {
            unsigned char *q = (unsigned char *)realloc(p, cap *= 2);
            if (!q) { free(p); return NULL; }
            p = q;
        }
    }
    *size = n;
    return p;
}

static int put(FILE *fp, const void *p, size_t n) { return fwrite(p, 1, n, fp) == n ? 0 : -1; }

static int fail(const char *what) { fprintf(stderr, "tok3_hip: %s\n", what); return 1; }

int main(int argc, char **argv)
{
    int decode = 0, raw = 0, arith = 0, level = 9, a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1]; a++) {
        if (!strcmp(argv[a], "-d")) decode = 1;
        else if (!strcmp(argv[a], "-r")) raw = 1;
        else if (!strcmp(argv[a], "-a")) arith = 1;
        else if (argv[a][1] >= '0' && argv[a][1] <= '9') level = atoi(argv[a] + 1);
        else {
            fprintf(stderr, "usage: tok3_hip [-d] [-r] [-a] [-<level 1..9>] [in [out]]\n");
            return 1;
        }
    }
    if (level >= 11) return fail("levels from 11 are not taken: for the arithmetic coder (use_arith) give -a and the level 1..9, -a -7 for -17");
    FILE *in = a < argc && strcmp(argv[a], "-") ? fopen(argv[a], "rb") : stdin;
    if (!in) { perror(argv[a]); return 1; }
    FILE *out = a + 1 < argc ? fopen(argv[a + 1], "wb") : stdout;
    if (!out) { perror(argv[a + 1]); return 1; }
    size_t size = 0;
    unsigned char *data = load(in, &size);
    if (!data) return fail("out of memory");

    if (raw) {
        if (size > 0x7fffffffu) return fail("the block is too large");
        if (decode) {
            uint32_t n = 0;
            unsigned char *names = decode_names(data, (uint32_t)size, &n);
            if (!names) return fail("decode_names failed");
            for (uint32_t i = 0; i < n; i++) if (!names[i]) names[i] = '\n';
            if (put(out, names, n) != 0) return fail("write error");
            free(names);
        } else {
            int n = 0, last_start = 0;
            unsigned char *c = encode_names((char *)data, (int)size, level, arith, &n, &last_start);
            if (!c) return fail("encode_names failed");
            if ((size_t)last_start < size) fprintf(stderr, "tok3_hip: %zu bytes behind the last line end were not encoded\n", size - (size_t)last_start);
            if (put(out, c, (size_t)n) != 0) return fail("write error");
            free(c);
        }
        free(data);
        return fclose(out) == 0 ? 0 : fail("write error");
    }

    /* the blocks of the file: where they start and how long they are */
    size_t nblk = 0, cap = 64;
    const unsigned char **ptr = (const unsigned char **)malloc(cap * sizeof(*ptr));
    unsigned int *len = (unsigned int *)malloc(cap * sizeof(*len));
    if (!ptr || !len) return fail("out of memory");
    for (size_t at = 0; at < size;) {
        size_t n;
        if (decode) {
            if (size - at < 4) return fail("truncated input: no container size");
            n = (size_t)data[at] | (size_t)data[at + 1] << 8 | (size_t)data[at + 2] << 16 | (size_t)data[at + 3] << 24;
            at += 4;
            if (n > size - at) return fail("truncated input: a container ends behind the file");
        } else {
            n = size - at < BLK_SIZE ? size - at : BLK_SIZE;
            if (at + n < size) {                       /* end the block behind its last line end */
                size_t e = n;
                while (e > 0 && data[at + e - 1] > '\n') e--;
                if (e == 0) return fail("a line longer than a block");
                n = e;
            }
        }
        if (nblk == cap) {
            cap *= 2;
            ptr = (const unsigned char **)realloc((void *)ptr, cap * sizeof(*ptr));
            len = (unsigned int *)realloc(len, cap * sizeof(*len));
            if (!ptr || !len) return fail("out of memory");
        }
        ptr[nblk] = data + at; len[nblk] = (unsigned int)n; nblk++;
        at += n;
    }
    rans4x16_hip_ctx *ctx = rans4x16_hip_create(-1);
    if (!ctx) return fail("no usable GPU");
    unsigned char **res = (unsigned char **)calloc(nblk ? nblk : 1, sizeof(*res));
    unsigned int *res_size = (unsigned int *)calloc(nblk ? nblk : 1, sizeof(*res_size));
    int *status = (int *)calloc(nblk ? nblk : 1, sizeof(*status));
    if (!res || !res_size || !status) return fail("out of memory");
    int methods[9], rc;
    if (rans4x16_hip_set_tok3_arith(ctx, decode ? R4X16_TOK3_ARITH_DECODE : arith ? R4X16_TOK3_ARITH_ENCODE : 0) < 0) return fail("set_tok3_arith");
    if (decode) rc = rans4x16_hip_tok3_decode_names_batch(ctx, (int)nblk, ptr, len, res, res_size, NULL, status);
    else rc = rans4x16_hip_tok3_encode_names_batch(ctx, (int)nblk, ptr, len, res, res_size, rans4x16_hip_tok3_level_methods(level, methods),
                                                   methods, NULL, NULL, status);
    if (rc < 0) { fprintf(stderr, "tok3_hip: %s\n", rans4x16_hip_last_error(ctx)); return 1; }
    for (size_t i = 0; i < nblk; i++) {
        if (status[i] != 0) { fprintf(stderr, "tok3_hip: block %zu failed with status %d\n", i, status[i]); return 1; }
        if (decode) {
            for (unsigned int j = 0; j < res_size[i]; j++) if (!res[i][j]) res[i][j] = '\n';
        } else {
            const unsigned char sz[4] = {(unsigned char)res_size[i], (unsigned char)(res_size[i] >> 8), (unsigned char)(res_size[i] >> 16),
                                         (unsigned char)(res_size[i] >> 24)};
            if (put(out, sz, 4) != 0) return fail("write error");
        }
        if (put(out, res[i], res_size[i]) != 0) return fail("write error");
        free(res[i]);
    }
    rans4x16_hip_destroy(ctx);
    free(res); free(res_size); free(status); free((void *)ptr); free(len); free(data);
    return fclose(out) == 0 ? 0 : fail("write error");
}
