/* rans_ref_driver: the reference's rANS 4x16 and 4x8 entry points over a file of records, one forked child a record.
 *
 * A stand-alone host program of this project's own; oracle/Makefile links it with the reference's unchanged sources
 * into oracle/_ref/rans_ref (sanitizers on, nothing preloaded).  Test infrastructure only.
 *
 *   rans_ref IN OUT
 *
 * IN,  all numbers 32-bit little endian: a count, then per record: op, arg, paint, dirty, length, the bytes.
 *        op 0  rans_compress_to_4x16    arg = order (flags, N << 8); out = a heap buffer of rans_compress_bound_4x16 bytes
 *        op 1  rans_uncompress_to_4x16  arg = capacity: out = a heap buffer of that size, *out_size = capacity
 *        op 2  rans_uncompress_4x16     out == NULL: the callee sizes and allocates the result
 *        op 3  rans_compress   (4x8)    arg = order
 *        op 4  rans_uncompress (4x8)
 * OUT: the count, then per record: answer (0 refused: the call returned NULL; 1 made; 2 report), a value, and for
 *      `made` the value's bytes.  value: the result's length; for `report` the signal that ended the child, or
 *      0x100 | its exit status where it ended itself (a sanitizer's report does: -fno-sanitize-recover=all).
 *
 * Every record is worked in a child forked from a parent that has never called a codec, so the codecs' per-thread
 * tables are as a thread's first call finds them, and a crash or a sanitizer report costs that record alone.  In the
 * child the bytes are a heap copy of exactly their length; with `dirty` set, one fixed order-1 input over 256 symbols is
 * first encoded and decoded by both codecs (their tables are then as an earlier call left them); a function that is not
 * inlined fills 3 MiB of stack with the paint byte and returns, and the call follows directly.  What a call reads without
 * having written it is then the paint (stack), the earlier call's (tables), or the allocator's fill (heap: set from
 * outside, by the environment the program is started in).  Exit status: 0, 2 for a bad command line or file.
 */
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include "rANS_static4x16.h"
#include "rANS_static.h"

enum { OP_C16, OP_U16_TO, OP_U16, OP_C8, OP_U8, OP_COUNT };
enum { REFUSED, MADE, REPORT };
#define PAINT_BYTES (3u << 20)

static int get32(FILE *f, uint32_t *v)
{
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return -1;
    *v = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
    return 0;
}

static void enc32(unsigned char *b, uint32_t v)
{
    b[0] = v & 0xff; b[1] = v >> 8 & 0xff; b[2] = v >> 16 & 0xff; b[3] = v >> 24 & 0xff;
}

static void put32(FILE *f, uint32_t v)
{
    unsigned char b[4];
    enc32(b, v);
    fwrite(b, 1, 4, f);
}

static int write_all(int fd, const void *p, size_t n)
{
    const char *c = p;
    while (n) {
        ssize_t w = write(fd, c, n);
        if (w <= 0) return -1;
        c += w; n -= (size_t)w;
    }
    return 0;
}

static __attribute__((noinline)) void paint_stack(int byte)
{
    volatile unsigned char wall[PAINT_BYTES];
    memset((void *)wall, byte, sizeof(wall));
    __asm__ volatile("" : : "r"(wall) : "memory");
}

/* The tables of both codecs as an earlier, valid, order-1 call leaves them.  The input: 128 KiB, a walk over all 256 byte
 * values in steps of 0 to 15.  Order 1 pays, so the 4x16 stream is no X_CAT copy; every row of either decoder's tables is
 * filled; byte 0 follows only the bytes next to it, so the lowest slots of a row hold another symbol than the zeros of a
 * first call; and the 4x8 decoder, which numbers its rows as bytes first appear in the tables, numbers them nearly by
 * value, so that the slot 4095 it copies per context (rANS_static.c:799-800) lands in rows that are filled by then. */
static void dirty_tables(void)
{
    enum { N = 1 << 17 };
    unsigned char *in = malloc(N), *c, *u;
    unsigned int i, clen, ulen, x = 12345;
    if (!in) _exit(3);
    for (i = 0; i < N; i++) {
        x = x * 1103515245u + 12345u;
        in[i] = i ? (unsigned char)(in[i - 1] + (x >> 16 & 15)) : 0;
    }
    c = rans_compress_4x16(in, N, &clen, 1);
    u = c && (c[0] & 0x21) == 1 ? rans_uncompress_4x16(c, clen, &ulen) : NULL;
    if (!u || ulen != N || memcmp(u, in, N)) _exit(3);
    free(c); free(u);
    c = rans_compress(in, N, &clen, 1);
    u = c ? rans_uncompress(c, clen, &ulen) : NULL;
    if (!u || ulen != N || memcmp(u, in, N)) _exit(3);
    free(c); free(u); free(in);
}

static void child(int fd, uint32_t op, uint32_t arg, int paint, int dirty, const unsigned char *bytes, uint32_t len)
{
    unsigned char *in = malloc(len ? len : 1), *out = NULL, *res = NULL, head[8];
    unsigned int n = 0;
    if (!in) _exit(3);
    memcpy(in, bytes, len);
    if (op == OP_C16) { n = rans_compress_bound_4x16(len, (int)arg); out = malloc(n ? n : 1); }
    if (op == OP_U16_TO) { n = arg; out = malloc(n ? n : 1); }
    if ((op == OP_C16 || op == OP_U16_TO) && !out) _exit(3);
    if (dirty) dirty_tables();
    alarm(60);
    paint_stack(paint);
    switch (op) {
    case OP_C16:    res = rans_compress_to_4x16(in, len, out, &n, (int)arg); break;
    case OP_U16_TO: res = rans_uncompress_to_4x16(in, len, out, &n); break;
    case OP_U16:    res = rans_uncompress_4x16(in, len, &n); break;
    case OP_C8:     res = rans_compress(in, len, &n, (int)arg); break;
    default:        res = rans_uncompress(in, len, &n); break;
    }
    enc32(head, res ? MADE : REFUSED);
    enc32(head + 4, res ? n : 0);
    if (write_all(fd, head, 8) || (res && write_all(fd, res, n))) _exit(3);
    _exit(0);
}

int main(int argc, char **argv)
{
    FILE *in, *out;
    uint32_t count, k;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: rans_ref IN OUT\n");
        return 2;
    }
    if (get32(in, &count) < 0) return 2;
    put32(out, count);
    for (k = 0; k < count; k++) {
        uint32_t op, arg, paint, dirty, len, answer = REPORT, value = 0;
        unsigned char *bytes, *got = NULL, head[8];
        size_t have = 0, room = 0;
        int fds[2], status = 0;
        pid_t pid;
        if (get32(in, &op) < 0 || get32(in, &arg) < 0 || get32(in, &paint) < 0 || get32(in, &dirty) < 0 || get32(in, &len) < 0) return 2;
        if (op >= OP_COUNT || !(bytes = malloc(len ? len : 1)) || fread(bytes, 1, len, in) != len) return 2;
        fflush(out);
        if (pipe(fds) < 0 || (pid = fork()) < 0) return 2;
        if (pid == 0) {
            close(fds[0]);
            if (!getenv("RANS_REF_VERBOSE") && !freopen("/dev/null", "w", stderr)) _exit(3);
            child(fds[1], op, arg, (int)paint, (int)dirty, bytes, len);
        }
        close(fds[1]);
        for (;;) {
            ssize_t r;
            if (have == room) {
                room = room ? room * 2 : 1 << 16;
                if (!(got = realloc(got, room))) return 2;
            }
            r = read(fds[0], got + have, room - have);
            if (r <= 0) break;
            have += (size_t)r;
        }
        close(fds[0]);
        if (waitpid(pid, &status, 0) != pid) return 2;
        if (WIFSIGNALED(status)) value = (uint32_t)WTERMSIG(status);
        else if (WEXITSTATUS(status) != 0) value = 0x100u | (uint32_t)WEXITSTATUS(status);
        else if (have >= 8) {
            memcpy(head, got, 8);
            answer = head[0];
            value = head[4] | head[5] << 8 | head[6] << 16 | (uint32_t)head[7] << 24;
            if (answer > MADE || have != 8 + (size_t)(answer == MADE ? value : 0)) return 2;
        } else return 2;
        put32(out, answer);
        put32(out, value);
        if (answer == MADE) fwrite(got + 8, 1, value, out);
        free(got);
        free(bytes);
    }
    if (fclose(out) != 0) return 2;
    fclose(in);
    return 0;
}
