// arith_parse_check.cpp - runs htscodecs_amd/csrc/r4x16_arith_parse.h on the host, alone: the header walk of
// arith_dynamic streams that the device's k_ar_front and the host calls share.  Built with g++ and
// -fsanitize=address,undefined and run as a program of its own (tests/test_arith_cpu.py).
//
// Input (argv[1]): cases behind each other - four little-endian 32-bit words (stream length, capacity or 0xffffffff for
// none, planes reserved, largest stripe block) and the stream.  Output: one line a case, "status out_size pieces
// decoded", decoded being the bytes the core decoders and X_CAT copies of the accepted pieces give.  Every stream is
// copied into a heap buffer of exactly its length, so a read beyond it stops the program under the sanitizer, and the
// source checks the index itself as well.
#include "r4x16_arith_parse.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct Src {
    const uint8_t *p; uint32_t n;
    uint8_t at(uint32_t i) const
    {
        if (i >= n) { printf("FAILED: read of byte %u of a stream of %u\n", i, n); exit(1); }
        return p[i];
    }
};

struct Sink {
    uint32_t pieces = 0; uint64_t decoded = 0; uint32_t size; bool bad = false;
    void put(uint32_t j, const ArPiece &pc)
    {
        if (j != pieces) bad = true;
        pieces++;
        decoded += pc.dec_size;
        // an accepted piece's payload lies inside the stream, and a packed piece has the bytes its size needs
        if ((uint64_t)pc.in_pos + pc.in_size > size) bad = true;
        if (pc.kind == AR_K_CAT && pc.dec_size > pc.in_size) bad = true;
        if (pc.kind == AR_K_NONE && pc.dec_size) bad = true;
        if (pc.kind != AR_K_NONE && pc.in_size == 0) bad = true;
        if (pc.nsym != AR_NOT_PACKED && pc.nsym > 1 && (uint64_t)pc.dec_size * pc.nsym < pc.out_size) bad = true;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: arith_parse_check CASES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t head[4];
    size_t cases = 0;
    while (fread(head, 4, 4, f) == 4) {
        std::vector<uint8_t> buf(head[0]);
        if (head[0] && fread(buf.data(), 1, head[0], f) != head[0]) { printf("FAILED: short case file\n"); return 1; }
        uint8_t *exact = (uint8_t *)malloc(head[0] ? head[0] : 1);
        if (head[0]) memcpy(exact, buf.data(), head[0]);
        Src src{exact, head[0]};
        Sink sink;
        sink.size = head[0];
        ArTop top;
        const int st = ar_parse(src, head[0], head[1], head[2], head[3], &top, sink);
        if (st == AR_OK && sink.bad) { printf("FAILED: case %zu: an accepted piece breaks its own bounds\n", cases); return 1; }
        if (st == AR_OK && (top.flags & AR_X_STRIPE) && sink.pieces != top.nplanes) { printf("FAILED: case %zu: %u pieces of %u planes\n", cases, sink.pieces, top.nplanes); return 1; }
        printf("%d %u %u %llu\n", st, st == AR_OK ? top.out_size : 0u, st == AR_OK ? sink.pieces : 0u,
               st == AR_OK ? (unsigned long long)sink.decoded : 0ull);
        free(exact);
        cases++;
    }
    fclose(f);
    printf("arith_parse_check: ok %zu\n", cases);
    return 0;
}
