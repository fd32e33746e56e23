// fqz_parse_check.cpp - runs htscodecs_amd/csrc/r4x16_fqz_parse.h on the host, alone: the header walk of fqzcomp_qual
// streams that the device's k_fq_front and the host calls share.  Built with g++ and -fsanitize=address,undefined and
// run as a program of its own (tests/test_fqz_cpu.py).
//
// Input (argv[1]): cases behind each other - two little-endian 32-bit words (stream length, capacity or 0xffffffff for
// none) and the stream.  Output: one line a case, "status stored_size header_bytes gflags nparam max_sel max_sym tables",
// tables being a checksum of everything the sink was given (0 for a refused stream).  Every stream is copied into a heap
// buffer of exactly its length, so a read beyond it stops the program under the sanitizer, and the source checks the
// index itself as well; the sink checks that every table entry lies inside its table and fits its width.
#include "r4x16_fqz_parse.h"

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

// the flat tables as the device lays them out: the selector table, then FQ_PARAM_BYTES a parameter block
struct Sink {
    std::vector<uint8_t> tab = std::vector<uint8_t>(FQ_STAB_BYTES + 256u * FQ_PARAM_BYTES, 0);
    bool bad = false;
    uint32_t params = 0;
    void put16(size_t at, uint32_t v) { if (v > 0xffffu) bad = true; tab[at] = (uint8_t)v; tab[at + 1] = (uint8_t)(v >> 8); }
    void stab(uint32_t i, uint32_t v) { if (i >= 256u) bad = true; else put16(2u * i, v); }
    void param(uint32_t k, const FqParam &pm)
    {
        if (k != params || k >= 256u) { bad = true; return; }
        params++;
        memcpy(&tab[FQ_STAB_BYTES + k * FQ_PARAM_BYTES], &pm, sizeof pm);
    }
    size_t base(uint32_t k) { if (k >= params) { bad = true; k = 0; } return FQ_STAB_BYTES + k * FQ_PARAM_BYTES; }
    void qmap(uint32_t k, uint32_t i, uint32_t v) { if (i >= 256u || v > 0xffu) bad = true; else tab[base(k) + FQ_OFF_QMAP + i] = (uint8_t)v; }
    void qtab(uint32_t k, uint32_t i, uint32_t v) { if (i >= 256u) bad = true; else put16(base(k) + FQ_OFF_QTAB + 2u * i, v); }
    void ptab(uint32_t k, uint32_t i, uint32_t v) { if (i >= 1024u) bad = true; else put16(base(k) + FQ_OFF_PTAB + 2u * i, v); }
    void dtab(uint32_t k, uint32_t i, uint32_t v) { if (i >= 256u) bad = true; else put16(base(k) + FQ_OFF_DTAB + 2u * i, v); }
};

static_assert(sizeof(FqParam) == 16, "the scalars of a parameter block take 16 bytes");

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: fqz_parse_check CASES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t head[2];
    size_t cases = 0;
    while (fread(head, 4, 2, f) == 2) {
        std::vector<uint8_t> buf(head[0]);
        if (head[0] && fread(buf.data(), 1, head[0], f) != head[0]) { printf("FAILED: short case file\n"); return 1; }
        uint8_t *exact = (uint8_t *)malloc(head[0] ? head[0] : 1);
        if (head[0]) memcpy(exact, buf.data(), head[0]);
        Src src{exact, head[0]};
        Sink sink;
        FqTop top;
        const int st = fq_parse(src, head[0], head[1], &top, sink);
        if (st == FQ_OK && (sink.bad || sink.params != top.nparam)) { printf("FAILED: case %zu: an accepted stream's tables break their bounds\n", cases); return 1; }
        if (st == FQ_OK && (top.hdr > head[0] || top.hdr < 10)) { printf("FAILED: case %zu: the header ends at %u of %u\n", cases, top.hdr, head[0]); return 1; }
        // the walk without a taker gives the same verdict
        FqNoSink none;
        FqTop again;
        if (fq_parse(src, head[0], head[1], &again, none) != st || again.hdr != top.hdr) { printf("FAILED: case %zu: the two walks differ\n", cases); return 1; }
        uint32_t sum = 0;
        if (st == FQ_OK) {
            const size_t n = FQ_STAB_BYTES + (size_t)top.nparam * FQ_PARAM_BYTES;
            for (size_t i = 0; i < n; i++) sum = sum * 31u + sink.tab[i];
        }
        printf("%d %u %u %u %u %u %u %u\n", st, top.out_size, top.hdr, top.gflags, top.nparam, top.max_sel, top.max_sym, sum);
        free(exact);
        cases++;
    }
    fclose(f);
    printf("fqz_parse_check: ok %zu\n", cases);
    return 0;
}
