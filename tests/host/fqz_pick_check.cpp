// fqz_pick_check.cpp - runs htscodecs_amd/csrc/r4x16_fqz_pick.h on the host, alone: the parameter choice of fqzcomp_qual
// encoding (fqz_pick_parameters, fqz_qual_stats, fqz_store_parameters).  Built with g++ and
// -fsanitize=address,undefined and run as a program of its own (tests/test_fqz_enc_cpu.py).
//
// Input (argv[1]): cases behind each other - five little-endian 32-bit words (vers, strat, records, bytes, the capacity
// offered for the parameter bytes or 0xffffffff for "enough"), the record lengths, the record flags (32 bits each), the
// bytes.  Output: one line a case, "status size-of-the-parameter-bytes" and then, for status 0, the parameter bytes, the
// lengths and the flags as the call leaves them, in hex.  Every array is copied into a heap buffer of exactly its size,
// so a read or write beyond it stops the program under the sanitizer.  The capacity rule is
// rans4x16_hip_fqz_pick_parameters' (r4x16_fqz_enc.hip), restated here in three lines.
#include "r4x16_fqz_pick.h"

#include <stdio.h>
#include <stdlib.h>

template <class T> static T *exact(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: fqz_pick_check CASES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5];
    size_t cases = 0;
    while (fread(head, 4, 5, f) == 5) {
        const uint32_t nrec = head[2], size = head[3], cap = head[4];
        std::vector<uint32_t> len(nrec), flags(nrec);
        std::vector<uint8_t> in(size);
        if ((nrec && (fread(len.data(), 4, nrec, f) != nrec || fread(flags.data(), 4, nrec, f) != nrec)) ||
            (size && fread(in.data(), 1, size, f) != size)) { printf("FAILED: short case file\n"); return 1; }
        uint32_t *l = exact(len), *fl = exact(flags);
        uint8_t *bytes = exact(in);
        std::vector<uint8_t> out;
        std::vector<uint32_t> L, F;
        int st = fqp_pick((int)head[0], (int)head[1], (int)nrec, l, fl, bytes, size, out, L, F);
        if (st == FQP_OK && cap != 0xffffffffu && out.size() > cap) st = FQP_E_CAPACITY;
        printf("%d %zu", st, out.size());
        if (st == FQP_OK) {
            printf(" ");
            for (uint8_t b : out) printf("%02x", b);
            printf(" ");
            for (uint32_t i = 0; i < nrec; i++) printf("%08x", L[i]);
            printf(" ");
            for (uint32_t i = 0; i < nrec; i++) printf("%08x", F[i]);
        }
        printf("\n");
        free(l); free(fl); free(bytes);
        cases++;
    }
    fclose(f);
    printf("fqz_pick_check: ok %zu\n", cases);
    return 0;
}
