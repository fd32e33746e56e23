// r4x16_tok3_scan.hip - rans4x16_hip_tok3_scan and rans4x16_hip_tok3_scan_any (include/rans4x16_hip.h part 2c): the walk
// of r4x16_tok3_walk.h over a container in host memory; _any admits the arith flavour (use_arith != 0) as well.  Pure host
// arithmetic, no GPU, no HIP header: this unit also compiles as plain C++ (g++ -x c++), which is how its sanitizer run is
// built (profiles/tok3.md, profiles/tok3_arith.md).
#include "../../include/rans4x16_hip.h"
#include "r4x16_tok3_walk.h"

namespace {
struct HostSrc {
    const unsigned char *p;
    uint8_t at(uint32_t pos) const { return p[pos]; }
};
// the scan only needs what a later descriptor may ask of an earlier column
struct HostDir {
    uint8_t kind[T3_MAX_IDS];
    uint16_t id[T3_MAX_IDS];
    uint32_t a[T3_MAX_IDS], size[T3_MAX_IDS];
    void put(uint32_t c, int id_, int k, uint32_t a_, uint32_t, uint32_t s, uint32_t) { kind[c] = (uint8_t)k; id[c] = (uint16_t)id_; a[c] = a_; size[c] = s; }
    int kind_at(uint32_t c) const { return kind[c]; }
    int id_at(uint32_t c) const { return id[c]; }
    uint32_t a_at(uint32_t c) const { return a[c]; }
    uint32_t size_at(uint32_t c) const { return size[c]; }
};
}

static int scan(const unsigned char *in, size_t size, uint32_t max_columns, uint32_t max_col_size,
                uint32_t *last_start, uint32_t *nreads, uint32_t *ndesc, uint32_t *ncol,
                uint64_t *total_col_size, uint32_t *largest_col, uint32_t *largest_stream, bool admit_arith, int *use_arith)
{
    T3Sum sum = {};
    int rc;
    if ((!in && size) || max_columns > T3_MAX_IDS) return -1;
    if (size > 0xffffffffull) rc = T3_E_UNSUPPORTED;
    else {
        static thread_local HostDir dir;
        uint16_t map[T3_MAX_IDS];
        for (int i = 0; i < T3_MAX_IDS; i++) map[i] = T3_NONE;
        HostSrc src = {in};
        rc = t3_walk(src, (uint32_t)size, max_columns ? max_columns : T3_MAX_IDS, max_col_size ? max_col_size : 0xffffffffu, admit_arith, map, dir, &sum);
    }
    if (last_start) *last_start = sum.last_start;
    if (nreads) *nreads = sum.nreads;
    if (ndesc) *ndesc = sum.ndesc;
    if (ncol) *ncol = sum.ncol;
    if (total_col_size) *total_col_size = sum.total;
    if (largest_col) *largest_col = sum.max_col;
    if (largest_stream) *largest_stream = sum.max_stream;
    if (use_arith) *use_arith = (int)sum.arith;
    return rc;
}

extern "C" int rans4x16_hip_tok3_scan(const unsigned char *in, size_t size, uint32_t max_columns, uint32_t max_col_size,
                                      uint32_t *last_start, uint32_t *nreads, uint32_t *ndesc, uint32_t *ncol,
                                      uint64_t *total_col_size, uint32_t *largest_col, uint32_t *largest_stream)
{
    return scan(in, size, max_columns, max_col_size, last_start, nreads, ndesc, ncol, total_col_size, largest_col, largest_stream, false, nullptr);
}

extern "C" int rans4x16_hip_tok3_scan_any(const unsigned char *in, size_t size, uint32_t max_columns, uint32_t max_col_size,
                                          uint32_t *last_start, uint32_t *nreads, uint32_t *ndesc, uint32_t *ncol,
                                          uint64_t *total_col_size, uint32_t *largest_col, uint32_t *largest_stream, int *use_arith)
{
    return scan(in, size, max_columns, max_col_size, last_start, nreads, ndesc, ncol, total_col_size, largest_col, largest_stream, true, use_arith);
}
