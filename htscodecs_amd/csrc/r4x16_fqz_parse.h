// r4x16_fqz_parse.h - the header walk of one fqzcomp_qual stream (htscodecs fqzcomp_qual.c: read_array :150-194, the
// parameter reader :1162-1283, uncompress_block_fqz2f :1286-1334 up to RC_StartDecode), written once for the host
// (rans4x16_hip_fqz_scan, the host-buffer calls' checks, tests/host/fqz_parse_check.cpp) and the device (k_fq_front,
// r4x16_fqz.hip): what one reports the other reports, because it is the same text.  Nothing here needs HIP: a plain C++
// compiler takes it.
//
// A stream: the stored size as a varint; the version (5); gflags; nparam if GFLAG_MULTI_PARAM; max_sel and the selector
// table if GFLAG_HAVE_STAB; then per parameter block the start context (2 bytes), pflags, max_sym, three bytes of widths
// and locations (qbits | qshift, qloc | sloc, ploc | dloc), max_sym bytes of qmap if PFLAG_HAVE_QMAP, and qtab, ptab and
// dtab, each behind its flag, through read_array's two run-length levels.  The range coder's bytes follow.
//
// The sink takes what the decode loop needs as flat tables: per parameter block qmap as bytes (entries the stream does
// not store are (unsigned char)INT_MAX, as the reference's loop stores them), qtab, ptab << ploc and dtab << dloc as
// 16-bit values (the context is masked with 0xffff at the end of fqz_update_ctx, so the addends may be kept modulo
// 65,536), the selector table, and the block's scalars.
//
// Where the reference is undefined this walk refuses:
//   - read_array returns -1: the reader adds it to its index unchecked and leaves tables partly unwritten
//     (FQ_E_TABLE).  That covers a table read that starts at the end of the stream (nothing to read: -1), after
//     which `in_size - in_idx` would wrap.
//   - PFLAG_DO_SEL in a parameter block while max_sel == 0: the selector model is never initialised (FQ_E_TABLE).
// Everything else follows the reference.
//
// Loops: the varint is read inside [0, size); read_array's first level consumes an input byte a trip and stops at
// `avail`; its inner loop emits at most 1,024 values; the parameter loop runs nparam <= 255 trips, each of which
// consumes at least 7 bytes.  size is checked against the call's max_in_size before the walk starts.
#pragma once
#include <stdint.h>
#include "r4x16_arith_parse.h"      // AR_HD, ar_var_get (varint.h's var_get_u32)

enum { FQ_GFLAG_MULTI_PARAM = 1, FQ_GFLAG_HAVE_STAB = 2, FQ_GFLAG_DO_REV = 4 };
enum { FQ_PFLAG_DO_DEDUP = 2, FQ_PFLAG_DO_LEN = 4, FQ_PFLAG_DO_SEL = 8, FQ_PFLAG_HAVE_QMAP = 16, FQ_PFLAG_HAVE_PTAB = 32,
       FQ_PFLAG_HAVE_DTAB = 64, FQ_PFLAG_HAVE_QTAB = 128 };
// the status codes of include/rans4x16_hip.h the walk and the decode loop give
enum { FQ_OK = 0, FQ_E_CAPACITY = 1, FQ_E_TRUNCATED = 2, FQ_E_TABLE = 3, FQ_E_SIZE = 5, FQ_E_UNSUPPORTED = 6, FQ_E_CONTEXT = 7,
       FQ_E_EMPTY = 9 };
#define FQ_VERS 5u
#define FQ_NO_CAP 0xffffffffu

// A parameter block's flat tables: 16 bytes of scalars, then qmap, qtab, ptab, dtab
struct FqParam {
    uint16_t context, qmask;
    uint8_t pflags, qshift, qloc, sloc;
    uint8_t max_sym, pad[7];
};
#define FQ_OFF_QMAP 16u
#define FQ_OFF_QTAB (FQ_OFF_QMAP + 256u)
#define FQ_OFF_PTAB (FQ_OFF_QTAB + 512u)
#define FQ_OFF_DTAB (FQ_OFF_PTAB + 2048u)
#define FQ_PARAM_BYTES (FQ_OFF_DTAB + 512u)         // 3,344: the 3,328 bytes of tables and the scalars
#define FQ_STAB_BYTES 512u                          // the selector table as 16-bit values

struct FqTop {
    uint32_t out_size;              // the stored size
    uint32_t hdr;                   // bytes in front of the range coder's input
    uint32_t gflags, nparam, max_sel, max_sym;
};

// what the walk does without a taker
struct FqNoSink {
    AR_HD void stab(uint32_t, uint32_t) {}
    AR_HD void param(uint32_t, const FqParam &) {}
    AR_HD void qmap(uint32_t, uint32_t, uint32_t) {}
    AR_HD void qtab(uint32_t, uint32_t, uint32_t) {}
    AR_HD void ptab(uint32_t, uint32_t, uint32_t) {}
    AR_HD void dtab(uint32_t, uint32_t, uint32_t) {}
};

// read_array (:150-194) over [pos, pos + avail): array[j] = value for j < min(1024, size) through put(j, value).  The
// first level's output is fed to the second as it is made instead of through R[1024]: the second level reads R from
// its start and stops when the array is full, and either level's -1 is the call's -1.  Bytes consumed, or -1.
template <class SRC, class PUT>
AR_HD inline int fq_read_array(SRC &in, uint32_t pos, uint32_t avail, uint32_t size, PUT &put)
{
    if (size > 1024u) size = 1024u;
    uint32_t i = 0, nr = 0;             // level one: input index, values written to R
    int z = 0, last = -1;
    uint32_t j = 0, val = 0, run_len = 0;   // level two: array index, the value of the run, its length so far
    for (; z < (int)size && i < avail; i++) {
        const int run = in.at(pos + i);
        int copy = 0;
        bool first = true;
        z += run;
        if (run == last) {
            if (i + 1 >= avail) return -1;
            copy = in.at(pos + ++i);
            z += run * copy;
        }
        // R gets `run` once, then again while (copy-- && z < size && nr < 1024)
        for (;;) {
            if (!first) { if (!(copy-- && z < (int)size && nr < 1024u)) break; }
            first = false;
            nr++;
            if (j < size) {                                          // level two takes R[nr - 1]
                run_len += (uint32_t)run;
                if (run != 255) {
                    while (run_len && j < size) { run_len--; put.set(j++, val); }
                    run_len = 0;
                    val++;
                }
            }
            if (run != last) break;
        }
        if (nr >= 1024u) return -1;
        last = run;
    }
    if (j < size) return -1;                                         // R ran out: z >= R_max, or inside a chain of 255s
    return (int)i;
}

template <class SINK> struct FqPutStab { SINK &s; AR_HD void set(uint32_t j, uint32_t v) { s.stab(j, v); } };
template <class SINK> struct FqPutQtab { SINK &s; uint32_t k; AR_HD void set(uint32_t j, uint32_t v) { s.qtab(k, j, v & 0xffffu); } };
template <class SINK> struct FqPutPtab { SINK &s; uint32_t k, loc; AR_HD void set(uint32_t j, uint32_t v) { s.ptab(k, j, (v << loc) & 0xffffu); } };
template <class SINK> struct FqPutDtab { SINK &s; uint32_t k, loc; AR_HD void set(uint32_t j, uint32_t v) { s.dtab(k, j, (v << loc) & 0xffffu); } };

// The whole header of a stream of `size` bytes.  cap: the caller's capacity, FQ_NO_CAP for none.
template <class SRC, class SINK>
AR_HD inline int fq_parse(SRC &in, uint32_t size, uint32_t cap, FqTop *top, SINK &sink)
{
    top->out_size = top->hdr = top->gflags = top->nparam = top->max_sel = top->max_sym = 0;
    if (size == 0) return FQ_E_EMPTY;
    uint32_t len = 0;
    uint32_t q = ar_var_get(in, 0, size, &len);                      // :1300
    top->out_size = len;
    if (size - q < 10) return FQ_E_TRUNCATED;                        // :1234
    if (in.at(q++) != FQ_VERS) return FQ_E_UNSUPPORTED;              // :1239
    const uint32_t gflags = in.at(q++);
    const uint32_t nparam = (gflags & FQ_GFLAG_MULTI_PARAM) ? in.at(q++) : 1u;
    if (nparam == 0) return FQ_E_SIZE;                               // :1247
    uint32_t max_sel = nparam > 1 ? nparam : 0;
    if (gflags & FQ_GFLAG_HAVE_STAB) {
        max_sel = in.at(q++);
        FqPutStab<SINK> put{sink};
        const int r = fq_read_array(in, q, size - q, 256u, put);
        if (r < 0) return FQ_E_TABLE;
        q += (uint32_t)r;
    } else
        for (uint32_t i = 0; i < 256u; i++) sink.stab(i, i < nparam ? i : nparam - 1u);
    uint32_t max_sym = 0;
    for (uint32_t k = 0; k < nparam; k++) {                          // :1163-1227
        const uint32_t avail = size - q;
        if (avail < 7) return FQ_E_TRUNCATED;
        FqParam pm;
        pm.context = (uint16_t)(in.at(q) | (in.at(q + 1) << 8));
        pm.pflags = in.at(q + 2);
        pm.max_sym = in.at(q + 3);
        const uint32_t qbits = in.at(q + 4) >> 4;
        pm.qmask = (uint16_t)((1u << qbits) - 1u);
        pm.qshift = in.at(q + 4) & 15u;
        pm.qloc = in.at(q + 5) >> 4;
        pm.sloc = in.at(q + 5) & 15u;
        const uint32_t ploc = in.at(q + 6) >> 4, dloc = in.at(q + 6) & 15u;
        for (int x = 0; x < 7; x++) pm.pad[x] = 0;
        uint32_t idx = 7;
        if ((pm.pflags & FQ_PFLAG_DO_SEL) && max_sel == 0) return FQ_E_TABLE;
        sink.param(k, pm);
        if (pm.pflags & FQ_PFLAG_HAVE_QMAP) {
            if (idx + pm.max_sym > avail) return FQ_E_TRUNCATED;     // :1197
            for (uint32_t i = 0; i < 256u; i++) sink.qmap(k, i, i < pm.max_sym ? in.at(q + idx + i) : 0xffu);
            idx += pm.max_sym;
        } else
            for (uint32_t i = 0; i < 256u; i++) sink.qmap(k, i, i);
        if (qbits && (pm.pflags & FQ_PFLAG_HAVE_QTAB)) {
            FqPutQtab<SINK> put{sink, k};
            const int r = fq_read_array(in, q + idx, avail - idx, 256u, put);
            if (r < 0) return FQ_E_TABLE;
            idx += (uint32_t)r;
        } else
            for (uint32_t i = 0; i < 256u; i++) sink.qtab(k, i, i);   // (without qbits the reference leaves it unset: masked with 0)
        if (pm.pflags & FQ_PFLAG_HAVE_PTAB) {
            FqPutPtab<SINK> put{sink, k, ploc};
            const int r = fq_read_array(in, q + idx, avail - idx, 1024u, put);
            if (r < 0) return FQ_E_TABLE;
            idx += (uint32_t)r;
        } else
            for (uint32_t i = 0; i < 1024u; i++) sink.ptab(k, i, 0);
        if (pm.pflags & FQ_PFLAG_HAVE_DTAB) {
            FqPutDtab<SINK> put{sink, k, dloc};
            const int r = fq_read_array(in, q + idx, avail - idx, 256u, put);
            if (r < 0) return FQ_E_TABLE;
            idx += (uint32_t)r;
        } else
            for (uint32_t i = 0; i < 256u; i++) sink.dtab(k, i, 0);
        q += idx;
        if (max_sym < pm.max_sym) max_sym = pm.max_sym;
    }
    top->hdr = q;
    top->gflags = gflags; top->nparam = nparam; top->max_sel = max_sel; top->max_sym = max_sym;
    if (cap != FQ_NO_CAP && cap < len) return FQ_E_CAPACITY;
    return FQ_OK;
}
