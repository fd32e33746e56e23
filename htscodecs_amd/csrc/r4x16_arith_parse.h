// r4x16_arith_parse.h - the header walk of one arith_dynamic stream (htscodecs arith_dynamic.c:870-1045,
// arith_uncompress_to up to the point where a core decoder is called, with pack.c's hts_unpack_meta and the size test
// of hts_unpack), written once for the host (rans4x16_hip_arith_uncompress*'s checks, tests/host/arith_parse_check.cpp)
// and the device (k_ar_front, r4x16_arith.hip): what one reports the other reports, because it is the same text.
// Nothing here needs HIP: a plain C++ compiler takes it.
//
// A stream: the flag byte; the stored size as a varint unless X_NOSZ; under X_PACK the symbol map (count, symbols) and
// the packed size; then the payload of a core coder (order 0 / 1, with or without run lengths), of X_CAT (the bytes
// themselves) or of X_EXT (bzip2, not supported).  Under X_STRIPE instead: the size, N, N varint lengths, N streams.
//
// The core decoders never refuse, so everything the reference refuses is refused here, and a piece that this walk
// accepts decodes to exactly piece.out_size bytes.  Deviations, on malformed input only: a plane that is itself an
// X_STRIPE stream, and a stripe block with more planes or bytes than the caller's limits, report UNSUPPORTED; N == 0
// with a size above 0 reports SIZE (the reference's unstripe does not return from it).
//
// Loops: a varint is read inside [pos, end) with end <= size; the symbol map reads at most 16 bytes; the plane loop
// runs N <= 255 trips.  size is checked against the call's max_in_size before the walk starts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AR_HD __host__ __device__
#else
#define AR_HD
#endif

enum { AR_X_PACK = 0x80, AR_X_RLE = 0x40, AR_X_CAT = 0x20, AR_X_NOSZ = 0x10, AR_X_STRIPE = 0x08, AR_X_EXT = 0x04 };
// the status codes of include/rans4x16_hip.h the walk gives
enum { AR_OK = 0, AR_E_CAPACITY = 1, AR_E_TRUNCATED = 2, AR_E_SIZE = 5, AR_E_UNSUPPORTED = 6, AR_E_EMPTY = 9 };
// what fills a piece's decoded bytes
enum { AR_K_NONE = 0, AR_K_CAT = 1, AR_K_O0 = 2, AR_K_O1 = 3, AR_K_O0_RLE = 4, AR_K_O1_RLE = 5 };
#define AR_NOT_PACKED 0xffu
#define AR_INT_MAX 0x7fffffffu
#define AR_NO_CAP 0xffffffffu       // "out == NULL": the size comes from the stream

struct ArPiece {
    uint32_t in_pos, in_size;       // the payload inside the stream: [in_pos, in_pos + in_size)
    uint32_t dec_size;              // bytes the core decoder (or the X_CAT copy) gives; 0 for AR_K_NONE
    uint32_t out_size;              // bytes of the piece once unpacked
    uint8_t kind;                   // AR_K_*
    uint8_t nsym;                   // X_PACK: values per byte 0, 1, 2, 4, 8; AR_NOT_PACKED without
    uint8_t map[16];                // X_PACK: code -> symbol (entries the stream does not give are 0)
};

struct ArTop {
    uint32_t flags, out_size;       // byte 0; the block's size
    uint32_t nplanes;               // 0: not a stripe block (one piece)
};

// varint.h:131-160 over [pos, end): bytes consumed, 0 if there is none (*v = 0 then)
template <class SRC>
AR_HD inline uint32_t ar_var_get(SRC &s, uint32_t pos, uint32_t end, uint32_t *v)
{
    uint32_t acc = 0, p = pos;
    uint8_t c;
    *v = 0;
    if (pos >= end) return 0;
    do {
        c = s.at(p++);
        acc = (acc << 7) | (c & 0x7fu);
    } while ((c & 0x80) && p < end);
    *v = acc;
    return p - pos;
}

// One stream without X_STRIPE at [pos, end) (:954-1045, :1091-1102).  cap: the caller's capacity, AR_NO_CAP for none.
template <class SRC>
AR_HD inline int ar_parse_piece(SRC &in, uint32_t pos, uint32_t end, uint32_t cap, ArPiece *pc)
{
    const uint32_t flags = in.at(pos);
    uint32_t p = pos + 1, osz = 0;
    pc->in_pos = pc->in_size = pc->dec_size = pc->out_size = 0;
    pc->kind = AR_K_NONE;
    pc->nsym = AR_NOT_PACKED;
    for (int k = 0; k < 16; k++) pc->map[k] = 0;
    if (flags & AR_X_NOSZ) {
        if (cap == AR_NO_CAP) return AR_E_SIZE;                                          // :980 "need one or the other"
        osz = cap;
    } else p += ar_var_get(in, p, end, &osz);
    if (osz >= AR_INT_MAX) return AR_E_SIZE;                                             // :971
    if (cap != AR_NO_CAP && cap < osz) return AR_E_CAPACITY;                             // :988
    uint32_t dec = osz;
    if (flags & AR_X_PACK) {                                                             // pack.c:165-198
        if (p >= end) return AR_E_TRUNCATED;
        uint32_t n = in.at(p);
        if (n == 0) n = 256;
        if (n > 16) { pc->nsym = 1; p += 1; }
        else {
            pc->nsym = n <= 1 ? 0 : n <= 2 ? 8 : n <= 4 ? 4 : 2;
            if (end - p <= 1) return AR_E_TRUNCATED;
            uint32_t j = 1, c = 0;
            do pc->map[c++] = in.at(p + j++); while (c < n && j < end - p);
            if (c < n) return AR_E_TRUNCATED;
            p += j;
        }
        p += ar_var_get(in, p, end, &dec);
        if (dec > osz) return AR_E_CAPACITY;                                             // :1039
    }
    if (end > p) {
        pc->in_pos = p; pc->in_size = end - p;
        if (flags & AR_X_CAT) {
            if (dec > end - p) return AR_E_TRUNCATED;                                    // :1055
            pc->kind = AR_K_CAT;
        } else if (flags & AR_X_EXT) return AR_E_UNSUPPORTED;                            // bzip2: a reference built without it
        else pc->kind = (uint8_t)(((flags & AR_X_RLE) ? AR_K_O0_RLE : AR_K_O0) + ((flags & 3) == 1));
    } else dec = 0;                                                                      // :1086
    pc->dec_size = dec;
    if (pc->nsym == AR_NOT_PACKED || pc->nsym == 1) pc->out_size = dec;                  // :1093, :1101
    else {
        // hts_unpack's own test (pack.c:239, :273, :315); no values per byte: the size alone
        if (pc->nsym && (osz + pc->nsym - 1) / pc->nsym > dec) return AR_E_SIZE;
        pc->out_size = osz;
    }
    return AR_OK;
}

// The whole stream of `size` bytes.  SINK: put(j, piece) takes piece j (plane j of a stripe block, piece 0 otherwise).
// max_planes / max_stripe_out: what the caller reserved for stripe blocks (0 planes: none are taken).
template <class SRC, class SINK>
AR_HD inline int ar_parse(SRC &in, uint32_t size, uint32_t cap, uint32_t max_planes, uint32_t max_stripe_out, ArTop *top, SINK &sink)
{
    top->flags = top->out_size = top->nplanes = 0;
    if (size == 0) return AR_E_EMPTY;                                                    // :876
    top->flags = in.at(0);
    ArPiece pc;
    if (!(top->flags & AR_X_STRIPE)) {
        const int st = ar_parse_piece(in, 0, size, cap, &pc);
        if (st != AR_OK) return st;
        top->out_size = pc.out_size;
        sink.put(0, pc);
        return AR_OK;
    }
    uint32_t ulen = 0;
    uint32_t meta = 1 + ar_var_get(in, 1, size, &ulen);                                  // :885
    if (meta >= size) return AR_E_TRUNCATED;
    const uint32_t N = in.at(meta++);
    if (cap == AR_NO_CAP) { if (ulen >= AR_INT_MAX) return AR_E_SIZE; }                   // :891
    else if (ulen != cap) return AR_E_CAPACITY;                                          // :898
    if (N > max_planes || ulen > max_stripe_out) return AR_E_UNSUPPORTED;
    if (N == 0 && ulen) return AR_E_SIZE;
    uint64_t tot = 0;
    const uint32_t lens = meta;
    for (uint32_t i = 0; i < N; i++) {                                                   // :903-912
        uint32_t c = 0;
        meta += ar_var_get(in, meta, size, &c);
        tot += c;
        if (c > size) return AR_E_TRUNCATED;
        if (c < 1) return AR_E_SIZE;
    }
    if (meta + tot > size) return AR_E_TRUNCATED;                                        // :917
    const uint32_t end = meta + (uint32_t)tot;                                           // :921: every plane's stream ends here
    uint32_t lp = lens;
    for (uint32_t i = 0; i < N; i++) {
        uint32_t c = 0;
        lp += ar_var_get(in, lp, size, &c);
        const uint32_t want = ulen / N + ((ulen % N) > i);
        if (in.at(meta) & AR_X_STRIPE) return AR_E_UNSUPPORTED;
        const int st = ar_parse_piece(in, meta, end, want, &pc);
        if (st != AR_OK) return st;
        if (pc.out_size != want) return AR_E_SIZE;                                       // :939
        sink.put(i, pc);
        meta += c;
    }
    top->out_size = ulen;
    top->nplanes = N;
    return AR_OK;
}
