// r4x16_tok3_walk.h - the walk over one tok3 column container (htscodecs tokenise_name3.c:1546-1669, decode_names up to
// the point where the columns are handed to the per-name decoder), written once for the host scan
// (rans4x16_hip_tok3_scan, r4x16_tok3_scan.hip) and the device walk (k_t3_walk, r4x16_tok3.hip): what one reports the
// other reports, because it is the same text.  Nothing here needs HIP: the scan's unit compiles with a plain C++ compiler.
//
// A container: last_start (4 bytes, little endian), nreads (4), use_arith (1), then descriptors until the end:
//   type byte t : t & 15 the token type, t & 128 "first column of the next token position", t & 64 duplicate
//   duplicate   : two bytes j >> 4, j & 15 - the id of an earlier column whose bytes this one repeats
//   plain       : var_put_u32(clen), then a stream of clen bytes - rANS 4x16, or arith_dynamic where use_arith is set;
//                 flag byte and stored size lie at the same places in both, so the walk is one
// A column's id is tnum << 4 | type.  A position opened by a column whose type is not 0 gets its type column (id
// tnum << 4) synthesised first: nreads bytes, the type and then N_MATCH repeated (:1581-1591, :1619-1629).
//
// Loops: the descriptor loop runs max_columns trips (an argument, never a value from the container); a varint is read
// inside [pos, end) with end <= size, and size is checked against the call's max_in_size before the walk starts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define T3_HD __host__ __device__
#else
#define T3_HD
#endif

#define T3_MAX_TOKENS 128       // tokenise_name3.c MAX_TOKENS
#define T3_MAX_IDS 2048         // MAX_TOKENS << 4: ids are strictly ascending, so also the most columns of one container
#define T3_N_MATCH 10           // enum name_type N_MATCH
#define T3_HEADER 9
#define T3_NONE 0xffffu         // map[] entry of an id that has no column

enum { T3_PLAIN = 0, T3_DUP = 1, T3_SYNTH = 2 };
// the status codes of include/rans4x16_hip.h the walk gives
enum { T3_OK = 0, T3_E_TRUNCATED = 2, T3_E_SIZE = 5, T3_E_UNSUPPORTED = 6, T3_E_EMPTY = 9 };

struct T3Sum {
    uint32_t last_start, nreads;   // header
    uint32_t ndesc, ncol;          // descriptors accepted; columns they give (descriptors + synthesised type columns)
    uint64_t total;                // bytes of all columns
    uint32_t max_col, max_stream;  // largest column, largest stream (clen)
    uint32_t arith;                // the block's flavour: byte 8 (use_arith) is set - its streams are arith_dynamic's
};

// varint.h:131-160 over [pos, end); returns the bytes consumed, 0 if there is none; *cont: the last byte read still had
// its continuation bit (the value ran into `end`)
template <class SRC>
T3_HD inline uint32_t t3_var_get(SRC &s, uint32_t pos, uint32_t end, uint32_t *v, bool *cont)
{
    uint32_t acc = 0, p = pos;
    uint8_t c = 0;
    *v = 0; *cont = false;
    if (pos >= end) return 0;
    do {
        c = s.at(p++);
        acc = (acc << 7) | (c & 0x7fu);
    } while ((c & 0x80) && p < end);
    *v = acc;
    *cont = (c & 0x80) != 0;
    return p - pos;
}

#define T3_LEAD 0x8000u         // map[] entry: the type column synthesised in front of descriptor (entry & 0x7fff)

// SRC: at(pos) -> byte pos of the container.  DIR: the directory being built, one entry per descriptor -
// put(d, id, kind, a, b, size, lead) records descriptor d: its column (PLAIN: a = where its stream starts in the
// container, b = clen; DUP: a = the descriptor whose PLAIN column it copies, T3_NONE for none; SYNTH: a copy of a type
// column, a = the type) and `lead`, the bytes of the type column synthesised in front of it (0: none; its type is
// id & 15) - and kind_at / a_at / size_at / id_at read back what was put.  map: T3_MAX_IDS entries, all T3_NONE on entry;
// id -> descriptor.  max_columns bounds the descriptors.  admit_arith: a container with use_arith set is walked (by the
// same rules) and sum->arith says so; without it such a container is refused.  Returns 0 or the status of the first
// descriptor that is refused; *sum is what was accepted up to there.
template <class SRC, class DIR>
T3_HD inline int t3_walk(SRC &in, uint32_t size, uint32_t max_columns, uint32_t max_col_size, bool admit_arith, uint16_t *map, DIR &dir,
                         T3Sum *sum)
{
    sum->last_start = sum->nreads = sum->ndesc = sum->ncol = sum->max_col = sum->max_stream = sum->arith = 0;
    sum->total = 0;
    if (size < T3_HEADER) return T3_E_TRUNCATED;                                         // :1547
    const uint32_t last_start = (uint32_t)in.at(0) | ((uint32_t)in.at(1) << 8) | ((uint32_t)in.at(2) << 16) | ((uint32_t)in.at(3) << 24);
    const uint32_t nreads = (uint32_t)in.at(4) | ((uint32_t)in.at(5) << 8) | ((uint32_t)in.at(6) << 16) | ((uint32_t)in.at(7) << 24);
    sum->last_start = last_start; sum->nreads = nreads;
    if (in.at(8) != 0) {                                                                 // use_arith
        if (!admit_arith) return T3_E_UNSUPPORTED;
        sum->arith = 1;
    }
    if (last_start >= 0x7fffffffu - 1024u) return T3_E_SIZE;                             // :1555 (negative as an int, or too large)
    uint32_t o = T3_HEADER;
    int tnum = -1, last_id = -1;
    for (uint32_t d = 0; d < max_columns && o < size; d++) {
        const uint32_t t = in.at(o++);
        uint32_t j = 0, lead = 0;
        if (t & 64) {
            if (o + 2 >= size) return T3_E_TRUNCATED;                                    // :1570 (refuses a duplicate at the very end)
            j = ((uint32_t)in.at(o) << 4) + in.at(o + 1);
            o += 2;
        }
        if (t & 128) {
            if (++tnum >= T3_MAX_TOKENS) return T3_E_SIZE;                               // :1575, :1613
            if (t & 15) {                                                                // :1581, :1619: the position's type column
                if (nreads == 0) return T3_E_SIZE;
                if (nreads > max_col_size) return T3_E_UNSUPPORTED;
                lead = nreads;
                map[tnum << 4] = (uint16_t)(T3_LEAD | d);
                last_id = tnum << 4;
            }
        }
        if (tnum < 0) return T3_E_SIZE;                                                  // :1593, :1637
        const int id = (tnum << 4) | (int)(t & 15);
        if ((t & 64) && j >= (uint32_t)id) return T3_E_SIZE;                             // :1595
        if (id <= last_id) return T3_E_UNSUPPORTED;                                      // stricter: ids strictly ascend
        uint32_t csize = 0;
        if (t & 64) {
            const uint32_t from = map[j];
            if (from != T3_NONE && (from & T3_LEAD)) {                                   // a copy of a type column is written like one
                const uint32_t fd = from & ~T3_LEAD;
                csize = nreads;
                dir.put(d, id, T3_SYNTH, fd == d ? (t & 15) : ((uint32_t)dir.id_at(fd) & 15u), 0, csize, lead);
            } else if (from == T3_NONE || dir.size_at(from) == 0) dir.put(d, id, T3_DUP, T3_NONE, 0, 0, lead);   // :1599: buf_a of a column never set is 0
            else {
                csize = dir.size_at(from);
                // a copy of a copy reads the original
                if (dir.kind_at(from) == T3_PLAIN) dir.put(d, id, T3_DUP, from, 0, csize, lead);
                else dir.put(d, id, dir.kind_at(from), dir.a_at(from), 0, csize, lead);
            }
        } else {
            uint32_t clen = 0, claim = 0;
            bool cont = false;
            const uint32_t nb = t3_var_get(in, o, size, &clen, &cont);                   // :1306
            if (nb == 0 || cont) return T3_E_TRUNCATED;
            const uint32_t so = o + nb;
            if (clen > size - so) return T3_E_TRUNCATED;                                 // stricter: the stream lies inside the container
            if (clen == 0) return T3_E_EMPTY;                                            // what peek says of such a stream
            const uint32_t flags = in.at(so);
            if (!(flags & 0x08) && (flags & 0x10)) return T3_E_SIZE;                     // stricter: X_NOSZ, the stream carries no size
            const uint32_t ub = t3_var_get(in, so + 1, so + clen, &claim, &cont);        // :1309, inside the stream
            if (ub == 0 || cont) return T3_E_TRUNCATED;
            if (claim > max_col_size) return T3_E_UNSUPPORTED;
            dir.put(d, id, T3_PLAIN, so, clen, claim, lead);
            if (clen > sum->max_stream) sum->max_stream = clen;
            csize = claim;
            o = so + clen;                                                               // :1660
        }
        map[id] = (uint16_t)d;
        last_id = id;
        sum->ndesc = d + 1;
        sum->ncol += lead ? 2u : 1u;
        sum->total += (uint64_t)lead + csize;
        if (lead > sum->max_col) sum->max_col = lead;
        if (csize > sum->max_col) sum->max_col = csize;
    }
    if (o < size) return T3_E_UNSUPPORTED;                                               // more descriptors than max_columns
    if (sum->total > 0xffffffffull) return T3_E_UNSUPPORTED;                             // a block's size is reported in 32 bits
    return T3_OK;
}
