// r4x16_best_qual.h - the method list of the best-of calls across codecs (r4x16_best_qual.hip, include/rans4x16_hip.h parts
// 2m and 2n) split by codec, and what of it a call refuses before it asks for the device.  Plain host C++ without a HIP
// header, so that the refusals are checked by a program of their own where there is no device
// (tests/host/best_qual_check.cpp).
#pragma once
#include <stdint.h>
#include "../../include/rans4x16_hip.h"

#define BQ_MAX_K 32
#define BQ_MAX_FQZ 16                       // part 2l's limit (FQB_MAX_K)
// a codec's side of a block, and as a mask the codec tags a call admits: part 2m's calls BQ_RANS | BQ_ARITH, part 2n's all three
enum { BQ_NONE = 0, BQ_RANS = 1, BQ_ARITH = 2, BQ_FQZ = 4 };
// the side of a codec tag (a method word's bits 24..27), BQ_NONE for a tag of no codec here (constexpr: the kernels' too)
static constexpr int bq_tag_side(int tag)
{
    return tag == R4X16_CODEC_RANS4X16 ? BQ_RANS : tag == R4X16_CODEC_ARITH ? BQ_ARITH : tag == R4X16_CODEC_FQZ ? BQ_FQZ : BQ_NONE;
}
// the caller's list, tags included; fpos[j]: where the fqzcomp sub-list's j-th strategy stands in it
struct BqMethods { int k; int m[BQ_MAX_K]; int fpos[BQ_MAX_FQZ]; };
// the three sub-lists, each in list order, tags off
struct BqSplit { BqMethods pm; int kr, ka, kf; int rm[BQ_MAX_K], am[BQ_MAX_K], sm[BQ_MAX_FQZ]; };

// nullptr and *p filled, or the reason the list is refused.  admit: the BQ_* of the tags the call takes - any other tag is
// unknown to it, and is met before the word's own checks.
static inline const char *bq_split(int k, const int *methods, BqSplit *p, unsigned admit)
{
    *p = BqSplit{};
    if (k < 1 || k > BQ_MAX_K || !methods) return "bad arguments";
    p->pm.k = k;
    for (int j = 0; j < k; j++) {
        const int m = methods[j], tag = m & R4X16_CODEC_MASK, word = m & ~R4X16_CODEC_MASK;
        // a negative word - a negative strategy under the tag is one - and a bit above the tag are no tag of the three
        if (m < 0 || (m >> 28) || !(bq_tag_side(tag) & admit)) return "unknown codec tag";
        // bits 0..15 are all a method carries: the order word's flags and, for a stripe method (bit 3), up to 255 planes
        // (rANS_static4x16pr.c:1158; arith_dynamic.c:648), or the strategy
        if (word >> 16) return tag == R4X16_CODEC_FQZ ? "a strategy above 16 bits" : (word & 8) ? "more than 255 stripes" : "an order word above 16 bits";
        p->pm.m[j] = m;
        if (tag == R4X16_CODEC_FQZ) {
            if (p->kf == BQ_MAX_FQZ) return "more than 16 fqzcomp_qual strategies";
            p->pm.fpos[p->kf] = j;
            p->sm[p->kf++] = word;
        } else if (tag == R4X16_CODEC_ARITH) p->am[p->ka++] = word;
        else p->rm[p->kr++] = word;
    }
    return nullptr;
}
