// r4x16_arith_enc_step.h - the encoding step of the adaptive coders on the model-across-the-wave layout: the range coder's
// encode side (c_range_coder.h:42-110) and one symbol of a model that lies across the wave (c_simple_model.h:100-135).
// Written once for arith_dynamic's encoder (r4x16_arith_enc.hip) and fqzcomp_qual's (r4x16_fqz_enc.hip), as
// r4x16_arith_step.h is for the two decoders: both compile this text.
#pragma once
#include "r4x16_arith_model.h"

// The range coder (c_range_coder.h:42-110) and its bytes (ArBytes; the alphabet byte is the first of them).  All of it
// wave-uniform.
struct AreCoder {
    u32 low, range, ffnum, carry, cache;
    ArBytes out;
    __device__ AreCoder(u32 *d, u32 first) : low(0), range(0xffffffffu), ffnum(0), carry(0), cache(0), out{d, first, 1u} {}
    // bytes the body has for certain: written, or pending behind the cache byte
    __device__ __forceinline__ u32 sure() const { return out.n + ffnum; }
    __device__ __forceinline__ void shift_low(u32 lane)             // RC_ShiftLow, :71-89
    {
        if (low < 0xff000000u || carry) {
            out.put((cache + carry) & 0xffu, lane);
            for (; ffnum; ffnum--) out.put((carry - 1u) & 0xffu, lane);
            cache = low >> 24;
            carry = 0;
        } else ffnum++;
        low <<= 8;
    }
    __device__ __forceinline__ void encode(u32 cum, u32 f, u32 tot, u32 lane)      // RC_Encode, :97-104
    {
        const u32 old = low;
        range /= tot;
        low += cum * range;
        range *= f;
        carry += low < old;
        while (range < AR_TOP) { range <<= 8; shift_low(lane); }
    }
    __device__ __forceinline__ void finish(u32 lane) { for (int k = 0; k < 5; k++) shift_low(lane); out.flush(lane); }
};

// One symbol of a model that lies across the wave (SIMPLE_MODEL(256,_encodeSymbol), c_simple_model.h:100-135): ar_symbol's
// step with the search turned round - the entry is found by its symbol, its cumulative frequency by the scan.
__device__ __forceinline__ void are_symbol(u32x4 &e, u32 &tot, u32 c, AreCoder &rc, u32 lane, bool *dirty)
{
    *dirty = false;
    // live means frequency != 0: the positions behind the list read as symbol 0
    const bool k0 = (e.x & 0xffffu) && (e.x >> 16) == c, k1 = (e.y & 0xffffu) && (e.y >> 16) == c,
               k2 = (e.z & 0xffffu) && (e.z >> 16) == c, k3 = (e.w & 0xffffu) && (e.w >> 16) == c;
    const u64 hit = __ballot(k0 || k1 || k2 || k3);
    if (hit == 0) return;                                           // (cannot be: c is below the alphabet byte)
    const int L = (int)__builtin_ctzll(hit);
    const u32 j_l = k0 ? 0u : k1 ? 1u : k2 ? 2u : 3u;
    const u32 c0 = e.x & 0xffffu, c1 = c0 + (e.y & 0xffffu), c2 = c1 + (e.z & 0xffffu), c3 = c2 + (e.w & 0xffffu);
    const u32 cum_l = wave_incl_scan(c3, lane) - c3 + (j_l == 0 ? 0u : j_l == 1 ? c0 : j_l == 2 ? c1 : c2);
    const u32 j = (u32)__builtin_amdgcn_readlane((int)j_l, L);
    const u32 cum = (u32)__builtin_amdgcn_readlane((int)cum_l, L);
    const u32 ent = (u32)__builtin_amdgcn_readlane((int)ar_get(e, j_l), L);
    rc.encode(cum, ent & 0xffffu, tot, lane);
    const bool own = lane == (u32)L;
    u32 cur = ent + AR_STEP;                                         // (a frequency is at most the total: no carry into the symbol)
    ar_set(e, j, cur, own);
    tot += AR_STEP;
    bool all = false;
    if (tot > AR_MAX_FREQ) {                                        // normalise: every live entry, the total summed again
        e.x = ar_half(e.x); e.y = ar_half(e.y); e.z = ar_half(e.z); e.w = ar_half(e.w);
        cur = ar_half(cur);
        tot = wave_sum((e.x & 0xffffu) + (e.y & 0xffffu) + (e.z & 0xffffu) + (e.w & 0xffffu));
        all = true;
    }
    // one step of bubble sort: strictly greater than the position before (position 0 has the sentinel before it)
    bool prev_lane = false;
    if (j || L) {
        const u32 prev = j ? (u32)__builtin_amdgcn_readlane((int)ar_get(e, j - 1), L) : (u32)__builtin_amdgcn_readlane((int)e.w, L - 1);
        if ((cur & 0xffffu) > (prev & 0xffffu)) {
            ar_set(e, j, prev, own);
            if (j) ar_set(e, j - 1, cur, own);
            else { ar_set(e, 3, cur, lane + 1 == (u32)L); prev_lane = lane + 1 == (u32)L; }
        }
    }
    *dirty = own || all || prev_lane;
}
