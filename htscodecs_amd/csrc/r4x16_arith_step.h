// r4x16_arith_step.h - the decoding step the adaptive coders share on the device: the carry-less range coder of
// c_range_coder.h on the input window in registers, and one symbol of a SIMPLE_MODEL whose list lies across the wave
// (c_simple_model.h).  r4x16_arith.hip (arith_dynamic) and r4x16_fqz.hip (fqzcomp_qual) decode with it; the window
// is r4x16_arith_model.h's, which the encoder reads its input through as well.
#pragma once
#include "r4x16_arith_model.h"

// ---- the step ---------------------------------------------------------------------------------------------------
struct ArCoder {
    u32 code, range, pos;           // wave-uniform
    ArWindow in;                    // the input in registers (r4x16_arith_model.h): held by value, never pointed at
    __device__ ArCoder(const u8 *src, u32 in_size, u32 lane) : code(0), range(0xffffffffu), pos(1), in(src, in_size)
    {
        if (pos + 5 >= in.end) pos = in.end;                        // c_range_coder.h:64-67: nothing is read, code stays 0
        else for (int k = 0; k < 5; k++) code = (code << 8) | in.byte(pos++, lane);
    }
    // RC_GetFreq: the guard included (c_range_coder.h:112-115)
    __device__ __forceinline__ u32 get_freq(u32 tot)
    {
        if (tot == 0 || range < tot) return 0;
        range /= tot;
        return code / range;
    }
    // RC_Decode (:117-127): stops renormalising where the input ends
    __device__ __forceinline__ void decode(u32 cum, u32 f, u32 lane)
    {
        code -= cum * range;
        range *= f;
        while (range < AR_TOP) {
            if (pos >= in.end) return;
            code = (code << 8) + in.byte(pos++, lane);
            range <<= 8;
        }
    }
};

// One symbol of a model that lies across the wave (SIMPLE_MODEL(256,_decodeSymbol), c_simple_model.h:148-179).  e: this
// lane's four entries, zero beyond the live ones; tot: their sum over the wave.  *dirty: this lane's entries changed.
__device__ __forceinline__ u32 ar_symbol(u32x4 &e, u32 &tot, ArCoder &rc, u32 lane, bool *dirty)
{
    *dirty = false;
    const u32 freq = rc.get_freq(tot);
    if (freq > AR_MAX_FREQ) return 0;                               // :153: no update, no RC_Decode
    const u32 c0 = e.x & 0xffffu, c1 = c0 + (e.y & 0xffffu), c2 = c1 + (e.z & 0xffffu), c3 = c2 + (e.w & 0xffffu);
    const u32 incl = wave_incl_scan(c3, lane);
    const u64 hit = __ballot(incl > freq);
    if (hit == 0) return 0;                                         // :158: the scan ran off the list (freq >= tot)
    const int L = (int)__builtin_ctzll(hit);
    const u32 excl = incl - c3;
    const u32 j_l = (u32)(excl + c0 <= freq) + (u32)(excl + c1 <= freq) + (u32)(excl + c2 <= freq);
    const u32 cum_l = excl + (j_l == 0 ? 0u : j_l == 1 ? c0 : j_l == 2 ? c1 : c2);
    const u32 j = (u32)__builtin_amdgcn_readlane((int)j_l, L);
    const u32 cum = (u32)__builtin_amdgcn_readlane((int)cum_l, L);
    const u32 ent = (u32)__builtin_amdgcn_readlane((int)ar_get(e, j_l), L);
    rc.decode(cum, ent & 0xffffu, lane);
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
    return ent >> 16;
}
