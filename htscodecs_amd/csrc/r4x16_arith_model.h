// r4x16_arith_model.h - what the adaptive coders share on the device, whichever way they code (r4x16_arith.hip decodes
// arith_dynamic, r4x16_arith_enc.hip encodes it, r4x16_fqz.hip decodes fqzcomp_qual, r4x16_fqz_enc.hip encodes it): the
// constants of c_simple_model.h and c_range_coder.h, a model's entries (frequency | symbol << 16), the homes of
// arith_dynamic's models, the input window in registers and the word-wise byte writer.  The steps on top of this:
// r4x16_arith_step.h (decoding), r4x16_arith_enc_step.h (encoding).
// The update behind a coded symbol and a step's row traffic are NOT here: each symbol step keeps its own statements,
// because as shared functions they changed the code of the hot kernels (profiles/adaptive_refactor.md).
#pragma once
#include "r4x16_dev.h"

#define AR_MAX_FREQ 65519u                       // c_simple_model.h MAX_FREQ
#define AR_STEP 16u
#define AR_TOP (1u << 24)
#define AR_NRUN 258
#define AR_LDS_BUDGET 32768u                     // order-1 wave: run models + rows + totals
#define AR_RUN_BYTES (AR_NRUN * 16u)
#define AR_ROWS_BYTES (AR_LDS_BUDGET - AR_RUN_BYTES)
#define AR_GLOBAL_ROW_BYTES (256u * 256u * 4u + 256u * 4u)
#define AR_GLOBAL_SLOTS 1024                     // waves of the global home in flight at most: four a compute unit

__host__ __device__ static inline u32 ar_r16(u32 v) { return (v + 15u) & ~15u; }
__host__ __device__ static inline u32 ar_row_stride(u32 m) { return (m + 3u) & ~3u; }
// the home of an order-1 stream's rows: LDS where m rows and their totals fit the budget, else a slot of the arena
__host__ __device__ static inline bool ar_lds_home(u32 m) { return m * ar_row_stride(m) * 4u + m * 4u <= AR_ROWS_BYTES; }

// a value one lane holds, in scalar registers
__device__ __forceinline__ u64 wave_uniform(u64 v)
{
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

// ---- entries ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 ar_get(const u32x4 &e, u32 k) { return k == 0 ? e.x : k == 1 ? e.y : k == 2 ? e.z : e.w; }
__device__ __forceinline__ void ar_set(u32x4 &e, u32 k, u32 v, bool on)
{
    e.x = on && k == 0 ? v : e.x; e.y = on && k == 1 ? v : e.y; e.z = on && k == 2 ? v : e.z; e.w = on && k == 3 ? v : e.w;
}
__device__ __forceinline__ u32 ar_half(u32 e) { const u32 f = e & 0xffffu; return (e & 0xffff0000u) | (f - (f >> 1)); }
// list positions p .. p + 3 of a model of m symbols after SIMPLE_MODEL_init: every symbol once, zero behind them
__device__ __forceinline__ u32x4 ar_fresh(u32 p, u32 m)
{
    u32x4 v;
    v.x = p < m ? 1u | (p << 16) : 0u; v.y = p + 1 < m ? 1u | ((p + 1) << 16) : 0u;
    v.z = p + 2 < m ? 1u | ((p + 2) << 16) : 0u; v.w = p + 3 < m ? 1u | ((p + 3) << 16) : 0u;
    return v;
}

// ---- homes of arith_dynamic's models, either direction --------------------------------------------------------
// The order-0 model lives in registers (ar_fresh(4 * lane, m)), the 258 run-length models at the start of the wave's
// LDS, an order-1 stream's rows behind them or in the workgroup's slot of the arena (ar_lds_home).  Rows of `stride`
// entries, their totals behind the last row.  (fqzcomp_qual's slots are its own: r4x16_fqz.hip.)
struct ArHome { u32 *rows, *tots; };
__device__ __forceinline__ ArHome ar_home(bool in_lds, u32 *lds, u8 *slots, u32 m, u32 stride)
{
    u32 *rows = in_lds ? lds + AR_RUN_BYTES / 4 : (u32 *)(slots + (size_t)blockIdx.x * AR_GLOBAL_ROW_BYTES);
    return ArHome{rows, rows + (in_lds ? m * stride : 256u * 256u)};
}
__device__ __forceinline__ void ar_runs_init(u32 *lds, u32 lane)
{
    for (u32 k = lane; k < AR_NRUN * 4u; k += WAVE) lds[k] = 1u | ((k & 3u) << 16);
}

// ---- bytes in, bytes out ----------------------------------------------------------------------------------------
// The input: a window of 1 KB held in registers, 16 bytes a lane, read by a scalar lane read (WinSrc's scheme,
// r4x16_dev.h), so that a byte-wise reader never waits for memory; the last bytes, which fill no whole 16-byte piece,
// are read from memory.  (Not WinSrc itself: it points at a ByteSrc, and the two as members of one object - the pointer
// to a sibling member - put the whole coder into scratch memory, 112 bytes a lane.  This holds no pointer to a member.)
struct ArWindow {
    const u8 *base;
    u32x4 held;
    u32 wbase, wlen, end;
    __device__ ArWindow(const u8 *in, u32 n) : base(in), held{0, 0, 0, 0}, wbase(0), wlen(0), end(n) {}
    __device__ __forceinline__ void fill(u32 p, u32 lane)
    {
        wbase = p & ~15u;
        const u32 mine = wbase + 16u * lane;
        held = u32x4{0, 0, 0, 0};
        if (mine + 16u <= end) held = *(const u32x4_unaligned *)(base + mine);
        const u32 room = (end - wbase) & ~15u;
        wlen = room < 1024u ? room : 1024u;
    }
    __device__ __forceinline__ u32 byte(u32 p, u32 lane)           // p < end
    {
        if (p - wbase >= wlen) {
            if (p + 16u > end) return base[p];
            fill(p, lane);
        }
        const u32 so = (u32)__builtin_amdgcn_readfirstlane((int)(p - wbase));
        const int ln = (int)(so >> 4);
        const u32 d0 = (u32)__builtin_amdgcn_readlane((int)held.x, ln), d1 = (u32)__builtin_amdgcn_readlane((int)held.y, ln),
                  d2 = (u32)__builtin_amdgcn_readlane((int)held.z, ln), d3 = (u32)__builtin_amdgcn_readlane((int)held.w, ln);
        const u32 lo = (so & 4u) ? d1 : d0, hi = (so & 4u) ? d3 : d2;
        return (((so & 8u) ? hi : lo) >> (8u * (so & 3u))) & 0xffu;
    }
};

// The output, four bytes at a time: n bytes so far, the last n & 3 of them in acc.  The stage slots are 16-byte aligned
// and hold their size rounded up to 16.  Wave-uniform; lane 0 stores.
struct ArBytes {
    u32 *dst; u32 acc, n;
    __device__ __forceinline__ void put(u32 b, u32 lane)
    {
        acc |= b << (8u * (n & 3u));
        if ((++n & 3u) == 0) { if (lane == 0) dst[(n >> 2) - 1] = acc; acc = 0; }
    }
    __device__ __forceinline__ void flush(u32 lane) { if ((n & 3u) && lane == 0) dst[n >> 2] = acc; }
};
