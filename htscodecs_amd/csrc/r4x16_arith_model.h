// r4x16_arith_model.h - what the two directions of the adaptive arithmetic codec share on the device (r4x16_arith.hip
// decodes, r4x16_arith_enc.hip encodes): the constants of c_simple_model.h and c_range_coder.h, the budget of the LDS home
// of the order-1 rows, and the accessors of a model's four list positions a lane.  An entry is frequency | symbol << 16.
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

__host__ __device__ static inline u32 ar_row_stride(u32 m) { return (m + 3u) & ~3u; }

__device__ __forceinline__ u32 ar_get(const u32x4 &e, u32 k) { return k == 0 ? e.x : k == 1 ? e.y : k == 2 ? e.z : e.w; }
__device__ __forceinline__ void ar_set(u32x4 &e, u32 k, u32 v, bool on)
{
    e.x = on && k == 0 ? v : e.x; e.y = on && k == 1 ? v : e.y; e.z = on && k == 2 ? v : e.z; e.w = on && k == 3 ? v : e.w;
}
__device__ __forceinline__ u32 ar_half(u32 e) { const u32 f = e & 0xffffu; return (e & 0xffff0000u) | (f - (f >> 1)); }
