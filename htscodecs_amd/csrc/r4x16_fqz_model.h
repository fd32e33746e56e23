// r4x16_fqz_model.h - what fqzcomp_qual's two directions share on the device (r4x16_fqz.hip decodes, r4x16_fqz_enc.hip
// encodes): the homes of a stream's tables, the LDS budget of a coding wave and the size of a model slot.  DESIGN 4.8.
#pragma once
#include "r4x16_arith_model.h"
#include "r4x16_fqz_parse.h"

enum { FQ_HOME_LDS = 0, FQ_HOME_GLOBAL = 1, FQ_HOME_NONE = 2 };
#define FQ_CTX_ROWS 65536u
// LDS of a decode wave: the four `len` models and the `sel` model (256 entries of 4 bytes each), the selector table,
// and up to FQ_LDS_PARAMS parameter blocks' flat tables: 5,120 + 512 + 8 x 3,344 = 32,384 bytes of a 32 KiB share -
// five waves a compute unit, one more than the four slots a compute unit the arena holds at most
#define FQ_LDS_MODELS (5u * 1024u)
#define FQ_LDS_PARAMS 8u
#define FQ_MAX_SLOTS 1024
#define FQ_REV_BIT 0x80000000u

// a slot: 65,536 rows of max_sym + 1 entries padded to four, 4 bytes an entry, and the rows' totals
__host__ __device__ static inline u64 fq_slot_bytes(u32 max_sym) { return (u64)FQ_CTX_ROWS * ar_row_stride(max_sym + 1u) * 4u + FQ_CTX_ROWS * 4u; }
__host__ __device__ static inline u32 fq_tab_bytes(u32 nparam) { return FQ_STAB_BYTES + nparam * FQ_PARAM_BYTES; }

// the walk's taker on the device: a block's flat tables at `tab`, written by the lanes with `on`
struct FqDevSink {
    u8 *tab; bool on;
    __device__ void stab(u32 i, u32 v) { if (on) ((u16 *)tab)[i] = (u16)v; }
    __device__ void param(u32 k, const FqParam &pm) { if (on) *(FqParam *)(tab + FQ_STAB_BYTES + k * FQ_PARAM_BYTES) = pm; }
    __device__ void qmap(u32 k, u32 i, u32 v) { if (on) tab[FQ_STAB_BYTES + k * FQ_PARAM_BYTES + FQ_OFF_QMAP + i] = (u8)v; }
    __device__ void qtab(u32 k, u32 i, u32 v) { if (on) ((u16 *)(tab + FQ_STAB_BYTES + k * FQ_PARAM_BYTES + FQ_OFF_QTAB))[i] = (u16)v; }
    __device__ void ptab(u32 k, u32 i, u32 v) { if (on) ((u16 *)(tab + FQ_STAB_BYTES + k * FQ_PARAM_BYTES + FQ_OFF_PTAB))[i] = (u16)v; }
    __device__ void dtab(u32 k, u32 i, u32 v) { if (on) ((u16 *)(tab + FQ_STAB_BYTES + k * FQ_PARAM_BYTES + FQ_OFF_DTAB))[i] = (u16)v; }
};
