// r4x16_pack.h - the gather of sparse encode results (r4x16_host.hip's pipeline; tools/pack_gather.hip times it on its own)
#pragma once
#include "r4x16_dev.h"
#include "r4x16_stage.h"                                // PackDesc

// Sparse results (encode: every block owns a bound-sized slot and fills a fraction of it) are gathered by the device
// into the slab's input region, which is dead once the slab's kernels have run, and cross PCIe as a few dense DMAs
// instead of one small DMA per block (15,000 small blocks: 140 ms of DMA calls before).
__global__ __launch_bounds__(256) void k_pack_results(const u8 *out, u8 *in, const PackDesc *d)
{
    const PackDesc p = d[blockIdx.x];
    const u8 *s = out + p.src;                // slots are 256-byte aligned; a packed result may start at any byte
    u8 *t = in + p.dst;
    const u32 n16 = p.len >> 4;
    for (u32 i = threadIdx.x; i < n16; i += 256) ((u32x4_unaligned *)t)[i] = ((const u32x4 *)s)[i];
    for (u32 i = (n16 << 4) + threadIdx.x; i < p.len; i += 256) t[i] = s[i];
}
