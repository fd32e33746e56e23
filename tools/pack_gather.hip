// pack_gather.hip - the host-batch pipeline's gather kernel (k_pack_results, htscodecs_amd/csrc/r4x16_pack.h) behind one
// C entry point, so that tools/packed_dev_rate.py can time "slot call, then gather" on device-resident blocks:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared tools/pack_gather.hip -o tools/probe/libpack_gather.so
// desc: device array of n {u64 src, u64 dst, u32 len, u32 pad}; block i is copied from slots + src to dense + dst.
#include <hip/hip_runtime.h>
#include "../htscodecs_amd/csrc/r4x16_common.h"
#include "../htscodecs_amd/csrc/r4x16_pack.h"

extern "C" __attribute__((visibility("default")))
int pack_gather(const unsigned char *slots, unsigned char *dense, const void *desc, int n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_pack_results, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const u8 *)slots, (u8 *)dense,
                       (const PackDesc *)desc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
