// Issue cost of v_lshrrev_b64 against v_lshrrev_b32 (and of a quad_perm DPP move) in a lone wave's dependent stream: does
// the 64-bit shift of the encode chain's packed-row step take two issue slots?  (profiles/enc_quad.md)
// build: hipcc --offload-arch=gfx950 -O3 -o tools/micro/valu_shift64_rate.bin tools/micro/valu_shift64_rate.hip (git-ignored)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define ITERS 16384
#define R8(x) x x x x x x x x
#define R64(x) R8(R8(x))
// mode 0: 32-bit shifts, each reading the one before; 1: 64-bit shifts, each reading the one before; 2: 32-bit shifts of
// four independent registers in turn; 3: 64-bit shifts of four independent pairs in turn; 4: DPP moves, each reading the
// one before behind two independent 32-bit shifts (the hazard's distance); 5: those two shifts and a plain move
__global__ __launch_bounds__(256) void k(uint32_t *out, unsigned long long *cyc, int mode, uint32_t sh)
{
    const uint32_t tid = threadIdx.x;
    uint32_t a = tid * 2654435761u | 1u, b = ~a, c = a ^ 0x5555u, d = b ^ 0x3333u;
    uint64_t p = ((uint64_t)a << 32) | b, q = ~p, r = p ^ 0x0f0f0f0full, s = q ^ 0x00ff00ffull;
    const unsigned long long t0 = wall_clock64();
    const unsigned long long c0 = clock64();
    for (int i = 0; i < ITERS / 64; i++) {
        switch (mode) {
        case 0: asm volatile(R64("v_lshrrev_b32_e32 %0, %1, %0\n\t") : "+v"(a) : "v"(sh)); break;
        case 1: asm volatile(R64("v_lshrrev_b64 %0, %1, %0\n\t") : "+v"(p) : "v"(sh)); break;
        case 2: asm volatile(R64("v_lshrrev_b32_e32 %0, %4, %0\n\tv_lshrrev_b32_e32 %1, %4, %1\n\tv_lshrrev_b32_e32 %2, %4, %2\n\tv_lshrrev_b32_e32 %3, %4, %3\n\t")
                             : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(sh)); break;
        case 3: asm volatile(R64("v_lshrrev_b64 %0, %4, %0\n\tv_lshrrev_b64 %1, %4, %1\n\tv_lshrrev_b64 %2, %4, %2\n\tv_lshrrev_b64 %3, %4, %3\n\t")
                             : "+v"(p), "+v"(q), "+v"(r), "+v"(s) : "v"(sh)); break;
        case 4: asm volatile(R64("v_mov_b32_dpp %0, %0 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\tv_lshrrev_b32_e32 %1, %3, %1\n\tv_lshrrev_b32_e32 %2, %3, %2\n\t")
                             : "+v"(a), "+v"(b), "+v"(c) : "v"(sh)); break;
        default: asm volatile(R64("v_mov_b32_e32 %0, %0\n\tv_lshrrev_b32_e32 %1, %3, %1\n\tv_lshrrev_b32_e32 %2, %3, %2\n\t")
                             : "+v"(a), "+v"(b), "+v"(c) : "v"(sh)); break;
        }
    }
    const unsigned long long c1 = clock64();
    const unsigned long long t1 = wall_clock64();
    if (tid == 0) { cyc[0] = c1 - c0; cyc[1] = t1 - t0; }
    out[blockIdx.x * blockDim.x + tid] = a + b + c + d + (uint32_t)(p + q + r + s) + (uint32_t)((p + q + r + s) >> 32);
}
int main()
{
    uint32_t *out; unsigned long long *cyc, h[2];
    if (hipMalloc(&out, 1 << 20) != hipSuccess || hipMalloc(&cyc, 64) != hipSuccess) { printf("no device memory\n"); return 1; }
    const char *names[] = {"v_lshrrev_b32, dependent", "v_lshrrev_b64, dependent", "v_lshrrev_b32, four independent", "v_lshrrev_b64, four independent",
                           "v_mov_b32_dpp + two b32 shifts", "v_mov_b32 + two b32 shifts"};
    const int per[] = {1, 1, 4, 4, 3, 3};
    for (int waves = 1; waves <= 4; waves *= 2)
        for (int mode = 0; mode < 6; mode++) {
            hipLaunchKernelGGL(k, dim3(1), dim3(64 * waves), 0, 0, out, cyc, mode, 0u);
            hipLaunchKernelGGL(k, dim3(1), dim3(64 * waves), 0, 0, out, cyc, mode, 0u);
            if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
            if (hipMemcpy(h, cyc, 16, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
            printf("waves %d  %-34s %7.3f ns per instruction (%d instructions, %.0f ns; %llu counter ticks)\n", waves, names[mode],
                   (double)h[1] * 10.0 / (ITERS * per[mode]), ITERS * per[mode], (double)h[1] * 10.0, h[0]);
        }
    return 0;
}
