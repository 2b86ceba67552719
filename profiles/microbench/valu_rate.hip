// Issue rate of the integer, address and transcendental vector instructions k_describe uses, on gfx950
// (cycles per wave64 instruction per SIMD), v_fma_f32 as the yardstick.
//   hipcc --offload-arch=gfx950 -O3 -o valu_rate valu_rate.hip && ./valu_rate
// 8 independent chains per lane, W waves per SIMD (as f64_rate.hip).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CHK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("err %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} }while(0)

// OP: 0 v_fma_f32, 1 v_mul_lo_u32, 2 v_mad_u64_u32, 3 v_mul_u32_u24, 4 v_mad_i32_i24, 5 v_lshl_add_u64,
//     6 v_rcp_f32, 7 v_sqrt_f32, 8 v_cvt_f32_i32
template <int OP>
__global__ __launch_bounds__(256) void k(double *out, int iters, int seed)
{
    uint32_t a[8];
    uint64_t w[8];
    float f[8];
    for (int i = 0; i < 8; i++) {
        a[i] = (uint32_t)(seed + i + threadIdx.x);
        w[i] = a[i];
        f[i] = 1.0f + 0.001f * (float)a[i];
    }
    const uint32_t m = 3u + seed;
    const float fm = 1.0000001f, fc = 1e-9f;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (OP == 0) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[i]) : "v"(fm), "v"(fc));
                if (OP == 1) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                if (OP == 2) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(w[i]) : "v"(a[i]), "v"(m) : "vcc");
                if (OP == 3) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a[i]) : "v"(m));
                if (OP == 4) asm volatile("v_mad_i32_i24 %0, %0, %1, %0" : "+v"(a[i]) : "v"(m));
                if (OP == 5) asm volatile("v_lshl_add_u64 %0, %1, 2, %0" : "+v"(w[i]) : "v"(w[(i + 1) & 7]));
                if (OP == 6) asm volatile("v_rcp_f32 %0, %0" : "+v"(f[i]));
                if (OP == 7) asm volatile("v_sqrt_f32 %0, %0" : "+v"(f[i]));
                if (OP == 8) asm volatile("v_cvt_f32_i32 %0, %1" : "=v"(f[i]) : "v"(a[i]));
            }
        }
    }
    double s = 0;
    for (int i = 0; i < 8; i++) s += (double)a[i] + (double)w[i] + f[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int OP> void run(const char *name, double *d_o)
{
    for (int bpc = 1; bpc <= 8; bpc *= 2) {            // blocks of 4 waves per CU: 1, 2, 4, 8 waves per SIMD
        const int iters = 4000;
        hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
        float ms = 0;
        for (int rep = 0; rep < 2; rep++) {
            CHK(hipEventRecord(e0));
            hipLaunchKernelGGL((k<OP>), dim3(256 * bpc), dim3(256), 0, 0, d_o, iters, 1);
            CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
            CHK(hipEventElapsedTime(&ms, e0, e1));
        }
        const double instr_per_simd = (double)bpc * iters * 32;
        printf("%-16s %d waves/SIMD: %8.3f ms -> %6.2f cycles / instruction / SIMD (2.4 GHz)\n", name, bpc, ms,
               ms * 1e-3 * 2.4e9 / instr_per_simd);
    }
}

int main()
{
    double *d_o; CHK(hipMalloc(&d_o, 256 * 8 * 256 * 8));
    run<0>("v_fma_f32", d_o);
    run<1>("v_mul_lo_u32", d_o);
    run<2>("v_mad_u64_u32", d_o);
    run<3>("v_mul_u32_u24", d_o);
    run<4>("v_mad_i32_i24", d_o);
    run<5>("v_lshl_add_u64", d_o);
    run<6>("v_rcp_f32", d_o);
    run<7>("v_sqrt_f32", d_o);
    run<8>("v_cvt_f32_i32", d_o);
    return 0;
}
