// Micro-benchmark: sustained issue rate of v_mfma_f64_16x16x4_f64 on MI355X, whole chip busy -- the yardstick of the
// mapping-confidence kernels (hmx_score.hip), which run on this instruction alone.
//   hipcc --offload-arch=gfx950 -O3 scripts/micro/mfma_f64_rate.hip -o build/mfma_f64_rate && build/mfma_f64_rate
// For each configuration: shader cycles per MFMA (s_memtime of one wave), nanoseconds per MFMA and SIMD (wall clock over
// the launch), the shader clock that follows, and the float64 matrix rate (2 * 16 * 16 * 4 flops per MFMA).
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// NACC independent accumulators; NACC = 1 chains every MFMA on the one before it (the latency)
template <int NACC>
__global__ __launch_bounds__(512, 1) void k(double* out, unsigned long long* cyc, int iters) {
    f64x4 acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double a = threadIdx.x * 1e-3, b = 1.0 + threadIdx.x * 1e-4;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = MFMA64(a, b, acc[i]);
        a += 1e-6;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    double s = 0.0;
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <int NACC>
void run(const char* name, int threads, int wgs, int iters) {
    double* out; unsigned long long* cyc;
    if (hipMalloc(&out, (size_t)wgs * threads * 8) != hipSuccess || hipMalloc(&cyc, 8) != hipSuccess) { printf("hipMalloc failed\n"); return; }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k<NACC>), dim3(wgs), dim3(threads), 0, 0, out, cyc, 10);   // warm-up
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<NACC>), dim3(wgs), dim3(threads), 0, 0, out, cyc, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    unsigned long long c; hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost);
    const double waves_per_simd = threads / 64.0 / 4.0 * (wgs / 256.0);
    const double mfma_per_simd = (double)iters * NACC * waves_per_simd;
    printf("%-44s %5.1f waves/SIMD | %6.1f cycles per MFMA of one wave = %5.1f per SIMD slot | %6.2f ns per MFMA and SIMD | clock %.2f GHz | %.1f TF\n",
           name, waves_per_simd, (double)c / ((double)iters * NACC), (double)c / ((double)iters * NACC) / waves_per_simd,
           ms * 1e6 / mfma_per_simd, (double)c / (ms * 1e6), 256.0 * 4 * mfma_per_simd * 2048 / (ms * 1e-3) / 1e12);
    hipFree(out); hipFree(cyc);
}

int main() {
    const int it = 4000;
    run<1>("1 accumulator (dependent chain), 1 wave/SIMD", 256, 256, it);
    run<2>("2 accumulators, 1 wave/SIMD", 256, 256, it);
    run<10>("10 accumulators, 1 wave/SIMD", 256, 256, it);
    run<10>("10 accumulators, 2 waves/SIMD", 512, 256, it);
    run<2>("2 accumulators, 2 waves/SIMD", 512, 256, it);
    run<10>("10 accumulators, 4 waves/SIMD", 512, 512, it);
    return 0;
}
