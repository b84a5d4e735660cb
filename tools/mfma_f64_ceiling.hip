// fp64 MFMA issue ceiling on MI355X for tom_tile_kernel / corr_tile_kernel / syrk_f64_kernel:
// v_mfma_f64_16x16x4_f64 back to back from registers (no loads, no LDS), four independent
// accumulators per wave as those kernels keep them, 256-thread workgroups at W waves per SIMD.
// Prints one JSON line per W: TFLOP/s (median of the timed launches).
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/mfma_f64_ceiling tools/mfma_f64_ceiling.hip
//   tools/mfma_f64_ceiling [mfma_per_wave=1048576] [reps=5]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHK(x)                                                                   \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));             \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

__global__ __launch_bounds__(256) void mfma_kernel(int64_t iters, double seed,
                                                   double* __restrict__ out) {
  f64x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
  const double a0 = seed * (double)(threadIdx.x & 63), a1 = a0 + 1.0;
  const double b0 = seed * (double)(threadIdx.x & 15), b1 = b0 - 1.0;
  for (int64_t it = 0; it < iters; ++it) {  // 16 MFMAs per trip
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[(int64_t)blockIdx.x * 256 + threadIdx.x] = s;
}

int main(int argc, char** argv) {
  const int64_t per_wave = argc > 1 ? atoll(argv[1]) : (int64_t)1 << 20;
  const int reps = argc > 2 ? atoi(argv[2]) : 5;
  hipDeviceProp_t prop;
  CHK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0));
  CHK(hipEventCreate(&e1));
  for (int w = 1; w <= 4; ++w) {  // waves per SIMD: one 4-wave workgroup per CU each
    const int blocks = cus * w;
    double* out = nullptr;
    CHK(hipMalloc(&out, sizeof(double) * blocks * 256));
    const int64_t iters = per_wave / 16;
    hipLaunchKernelGGL(mfma_kernel, dim3(blocks), dim3(256), 0, 0, iters, 1e-9, out);  // warm-up
    CHK(hipDeviceSynchronize());
    std::vector<float> ms(reps);
    for (int r = 0; r < reps; ++r) {
      CHK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(mfma_kernel, dim3(blocks), dim3(256), 0, 0, iters, 1e-9, out);
      CHK(hipEventRecord(e1, 0));
      CHK(hipEventSynchronize(e1));
      CHK(hipEventElapsedTime(&ms[r], e0, e1));
    }
    std::sort(ms.begin(), ms.end());
    const double flop = 2048.0 * 16.0 * (double)iters * 4.0 * blocks;
    printf("{\"waves_per_simd\": %d, \"cus\": %d, \"mfma_per_wave\": %lld, \"median_ms\": %.3f, "
           "\"TFLOP_per_s\": %.2f}\n", w, cus, (long long)(iters * 16), ms[reps / 2],
           flop / ms[reps / 2] / 1e9);
    fflush(stdout);
    CHK(hipFree(out));
  }
  return 0;
}
