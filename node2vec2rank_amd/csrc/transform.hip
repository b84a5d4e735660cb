// Threshold / top-percent / binarize of a dense layer in place (n2v2r_transform_layer,
// include/n2v2r.h): network_transform (preprocessing_utils.py:116-141) as ingest.transform pins
// it, on a layer that lives only in HBM.  All three kernels stream the layer's nloc x lda fp32
// buffer flat with 16-B loads: a zero is never alive, so the zero padding columns [n, lda) need no
// column test and stay zero.
//
// An entry a (|a| with `absolute`) is ALIVE when a != 0 and a >= lim; the host folds the
// threshold into lim (the smallest fp32 >= threshold, so the fp32 compare decides exactly as the
// reference's fp64 `a < threshold` does; -inf without a threshold).  Its KEY is the order-
// preserving u32 of its fp32 bits: all bits flipped when the sign is set, the top bit set
// otherwise.
//
//   tf_hist_kernel  one pass of the MSD radix select over the alive keys, 8 bits per pass: counts
//     the next digit of every alive key that matches the current prefix.  Bin contention: a
//     correlation layer's keys share a handful of exponents, so the top digit of a whole wave
//     lands in a few bins, and same-address LDS atomics serialise.  Every lane therefore counts
//     into its own copy of the histogram, picked by lane & 31: 32 copies of 256 bins, 32 KB of LDS,
//     laid out [bin][copy] so that a wave-instruction touches each bank from at most two lanes
//     (lane l and l + 32), whatever the keys are.  The copies are summed per bin after the
//     stream (column (c + bin) & 31 first: no bank conflict) and merged into the global u64
//     histogram with one add per non-empty bin per workgroup.  The first pass also counts NaNs.
//   tf_min_kernel  the smallest alive key above a given key (the second order statistic when it
//     is not the first), as an atomicMax of the complemented key: one per workgroup.
//   tf_apply_kernel  survivors (alive under the final lim = max(threshold, cut)) keep their value
//     or become 1.0f, everything else +0.0f; counts the survivors.
//
// Every count is an integer and the min a max of integers: no result depends on arrival order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

#define TF_COPIES 32
#define TF_UNROLL 4

__device__ __forceinline__ uint32_t tf_key(uint32_t bits) {
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// A workgroup reads TF_UNROLL x 256 contiguous 16-B pieces per trip (16 KB), every thread's
// TF_UNROLL loads issued before the first use; a slot beyond the buffer reads as zeros (never
// alive, never NaN).  NT: non-temporal loads for the read-only passes (a layer beyond the caches
// streams faster that way: tools/stream_ceiling.hip, whose access pattern this is).
template <bool NT>
__device__ __forceinline__ void tf_load(const f32x4* __restrict__ p, int64_t i, int64_t count4,
                                        f32x4 (&v)[TF_UNROLL]) {
#pragma unroll
  for (int u = 0; u < TF_UNROLL; ++u) {
    const int64_t j = i + u * 256;
    v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (j < count4) v[u] = NT ? __builtin_nontemporal_load(p + j) : p[j];
  }
}

// out[0 .. 255] += digit counts, out[256] += NaNs (first pass only).  first: no prefix yet
// (shift = 24); else the keys counted are those with key >> (shift + 8) == prefix.
__global__ __launch_bounds__(256) void tf_hist_kernel(const f32x4* __restrict__ p, int64_t count4,
                                                      uint32_t absmask, float lim, int first,
                                                      uint32_t prefix, int shift,
                                                      unsigned long long* __restrict__ out) {
  __shared__ uint32_t hist[256 * TF_COPIES];
  const int tid = threadIdx.x, copy = tid & (TF_COPIES - 1);
  for (int e = tid; e < 256 * TF_COPIES; e += 256) hist[e] = 0;
  __syncthreads();
  const int pshift = first ? 0 : shift + 8;  // (the prefix test is skipped when first)
  uint32_t nans = 0;
  const int64_t stride = (int64_t)gridDim.x * 256 * TF_UNROLL;
  for (int64_t i = (int64_t)blockIdx.x * 256 * TF_UNROLL + tid; i < count4; i += stride) {
    f32x4 v[TF_UNROLL];
    tf_load<true>(p, i, count4, v);
#pragma unroll
    for (int u = 0; u < TF_UNROLL; ++u) {
      const float f4[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t bits = __float_as_uint(f4[q]) & absmask;
        const float a = __uint_as_float(bits);
        nans += (bits & 0x7fffffffu) > 0x7f800000u;
        const uint32_t key = tf_key(bits);
        const bool alive = a != 0.f && a >= lim;  // (false for a NaN)
        if (alive && (first || (key >> pshift) == prefix))
          atomicAdd(&hist[((key >> shift) & 255u) * TF_COPIES + copy], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int c = 0; c < TF_COPIES; ++c) s += hist[tid * TF_COPIES + ((c + tid) & (TF_COPIES - 1))];
  if (s) atomicAdd(&out[tid], (unsigned long long)s);
  if (first && nans) atomicAdd(&out[256], (unsigned long long)nans);
}

// *out = max(*out, ~key) over the alive keys > xkey (*out zeroed by the caller; ~key >= 1 for
// every key a non-NaN value has, so 0 means none)
__global__ __launch_bounds__(256) void tf_min_kernel(const f32x4* __restrict__ p, int64_t count4,
                                                     uint32_t absmask, float lim, uint32_t xkey,
                                                     unsigned long long* __restrict__ out) {
  __shared__ uint32_t wmin[4];
  const int tid = threadIdx.x;
  uint32_t best = 0xFFFFFFFFu;
  const int64_t stride = (int64_t)gridDim.x * 256 * TF_UNROLL;
  for (int64_t i = (int64_t)blockIdx.x * 256 * TF_UNROLL + tid; i < count4; i += stride) {
    f32x4 v[TF_UNROLL];
    tf_load<true>(p, i, count4, v);
#pragma unroll
    for (int u = 0; u < TF_UNROLL; ++u) {
      const float f4[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t bits = __float_as_uint(f4[q]) & absmask;
        const float a = __uint_as_float(bits);
        const uint32_t key = tf_key(bits);
        if (a != 0.f && a >= lim && key > xkey) best = min(best, key);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m, 64));
  if ((tid & 63) == 0) wmin[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    best = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    if (best != 0xFFFFFFFFu) atomicMax(out, (unsigned long long)(~best));
  }
}

// in place; *kept (optional) += survivors
__global__ __launch_bounds__(256) void tf_apply_kernel(f32x4* __restrict__ p, int64_t count4,
                                                       uint32_t absmask, float lim, int binarize,
                                                       unsigned long long* __restrict__ kept) {
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x;
  uint32_t cnt = 0;
  const int64_t stride = (int64_t)gridDim.x * 256 * TF_UNROLL;
  for (int64_t i = (int64_t)blockIdx.x * 256 * TF_UNROLL + tid; i < count4; i += stride) {
    f32x4 v[TF_UNROLL];
    tf_load<false>(p, i, count4, v);
#pragma unroll
    for (int u = 0; u < TF_UNROLL; ++u) {
      float f4[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float a = __uint_as_float(__float_as_uint(f4[q]) & absmask);
        const bool keep = a != 0.f && a >= lim;
        cnt += keep;
        f4[q] = keep ? (binarize ? 1.0f : a) : 0.0f;
      }
      const int64_t j = i + u * 256;
      if (j < count4) p[j] = (f32x4){f4[0], f4[1], f4[2], f4[3]};
    }
  }
  if (!kept) return;  // (uniform)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long s = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (s) atomicAdd(kept, s);
  }
}

// A workgroup counts in u32: its share of the buffer must stay below 2^32 entries (a buffer of
// 2^41 entries at 1024 workgroups; no HBM holds one).
static inline bool tf_args_ok(const void* A, int64_t count) {
  return A && count >= 0 && count % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0 &&
         count < ((int64_t)1 << 40);
}
static inline unsigned tf_grid(int64_t count4, int cap) {
  const int64_t g = (count4 + 256 * TF_UNROLL - 1) / (256 * TF_UNROLL);
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// A: count fp32 (count a multiple of 4, A 16-B aligned).  absolute: keys and values are |a|.
// pass 0..3: digit bits [24 - 8 pass, 32 - 8 pass) of the alive keys whose higher bits equal
// prefix (pass 0: no prefix).  out: 257 u64, added to (zeroed by the caller).
extern "C" hipError_t n2v2r_launch_tf_hist(const float* A, int64_t count, int absolute, float lim,
                                           int pass, uint32_t prefix, unsigned long long* out,
                                           hipStream_t stream) {
  if (!tf_args_ok(A, count) || pass < 0 || pass > 3 || !out) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const int64_t c4 = count / 4;
  hipLaunchKernelGGL(tf_hist_kernel, dim3(tf_grid(c4, 1024)), dim3(256), 0, stream,
                     reinterpret_cast<const f32x4*>(A), c4, absolute ? 0x7fffffffu : 0xffffffffu,
                     lim, pass == 0 ? 1 : 0, prefix, 24 - 8 * pass, out);
  return hipGetLastError();
}

extern "C" hipError_t n2v2r_launch_tf_min(const float* A, int64_t count, int absolute, float lim,
                                          uint32_t xkey, unsigned long long* out,
                                          hipStream_t stream) {
  if (!tf_args_ok(A, count) || !out) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const int64_t c4 = count / 4;
  hipLaunchKernelGGL(tf_min_kernel, dim3(tf_grid(c4, 2048)), dim3(256), 0, stream,
                     reinterpret_cast<const f32x4*>(A), c4, absolute ? 0x7fffffffu : 0xffffffffu,
                     lim, xkey, out);
  return hipGetLastError();
}

extern "C" hipError_t n2v2r_launch_tf_apply(float* A, int64_t count, int absolute, float lim,
                                            int binarize, unsigned long long* kept,
                                            hipStream_t stream) {
  if (!tf_args_ok(A, count)) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  const int64_t c4 = count / 4;
  hipLaunchKernelGGL(tf_apply_kernel, dim3(tf_grid(c4, 2048)), dim3(256), 0, stream,
                     reinterpret_cast<f32x4*>(A), c4, absolute ? 0x7fffffffu : 0xffffffffu, lim,
                     binarize, kept);
  return hipGetLastError();
}
