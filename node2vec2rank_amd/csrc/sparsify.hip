// Dense layer -> CSR in HBM (n2v2r_layers_to_csr, include/n2v2r.h): after a sparsifying transform
// (threshold / top-percent / binarize) a dense-storage layer becomes the CSR the sparse fit reads,
// without visiting the host.  The input is a layer's dA (or dAT): n_rows local rows of fp32,
// leading dimension lda = 64 ceil(n / 64), every row 256-B aligned.
//
// An entry is STORED when a != 0 and its column is < n: -0 is zero and dropped, a NaN is non-zero
// and kept (scipy.sparse.csr_matrix(dense)'s rule).  The column bound is tested explicitly: the
// padding columns [n, lda) need not be zero (a poisoned allocation holds 0xFF bytes there).
//
//   dense_row_count_kernel    one wave per row, 16-B non-temporal loads: the row's count of stored
//     entries (int64) and, per launch, one flag word with bit 0 set when some stored value is not
//     1.0f (integer add / OR only).
//   row_scan_kernel           exclusive scan of the n_rows counts into int64 indptr[n_rows + 1]:
//     one workgroup, wave shuffle scans and a carried base (n_rows is at most tens of thousands in
//     dense storage).
//   dense_row_compact_kernel  one wave per row walking it in chunks of 256 columns (one 16-B load
//     per lane): per chunk the four flag ballots, each lane's count of stored entries below it
//     (mbcnt over the ballots) and a running row offset; a stored entry's int32 column (and its
//     fp32 value unless the layer is unit) goes to indptr[row] + offset + prefix.  The next chunk's
//     load is issued before this chunk's stores.  Columns come out ascending in every row and there
//     are no atomics: the output is a function of the input alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

#define SP_WAVES 4   // rows per workgroup (one wave each)
#define SP_UNROLL 4  // the count kernel's loads in flight per lane

__device__ __forceinline__ bool sp_stored(float v, int64_t col, int64_t n) {
  return v != 0.f && col < n;  // (true for a NaN, false for -0)
}

__global__ __launch_bounds__(64 * SP_WAVES) void dense_row_count_kernel(
    const float* __restrict__ A, int64_t n_rows, int64_t lda, int64_t n,
    int64_t* __restrict__ counts, unsigned* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // (wave-uniform)
  const f32x4* __restrict__ p = reinterpret_cast<const f32x4*>(A + row * lda);
  const int64_t l4 = lda / 4;
  uint32_t cnt = 0, notone = 0;  // (a row holds fewer than 2^31 entries)
  for (int64_t j0 = lane; j0 < l4; j0 += 64 * SP_UNROLL) {
    f32x4 v[SP_UNROLL];
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) {
      const int64_t j = j0 + u * 64;
      v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (j < l4) v[u] = __builtin_nontemporal_load(p + j);
    }
#pragma unroll
    for (int u = 0; u < SP_UNROLL; ++u) {
      const int64_t col0 = (j0 + u * 64) * 4;
      const float f4[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool s = sp_stored(f4[q], col0 + q, n);
        cnt += s;
        notone |= (uint32_t)(s && __float_as_uint(f4[q]) != 0x3F800000u);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
    notone |= (uint32_t)__shfl_xor((int)notone, m, 64);
  }
  if (lane == 0) {
    counts[row] = (int64_t)cnt;
    if (notone) atomicOr(flag, 1u);
  }
}

__global__ __launch_bounds__(256) void row_scan_kernel(const int64_t* __restrict__ counts,
                                                       int64_t n_rows,
                                                       int64_t* __restrict__ indptr) {
  __shared__ long long wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long base = 0;
  for (int64_t i0 = 0; i0 < n_rows; i0 += 256) {
    const int64_t i = i0 + tid;
    const long long c = i < n_rows ? (long long)counts[i] : 0;
    long long inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long long woff = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < w) woff += wsum[k];
      total += wsum[k];
    }
    if (i < n_rows) indptr[i] = (int64_t)(base + woff + inc - c);
    base += total;
    __syncthreads();  // (wsum is rewritten by the next trip)
  }
  if (tid == 0) indptr[n_rows] = (int64_t)base;
}

// val == nullptr: a unit layer (no value stream).  A position at or past indptr[row + 1] is never
// written (it cannot arise while A is the array the counts came from).
__global__ __launch_bounds__(64 * SP_WAVES) void dense_row_compact_kernel(
    const float* __restrict__ A, int64_t n_rows, int64_t lda, int64_t n,
    const int64_t* __restrict__ indptr, int32_t* __restrict__ idx, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // (wave-uniform)
  const f32x4* __restrict__ p = reinterpret_cast<const f32x4*>(A + row * lda);
  const int64_t l4 = lda / 4;
  int64_t pos = indptr[row];
  const int64_t end = indptr[row + 1];
  f32x4 cur = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (lane < l4) cur = __builtin_nontemporal_load(p + lane);
  for (int64_t jb = 0; jb < l4; jb += 64) {  // (jb is wave-uniform)
    const int64_t j = jb + lane;
    f32x4 nxt = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (j + 64 < l4) nxt = __builtin_nontemporal_load(p + j + 64);
    const float f4[4] = {cur[0], cur[1], cur[2], cur[3]};
    bool s[4];
    uint32_t below = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s[q] = sp_stored(f4[q], j * 4 + q, n);  // (a lane past the row holds zeros)
      const unsigned long long b = __ballot(s[q]);
      below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                         __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
      total += (uint32_t)__popcll(b);
    }
    int64_t o = pos + below;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (s[q]) {
        if (o < end) {
          idx[o] = (int32_t)(j * 4 + q);
          if (val) val[o] = f4[q];
        }
        ++o;
      }
    pos += total;
    cur = nxt;
  }
}

static inline bool sp_args_ok(const float* A, int64_t n_rows, int64_t lda, int64_t n) {
  return A && (reinterpret_cast<uintptr_t>(A) & 15) == 0 && n_rows >= 0 &&
         n_rows <= (int64_t)INT32_MAX && lda > 0 && lda % 4 == 0 && n >= 1 && n <= lda &&
         n <= (int64_t)INT32_MAX;
}

// counts[n_rows]; *flag |= 1 when a stored value is not 1.0f (zeroed by the caller)
extern "C" hipError_t n2v2r_launch_dense_row_count(const float* A, int64_t n_rows, int64_t lda,
                                                   int64_t n, int64_t* counts, unsigned* flag,
                                                   hipStream_t stream) {
  if (!sp_args_ok(A, n_rows, lda, n) || !counts || !flag) return hipErrorInvalidValue;
  if (n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(dense_row_count_kernel, dim3((unsigned)((n_rows + SP_WAVES - 1) / SP_WAVES)),
                     dim3(64 * SP_WAVES), 0, stream, A, n_rows, lda, n, counts, flag);
  return hipGetLastError();
}

// indptr[n_rows + 1] = the exclusive scan of counts[n_rows] (n_rows == 0: indptr[0] = 0)
extern "C" hipError_t n2v2r_launch_row_scan(const int64_t* counts, int64_t n_rows, int64_t* indptr,
                                            hipStream_t stream) {
  if (n_rows < 0 || !indptr || (n_rows > 0 && !counts)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(256), 0, stream, counts, n_rows, indptr);
  return hipGetLastError();
}

// idx / val: indptr[n_rows] elements each (val == nullptr for a unit layer)
extern "C" hipError_t n2v2r_launch_dense_row_compact(const float* A, int64_t n_rows, int64_t lda,
                                                     int64_t n, const int64_t* indptr,
                                                     int32_t* idx, float* val,
                                                     hipStream_t stream) {
  if (!sp_args_ok(A, n_rows, lda, n) || !indptr || !idx) return hipErrorInvalidValue;
  if (n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(dense_row_compact_kernel,
                     dim3((unsigned)((n_rows + SP_WAVES - 1) / SP_WAVES)), dim3(64 * SP_WAVES), 0,
                     stream, A, n_rows, lda, n, indptr, idx, val);
  return hipGetLastError();
}
