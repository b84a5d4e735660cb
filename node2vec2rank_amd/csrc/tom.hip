// Topological overlap of a symmetric dense layer on the GPU (n2v2r_tom_layer, include/n2v2r.h):
// WGCNA's TOMsimilarity with TOMDenom = "min".  With a0 = the layer's stored fp32 values as fp64,
// diagonal replaced by 0:
//   unsigned  T_ij = (L_ij + a0_ij) / (min(k_i, k_j) + 1 - a0_ij),  k_i = sum_u a0[i,u]
//   signed    T_ij = |L_ij + a0_ij| / (min(k_i, k_j) + 1 - |a0_ij|), k_i = sum_u |a0[i,u]|
//   L = A0 A0,  T_ii = 1.
//
//   tom_check_kernel  the validation reduction: NaNs and entries outside [0, 1] (unsigned) or
//     [-1, 1] (signed) over the rows given, diagonal included, columns [0, n) only (the padding
//     is never looked at).  Integer counts: no result depends on arrival order.
//   tom_rowsum_kernel  k_i in fp64, one wave per row over 16-B loads, diagonal excluded.
//   tom_tile_kernel  L = A0 A0^T (= A0 A0: the layer is symmetric, so both operands are
//     k-contiguous rows, the shape of corr_tile_kernel's Z Z^T) by v_mfma_f64_16x16x4_f64 over
//     64 x 64 upper-triangle tiles: four waves, each a 32 x 32 quarter as 2 x 2 MFMA tiles, 32 k
//     per LDS round.  A round's 64 x 32 fp32 operand tile is loaded as 16-B pieces, 8 lanes per
//     128-B row segment, one round ahead into registers (in flight across the MFMAs), widened to
//     fp64 on its way into LDS and masked there: element (row r, column k) becomes 0 when r == k
//     (the diagonal is excluded exactly, nothing is subtracted afterwards) or k >= n, and a tile
//     row >= n is not read at all (the layer has n rows, not 64 ceil(n / 64)).  Only the rounds
//     whose k range meets the tile's own rows or the padding test their elements (a
//     workgroup-uniform choice); every other round widens plainly.  LDS keeps [row][k] with a
//     row pitch of 34 doubles: the operand read of lane l, row l & 15 at k = ks + (l >> 4), falls
//     on bank pair (34 r + k) mod 32 = (2 r + k) mod 32, distinct for the 32 lanes of a half
//     wave.  The epilogue is fused: the formula per entry in fp64, ONE rounding to fp32, the
//     diagonal exactly 1.0f, columns [n, lda) +0.0f; the fp32 tile goes through LDS (in the
//     operand tiles' place, once every wave has read its last operands) so that both the tile
//     and its mirror are stored as contiguous rows.  34,816 B of LDS and 102 VGPRs: four
//     workgroups per CU, four waves per SIMD (with a tile of its own the output took the LDS to
//     51 KB and the kernel to three: 161.9 ms against 134.7 ms at n = 20,000).
//
// Symmetry and partitioned handles, as corr.hip: entry (i, j) is always the (min, max) element of
// the upper-triangle tile that holds it, same accumulator, same k order, and that one fp32 value
// is stored to (i, j) and (j, i).  A rank that owns rows [row0, row0 + nloc) is given the whole
// layer (all-gathered), runs the tiles that intersect its band and stores only its rows: the bits
// one GPU gets.  In an off-diagonal tile the entry reads a0_ij from the upper place (i, j); in a
// diagonal tile the upper element serves both places.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

#define TOM_KC 32            // k per LDS round; lda is a multiple of 64
#define TOM_ZP (TOM_KC + 2)  // LDS row pitch of an operand tile, in doubles (see above)

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// counts[0] += NaNs, counts[1] += entries outside [lo, 1]; A: rows x lda, columns [0, n) looked at
__global__ __launch_bounds__(256) void tom_check_kernel(const float* __restrict__ A, int64_t rows,
                                                        int64_t lda, int64_t n, float lo,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ uint32_t wsum[2][4];
  const int tid = threadIdx.x;
  const int64_t lda4 = lda / 4, count4 = rows * lda4;
  uint32_t nans = 0, outs = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + tid; j < count4; j += (int64_t)gridDim.x * 256) {
    const int64_t col = (j % lda4) * 4;
    if (col >= n) continue;
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A) + j);
    const float f4[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (col + q >= n) continue;
      const float a = f4[q];
      if (a != a) ++nans;
      else if (a < lo || a > 1.0f) ++outs;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    nans += (uint32_t)__shfl_xor((int)nans, m, 64);
    outs += (uint32_t)__shfl_xor((int)outs, m, 64);
  }
  if ((tid & 63) == 0) {
    wsum[0][tid >> 6] = nans;
    wsum[1][tid >> 6] = outs;
  }
  __syncthreads();
  if (tid < 2) {
    const unsigned long long s =
        (unsigned long long)wsum[tid][0] + wsum[tid][1] + wsum[tid][2] + wsum[tid][3];
    if (s) atomicAdd(&counts[tid], s);
  }
}

__global__ __launch_bounds__(256) void tom_rowsum_kernel(const float* __restrict__ A, int64_t lda,
                                                         int64_t n, int sgn,
                                                         double* __restrict__ ksum) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform)
  const float* a = A + r * lda;
  double s = 0.0;
  for (int64_t c = 4 * lane; c < n; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(a + c);
    const float f4[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double x = sgn ? fabs((double)f4[q]) : (double)f4[q];
      if (c + q < n && c + q != r) s += x;
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) ksum[r] = s;
}

// rows [r0, r0 + 64) x columns [k0, k0 + 32) of A as they are stored; a row >= n is not read
__device__ __forceinline__ void tom_load(const float* __restrict__ A, int64_t lda, int64_t n,
                                         int64_t r0, int64_t k0, f32x4 (&v)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t row = r0 + (t >> 3) + 32 * u;
    v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (row < n) v[u] = *reinterpret_cast<const f32x4*>(A + row * lda + k0 + 4 * (t & 7));
  }
}

// ... widened to fp64 into z[row][k], the diagonal and the columns >= n as zeros.  MASK = false:
// a round that holds neither (the caller's test, workgroup-uniform): a plain widening
template <bool MASK>
__device__ __forceinline__ void tom_stage(double (*z)[TOM_ZP], int64_t n, int64_t r0, int64_t k0,
                                          const f32x4 (&v)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int lr = (t >> 3) + 32 * u;
    const int64_t row = r0 + lr, col = k0 + 4 * (t & 7);
    const float f4[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
    double d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      d[q] = (MASK && (col + q == row || col + q >= n)) ? 0.0 : (double)f4[q];
    *reinterpret_cast<f64x2*>(&z[lr][4 * (t & 7)]) = (f64x2){d[0], d[1]};
    *reinterpret_cast<f64x2*>(&z[lr][4 * (t & 7) + 2]) = (f64x2){d[2], d[3]};
  }
}

// whether columns [k0, k0 + TOM_KC) of tile rows [r0, r0 + 64) hold a diagonal or a padding element
__device__ __forceinline__ bool tom_masked(int64_t n, int64_t r0, int64_t k0) {
  return k0 + TOM_KC > n || (k0 + TOM_KC > r0 && k0 < r0 + 64);
}

__global__ __launch_bounds__(256, 4) void tom_tile_kernel(const float* __restrict__ A, int64_t lda,
                                                       int64_t n, const double* __restrict__ ksum,
                                                       int sgn, int64_t row0, int64_t nloc,
                                                       int tb0, float* __restrict__ T) {
  // (the fp32 output tile takes the operand tiles' place once the last round is read)
  __shared__ __attribute__((aligned(16))) double zs[2][64][TOM_ZP];
  double(*za)[TOM_ZP] = zs[0], (*zb)[TOM_ZP] = zs[1];
  float(*tt)[65] = reinterpret_cast<float(*)[65]>(&zs[0][0][0]);
  const int c = blockIdx.x, R = tb0 + blockIdx.y;
  if (c < R && c >= tb0) return;  // block (c, R) of this launch stores this tile's mirror
  const int bi = c < R ? c : R, bj = c < R ? R : c;
  const int64_t i0 = (int64_t)bi * 64, j0 = (int64_t)bj * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
  f32x4 va[2], vb[2];
  tom_load(A, lda, n, i0, 0, va);
  tom_load(A, lda, n, j0, 0, vb);
  for (int64_t k0 = 0; k0 < lda; k0 += TOM_KC) {
    __syncthreads();  // the previous round's LDS reads are done
    if (tom_masked(n, i0, k0)) tom_stage<true>(za, n, i0, k0, va);
    else tom_stage<false>(za, n, i0, k0, va);
    if (tom_masked(n, j0, k0)) tom_stage<true>(zb, n, j0, k0, vb);
    else tom_stage<false>(zb, n, j0, k0, vb);
    __syncthreads();
    if (k0 + TOM_KC < lda) {
      tom_load(A, lda, n, i0, k0 + TOM_KC, va);
      tom_load(A, lda, n, j0, k0 + TOM_KC, vb);
    }
#pragma unroll
    for (int ks = 0; ks < TOM_KC; ks += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        av[t] = za[wi + t * 16 + (lane & 15)][ks + (lane >> 4)];
        bv[t] = zb[wj + t * 16 + (lane & 15)][ks + (lane >> 4)];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
  }
  __syncthreads();  // every wave has read its last operands: tt may overwrite them
  // f64 16x16x4 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = wi + a * 16 + (lane >> 4) + 4 * q, jj = wj + b * 16 + (lane & 15);
        const int64_t gi = i0 + ii, gj = j0 + jj;
        float f = 0.f;
        if (gi < n && gj < n) {
          const double x = (double)A[gi * lda + gj];
          const double num = acc[a][b][q] + x;
          const double den = fmin(ksum[gi], ksum[gj]) + 1.0 - (sgn ? fabs(x) : x);
          f = (float)((sgn ? fabs(num) : num) / den);
          if (gi == gj) f = 1.0f;
        }
        tt[ii][jj] = f;
      }
  __syncthreads();
  const bool diag = bi == bj;
  for (int e = tid; e < 64 * 64; e += 256) {
    const int ii = e >> 6, jj = e & 63;
    const int64_t lr = i0 + ii - row0;
    if (lr >= 0 && lr < nloc) T[lr * lda + j0 + jj] = (diag && ii > jj) ? tt[jj][ii] : tt[ii][jj];
  }
  if (!diag) {
    for (int e = tid; e < 64 * 64; e += 256) {
      const int jj = e >> 6, ii = e & 63;
      const int64_t lr = j0 + jj - row0;
      if (lr >= 0 && lr < nloc) T[lr * lda + i0 + ii] = tt[ii][jj];
    }
  }
}

static inline bool tom_args_ok(const void* A, int64_t lda, int64_t n, int type) {
  return A && n >= 1 && n <= 0x7fffffffLL && lda == (n + 63) / 64 * 64 && (type == 0 || type == 1) &&
         (reinterpret_cast<uintptr_t>(A) & 15) == 0;
}

// counts (2 u64, zeroed by the caller): NaNs and out-of-range entries of A (rows x lda fp32)
extern "C" hipError_t n2v2r_launch_tom_check(const float* A, int64_t rows, int64_t lda, int64_t n,
                                             int type, unsigned long long* counts,
                                             hipStream_t stream) {
  if (!tom_args_ok(A, lda, n, type) || rows < 0 || rows > n || !counts)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  // (a workgroup counts in u32: its share of the 2^31 x 2^31 entries at most stays below 2^32
  // only with enough workgroups; 4096 of them hold any layer that fits an HBM)
  const int64_t g = (rows * (lda / 4) + 255) / 256;
  hipLaunchKernelGGL(tom_check_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, stream,
                     A, rows, lda, n, type ? -1.0f : 0.0f, counts);
  return hipGetLastError();
}

// ksum (n fp64) = the row sums of A0 (|A0| for the signed type); A: all n rows
extern "C" hipError_t n2v2r_launch_tom_rowsum(const float* A, int64_t lda, int64_t n, int type,
                                              double* ksum, hipStream_t stream) {
  if (!tom_args_ok(A, lda, n, type) || !ksum) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tom_rowsum_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, A, lda,
                     n, type, ksum);
  return hipGetLastError();
}

// Rows [row0, row0 + nloc) of the n x n overlap into T (nloc x lda fp32); A: all n rows.
extern "C" hipError_t n2v2r_launch_tom_tiles(const float* A, int64_t lda, int64_t n,
                                             const double* ksum, int type, int64_t row0,
                                             int64_t nloc, float* T, hipStream_t stream) {
  if (nloc <= 0) return hipSuccess;
  if (!tom_args_ok(A, lda, n, type) || !ksum || !T || row0 < 0 || row0 + nloc > n)
    return hipErrorInvalidValue;
  const int64_t nt = lda / 64, tb0 = row0 / 64, tb1 = (row0 + nloc - 1) / 64;
  if (tb1 - tb0 + 1 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tom_tile_kernel, dim3((unsigned)nt, (unsigned)(tb1 - tb0 + 1)), dim3(256), 0,
                     stream, A, lda, n, ksum, type, row0, nloc, (int)tb0, T);
  return hipGetLastError();
}
