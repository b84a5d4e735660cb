// Co-expression layers built on the GPU (n2v2r_set_layer_corr, include/n2v2r.h): the caller hands
// over an n x s fp64 expression matrix E (n genes, s samples) and the dense fp32 layer
// t(corrcoef(E)) appears in the layer's dA, in the layout n2v2r_set_layer_dense gives it
// (lda = 64 ceil(n / 64)); no n x n array exists on the host.
//
//   corr_standardise_kernel  one wave per row of E, fp64: two-pass mean, centre, divide by the
//     centred row's 2-norm -> Z (npad x sp, npad = 64 ceil(n / 64), sp = 16 ceil(s / 16); columns
//     [s, sp) and rows [n, npad) zero, so the tile kernel loads without bounds tests).  A bad row
//     (a non-finite value, or a constant row: zero centred norm) is written as zeros and its index
//     goes into *bad by atomicMin (the smallest bad row wins, whichever wave gets there first).
//   corr_tile_kernel  C = Z Z^T by v_mfma_f64_16x16x4_f64 over 64 x 64 tiles, as syrk_f64_kernel
//     (gemm.hip): four waves, each a 32 x 32 quarter as 2 x 2 MFMA tiles, 16 k per LDS round.  Z
//     is k-contiguous per row, so a round's 64 x 16 operand tile is loaded as 16-B pieces, 8 lanes
//     per 128-B row segment, one round ahead into registers (in flight across the MFMAs), and
//     kept in LDS as [row][k] with a row pitch of 18 doubles: the operand read of lane l, row
//     l & 15 at k = ks + (l >> 4), then falls on bank pair (18 r + k) mod 32, distinct for the 32
//     lanes of a half wave.  The epilogue is fused: per entry, in fp64, r = clamp(C, -1, 1) (as
//     np.corrcoef clips), the kind's transform, pow(., power) when power != 1, ONE rounding to
//     fp32, the diagonal exactly 1.0f; the fp32 tile goes through LDS so that both the tile and
//     its mirror are stored as contiguous rows.
//
// Symmetry and partitioned handles: entry (i, j) is always computed as the (min, max) element of
// the upper-triangle tile (bi <= bj) that holds it -- the same accumulator of the same lane in
// the same k order whoever asks for it -- and that one fp32 value is stored to (i, j) and (j, i)
// (inside a diagonal tile the upper element serves both places).  The layer is bit-exactly
// symmetric, and a rank that owns rows [row0, row0 + nloc) gets the bits one GPU gets: it
// standardises all of E (the same kernel on the same data), runs the tiles that intersect its row
// band (grid = tile columns x the band's tile rows; a block below the diagonal evaluates its
// tile in the upper orientation and stores it transposed, unless the band also holds the tile's
// own row, whose block then stores both) and writes only its rows.  row0 need not be a multiple
// of 64: every store tests its row against the band.
//
// Padding: columns [n, lda) of the rows written are stored as zeros, the state a fresh
// n2v2r_set_layer_dense allocation has there (DevBuf zero fill; its hipMemcpy2D never touches
// them).  The GEMMs do not depend on it: dense_gemm_kernel masks k >= kdim with a select at its
// LDS store and dense_tn_kernel drops the output columns >= ncols (gemm.hip).  The layer buffer
// holds nloc rows only: nothing is written beyond them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "corr_tile.h"

__global__ __launch_bounds__(256) void corr_standardise_kernel(const double* __restrict__ E,
                                                               int64_t n, int64_t s,
                                                               double* __restrict__ Z, int64_t sp,
                                                               int64_t npad,
                                                               unsigned* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= npad) return;  // (wave-uniform)
  double* z = Z + r * sp;
  if (r >= n) {
    for (int64_t k = lane; k < sp; k += 64) z[k] = 0.0;
    return;
  }
  const double* e = E + r * s;
  double sum = 0.0, lo = e[0], hi = e[0];
  for (int64_t k = lane; k < s; k += 64) {
    const double x = e[k];
    sum += x;
    lo = fmin(lo, x);
    hi = fmax(hi, x);
  }
  sum = wave_sum_f64(sum);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, m, 64));
    hi = fmax(hi, __shfl_xor(hi, m, 64));
  }
  const double mean = sum / (double)s;
  double ss = 0.0;
  for (int64_t k = lane; k < s; k += 64) {
    const double c = e[k] - mean;
    ss += c * c;
  }
  ss = wave_sum_f64(ss);
  // a NaN or an infinity anywhere in the row makes ss non-finite (inf - inf, NaN); a constant
  // row has zero centred norm exactly, whatever the rounding of its mean leaves in ss
  const bool ok = isfinite(ss) && ss > 0.0 && lo < hi;
  if (!ok && lane == 0) atomicMin(bad, (unsigned)r);
  const double norm = sqrt(ss);
  for (int64_t k = lane; k < sp; k += 64) z[k] = (ok && k < s) ? (e[k] - mean) / norm : 0.0;
}

// kind: N2V2R_CORR_* (include/n2v2r.h)
__device__ __forceinline__ float corr_entry(double c, int kind, double power) {
  return (float)corr_value(c, kind, power);
}

__global__ __launch_bounds__(256) void corr_tile_kernel(const double* __restrict__ Z, int64_t sp,
                                                        int64_t n, int64_t row0, int64_t nloc,
                                                        int tb0, float* __restrict__ A,
                                                        int64_t lda, int kind, double power) {
  __shared__ __attribute__((aligned(16))) double za[64][CORR_ZP], zb[64][CORR_ZP];
  __shared__ float tt[64][65];
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
  f64x2 va[2], vb[2];
  corr_load(Z, sp, i0, j0, 0, va, vb);
  for (int64_t k0 = 0; k0 < sp; k0 += CORR_KC) {
    __syncthreads();  // the previous round's LDS reads are done
    corr_stage(za, zb, va, vb);
    __syncthreads();
    if (k0 + CORR_KC < sp) corr_load(Z, sp, i0, j0, k0 + CORR_KC, va, vb);
    corr_mfma_round(za, zb, wi, wj, lane, acc);
  }
  // f64 16x16x4 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = wi + a * 16 + (lane >> 4) + 4 * q, jj = wj + b * 16 + (lane & 15);
        const int64_t gi = i0 + ii, gj = j0 + jj;
        float f = corr_entry(acc[a][b][q], kind, power);
        if (gi == gj) f = 1.0f;
        if (gi >= n || gj >= n) f = 0.f;
        tt[ii][jj] = f;
      }
  __syncthreads();
  const bool diag = bi == bj;
  for (int e = tid; e < 64 * 64; e += 256) {
    const int ii = e >> 6, jj = e & 63;
    const int64_t lr = i0 + ii - row0;
    if (lr >= 0 && lr < nloc) A[lr * lda + j0 + jj] = (diag && ii > jj) ? tt[jj][ii] : tt[ii][jj];
  }
  if (!diag) {
    for (int e = tid; e < 64 * 64; e += 256) {
      const int jj = e >> 6, ii = e & 63;
      const int64_t lr = j0 + jj - row0;
      if (lr >= 0 && lr < nloc) A[lr * lda + i0 + ii] = tt[ii][jj];
    }
  }
}

// Z (64 ceil(n / 64) x sp fp64, sp = n2v2r_corr_spad(s)) = the standardised rows of E (n x s,
// row-major fp64); *bad (set to 0xFFFFFFFF by the caller) = the smallest bad row index.
extern "C" int64_t n2v2r_corr_spad(int64_t s) { return (s + CORR_KC - 1) / CORR_KC * CORR_KC; }

extern "C" hipError_t n2v2r_launch_corr_standardise(const double* E, int64_t n, int64_t s,
                                                    double* Z, unsigned* bad,
                                                    hipStream_t stream) {
  if (n < 1 || s < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  const int64_t npad = (n + 63) / 64 * 64;
  hipLaunchKernelGGL(corr_standardise_kernel, dim3((unsigned)(npad / 4)), dim3(256), 0, stream, E,
                     n, s, Z, n2v2r_corr_spad(s), npad, bad);
  return hipGetLastError();
}

// Rows [row0, row0 + nloc) of the n x n layer into A (nloc x lda fp32, lda = 64 ceil(n / 64)).
extern "C" hipError_t n2v2r_launch_corr_tiles(const double* Z, int64_t s, int64_t n, int64_t row0,
                                              int64_t nloc, float* A, int64_t lda, int kind,
                                              double power, hipStream_t stream) {
  if (nloc <= 0) return hipSuccess;
  const int64_t nt = (n + 63) / 64;
  if (n < 1 || s < 1 || row0 < 0 || row0 + nloc > n || lda != nt * 64 || kind < 0 || kind > 3)
    return hipErrorInvalidValue;
  const int64_t tb0 = row0 / 64, tb1 = (row0 + nloc - 1) / 64;
  if (nt > 0x7fffffffLL || tb1 - tb0 + 1 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(corr_tile_kernel, dim3((unsigned)nt, (unsigned)(tb1 - tb0 + 1)), dim3(256), 0,
                     stream, Z, n2v2r_corr_spad(s), n, row0, nloc, (int)tb0, A, lda, kind, power);
  return hipGetLastError();
}
