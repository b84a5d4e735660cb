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
//   corr_rank_kernel  (Spearman) one wave per row: E -> its per-row average ranks R, ties sharing
//     their mean rank (scipy.stats.rankdata, R's rank()), by a counting pass over the row in LDS;
//     corr_standardise_kernel then takes R for E: Spearman's Z is Pearson's Z of the ranks.
//   corr_bicor_kernel  (biweight midcorrelation, WGCNA's bicor with maxPOutliers = 1) one wave
//     per row: median and raw MAD selected from the same counts, rows centred by the median and
//     weighted by (1 - u^2)^2, u = (x - med) / (9 MAD), |u| < 1, normalised -> Z in the same
//     layout; a row with MAD = 0 takes the Pearson row (pearsonFallback = "individual").
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

// Row r of E (e, s values in global memory) standardised by its wave into z (sp values): the one
// copy of the Pearson arithmetic, run by corr_standardise_kernel for every row and by
// corr_bicor_kernel for a row whose MAD is zero.
__device__ __forceinline__ void corr_pearson_row(const double* __restrict__ e, int64_t s,
                                                 double* __restrict__ z, int64_t sp, int64_t r,
                                                 int lane, unsigned* __restrict__ bad) {
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
  corr_pearson_row(E + r * s, s, z, sp, r, lane, bad);
}

// ---- the row passes of the other correlation methods ----------------------------------------
// Both rest on one counting pass: for a value x of the row, less = #{j : v_j < x} and equal =
// #{j : v_j == x} over the row's values v (integers, so nothing rounds; IEEE ==, so -0.0 and
// +0.0 tie).  x then has the 1-based average rank less + (equal + 1) / 2, and it is the k-th
// order statistic (0-based) exactly when less <= k < less + equal.  A lane counts for
// CORR_ROW_CB of its elements (lane, lane + 64, ...) at a time while all lanes walk j together:
// every lane reads the same v_j, a broadcast read of the row, which the wave keeps in LDS when
// s <= CORR_ROW_LDS (four waves x 16 KiB: the 64 KiB a launch gets without opting in) and reads
// from global memory (the caches) beyond that.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
// corr_rank_kernel 52 VGPRs, corr_bicor_kernel 60 VGPRs, scratch 0, dynamic LDS only.
#define CORR_ROW_LDS 2048
#define CORR_ROW_CB 4

// DEV: v_j = |row[j] - med| (the deviations whose median is the MAD) instead of row[j].  A slot
// x[c] beyond the row holds NaN and counts nothing.
template <bool DEV>
__device__ __forceinline__ void corr_row_counts(const double* row, int64_t s, double med,
                                                const double (&x)[CORR_ROW_CB],
                                                int (&less)[CORR_ROW_CB],
                                                int (&equal)[CORR_ROW_CB]) {
#pragma unroll
  for (int c = 0; c < CORR_ROW_CB; ++c) less[c] = equal[c] = 0;
#pragma unroll 4
  for (int64_t j = 0; j < s; ++j) {
    const double v = DEV ? fabs(row[j] - med) : row[j];
#pragma unroll
    for (int c = 0; c < CORR_ROW_CB; ++c) {
      less[c] += v < x[c] ? 1 : 0;
      equal[c] += v == x[c] ? 1 : 0;
    }
  }
}

// this lane's elements i0 + lane + 64 c of the row (DEV: their deviations), NaN beyond s
template <bool DEV>
__device__ __forceinline__ void corr_row_own(const double* row, int64_t s, double med, int64_t i0,
                                             int lane, double (&x)[CORR_ROW_CB]) {
#pragma unroll
  for (int c = 0; c < CORR_ROW_CB; ++c) {
    const int64_t i = i0 + lane + 64 * c;
    x[c] = i < s ? (DEV ? fabs(row[i] - med) : row[i]) : __builtin_nan("");
  }
}

// np.median of the row's finite values (DEV: of their deviations from med): the middle order
// statistic, or (a + b) / 2 of the two middle ones.  Every element that is the k-th order
// statistic carries the same value, so a wave maximum over -inf elsewhere broadcasts it.
template <bool DEV>
__device__ __forceinline__ double corr_row_median(const double* row, int64_t s, double med,
                                                  int lane) {
  const int64_t k0 = (s - 1) / 2, k1 = s / 2;
  double a = -__builtin_inf(), b = -__builtin_inf();
  for (int64_t i0 = 0; i0 < s; i0 += 64 * CORR_ROW_CB) {  // (wave-uniform trip count)
    double x[CORR_ROW_CB];
    int less[CORR_ROW_CB], equal[CORR_ROW_CB];
    corr_row_own<DEV>(row, s, med, i0, lane, x);
    corr_row_counts<DEV>(row, s, med, x, less, equal);
#pragma unroll
    for (int c = 0; c < CORR_ROW_CB; ++c) {
      if (less[c] <= k0 && k0 < (int64_t)less[c] + equal[c]) a = x[c];
      if (less[c] <= k1 && k1 < (int64_t)less[c] + equal[c]) b = x[c];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    a = fmax(a, __shfl_xor(a, m, 64));
    b = fmax(b, __shfl_xor(b, m, 64));
  }
  return k0 == k1 ? a : (a + b) / 2.0;
}

// the average ranks of a row of finite values into out (s values)
__device__ __forceinline__ void corr_rank_row(const double* row, int64_t s, int lane,
                                              double* __restrict__ out) {
  for (int64_t i0 = 0; i0 < s; i0 += 64 * CORR_ROW_CB) {
    double x[CORR_ROW_CB];
    int less[CORR_ROW_CB], equal[CORR_ROW_CB];
    corr_row_own<false>(row, s, 0.0, i0, lane, x);
    corr_row_counts<false>(row, s, 0.0, x, less, equal);
#pragma unroll
    for (int c = 0; c < CORR_ROW_CB; ++c) {
      const int64_t i = i0 + lane + 64 * c;
      if (i < s) out[i] = (double)less[c] + 0.5 * (double)(equal[c] + 1);
    }
  }
}

// R (n x s) = the average ranks of the rows of E, one wave per row (dynamic LDS: 4 s doubles when
// staged, none otherwise).  A row that holds a non-finite value gets NaN in every place: a
// comparison with NaN is false, its ranks would be made of finite numbers, and
// corr_standardise_kernel, which takes R next, must refuse the row as it refuses it in E.
__global__ __launch_bounds__(256) void corr_rank_kernel(const double* __restrict__ E, int64_t n,
                                                        int64_t s, double* __restrict__ R,
                                                        int staged) {
  extern __shared__ __attribute__((aligned(16))) double corr_rows[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  const bool live = r < n;  // (wave-uniform)
  const double* e = E + (live ? r : 0) * s;
  double* row = corr_rows + (staged ? (int64_t)wave * s : 0);
  int fin = 1;
  if (live)
    for (int64_t k = lane; k < s; k += 64) {
      const double x = e[k];
      fin &= isfinite(x) ? 1 : 0;
      if (staged) row[k] = x;
    }
  __syncthreads();  // the staged row is visible to every lane of its wave
  if (!live) return;
  double* out = R + r * s;
  if (!__all(fin)) {
    for (int64_t k = lane; k < s; k += 64) out[k] = __builtin_nan("");
    return;
  }
  if (staged)
    corr_rank_row(row, s, lane, out);
  else
    corr_rank_row(e, s, lane, out);
}

// a = (x - med) w, w = (1 - u^2)^2 where |u| < 1, else 0, u = (x - med) / d, d = 9 MAD
__device__ __forceinline__ double corr_bicor_weighted(double x, double med, double d) {
  const double c = x - med, u = c / d, v = 1.0 - u * u;
  return fabs(u) < 1.0 ? c * (v * v) : 0.0;
}

// row: the row's values, in LDS or e itself; e: the row in global memory
__device__ __forceinline__ void corr_bicor_row(const double* row, const double* __restrict__ e,
                                               int64_t s, double* __restrict__ z, int64_t sp,
                                               int64_t r, int lane, unsigned* __restrict__ flag) {
  const double med = corr_row_median<false>(row, s, 0.0, lane);
  const double mad = corr_row_median<true>(row, s, med, lane);  // (>= +0: wave-uniform)
  if (mad == 0.0) {
    // at least half of the row sits on its median: no robust scale.  The Pearson row instead.
    if (lane == 0) {
      atomicAdd(flag + 1, 1u);
      atomicMin(flag + 2, (unsigned)r);
    }
    corr_pearson_row(e, s, z, sp, r, lane, flag);
    return;
  }
  const double d = 9.0 * mad;
  double ss = 0.0;
  for (int64_t k = lane; k < s; k += 64) {
    const double a = corr_bicor_weighted(row[k], med, d);
    ss += a * a;
  }
  ss = wave_sum_f64(ss);
  // (the upper middle deviation is > 0 and <= 2 MAD: |u| <= 2/9 and a != 0 there, so ss > 0
  // unless a^2 underflows or overflows)
  const bool ok = isfinite(ss) && ss > 0.0;
  if (!ok && lane == 0) atomicMin(flag, (unsigned)r);
  const double norm = sqrt(ss);
  for (int64_t k = lane; k < sp; k += 64)
    z[k] = (ok && k < s) ? corr_bicor_weighted(row[k], med, d) / norm : 0.0;
}

// Z as corr_standardise_kernel lays it out, rows standardised for the biweight midcorrelation.
// flag[0]: the smallest bad row (atomicMin, as *bad above: a non-finite value or a constant row);
// flag[1]: the rows that took the Pearson fallback (MAD = 0), flag[2]: the smallest of them.
__global__ __launch_bounds__(256) void corr_bicor_kernel(const double* __restrict__ E, int64_t n,
                                                         int64_t s, double* __restrict__ Z,
                                                         int64_t sp, int64_t npad,
                                                         unsigned* __restrict__ flag, int staged) {
  extern __shared__ __attribute__((aligned(16))) double corr_rows[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  const bool live = r < n;  // (wave-uniform)
  const double* e = E + (live ? r : 0) * s;
  double* row = corr_rows + (staged ? (int64_t)wave * s : 0);
  int fin = 1;
  double lo = e[0], hi = e[0];
  if (live)
    for (int64_t k = lane; k < s; k += 64) {
      const double x = e[k];
      fin &= isfinite(x) ? 1 : 0;
      lo = fmin(lo, x);
      hi = fmax(hi, x);
      if (staged) row[k] = x;
    }
  __syncthreads();  // the staged row is visible to every lane of its wave
  if (r >= npad) return;
  double* z = Z + r * sp;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, m, 64));
    hi = fmax(hi, __shfl_xor(hi, m, 64));
  }
  const bool ok = live && __all(fin) && lo < hi;
  if (!ok) {
    if (live && lane == 0) atomicMin(flag, (unsigned)r);
    for (int64_t k = lane; k < sp; k += 64) z[k] = 0.0;
    return;
  }
  if (staged)
    corr_bicor_row(row, e, s, z, sp, r, lane, flag);
  else
    corr_bicor_row(e, e, s, z, sp, r, lane, flag);
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

// R (n x s fp64) = the average ranks of the rows of E (a row with a non-finite value: NaNs)
extern "C" hipError_t n2v2r_launch_corr_ranks(const double* E, int64_t n, int64_t s, double* R,
                                              hipStream_t stream) {
  if (!E || !R || n < 1 || s < 1 || n > 0x7fffffffLL || s > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const int staged = s <= CORR_ROW_LDS;
  hipLaunchKernelGGL(corr_rank_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256),
                     staged ? sizeof(double) * 4 * (size_t)s : 0, stream, E, n, s, R, staged);
  return hipGetLastError();
}

// Z as n2v2r_launch_corr_standardise lays it out, for the biweight midcorrelation; flag: three
// words set by the caller to {0xFFFFFFFF, 0, 0xFFFFFFFF} (corr_bicor_kernel)
extern "C" hipError_t n2v2r_launch_corr_bicor(const double* E, int64_t n, int64_t s, double* Z,
                                              unsigned* flag, hipStream_t stream) {
  if (!E || !Z || !flag || n < 1 || s < 1 || n > 0x7fffffffLL || s > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const int64_t npad = (n + 63) / 64 * 64;
  const int staged = s <= CORR_ROW_LDS;
  hipLaunchKernelGGL(corr_bicor_kernel, dim3((unsigned)(npad / 4)), dim3(256),
                     staged ? sizeof(double) * 4 * (size_t)s : 0, stream, E, n, s, Z,
                     n2v2r_corr_spad(s), npad, flag, staged);
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
