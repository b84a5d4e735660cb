// Soft-threshold scan on the GPU (n2v2r_soft_connectivity, include/n2v2r.h): WGCNA's
// pickSoftThreshold needs, for every candidate power p_q, the connectivity of every gene,
//   k[q][i] = sum_{j < n, j != i} pow(t(clamp(z_i . z_j, -1, 1)), p_q),
// with Z the standardised rows corr_standardise_kernel (corr.hip) writes and t the kind's map.
// It is corr_tile_kernel's Z Z^T tile product with another epilogue: every power is applied to an
// entry while the tile is on the chip and the rows are summed instead of stored, all in fp64 (the
// per-entry value is corr_value of corr_tile.h, the one the layer build rounds to fp32).  Nothing
// n x n is written anywhere; the output is P x n doubles.
//
//   soft_conn_kernel  grid (tile rows, G chunks, ceil(P / 8) power groups), 256 threads.  A
//     workgroup owns one 64-row tile row and one contiguous chunk of the tile columns, [g nt / G,
//     (g + 1) nt / G), and walks it tile by tile.  Per tile: the product through corr_tile.h's
//     operand path (64 x 64 tile, four waves, v_mfma_f64_16x16x4_f64, 16 k per LDS round at the
//     18-double pitch, loads one round ahead -- the next tile's first round is in flight across
//     the epilogue); then the r tile goes through LDS ([64][65] doubles, in the operand tiles'
//     place once every wave has read its last operands, as tom_tile_kernel's output tile), because
//     in the MFMA C/D layout a lane holds 8 rows and 8 rows x 8 powers of fp64 sums do not fit
//     the register file.  From LDS thread (lane, wave) owns row `lane` and the 16 columns
//     [16 wave, 16 wave + 16): a wave reads one column of 64 rows at a time (pitch 65: the 32
//     lanes of a half wave fall on distinct bank pairs) and keeps 8 sums, one per power of its
//     group, in registers indexed at compile time, across the whole walk.  A power group beyond
//     the first recomputes the product: 2 sp flops per entry against 8 pow()s.
//     Columns j >= n and the diagonal j == i are masked, never subtracted afterwards: a padded
//     column has r = 0, which is t = 0.5 for the signed kind, not 0.  Rows >= n are not summed.
//     At the end the four column segments of a row are added in ascending order through LDS and
//     the workgroup writes part[g][q][row], one partial per chunk.
//   soft_conn_sum_kernel  conn[q][i] = sum over g ascending of part[g][q][i].
//
// Determinism: no floating-point atomics; each sum has one owner and a fixed order, so the
// result is a function of (E, kind, powers, G) alone, and G = n2v2r_soft_chunks(n) is a function
// of n: with three workgroups resident per CU (below) the 256 CUs take 768 of them, so
// G = ceil(768 / nt), at most nt, and 1 once the tile rows alone fill the CUs.  The partial
// buffer is G P npad doubles (9.6 MB at n = 20,000 with 15 powers).
//
// The full square, not the upper triangle: a symmetric scheme would halve the pow() work, but a
// tile's column sums then belong to another tile row's genes, which takes either floating-point
// atomics (order-dependent) or an (n / 64) x n x P partial buffer (1 GB at n = 20,000).  The
// symmetric variant is out of scope.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   soft_conn_kernel      163 VGPRs, 0 AGPRs, 106 SGPRs (21 spilled to VGPR lanes), scratch 0,
//                         33,280 B LDS, occupancy 3 waves per SIMD = 3 workgroups per CU
//                         (__launch_bounds__(256, 3); held to 128 VGPRs for four it spills 37
//                         VGPRs to 152 B of scratch per lane: pow() inlined eight times)
//   soft_conn_sum_kernel  13 VGPRs, 32 SGPRs, scratch 0, no LDS, occupancy 8
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "corr_tile.h"

#define SOFT_PG 8       // powers per group (the sums a thread keeps)
#define SOFT_RP 65      // LDS row pitch of the r tile, in doubles
#define SOFT_WG_PER_CU 3  // resident workgroups per CU (the resource report above)

__global__ __launch_bounds__(256, 3) void soft_conn_kernel(const double* __restrict__ Z,
                                                           int64_t sp, int64_t n, int64_t npad,
                                                           int nt, int kind,
                                                           const double* __restrict__ powers,
                                                           int P, double* __restrict__ part) {
  // the operand tiles (2 x 64 x 18 doubles), then the r tile, then the four segments' sums
  // (4 x 8 x 64 doubles) share one allocation
  __shared__ __attribute__((aligned(16))) double smem[64 * SOFT_RP];
  double(*za)[CORR_ZP] = reinterpret_cast<double(*)[CORR_ZP]>(smem);
  double(*zb)[CORR_ZP] = za + 64;
  double(*rt)[SOFT_RP] = reinterpret_cast<double(*)[SOFT_RP]>(smem);
  double(*red)[SOFT_PG][64] = reinterpret_cast<double(*)[SOFT_PG][64]>(smem);
  const int R = blockIdx.x, g = blockIdx.y, G = gridDim.y, q0 = blockIdx.z * SOFT_PG;
  const int c0 = (int)((int64_t)g * nt / G), c1 = (int)((int64_t)(g + 1) * nt / G);
  const int np = P - q0 < SOFT_PG ? P - q0 : SOFT_PG;
  const int64_t i0 = (int64_t)R * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
  const int64_t gi = i0 + lane;  // the row this thread sums
  double pw[SOFT_PG], ks[SOFT_PG];
#pragma unroll
  for (int q = 0; q < SOFT_PG; ++q) {
    pw[q] = q < np ? powers[q0 + q] : 1.0;
    ks[q] = 0.0;
  }
  f64x2 va[2], vb[2];
  if (c0 < c1) corr_load(Z, sp, i0, (int64_t)c0 * 64, 0, va, vb);
  for (int c = c0; c < c1; ++c) {
    const int64_t j0 = (int64_t)c * 64;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < sp; k0 += CORR_KC) {
      __syncthreads();  // the previous round's (or the previous tile's r) LDS reads are done
      corr_stage(za, zb, va, vb);
      __syncthreads();
      if (k0 + CORR_KC < sp) corr_load(Z, sp, i0, j0, k0 + CORR_KC, va, vb);
      else if (c + 1 < c1) corr_load(Z, sp, i0, j0 + 64, 0, va, vb);
      corr_mfma_round(za, zb, wi, wj, lane, acc);
    }
    __syncthreads();  // every wave has read its last operands: rt may overwrite them
    // f64 16x16x4 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          rt[wi + a * 16 + (lane >> 4) + 4 * q][wj + b * 16 + (lane & 15)] = acc[a][b][q];
    __syncthreads();
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
      const int jj = wave * 16 + e;
      const int64_t gj = j0 + jj;
      if (gi < n && gj < n && gj != gi) {
        const double t = corr_kind(rt[lane][jj], kind);
#pragma unroll
        for (int q = 0; q < SOFT_PG; ++q)
          if (q < np) ks[q] += pw[q] != 1.0 ? pow(t, pw[q]) : t;  // (as corr_value)
      }
    }
  }
  __syncthreads();  // the last tile's r reads are done
#pragma unroll
  for (int q = 0; q < SOFT_PG; ++q) red[wave][q][lane] = ks[q];
  __syncthreads();
  for (int e = tid; e < SOFT_PG * 64; e += 256) {
    const int q = e >> 6, r = e & 63;
    if (q < np)
      part[((int64_t)g * P + q0 + q) * npad + i0 + r] =
          ((red[0][q][r] + red[1][q][r]) + red[2][q][r]) + red[3][q][r];
  }
}

__global__ __launch_bounds__(256) void soft_conn_sum_kernel(const double* __restrict__ part,
                                                            int G, int P, int64_t npad, int64_t n,
                                                            double* __restrict__ conn) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)P * n) return;
  const int64_t q = idx / n, i = idx % n;
  double s = part[q * npad + i];
  for (int g = 1; g < G; ++g) s += part[((int64_t)g * P + q) * npad + i];
  conn[idx] = s;
}

// the chunk count of the scan: a function of n alone (see the header)
extern "C" int n2v2r_soft_chunks(int64_t n) {
  const int64_t nt = (n + 63) / 64, slots = 256 * SOFT_WG_PER_CU;
  const int64_t G = (slots + nt - 1) / nt;
  return (int)(G < nt ? G : nt);
}

// part (G x P x npad fp64, npad = 64 ceil(n / 64)) = the chunks' partial connectivities of the
// standardised rows Z (npad x n2v2r_corr_spad(s)); powers: P <= 32 doubles on the device
extern "C" hipError_t n2v2r_launch_soft_conn(const double* Z, int64_t s, int64_t n, int kind,
                                             const double* powers, int P, int G, double* part,
                                             hipStream_t stream) {
  const int64_t nt = (n + 63) / 64;
  if (!Z || !powers || !part || n < 1 || s < 1 || nt > 0x7fffffffLL || kind < 0 || kind > 2 ||
      P < 1 || P > 32 || G < 1 || G > nt || G > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(soft_conn_kernel,
                     dim3((unsigned)nt, (unsigned)G, (unsigned)((P + SOFT_PG - 1) / SOFT_PG)),
                     dim3(256), 0, stream, Z, n2v2r_corr_spad(s), n, nt * 64, (int)nt, kind, powers,
                     P, part);
  return hipGetLastError();
}

// conn (P x n fp64) = the chunks' partials summed in ascending chunk order
extern "C" hipError_t n2v2r_launch_soft_conn_sum(const double* part, int G, int P, int64_t n,
                                                 double* conn, hipStream_t stream) {
  if (!part || !conn || n < 1 || P < 1 || P > 32 || G < 1) return hipErrorInvalidValue;
  const int64_t npad = (n + 63) / 64 * 64, blocks = ((int64_t)P * n + 255) / 256;
  hipLaunchKernelGGL(soft_conn_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, part, G,
                     P, npad, n, conn);
  return hipGetLastError();
}
