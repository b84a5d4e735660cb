// The operand path of the Z Z^T tile product (Z = the standardised rows corr_standardise_kernel
// writes: npad x sp fp64, zero padded) and the per-entry evaluation, shared by corr_tile_kernel
// (corr.hip: the layer build) and soft_conn_kernel (soft_threshold.hip: the soft-threshold scan).
// 64 x 64 tiles, four waves, each a 32 x 32 quarter as 2 x 2 v_mfma_f64_16x16x4_f64 tiles, 16 k
// per LDS round; corr.hip's header explains the load shape and the LDS pitch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define CORR_KC 16            // k per LDS round; Z's row pitch sp is a multiple of it
#define CORR_ZP (CORR_KC + 2)  // LDS row pitch of an operand tile, in doubles

// Z's row pitch for s samples: s rounded up to a multiple of CORR_KC (corr.hip)
extern "C" int64_t n2v2r_corr_spad(int64_t s);

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// one round's 64 x 16 operand tiles (rows i0.. and j0.., columns k0..) into registers
__device__ __forceinline__ void corr_load(const double* __restrict__ Z, int64_t sp, int64_t i0,
                                          int64_t j0, int64_t k0, f64x2 (&va)[2],
                                          f64x2 (&vb)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t off = (int64_t)((t >> 3) + 32 * u) * sp + k0 + 2 * (t & 7);
    va[u] = *reinterpret_cast<const f64x2*>(Z + i0 * sp + off);
    vb[u] = *reinterpret_cast<const f64x2*>(Z + j0 * sp + off);
  }
}

// ... and from registers into LDS
__device__ __forceinline__ void corr_stage(double (*za)[CORR_ZP], double (*zb)[CORR_ZP],
                                           const f64x2 (&va)[2], const f64x2 (&vb)[2]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    *reinterpret_cast<f64x2*>(&za[(tid >> 3) + 32 * u][2 * (tid & 7)]) = va[u];
    *reinterpret_cast<f64x2*>(&zb[(tid >> 3) + 32 * u][2 * (tid & 7)]) = vb[u];
  }
}

// one round's MFMAs of the wave whose quarter starts at (wi, wj)
__device__ __forceinline__ void corr_mfma_round(const double (*za)[CORR_ZP],
                                                const double (*zb)[CORR_ZP], int wi, int wj,
                                                int lane, f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < CORR_KC; ks += 4) {
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

// the kind's map of a product entry c, in fp64; kind: N2V2R_CORR_* (include/n2v2r.h)
__device__ __forceinline__ double corr_kind(double c, int kind) {
  const double r = fmin(fmax(c, -1.0), 1.0);
  double t = r;                                // raw
  if (kind == 0) t = fabs(r);                  // unsigned
  else if (kind == 1) t = (1.0 + r) * 0.5;     // signed
  else if (kind == 2) t = fmax(r, 0.0);        // signed hybrid
  return t;
}

// ... to the power, still in fp64: the value the layer build rounds to fp32
__device__ __forceinline__ double corr_value(double c, int kind, double power) {
  double t = corr_kind(c, kind);
  if (power != 1.0) t = pow(t, power);
  return t;
}
