// One BCGS-PIP orthogonalisation pass as its launchers (dense.hip) take it, and the prototypes of
// those launchers and of the Grams that feed them: shared by the solver (through engine.h) and
// the stand-alone probes under tools/, so an argument added here reaches every caller.
#pragma once

#include "common.h"

// What a pass does besides Z <- (Z - Q C) R^{-1}.  The solver's three kinds of pass (first,
// selective full, conditional third: Eig::first_pass and its neighbours in solver.cpp) differ
// only in these fields.
struct PipPass {
  const int* cond = nullptr;  // device word; the pass is skipped when it is zero (nullptr: always)
  int* flags = nullptr;       // out: flags[j] != 0 where column j was refilled
  int* any_flag = nullptr;    // out: set when any column was
  double* save = nullptr;     // band save: rows [save_row0, save_row0 + save_rows) of the Gram
  int save_row0 = 0;
  int save_rows = 0;
  int* sticky = nullptr;      // out: set by a refill or a cancelled column, and cleared only by
                              // the cycle's read-back (then the cycle is expanded again)
  uint64_t seed = 0;          // of the refill's counter deviates
  int64_t row0 = 0;           // global index of local row 0 (the deviates' counters)
  double* rsave = nullptr;    // out: R of the pass (8 x 8 fp64; b = 8 only)
  float skip_tol = 0.f;       // selective: blocks with max |Q^T z_j| <= skip_tol ||z_j|| are
                              // left out (fused launch only; 0: every block)
  int* skipped = nullptr;     // skip counters (with skip_tol != 0)
  int first = 0;              // the block's first pass: a pivot the Pythagorean Gram cannot
                              // resolve is clamped and the column kept; later passes refill it
};

// The Gram launcher's decision for a shape (n2v2r_ts_tn_plan): which kernel, over how many row
// chunks, and for the narrow form whether the instantiation that flushes its fp32 sums ran.
enum { TN_FORM_STREAM = 0, TN_FORM_LINES = 1, TN_FORM_NARROW = 2, TN_FORM_MFMA = 3 };
struct TnPlan {
  int form;
  int flush;
  int64_t nchunks, rows_per_chunk;
};

extern "C" {
// The launchers' shape decisions as pure functions; each launcher calls its own.
hipError_t n2v2r_ts_tn_plan(int a_count, int a_width, int b_count, int b_width, int64_t n,
                            size_t partial_elems, TnPlan* plan);
void n2v2r_pip_chol_plan(int c, int b, int with_f, int* stage, int* nwg);
int n2v2r_nn_kernel(int a_count, int a_width, int cb);
hipError_t n2v2r_launch_ts_tn(const BlockList& A, const BlockList& B, int64_t n, double* partial,
                              size_t partial_elems, double* out, const int* cond,
                              hipStream_t stream);
hipError_t n2v2r_launch_ts_tn_zsum(const BlockList& A, int64_t n, const float* const* parts,
                                   int count, float* zout, double* partial, size_t partial_elems,
                                   double* out, hipStream_t stream);
// b = 8, c <= N2V2R_BAND_MAXC: the Cholesky step inside the apply launch.  Reads every field.
hipError_t n2v2r_launch_pip_fused(const BlockList& Q, const float* Zin, float* Zout,
                                  const double* G, int c, int64_t n, const PipPass& pass,
                                  hipStream_t stream);
// The two-launch form (b > 8): pip_chol leaves F = [-C R^{-1}; R^{-1}] in fout for pip_apply.
// pip_chol reads cond, flags, any_flag, save*, sticky, rsave and first; pip_apply reads cond,
// flags, seed and row0.
hipError_t n2v2r_launch_pip_chol(const double* G, int c, int b, double* xinv, float* fout,
                                 const PipPass& pass, hipStream_t stream);
hipError_t n2v2r_launch_pip_apply(const BlockList& QZ, const float* F, int c, int b,
                                  const OutBlockList& Z, int64_t n, const PipPass& pass,
                                  hipStream_t stream);
}
