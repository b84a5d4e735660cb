// The Gram operator of a fit, W = M X = sum_k A_k (A_k^T X), on one handle or one rank of a
// row-partitioned one: which form an application takes (row kernels, XCD-split second stage,
// flat-window tiled SpMM, reduce-scatter stage 2, dense GEMMs), the buffers of its stages and the
// launch arguments of every form.  The eigensolver (solver.cpp), the embedding step and the SpMM
// diagnostics (engine.cpp) all take them from here.
#pragma once

#include "engine.h"

namespace n2v2r_int {

// h->K >= 1 and every layer loaded; else the reason in h->err (the call returns N2V2R_ERR_BAD_ARG)
bool layers_ready(n2v2r_handle* h);

// N2V2R_POISON: NaN bytes into every CU's LDS before the next launch
inline void lds_poison(hipStream_t st) {
  if (debug_poison()) HIPCHK(n2v2r_launch_lds_poison(st));
}

// The column-block SpMM (the flat-window tiled form): b = 8 CSR panels beyond 8 MB (beyond one
// XCD's L2); N2V2R_SPMM_CB=1 / 0 forces it on / off (tests, A/B runs).
// Read on every call, so a test can switch it between fits.
bool col_blocks_wanted(const n2v2r_handle* h, int b);
// Partitioned handles: the stage-1 panel Z_k of each layer all-gathered on a stream of its own
// while the next layer's stage 1 runs, unless N2V2R_GATHER_OVERLAP=0.  Read per call.
bool gather_overlap();
// XCD-split second SpMM stage: b = 8 CSR layers on one GPU whose K stage-2 panels together
// exceed an XCD's 4 MB L2 (cfg2: 33.5 -> 24 us per stage; at N = 30k, where both panels fit,
// 4 % slower).  N2V2R_SPMM_SPLIT=1 / 0 forces it on / off.
bool split2_wanted(const n2v2r_handle* h, int b);

// The tiled SpMM's automatic column-block (phase) count per layer for a graph of nglob nodes
int tile_nb_auto(int64_t nglob);
// its row tile on this handle's device for windows of 2^wbits rows
int tile_rows_for(const n2v2r_handle* h, int wbits);
// The launch arguments of one tiled SpMM over layers k0 .. k0 + nk - 1 of a stage's block table
// ([layers][nb]: the blocks of A_k^T for stage 1, of A_k for stage 2), b = 8 panels in, rows of
// ldy floats out, summed into Y[0] (sum) or one output per layer.  The caller names X[] and Y[].
SpmmTileArgs spmm_tile_args(const CsrBlk* table, int nb, int wbits, int tile_rows, int64_t n,
                            int k0, int nk, int sum, int64_t ldy);

struct GramOp {
  n2v2r_handle* h;
  hipStream_t st;
  int64_t n;     // local rows
  int64_t npad;  // local rows incl. padding (panel allocation)
  int K;
  int b = 0;     // panel width (setup)
  // the flat-window tiled column-block SpMM (b = 8, panels beyond 8 MB): row tiles with LDS
  // accumulators walking tile_nb column-block phases, one launch per stage
  bool col_blocks = false;
  int tile_rows = 0, tile_nb = CB_NB, tile_wb = CB_WIN_BITS_MIN;
  // partitioned CSR handles: stage 2 as a reduce-scatter of this rank's column share (default
  // at W > 1) instead of all-gathers of every layer's stage-1 panel (N2V2R_DIST_STAGE2=gather)
  bool rs_form = false;
  // reduce-scatter form: stage 2 in rs_chunks row chunks of rs_rc local rows, each chunk's
  // reduce-scatter overlapped with the next chunk's product (N2V2R_RS_CHUNKS, default 4; 1: one
  // launch and one reduce-scatter)
  int rs_chunks = 1;
  int64_t rs_rc = 0;
  // XCD-split second SpMM stage (b = 8, one GPU): A_k Z_k lands in per-layer partials on the
  // XCDs of layer k; the image W = sum_k of them is stored by the next Gram pass that reads it
  // (the local first pass of the next expansion), or by materialize() before any other use
  bool split2 = false;
  float* pending = nullptr;  // the W block whose value still sits in the partials
  // rows per wave of the last row-kernel launch of stage 1 / stage 2 (0: none yet; diagnostics)
  int rpw1 = 0, rpw2 = 0;
  double t_spmm = 0;  // host ms in apply
  int64_t launches = 0;
  double algo_bytes = 0;
  // N2V2R_EIG_TIME_SPMM: an event pair around every SpMM stage launch (h->tev, reused), its
  // stage (0: A_k^T X, 1: A_k Z_k) and algorithmic bytes; summed after the fit's last sync
  bool time_spmm = false;
  std::vector<int> tkind;
  std::vector<double> tbytes;

  explicit GramOp(n2v2r_handle* h_)
      : h(h_), st(h_->stream), n(h_->nloc), npad(h_->npad), K(h_->K) {}

  // The form of the applications at panel width b_ under the switches in force, the derived
  // layer forms it needs (column blocks, column shares) and the stages' buffers.
  void setup(int b_, bool time_stages = false);
  // W = M X = sum_k A_k (A_k^T X); X, W local, gathered panels for the column side
  void apply(const float* X, float* Wout);

  float* zk(int k) const { return h->ews.zk[k]->as<float>(); }  // stage 1's Z_k (local rows)
  float* s2part(int k) const { return h->ews.s2part.as<float>() + (size_t)k * npad * 8; }
  // store the pending image W = sum_k partial_k (fixed layer order)
  void materialize();
  // the pending image's K partials, for a Gram pass that sums and stores the image as it reads
  // it; that pass then calls stored()
  int pending_parts(const float* parts[SPMM_MAX_LAYERS]) const {
    for (int k = 0; k < K; ++k) parts[k] = s2part(k);
    return K;
  }
  void stored() { pending = nullptr; }
  // the tiled launch of stage 1 (A_k^T) or stage 2 (A_k) over layers k0 .. k0 + nk - 1
  SpmmTileArgs tile_args(bool stage2, int k0, int nk, int sum, int64_t ldy) const {
    return spmm_tile_args(h->ews.tblk.as<CsrBlk>() + (size_t)(stage2 ? K : 0) * tile_nb, tile_nb,
                          tile_wb, tile_rows, n, k0, nk, sum, ldy);
  }
  // the application's form as n2v2r_eig_stats.spmm_form codes it
  int spmm_form() const { return h->dense_layers() ? 4 : col_blocks ? 5 : split2 ? 1 : 0; }
  void tsum(n2v2r_eig_stats* out);
  void poison_scratch();  // N2V2R_POISON: NaN bytes into the stage-1 panels

 private:
  int tbeg();
  void tend(int i, int kind, double bytes);
  double layer_bytes(int k, bool transposed) const;
  double stage_bytes(bool transposed) const;
  // partitioned handles: Z_k all-gathered from every rank (rank-major, global rows)
  float* gathered_z(int k) const {
    return h->ews.zg.as<float>() + (size_t)k * h->world * npad * b;
  }
  const float* stage2_in(int k) const { return h->comm ? gathered_z(k) : zk(k); }
  void setup_tiled();
  void setup_stage2_form();
  void stage1(const float* xg, int layer = -1);
  void stage1_gathered(const float* xg);
  void stage2_flat(float* Wout);
  void stage2_tiled(float* Wout);
  void stage2_rs(float* Wout);
  void apply_M_dense(const float* xg, float* Wout);
};

}  // namespace n2v2r_int
