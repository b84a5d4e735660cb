// The Gram operator (gram_op.h): the form of an application of M = sum_k A_k A_k^T, its set-up
// and its stages, and the diagnostic entry n2v2r_gram_apply (include/n2v2r_diag.h).
#include "gram_op.h"

using namespace n2v2r_int;

namespace n2v2r_int {

bool layers_ready(n2v2r_handle* h) {
  if (h->K < 1) {
    h->err = "no layers set";
    return false;
  }
  for (auto& L : h->layers)
    if (!L->loaded) {
      h->err = "a layer was not loaded";
      return false;
    }
  return true;
}

bool col_blocks_wanted(const n2v2r_handle* h, int b) {
  if (b != 8 || h->dense_layers() || h->layers.empty()) return false;
  const char* e = std::getenv("N2V2R_SPMM_CB");
  if (e && e[0] == '1') return true;
  if (e && e[0] == '0') return false;
  // measured (tools/cb_probe.py, one layer, HIP events): row kernel / column blocks =
  // 0.56 at a 3.2 MB panel (N = 100k: the panel already fits one L2), 1.35 at 9.6 MB,
  // 1.61 at 32 MB, 1.16 at 96 MB, 0.93 at 320 MB (beyond the Infinity Cache the gathers go
  // to HBM either way and the partials only add traffic)
  // round 3: the flat-window tiled form also wins beyond the Infinity Cache -- each phase
  // gathers from one panel block, which the Infinity Cache holds even when the whole panel does
  // not (cfg5 on one GPU, 320 MB panel: 9.5 vs 11.5 ms per stage launch) -- so the window has no
  // upper end
  const double panel = 4.0 * b * (double)h->n;
  return panel > 8.0e6;
}

bool gather_overlap() {
  const char* e = std::getenv("N2V2R_GATHER_OVERLAP");
  return !(e && e[0] == '0');
}

bool split2_wanted(const n2v2r_handle* h, int b) {
  const char* e = std::getenv("N2V2R_SPMM_SPLIT");  // read per fit (tests flip it)
  const int force = e ? (e[0] == '0' ? 0 : 1) : -1;
  if (b != 8 || h->comm || h->dense_layers() || h->K < 2 || h->K > 8) return false;
  if (force >= 0) return force == 1;
  return (double)h->K * (double)h->n * 32.0 > 4.0 * 1024 * 1024;
}

// Column blocks (phases) per layer of <= 2 MB of panel, so a phase's block stays in the XCD's
// 4 MB L2 beside the index stream (cfg4: 16 blocks, 0.748 ms per stage launch; 8 blocks 0.896,
// 32 blocks 0.817: 4 MB blocks left 31 % of the gathers missing L2), at most 64 (cfg5's 320 MB
// panel, one layer launch: 4.36 ms at 64 blocks of 5 MB, 4.62 at 32 of 10 MB, 5.14 at 16 --
// round 5, window offsets, profiles/r05_tile_cfg5.jsonl; with round 4's per-row block pointers
// 64 blocks lost).
int tile_nb_auto(int64_t nglob) {
  int nb = 4;
  while (nb < 64 && (double)nglob * 32.0 / nb > 2.0 * 1024 * 1024) nb *= 2;
  return nb;
}

int tile_rows_for(const n2v2r_handle* h, int wbits) {
  int ncu = 0;
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
  return n2v2r_spmm_tile_rows(h->nloc, ncu, 2, wbits);
}

SpmmTileArgs spmm_tile_args(const CsrBlk* table, int nb, int wbits, int tile_rows, int64_t n,
                            int k0, int nk, int sum, int64_t ldy) {
  SpmmTileArgs a{};
  a.blk = table + (size_t)k0 * nb;
  a.ldx = 8;
  a.ldy = ldy;
  a.n = n;
  a.K = nk;
  a.nb = nb;
  a.sum = sum;
  a.tile_rows = tile_rows;
  a.wbits = wbits;
  return a;
}

// ---- set-up ----------------------------------------------------------------------------------

void GramOp::setup(int b_, bool time_stages) {
  b = b_;
  time_spmm = time_stages;
  tkind.clear();
  tbytes.clear();
  const size_t bb = sizeof(float) * npad * b;
  while ((int)h->ews.zk.size() < K) h->ews.zk.emplace_back(new DevBuf());
  for (int k = 0; k < K; ++k) h->ews.zk[k]->ensure(bb);
  if (h->comm) {
    h->gath.ensure(sizeof(float) * h->world * npad * b);
    h->ews.zg.ensure(sizeof(float) * (size_t)K * h->world * npad * b);
  }
  setup_tiled();
  setup_stage2_form();
}

// the flat-window tiled SpMM: the layers' column blocks and the two stages' block table
void GramOp::setup_tiled() {
  const int64_t nglob = h->n;
  col_blocks = col_blocks_wanted(h, b);
  if (!col_blocks) return;
  // N2V2R_SPMM_TILE_NB = 4..64 overrides the automatic count (read per fit).
  const int nb_auto = tile_nb_auto(nglob);
  const char* tn_ = std::getenv("N2V2R_SPMM_TILE_NB");
  tile_nb = tn_ ? std::atoi(tn_) : nb_auto;
  if (tile_nb != 4 && tile_nb != 8 && tile_nb != 16 && tile_nb != 32 && tile_nb != 64 &&
      tile_nb != 128)
    tile_nb = nb_auto;
  // packed entries need the in-block column bits to fit beside the row-in-window bits
  // (always, for N < 2^26 per block); otherwise the row kernel runs
  tile_wb = tile_wbits(h->layers, tile_nb);
  for (auto& Lp : h->layers)
    col_blocks = ensure_col_blocks(*Lp, nglob, st, tile_nb, tile_wb) && col_blocks;
  if (!col_blocks) return;
  tile_rows = tile_rows_for(h, tile_wb);
  const int nb = tile_nb;
  std::vector<CsrBlk> hb((size_t)2 * K * nb);
  for (int k = 0; k < K; ++k) {
    const LayerDev& L = *h->layers[k];
    for (int j = 0; j < nb; ++j) {
      hb[(size_t)k * nb + j] = (L.symmetric ? L.cb : L.cb_t).blk[j];
      hb[(size_t)(K + k) * nb + j] = L.cb.blk[j];
    }
  }
  h->ews.tblk.ensure(sizeof(CsrBlk) * hb.size());
  HIPCHK(hipMemcpyAsync(h->ews.tblk.p, hb.data(), sizeof(CsrBlk) * hb.size(),
                        hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // hb dies here
}

// the second SpMM stage's form: a reduce-scatter on a row partition, XCD-split on one GPU
void GramOp::setup_stage2_form() {
  rs_form = false;
  if (h->comm && !h->dense_layers()) {
    // read per fit (tests, A/B runs): "rs" / "gather" force a form; unset: the reduce-scatter
    // when there is more than one rank (one rank's "column share" is every row: its stage 2
    // would gather from the whole Z with the row kernel, slower than the tiled gather form)
    const char* e = std::getenv("N2V2R_DIST_STAGE2");
    rs_form = e && std::strcmp(e, "rs") == 0 ? true
              : e && std::strcmp(e, "gather") == 0 ? false
              : h->world > 1;
    if (rs_form) {
      const char* ce = std::getenv("N2V2R_RS_CHUNKS");  // read per fit (tests, A/B runs)
      rs_chunks = std::max(1, std::min(SPMM_MAX_LAYERS, ce ? std::atoi(ce) : 4));
      rs_rc = (npad + rs_chunks - 1) / rs_chunks;
      rs_chunks = (int)((npad + rs_rc - 1) / rs_rc);
      if (rs_chunks <= 1) rs_rc = 0;
      for (auto& Lp : h->layers)
        ensure_colcsr(*Lp, h->n, (int64_t)h->world * npad, st, npad, h->world, rs_rc);
    }
  }
  split2 = split2_wanted(h, b) && !col_blocks;
  pending = nullptr;
  if (split2) h->ews.s2part.ensure(sizeof(float) * (size_t)K * npad * 8);
}

void GramOp::poison_scratch() {
  for (auto& d : h->ews.zk) HIPCHK(hipMemsetAsync(d->p, 0xFF, d->bytes, st));
}

// ---- the stage timers and byte counts --------------------------------------------------------

int GramOp::tbeg() {
  if (!time_spmm) return -1;
  const size_t i = tkind.size();
  while (h->tev.size() < 2 * (i + 1)) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    h->tev.push_back(e);
  }
  HIPCHK(hipEventRecord(h->tev[2 * i], st));
  tkind.push_back(-1);
  tbytes.push_back(0.0);
  return (int)i;
}
void GramOp::tend(int i, int kind, double bytes) {
  if (i < 0) return;
  HIPCHK(hipEventRecord(h->tev[2 * (size_t)i + 1], st));
  tkind[i] = kind;
  tbytes[i] = bytes;
}
void GramOp::tsum(n2v2r_eig_stats* out) {
  if (!time_spmm || !out) return;
  HIPCHK(hipStreamSynchronize(st));
  for (size_t i = 0; i < tkind.size(); ++i) {
    if (tkind[i] < 0) continue;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->tev[2 * i], h->tev[2 * i + 1]));
    out->gpu_ms_spmm[tkind[i]] += ms;
    out->spmm_timed_launches[tkind[i]] += 1;
    out->spmm_stage_bytes[tkind[i]] += tbytes[i];
  }
}
double GramOp::layer_bytes(int k, bool transposed) const {
  const LayerDev& L = *h->layers[k];
  const bool t = transposed && !L.symmetric;
  return spmm_algo_bytes(t ? L.t_nnz : L.nnz, t ? L.t_unit : L.unit, n,
                         (int64_t)h->world * npad, b);
}
// algorithmic bytes of one stage over all layers (fixed layer order)
double GramOp::stage_bytes(bool transposed) const {
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += layer_bytes(k, transposed);
  return s;
}

// ---- W = M X: stage 1, Z_k = A_k^T X, and the forms of stage 2, W = sum_k A_k Z_k -------------

void GramOp::materialize() {
  if (!pending) return;
  const float* parts[SPMM_MAX_LAYERS];
  const int np = pending_parts(parts);
  HIPCHK(n2v2r_launch_zsum(parts, np, pending, n, st));
  pending = nullptr;
}

// Stage 1 of the CSR forms, one launch: Z_k = A_k^T xg for every layer, or for `layer` alone;
// the tiled column-block form when the fit uses it (col_blocks), else the flat one.
void GramOp::stage1(const float* xg, int layer) {
  const int k0 = layer < 0 ? 0 : layer, nk = layer < 0 ? K : 1;
  const double bytes = layer < 0 ? stage_bytes(true) : layer_bytes(layer, true);
  int te;
  if (col_blocks) {
    SpmmTileArgs a = tile_args(false, k0, nk, 0, 8);
    for (int i = 0; i < nk; ++i) {
      a.X[i] = xg;
      a.Y[i] = zk(k0 + i);
    }
    te = tbeg();
    HIPCHK(n2v2r_launch_spmm_tile(a, st));
  } else {
    SpmmArgs a{};
    a.K = nk;
    a.ldx = a.ldy = b;
    // split over the XCDs like the split stage 2 (24.2 -> 23.4 us at cfg2); one GPU only,
    // where every launch takes all layers
    a.split = split2 ? 1 : 0;
    for (int i = 0; i < nk; ++i) {
      a.A[i] = h->layers[k0 + i]->csr_t();
      a.X[i] = xg;
      a.Y[i] = zk(k0 + i);
    }
    a.rpw = rpw1 = n2v2r_spmm_rpw(a, b);  // (the launcher's own choice, kept for n2v2r_gram_apply)
    te = tbeg();
    HIPCHK(n2v2r_launch_spmm(a, b, st));
  }
  tend(te, 0, bytes);
}

// Stage 1 of the gather forms.  Partitioned: every Z_k all-gathered for stage 2 -- one launch
// per layer, each Z_k gathered on the collective stream while the next layer's stage 1 runs, or
// (N2V2R_GATHER_OVERLAP=0, K = 1) one launch and the gathers in line.
void GramOp::stage1_gathered(const float* xg) {
  if (h->comm && K > 1 && gather_overlap() && st == h->stream) {
    for (int k = 0; k < K; ++k) {
      stage1(xg, k);
      h->gather_panel_async(zk(k), gathered_z(k), b, k);
    }
    for (int k = 0; k < K; ++k) h->gather_wait(k);
    return;
  }
  stage1(xg);
  if (h->comm)
    for (int k = 0; k < K; ++k) h->gather_panel(zk(k), gathered_z(k), b);
}

// Stage 2, flat: one launch summing the layers into W -- or (split2) leaving per-layer partials
// on the layers' XCDs, W pending until the next Gram pass or materialize() sums them.
void GramOp::stage2_flat(float* Wout) {
  SpmmArgs s{};
  s.K = K;
  s.sum = 1;
  s.ldx = s.ldy = b;
  for (int k = 0; k < K; ++k) {
    s.A[k] = h->layers[k]->csr();
    s.X[k] = stage2_in(k);
  }
  s.Y[0] = Wout;
  if (split2) {
    materialize();  // (a previous image is always consumed by now; kept for safety)
    s.sum = 0;
    s.split = 1;
    for (int k = 0; k < K; ++k) s.Y[k] = s2part(k);
    pending = Wout;
  }
  s.rpw = rpw2 = n2v2r_spmm_rpw(s, b);
  const double bytes = stage_bytes(false);
  const int te = tbeg();
  HIPCHK(n2v2r_launch_spmm(s, b, st));
  tend(te, 1, bytes);
  for (int k = 0; k < K; ++k) {
    const LayerDev& L = *h->layers[k];
    algo_bytes += spmm_algo_bytes(L.nnz, L.unit, n, n, b) +
                  spmm_algo_bytes(L.symmetric ? L.nnz : L.t_nnz,
                                  L.symmetric ? L.unit : L.t_unit, n, n, b);
  }
  launches += 2;
}

// Stage 2, tiled column blocks: one launch over all layers
void GramOp::stage2_tiled(float* Wout) {
  SpmmTileArgs s = tile_args(true, 0, K, 1, 8);
  for (int k = 0; k < K; ++k) s.X[k] = stage2_in(k);
  s.Y[0] = Wout;
  const double b0 = stage_bytes(true), b1 = stage_bytes(false);
  const int te = tbeg();
  HIPCHK(n2v2r_launch_spmm_tile(s, st));
  tend(te, 1, b1);
  algo_bytes += b0 + b1;
  launches += 2;
}

// Stage 2, reduce-scatter form (partitioned CSR handles, the default at W > 1, DESIGN section
// 6): after stage 1 on the all-gathered X, this rank's column share of stage 2,
// P = sum_k A_k[:, own rows] Z_k[own rows] over all (padded) global rows -- gathered from the
// rank's own Z rows only -- and ONE reduce-scatter of P into W's own rows: one all-gather + one
// reduce-scatter per application instead of K + 1 all-gathers.
void GramOp::stage2_rs(float* Wout) {
  const int64_t ng = (int64_t)h->world * npad;
  float* P = h->ews.zg.as<float>();  // the gather form's Z panels' buffer (>= ng x b)
  const double b0 = stage_bytes(true);
  double b1 = 0.0;
  SpmmArgs s2{};
  s2.K = K;
  s2.sum = 1;
  s2.ldx = s2.ldy = b;
  for (int k = 0; k < K; ++k) {
    const LayerDev& L = *h->layers[k];
    s2.A[k] = L.csr_c();
    s2.X[k] = zk(k);
    b1 += spmm_algo_bytes(L.c_nnz, s2.A[k].unit != 0, ng, npad, b);
  }
  s2.Y[0] = P;
  // the whole share's choice, for every chunk: each row is summed as in one launch
  s2.rpw = rpw2 = n2v2r_spmm_rpw(s2, b);
  const int te = tbeg();
  if (rs_chunks <= 1) {
    HIPCHK(n2v2r_launch_spmm(s2, b, st));
    tend(te, 1, b1);
    h->comm->reduce_scatter_sum_f32(P, Wout, (size_t)npad * b, st);
  } else {
    // pipelined: the column share's rows are chunk-major (ensure_colcsr), so chunk c's product
    // -- rows [c rs_rc, ...) of every rank's block -- is one contiguous range of P, reduce-
    // scattered on the collective stream while chunk c + 1's product runs.  Every row is
    // summed as in the one-launch form (same rows per wave), and every element of W sums the
    // same ranks' values: the same result, with one chunk's reduce-scatter exposed.
    const int W = h->world;
    for (int c = 0; c < rs_chunks; ++c) {
      const int64_t r0 = (int64_t)c * rs_rc;
      const int64_t rows_c = std::min<int64_t>(rs_rc, npad - r0);
      if (rows_c <= 0) break;
      SpmmArgs sc = s2;
      for (int k = 0; k < K; ++k) {
        sc.A[k].indptr = s2.A[k].indptr + (size_t)r0 * W;
        sc.A[k].n_rows = (int64_t)W * rows_c;
      }
      float* pc = P + (size_t)r0 * W * b;
      sc.Y[0] = pc;
      HIPCHK(n2v2r_launch_spmm(sc, b, st));
      h->reduce_scatter_async(pc, Wout + (size_t)r0 * b, (size_t)rows_c * b);
    }
    tend(te, 1, b1);
    h->rs_wait_all();
  }
  algo_bytes += b0 + b1;
  launches += 2;
}

// Dense layers, both stages: Z_k = A_k^T X, W = sum_k A_k Z_k (fixed layer order), GEMMs on
// the local rows
void GramOp::apply_M_dense(const float* xg, float* Wout) {
  const int64_t ng = (int64_t)h->world * npad;  // rows of a gathered panel
  // per GEMM launch: the layer rows read once (4 n N) + the panel read and the output rows
  const double gb = 4.0 * (double)n * (double)h->n + 4.0 * (double)(ng + n) * b;
  for (int k = 0; k < K; ++k) {
    const LayerDev& L = *h->layers[k];
    const int te = tbeg();
    h->dense_apply(L.dense_at(), L.lda, xg, b, b, zk(k), b, 0.f, nullptr,
                   h->comm ? nullptr : L.dense_a());
    tend(te, 0, gb);
  }
  for (int k = 0; k < K; ++k) {
    const LayerDev& L = *h->layers[k];
    if (h->comm) h->gather_panel(zk(k), gathered_z(k), b);
    const int te = tbeg();
    h->dense_apply(L.dense_a(), L.lda, stage2_in(k), b, b, Wout, b, k == 0 ? 0.f : 1.f, nullptr,
                   h->comm ? nullptr : L.dense_at());
    tend(te, 1, gb);
    algo_bytes += 2.0 * gb;
  }
  launches += 2 * K;
}

void GramOp::apply(const float* X, float* Wout) {
  const double t0 = now_ms();
  lds_poison(st);
  const float* xg = X;
  if (h->comm) {
    float* xgb = h->gath.as<float>();
    h->gather_panel(X, xgb, b);
    xg = xgb;
  }
  if (h->dense_layers()) {
    apply_M_dense(xg, Wout);
  } else if (rs_form) {
    stage1(xg);
    stage2_rs(Wout);
  } else {
    stage1_gathered(xg);
    if (col_blocks)
      stage2_tiled(Wout);
    else
      stage2_flat(Wout);
  }
  t_spmm += now_ms() - t0;
}

}  // namespace n2v2r_int

extern "C" {

// One application of M alone (tests): a GramOp set up as a fit's, its apply on a host panel.
int n2v2r_gram_apply(n2v2r_handle* h, int b, const float* X, float* Z, float* W,
                     n2v2r_gram_info* info) {
  return guarded(h, [&]() -> int {
    if (h->multi() || (b != 8 && b != 16 && b != 32 && b != 64) || !X || !W) return N2V2R_ERR_BAD_ARG;
    if (!layers_ready(h)) return N2V2R_ERR_BAD_ARG;
    GramOp op(h);
    op.setup(b);
    hipStream_t st = op.st;
    DevBuf xb, wb;
    xb.ensure(sizeof(float) * op.npad * b, st);
    wb.ensure(sizeof(float) * op.npad * b, st);
    float* x = xb.as<float>();
    float* w = wb.as<float>();
    // NaN bytes wherever the application has to write: the local rows of W, of every Z_k and of
    // the split form's partials (padding rows stay the zeros the solver keeps there), and a rank's
    // gathered panels whole (the collectives write all of them, or all that is read)
    const size_t rows = sizeof(float) * (size_t)op.n * b;
    HIPCHK(hipMemsetAsync(w, 0xFF, rows, st));
    for (int k = 0; k < op.K; ++k) HIPCHK(hipMemsetAsync(op.zk(k), 0xFF, rows, st));
    if (op.split2)
      for (int k = 0; k < op.K; ++k) HIPCHK(hipMemsetAsync(op.s2part(k), 0xFF, rows, st));
    if (h->comm) {
      HIPCHK(hipMemsetAsync(h->gath.p, 0xFF, h->gath.bytes, st));
      HIPCHK(hipMemsetAsync(h->ews.zg.p, 0xFF, h->ews.zg.bytes, st));
    }
    HIPCHK(hipMemcpyAsync(x, X + (size_t)h->row0 * b, rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable source: complete before the kernels
    op.apply(x, w);
    op.materialize();
    HIPCHK(hipMemcpyAsync(W, w, rows, hipMemcpyDeviceToHost, st));
    if (Z)
      for (int k = 0; k < op.K; ++k)
        HIPCHK(hipMemcpyAsync(Z + (size_t)k * op.n * b, op.zk(k), rows, hipMemcpyDeviceToHost,
                              st));
    HIPCHK(hipStreamSynchronize(st));  // (the two panels die here)
    if (info) {
      info->form = op.spmm_form();
      info->rs_form = op.rs_form ? 1 : 0;
      info->rs_chunks = op.rs_form ? op.rs_chunks : 0;
      info->split2 = op.split2 ? 1 : 0;
      info->tile_nb = op.col_blocks ? op.tile_nb : 0;
      info->tile_wb = op.col_blocks ? op.tile_wb : 0;
      info->tile_rows = op.col_blocks ? op.tile_rows : 0;
      info->rpw1 = op.rpw1;
      info->rpw2 = op.rpw2;
    }
    return N2V2R_OK;
  });
}

}  // extern "C"
