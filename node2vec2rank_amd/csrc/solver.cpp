// UASE solver (n2v2r_uase and the embedding getters of include/n2v2r.h): the block
// Krylov-Schur driver, on one GPU or on one rank of a row-partitioned handle.
//
// UASE (replaces se.UASE -> scipy svds/ARPACK, model.py:51-55): top-d eigenpairs of
// M = sum_k A_k A_k^T (N x N, = A A^T for the unfolded A = [A_1 | ... | A_K]) by a block
// Krylov-Schur iteration with explicit Rayleigh-Ritz:
//   basis Q = [Q_0 .. Q_{m-1}] (b-wide fp32 blocks in HBM), W_j = M Q_j kept beside it;
//   expand: Z = W_last, two fused BCGS + CholeskyQR passes (+random refill of deficient
//           columns, third pass only then), Q_m = Z, W_m = M Q_m
//           (2 SpMM launches: Z_k = A_k^T Q ; W = sum_k A_k Z_k);
//   cycle:  H = Q^T W (fp64) -> host top-p eigenpairs -> Ritz X = Q S, MX = W S,
//           residuals ||MX_j - theta_j X_j||; converged when all d <= tol * theta_1;
//   restart: next block = orth(W_last) against the old Q, keep [X_p | next] (thick restart).
// Embedding: Y_k = A_k^T U diag(sigma)^(-1/2) (= V diag(sigma)^(1/2) split per layer),
// sigma = sqrt(theta), columns in descending sigma order.
//
// Multi-GPU: rank g of W owns rows [g R, min(N, (g+1) R)), R = ceil(N / W), of
// every layer (and of A_k^T), of every basis block and of the embedding.  Column indices stay
// global: a panel gathered from all ranks (W x R rows, rank-major) is indexed by them directly.
// Per application of M: all-gather X, local SpMM, all-gather each Z_k, local SpMM.  Every
// reduction over rows (Gram blocks, H, residuals, sign keys) is a local fixed-order partial
// + an all-reduce, so every rank holds identical small matrices and runs the identical host
// Rayleigh-Ritz.  Communicators: RCCL (one process per GPU) or an in-process thread group
// (W ranks on one GPU, for testing the partitioned algorithm without W devices).
#include "gram_op.h"

#include <optional>

using namespace n2v2r_int;

namespace n2v2r_int {
// The default basis cap of the b = 8 banded fits: 640 columns, N2V2R_BAND_MAXC = 768 for graphs
// from 4M nodes (round 6: the fused PIP pass past 64 KB of LDS; at cfg4's 1M nodes 768 columns
// are no better -- 771 block applications against 788 on one graph, 846 against 788 on the
// bench's --, at cfg5's 10M they are, see the kept-set rule below; profiles/r06_keep_basis.jsonl).
// The reducing banded Rayleigh-Ritz keeps 640 (kReduceMaxc, engine.h: its arrow, chase and
// back-transform were never run past 640 columns: the Sturm form's fallback beyond is the dense
// one on H expanded from the band).
constexpr int kAutoMaxc = 640;

// The block / keep / basis rule of a fit: block width b, kept Ritz vectors at a restart and the
// basis columns at most, from the wanted dimension d, the graph's N nodes and the caller's
// options (0 = the rule's choice).  Pure: no handle, no HIP call.  Throws N2V2R_ERR_BAD_ARG.
struct BasisPlan {
  int b, keep, maxc;
};
BasisPlan plan_basis(int d, int64_t nglob, int block_opt, int keep_opt, int max_basis_opt,
                     bool dense_rr, bool dense_layers) {
  // default panel width: 8 for CSR layers (vector-applications grow with b); 32 for dense
  // layers, where one application streams all of A whatever b is (HBM-bound up to b = 32)
  int b = block_opt ? block_opt : (dense_layers ? 32 : 8);
  if (b != 8 && b != 16 && b != 32 && b != 64)
    throw StatusFail{N2V2R_ERR_BAD_ARG, "block must be 8, 16, 32 or 64"};
  // small graphs: shrink the block until the Krylov space fits well inside R^n
  int keep = 0, maxc = 0;
  // CSR layers: keep 21d/16 (rounded up to b) -- round 4, on two graphs each: cfg4 795-838
  // block applications against 812-856 at the former 5d/4 (1.51-1.59 vs 1.53-1.63 s), cfg2
  // (84 -> 88) 270 against 276-314, and 11d/8 mixed (profiles/r04_keep_sweep.jsonl); round 5
  // at basis 640, cfg4: keep 152 / 168 / 184 / 200 / 224 / 256 -> 812 / 788 / 821 / 795 / 808
  // / 800 block applications (profiles/r05_keep_b8.jsonl)
  // dense layers (b = 32): keep d + b, basis <= 704 -- on three cfg3-family graphs 61 block
  // applications and 215-218 ms per fit against 66 and 236-240 ms with the general rule's
  // keep 5d/4 = 320 and basis 768 (profiles/r04_cfg3_sweep*.jsonl)
  const bool dense_rule = dense_layers && !block_opt;
  // graphs from 4M nodes (d <= 160, CSR layers): keep 7d/4 and bases up to 768 columns (round
  // 6, d = 128: cfg5's N = 10M 1,728 block applications and 41.9 s per fit against 1,909 and
  // 44.7 s at keep 168 / basis 640; at N = 3M keep 224 and 168 tie, at cfg4's 1M keep 168 and
  // basis 640 win; profiles/r06_keep_basis.jsonl)
  const bool big_graph = !dense_rule && nglob >= ((int64_t)1 << 22) && d <= 160;
  for (;; b /= 2) {
    keep = keep_opt ? keep_opt : (dense_rule ? d + b : std::max(d + 16, (d * 21) / 16));
    keep = ((keep + b - 1) / b) * b;
    // (not past the banded Rayleigh-Ritz's 184 kept vectors where the former rule fit them)
    if (!keep_opt && !dense_rule && b == 8 && keep > 184 && std::max(d + 16, (d * 5) / 4) <= 184)
      keep = 184;
    if (!keep_opt && big_graph && b == 8) keep = std::max(keep, ((d * 7) / 4 + 7) / 8 * 8);
    // default basis: 3.2 keep for the dense Rayleigh-Ritz (its cost grows as c^3); 4.8 keep
    // (<= 512) for the banded one (b = 8), where fewer, longer cycles win (cfg2: 14 cycles
    // at c = 256, 7 at c = 384, 13 % fewer block applications)
    // (a keep that does not fit the banded form's 512-column basis takes the dense one's)
    // (the banded form's basis follows the former keep rule, 5d/4: cfg2 keeps c = 384 -- 270
    // block applications against 305 at 4.8 x 88 = 424)
    const int keep_basis = (keep_opt || dense_rule)
                               ? keep
                               : ((std::max(d + 16, (d * 5) / 4) + b - 1) / b) * b;
    const bool band_ok = b == 8 && !dense_rr && keep + b <= 512;
    // (round 5: up to N2V2R_BAND_MAXC = 640 columns -- cfg4 786-791 block applications and
    // 1.41-1.42 s per fit at c = 576-640 against 838 and 1.51 s at 512,
    // profiles/r05_basis_b8.jsonl)
    maxc = max_basis_opt ? max_basis_opt
                         : (band_ok ? std::min(big_graph ? N2V2R_BAND_MAXC : kAutoMaxc,
                                               std::max(keep + 3 * b, (24 * keep_basis) / 5))
                                    : std::max(keep + 3 * b, (16 * keep_basis) / 5));
    maxc = ((maxc + b - 1) / b) * b;
    const int cap =
        (int)std::min<int64_t>((nglob / 2) / b * b, (int64_t)(N2V2R_MAX_BLOCKS - 1) * b);
    if (maxc > cap) maxc = cap;
    if (maxc > 768) maxc = 768 / b * b;  // Rayleigh-Ritz kernels: c <= 768
    if (dense_rule && !max_basis_opt && maxc > 704) maxc = 704 / b * b;
    if (maxc >= keep + b) break;
    // the auto keep 21d/16 does not fit the basis (d near the 600 limit, small graphs): the
    // former 5d/4
    const int keep_old = ((std::max(d + 16, (d * 5) / 4) + b - 1) / b) * b;
    if (!keep_opt && !dense_rule && keep > keep_old && maxc >= keep_old + b) {
      keep = keep_old;
      break;
    }
    if (b == 8)
      throw StatusFail{N2V2R_ERR_BAD_ARG,
                       "graph too small for the requested dimension: need n >= 2*(keep+8)"};
  }
  return {b, keep, maxc};
}

// The cycle's pinned read-back [res | theta | flags[8] | R | S_last]: residuals and Ritz values
// (keep doubles each), eight flag words, lean images' R (8 x 8 doubles) and the last 8 rows of S
// (floats).  One layout, in 4-byte words, for the device-side pack and the host reads.
struct ReadBack {
  enum Flag { kRefilled = 1, kRrErr = 2, kSecondSolves = 3, kTriErr = 4 };  // slots of flags[8]
  static constexpr int nrr = 64, nsl = 8;
  int wres = 0, wth = 0, wflag = 0, wrr = 0, wsl = 0, words = 0;
  void lay_out(int keep) {
    wth = wres + 2 * keep;
    wflag = wth + 2 * keep;
    wrr = wflag + 8;
    wsl = wrr + 2 * nrr;
    words = wsl + nsl * keep;
  }
  size_t bytes(int upto_word) const { return sizeof(int32_t) * (size_t)upto_word; }
  template <class T>
  T* at(void* pin, int word) const {
    return reinterpret_cast<T*>(static_cast<int32_t*>(pin) + word);
  }
};

// The two selective passes of a pair after its Gram g2 = [Q Za Zb]^T [Za Zb] (ts_tn2): Za's pass
// against Q, Zb's Gram against the corrected Za (pair_fixup), Zb's pass against [Q Za].  With a
// plan buffer, and where the plan fits it, one small launch plans both and one applies them in
// one read of Q (pip_pair: returns true); else the three launches.
bool pair_apply_launches(const BlockList& all, double* g2, int64_t n, const PipPass& pa,
                         const PipPass& pz, int* plan, size_t plan_bytes, hipStream_t st) {
  const int nq_old = all.count - 2;
  float* za = const_cast<float*>(all.blk[nq_old]);
  float* zb = const_cast<float*>(all.blk[nq_old + 1]);
  BlockList q = all;
  q.count = nq_old;
  if (plan) {
    const hipError_t pe = n2v2r_launch_pip_pair(q, za, zb, g2, n, pa.flags, pa.any_flag, pa.sticky,
                                                pa.seed, pz.seed, pa.row0, pa.skip_tol, pa.skipped,
                                                plan, plan_bytes, st);
    if (pe == hipSuccess) return true;
    if (pe != hipErrorNotSupported) throw HipFail{pe, "n2v2r_launch_pip_pair"};
  }
  HIPCHK(n2v2r_launch_pip_fused(q, za, za, g2, nq_old * 8, n, pa, st));
  HIPCHK(n2v2r_launch_pair_fixup(g2, nq_old + 2, nq_old, pa.rsave, st));
  q.count = nq_old + 1;
  HIPCHK(n2v2r_launch_pip_fused(q, zb, zb, g2 + (size_t)(nq_old + 2) * 64, (nq_old + 1) * 8, n, pz,
                                st));
  return false;
}

// ---- the eigensolver ----------------------------------------------------------------------
struct Eig {
  n2v2r_handle* h;
  hipStream_t st;
  int64_t n;        // local rows
  int64_t npad;     // local rows incl. padding (panel allocation)
  int64_t row0;     // global index of local row 0
  int K;
  GramOp op;        // W = M X in the fit's form
  int b = 0;        // block width
  int nb_max = 0;   // max basis blocks
  int pb = 0;       // kept blocks at restart
  int d = 0;
  uint64_t seed = 0;
  std::vector<float*> freelist;
  std::vector<float*> Q, W;                   // current basis / images
  n2v2r_eig_stats* stats = nullptr;
  double t_ortho = 0;
  uint64_t fill_counter = 0;
  int kry0 = 0;             // index of the first Krylov block of the current cycle
  bool full_first = false;  // N2V2R_EIG_FULL_FIRST_PASS
  bool band_rr = false;     // banded Rayleigh-Ritz (b = 8, c <= 640), else dense
  bool band_reduce = false; // the reducing banded path takes the cycle (keep + 8 <= 192, c <= 640)
  // the final lean check's stage-1 products Z_k = A_k^T X[q] of the d wanted Ritz vectors, kept
  // in the embedding buffer (h->Y, unscaled): they ARE the embedding's A_k^T U before the sign
  // and sigma^-1/2 column scaling -- the same tiled launch, the same summation order -- so the
  // embedding step skips its d/8 SpMM launches (cfg4: 16 x 0.74 ms)
  bool y_captured = false;
  // the last ritz_vectors: whether the fused kernel made the products, and the product launches
  // (1 fused; else one ts_nn launch per slice and product) (diagnostics)
  bool ritz_done = false;
  int ritz_launches = 0;
  int stats_rr_fallbacks = 0;  // Sturm Rayleigh-Ritz cycles redone by the reducing path
  // dense Rayleigh-Ritz: the multi-workgroup tridiagonalisation's error word of the current
  // cycle (nullptr: the one-workgroup kernel ran), and whether a timeout switched the fit to the
  // one-workgroup kernel
  int* tri_err = nullptr;
  bool tri_single = false;
  int tri_fallbacks = 0;
  // Lean images: only the images a later step reads are kept (the cycle's input and the newest
  // one), so the basis alone (<= 154 MB at cfg2) stays in the 256 MB Infinity Cache between its
  // Gram and apply passes.  Residuals are the Krylov-Schur estimates ||R_E s_j|| (R_E: the
  // triangular factor of the restart block's projection), and a fit is finished only after the
  // true residuals of its d vectors (their images by SpMM) pass.
  bool lean_off = false;  // set by the caller to rerun a fit without lean images
  // selective reorthogonalisation: a full pass after the local one is skipped (in the fused
  // launch, by every workgroup alike) when max |Q^T z_j| <= reorth_tol ||z_j||
  float reorth_tol = 0.f;
  // deferred full passes (lean images, lazy two-pass mode; N2V2R_REORTH_DEFER=0: off): every other Krylov
  // block goes to its SpMM after the local pass alone and gets its full pass together with the
  // next block's (a pair shares one read of the old basis once a two-block Gram exists); its
  // image keeps the uncorrected block, whose components along older blocks are removed from
  // the next block by that block's full pass.  `deferred`: the block awaiting its full pass.
  bool defer = false;
  bool pair_apply = false;  // a pair's two selective passes in one launch (N2V2R_PAIR_APPLY)
  float* deferred = nullptr;
  struct LeanRetry {};
  // an Eig on a handle, or on one rank of a partitioned one
  explicit Eig(n2v2r_handle* h_)
      : h(h_), st(h_->stream), n(h_->nloc), npad(h_->npad), row0(h_->row0), K(h_->K), op(h_) {}

  // ---- the fit's plan: what run()'s set-up steps decide and the cycle's steps read ----
  int flags = 0;  // n2v2r_eig_opts.solver_flags
  bool flag(int f) const { return (flags & f) != 0; }
  int keep = 0, c_max = 0;  // kept Ritz vectors at a restart; basis columns at most
  double tol = 0, stag_cap = 0;
  int max_restarts = 0;
  bool sturm = false;  // banded cycles start with the Sturm form
  bool lean = false;   // lean images (above)
  bool lazy = true;    // two orthogonalisation passes, until a cycle had to be expanded again
  ReadBack rb;
  // ---- the fit's progress ----
  int cycle = 0, apps = 0, conv = 0, stagnated = 0, lean_checks = 0;
  double maxres = 0, t_start = 0, t_rr = 0;
  double est_scale = 1.0;    // lean: true / estimated residual seen at a failed final check
  double last_true = 1e300;  // lean: the worst true residual of the previous check
  bool rr_armed = false;  // the Rayleigh-Ritz error words zeroed (then by every read-back)
  bool tri_test_armed = false;  // N2V2R_EIG_TEST_TRI_TIMEOUT: until the first error word read
  std::vector<float*> X, MX;    // the cycle's Ritz vectors and images (pb blocks)
  float* E_lean = nullptr;      // lean: the restart block, built before the convergence test
  std::vector<double> wh, res2, hist_res;  // Ritz values, squared residuals, max_res per cycle

  // Gram scratch of the orthogonalisation passes (the workspace's)
  double* part_p = nullptr;
  size_t part_n = 0;
  double* gsm_p = nullptr;
  int* flg_p = nullptr;
  int* any_p = nullptr;

  // N2V2R_DEBUG_FINITE: stop at the first stage whose output holds a non-finite value
  int dbg_cycle = 0, dbg_apps = 0;
  void dbg(const void* p, int64_t count, bool f64, const char* what) {
    if (!debug_finite() || !p || count <= 0) return;
    int* flag = h->ews.dbgflag.as<int>();
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), st));
    HIPCHK(n2v2r_launch_nonfinite(p, count, f64 ? 1 : 0, flag, st));
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) {
      const std::string msg = std::string("non-finite values first seen in ") + what +
                              " (cycle " + std::to_string(dbg_cycle) + ", block application " +
                              std::to_string(dbg_apps) + ", b " + std::to_string(b) + ")";
      fprintf(stderr, "[n2v2r] %s\n", msg.c_str());
      throw StatusFail{N2V2R_ERR_INTERNAL, msg};
    }
  }
  // N2V2R_DEBUG_ORTHO=1 (diagnostics): the Gram of a new block against the basis and itself,
  // reported on stderr when it is off the identity by more than 1e-3 (the block may still be
  // waiting for its deferred full pass: then its coupling to the old blocks is expected)
  void dbg_ortho(float* z, const std::vector<float*>& basis, const char* what,
                 const int* flags = nullptr) {
    if (!debug_ortho()) return;
    std::vector<float*> all(basis);
    all.push_back(z);
    const int nq = (int)all.size();
    DevBuf g;
    g.ensure(sizeof(double) * (size_t)nq * b * b);
    tn(blocks(all, 0, nq), one(z), g.as<double>(), nullptr);
    std::vector<double> hg((size_t)nq * b * b);
    HIPCHK(hipMemcpyAsync(hg.data(), g.p, sizeof(double) * hg.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double off = 0.0, self = 0.0, nrm = 0.0;
    for (int r = 0; r < nq * b; ++r)
      for (int j = 0; j < b; ++j) {
        const double v = hg[(size_t)r * b + j];
        if (r >= (nq - 1) * b) {
          const int i = r - (nq - 1) * b;
          self = std::max(self, std::fabs(v - (i == j ? 1.0 : 0.0)));
          if (i == j) nrm = std::max(nrm, v);
        } else {
          off = std::max(off, std::fabs(v));
        }
      }
    int fl[8] = {};
    if (flags) {
      HIPCHK(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (off > 1e-3 || self > 1e-3)
      fprintf(stderr, "[n2v2r] %s: cycle %d, application %d, basis %d blocks: |Q^T z| %.3e, "
              "|z^T z - I| %.3e, max z_j^T z_j %.3e%s flags %d%d%d%d%d%d%d%d\n", what,
              dbg_cycle, dbg_apps, nq - 1, off, self, nrm, deferred == z ? " (deferred)" : "",
              fl[0], fl[1], fl[2], fl[3], fl[4], fl[5], fl[6], fl[7]);
  }

  // N2V2R_POISON: NaN-fill the scratch a fit must write before it reads it
  void poison_scratch() {
    if (!debug_poison()) return;
    EigWorkspace& w = h->ews;
    for (DevBuf* d : {&w.rinv, &w.flg, &w.anyflag, &w.gsmall, &w.csmall, &w.tri, &w.refl,
                      &w.ytri, &w.tscr, &w.hband, &w.band, &w.varr, &w.taua, &w.rrerr, &w.fcoef,
                      &h->partial, &h->theta, &h->resid})
      if (d->p) HIPCHK(hipMemsetAsync(d->p, 0xFF, d->bytes, st));
    for (auto& d : w.pool) HIPCHK(hipMemsetAsync(d->p, 0xFF, d->bytes, st));
    op.poison_scratch();
  }

  float* take() {
    if (freelist.empty()) {
      h->ews.pool.emplace_back(new DevBuf());
      h->ews.pool.back()->ensure(sizeof(float) * npad * b, st);
      return h->ews.pool.back()->as<float>();
    }
    float* p = freelist.back();
    freelist.pop_back();
    return p;
  }
  void give(float* p) {
    if (p) freelist.push_back(p);
  }

  BlockList blocks(const std::vector<float*>& v, int from, int count) const {
    BlockList L{};
    L.count = count;
    L.width = b;
    for (int i = 0; i < count; ++i) L.blk[i] = v[from + i];
    return L;
  }
  BlockList one(const float* p) const {
    BlockList L{};
    L.count = 1;
    L.width = b;
    L.blk[0] = p;
    return L;
  }
  OutBlockList out_one(float* p) const {
    OutBlockList L{};
    L.count = 1;
    L.width = b;
    L.blk[0] = p;
    return L;
  }

  // TN over local rows, summed over ranks
  void tn(const BlockList& A, const BlockList& B, double* out, const int* cond) {
    HIPCHK(n2v2r_launch_ts_tn(A, B, n, part_p, part_n, out, cond, st));
    if (h->comm)
      h->allreduce_f64(out, (size_t)A.count * A.width * B.count * B.width);
  }

  // ---- the orthogonalisation passes --------------------------------------------------------------
  // Three kinds of pass, each with a flag slot s of its own: refill flags at
  // flg_p + 64 s, any-flag at any_p + s.  any_p + 3 is the cycle's sticky flag.

  // the refill seed of the next pass: one per pass, in launch order
  uint64_t last_fill_seed = 0;  // (diagnostics)
  uint64_t next_fill_seed() { return last_fill_seed = seed ^ (0xABCDull + ++fill_counter); }

  PipPass pass_in_slot(int s) const {
    PipPass p;
    p.flags = flg_p + 64 * s;
    p.any_flag = any_p + s;
    p.row0 = row0;
    return p;
  }
  // The blocks a block's first pass takes: `local` (the blocks W_from couples to in exact
  // arithmetic), or the whole basis when there is no such subset or full_first asks for it.
  const std::vector<float*>& first_blocks(const std::vector<float*>& basis,
                                          const std::vector<float*>* local) const {
    return local && !full_first && local->size() < basis.size() ? *local : basis;
  }
  // First pass (slot 0) against `first` = first_blocks(basis, local).  save (band Rayleigh-Ritz):
  // the Gram rows of the `local` blocks, the last ones of `first`, are kept as a band column.
  PipPass first_pass(const std::vector<float*>& first, const std::vector<float*>* local,
                     double* save, int* sticky, double* rsave) const {
    const int nsave = (save && local) ? (int)local->size() : 0;
    PipPass p = pass_in_slot(0);
    p.first = 1;
    p.save = nsave ? save : nullptr;
    p.save_row0 = ((int)first.size() - nsave) * b;
    p.save_rows = nsave * b;
    p.sticky = sticky;
    p.rsave = rsave;
    return p;
  }
  // Selective full pass (slot 1): blocks whose coupling to Z is within reorth_tol are left out
  PipPass selective_pass(int* sticky, double* rsave = nullptr) const {
    PipPass p = pass_in_slot(1);
    p.skip_tol = reorth_tol;
    p.skipped = reorth_tol != 0.f ? h->ews.skipc.as<int>() : nullptr;
    p.sticky = sticky;
    p.rsave = rsave;
    return p;
  }
  // Third pass (slot 2): runs only when the selective pass had to refill a column
  PipPass third_pass() const {
    PipPass p = pass_in_slot(2);
    p.cond = any_p + 1;
    return p;
  }

  // One fused BCGS + CholQR pass: G = [Q Z]^T Z -> R^{-1} -> Z <- [Q Z] [-C R^{-1}; R^{-1}],
  // refill deficient columns.  Takes the next refill seed.
  // Zin (default Z): the block to orthogonalise; the result is written to Z
  void pip_pass(float* Z, const std::vector<float*>& basis, PipPass p,
                const float* Zin = nullptr) {
    p.seed = next_fill_seed();
    const float* zin = Zin ? Zin : Z;
    const int nq = (int)basis.size();
    std::vector<float*> qz(basis);
    qz.push_back(const_cast<float*>(zin));
    const BlockList L = blocks(qz, 0, nq + 1);
    bool done = false;
    if (op.pending && zin == op.pending && !p.cond && !h->comm) {
      // the Gram pass that first reads the pending image also stores it
      const float* parts[SPMM_MAX_LAYERS];
      const int np = op.pending_parts(parts);
      const hipError_t e = n2v2r_launch_ts_tn_zsum(L, n, parts, np, op.pending, part_p, part_n,
                                                   gsm_p, st);
      if (e == hipSuccess) {
        op.stored();
        done = true;
      } else if (e != hipErrorNotSupported) {
        throw HipFail{e, "n2v2r_launch_ts_tn_zsum"};
      }
    }
    if (!done) {
      if (zin == op.pending) op.materialize();
      tn(L, one(zin), gsm_p, p.cond);
    }
    if (b == 8 && nq * b <= N2V2R_BAND_MAXC) {
      // b = 8: the Cholesky step runs inside the apply launch (every workgroup factors G)
      HIPCHK(n2v2r_launch_pip_fused(blocks(qz, 0, nq), zin, Z, gsm_p, nq * b, n, p, st));
      return;
    }
    // wider blocks: the two-launch form
    if (p.rsave && b != 8) throw StatusFail{N2V2R_ERR_INTERNAL, "R output needs b = 8"};
    // (skip_tol: the unfused pass always applies)
    HIPCHK(n2v2r_launch_pip_chol(gsm_p, nq * b, b, h->ews.rinv.as<double>(),
                                 h->ews.fcoef.as<float>(), p, st));
    // rank-deficient columns (p.flags) are refilled with random values by the same launch
    HIPCHK(n2v2r_launch_pip_apply(L, h->ews.fcoef.as<float>(), nq * b, b, out_one(Z), n, p, st));
  }

  // orthonormalise Zin (default: Z in place) against `basis` and within itself into Z.
  // Default: a first fused pass against `local` only (the blocks W_from = M Q_last couples to in
  // exact arithmetic: the block three-term recurrence), then one full pass (block CGS2 with a
  // local first pass: the full pass removes the fp32 loss-of-orthogonality components); a third
  // full pass only when the second one had to refill a rank-deficient column.  `local` empty or
  // full_first: the first pass is a full one too (BCGS-PIP2).
  // save (band Rayleigh-Ritz): the first pass's Gram rows of the `local` blocks,
  // Q_loc^T W_from, are kept as band column j of the projected matrix.
  // lazy: no third pass; a refill in the second pass sets the cycle's sticky flag instead and
  // the cycle is expanded again with the third pass (rank deficiency after a local + full pass
  // is rare: it saves four launches per block).
  // rsave_first: R of the first pass (lean images: its column norms are the residual estimates)
  void orthonormalize(float* Z, const std::vector<float*>& basis, const float* Zin = nullptr,
                      const std::vector<float*>* local = nullptr, double* save = nullptr,
                      bool lazy = false, double* rsave_first = nullptr) {
    const double t0 = now_ms();
    lds_poison(st);
    int* flg = flg_p;
    const std::vector<float*>& first = first_blocks(basis, local);
    // (no sticky flag here: a column the first pass cancelled -- scaled, not normalised -- is
    // normalised by the full pass that always follows; a refill there (a later pass) sets it.
    // BASELINE cfg3's first images cancel: with the flag each fit expanded cycle 0 twice)
    pip_pass(Z, first, first_pass(first, local, save, nullptr, rsave_first), Zin);
    if (debug_ortho()) {  // pass 1's Gram [Q Z]^T Z (still in gsm_p)
      const int c1 = (int)first.size() * b;
      std::vector<double> g((size_t)(c1 + b) * b);
      HIPCHK(hipMemcpyAsync(g.data(), gsm_p, sizeof(double) * g.size(), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      fprintf(stderr, "[n2v2r] pass 1 Gram (c %d): Z^T Z diag", c1);
      for (int j = 0; j < b; ++j) fprintf(stderr, " %.4e", g[(size_t)(c1 + j) * b + j]);
      fprintf(stderr, "; C^T C diag");
      for (int j = 0; j < b; ++j) {
        double a = 0.0;
        for (int r = 0; r < c1; ++r) a += g[(size_t)r * b + j] * g[(size_t)r * b + j];
        fprintf(stderr, " %.4e", a);
      }
      fprintf(stderr, "\n");
    }
    dbg_ortho(Z, first, "after pass 1 (local)", flg);
    // (rsave_first: the second pass's R too, folded into the first's: R2 R1)
    pip_pass(Z, basis, selective_pass(lazy ? any_p + 3 : nullptr,
                                      rsave_first ? rsave_first + 64 : nullptr));
    if (rsave_first) HIPCHK(n2v2r_launch_rmul8(rsave_first + 64, rsave_first, st));
    dbg_ortho(Z, basis, "after pass 2 (full, selective)", flg + 64);
    if (!lazy) pip_pass(Z, basis, third_pass());
    if (!lazy) dbg_ortho(Z, basis, "after pass 3", flg + 128);
    t_ortho += now_ms() - t0;
  }

  // the deferred block's full pass against the blocks before it (its place in `basis`)
  void flush_deferred(const std::vector<float*>& basis) {
    if (!deferred) return;
    const auto it = std::find(basis.begin(), basis.end(), deferred);
    if (it == basis.end()) throw StatusFail{N2V2R_ERR_INTERNAL, "deferred block left the basis"};
    const std::vector<float*> pre(basis.begin(), it);
    const double t0 = now_ms();
    if (!pre.empty()) pip_pass(deferred, pre, selective_pass(any_p + 3));
    t_ortho += now_ms() - t0;
    deferred = nullptr;
  }

  // The full passes of the deferred block Za (the last block of `basis`) and of the new block
  // Zb in one read of the old basis Q: G = [Q Za Zb]^T [Za Zb] (ts_tn_stream2), Za's selective
  // pass against Q (its R kept), Zb's Gram against the corrected Za (pair_fixup), Zb's selective
  // pass against [Q Za] -- planned by one small launch and applied by one that loads each basis
  // block once for both (pip_pair, N2V2R_PAIR_APPLY=fused), or as three launches (the default).
  // false when the two-block Gram does not apply (then the caller runs the two passes one after
  // the other).
  bool pair_pass(float* zb, const std::vector<float*>& basis) {
    if (!deferred || basis.empty() || basis.back() != deferred) return false;
    const int nq_old = (int)basis.size() - 1;
    if (nq_old + 2 > N2V2R_MAX_BLOCKS || (nq_old + 1) * 8 > N2V2R_BAND_MAXC) return false;
    std::vector<float*> all(basis);
    all.push_back(zb);
    // sized for the largest basis when the fit starts (a growing buffer reallocated here cost a
    // device-wide synchronisation per pair in a fit's first cycle: cfg2 +1.5 ms per fit)
    if (h->ews.g2.bytes < sizeof(double) * 2 * (size_t)(nq_old + 2) * 64) return false;
    double* g2 = h->ews.g2.as<double>();
    const double t0 = now_ms();
    lds_poison(st);
    const BlockList L = blocks(all, 0, nq_old + 2);
    const hipError_t e = n2v2r_launch_ts_tn2(L, deferred, zb, n, part_p, part_n, g2, st);
    if (e == hipErrorNotSupported) return false;
    if (e != hipSuccess) throw HipFail{e, "n2v2r_launch_ts_tn2"};
    if (h->comm) h->allreduce_f64(g2, 2 * (size_t)(nq_old + 2) * 64);
    // Za's selective pass (its R kept for the fix-up), then Zb's; each with its refill seed
    PipPass pa = selective_pass(any_p + 3, h->ews.pair_ra.as<double>()),
            pz = selective_pass(any_p + 3);
    pa.seed = next_fill_seed();
    pz.seed = next_fill_seed();
    pair_apply_launches(L, g2, n, pa, pz, pair_apply ? h->ews.pair_plan.as<int>() : nullptr,
                        h->ews.pair_plan.bytes, st);
    t_ortho += now_ms() - t0;
    deferred = nullptr;
    return true;
  }

  // blocks M Q[last] couples to: Q[last-1], Q[last]; for the first Krylov block of a cycle
  // (kry0: the start block, or the block E appended at a thick restart) every block before it
  // (the kept Ritz vectors X, whose residuals M X - X Theta lie in span(E))
  std::vector<float*> local_of(const std::vector<float*>& basis) const {
    const int last = (int)basis.size() - 1;
    const int lo = last <= kry0 ? 0 : last - 1;
    return std::vector<float*>(basis.begin() + lo, basis.end());
  }

  // offset of band column j (the local Gram of W_j) in the band store: column kry0 holds
  // [X E]^T W_E ((kry0 + 1) b x b), later ones [Q_{j-1} Q_j]^T W_j (2b x b)
  size_t band_off(int j) const {
    if (j == kry0) return 0;
    return (size_t)(kry0 * b + b) * b + (size_t)(j - kry0 - 1) * 2 * b * b;
  }

  // z = orth(W_from) against `basis`, w = M z; appended to (qs, ws).  save_band: W_from is the
  // image of the last basis block; keep its local Gram as a band column.
  void expand_one(const float* w_from, const std::vector<float*>& basis, std::vector<float*>& qs,
                  std::vector<float*>& ws, bool save_band = false, bool lazy = false) {
    float* z = take();
    const std::vector<float*> loc = local_of(basis);
    double* save = (save_band && band_rr)
                       ? h->ews.hband.as<double>() + band_off((int)basis.size() - 1)
                       : nullptr;
    if (defer && lazy && !full_first) {
      // local pass; then either this block waits (its full pass with the next one) or the
      // waiting block and this one get their full passes
      const double t0 = now_ms();
      lds_poison(st);
      const std::vector<float*>& first = first_blocks(basis, &loc);
      // a refill or heavy cancellation here sets the sticky flag: the block may not go to its
      // SpMM before its full pass, so the cycle is expanded again without deferral
      pip_pass(z, first, first_pass(first, &loc, save, any_p + 3, nullptr), w_from);
      t_ortho += now_ms() - t0;
      if (deferred && pair_pass(z, basis)) {
        // (both full passes done)
      } else if (deferred) {
        flush_deferred(basis);
        const double t1 = now_ms();
        pip_pass(z, basis, selective_pass(any_p + 3));
        t_ortho += now_ms() - t1;
      } else {
        deferred = z;
      }
    } else {
      orthonormalize(z, basis, w_from, &loc, save, lazy);  // reads W_from, writes z: no copy
    }
    dbg(z, n * b, false, "orthonormalised Krylov block");
    dbg_ortho(z, basis, "Krylov block before its SpMM");
    float* w = take();
    op.apply(z, w);
    if (debug_finite()) op.materialize();
    dbg(w, n * b, false, "SpMM image M q");
    ++dbg_apps;
    qs.push_back(z);
    ws.push_back(w);
  }

  // ---- set-up steps of a fit -----------------------------------------------------------------

  // reuse the workspace of the previous fit: every pool block is free again
  void reuse_pool() {
    const size_t bb = sizeof(float) * npad * b;
    if (h->ews.block_bytes != bb) {
      h->ews.pool.clear();
      h->ews.block_bytes = bb;
    }
    freelist.clear();
    for (auto& blk : h->ews.pool) freelist.push_back(blk->as<float>());
  }

  // every scratch buffer's size, and with them which Rayleigh-Ritz forms and images the fit has
  void size_scratch() {
    // chunk partials: also the streaming Gram form at b = 8 (chunks of <= 8192 rows, rounded to
    // a multiple of 8, (c + b) x b fp64 each) and the paired full passes' two-block Gram
    // (2 (c + 2b) x b per chunk; round 6: sized for one block's, the pair fell back to two
    // separate full passes past ~48 basis blocks at N = 10M -- 2 x 3.7 ms instead of one read)
    h->partial_elems = std::max<size_t>(4096ull * 1024ull, (size_t)c_max * c_max * 8);
    h->partial_elems = std::max<size_t>(h->partial_elems,
                                        (size_t)((n + 8191) / 8192 + 24) * 2 * (c_max + 2 * b) * b);
    h->partial.ensure(sizeof(double) * h->partial_elems);
    h->ews.gsmall.ensure(sizeof(double) * (size_t)c_max * c_max);
    h->ews.csmall.ensure(sizeof(float) * (size_t)c_max * c_max);
    h->ews.tri.ensure(sizeof(double) * 3 * (size_t)c_max);
    h->ews.refl.ensure(sizeof(double) * std::max<size_t>((size_t)c_max * c_max,
                                                        (size_t)c_max * (c_max / 8 + 2) * 9));
    h->ews.ytri.ensure(sizeof(double) * (size_t)c_max * keep);
    h->ews.tscr.ensure(sizeof(double) * 6 * (size_t)((keep + 63) / 64 * 64) * c_max);
    h->ews.trcoop.ensure(n2v2r_rr_tridiag_scratch_bytes(c_max));
    h->ews.btf.ensure(n2v2r_rr_bt_scratch_bytes(c_max));
    h->ews.rinv.ensure(sizeof(double) * 64 * 64);
    h->ews.fcoef.ensure(sizeof(float) * (size_t)(c_max + 64) * 64);
    h->ews.flg.ensure(sizeof(int) * 256);
    h->ews.anyflag.ensure(sizeof(int) * 4);
    h->theta.ensure(sizeof(double) * c_max);
    h->resid.ensure(sizeof(double) * c_max);
    // (kept sets past the reducing path's 192-row arrow, and bases past its 640 columns, take
    // the banded form only with the Sturm one, whose failure falls back to the dense
    // Rayleigh-Ritz on H expanded from the band)
    band_reduce = rr_reduce_fits(keep, c_max);
    band_rr = b == 8 && !flag(N2V2R_EIG_DENSE_RR) && c_max <= N2V2R_BAND_MAXC &&
              (band_reduce || rr_sturm_enabled());
    if (band_rr) {
      h->ews.hband.ensure(sizeof(double) * ((size_t)(keep + b) * b + (size_t)nb_max * 2 * b * b));
      h->ews.band.ensure(sizeof(double) * (size_t)c_max * (b + 1));
      h->ews.varr.ensure(sizeof(double) * (size_t)(keep + b) * (keep + b));
      h->ews.taua.ensure(sizeof(double) * (size_t)(keep + b));
      h->ews.rrerr.ensure(sizeof(int) * 4);
      h->ews.sturm.ensure(sizeof(double) * n2v2r_rr_sturm_scratch(c_max, keep));
    }
    sturm = band_rr && rr_sturm_enabled();
    part_p = h->partial.as<double>();
    part_n = h->partial_elems;
    gsm_p = h->ews.gsmall.as<double>();
    flg_p = h->ews.flg.as<int>();
    any_p = h->ews.anyflag.as<int>();
    // Lean images on a partitioned handle too: every quantity they read back (R of the restart
    // projection, the Ritz values and coefficients, the true residuals) is all-reduced first,
    // so every rank takes the same decisions.
    lean = b == 8 && band_rr && sturm && !lean_off && lean_enabled();
    h->ews.skipc.ensure(sizeof(int) * (4 + N2V2R_BAND_MAXC / 8));  // [0]: skipped, [1 + blk]
    HIPCHK(hipMemsetAsync(h->ews.skipc.p, 0, sizeof(int) * (4 + N2V2R_BAND_MAXC / 8), st));
    // R of the restart block's two passes
    if (lean) h->ews.rres.ensure(sizeof(double) * 128);
    rb.lay_out(keep);
    h->ews.dbgflag.ensure(sizeof(int) * 4);
    h->ews.tflag.ensure(sizeof(double) * 2);
    wh.assign(keep, 0.0);
    res2.assign(keep, 0.0);
  }

  // A plan without a fit (the diagnostic entries): block width, kept vectors and basis blocks as
  // given, the pool and the scratch as run() sets them up for that plan
  void set_plan(int b_, int keep_, int nblk) {
    b = b_;
    keep = keep_;
    pb = keep / b;
    nb_max = nblk;
    c_max = nblk * b;
    reuse_pool();
    size_scratch();
  }

  // the reorthogonalisation threshold and the deferral of full passes (needs `lean`)
  void read_reorth_switches() {
    // default: a tenth of the residual tolerance.  The residuals stall near the level of
    // orthogonality left in the basis (~1.5x it in cfg2 sweeps: 2e-6 stalls at 3e-6); at
    // 1e-7 .. 2.5e-7 cfg2 keeps its residuals and gains alike (most passes then touch only the
    // few blocks, the kept Ritz vectors, that lost orthogonality).  N2V2R_REORTH_TOL=0: every
    // block of every full pass.
    const char* rt = std::getenv("N2V2R_REORTH_TOL");
    // capped at 1e-6: a loose residual tolerance must not loosen the basis orthogonality the
    // Rayleigh-Ritz and the lean residual estimates assume
    reorth_tol = rt ? (float)std::atof(rt) : (float)std::min(0.1 * tol, 1e-6);
    // (the pass-level form -- all blocks or none -- gained less at the same threshold, 37.8 vs
    // 36.5 ms per cfg2 fit; its switch N2V2R_REORTH_MODE was retired in round 6)
    const char* e = std::getenv("N2V2R_REORTH_DEFER");  // read per fit (A/B runs)
    // lean images only: with every image kept, the Rayleigh-Ritz and the residuals read the
    // images themselves, and a deferred block's image is the uncorrected block's
    defer = !(e && e[0] == '0') && lean;
    deferred = nullptr;
    // a pair's two selective passes: fused (planned by one small launch, applied in one read
    // of the basis) from 2^19 rows on, where the second read of the basis costs more than the
    // serial plan launch (cfg4 against cfg2); below that split (three launches:
    // apply, fixup, apply -- also the fused form's reference and its fall-back).
    // Bit-identical fits.  N2V2R_PAIR_APPLY=fused / split forces one; read per fit (tests,
    // A/B runs)
    const char* pa = std::getenv("N2V2R_PAIR_APPLY");
    pair_apply = pa && std::strcmp(pa, "fused") == 0   ? true
                 : pa && std::strcmp(pa, "split") == 0 ? false
                                                       : n >= (int64_t)1 << 19;
    if (defer) {
      h->ews.g2.ensure(sizeof(double) * 2 * (size_t)(nb_max + 2) * 64, st);
      // R of the pair's first pass: the identity until a pass writes it
      static const double eye[64] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0,
                                     0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0,
                                     0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0,
                                     0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1};
      h->ews.pair_ra.ensure(sizeof(double) * 64, st);
      h->ews.pair_plan.ensure(sizeof(int) * N2V2R_PAIR_PLAN_WORDS, st);
      HIPCHK(hipMemcpyAsync(h->ews.pair_ra.p, eye, sizeof(eye), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  }

  // ---- steps of a cycle ------------------------------------------------------------------------

  static bool trace() {  // N2V2R_TRACE=1: stderr lines per Rayleigh-Ritz cycle
    static const bool v = [] {
      const char* e = std::getenv("N2V2R_TRACE");
      return e && *e && *e != '0';
    }();
    return v;
  }

  // One Rayleigh-Ritz of the basis Q (nq blocks) in the given form, all on the GPU, into the
  // fp32 Ritz coefficients S (c x keep, ld keep) and theta (kept in HBM until the read-back).
  //   banded: the band columns saved by the expansions (+ the last block's, computed here) ->
  //     Sturm: bisection -> band inverse iteration; BandReduce: arrow reduction + bulge chasing
  //     -> bisection -> inverse iteration;
  //   dense: H = Q^T W (fp64, all-reduced; DenseFromBand: expanded from the band columns) ->
  //     Householder tridiagonal -> bisection + inverse iteration on T -> compact-WY
  //     back-transform.
  // Returns the host clock at its start (N2V2R_TRACE).
  double launch_rr(RrForm form, int nq) {
    const int c = nq * b;
    double* trid = h->ews.tri.as<double>();
    op.materialize();  // W.back() (every other W block was stored by its expansion's Gram pass)
    const double tr0 = now_ms();
    lds_poison(st);
    if (banded(form)) {
      const std::vector<float*> loc = local_of(Q);
      tn(blocks(loc, 0, (int)loc.size()), one(W.back()),
         h->ews.hband.as<double>() + band_off(nq - 1), nullptr);
      if (!rr_armed) HIPCHK(hipMemsetAsync(h->ews.rrerr.as<int>(), 0, 4 * sizeof(int), st));
      rr_armed = true;  // from here on each read-back zeroes the words it reads
      lds_poison(st);
      if (form == RrForm::Sturm) {
        HIPCHK(n2v2r_launch_rr_sturm(h->ews.hband.as<double>(), c, kry0 * b,
                                     h->theta.as<double>(), h->ews.sturm.as<double>(),
                                     h->ews.sturm.bytes / sizeof(double),
                                     h->ews.ytri.as<double>(), h->ews.csmall.as<float>(), keep,
                                     keep, h->ews.rrerr.as<int>(), st));
      } else {
        HIPCHK(n2v2r_launch_rr_band(h->ews.hband.as<double>(), c, kry0 * b, h->theta.as<double>(),
                                    h->ews.band.as<double>(), h->ews.varr.as<double>(),
                                    h->ews.taua.as<double>(), trid, trid + c_max,
                                    h->ews.refl.as<double>(), h->ews.ytri.as<double>(),
                                    h->ews.csmall.as<float>(), keep, keep,
                                    h->ews.rrerr.as<int>(), st));
      }
    } else {
      if (form == RrForm::DenseFromBand) {
        // the kept Ritz values: the copy the Sturm assembly made (h->theta is overwritten by the
        // dense steps below, and a retry of this form must read what its first attempt read)
        HIPCHK(n2v2r_launch_rr_band_expand(h->ews.hband.as<double>(), c, kry0 * b,
                                           h->ews.sturm.as<double>() + 4,
                                           h->ews.gsmall.as<double>(), st));
      } else {
        tn(blocks(Q, 0, nq), blocks(W, 0, nq), h->ews.gsmall.as<double>(), nullptr);
      }
      dbg(h->ews.gsmall.p, (int64_t)c * c, true, "projected matrix H = Q^T W");
      lds_poison(st);
      // ranks that share this device (thread group): their concurrent launches of the
      // multi-workgroup form could not all be resident, so they keep the one-workgroup kernel;
      // so does a fit whose multi-workgroup launch once timed out (tri_err, rr_next)
      const bool shared_device = h->comm && h->comm->shares_device();
      const bool coop = !shared_device && !tri_single;
      tri_err = coop ? n2v2r_rr_tridiag_err(h->ews.trcoop.p, c) : nullptr;
      HIPCHK(n2v2r_launch_rr_tridiag(h->ews.gsmall.as<double>(), c, trid, trid + c_max,
                                     trid + 2 * c_max, h->ews.refl.as<double>(),
                                     coop ? h->ews.trcoop.p : nullptr, st));
      dbg(trid, c, true, "tridiagonal diagonal");
      dbg(trid + c_max, c - 1, true, "tridiagonal off-diagonal");
      lds_poison(st);
      HIPCHK(n2v2r_launch_rr_tri_eig(trid, trid + c_max, c, keep, h->theta.as<double>(),
                                     h->ews.ytri.as<double>(), h->ews.tscr.as<double>(), st));
      dbg(h->theta.p, keep, true, "tridiagonal eigenvalues (bisection)");
      dbg(h->ews.ytri.p, (int64_t)c * keep, true, "tridiagonal eigenvectors");
      lds_poison(st);
      HIPCHK(n2v2r_launch_rr_backtransform(h->ews.refl.as<double>(), trid + 2 * c_max, c,
                                           h->ews.ytri.as<double>(), keep,
                                           h->ews.csmall.as<float>(), keep,
                                           h->ews.btf.as<double>(), st));
    }
    dbg(h->theta.p, keep, true, "Ritz values");
    dbg(h->ews.csmall.p, (int64_t)c * keep, false, "Ritz coefficients S");
    t_rr += now_ms() - tr0;
    return tr0;
  }

  // Ritz vectors X = Q S, MX = W S (keep columns, pb blocks; lean images: X only)
  void ritz_vectors(int nq) {
    lds_poison(st);
    const int per_launch = std::max(1, 128 / b);  // output blocks per ts_nn launch (<= 128 cols)
    ritz_done = false;
    ritz_launches = 0;
    if (b == 8 && keep <= 96) {
      // both products in one launch (ritz_nn_kernel), the coefficients staged once per CU
      OutBlockList ox{}, omx{};
      ox.width = omx.width = b;
      ox.count = omx.count = pb;
      for (int t = 0; t < pb; ++t) {
        ox.blk[t] = X[t];
        omx.blk[t] = MX[t];
      }
      if (lean) omx.count = 0;  // X only
      const hipError_t e = n2v2r_launch_ritz_nn(blocks(Q, 0, nq), lean ? one(nullptr) : blocks(W, 0, nq),
                                                h->ews.csmall.as<float>(), keep, keep, ox, omx,
                                                n, 0, st);
      if (e == hipSuccess) ritz_done = true;
      else if (e != hipErrorNotSupported) throw HipFail{e, "n2v2r_launch_ritz_nn"};
      ritz_launches = ritz_done ? 1 : 0;
    }
    for (int q0b = 0; !ritz_done && q0b < pb; q0b += per_launch) {
      const int nt = std::min(per_launch, pb - q0b);
      OutBlockList ox{}, omx{};
      ox.width = omx.width = b;
      ox.count = omx.count = nt;
      for (int t = 0; t < nt; ++t) {
        ox.blk[t] = X[q0b + t];
        omx.blk[t] = MX[q0b + t];
      }
      // G slice: columns [q0b*b, q0b*b + nt*b) of S (ld = keep)
      const float* g = h->ews.csmall.as<float>() + q0b * b;
      HIPCHK(n2v2r_launch_ts_nn(blocks(Q, 0, nq), g, keep, nt * b, ox, one(nullptr), 1.f, 0.f, n,
                                st));
      if (!lean)
        HIPCHK(n2v2r_launch_ts_nn(blocks(W, 0, nq), g, keep, nt * b, omx, one(nullptr), 1.f, 0.f,
                                  n, st));
      ritz_launches += lean ? 1 : 2;
    }
    for (int q = 0; q < pb; ++q) {
      dbg(X[q], n * b, false, "Ritz vectors X = Q S");
      if (!lean) dbg(MX[q], n * b, false, "Ritz images MX = W S");
    }
  }

  // what the residuals are read from.  Lean images: the restart block (it needs nothing from the
  // Rayleigh-Ritz stage) -- its first, local pass leaves R with W_last - Q_loc C = Z_{m+1} R,
  // Z_{m+1} orthonormal; built once per cycle, a Rayleigh-Ritz retry reuses it and R.  Else the
  // true residuals ||MX_j - theta_j X_j||^2.
  void launch_residuals() {
    if (lean) {
      if (E_lean) return;
      E_lean = take();
      const std::vector<float*> loc = local_of(Q);
      orthonormalize(E_lean, Q, W.back(), &loc, nullptr, false, h->ews.rres.as<double>());
      return;
    }
    HIPCHK(n2v2r_launch_resid(blocks(X, 0, pb), blocks(MX, 0, pb), h->theta.as<double>(), n,
                              h->partial.as<double>(), h->partial_elems, h->resid.as<double>(),
                              st));
    h->allreduce_f64(h->resid.as<double>(), keep);
  }

  // the cycle's one host synchronisation: one pack launch + one copy into the pinned buffer
  // (the layout of ReadBack).  The sticky refill flag and the Rayleigh-Ritz error words are
  // zeroed as they are read: armed for the next cycle (or a retry) without a memset.
  void read_back(RrForm form, int c, double tr0) {
    h->ensure_pin(rb.bytes(rb.words));
    h->ews.rback.ensure(rb.bytes(rb.words));
    void* src[12];
    int dw[12], nw[12], clr[12], ns = 0;
    auto seg = [&](void* sp, int d0, int n0, int cl = 0) {
      src[ns] = sp;
      dw[ns] = d0;
      nw[ns] = n0;
      clr[ns] = cl;
      ++ns;
    };
    if (lean) {
      seg(h->ews.rres.p, rb.wrr, 2 * ReadBack::nrr);
      seg(h->ews.csmall.as<float>() + (size_t)(c - b) * keep, rb.wsl, ReadBack::nsl * keep);
    } else {
      seg(h->resid.p, rb.wres, 2 * keep);
    }
    seg(h->theta.p, rb.wth, 2 * keep);
    seg(nullptr, rb.wflag, 1);
    if (lazy) seg(h->ews.anyflag.as<int>() + 3, rb.wflag + ReadBack::kRefilled, 1, 1);
    else seg(nullptr, rb.wflag + ReadBack::kRefilled, 1);
    if (banded(form)) seg(h->ews.rrerr.p, rb.wflag + ReadBack::kRrErr, 2, 1);  // + kSecondSolves
    else seg(nullptr, rb.wflag + ReadBack::kRrErr, 2);
    seg(banded(form) ? nullptr : tri_err, rb.wflag + ReadBack::kTriErr, 1);
    HIPCHK(n2v2r_launch_pack_words(src, dw, nw, clr, ns, h->ews.rback.p, st));
    const size_t upto = rb.bytes(lean ? rb.words : rb.wflag + 8);
    HIPCHK(hipMemcpyAsync(h->pin, h->ews.rback.p, upto, hipMemcpyDeviceToHost, st));
    const double th_sync0 = now_ms();
    HIPCHK(hipStreamSynchronize(st));
    if (trace())
      fprintf(stderr, "[n2v2r] cycle %d host: rr start %.3f, to sync %.3f, sync %.3f ms\n",
              cycle, tr0 - t_start, th_sync0 - tr0, now_ms() - th_sync0);
  }

  // the read-back's Ritz values into wh and squared residuals into res2.  Lean images:
  // ||M x_j - theta_j x_j||^2 = ||R s_j(last block)||^2 (Krylov-Schur), scaled
  void read_estimates() {
    const double* pth = rb.at<double>(h->pin, rb.wth);
    if (lean) {
      const double* prr = rb.at<double>(h->pin, rb.wrr);
      const float* psl = rb.at<float>(h->pin, rb.wsl);
      for (int j = 0; j < keep; ++j) {
        double acc = 0.0;
        for (int r = 0; r < 8; ++r) {
          double v = 0.0;
          for (int cc = r; cc < 8; ++cc) v += prr[r * 8 + cc] * (double)psl[cc * keep + j];
          acc += v * v;
        }
        res2[j] = acc * est_scale * est_scale;
      }
    } else {
      const double* pres = rb.at<double>(h->pin, rb.wres);
      std::copy(pres, pres + keep, res2.begin());
    }
    std::copy(pth, pth + keep, wh.begin());
  }

  // What the read-back's error words say of the Rayleigh-Ritz just run: nothing (its result
  // stands), or the form to run next on the same basis; under lean images the dense H = Q^T W
  // cannot be formed (it needs every image), so LeanRetry.
  std::optional<RrForm> rr_next(RrForm form, int c) {
    const int* pflag = rb.at<int>(h->pin, rb.wflag);
    if (!banded(form)) {
      bool timed_out = pflag[ReadBack::kTriErr] != 0;
      if (tri_test_armed && tri_err && !tri_single) {  // tests: a good result discarded
        timed_out = true;
        tri_test_armed = false;
      }
      if (h->comm) {
        // each rank read its own device's error word: agree on it (max over ranks) before
        // branching, so every rank redoes the step together (a rank that alone ran it again
        // would run one more all-reduce of H than its peers)
        double* fl = h->ews.tflag.as<double>();
        const double mine = timed_out ? 1.0 : 0.0;
        HIPCHK(hipMemcpyAsync(fl, &mine, sizeof(double), hipMemcpyHostToDevice, st));
        h->allreduce_f64(fl, 1);
        double any_to = 0.0;
        HIPCHK(hipMemcpyAsync(&any_to, fl, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        timed_out = any_to > 0.0;
      }
      if (!timed_out) return std::nullopt;
      // the multi-workgroup tridiagonalisation's grid barrier timed out (a workgroup was not
      // resident): its output is invalid; this cycle's Rayleigh-Ritz again, and every later
      // one, with the one-workgroup kernel
      fprintf(stderr, "[n2v2r] multi-workgroup tridiagonalisation timed out at cycle %d (c %d); "
                      "one-workgroup kernel from here on\n", cycle, c);
      tri_single = true;
      ++tri_fallbacks;
      return form;
    }
    const bool failed = pflag[ReadBack::kRrErr] != 0 || flag(N2V2R_EIG_TEST_BAND_FAIL) ||
                        (flag(N2V2R_EIG_TEST_STURM_FAIL) && form == RrForm::Sturm);
    if (form == RrForm::Sturm) {
      if (trace())
        fprintf(stderr, "[n2v2r] cycle %d: %d of %d Ritz vectors took a second solve\n", cycle,
                pflag[ReadBack::kSecondSolves], keep);
      if (!failed) return std::nullopt;
      // a Sturm vector failed its residual check
      if (trace()) fprintf(stderr, "[n2v2r] Sturm Rayleigh-Ritz failed, reducing fallback\n");
      ++stats_rr_fallbacks;
      const RrForm next = rr_after_sturm(keep, c_max);
      if (next == RrForm::DenseFromBand) return next;  // past the reducing path's arrow
      // the kept Ritz values the reducing path reads: the copy the Sturm assembly made
      if (kry0 > 0)
        HIPCHK(hipMemcpyAsync(h->theta.as<double>(), h->ews.sturm.as<double>() + 4,
                              sizeof(double) * kry0 * b, hipMemcpyDeviceToDevice, st));
      return RrForm::BandReduce;
    }
    if (!failed) return std::nullopt;
    if (lean) throw LeanRetry{};
    // the bulge chase gave up (should not happen)
    if (trace()) fprintf(stderr, "[n2v2r] banded Rayleigh-Ritz failed, dense fallback\n");
    return RrForm::Dense;
  }

  // the first Ritz pair with a non-finite value or (among the d wanted) residual; -1: none
  int nonfinite_pair() const {
    for (int j = 0; j < keep; ++j)
      if (!std::isfinite(wh[j]) || (j < d && !std::isfinite(res2[j]))) return j;
    return -1;
  }

  // give back the cycle's Ritz blocks and the basis blocks from q_start on
  void drop_cycle(int q_start) {
    const int nq = (int)Q.size();
    give(E_lean);
    for (int q = 0; q < pb; ++q) {
      give(X[q]);
      give(MX[q]);
    }
    for (int q = q_start; q < nq; ++q) {
      give(Q[q]);
      give(W[q]);
    }
    apps -= nq - q_start;
    Q.resize(q_start);
    W.resize(q_start);
  }

  // fp32 noise floor: the true residual of W = M Q cannot fall below ~eps32 * sqrt(nnz/row) *
  // theta_1.  Stop when the best worst-residual of the last 8 cycles is not 10% below the best
  // one before them (slow but steady convergence on clustered spectra keeps going) and it is
  // within 100x of tol.
  bool residuals_flat() {
    hist_res.push_back(maxres);
    const size_t W8 = 8;
    if (hist_res.size() < 2 * W8) return false;
    const double recent = *std::min_element(hist_res.end() - W8, hist_res.end());
    const double before = *std::min_element(hist_res.begin(), hist_res.end() - W8);
    return !flag(N2V2R_EIG_TEST_NO_STAGNATION) && recent > 0.9 * before && recent <= 100.0 * tol;
  }

  // lean images: the estimates say stop; the true residuals of the d wanted vectors (their
  // images by SpMM) decide.  Sets maxres, conv and stagnated from them; false: the fit goes on.
  bool lean_final_check(double th1, int ldu) {
    ++lean_checks;
    const int qd = (d + b - 1) / b;
    std::vector<float*> MV(qd);
    // one GPU, tiled SpMM, every column of the embedding covered: keep the stage-1 products
    // (N2V2R_YCAP=0, read per fit: the embedding step computes its SpMM launches; A/B, tests)
    const char* ycv = std::getenv("N2V2R_YCAP");
    const bool cap = op.col_blocks && !h->comm && b == 8 && qd * b == ldu &&
                     !(ycv && ycv[0] == '0');
    if (cap) h->Y.ensure(sizeof(float) * (size_t)K * npad * ldu, st);
    for (int q = 0; q < qd; ++q) {
      MV[q] = take();
      op.apply(X[q], MV[q]);
      op.materialize();
      if (cap)
        for (int k = 0; k < K; ++k)
          HIPCHK(hipMemcpy2DAsync(h->Y.as<float>() + (size_t)k * npad * ldu + (size_t)q * b,
                                  sizeof(float) * ldu, op.zk(k),
                                  sizeof(float) * b, sizeof(float) * b, n,
                                  hipMemcpyDeviceToDevice, st));
    }
    y_captured = cap;
    double* pres = rb.at<double>(h->pin, rb.wres);
    HIPCHK(n2v2r_launch_resid(blocks(X, 0, qd), blocks(MV, 0, qd), h->theta.as<double>(), n,
                              h->partial.as<double>(), h->partial_elems,
                              h->resid.as<double>(), st));
    h->allreduce_f64(h->resid.as<double>(), (size_t)qd * b);
    HIPCHK(hipMemcpyAsync(pres, h->resid.as<double>(), sizeof(double) * qd * b,
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (float* p : MV) give(p);
    double worst = 0.0, est_max = 0.0;
    int tconv = 0;
    for (int j = 0; j < d; ++j) {
      const double r = std::sqrt(std::max(pres[j], 0.0)) / th1;
      const double e = std::sqrt(std::max(res2[j], 0.0)) / th1;
      worst = std::max(worst, r);
      est_max = std::max(est_max, e);
      if (r <= tol) ++tconv;
    }
    // the scale that brings the worst estimate to the worst true residual (a ratio taken
    // vector by vector blew up on estimates at the fp32 noise level: 1e-12 against a true
    // 1e-7 gave a scale of 1e5, and the scaled estimates never came back below tol)
    const double ratio = est_max > 0.0 ? worst / est_max : 0.0;
    if (trace())
      fprintf(stderr, "[n2v2r] cycle %d: true max_res %.3e converged %d/%d (estimate %.3e)\n",
              cycle, worst, tconv, d, maxres);
    maxres = worst;
    conv = tconv;
    stagnated = 0;
    bool done = true;
    if (conv < d && cycle + 1 < max_restarts) {
      // at the fp32 floor the true residual stops falling: finish within 100x tol once a
      // check shows no 10 % gain over the previous one (or after 4 checks)
      const bool flat = lean_checks >= 2 && worst > 0.9 * last_true;
      if (!flag(N2V2R_EIG_TEST_NO_STAGNATION) && (flat || lean_checks >= 4) &&
          worst <= 100.0 * tol) {
        stagnated = 1;
      } else {
        done = false;
        // the estimates (already scaled) trail the true residual by `ratio`: rescale from
        // this check (it may also shrink back towards 1 after a pessimistic one), at most
        // by 1e3 in all
        if (ratio > 0.0) est_scale = std::min(1e3, std::max(1.0, est_scale * 1.25 * ratio));
        hist_res.clear();
      }
    }
    last_true = worst;
    return done;
  }

  // thick restart: the basis becomes [X | orth(W_last) against the old basis]
  void restart() {
    std::vector<float*> E, EW;
    if (lean) {
      E.push_back(E_lean);
      EW.push_back(take());
      op.apply(E_lean, EW[0]);
    } else {
      expand_one(W.back(), Q, E, EW);
    }
    ++apps;
    for (float* p : Q) give(p);
    for (float* p : W) give(p);
    Q.assign(X.begin(), X.end());
    W.assign(MX.begin(), MX.end());
    Q.insert(Q.end(), E.begin(), E.end());
    W.insert(W.end(), EW.begin(), EW.end());
    kry0 = pb;
  }

  void fill_stats() {
    if (!stats) return;
    stats->restarts = cycle + 1;
    stats->block_applications = apps;
    stats->converged = conv;
    stats->basis = c_max;
    stats->max_residual = maxres;
    stats->ms_total = now_ms() - t_start;
    stats->ms_spmm = op.t_spmm;
    stats->ms_ortho = t_ortho;
    stats->ms_rr_host = t_rr;
    stats->spmm_launches = op.launches;
    stats->spmm_algo_bytes = op.algo_bytes;
    stats->stagnated = stagnated;
    stats->rr_fallbacks = stats_rr_fallbacks;
    stats->est_scale = est_scale;
    stats->lean_checks = lean_checks;
    stats->pool_blocks = (int)h->ews.pool.size();
    stats->spmm_form = op.spmm_form();
    stats->stag_cap = stag_cap;
    stats->y_captured = y_captured ? 1 : 0;
    stats->tri_fallbacks = tri_fallbacks;
    op.tsum(stats);
  }

  int run(int d_, const n2v2r_eig_opts& o, std::vector<double>& theta_out, float* Uout,
          int ldu) {
    d = d_;
    seed = o.seed ? o.seed : 0x5EEDull;
    flags = o.solver_flags;
    full_first = flag(N2V2R_EIG_FULL_FIRST_PASS);
    tri_test_armed = flag(N2V2R_EIG_TEST_TRI_TIMEOUT);
    kry0 = 0;
    tol = o.tol > 0 ? o.tol : 1e-6;
    max_restarts = o.max_restarts > 0 ? o.max_restarts : 2000;
    const BasisPlan plan = plan_basis(d, h->n, o.block, o.keep, o.max_basis,
                                      flag(N2V2R_EIG_DENSE_RR), h->dense_layers());
    b = plan.b;
    keep = plan.keep;
    c_max = plan.maxc;
    pb = keep / b;
    nb_max = c_max / b;
    // A fit that stops because its residuals went flat (the fp32 floor) is a success only within
    // stag_cap.  The floor: a Ritz vector X = Q S is assembled in fp32 from c basis columns, so
    // its entries carry ~sqrt(c) 2^-24 relative rounding, and ||M x - theta x|| / theta_1 cannot
    // fall much below that (1.35e-6 at c = 512; the cfg4-grid fixture's last column stops at
    // 1.28e-6, its host fp64 residual agrees, and 12 more cycles do not lower it:
    // tests/test_gpu_configs.py::test_cfg4_grid_vs_reference).  Past the cap the fit returns
    // N2V2R_ERR_NO_CONVERGENCE.
    stag_cap = 2.0 * std::max(tol, std::sqrt((double)c_max) * 0x1p-24);
    reuse_pool();
    op.setup(b, flag(N2V2R_EIG_TIME_SPMM));
    size_scratch();
    read_reorth_switches();
    poison_scratch();

    // start block (counter-based: the same values whatever the row partition)
    float* q0 = take();
    HIPCHK(n2v2r_launch_fill_normal(q0, b, n, seed, nullptr, nullptr, (uint64_t)row0 * b, st));
    Q.assign(1, q0);
    orthonormalize(q0, {});
    dbg(q0, n * b, false, "orthonormalised start block");
    W.assign(1, take());
    op.apply(Q[0], W[0]);
    if (debug_finite()) op.materialize();
    dbg(W[0], n * b, false, "SpMM image of the start block");
    if (flag(N2V2R_EIG_TEST_FAIL_ALONE) && h->comm && h->rank == 1)
      throw StatusFail{N2V2R_ERR_INTERNAL, "test: rank 1 fails alone"};
    apps = 1;
    X.assign(pb, nullptr);
    MX.assign(pb, nullptr);
    t_start = now_ms();
    for (cycle = 0;; ++cycle) {
      dbg_cycle = cycle;
      y_captured = false;
      // expand the basis to nb_max blocks
      const int q_start = (int)Q.size();
      // (cycle 0: armed here; later cycles: the previous cycle's read-back zeroed it)
      if (lazy && cycle == 0) HIPCHK(hipMemsetAsync(h->ews.anyflag.as<int>() + 3, 0, sizeof(int), st));
      while ((int)Q.size() < nb_max) {
        expand_one(W.back(), Q, Q, W, /*save_band=*/true, lazy);
        ++apps;
        if (lean && (int)W.size() - 2 > q_start - 1) {  // consumed; the cycle's input stays
          give(W[W.size() - 2]);
          W[W.size() - 2] = nullptr;
        }
      }
      flush_deferred(Q);  // (deferred full passes) the cycle's last block
      const int nq = (int)Q.size();
      const int c = nq * b;
      for (int q = 0; q < pb; ++q) {
        X[q] = take();
        MX[q] = lean ? nullptr : take();
      }
      E_lean = nullptr;
      // Rayleigh-Ritz, Ritz vectors and the read-back, until a form's result stands
      RrForm form = !band_rr ? RrForm::Dense : sturm ? RrForm::Sturm : RrForm::BandReduce;
      for (;;) {
        const double tr0 = launch_rr(form, nq);
        const double to0 = now_ms();
        ritz_vectors(nq);
        launch_residuals();
        read_back(form, c, tr0);
        read_estimates();
        t_ortho += now_ms() - to0;
        const std::optional<RrForm> next = rr_next(form, c);
        if (!next) break;
        form = *next;
      }
      int refilled = lazy ? rb.at<int>(h->pin, rb.wflag)[ReadBack::kRefilled] : 0;
      if (flag(N2V2R_EIG_TEST_REDO_CYCLE) && cycle == 0 && lazy) refilled = 1;  // tests
      // a non-finite Ritz pair under the lazy (two-pass) orthogonalisation: diagnostic
      // fallback only (no known cause remains; N2V2R_DEBUG_FINITE=1 names the first stage that
      // produces one).  Always reported on stderr, then the cycle's expansion is redone with
      // three passes from the kept (finite) basis before giving up below.
      const int bad = nonfinite_pair();
      if (lazy && !refilled && bad >= 0) {
        fprintf(stderr,
                "[n2v2r] WARNING: non-finite Ritz pair %d at cycle %d (c %d, b %d, %s "
                "Rayleigh-Ritz); cycle expanded again with three passes.  Rerun with "
                "N2V2R_DEBUG_FINITE=1 to locate the stage.\n",
                bad, cycle, c, b, banded(form) ? "banded" : "dense");
        refilled = 1;
      }
      if (refilled) {  // a second pass refilled a column: expand this cycle again, 3 passes
        if (trace()) fprintf(stderr, "[n2v2r] rank-deficient block, cycle %d expanded again\n", cycle);
        drop_cycle(q_start);
        lazy = false;
        --cycle;
        continue;
      }
      if (bad >= 0)  // a non-finite Ritz pair cannot recover: stop with details
        throw StatusFail{N2V2R_ERR_NO_CONVERGENCE,
                         "non-finite Ritz pair " + std::to_string(bad) + " at cycle " +
                             std::to_string(cycle) + " (c " + std::to_string(c) + ", b " +
                             std::to_string(b) + (banded(form) ? ", banded" : ", dense") +
                             " Rayleigh-Ritz, theta " + std::to_string(wh[bad]) + ")"};
      maxres = 0;
      conv = 0;
      const double th1 = std::max(wh[0], 1e-300);
      for (int j = 0; j < d; ++j) {
        const double r = std::sqrt(std::max(res2[j], 0.0)) / th1;
        maxres = std::max(maxres, r);
        if (r <= tol) ++conv;
      }
      if (trace())
        fprintf(stderr, "[n2v2r] rank %d cycle %d apps %d c %d max_res %.3e converged %d/%d %.1f ms\n",
                h->rank, cycle, apps, c, maxres, conv, d, now_ms() - t_start);
      bool done = conv == d || cycle + 1 >= max_restarts;
      if (!done && residuals_flat()) {
        stagnated = 1;
        done = true;
      }
      if (lean && done) done = lean_final_check(th1, ldu);
      if (done) {
        give(E_lean);
        break;
      }
      restart();
    }
    op.materialize();
    if (trace() && reorth_tol != 0.f) {
      int sk[65] = {};
      HIPCHK(hipMemcpyAsync(sk, h->ews.skipc.p, sizeof(int) * 65, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      fprintf(stderr, "[n2v2r] %d full reorthogonalisation passes skipped (tol %.1e); applied "
              "per basis block:", sk[0], (double)reorth_tol);
      for (int q = 0; q < 64; ++q) fprintf(stderr, " %d", sk[1 + q]);
      fprintf(stderr, "\n");
    }
    // U = first d columns of X (row stride ldu); theta
    theta_out.assign(wh.begin(), wh.begin() + d);
    for (int q = 0; q * b < d; ++q) {
      const int cols = std::min(b, d - q * b);
      HIPCHK(hipMemcpy2DAsync(Uout + q * b, sizeof(float) * ldu, X[q], sizeof(float) * b,
                              sizeof(float) * cols, npad, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    fill_stats();
    return (conv == d || (stagnated && maxres <= stag_cap)) ? N2V2R_OK : N2V2R_ERR_NO_CONVERGENCE;
  }
};

// layer k's local rows (nloc x d, the embedding's first d of its ldy columns) to Y + k * stride
void copy_embedding(n2v2r_handle* h, float* Y, int64_t layer_stride) {
  HIPCHK(hipSetDevice(h->device));
  for (int k = 0; k < h->K; ++k)
    HIPCHK(hipMemcpy2DAsync(Y + (size_t)k * layer_stride, sizeof(float) * h->d,
                            h->Y.as<float>() + (size_t)k * h->npad * h->ldy,
                            sizeof(float) * h->ldy, sizeof(float) * h->d, h->nloc,
                            hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
}

// The embedding of a finished fit from its left vectors U (h->U, ld ldu) and Ritz values theta:
// deterministic signs, sigma = sqrt(theta), and Y_k = A_k^T U sigma^(-1/2) into h->Y -- the
// products the final lean check captured (`captured`), the fit's tiled SpMM, or the row kernel /
// the dense GEMM.  info (n2v2r_embed_step): what was launched, by the launchers' own rules.
static void build_embedding(n2v2r_handle* h, const GramOp& op, const std::vector<double>& theta,
                            int ldu, bool captured, n2v2r_embed_info* info = nullptr) {
  const int d = (int)theta.size(), b = op.b;
  const bool tiled = op.col_blocks;  // (b = 8 then)
  if (info) {
    *info = n2v2r_embed_info{};
    info->form = h->dense_layers() ? 4 : tiled ? 5 : 0;
    info->ldu = ldu;
    HIPCHK(n2v2r_colmax_plan(h->nloc, d, 1024 * (size_t)ldu, &info->colmax_chunks,
                             &info->colmax_rows));
  }
  // deterministic signs: largest-magnitude entry of every column of U positive
  h->keys.ensure(sizeof(unsigned long long) * 1024 * (size_t)ldu);
  h->best.ensure(sizeof(unsigned long long) * ldu);
  h->colscale.ensure(sizeof(float) * ldu);
  HIPCHK(n2v2r_launch_colmax_keys(h->U.as<float>(), ldu, h->nloc, d, h->row0,
                                  h->keys.as<unsigned long long>(), 1024 * (size_t)ldu,
                                  h->best.as<unsigned long long>(), h->stream));
  if (h->comm)
    h->comm->allreduce_max_u64(h->best.as<unsigned long long>(), ldu, h->stream);
  HIPCHK(n2v2r_launch_colmax_sign(h->best.as<unsigned long long>(), ldu, h->U.as<float>(), ldu, d,
                                  h->row0, h->nloc, h->colscale.as<float>(), h->stream));
  if (h->comm)
    h->comm->allreduce_sum_f32(h->colscale.as<float>(), ldu, h->stream);
  HIPCHK(n2v2r_launch_scale_cols(h->U.as<float>(), ldu, h->npad, h->colscale.as<float>(),
                                 h->stream));
  // Y_k = A_k^T U diag(theta)^(-1/4)  (sigma = sqrt(theta); V sqrt(sigma) = A^T U sigma^-1/2)
  h->d = d;
  h->ldy = ldu;
  h->sigma.assign(d, 0.0);
  std::vector<float> sc(ldu, 0.f);
  for (int j = 0; j < d; ++j) {
    h->sigma[j] = std::sqrt(std::max(theta[j], 0.0));
    sc[j] = h->sigma[j] > 0 ? (float)(1.0 / std::sqrt(h->sigma[j])) : 0.f;
  }
  if (captured) {
    // the captured A_k^T X come from the Ritz vectors before the sign pass: fold each column's
    // sign (+-1, exact) into its scale
    std::vector<float> sgn(ldu, 1.f);
    HIPCHK(hipMemcpyAsync(sgn.data(), h->colscale.p, sizeof(float) * ldu, hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int j = 0; j < d; ++j) sc[j] *= sgn[j];
  }
  HIPCHK(hipMemcpyAsync(h->colscale.p, sc.data(), sizeof(float) * ldu, hipMemcpyHostToDevice,
                        h->stream));
  const float* ug = h->U.as<float>();
  DevBuf ugath;
  if (h->comm) {
    ugath.ensure(sizeof(float) * h->world * h->npad * ldu);
    h->gather_panel(h->U.as<float>(), ugath.as<float>(), ldu);
    ug = ugath.as<float>();
  }
  h->Y.ensure(sizeof(float) * (size_t)h->K * h->npad * ldu);
  if (h->dense_layers()) {
    for (int k = 0; k < h->K; ++k) {
      const LayerDev& L = *h->layers[k];
      // one GEMM per layer over all ldu columns (ldu <= 256: 64-column slices)
      for (int q = 0; q * 64 < ldu; ++q)
        h->dense_apply(L.dense_at(), L.lda, ug + q * 64, ldu, std::min(64, ldu - q * 64),
                       h->Y.as<float>() + (size_t)k * h->npad * ldu + q * 64, ldu, 0.f,
                       h->colscale.as<float>() + q * 64);
      if (info) info->launches += (ldu + 63) / 64;
    }
  }
  if (!h->dense_layers() && tiled) {
    // the fit's tiled SpMM (stage-1 blocks, A_k^T) on b-column slices of U copied to a
    // contiguous panel, then one column scaling of every Y_k (the row kernel below gathers
    // 32 B out of each 512-B row of U -- a 512 MB panel at cfg4 -- and scales in-kernel)
    const int64_t ng = h->comm ? (int64_t)h->world * h->npad : h->npad;
    DevBuf& panel = h->ypanel;
    panel.ensure_raw(sizeof(float) * ng * 8);
    SpmmTileArgs a = op.tile_args(false, 0, h->K, 0, ldu);
    for (int q = 0; !captured && q * 8 < ldu; ++q) {
      HIPCHK(hipMemcpy2DAsync(panel.p, sizeof(float) * 8, ug + q * 8, sizeof(float) * ldu,
                              sizeof(float) * 8, ng, hipMemcpyDeviceToDevice, h->stream));
      for (int k = 0; k < h->K; ++k) {
        a.X[k] = panel.as<float>();
        a.Y[k] = h->Y.as<float>() + (size_t)k * h->npad * ldu + q * 8;
      }
      HIPCHK(n2v2r_launch_spmm_tile(a, h->stream));
      if (info) ++info->launches;
    }
    for (int k = 0; k < h->K; ++k)
      HIPCHK(n2v2r_launch_scale_cols(h->Y.as<float>() + (size_t)k * h->npad * ldu, ldu,
                                     h->npad, h->colscale.as<float>(), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // the panel dies here
  }
  for (int q = 0; !h->dense_layers() && !tiled && q * b < ldu; ++q) {
    SpmmArgs a{};
    a.K = h->K;
    a.sum = 0;
    a.ldx = ldu;
    a.ldy = ldu;
    a.colscale = h->colscale.as<float>() + q * b;
    for (int k = 0; k < h->K; ++k) {
      a.A[k] = h->layers[k]->csr_t();
      a.X[k] = ug + q * b;
      a.Y[k] = h->Y.as<float>() + (size_t)k * h->npad * ldu + q * b;
    }
    HIPCHK(n2v2r_launch_spmm(a, b, h->stream));
    if (info) {
      ++info->launches;
      info->rpw = n2v2r_spmm_rpw(a, b);
    }
  }
  HIPCHK(hipStreamSynchronize(h->stream));
}
}  // namespace n2v2r_int

extern "C" {

int n2v2r_uase(n2v2r_handle* h, int d, const n2v2r_eig_opts* opts, n2v2r_eig_stats* stats) {
  if (h && h->multi()) return multi_uase(h, d, opts, stats);
  return guarded(h, [&]() -> int {
    if (!layers_ready(h)) return N2V2R_ERR_BAD_ARG;
    // d <= 600: the kept Ritz vectors (max(d + 16, 5 d / 4)) plus one block must fit the
    // Rayleigh-Ritz kernels' 768-column basis
    if (d < 1 || d > 600 || d >= h->n) {
      h->set_err("embedding dimension %d out of range [1, min(600, n-1)]", d);
      return N2V2R_ERR_BAD_ARG;
    }
    n2v2r_eig_opts o{};
    if (opts) o = *opts;
    if (stats) memset(stats, 0, sizeof(*stats));
    // a fit that fails part-way must not leave a stale embedding (U, Y and the capture below are
    // rewritten from here on) or stale ranking results readable
    h->have_embedding = false;
    h->ncmp = h->ncols = 0;
    h->have_borda = false;
    // the ingest's radix scratch (~24 B per entry of the largest layer that needed a transpose)
    // is kept across n2v2r_set_layer_csr calls only; the fit's buffers get the HBM back
    for (DevBuf* b : {&h->ing_keys[0], &h->ing_keys[1], &h->ing_pay[0], &h->ing_pay[1],
                      &h->ing_hist})
      b->release();
    const int ldu = ((d + 63) / 64) * 64;  // a multiple of every block width
    h->U.ensure(sizeof(float) * h->npad * ldu);
    HIPCHK(hipMemsetAsync(h->U.p, 0, sizeof(float) * h->npad * ldu, h->stream));
    std::vector<double> theta;
    int st = 0;
    std::optional<Eig> eig;
    for (int attempt = 0;; ++attempt) {
      eig.emplace(h);
      eig->stats = stats;
      eig->lean_off = attempt > 0;
      try {
        st = eig->run(d, o, theta, h->U.as<float>(), ldu);
      } catch (const Eig::LeanRetry&) {
        // lean images cannot take the dense Rayleigh-Ritz fallback: the fit again with images
        fprintf(stderr, "[n2v2r] banded Rayleigh-Ritz failed under lean images; fit rerun\n");
        HIPCHK(hipStreamSynchronize(h->stream));
        continue;
      }
      break;
    }
    build_embedding(h, eig->op, theta, ldu, eig->y_captured);
    h->have_embedding = true;
    h->ncmp = h->ncols = 0;
    if (st != N2V2R_OK)
      h->set_err("UASE did not converge: max residual %.3e (tol %.1e%s)",
                 stats ? stats->max_residual : -1.0, o.tol > 0 ? o.tol : 1e-6,
                 stats && stats->stagnated ? "; stopped flat above the fp32-floor cap" : "");
    return st;
  });
}

// The embedding step alone (tests): a GramOp set up as a fit's at width b, build_embedding on a
// host U and theta, the result installed as a fit installs it.
int n2v2r_embed_step(n2v2r_handle* h, int b, int d, const float* U, const double* theta,
                     n2v2r_embed_info* info) {
  if (info) {
    *info = n2v2r_embed_info{};
    info->form = -1;
  }
  return guarded(h, [&]() -> int {
    if (h->multi() || (b != 8 && b != 16 && b != 32 && b != 64) || !U || !theta)
      return N2V2R_ERR_BAD_ARG;
    if (!layers_ready(h)) return N2V2R_ERR_BAD_ARG;
    if (d < 1 || d > 600 || d >= h->n) {
      h->set_err("embedding dimension %d out of range [1, min(600, n-1)]", d);
      return N2V2R_ERR_BAD_ARG;
    }
    GramOp op(h);
    op.setup(b);
    hipStream_t st = h->stream;
    // as n2v2r_uase: no stale embedding or ranking results readable from here on
    h->have_embedding = false;
    h->ncmp = h->ncols = 0;
    h->have_borda = false;
    const int ldu = ((d + 63) / 64) * 64;
    h->U.ensure(sizeof(float) * h->npad * ldu);
    HIPCHK(hipMemsetAsync(h->U.p, 0, sizeof(float) * h->npad * ldu, st));
    if (h->nloc > 0)
      HIPCHK(hipMemcpy2DAsync(h->U.p, sizeof(float) * ldu, U + (size_t)h->row0 * d,
                              sizeof(float) * d, sizeof(float) * d, h->nloc,
                              hipMemcpyHostToDevice, st));
    // NaN bytes wherever the step has to write (the sizes are build_embedding's own): the local
    // rows of every Y_k, the column scales, the chunk keys and the winning keys
    h->keys.ensure(sizeof(unsigned long long) * 1024 * (size_t)ldu);
    h->best.ensure(sizeof(unsigned long long) * ldu);
    h->colscale.ensure(sizeof(float) * ldu);
    h->Y.ensure(sizeof(float) * (size_t)h->K * h->npad * ldu);
    HIPCHK(hipMemsetAsync(h->keys.p, 0xFF, sizeof(unsigned long long) * 1024 * (size_t)ldu, st));
    HIPCHK(hipMemsetAsync(h->best.p, 0xFF, sizeof(unsigned long long) * ldu, st));
    HIPCHK(hipMemsetAsync(h->colscale.p, 0xFF, sizeof(float) * ldu, st));
    for (int k = 0; k < h->K && h->nloc > 0; ++k)
      HIPCHK(hipMemsetAsync(h->Y.as<float>() + (size_t)k * h->npad * ldu, 0xFF,
                            sizeof(float) * h->nloc * ldu, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable source: complete before the kernels
    build_embedding(h, op, std::vector<double>(theta, theta + d), ldu, false, info);
    h->have_embedding = true;
    h->ncmp = h->ncols = 0;
    return N2V2R_OK;
  });
}

// One restart step alone (tests): an Eig set up as a fit's with the given plan, its ritz_vectors
// and launch_residuals on host arrays.
int n2v2r_ritz_step(n2v2r_handle* h, int b, int nq, int keep, int lean, const float* Q,
                    const float* W, const float* S, const double* theta, float* X, float* MX,
                    double* res, n2v2r_ritz_info* info) {
  return guarded(h, [&]() -> int {
    if (h->multi() || (b != 8 && b != 16 && b != 32 && b != 64) || nq < 1 || keep < b ||
        keep % b != 0 || (int64_t)keep + b > (int64_t)nq * b || (int64_t)nq * b > N2V2R_BAND_MAXC ||
        (lean && b != 8) || !Q || !S || !theta || !X || (!lean && (!W || !MX || !res)))
      return N2V2R_ERR_BAD_ARG;
    if (!layers_ready(h)) return N2V2R_ERR_BAD_ARG;
    Eig eig(h);
    eig.set_plan(b, keep, nq);
    eig.lean = lean != 0;  // (set_plan chose what a fit of this plan would take)
    hipStream_t st = eig.st;
    const int pb = eig.pb;
    const size_t rows = sizeof(float) * (size_t)eig.n * b;
    for (int q = 0; q < nq; ++q) {
      eig.Q.push_back(eig.take());
      HIPCHK(hipMemcpyAsync(eig.Q[q], Q + (size_t)q * eig.n * b, rows, hipMemcpyHostToDevice, st));
      if (eig.lean) continue;
      eig.W.push_back(eig.take());
      HIPCHK(hipMemcpyAsync(eig.W[q], W + (size_t)q * eig.n * b, rows, hipMemcpyHostToDevice, st));
    }
    // NaN bytes in every row the step has to write
    for (int q = 0; q < pb; ++q) {
      eig.X.push_back(eig.take());
      eig.MX.push_back(eig.lean ? nullptr : eig.take());
      HIPCHK(hipMemsetAsync(eig.X[q], 0xFF, rows, st));
      if (!eig.lean) HIPCHK(hipMemsetAsync(eig.MX[q], 0xFF, rows, st));
    }
    HIPCHK(hipMemsetAsync(h->resid.p, 0xFF, sizeof(double) * keep, st));
    HIPCHK(hipMemcpyAsync(h->ews.csmall.p, S, sizeof(float) * (size_t)nq * b * keep,
                          hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->theta.p, theta, sizeof(double) * keep, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable sources: complete before the kernels
    eig.ritz_vectors(nq);
    if (!eig.lean) eig.launch_residuals();
    for (int q = 0; q < pb; ++q) {
      HIPCHK(hipMemcpyAsync(X + (size_t)q * eig.n * b, eig.X[q], rows, hipMemcpyDeviceToHost, st));
      if (!eig.lean)
        HIPCHK(hipMemcpyAsync(MX + (size_t)q * eig.n * b, eig.MX[q], rows, hipMemcpyDeviceToHost,
                              st));
    }
    if (!eig.lean)
      HIPCHK(hipMemcpyAsync(res, h->resid.p, sizeof(double) * keep, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
      info->fused = eig.ritz_done ? 1 : 0;
      info->launches = eig.ritz_launches;
      info->lds_bytes = eig.ritz_done ? (int)n2v2r_ritz_nn_lds_bytes(nq, keep) : 0;
    }
    return N2V2R_OK;
  });
}

// An Eig set up as a fit's whose plan is block width b and a basis of nblk blocks (the Gram and
// pass diagnostics below); 0, or the status to return.
static int diag_eig(n2v2r_handle* h, int b, int nblk, Eig& eig) {
  if (h->multi() || h->comm || (b != 8 && b != 16 && b != 32 && b != 64) || nblk < 1 ||
      (int64_t)nblk * b > N2V2R_BAND_MAXC)
    return N2V2R_ERR_BAD_ARG;
  if (!layers_ready(h)) return N2V2R_ERR_BAD_ARG;
  eig.set_plan(b, b, nblk);
  return N2V2R_OK;
}

// the Gram launcher's plan for [na blocks]^T [nb blocks] on this Eig's partial buffer
static int diag_gram_info(const Eig& eig, int na, int nb, n2v2r_pass_info* info) {
  TnPlan plan{};
  if (n2v2r_ts_tn_plan(na, eig.b, nb, eig.b, eig.n, eig.part_n, &plan) != hipSuccess)
    return N2V2R_ERR_BAD_ARG;
  if (info) {
    *info = n2v2r_pass_info{};
    info->gram_form = plan.form;
    info->gram_flush = plan.flush;
    info->nchunks = plan.nchunks;
    info->rows_per_chunk = plan.rows_per_chunk;
  }
  return N2V2R_OK;
}

// One Gram alone (tests): an Eig set up as a fit's with the given plan, its tn on host blocks.
int n2v2r_block_gram(n2v2r_handle* h, int b, int na, int nb, const float* A, const float* B,
                     double* G, n2v2r_pass_info* info) {
  return guarded(h, [&]() -> int {
    if (na < 1 || nb < 1 || !A || !B || !G) return N2V2R_ERR_BAD_ARG;
    Eig eig(h);
    if (const int s = diag_eig(h, b, std::max(na, nb), eig)) return s;
    if (const int s = diag_gram_info(eig, na, nb, info)) return s;
    hipStream_t st = eig.st;
    const size_t rows = sizeof(float) * (size_t)eig.n * b;
    std::vector<float*> a, bb;
    for (int q = 0; q < na; ++q) {
      a.push_back(eig.take());
      HIPCHK(hipMemcpyAsync(a[q], A + (size_t)q * eig.n * b, rows, hipMemcpyHostToDevice, st));
    }
    for (int q = 0; q < nb; ++q) {
      bb.push_back(eig.take());
      HIPCHK(hipMemcpyAsync(bb[q], B + (size_t)q * eig.n * b, rows, hipMemcpyHostToDevice, st));
    }
    // NaN bytes in the Gram and in every chunk partial the launch has to write
    const size_t gbytes = sizeof(double) * (size_t)na * b * nb * b;
    HIPCHK(hipMemsetAsync(eig.gsm_p, 0xFF, gbytes, st));
    HIPCHK(hipMemsetAsync(eig.part_p, 0xFF, h->partial.bytes, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable sources: complete before the kernels
    eig.tn(eig.blocks(a, 0, na), eig.blocks(bb, 0, nb), eig.gsm_p, nullptr);
    HIPCHK(hipMemcpyAsync(G, eig.gsm_p, gbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return N2V2R_OK;
  });
}

// One orthogonalisation pass alone (tests): an Eig set up as a fit's with the given plan, its
// pip_pass on host blocks.
int n2v2r_ortho_pass(n2v2r_handle* h, int b, int nq, const float* Q, float* Z, int in_place,
                     int first, int cond, uint64_t seed, double* gram, double* xinv, float* F,
                     int* flags, int* any_flag, n2v2r_pass_info* info) {
  return guarded(h, [&]() -> int {
    if (nq < 0 || (nq > 0 && !Q) || !Z || !gram || !flags || !any_flag || cond < -1 || cond > 1 ||
        (b != 8 && (!xinv || !F)))
      return N2V2R_ERR_BAD_ARG;
    Eig eig(h);
    if (const int s = diag_eig(h, b, nq + 1, eig)) return s;
    if (const int s = diag_gram_info(eig, nq + 1, 1, info)) return s;
    const int c = nq * b;
    const int kern = b == 8 ? 0 : n2v2r_nn_kernel(nq + 1, b, b);
    if (kern < 0) return N2V2R_ERR_BAD_ARG;
    eig.seed = seed;
    hipStream_t st = eig.st;
    const size_t rows = sizeof(float) * (size_t)eig.n * b;
    std::vector<float*> basis;
    for (int q = 0; q < nq; ++q) {
      basis.push_back(eig.take());
      HIPCHK(hipMemcpyAsync(basis[q], Q + (size_t)q * eig.n * b, rows, hipMemcpyHostToDevice, st));
    }
    float* zin = eig.take();
    float* z = in_place ? zin : eig.take();
    HIPCHK(hipMemcpyAsync(zin, Z, rows, hipMemcpyHostToDevice, st));
    // NaN bytes wherever the pass has to write, a non-zero pattern in the flag words
    if (!in_place) HIPCHK(hipMemsetAsync(z, 0xFF, rows, st));
    const size_t gbytes = sizeof(double) * (size_t)(c + b) * b;
    HIPCHK(hipMemsetAsync(eig.gsm_p, 0xFF, gbytes, st));
    HIPCHK(hipMemsetAsync(eig.part_p, 0xFF, h->partial.bytes, st));
    HIPCHK(hipMemsetAsync(h->ews.rinv.p, 0xFF, h->ews.rinv.bytes, st));
    HIPCHK(hipMemsetAsync(h->ews.fcoef.p, 0xFF, h->ews.fcoef.bytes, st));
    HIPCHK(hipMemsetAsync(eig.flg_p, 0x5A, sizeof(int) * 256, st));
    HIPCHK(hipMemsetAsync(eig.any_p, 0x5A, sizeof(int) * 4, st));
    // the pass's slot as the solver gives it: first (0), full (1), or the conditional third (2)
    PipPass p = cond >= 0 ? eig.third_pass() : eig.pass_in_slot(first ? 0 : 1);
    p.first = first;
    if (cond >= 0)
      HIPCHK(hipMemcpyAsync(const_cast<int*>(p.cond), &cond, sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable sources: complete before the kernels
    eig.pip_pass(z, basis, p, in_place ? nullptr : zin);
    HIPCHK(hipMemcpyAsync(Z, z, rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(gram, eig.gsm_p, gbytes, hipMemcpyDeviceToHost, st));
    if (b != 8) {
      HIPCHK(hipMemcpyAsync(xinv, h->ews.rinv.p, sizeof(double) * b * b, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(F, h->ews.fcoef.p, sizeof(float) * (size_t)(c + b) * b,
                            hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(flags, p.flags, sizeof(int) * b, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(any_flag, p.any_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
      if (b != 8) n2v2r_pip_chol_plan(c, b, 1, &info->stage, &info->nwg);
      info->apply_kernel = kern;
      info->fill_seed = eig.last_fill_seed;
    }
    return N2V2R_OK;
  });
}

// local rows (row0 .. row0 + n_local) on a distributed handle
int n2v2r_get_embedding(n2v2r_handle* h, float* Y) {
  if (h && h->multi()) return multi_get_embedding(h, Y);
  return guarded(h, [&]() -> int {
    if (!h->have_embedding) {
      h->err = "No n2v2r embeddings found";
      return N2V2R_ERR_NOT_READY;
    }
    copy_embedding(h, Y, (int64_t)h->nloc * h->d);
    return N2V2R_OK;
  });
}

int n2v2r_get_left_embedding(n2v2r_handle* h, float* X) {
  if (h && h->multi()) return multi_get_left_embedding(h, X);
  return guarded(h, [&]() -> int {
    if (!h->have_embedding || h->U.p == nullptr) {
      h->err = "No n2v2r embeddings found";
      return N2V2R_ERR_NOT_READY;
    }
    HIPCHK(hipMemcpy2DAsync(X, sizeof(float) * h->d, h->U.as<float>(), sizeof(float) * h->ldy,
                            sizeof(float) * h->d, h->nloc, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < h->nloc; ++i)
      for (int j = 0; j < h->d; ++j) X[i * h->d + j] *= (float)std::sqrt(h->sigma[j]);
    return N2V2R_OK;
  });
}

int n2v2r_get_singular_values(n2v2r_handle* h, double* s) {
  if (h && h->multi()) h = h->ranks[0];  // identical on every rank
  return guarded(h, [&]() -> int {
    if (!h->have_embedding) {
      h->err = "No n2v2r embeddings found";
      return N2V2R_ERR_NOT_READY;
    }
    std::copy(h->sigma.begin(), h->sigma.end(), s);
    return N2V2R_OK;
  });
}

int n2v2r_set_embedding(n2v2r_handle* h, int num_layers, int64_t n, int d, const float* Y) {
  return guarded(h, [&]() -> int {
    if (num_layers < 1 || n < 1 || d < 1 || !Y) return N2V2R_ERR_BAD_ARG;
    if (h->comm || h->multi()) {
      h->err = "set_embedding is single-GPU only";
      return N2V2R_ERR_BAD_ARG;
    }
    h->K = num_layers;
    h->set_partition(n);
    h->d = d;
    h->ldy = d;
    h->Y.ensure(sizeof(float) * (size_t)num_layers * n * d);
    HIPCHK(hipMemcpyAsync(h->Y.p, Y, sizeof(float) * (size_t)num_layers * n * d,
                          hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sigma.assign(d, 0.0);
    h->have_embedding = true;
    h->ncmp = h->ncols = 0;
    return N2V2R_OK;
  });
}

}  // extern "C"
