// n2v2r engine: handle lifecycle and the diagnostic entry points (include/n2v2r_diag.h).
// The rest of the C-ABI: layers.cpp (ingest), solver.cpp (UASE), gram_op.cpp (the Gram operator),
// ranking.cpp (distances, Borda), comm.cpp (row-partitioned communicators), multi.cpp (one
// process, N GPUs).
#include "gram_op.h"

using namespace n2v2r_int;

namespace n2v2r_int {
n2v2r_handle* new_handle(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return nullptr;
  if (device < 0 || device >= count) return nullptr;
  auto* h = new (std::nothrow) n2v2r_handle();
  if (!h) return nullptr;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return nullptr;
  }
  return h;
}

}  // namespace n2v2r_int

extern "C" {

const char* n2v2r_version(void) { return "n2v2r-mi355x 0.2.0 (gfx950)"; }

int n2v2r_create(int device, n2v2r_handle** out) {
  if (!out) return N2V2R_ERR_BAD_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return N2V2R_ERR_HIP;
  if (device < 0 || device >= count) return N2V2R_ERR_BAD_ARG;
  n2v2r_handle* h = new_handle(device);
  if (!h) return N2V2R_ERR_HIP;
  *out = h;
  return N2V2R_OK;
}

void n2v2r_destroy(n2v2r_handle* h) {
  if (!h) return;
  if (h->multi()) {
    (void)multi_destroy(h);
    return;
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->layers.clear();
  h->comm.reset();
  for (hipEvent_t& e : h->cb_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->pin) (void)hipHostFree(h->pin);
  for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
  if (h->cstream) (void)hipStreamSynchronize(h->cstream);
  for (hipEvent_t& e : h->cev)
    if (e) (void)hipEventDestroy(e);
  if (h->cstream) (void)hipStreamDestroy(h->cstream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int n2v2r_last_error(const n2v2r_handle* h, char* buf, size_t len) {
  if (!h || !buf || len == 0) return N2V2R_ERR_BAD_ARG;
  snprintf(buf, len, "%s", h->err.c_str());
  return N2V2R_OK;
}

int n2v2r_synchronize(n2v2r_handle* h) {
  if (h && h->multi()) return multi_synchronize(h);
  return guarded(h, [&]() -> int {
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}

// Rayleigh-Ritz stage alone (tests): top-p eigenpairs of a host symmetric c x c matrix through
// the same GPU tridiagonalisation + host tridiagonal solve + GPU back-transform as UASE.
int n2v2r_rr_top(n2v2r_handle* h, int c, const double* H, int p, double* w, float* S) {
  if (h && h->multi()) h = h->ranks[0];  // (diagnostics: rank 0)
  return guarded(h, [&]() -> int {
    if (c < 3 || c > 768 || p < 1 || p > c || !H || !w || !S) return N2V2R_ERR_BAD_ARG;
    DevBuf a, tri, refl, y, s;
    a.ensure(sizeof(double) * c * c);
    tri.ensure(sizeof(double) * 3 * c);
    refl.ensure(sizeof(double) * c * c);
    y.ensure(sizeof(double) * c * p);
    s.ensure(sizeof(float) * c * p);
    HIPCHK(hipMemcpyAsync(a.p, H, sizeof(double) * c * c, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // pageable source: complete before the kernel
    double* t = tri.as<double>();
    DevBuf trs;
    trs.ensure(n2v2r_rr_tridiag_scratch_bytes(c));
    HIPCHK(n2v2r_launch_rr_tridiag(a.as<double>(), c, t, t + c, t + 2 * c, refl.as<double>(),
                                   trs.p, h->stream));
    DevBuf wd, scr;
    wd.ensure(sizeof(double) * p);
    scr.ensure(sizeof(double) * 6 * (size_t)((p + 63) / 64 * 64) * c);
    HIPCHK(n2v2r_launch_rr_tri_eig(t, t + c, c, p, wd.as<double>(), y.as<double>(),
                                   scr.as<double>(), h->stream));
    HIPCHK(hipMemcpyAsync(w, wd.p, sizeof(double) * p, hipMemcpyDeviceToHost, h->stream));
    DevBuf btf;
    btf.ensure(n2v2r_rr_bt_scratch_bytes(c));
    HIPCHK(n2v2r_launch_rr_backtransform(refl.as<double>(), t + 2 * c, c, y.as<double>(), p,
                                         s.as<float>(), p, btf.as<double>(), h->stream));
    HIPCHK(hipMemcpyAsync(S, s.p, sizeof(float) * c * p, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}

// One orthogonalisation pass at b = 8 alone (tests): the solver's launchers on host arrays.
int n2v2r_pip_pass(n2v2r_handle* h, int64_t n, int nq, const float* Q, float* Za, float* Zb,
                   float tau, int first, int form, uint64_t seed, double* gram, double* R,
                   int* flags, int* any_flag, int* skipped) {
  return guarded(h, [&]() -> int {
    const int nz = Zb ? 2 : 1;
    if (h->multi() || h->comm || n < 1 || nq < 1 || (nq + nz - 1) * 8 > N2V2R_BAND_MAXC || !Q || !Za ||
        !gram || !flags || !any_flag || !skipped || (Zb && (first || form < 0 || form > 1)) ||
        (!Zb && !R))
      return N2V2R_ERR_BAD_ARG;
    hipStream_t st = h->stream;
    const size_t blk = sizeof(float) * (size_t)n * 8;
    const int nskip = 4 + N2V2R_BAND_MAXC / 8;
    DevBuf basis, part, g, r, words, plan;
    basis.ensure(blk * (nq + nz));
    // the streaming Grams' partials: their chunk plan's largest count, two right-hand sides
    const size_t part_n =
        (size_t)std::max<int64_t>(4096 / (nq + nz), n / 8192) * (nq + nz) * 128 + 9 * 128 * (nq + nz);
    part.ensure(sizeof(double) * part_n);
    g.ensure(sizeof(double) * nz * (size_t)(nq + nz) * 64);
    r.ensure(sizeof(double) * 64);
    words.ensure(sizeof(int) * (64 + 4 + nskip));  // flags | any_flag, sticky | skip counters
    int* fl = words.as<int>();
    HIPCHK(hipMemsetAsync(fl, 0, sizeof(int) * (64 + 4 + nskip), st));
    BlockList all{};
    all.count = nq + nz;
    all.width = 8;
    for (int i = 0; i < nq + nz; ++i) all.blk[i] = basis.as<float>() + (size_t)i * n * 8;
    float* za = basis.as<float>() + (size_t)nq * n * 8;
    float* zb = za + (size_t)n * 8;
    HIPCHK(hipMemcpyAsync(basis.p, Q, blk * nq, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(za, Za, blk, hipMemcpyHostToDevice, st));
    if (Zb) HIPCHK(hipMemcpyAsync(zb, Zb, blk, hipMemcpyHostToDevice, st));
    const double eye[64] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0,
                            0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0,
                            0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    HIPCHK(hipMemcpyAsync(r.p, eye, sizeof(eye), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable sources: complete before the kernels
    PipPass p;
    p.flags = fl;
    p.any_flag = fl + 64;
    p.sticky = fl + 65;
    p.seed = seed;
    p.rsave = r.as<double>();
    p.skip_tol = tau;
    p.skipped = tau != 0.f ? fl + 68 : nullptr;
    p.first = first;
    hipError_t e;
    bool paired = true;
    if (!Zb) {
      BlockList B{};
      B.count = 1;
      B.width = 8;
      B.blk[0] = za;
      e = n2v2r_launch_ts_tn(all, B, n, part.as<double>(), part_n, g.as<double>(), nullptr, st);
      all.count = nq;
      if (e == hipSuccess)
        e = n2v2r_launch_pip_fused(all, za, za, g.as<double>(), nq * 8, n, p, st);
    } else {
      e = n2v2r_launch_ts_tn2(all, za, zb, n, part.as<double>(), part_n, g.as<double>(), st);
      if (e == hipSuccess) {
        PipPass pz = p;  // Zb's pass: the next seed, no R
        pz.seed = seed + 1;
        pz.rsave = nullptr;
        if (form == 1) plan.ensure(sizeof(int) * N2V2R_PAIR_PLAN_WORDS);
        paired = pair_apply_launches(all, g.as<double>(), n, p, pz, form == 1 ? plan.as<int>() : nullptr,
                                     plan.bytes, st) == (form == 1);
      }
    }
    if (e == hipErrorInvalidValue || e == hipErrorNotSupported) return N2V2R_ERR_BAD_ARG;
    HIPCHK(e);
    HIPCHK(hipMemcpyAsync(Za, za, blk, hipMemcpyDeviceToHost, st));
    if (Zb) HIPCHK(hipMemcpyAsync(Zb, zb, blk, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(gram, g.p, sizeof(double) * nz * (size_t)(nq + nz) * 64,
                          hipMemcpyDeviceToHost, st));
    if (!Zb) HIPCHK(hipMemcpyAsync(R, r.p, sizeof(double) * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(flags, fl, sizeof(int) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(any_flag, fl + 64, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(skipped, fl + 68, sizeof(int) * (nq + nz), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return paired ? N2V2R_OK : N2V2R_ERR_BAD_ARG;  // (form 1 where the plan does not fit)
  });
}

// One Rayleigh-Ritz of a Krylov-Schur projected matrix in a chosen form alone (tests), through
// the solver's launchers, in buffers of its own.
int n2v2r_rr_stage(n2v2r_handle* h, int c, int kp, const double* hband, int64_t hband_len,
                   const double* theta_prev, int p, int form, double* w, float* S, double* Y,
                   n2v2r_rr_info* info) {
  if (h && h->multi()) h = h->ranks[0];  // (diagnostics: rank 0)
  return guarded(h, [&]() -> int {
    const int b = 8;
    n2v2r_rr_info inf = {-1, -1, -1, -1, -1, 0, 0, 0};
    if (info) *info = inf;
    // the launchers' own limits (n2v2r_launch_rr_sturm, _rr_band_expand: c >= 9; _rr_band)
    if (form < -1 || form > 2 || c < 2 * b || c > N2V2R_BAND_MAXC || c % b || kp < 0 || kp % b ||
        kp + b > c || p < 1 || p > c || !hband || !w || !S || (kp > 0 && !theta_prev) ||
        (form == (int)RrForm::BandReduce && kp + b > 192))
      return N2V2R_ERR_BAD_ARG;
    const int64_t need = (int64_t)(kp + b) * b + (int64_t)(c / b - kp / b - 1) * 2 * b * b;
    if (hband_len < need) return N2V2R_ERR_BAD_ARG;
    hipStream_t st = h->stream;
    DevBuf hb, th, y, s, er, scr;
    hb.ensure(sizeof(double) * hband_len);
    th.ensure(sizeof(double) * c);
    y.ensure(sizeof(double) * c * p);
    s.ensure(sizeof(float) * c * p);
    er.ensure(4 * sizeof(int));
    HIPCHK(hipMemcpyAsync(hb.p, hband, sizeof(double) * hband_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable source: complete before the kernels
    // what a form starts from: NaN bytes behind w, S and Y, the kept Ritz values in theta, the
    // error words zero (the kernels only set them)
    auto arm = [&]() {
      HIPCHK(hipMemsetAsync(th.p, 0xFF, sizeof(double) * c, st));
      HIPCHK(hipMemsetAsync(y.p, 0xFF, sizeof(double) * c * p, st));
      HIPCHK(hipMemsetAsync(s.p, 0xFF, sizeof(float) * c * p, st));
      HIPCHK(hipMemsetAsync(er.p, 0, 4 * sizeof(int), st));
      if (kp > 0)
        HIPCHK(hipMemcpyAsync(th.p, theta_prev, sizeof(double) * kp, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    };
    auto refused = [](hipError_t e) { return e == hipErrorInvalidValue; };
    bool y_valid = false;
    RrForm run = form < 0 ? RrForm::Sturm : (RrForm)form;
    if (run == RrForm::Sturm) {
      arm();
      scr.ensure(sizeof(double) * n2v2r_rr_sturm_scratch(c, p));
      const hipError_t e = n2v2r_launch_rr_sturm(
          hb.as<double>(), c, kp, th.as<double>(), scr.as<double>(), scr.bytes / sizeof(double),
          y.as<double>(), s.as<float>(), p, p, er.as<int>(), st);
      if (refused(e)) return N2V2R_ERR_BAD_ARG;
      HIPCHK(e);
      int ew[2] = {0, 0};
      HIPCHK(hipMemcpyAsync(ew, er.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      inf.sturm_err = ew[0];
      inf.second_solves = ew[1];
      n2v2r_rr_sturm_msect(p, &inf.msect_points, &inf.msect_rounds);
      y_valid = true;
      // as a fit moves: the form rr_next takes after a failed Sturm result
      // (N2V2R_RR_STAGE_TEST_STURM_FAIL=1, tests: a good result discarded, as a fit's
      // N2V2R_EIG_TEST_STURM_FAIL does; sturm_err still reports the launch's own word)
      if (form < 0 && (ew[0] != 0 || env_flag("N2V2R_RR_STAGE_TEST_STURM_FAIL")))
        run = rr_after_sturm(kp, c);
    }
    if (run == RrForm::BandReduce) {
      DevBuf ab, va, ta, tri, rf;
      rf.ensure(sizeof(double) * c * n2v2r_rr_band_jm(c) * 9);
      ab.ensure(sizeof(double) * c * (b + 1));
      va.ensure(sizeof(double) * (kp + b) * (kp + b));
      ta.ensure(sizeof(double) * (kp + b));
      tri.ensure(sizeof(double) * 2 * c);
      arm();
      const hipError_t e = n2v2r_launch_rr_band(
          hb.as<double>(), c, kp, th.as<double>(), ab.as<double>(), va.as<double>(),
          ta.as<double>(), tri.as<double>(), tri.as<double>() + c, rf.as<double>(),
          y.as<double>(), s.as<float>(), p, p, er.as<int>(), st);
      if (refused(e)) {
        HIPCHK(hipStreamSynchronize(st));
        return N2V2R_ERR_BAD_ARG;
      }
      HIPCHK(e);
      HIPCHK(hipMemcpyAsync(&inf.reduce_err, er.p, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      y_valid = false;  // the inverse iteration's vectors are in the tridiagonal's basis
    } else if (run == RrForm::DenseFromBand) {
      DevBuf a, tri, refl, trs, btf, kept;
      a.ensure(sizeof(double) * c * c);
      tri.ensure(sizeof(double) * 3 * c);
      refl.ensure(sizeof(double) * c * c);
      trs.ensure(n2v2r_rr_tridiag_scratch_bytes(c));
      btf.ensure(n2v2r_rr_bt_scratch_bytes(c));
      double* t = tri.as<double>();
      // the kept Ritz values: after a Sturm launch the copy its assembly made (as a fit reads
      // them), else theta_prev
      const double* kth = nullptr;
      if (kp > 0) {
        if (scr.p) {
          kth = scr.as<double>() + 4;
        } else {
          kept.ensure(sizeof(double) * kp);
          HIPCHK(hipMemcpyAsync(kept.p, theta_prev, sizeof(double) * kp, hipMemcpyHostToDevice,
                                st));
          HIPCHK(hipStreamSynchronize(st));
          kth = kept.as<double>();
        }
      }
      arm();
      // the multi-workgroup tridiagonalisation first; after a timed-out grid barrier (its error
      // word) the step again with the one-workgroup kernel, as rr_next does
      for (int attempt = 0; attempt < 2; ++attempt) {
        hipError_t e = n2v2r_launch_rr_band_expand(hb.as<double>(), c, kp, kth, a.as<double>(), st);
        if (refused(e)) return N2V2R_ERR_BAD_ARG;
        HIPCHK(e);
        int coop = 0;
        HIPCHK(n2v2r_launch_rr_tridiag(a.as<double>(), c, t, t + c, t + 2 * c, refl.as<double>(),
                                       attempt == 0 ? trs.p : nullptr, st, &coop));
        inf.tri_coop = coop;
        if (!coop) break;
        int terr = 0;
        HIPCHK(hipMemcpyAsync(&terr, n2v2r_rr_tridiag_err(trs.p, c), sizeof(int),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!terr) break;
      }
      HIPCHK(n2v2r_launch_rr_tri_eig(t, t + c, c, p, th.as<double>(), y.as<double>(), nullptr, st));
      HIPCHK(n2v2r_launch_rr_backtransform(refl.as<double>(), t + 2 * c, c, y.as<double>(), p,
                                           s.as<float>(), p, btf.as<double>(), st));
      HIPCHK(hipStreamSynchronize(st));  // the buffers above die here
      y_valid = false;  // as above: fp64 vectors of the tridiagonal only
    }
    inf.form_ran = (int)run;
    HIPCHK(hipMemcpyAsync(w, th.p, sizeof(double) * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(S, s.p, sizeof(float) * c * p, hipMemcpyDeviceToHost, st));
    if (Y) {
      if (!y_valid) HIPCHK(hipMemsetAsync(y.p, 0xFF, sizeof(double) * c * p, st));
      HIPCHK(hipMemcpyAsync(Y, y.p, sizeof(double) * c * p, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (info) *info = inf;
    return N2V2R_OK;
  });
}

int n2v2r_rr_band_top(n2v2r_handle* h, int c, int kp, const double* hband, int64_t hband_len,
                      const double* theta_prev, int p, double* w, float* S) {
  // the limits this entry has always had (inside the reducing path's, which is its fallback)
  if (c < 3 || c > 512 || kp + 8 > 192) return N2V2R_ERR_BAD_ARG;
  n2v2r_rr_info info;
  // the solver's default form as a fit moves (N2V2R_RR=band: the reducing one)
  const int st = n2v2r_rr_stage(h, c, kp, hband, hband_len, theta_prev, p,
                                rr_sturm_enabled() ? -1 : (int)RrForm::BandReduce, w, S, nullptr,
                                &info);
  if (st != N2V2R_OK) return st;
  if (info.reduce_err > 0) {
    if (h->multi()) h = h->ranks[0];
    h->err = "banded Rayleigh-Ritz: bulge chase aborted";
    return N2V2R_ERR_NO_CONVERGENCE;
  }
  return N2V2R_OK;
}

int n2v2r_spmm_col_blocks(const n2v2r_handle* h, int b) {
  if (h && h->multi()) h = h->ranks[0];  // (diagnostics: rank 0)
  if (!h) return N2V2R_ERR_BAD_ARG;
  return col_blocks_wanted(h, b) ? 1 : 0;
}

// The flat-window tiled SpMM of layer k (A_k X, or A_k^T X) with `nb` column blocks (0: the fit's
// rule, panel blocks of <= 2 MB, at most 64) from device panels, timed with HIP events over `reps`
// launches after a warm-up.  N2V2R_ERR_BAD_ARG when the layer cannot take packed blocks.
static int time_tiled(n2v2r_handle* h, int k, int transpose, int nb, const float* xd, float* yd,
                      int reps, double* avg_ms) {
  if (nb <= 0) nb = tile_nb_auto(h->n);
  if (nb != 4 && nb != 8 && nb != 16 && nb != 32 && nb != 64 && nb != 128) return N2V2R_ERR_BAD_ARG;
  LayerDev& L = *h->layers[k];
  const int wb = tile_wbits(h->layers, nb);
  if (!ensure_col_blocks(L, h->n, h->stream, nb, wb)) return N2V2R_ERR_BAD_ARG;
  const LayerDev::ColBlocks& cbs = (transpose && !L.symmetric) ? L.cb_t : L.cb;
  DevBuf tb;  // this layer's blocks alone
  tb.ensure(sizeof(CsrBlk) * nb);
  HIPCHK(hipMemcpyAsync(tb.p, cbs.blk, sizeof(CsrBlk) * nb, hipMemcpyHostToDevice, h->stream));
  SpmmTileArgs a =
      spmm_tile_args(tb.as<CsrBlk>(), nb, wb, tile_rows_for(h, wb), h->nloc, 0, 1, 0, 8);
  a.X[0] = xd;
  a.Y[0] = yd;
  HIPCHK(n2v2r_launch_spmm_tile(a, h->stream));  // warm-up
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, h->stream));
  for (int r = 0; r < reps; ++r) HIPCHK(n2v2r_launch_spmm_tile(a, h->stream));
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (avg_ms) *avg_ms = (double)ms / reps;
  HIPCHK(hipStreamSynchronize(h->stream));  // tb dies here
  return N2V2R_OK;
}

int n2v2r_bench_spmm(n2v2r_handle* h, int k, int transpose, int b, int reps, const float* X,
                     float* Y, double* avg_ms, double* algo_bytes) {
  if (h && h->multi()) h = h->ranks[0];  // (diagnostics: rank 0)
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !h->layers[k]->loaded || (b != 8 && b != 16 && b != 32 && b != 64) ||
        reps < 1 || !X)
      return N2V2R_ERR_BAD_ARG;
    const LayerDev& L = *h->layers[k];
    DevBuf xd, yd;
    xd.ensure(sizeof(float) * h->n * b);
    yd.ensure(sizeof(float) * std::max<int64_t>(h->nloc, 1) * b);
    HIPCHK(hipMemcpyAsync(xd.p, X, sizeof(float) * h->n * b, hipMemcpyHostToDevice, h->stream));
    if (L.dense) {
      // dense layer: the GEMM Y = A_k X (or A_k^T X) over this rank's rows
      const float* am = transpose ? L.dense_at() : L.dense_a();
      const float* bt = h->comm ? nullptr : (transpose ? L.dense_a() : L.dense_at());
      h->dense_apply(am, L.lda, xd.as<float>(), b, b, yd.as<float>(), b, 0.f, nullptr, bt);
      hipEvent_t e0, e1;
      HIPCHK(hipEventCreate(&e0));
      HIPCHK(hipEventCreate(&e1));
      HIPCHK(hipEventRecord(e0, h->stream));
      for (int r = 0; r < reps; ++r)
        h->dense_apply(am, L.lda, xd.as<float>(), b, b, yd.as<float>(), b, 0.f, nullptr, bt);
      HIPCHK(hipEventRecord(e1, h->stream));
      HIPCHK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      if (avg_ms) *avg_ms = (double)ms / reps;
      if (algo_bytes)
        *algo_bytes = 4.0 * (double)h->nloc * (double)h->n + 4.0 * (double)(h->n + h->nloc) * b;
      if (Y)
        HIPCHK(hipMemcpyAsync(Y, yd.p, sizeof(float) * h->nloc * b, hipMemcpyDeviceToHost,
                              h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      return N2V2R_OK;
    }
    if (col_blocks_wanted(h, b)) {
      // the flat-window tiled SpMM of one layer (the fit's form at this panel size)
      double ms = 0.0;
      const int st_ = time_tiled(h, k, transpose, 0, xd.as<float>(), yd.as<float>(), reps, &ms);
      if (st_ == N2V2R_OK) {
        const CsrDev c0 = transpose ? L.csr_t() : L.csr();
        if (avg_ms) *avg_ms = ms;
        if (algo_bytes) *algo_bytes = spmm_algo_bytes(c0.nnz, c0.unit != 0, h->nloc, h->n, b);
        if (Y)
          HIPCHK(hipMemcpyAsync(Y, yd.p, sizeof(float) * h->nloc * b, hipMemcpyDeviceToHost,
                                h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return N2V2R_OK;
      }
    }
    SpmmArgs a{};
    a.K = 1;
    a.sum = 0;
    a.ldx = b;
    a.ldy = b;
    a.colscale = nullptr;
    a.A[0] = transpose ? L.csr_t() : L.csr();
    a.X[0] = xd.as<float>();
    a.Y[0] = yd.as<float>();
    HIPCHK(n2v2r_launch_spmm(a, b, h->stream));  // warm-up
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, h->stream));
    for (int r = 0; r < reps; ++r) HIPCHK(n2v2r_launch_spmm(a, b, h->stream));
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (avg_ms) *avg_ms = (double)ms / reps;
    if (algo_bytes)
      *algo_bytes = spmm_algo_bytes(a.A[0].nnz, a.A[0].unit != 0, h->nloc, h->n, b);
    if (Y)
      HIPCHK(hipMemcpyAsync(Y, yd.p, sizeof(float) * h->nloc * b, hipMemcpyDeviceToHost,
                            h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}


int n2v2r_bench_spmm_tiled(n2v2r_handle* h, int k, int transpose, int b, int nb, int reps,
                           const float* X, float* Y, double* avg_ms) {
  if (h && h->multi()) h = h->ranks[0];  // (diagnostics: rank 0)
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !h->layers[k]->loaded || h->layers[k]->dense ||
        b != 8 || reps < 1 || !X || h->comm)
      return N2V2R_ERR_BAD_ARG;
    DevBuf xd, yd;
    xd.ensure(sizeof(float) * h->n * b);
    yd.ensure(sizeof(float) * std::max<int64_t>(h->nloc, 1) * b);
    HIPCHK(hipMemcpyAsync(xd.p, X, sizeof(float) * h->n * b, hipMemcpyHostToDevice, h->stream));
    const int st_ =
        time_tiled(h, k, transpose, nb, xd.as<float>(), yd.as<float>(), reps, avg_ms);
    if (st_ != N2V2R_OK) return st_;
    if (Y)
      HIPCHK(hipMemcpyAsync(Y, yd.p, sizeof(float) * h->nloc * b, hipMemcpyDeviceToHost,
                            h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}

}  // extern "C"
