// Layer ingest: CSR / dense layers to HBM (range check, GPU transpose and symmetry test, row
// slices of partitioned handles), the column-block copies of the flat tiled SpMM, the
// column sums (DeDi) and the bipartite projection.
#include "engine.h"

using namespace n2v2r_int;

namespace n2v2r_int {
// Split a CSR into nb column blocks of ceil(ncols / nb) columns, packed for the flat tiled SpMM
// (spmm.hip): per-row block counts on the GPU, a device scan into entry positions, the window
// offsets of windows of 2^wbits rows, and a scatter keeping each row's entries in order.  One-off
// per layer; not part of a fit's timed work.  cbits stays 0 (the layer not packable) when the
// column bits of a block and the row-in-window bits do not fit 31 bits.
void build_col_blocks(const CsrDev& A, int64_t ncols, LayerDev::ColBlocks& out, hipStream_t st,
                      int nb, int wbits) {
  const int64_t n = A.n_rows;
  const int64_t cw = (ncols + nb - 1) / nb;
  int cbits = 1;
  while (((int64_t)1 << cbits) < cw) ++cbits;
  out.ncols = ncols;
  out.nb = nb;
  out.wbits = wbits;
  out.cbits = cbits + wbits <= 31 ? cbits : 0;
  out.built = true;
  out.usable = false;
  if (n <= 0 || out.cbits == 0) return;
  // per-row block counts, then every entry position by a device scan (no host round trip)
  DevBuf cnt, rp64, tsum;
  cnt.ensure(sizeof(int32_t) * nb * n, st);
  HIPCHK(n2v2r_launch_cb_count(A, cw, nb, cnt.as<int32_t>(), st));
  const int64_t ntiles = n2v2r_cb_scan_tiles(n, nb);
  tsum.ensure(sizeof(int64_t) * ntiles, st);
  rp64.ensure(sizeof(int64_t) * nb * (n + 1), st);
  const int64_t nw1 = ((n + ((int64_t)1 << wbits) - 1) >> wbits) + 1;
  out.wo.ensure(sizeof(int32_t) * nb * nw1, st);
  HIPCHK(n2v2r_launch_cb_rowptrs(cnt.as<int32_t>(), n, nb, A.nnz, tsum.as<int64_t>(),
                                 (size_t)ntiles, rp64.as<int64_t>(), out.wo.as<int32_t>(), wbits,
                                 st));
  // block bases and ends: rp[j][0], rp[j][n]
  std::vector<int64_t> ends(2 * (size_t)nb);
  for (int j = 0; j < nb; ++j) {
    HIPCHK(hipMemcpyAsync(&ends[2 * j], rp64.as<int64_t>() + (size_t)j * (n + 1),
                          sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&ends[2 * j + 1], rp64.as<int64_t>() + (size_t)j * (n + 1) + n,
                          sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (ends[2 * (nb - 1) + 1] != A.nnz || ends[0] != 0)
    throw StatusFail{N2V2R_ERR_INTERNAL, "column-block split lost entries"};
  for (int j = 0; j < nb; ++j)
    if (ends[2 * j + 1] - ends[2 * j] > (int64_t)INT32_MAX) return;  // int32 offsets: row kernel
  out.idx.ensure(sizeof(int32_t) * std::max<int64_t>(A.nnz, 1), st);
  if (!A.unit) out.dat.ensure(sizeof(float) * std::max<int64_t>(A.nnz, 1), st);
  HIPCHK(n2v2r_launch_cb_fill(A, cw, nb, rp64.as<int64_t>(), out.idx.as<int32_t>(),
                              A.unit ? nullptr : out.dat.as<float>(), out.cbits, wbits, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < nb; ++j)
    out.blk[j] = CsrBlk{out.wo.as<int32_t>() + (size_t)j * nw1, out.idx.as<int32_t>(),
                        A.unit ? nullptr : out.dat.as<float>(), ends[2 * j], n,
                        ends[2 * j + 1] - ends[2 * j], A.unit, out.cbits, (int64_t)j * cw};
  out.usable = true;
}

// false when a block would exceed int32 offsets or the packed bits do not fit (then the row
// kernel runs)
bool ensure_col_blocks(LayerDev& L, int64_t ncols, hipStream_t st, int nb, int wbits) {
  auto stale = [&](const LayerDev::ColBlocks& c) {
    return !c.built || c.ncols != ncols || c.nb != nb || c.wbits != wbits;
  };
  if (stale(L.cb)) build_col_blocks(L.csr(), ncols, L.cb, st, nb, wbits);
  if (!L.symmetric && stale(L.cb_t)) build_col_blocks(L.csr_t(), ncols, L.cb_t, st, nb, wbits);
  return L.cb.usable && L.cb.cbits && (L.symmetric || (L.cb_t.usable && L.cb_t.cbits));
}

// Window rows of the flat tiled SpMM: 64 (wbits 6).  Layer launches, round 5 sweeps
// (profiles/r05_tile_cfg4.jsonl, r05_tile_cfg5.jsonl): cfg4 (16 blocks, ~3 entries per row and
// block) 0.356 / 0.348 / 0.357 ms at windows of 32 / 64 / 128 rows; cfg5 (64 blocks, ~0.5)
// 5.13 / 4.36 / 4.79 ms -- longer runs per window and block until a wave's windows get too
// few to balance.  N2V2R_SPMM_WBITS (5..7) overrides (read per call).
int tile_wbits(const std::vector<std::unique_ptr<LayerDev>>& layers, int nb) {
  (void)layers;
  (void)nb;
  if (const char* e = std::getenv("N2V2R_SPMM_WBITS")) {
    const int v = std::atoi(e);
    if (v >= CB_WIN_BITS_MIN && v <= CB_WIN_BITS_MAX) return v;
  }
  return 6;
}

// A[:, own rows] of a partitioned layer as a CSR over rows_out (>= N) global rows, columns local:
// the transpose of the rank's rows of A^T (A's own columns), by the ingest's GPU transpose (the
// stable LSD radix sort of col << 32 | row keys over the column digits).  Stage 2 of the
// reduce-scatter form gathers from this rank's Z rows only.  One-off per layer.
void ensure_colcsr(LayerDev& L, int64_t ncols, int64_t rows_out, hipStream_t st, int64_t npad,
                   int W, int64_t rc) {
  if (rc <= 0 || rc >= npad) rc = 0;  // one chunk: the natural row order
  if (L.c_built && L.c_rows == rows_out && L.c_rc == rc) return;
  const CsrDev s = L.csr_t();
  const int64_t nnz = s.nnz;
  if (nnz > (int64_t)INT32_MAX)
    throw StatusFail{N2V2R_ERR_BAD_ARG, "a rank's layer block over 2^31 - 1 entries"};
  L.c_indptr.ensure(sizeof(int64_t) * (rows_out + 1));
  L.c_indices.ensure(sizeof(int32_t) * std::max<int64_t>(nnz, 1));
  if (!s.unit) L.c_data.ensure(sizeof(float) * std::max<int64_t>(nnz, 1));
  if (nnz == 0) {
    HIPCHK(n2v2r_launch_csr_from_sorted(nullptr, nullptr, nullptr, 0, rows_out,
                                        L.c_indptr.as<int64_t>(), nullptr, nullptr, st));
  } else {
    DevBuf keys[2], pay[2], hist, flag;
    for (int i = 0; i < 2; ++i) {
      keys[i].ensure(sizeof(uint64_t) * nnz);
      pay[i].ensure(sizeof(int32_t) * nnz);
    }
    flag.ensure(sizeof(unsigned) * 4, st);
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(unsigned) * 4, st));
    // (a unit A^T copy keeps no value stream; the scan's flags are not read here)
    HIPCHK(n2v2r_launch_csr_scan(s.indptr, s.indices, s.unit ? nullptr : s.data, s.n_rows,
                                 ncols, keys[0].as<uint64_t>(), pay[0].as<int32_t>(),
                                 flag.as<unsigned>(), st));
    if (rc > 0)
      HIPCHK(n2v2r_launch_chunk_major_keys(keys[0].as<uint64_t>(), nnz, npad, W, rc, st));
    hist.ensure(sizeof(uint32_t) * n2v2r_radix_hist_elems(nnz, 1));
    int bits = 1;
    const int64_t span = rc > 0 ? rows_out : ncols;
    while (bits < 31 && ((int64_t)1 << bits) < span) ++bits;
    int cur = 0;
    for (int sh = 32; sh < 32 + bits; sh += 8) {
      HIPCHK(n2v2r_launch_radix_pass(keys[cur].as<uint64_t>(), pay[cur].as<int32_t>(),
                                     keys[cur ^ 1].as<uint64_t>(), pay[cur ^ 1].as<int32_t>(),
                                     nnz, 1, sh, hist.as<uint32_t>(), st));
      cur ^= 1;
    }
    HIPCHK(n2v2r_launch_csr_from_sorted(keys[cur].as<uint64_t>(), pay[cur].as<int32_t>(), s.data,
                                        nnz, rows_out, L.c_indptr.as<int64_t>(),
                                        L.c_indices.as<int32_t>(),
                                        s.unit ? nullptr : L.c_data.as<float>(), st));
    HIPCHK(hipStreamSynchronize(st));  // the sort scratch dies here
  }
  L.c_nnz = nnz;
  L.c_rows = rows_out;
  L.c_rc = rc;
  L.c_built = true;
}

// ---- host CSR helpers -------------------------------------------------------------------
int host_threads() {
  return (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
}

// every value exactly 1.0f (an unweighted layer: its value array need not cross PCIe -- the
// device copy is filled with 1.0f instead); large layers in up to 16 host threads
bool host_all_ones(int64_t nnz, const float* dv) {
  auto ok = [&](int64_t p0, int64_t p1) {
    bool good = true;
    for (int64_t p = p0; p < p1; ++p) good &= dv[p] == 1.0f;
    return good;
  };
  int nt = host_threads();
  if (nnz < (int64_t)1 << 22) nt = 1;
  if (nt == 1) return ok(0, nnz);
  std::vector<char> res(nt, 1);
  const int64_t per = (nnz + nt - 1) / nt;
  parallel_chunks(nt, [&](int t) {
    const int64_t p0 = std::min<int64_t>(nnz, t * per);
    res[t] = ok(p0, std::min<int64_t>(nnz, p0 + per)) ? 1 : 0;
  });
  for (char c : res)
    if (!c) return false;
  return true;
}

// every column index in [0, n); large layers are checked in up to 16 host threads
bool host_indices_in_range(int64_t nnz, const int32_t* ix, int64_t n) {
  auto ok = [&](int64_t p0, int64_t p1) {
    bool good = true;
    for (int64_t p = p0; p < p1; ++p) good &= (ix[p] >= 0) & ((int64_t)ix[p] < n);
    return good;
  };
  int nt = host_threads();
  if (nnz < (int64_t)1 << 22) nt = 1;
  if (nt == 1) return ok(0, nnz);
  std::vector<char> res(nt, 1);
  const int64_t per = (nnz + nt - 1) / nt;
  parallel_chunks(nt, [&](int t) {
    const int64_t p0 = std::min<int64_t>(nnz, t * per);
    res[t] = ok(p0, std::min<int64_t>(nnz, p0 + per)) ? 1 : 0;
  });
  for (char c : res)
    if (!c) return false;
  return true;
}

// upload rows [r0, r0 + nr) of a CSR (global column indices kept) into (ip, ix, dv) buffers;
// returns whether every uploaded value is 1.0f (an unweighted graph: the SpMM skips values)
bool upload_rows(hipStream_t st, int64_t r0, int64_t nr, const int64_t* ip, const int32_t* ix,
                 const float* dv, DevBuf& dip, DevBuf& dix, DevBuf& ddv, int64_t& nnz_out) {
  const int64_t p0 = ip[r0], p1 = ip[r0 + nr];
  nnz_out = p1 - p0;
  const bool unit = host_all_ones(nnz_out, dv + p0);
  std::vector<int64_t> lip(nr + 1);
  for (int64_t r = 0; r <= nr; ++r) lip[r] = ip[r0 + r] - p0;
  dip.ensure(sizeof(int64_t) * (nr + 1));
  dix.ensure(sizeof(int32_t) * std::max<int64_t>(nnz_out, 1));
  ddv.ensure(sizeof(float) * std::max<int64_t>(nnz_out, 1));
  HIPCHK(hipMemcpyAsync(dip.p, lip.data(), sizeof(int64_t) * (nr + 1), hipMemcpyHostToDevice, st));
  if (nnz_out) {
    HIPCHK(hipMemcpyAsync(dix.p, ix + p0, sizeof(int32_t) * nnz_out, hipMemcpyHostToDevice, st));
    if (unit)  // (0x3F800000 = 1.0f)
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ddv.p, 0x3F800000, (size_t)nnz_out, st));
    else
      HIPCHK(hipMemcpyAsync(ddv.p, dv + p0, sizeof(float) * nnz_out, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // lip dies here
  return unit;
}

namespace {
inline uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
}  // namespace

// Multiset equality of {(r, c, v)} and {(c, r, v)} by two hash sums each (mod 2^64): a
// non-symmetric layer passes with probability ~2^-128.  Values compare by their bits (-0 and +0
// differ, which only makes a layer count as directed: the slower, always correct path).
bool host_csr_symmetric(int64_t n, const int64_t* ip, const int32_t* ix, const float* dv) {
  int nt = host_threads();
  const int64_t nnz = ip[n];
  if (nnz < (int64_t)1 << 20) nt = 1;
  std::vector<uint64_t> acc((size_t)nt * 4, 0);
  const int64_t per = (n + nt - 1) / nt;
  parallel_chunks(nt, [&](int t) {
    const int64_t r0 = std::min<int64_t>(n, t * per), r1 = std::min<int64_t>(n, r0 + per);
    uint64_t a1 = 0, a2 = 0, b1 = 0, b2 = 0;
    for (int64_t r = r0; r < r1; ++r)
      for (int64_t p = ip[r]; p < ip[r + 1]; ++p) {
        uint32_t vb;
        std::memcpy(&vb, dv + p, sizeof(vb));
        const uint64_t c = (uint32_t)ix[p], rr = (uint64_t)r;
        const uint64_t kf = (rr << 32) | c, kt = (c << 32) | rr;
        a1 += mix64(mix64(kf + 0x9E3779B97F4A7C15ull) ^ vb);
        b1 += mix64(mix64(kt + 0x9E3779B97F4A7C15ull) ^ vb);
        a2 += mix64(mix64(kf ^ 0xD1B54A32D192ED03ull) + ((uint64_t)vb << 17));
        b2 += mix64(mix64(kt ^ 0xD1B54A32D192ED03ull) + ((uint64_t)vb << 17));
      }
    acc[(size_t)t * 4 + 0] = a1;
    acc[(size_t)t * 4 + 1] = a2;
    acc[(size_t)t * 4 + 2] = b1;
    acc[(size_t)t * 4 + 3] = b2;
  });
  uint64_t s[4] = {0, 0, 0, 0};
  for (int t = 0; t < nt; ++t)
    for (int i = 0; i < 4; ++i) s[i] += acc[(size_t)t * 4 + i];
  return s[0] == s[2] && s[1] == s[3];
}

void host_transpose_rows(int64_t n, const int64_t* ip, const int32_t* ix, const float* dv,
                         int64_t r0, int64_t nr, std::vector<int64_t>& tip,
                         std::vector<int32_t>& tix, std::vector<float>& tdv) {
  tip.assign((size_t)nr + 1, 0);
  const uint64_t span = (uint64_t)nr;
  for (int64_t r = 0; r < n; ++r)
    for (int64_t p = ip[r]; p < ip[r + 1]; ++p) {
      const uint64_t c = (uint64_t)((int64_t)ix[p] - r0);
      if (c < span) ++tip[c + 1];
    }
  for (int64_t i = 0; i < nr; ++i) tip[i + 1] += tip[i];
  tix.resize((size_t)std::max<int64_t>(tip[nr], 1));
  tdv.resize((size_t)std::max<int64_t>(tip[nr], 1));
  std::vector<int64_t> pos(tip.begin(), tip.end() - 1);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t p = ip[r]; p < ip[r + 1]; ++p) {
      const uint64_t c = (uint64_t)((int64_t)ix[p] - r0);
      if (c < span) {
        const int64_t q = pos[c]++;
        tix[q] = (int32_t)r;
        tdv[q] = dv[p];
      }
    }
}

int set_layer_rows_directed(n2v2r_handle* h, int k, const int64_t* aip, const int32_t* aix,
                            const float* adv, const int64_t* tip, const int32_t* tix,
                            const float* tdv) {
  return guarded(h, [&]() -> int {
    const int64_t nr = h->nloc;
    if (k < 0 || k >= h->K || aip[0] != 0 || tip[0] != 0) return N2V2R_ERR_BAD_ARG;
    for (int64_t r = 0; r < nr; ++r)
      if (aip[r + 1] < aip[r]) {
        h->set_err("layer %d: indptr not monotone", k);
        return N2V2R_ERR_BAD_ARG;
      }
    if (!host_indices_in_range(aip[nr], aix, h->n)) {
      h->set_err("layer %d: column index out of range", k);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int j = 0; j < h->K; ++j)
      if (j != k && h->layers[j]->loaded && h->layers[j]->dense) {
        h->err = "layers must be all CSR or all dense";
        return N2V2R_ERR_BAD_ARG;
      }
    LayerDev& L = *h->layers[k];
    L.dense = false;
    L.loaded = false;
    L.drop_col_blocks();
    L.n_rows = nr;
    L.unit = upload_rows(h->stream, 0, nr, aip, aix, adv, L.indptr, L.indices, L.data, L.nnz);
    L.t_unit = upload_rows(h->stream, 0, nr, tip, tix, tdv, L.t_indptr, L.t_indices, L.t_data,
                           L.t_nnz);
    h->h2d_layer_bytes += 16 * (nr + 1) + (L.unit ? 4 : 8) * L.nnz + (L.t_unit ? 4 : 8) * L.t_nnz;
    L.symmetric = false;
    L.loaded = true;
    h->have_embedding = false;
    return N2V2R_OK;
  });
}
}  // namespace n2v2r_int

namespace {
// what the row pass of a correlation method reports (corr.hip)
struct CorrRows {
  unsigned bad = 0xFFFFFFFFu;     // the smallest bad row, or 0xFFFFFFFF
  int64_t fallback[2] = {0, -1};  // bicor rows with MAD = 0 (the Pearson row): count, smallest
};

bool corr_method_known(int method) {
  return method == N2V2R_COR_PEARSON || method == N2V2R_COR_SPEARMAN ||
         method == N2V2R_COR_BICOR;
}

// z (npad x n2v2r_corr_spad(s)) = the rows of e (n x s, on the device) standardised for `method`:
// Pearson by corr_standardise_kernel, Spearman by the same kernel on the rows' average ranks,
// bicor by corr_bicor_kernel.  flag: four device words of scratch.  The stream is synchronised
// on return (the rank buffer dies here).
CorrRows corr_standardise_rows(hipStream_t st, const double* e, int64_t n, int64_t s, int method,
                               double* z, unsigned* flag) {
  CorrRows out;
  DevBuf ranks;
  HIPCHK(hipMemsetAsync(flag, 0xFF, sizeof(unsigned), st));
  if (method == N2V2R_COR_BICOR) {
    HIPCHK(hipMemsetAsync(flag + 1, 0, sizeof(unsigned), st));
    HIPCHK(hipMemsetAsync(flag + 2, 0xFF, sizeof(unsigned), st));
    HIPCHK(n2v2r_launch_corr_bicor(e, n, s, z, flag, st));
  } else if (method == N2V2R_COR_SPEARMAN) {
    ranks.ensure_raw(sizeof(double) * n * s);
    HIPCHK(n2v2r_launch_corr_ranks(e, n, s, ranks.as<double>(), st));
    HIPCHK(n2v2r_launch_corr_standardise(ranks.as<double>(), n, s, z, flag, st));
  } else {
    HIPCHK(n2v2r_launch_corr_standardise(e, n, s, z, flag, st));
  }
  unsigned w[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(w, flag, sizeof(unsigned) * (method == N2V2R_COR_BICOR ? 3 : 1),
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  out.bad = w[0];
  if (method == N2V2R_COR_BICOR && w[1] > 0) {
    out.fallback[0] = (int64_t)w[1];
    out.fallback[1] = (int64_t)w[2];
  }
  return out;
}
}  // namespace

extern "C" {

int n2v2r_set_num_layers(n2v2r_handle* h, int num_layers, int64_t n) {
  if (h && h->multi()) return multi_set_num_layers(h, num_layers, n);
  return guarded(h, [&]() -> int {
    if (num_layers < 1 || n < 1 || n > (int64_t)INT32_MAX) {
      h->set_err("bad layer count %d or node count %lld", num_layers, (long long)n);
      return N2V2R_ERR_BAD_ARG;
    }
    if (num_layers > SPMM_MAX_LAYERS) {
      h->set_err("at most %d layers are supported", SPMM_MAX_LAYERS);
      return N2V2R_ERR_BAD_ARG;
    }
    h->K = num_layers;
    h->set_partition(n);
    h->layers.clear();
    for (int k = 0; k < num_layers; ++k) h->layers.emplace_back(new LayerDev());
    h->have_embedding = false;
    h->ncmp = h->ncols = 0;
    return N2V2R_OK;
  });
}

int n2v2r_set_layer_csr(n2v2r_handle* h, int k, int64_t n, int64_t nnz, const int64_t* indptr,
                        const int32_t* indices, const float* data, int symmetric) {
  if (h && h->multi()) return multi_set_layer_csr(h, k, n, nnz, indptr, indices, data, symmetric);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || n != h->n || nnz < 0 || !indptr || (nnz > 0 && (!indices || !data))) {
      h->set_err("bad CSR arguments for layer %d", k);
      return N2V2R_ERR_BAD_ARG;
    }
    if (indptr[0] != 0 || indptr[n] != nnz) {
      h->set_err("layer %d: indptr must start at 0 and end at nnz", k);
      return N2V2R_ERR_BAD_ARG;
    }
    // the GPU transpose (and the symmetry test built on it) sorts int32 entry indices: a layer
    // that needs it is limited to 2^31 - 1 entries; N2V2R_SYM_YES layers are not
    if (symmetric != N2V2R_SYM_YES && nnz > (int64_t)INT32_MAX) {
      h->set_err("layer %d: more than 2^31 - 1 entries need symmetric = N2V2R_SYM_YES (the GPU "
                 "transpose / symmetry test sorts int32 entry indices)", k);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int64_t r = 0; r < n; ++r)
      if (indptr[r + 1] < indptr[r]) {
        h->set_err("layer %d: indptr not monotone", k);
        return N2V2R_ERR_BAD_ARG;
      }
    for (int j = 0; j < h->K; ++j)
      if (j != k && h->layers[j]->loaded && h->layers[j]->dense) {
        h->err = "layers must be all CSR or all dense";
        return N2V2R_ERR_BAD_ARG;
      }
    LayerDev& L = *h->layers[k];
    L.dense = false;
    L.loaded = false;
    L.drop_col_blocks();
    L.n_rows = h->nloc;
    const hipStream_t st = h->stream;
    // the whole layer to HBM (on one GPU straight into the layer's buffers; a partitioned
    // handle keeps its row slice and the slice of the transpose)
    const bool whole = !h->comm;
    DevBuf gip, gix, gdv;
    DevBuf& dip = whole ? L.indptr : gip;
    DevBuf& dix = whole ? L.indices : gix;
    DevBuf& ddv = whole ? L.data : gdv;
    dip.ensure(sizeof(int64_t) * (n + 1));
    dix.ensure(sizeof(int32_t) * std::max<int64_t>(nnz, 1));
    ddv.ensure(sizeof(float) * std::max<int64_t>(nnz, 1));
    HIPCHK(hipMemcpyAsync(dip.p, indptr, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
    const bool ones = nnz > 0 && host_all_ones(nnz, data);  // unweighted: no value upload
    if (nnz) {
      HIPCHK(hipMemcpyAsync(dix.p, indices, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, st));
      if (ones)
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ddv.p, 0x3F800000, (size_t)nnz, st));
      else
        HIPCHK(hipMemcpyAsync(ddv.p, data, sizeof(float) * nnz, hipMemcpyHostToDevice, st));
    }
    h->h2d_layer_bytes += 8 * (n + 1) + (ones ? 4 : 8) * nnz;
    const bool need_t = symmetric != N2V2R_SYM_YES;
    DevBuf* keys = h->ing_keys;
    DevBuf* pay = h->ing_pay;
    DevBuf& hist = h->ing_hist;
    DevBuf& flag = h->ing_flag;
    flag.ensure_raw(sizeof(unsigned) * 4);
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(unsigned) * 4, st));
    if (need_t && nnz) {
      keys[0].ensure_raw(sizeof(uint64_t) * nnz);
      pay[0].ensure_raw(sizeof(int32_t) * nnz);
    }
    HIPCHK(n2v2r_launch_csr_scan(dip.as<int64_t>(), dix.as<int32_t>(), ddv.as<float>(), n, n,
                                 need_t && nnz ? keys[0].as<uint64_t>() : nullptr,
                                 need_t && nnz ? pay[0].as<int32_t>() : nullptr,
                                 flag.as<unsigned>(), st));
    unsigned fl = 0;
    HIPCHK(hipMemcpyAsync(&fl, flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (fl & 1u) {
      h->set_err("layer %d: column index out of range", k);
      return N2V2R_ERR_BAD_ARG;
    }
    const bool unit = !(fl & 2u);
    const bool sorted = !(fl & 4u);
    // A^T = the entries stably sorted by column (LSD radix over the column digits only)
    auto transpose = [&](const int64_t* ip_, const int32_t* ix_, const float* dv_, bool have_keys,
                         DevBuf& tp, DevBuf& tx, DevBuf& td) {
      tp.ensure(sizeof(int64_t) * (n + 1));
      tx.ensure(sizeof(int32_t) * std::max<int64_t>(nnz, 1));
      if (!unit) td.ensure(sizeof(float) * std::max<int64_t>(nnz, 1));
      if (nnz == 0) {
        HIPCHK(n2v2r_launch_csr_from_sorted(nullptr, nullptr, nullptr, 0, n, tp.as<int64_t>(),
                                            nullptr, nullptr, st));
        return;
      }
      keys[0].ensure_raw(sizeof(uint64_t) * nnz);
      pay[0].ensure_raw(sizeof(int32_t) * nnz);
      keys[1].ensure_raw(sizeof(uint64_t) * nnz);
      pay[1].ensure_raw(sizeof(int32_t) * nnz);
      if (!have_keys)
        HIPCHK(n2v2r_launch_csr_scan(ip_, ix_, dv_, n, n, keys[0].as<uint64_t>(),
                                     pay[0].as<int32_t>(), flag.as<unsigned>() + 1, st));
      hist.ensure_raw(sizeof(uint32_t) * n2v2r_radix_hist_elems(nnz, 1));
      int bits = 1;
      while (bits < 31 && ((int64_t)1 << bits) < n) ++bits;
      int cur = 0;
      for (int sh = 32; sh < 32 + bits; sh += 8) {
        HIPCHK(n2v2r_launch_radix_pass(keys[cur].as<uint64_t>(), pay[cur].as<int32_t>(),
                                       keys[cur ^ 1].as<uint64_t>(), pay[cur ^ 1].as<int32_t>(),
                                       nnz, 1, sh, hist.as<uint32_t>(), st));
        cur ^= 1;
      }
      HIPCHK(n2v2r_launch_csr_from_sorted(keys[cur].as<uint64_t>(), pay[cur].as<int32_t>(), dv_,
                                          nnz, n, tp.as<int64_t>(), tx.as<int32_t>(),
                                          unit ? nullptr : td.as<float>(), st));
    };
    bool sym = symmetric == N2V2R_SYM_YES;
    DevBuf gtp, gtx, gtd;
    DevBuf& tp = whole ? L.t_indptr : gtp;
    DevBuf& tx = whole ? L.t_indices : gtx;
    DevBuf& td = whole ? L.t_data : gtd;
    if (need_t) {
      transpose(dip.as<int64_t>(), dix.as<int32_t>(), ddv.as<float>(), true, tp, tx, td);
      if (symmetric == N2V2R_SYM_DETECT) {
        // unit layers compare their (absent) values as equal: both sides read A's values
        const float* tv = unit ? ddv.as<float>() : td.as<float>();
        HIPCHK(hipMemsetAsync(flag.as<unsigned>() + 2, 0, sizeof(unsigned), st));
        if (sorted) {
          HIPCHK(n2v2r_launch_csr_compare(dip.as<int64_t>(), dix.as<int32_t>(), ddv.as<float>(),
                                          tp.as<int64_t>(), tx.as<int32_t>(), tv, n, nnz,
                                          flag.as<unsigned>() + 2, st));
        } else {  // A's rows sorted = (A^T)^T
          DevBuf sp_, sx, sv;
          transpose(tp.as<int64_t>(), tx.as<int32_t>(), tv, false, sp_, sx, sv);
          HIPCHK(n2v2r_launch_csr_compare(sp_.as<int64_t>(), sx.as<int32_t>(),
                                          unit ? ddv.as<float>() : sv.as<float>(),
                                          tp.as<int64_t>(), tx.as<int32_t>(), tv, n, nnz,
                                          flag.as<unsigned>() + 2, st));
          HIPCHK(hipStreamSynchronize(st));
        }
        unsigned mism = 0;
        HIPCHK(hipMemcpyAsync(&mism, flag.as<unsigned>() + 2, sizeof(unsigned),
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        sym = mism == 0;
      }
    }
    HIPCHK(hipStreamSynchronize(st));  // the sort scratch dies here
    keys[0].release();
    keys[1].release();
    pay[0].release();
    pay[1].release();
    // this rank's rows of A and (not symmetric) of A^T
    auto slice = [&](DevBuf& sip, DevBuf& six, DevBuf& sdv, bool copy_values, DevBuf& oip,
                     DevBuf& oix, DevBuf& odv, int64_t& onnz) {
      int64_t p0 = 0, p1 = 0;
      HIPCHK(hipMemcpyAsync(&p0, sip.as<int64_t>() + h->row0, sizeof(int64_t),
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&p1, sip.as<int64_t>() + h->row0 + h->nloc, sizeof(int64_t),
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      onnz = p1 - p0;
      oip.ensure(sizeof(int64_t) * (h->nloc + 1));
      oix.ensure(sizeof(int32_t) * std::max<int64_t>(onnz, 1));
      odv.ensure(sizeof(float) * std::max<int64_t>(onnz, 1));
      HIPCHK(n2v2r_launch_csr_rebase(sip.as<int64_t>(), h->row0, h->nloc, oip.as<int64_t>(), st));
      if (onnz) {
        HIPCHK(hipMemcpyAsync(oix.p, six.as<int32_t>() + p0, sizeof(int32_t) * onnz,
                              hipMemcpyDeviceToDevice, st));
        if (copy_values)
          HIPCHK(hipMemcpyAsync(odv.p, sdv.as<float>() + p0, sizeof(float) * onnz,
                                hipMemcpyDeviceToDevice, st));
      }
      HIPCHK(hipStreamSynchronize(st));
    };
    if (whole) {
      L.nnz = nnz;
      L.t_nnz = nnz;
      if (sym) {
        L.t_indptr.release();
        L.t_indices.release();
        L.t_data.release();
      }
    } else {
      slice(gip, gix, gdv, true, L.indptr, L.indices, L.data, L.nnz);
      if (!sym) slice(gtp, gtx, gtd, !unit, L.t_indptr, L.t_indices, L.t_data, L.t_nnz);
    }
    L.unit = unit;
    L.t_unit = unit;
    L.symmetric = sym;
    L.loaded = true;
    h->have_embedding = false;
    return N2V2R_OK;
  });
}

int n2v2r_set_layer_dense(n2v2r_handle* h, int k, int64_t n, const float* A, int symmetric) {
  if (h && h->multi()) return multi_set_layer_dense(h, k, n, A, symmetric);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || n != h->n || !A) {
      h->set_err("bad dense arguments for layer %d", k);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int j = 0; j < h->K; ++j)
      if (j != k && h->layers[j]->loaded && !h->layers[j]->dense) {
        h->err = "layers must be all CSR or all dense";
        return N2V2R_ERR_BAD_ARG;
      }
    LayerDev& L = *h->layers[k];
    L.dense = true;
    L.n_rows = h->nloc;
    L.lda = (n + 63) / 64 * 64;
    const int64_t nl = std::max<int64_t>(h->nloc, 1);
    L.dA.ensure(sizeof(float) * nl * L.lda);
    HIPCHK(hipMemcpy2D(L.dA.p, sizeof(float) * L.lda, A + h->row0 * n, sizeof(float) * n,
                       sizeof(float) * n, h->nloc, hipMemcpyHostToDevice));
    bool sym = symmetric == N2V2R_SYM_YES;
    if (!sym) {
      // A^T rows [row0, row0 + nloc) = columns of A: a partitioned handle stages all of A once
      // (one GPU: the rows already uploaded are all of A)
      DevBuf full;
      const float* src = L.dA.as<float>();
      if (h->comm) {
        full.ensure(sizeof(float) * n * L.lda);
        HIPCHK(hipMemcpy2D(full.p, sizeof(float) * L.lda, A, sizeof(float) * n,
                           sizeof(float) * n, n, hipMemcpyHostToDevice));
        src = full.as<float>();
      }
      L.dAT.ensure(sizeof(float) * nl * L.lda);
      HIPCHK(n2v2r_launch_transpose(src + h->row0, L.lda, n, h->nloc, L.dAT.as<float>(), L.lda,
                                    h->stream));
      if (symmetric == N2V2R_SYM_DETECT) {
        DevBuf cnt;
        cnt.ensure(sizeof(unsigned long long));
        HIPCHK(n2v2r_launch_mismatch(L.dA.as<float>(), L.dAT.as<float>(), L.lda, h->nloc, n,
                                     cnt.as<unsigned long long>(), h->stream));
        unsigned long long mism = 0;
        HIPCHK(hipMemcpyAsync(&mism, cnt.p, sizeof(mism), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        sym = mism == 0;
      }
      HIPCHK(hipStreamSynchronize(h->stream));
      if (sym) L.dAT.release();
    }
    L.symmetric = sym;
    L.loaded = true;
    h->have_embedding = false;
    return N2V2R_OK;
  });
}

// Co-expression layer from its n x samples expression matrix (corr.hip): E is uploaded whole
// (8 n samples bytes, on every rank of a partitioned handle), standardised on the GPU, and this
// rank's rows of t(corrcoef(E)) are written straight into the layer's dA by the fused tile
// kernel.  The layer counts as not loaded from the first check on until the kernels succeeded.
// method: N2V2R_COR_*, the way the rows are standardised (corr_standardise_rows above); the tile
// product and everything after it are the same for all of them.
int n2v2r_set_layer_corr(n2v2r_handle* h, int k, int64_t n, int64_t samples, const double* E,
                         int kind, double power) {
  return n2v2r_set_layer_corr_method(h, k, n, samples, E, kind, power, N2V2R_COR_PEARSON, nullptr);
}

int n2v2r_set_layer_corr_method(n2v2r_handle* h, int k, int64_t n, int64_t samples,
                                const double* E, int kind, double power, int method,
                                int64_t* fallback) {
  if (h && h->multi())
    return multi_set_layer_corr(h, k, n, samples, E, kind, power, method, fallback);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || n != h->n || n < 1 || !E) {
      h->set_err("bad co-expression arguments for layer %d", k);
      return N2V2R_ERR_BAD_ARG;
    }
    LayerDev& L = *h->layers[k];
    L.loaded = false;
    h->have_embedding = false;
    if (samples < 2) {
      h->set_err("layer %d: a correlation needs at least 2 samples, got %lld", k,
                 (long long)samples);
      return N2V2R_ERR_BAD_ARG;
    }
    if (kind != N2V2R_CORR_UNSIGNED && kind != N2V2R_CORR_SIGNED &&
        kind != N2V2R_CORR_SIGNED_HYBRID && kind != N2V2R_CORR_RAW) {
      h->set_err("layer %d: unknown correlation kind %d", k, kind);
      return N2V2R_ERR_BAD_ARG;
    }
    if (!std::isfinite(power) || power < 1.0) {
      h->set_err("layer %d: power must be finite and >= 1, got %g", k, power);
      return N2V2R_ERR_BAD_ARG;
    }
    if (kind == N2V2R_CORR_RAW && power != 1.0) {
      h->set_err("layer %d: a raw correlation layer takes power 1 (r may be negative), got %g", k,
                 power);
      return N2V2R_ERR_BAD_ARG;
    }
    if (!corr_method_known(method)) {
      h->set_err("layer %d: unknown correlation method %d", k, method);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int j = 0; j < h->K; ++j)
      if (j != k && h->layers[j]->loaded && !h->layers[j]->dense) {
        h->err = "layers must be all CSR or all dense";
        return N2V2R_ERR_BAD_ARG;
      }
    hipStream_t st = h->stream;  // (n <= 2^31 - 1: n2v2r_set_num_layers)
    const int64_t npad = (n + 63) / 64 * 64, sp = n2v2r_corr_spad(samples);
    DevBuf e, z;  // (the kernels write every element of z)
    e.ensure_raw(sizeof(double) * n * samples);
    z.ensure_raw(sizeof(double) * npad * sp);
    DevBuf& flag = h->ing_flag;
    flag.ensure_raw(sizeof(unsigned) * 4);
    HIPCHK(hipMemcpyAsync(e.p, E, sizeof(double) * n * samples, hipMemcpyHostToDevice, st));
    h->h2d_layer_bytes += 8 * n * samples;
    const CorrRows rows = corr_standardise_rows(st, e.as<double>(), n, samples, method,
                                                z.as<double>(), flag.as<unsigned>());
    if (rows.bad != 0xFFFFFFFFu) {
      h->set_err("layer %d: row %u of the expression matrix holds a non-finite value or is "
                 "constant (zero variance): its correlations are undefined", k, rows.bad);
      return N2V2R_ERR_BAD_ARG;
    }
    L.dense = true;
    L.n_rows = h->nloc;
    L.lda = npad;
    L.dA.ensure(sizeof(float) * std::max<int64_t>(h->nloc, 1) * L.lda);
    L.dAT.release();
    HIPCHK(n2v2r_launch_corr_tiles(z.as<double>(), samples, n, h->row0, h->nloc, L.dA.as<float>(),
                                   L.lda, kind, power, st));
    HIPCHK(hipStreamSynchronize(st));  // e and z die here
    L.symmetric = true;
    L.loaded = true;
    if (fallback) std::copy(rows.fallback, rows.fallback + 2, fallback);
    return N2V2R_OK;
  });
}

// the smallest fp32 >= v (v not NaN): for fp32 a, a >= tf_ceil32(v) exactly when !(a < v) in fp64
static float tf_ceil32(double v) {
  float f = (float)v;  // (round to nearest; +-inf beyond the fp32 range)
  if ((double)f < v) f = std::nextafterf(f, INFINITY);
  return f;
}
static double tf_key_value(uint32_t key) {
  const uint32_t bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  float f;
  std::memcpy(&f, &bits, sizeof(f));
  return (double)f;
}

// one histogram pass of the radix select over this handle's rows, summed over the ranks:
// host[0 .. 255] the digit counts, host[256] the NaNs (pass 0)
static void tf_hist_pass(n2v2r_handle* h, const float* A, int64_t count, int absolute, float lim,
                         int pass, uint32_t prefix, unsigned long long* host) {
  unsigned long long* scr = h->tf_scr.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(scr, 0, sizeof(unsigned long long) * 257, h->stream));
  HIPCHK(n2v2r_launch_tf_hist(A, count, absolute, lim, pass, prefix, scr, h->stream));
  if (h->comm) h->comm->allreduce_sum_u64(scr, 257, h->stream);
  HIPCHK(hipMemcpyAsync(host, scr, sizeof(unsigned long long) * 257, hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
}

// network_transform of a dense layer in place (transform.hip).  Nothing is written before the
// cut is known: the threshold is a predicate of the select passes.  Every decision below is taken
// on numbers already reduced over the ranks, so all ranks of a partitioned handle take the same
// one (the error returns included) and run the same collectives.
int n2v2r_transform_layer(n2v2r_handle* h, int k, int flags, double threshold,
                          double top_percent_keep, n2v2r_transform_stats* stats) {
  if (h && h->multi())
    return multi_transform_layer(h, k, flags, threshold, top_percent_keep, stats);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !h->layers[k]->loaded) {
      h->set_err("transform_layer: layer %d is not loaded", k);
      return N2V2R_ERR_BAD_ARG;
    }
    LayerDev& L = *h->layers[k];
    if (!L.dense) {
      h->set_err("transform_layer: layer %d is stored as CSR; transform sparse layers on the host "
                 "with node2vec2rank_amd.ingest.transform before loading them", k);
      return N2V2R_ERR_BAD_ARG;
    }
    if (flags & ~(N2V2R_TF_ABSOLUTE | N2V2R_TF_BINARIZE | N2V2R_TF_THRESHOLD)) {
      h->set_err("transform_layer: unknown flag bits in %d", flags);
      return N2V2R_ERR_BAD_ARG;
    }
    if (!std::isfinite(top_percent_keep) || top_percent_keep < 0.0 || top_percent_keep > 100.0) {
      h->set_err("transform_layer: top_percent_keep must lie in [0, 100], got %g",
                 top_percent_keep);
      return N2V2R_ERR_BAD_ARG;
    }
    const bool thr = (flags & N2V2R_TF_THRESHOLD) != 0;
    if (thr && std::isnan(threshold)) {
      h->err = "transform_layer: the threshold is NaN";
      return N2V2R_ERR_BAD_ARG;
    }
    const int absolute = (flags & N2V2R_TF_ABSOLUTE) ? 1 : 0;
    const float lim = thr ? tf_ceil32(threshold) : -INFINITY;
    hipStream_t st = h->stream;
    const float* A = L.dA.as<float>();
    const int64_t count = h->nloc * L.lda;
    // [0, 256) digit counts, [256] NaNs, [257] complemented min key, [258] survivors
    h->tf_scr.ensure_raw(sizeof(unsigned long long) * 260);
    unsigned long long* scr = h->tf_scr.as<unsigned long long>();
    unsigned long long host[260];

    int64_t m = 0, lo = 0, hi = 0, rank = 0, below = 0;
    double g = 0.0;
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
      tf_hist_pass(h, A, count, absolute, lim, pass, prefix, host);
      if (pass == 0) {
        if (host[256]) {
          h->set_err("transform_layer: layer %d holds %llu NaN entries", k, host[256]);
          return N2V2R_ERR_BAD_ARG;
        }
        for (int b = 0; b < 256; ++b) m += (int64_t)host[b];
        if (m == 0) {
          h->set_err("transform_layer: layer %d has no non-zero entry left%s", k,
                     thr ? " at this threshold" : "");
          return N2V2R_ERR_BAD_ARG;
        }
        // np.percentile's "linear" method
        const double q = 100.0 - top_percent_keep;
        const double pos = (double)(m - 1) * (q / 100.0);
        lo = std::min<int64_t>((int64_t)std::floor(pos), m - 1);
        g = pos - (double)lo;
        hi = std::min<int64_t>(lo + 1, m - 1);
        rank = lo;
      }
      int b = 0;
      for (; b < 255 && rank >= (int64_t)host[b]; ++b) {
        rank -= (int64_t)host[b];
        below += (int64_t)host[b];
      }
      if (rank >= (int64_t)host[b]) {
        h->err = "transform_layer: the digit histogram does not hold the order statistic";
        return N2V2R_ERR_INTERNAL;
      }
      prefix = (prefix << 8) | (uint32_t)b;
      if (pass == 3) below += (int64_t)host[b];  // now: the alive entries <= x
    }
    const uint32_t xkey = prefix;
    uint32_t ykey = xkey;
    if (hi > lo && below <= lo + 1) {  // the hi-th smallest lies above x
      HIPCHK(hipMemsetAsync(scr + 257, 0, sizeof(unsigned long long), st));
      HIPCHK(n2v2r_launch_tf_min(A, count, absolute, lim, xkey, scr + 257, st));
      if (h->comm) h->comm->allreduce_max_u64(scr + 257, 1, st);
      HIPCHK(hipMemcpyAsync(host, scr + 257, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            st));
      HIPCHK(hipStreamSynchronize(st));
      if (host[0] == 0 || host[0] > 0xFFFFFFFFull) {
        h->err = "transform_layer: no alive entry above the first order statistic";
        return N2V2R_ERR_INTERNAL;
      }
      ykey = ~(uint32_t)host[0];
    }
    const double x = tf_key_value(xkey), y = tf_key_value(ykey), d = y - x;
    const double cut = g < 0.5 ? x + d * g : y - d * (1.0 - g);
    // `a < cut` is false for a NaN cut (infinite order statistics): nothing more dies
    const float lim2 = std::isnan(cut) ? lim : std::max(lim, tf_ceil32(cut));

    h->have_embedding = false;
    HIPCHK(hipMemsetAsync(scr + 258, 0, sizeof(unsigned long long), st));
    HIPCHK(n2v2r_launch_tf_apply(L.dA.as<float>(), count, absolute, lim2,
                                 (flags & N2V2R_TF_BINARIZE) ? 1 : 0, scr + 258, st));
    if (!L.symmetric)
      HIPCHK(n2v2r_launch_tf_apply(L.dAT.as<float>(), count, absolute, lim2,
                                   (flags & N2V2R_TF_BINARIZE) ? 1 : 0, nullptr, st));
    if (h->comm) h->comm->allreduce_sum_u64(scr + 258, 1, st);
    HIPCHK(hipMemcpyAsync(host, scr + 258, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (stats) {
      stats->nonzero = m;
      stats->kept = (int64_t)host[0];
      stats->cut = cut;
    }
    return N2V2R_OK;
  });
}

// Topological overlap of a symmetric dense layer (tom.hip) into the handle's scratch buffer, which
// then changes places with the layer's dA.  A partitioned rank gathers every band into a full
// copy first (bands of npad rows, rank r's at row r npad = its row0; a shorter last band is sent
// from a zero-padded staging copy) and computes the tiles that meet its own band.  Every decision
// that is not the same on all ranks by construction (the counts, and whether some rank keeps an
// A^T copy) is taken on numbers summed over the ranks, so all ranks return alike and run the same
// collectives.
int n2v2r_tom_layer(n2v2r_handle* h, int k, int type) {
  if (h && h->multi()) return multi_tom_layer(h, k, type);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !h->layers[k]->loaded) {
      h->set_err("tom_layer: layer %d is not loaded", k);
      return N2V2R_ERR_BAD_ARG;
    }
    LayerDev& L = *h->layers[k];
    if (!L.dense) {
      h->set_err("tom_layer: layer %d is stored as CSR; the topological overlap is dense: load "
                 "the layer with dense storage", k);
      return N2V2R_ERR_BAD_ARG;
    }
    if (type != N2V2R_TOM_UNSIGNED && type != N2V2R_TOM_SIGNED) {
      h->set_err("tom_layer: unknown type %d", type);
      return N2V2R_ERR_BAD_ARG;
    }
    hipStream_t st = h->stream;
    const int64_t n = h->n, lda = L.lda;
    // [0] NaNs, [1] entries outside the type's range, [2] ranks that keep an A^T copy
    h->tf_scr.ensure_raw(sizeof(unsigned long long) * 260);
    unsigned long long* scr = h->tf_scr.as<unsigned long long>();
    unsigned long long host[3] = {0, 0, L.symmetric ? 0ull : 1ull};
    HIPCHK(hipMemcpyAsync(scr, host, sizeof(host), hipMemcpyHostToDevice, st));
    HIPCHK(n2v2r_launch_tom_check(L.dA.as<float>(), h->nloc, lda, n, type, scr, st));
    if (h->comm) h->comm->allreduce_sum_u64(scr, 3, st);
    HIPCHK(hipMemcpyAsync(host, scr, sizeof(host), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (host[2]) {
      h->set_err("tom_layer: layer %d is directed (it keeps an A^T copy); the topological overlap "
                 "is defined for symmetric adjacencies", k);
      return N2V2R_ERR_BAD_ARG;
    }
    if (host[0]) {
      h->set_err("tom_layer: layer %d holds %llu NaN entries", k, host[0]);
      return N2V2R_ERR_BAD_ARG;
    }
    if (host[1]) {
      h->set_err("tom_layer: layer %d holds %llu entries outside the range %s of the %s overlap",
                 k, host[1], type == N2V2R_TOM_SIGNED ? "[-1, 1]" : "[0, 1]",
                 type == N2V2R_TOM_SIGNED ? "signed" : "unsigned");
      return N2V2R_ERR_BAD_ARG;
    }
    DevBuf full, stage, ksum;
    const float* A = L.dA.as<float>();
    if (h->comm) {
      const size_t band = sizeof(float) * (size_t)h->npad * lda;
      full.ensure_raw(band * h->world);
      const void* send = L.dA.p;
      if (h->nloc < h->npad) {
        stage.ensure(band, st);
        if (h->nloc > 0)
          HIPCHK(hipMemcpyAsync(stage.p, L.dA.p, sizeof(float) * (size_t)h->nloc * lda,
                                hipMemcpyDeviceToDevice, st));
        send = stage.p;
      }
      h->comm->allgather(send, full.p, band, st);
      A = full.as<float>();
    }
    ksum.ensure_raw(sizeof(double) * n);
    h->tom_out.ensure_raw(sizeof(float) * std::max<int64_t>(h->nloc, 1) * lda);
    HIPCHK(n2v2r_launch_tom_rowsum(A, lda, n, type, ksum.as<double>(), st));
    HIPCHK(n2v2r_launch_tom_tiles(A, lda, n, ksum.as<double>(), type, h->row0, h->nloc,
                                  h->tom_out.as<float>(), st));
    HIPCHK(hipStreamSynchronize(st));  // full, stage and ksum die here
    h->have_embedding = false;
    L.dA.swap(h->tom_out);
    return N2V2R_OK;
  });
}

}  // extern "C"

namespace {
// one matrix of a layer (its dA or dAT rows) on its way to CSR
struct CsrBuild {
  DevBuf ip, ix, dv;
  int64_t nnz = 0;
  bool unit = true;
};

// row pointers of the stored entries of the handle's rows of A (nloc x lda): b.ip, b.nnz, b.unit.
// cnt: scratch of the per-row counts
void sparsify_count(n2v2r_handle* h, const float* A, int64_t lda, DevBuf& cnt, CsrBuild& b) {
  hipStream_t st = h->stream;
  const int64_t nr = h->nloc;
  cnt.ensure_raw(sizeof(int64_t) * std::max<int64_t>(nr, 1));
  b.ip.ensure_raw(sizeof(int64_t) * (nr + 1));
  h->ing_flag.ensure_raw(sizeof(unsigned) * 4);
  unsigned* flag = h->ing_flag.as<unsigned>();
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned), st));
  HIPCHK(n2v2r_launch_dense_row_count(A, nr, lda, h->n, cnt.as<int64_t>(), flag, st));
  HIPCHK(n2v2r_launch_row_scan(cnt.as<int64_t>(), nr, b.ip.as<int64_t>(), st));
  unsigned fl = 0;
  int64_t total = 0;
  HIPCHK(hipMemcpyAsync(&fl, flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&total, b.ip.as<int64_t>() + nr, sizeof(int64_t), hipMemcpyDeviceToHost,
                        st));
  HIPCHK(hipStreamSynchronize(st));
  b.nnz = total;
  b.unit = !(fl & 1u);
}

// the refusals n2v2r_layers_to_csr and n2v2r_count_layer_nonzeros share (nothing changed)
int sparsify_refusal(n2v2r_handle* h, const char* what) {
  if (h->K < 1 || h->layers.empty()) {
    h->set_err("%s: no layers set", what);
    return N2V2R_ERR_BAD_ARG;
  }
  for (int k = 0; k < h->K; ++k)
    if (!h->layers[k]->loaded) {
      h->set_err("%s: layer %d is not loaded", what, k);
      return N2V2R_ERR_BAD_ARG;
    }
  if (!h->layers[0]->dense) {
    h->set_err("%s: the layers of this handle are already CSR", what);
    return N2V2R_ERR_BAD_ARG;
  }
  return N2V2R_OK;
}

// the loaded CSR layer k's A (or A^T) rows for the read-back; nullptr with the error set
const LayerDev* csr_layer_for_read(n2v2r_handle* h, int k, int transpose) {
  if (k < 0 || k >= h->K || !h->layers[k]->loaded || h->layers[k]->dense) {
    h->set_err("get_layer_csr: layer %d is not a loaded CSR layer", k);
    return nullptr;
  }
  if (transpose && h->layers[k]->symmetric) {
    h->set_err("get_layer_csr: layer %d is symmetric: it keeps no A^T copy", k);
    return nullptr;
  }
  return h->layers[k].get();
}
}  // namespace

extern "C" {

// Every dense layer to CSR in HBM (sparsify.hip).  Counts first, then every allocation, then the
// compaction kernels, all into buffers of this call; the layers change only after every kernel
// has succeeded on every rank (the failure status is reduced over the ranks before the commit),
// so a refused or failed call leaves the dense layers as they were.
int n2v2r_layers_to_csr(n2v2r_handle* h, int64_t* nnz) {
  if (h && h->multi()) return multi_layers_to_csr(h, nnz);
  return guarded(h, [&]() -> int {
    if (const int st = sparsify_refusal(h, "layers_to_csr")) return st;
    const int K = h->K;
    hipStream_t st = h->stream;
    DevBuf red;  // [0, K) this rank's counts, [K] its status
    if (h->comm) red.ensure_raw(sizeof(unsigned long long) * (K + 1));
    std::vector<CsrBuild> a(K), t(K);
    int fail = N2V2R_OK;
    std::string why;
    try {
      DevBuf cnt;
      for (int k = 0; k < K; ++k) {
        const LayerDev& L = *h->layers[k];
        sparsify_count(h, L.dA.as<float>(), L.lda, cnt, a[k]);
        if (!L.symmetric) sparsify_count(h, L.dAT.as<float>(), L.lda, cnt, t[k]);
      }
      for (int k = 0; k < K; ++k)
        for (CsrBuild* b : {&a[k], &t[k]}) {
          if (b == &t[k] && h->layers[k]->symmetric) continue;
          b->ix.ensure_raw(sizeof(int32_t) * std::max<int64_t>(b->nnz, 1));
          b->dv.ensure_raw(sizeof(float) * std::max<int64_t>(b->nnz, 1));
        }
      for (int k = 0; k < K; ++k) {
        const LayerDev& L = *h->layers[k];
        for (CsrBuild* b : {&a[k], &t[k]}) {
          const bool tr = b == &t[k];
          if (tr && L.symmetric) continue;
          if (b->unit && b->nnz)  // (0x3F800000 = 1.0f: the values of an unweighted layer)
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b->dv.p, 0x3F800000, (size_t)b->nnz, st));
          HIPCHK(n2v2r_launch_dense_row_compact((tr ? L.dAT : L.dA).as<float>(), h->nloc, L.lda,
                                                h->n, b->ip.as<int64_t>(), b->ix.as<int32_t>(),
                                                b->unit ? nullptr : b->dv.as<float>(), st));
        }
      }
      HIPCHK(hipStreamSynchronize(st));
    } catch (const StatusFail& sf) {
      fail = sf.code;
      why = sf.msg;
      (void)hipGetLastError();
    } catch (const HipFail& hf) {
      fail = N2V2R_ERR_HIP;
      why = std::string("HIP error (") + hipGetErrorString(hf.e) + ") at " + hf.where;
      (void)hipGetLastError();
    }
    std::vector<unsigned long long> tot(K + 1);
    for (int k = 0; k < K; ++k) tot[k] = fail ? 0ull : (unsigned long long)a[k].nnz;
    tot[K] = (unsigned long long)fail;
    if (h->comm) {  // the global counts, and one status for every rank
      unsigned long long* r = red.as<unsigned long long>();
      HIPCHK(hipMemcpyAsync(r, tot.data(), sizeof(unsigned long long) * (K + 1),
                            hipMemcpyHostToDevice, st));
      h->comm->allreduce_sum_u64(r, K, st);
      h->comm->allreduce_max_u64(r + K, 1, st);
      HIPCHK(hipMemcpyAsync(tot.data(), r, sizeof(unsigned long long) * (K + 1),
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (tot[K] != N2V2R_OK) {
      if (fail)
        h->err = "layers_to_csr: " + why;
      else
        h->set_err("layers_to_csr: another rank failed (status %d); nothing was converted",
                   (int)tot[K]);
      return fail ? fail : (int)tot[K];
    }
    for (int k = 0; k < K; ++k) {
      LayerDev& L = *h->layers[k];
      L.drop_col_blocks();
      L.indptr.swap(a[k].ip);
      L.indices.swap(a[k].ix);
      L.data.swap(a[k].dv);
      L.nnz = a[k].nnz;
      L.unit = a[k].unit;
      if (L.symmetric) {
        L.t_indptr.release();
        L.t_indices.release();
        L.t_data.release();
        L.t_nnz = L.nnz;
        L.t_unit = L.unit;
      } else {
        L.t_indptr.swap(t[k].ip);
        L.t_indices.swap(t[k].ix);
        L.t_data.swap(t[k].dv);
        L.t_nnz = t[k].nnz;
        L.t_unit = t[k].unit;
      }
      L.n_rows = h->nloc;
      L.dense = false;
      L.dA.release();
      L.dAT.release();
      if (nnz) nnz[k] = (int64_t)tot[k];
    }
    h->tom_out.release();
    h->dense_work.release();
    h->dense_work_elems = 0;
    h->have_embedding = false;
    return N2V2R_OK;
  });
}

// the count pass of n2v2r_layers_to_csr alone: nothing changes
int n2v2r_count_layer_nonzeros(n2v2r_handle* h, int64_t* nnz) {
  if (h && h->multi()) return multi_count_layer_nonzeros(h, nnz);
  return guarded(h, [&]() -> int {
    if (!nnz) {
      h->err = "count_layer_nonzeros: null output buffer";
      return N2V2R_ERR_BAD_ARG;
    }
    if (const int st = sparsify_refusal(h, "count_layer_nonzeros")) return st;
    const int K = h->K;
    hipStream_t st = h->stream;
    std::vector<unsigned long long> tot(K);
    DevBuf cnt;
    for (int k = 0; k < K; ++k) {
      CsrBuild b;
      sparsify_count(h, h->layers[k]->dA.as<float>(), h->layers[k]->lda, cnt, b);
      tot[k] = (unsigned long long)b.nnz;
    }
    if (h->comm) {
      DevBuf red;
      red.ensure_raw(sizeof(unsigned long long) * K);
      unsigned long long* r = red.as<unsigned long long>();
      HIPCHK(hipMemcpyAsync(r, tot.data(), sizeof(unsigned long long) * K, hipMemcpyHostToDevice,
                            st));
      h->comm->allreduce_sum_u64(r, K, st);
      HIPCHK(hipMemcpyAsync(tot.data(), r, sizeof(unsigned long long) * K, hipMemcpyDeviceToHost,
                            st));
      HIPCHK(hipStreamSynchronize(st));
    }
    for (int k = 0; k < K; ++k) nnz[k] = (int64_t)tot[k];
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): a CSR layer's local rows back on the host
int n2v2r_get_layer_csr_nnz(n2v2r_handle* h, int k, int transpose, int64_t* nnz) {
  if (h && h->multi()) return multi_get_layer_csr_nnz(h, k, transpose, nnz);
  return guarded(h, [&]() -> int {
    const LayerDev* L = nnz ? csr_layer_for_read(h, k, transpose) : nullptr;
    if (!L) {
      if (!nnz) h->err = "get_layer_csr_nnz: null output";
      return N2V2R_ERR_BAD_ARG;
    }
    *nnz = transpose ? L->t_nnz : L->nnz;
    return N2V2R_OK;
  });
}

int n2v2r_get_layer_csr(n2v2r_handle* h, int k, int transpose, int64_t* indptr, int32_t* indices,
                        float* data) {
  if (h && h->multi()) return multi_get_layer_csr(h, k, transpose, indptr, indices, data);
  return guarded(h, [&]() -> int {
    const LayerDev* L = indptr ? csr_layer_for_read(h, k, transpose) : nullptr;
    if (!L) {
      if (!indptr) h->err = "get_layer_csr: null output buffer";
      return N2V2R_ERR_BAD_ARG;
    }
    const CsrDev c = transpose ? L->csr_t() : L->csr();
    if (c.nnz > 0 && (!indices || !data)) {
      h->err = "get_layer_csr: null output buffer";
      return N2V2R_ERR_BAD_ARG;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(indptr, c.indptr, sizeof(int64_t) * (c.n_rows + 1), hipMemcpyDeviceToHost));
    if (c.nnz > 0) {
      HIPCHK(hipMemcpy(indices, c.indices, sizeof(int32_t) * c.nnz, hipMemcpyDeviceToHost));
      if (c.unit)  // (an unweighted layer may keep no value stream)
        std::fill(data, data + c.nnz, 1.0f);
      else
        HIPCHK(hipMemcpy(data, c.data, sizeof(float) * c.nnz, hipMemcpyDeviceToHost));
    }
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): one kernel of the conversion alone, timed with HIP events
int n2v2r_bench_sparsify_pass(n2v2r_handle* h, int k, int which, int reps, double* avg_ms,
                              double* bytes) {
  return guarded(h, [&]() -> int {
    if (h->multi() || h->comm || k < 0 || k >= h->K || !h->layers[k]->loaded ||
        !h->layers[k]->dense || which < 0 || which > 1 || reps < 1 || !avg_ms) {
      h->err = "bench_sparsify_pass: a loaded dense layer of a one-GPU handle, which in [0, 1], "
               "reps >= 1";
      return N2V2R_ERR_BAD_ARG;
    }
    const LayerDev& L = *h->layers[k];
    hipStream_t st = h->stream;
    const float* A = L.dA.as<float>();
    DevBuf cnt;
    CsrBuild b;
    sparsify_count(h, A, L.lda, cnt, b);
    b.ix.ensure_raw(sizeof(int32_t) * std::max<int64_t>(b.nnz, 1));
    b.dv.ensure_raw(sizeof(float) * std::max<int64_t>(b.nnz, 1));
    unsigned* flag = h->ing_flag.as<unsigned>();
    auto launch = [&]() {
      if (which == 0)
        return n2v2r_launch_dense_row_count(A, h->nloc, L.lda, h->n, cnt.as<int64_t>(), flag, st);
      return n2v2r_launch_dense_row_compact(A, h->nloc, L.lda, h->n, b.ip.as<int64_t>(),
                                            b.ix.as<int32_t>(),
                                            b.unit ? nullptr : b.dv.as<float>(), st);
    };
    HIPCHK(launch());  // warm-up
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    // one event pair around `reps` launches back to back, as tools/stream_ceiling.hip times its
    // kernels
    hipError_t err = hipEventRecord(e0, st);
    for (int r = 0; r < reps && err == hipSuccess; ++r) err = launch();
    if (err == hipSuccess) err = hipEventRecord(e1, st);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) throw HipFail{err, "bench_sparsify_pass"};
    *avg_ms = (double)ms / reps;
    if (bytes) *bytes = 4.0 * (double)h->nloc * (double)L.lda;
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): tom_tile_kernel alone, one HIP event pair per launch
int n2v2r_bench_tom_tiles(n2v2r_handle* h, int k, int type, int reps, double* ms, double* flop) {
  return guarded(h, [&]() -> int {
    if (h->multi() || h->comm || k < 0 || k >= h->K || !h->layers[k]->loaded ||
        !h->layers[k]->dense || !h->layers[k]->symmetric || reps < 1 || !ms ||
        (type != N2V2R_TOM_UNSIGNED && type != N2V2R_TOM_SIGNED)) {
      h->err = "bench_tom_tiles: a loaded symmetric dense layer of a one-GPU handle, a known "
               "type, reps >= 1";
      return N2V2R_ERR_BAD_ARG;
    }
    LayerDev& L = *h->layers[k];
    hipStream_t st = h->stream;
    const int64_t n = h->n;
    DevBuf ksum;
    ksum.ensure_raw(sizeof(double) * n);
    h->tom_out.ensure_raw(sizeof(float) * n * L.lda);
    HIPCHK(n2v2r_launch_tom_rowsum(L.dA.as<float>(), L.lda, n, type, ksum.as<double>(), st));
    auto launch = [&]() {
      return n2v2r_launch_tom_tiles(L.dA.as<float>(), L.lda, n, ksum.as<double>(), type, 0, n,
                                    h->tom_out.as<float>(), st);
    };
    HIPCHK(launch());  // warm-up
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    hipError_t err = hipSuccess;
    for (int r = 0; r < reps && err == hipSuccess; ++r) {
      err = hipEventRecord(e0, st);
      if (err == hipSuccess) err = launch();
      if (err == hipSuccess) err = hipEventRecord(e1, st);
      if (err == hipSuccess) err = hipEventSynchronize(e1);
      float t = 0.f;
      if (err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
      ms[r] = (double)t;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) throw HipFail{err, "bench_tom_tiles"};
    if (flop) {  // the tiles computed: the upper triangle of 64 x 64 tiles, k over all of lda
      const double nt = (double)(L.lda / 64);
      *flop = nt * (nt + 1.0) / 2.0 * 2.0 * 64.0 * 64.0 * (double)L.lda;
    }
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): one kernel of the transform alone, timed with HIP events
int n2v2r_bench_transform_pass(n2v2r_handle* h, int k, int which, int flags, double threshold,
                               int reps, double* avg_ms, double* bytes) {
  return guarded(h, [&]() -> int {
    if (h->multi() || h->comm || k < 0 || k >= h->K || !h->layers[k]->loaded ||
        !h->layers[k]->dense || which < 0 || which > 5 || reps < 1 || !avg_ms ||
        ((flags & N2V2R_TF_THRESHOLD) && std::isnan(threshold))) {
      h->err = "bench_transform_pass: a loaded dense layer of a one-GPU handle, which in [0, 5], "
               "reps >= 1";
      return N2V2R_ERR_BAD_ARG;
    }
    LayerDev& L = *h->layers[k];
    const int absolute = (flags & N2V2R_TF_ABSOLUTE) ? 1 : 0;
    const float lim = (flags & N2V2R_TF_THRESHOLD) ? tf_ceil32(threshold) : -INFINITY;
    hipStream_t st = h->stream;
    float* A = L.dA.as<float>();
    const int64_t count = h->nloc * L.lda;
    h->tf_scr.ensure_raw(sizeof(unsigned long long) * 260);
    unsigned long long* scr = h->tf_scr.as<unsigned long long>();
    unsigned long long host[260];
    // the digits of the median alive key, as far as the timed pass needs them
    uint32_t prefix = 0;
    int64_t rank = 0;
    for (int pass = 0; pass < std::min(which, 4); ++pass) {
      tf_hist_pass(h, A, count, absolute, lim, pass, prefix, host);
      if (pass == 0) {
        int64_t m = 0;
        for (int b = 0; b < 256; ++b) m += (int64_t)host[b];
        rank = m / 2;
      }
      int b = 0;
      for (; b < 255 && rank >= (int64_t)host[b]; ++b) rank -= (int64_t)host[b];
      prefix = (prefix << 8) | (uint32_t)b;
    }
    auto launch = [&]() {
      if (which < 4) return n2v2r_launch_tf_hist(A, count, absolute, lim, which, prefix, scr, st);
      if (which == 4) return n2v2r_launch_tf_min(A, count, absolute, lim, prefix, scr + 257, st);
      return n2v2r_launch_tf_apply(A, count, 0, -INFINITY, 0, scr + 258, st);
    };
    HIPCHK(hipMemsetAsync(scr, 0, sizeof(unsigned long long) * 260, st));
    HIPCHK(launch());
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    // one event pair around `reps` launches back to back, as tools/stream_ceiling.hip times its
    // kernels (the counts just keep adding up: nothing reads them)
    hipError_t err = hipEventRecord(e0, st);
    for (int r = 0; r < reps && err == hipSuccess; ++r) err = launch();
    if (err == hipSuccess) err = hipEventRecord(e1, st);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) throw HipFail{err, "bench_transform_pass"};
    *avg_ms = (double)ms / reps;
    if (bytes) *bytes = 4.0 * (double)count;
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): a dense layer's rows back on the host
int n2v2r_get_layer_dense(n2v2r_handle* h, int k, float* A) {
  if (h && h->multi()) return multi_get_layer_dense(h, k, A);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !A || !h->layers[k]->loaded || !h->layers[k]->dense) {
      h->set_err("get_layer_dense: layer %d is not a loaded dense layer", k);
      return N2V2R_ERR_BAD_ARG;
    }
    const LayerDev& L = *h->layers[k];
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->nloc > 0)
      HIPCHK(hipMemcpy2D(A + h->row0 * h->n, sizeof(float) * h->n, L.dA.p, sizeof(float) * L.lda,
                         sizeof(float) * h->n, h->nloc, hipMemcpyDeviceToHost));
    return N2V2R_OK;
  });
}

int n2v2r_set_layer_csr_rows(n2v2r_handle* h, int k, int64_t n, int64_t row0, int64_t n_rows,
                             int64_t nnz, const int64_t* indptr, const int32_t* indices,
                             const float* data) {
  return guarded(h, [&]() -> int {
    if (h->multi()) {
      h->err = "n2v2r_set_layer_csr_rows: a multi-GPU handle takes whole layers (it slices them)";
      return N2V2R_ERR_BAD_ARG;
    }
    if (k < 0 || k >= h->K || n != h->n || row0 != h->row0 || n_rows != h->nloc || nnz < 0 ||
        !indptr || (nnz > 0 && (!indices || !data)) || indptr[0] != 0 || indptr[n_rows] != nnz) {
      h->set_err("bad local CSR rows for layer %d (expected rows [%lld, %lld))", k,
                 (long long)h->row0, (long long)(h->row0 + h->nloc));
      return N2V2R_ERR_BAD_ARG;
    }
    for (int64_t r = 0; r < n_rows; ++r)  // a non-monotone block would hand the SpMM bad spans
      if (indptr[r + 1] < indptr[r]) {
        h->set_err("layer %d: indptr not monotone", k);
        return N2V2R_ERR_BAD_ARG;
      }
    if (!host_indices_in_range(nnz, indices, n)) {
      h->set_err("layer %d: column index out of range", k);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int j = 0; j < h->K; ++j)
      if (j != k && h->layers[j]->loaded && h->layers[j]->dense) {
        h->err = "layers must be all CSR or all dense";
        return N2V2R_ERR_BAD_ARG;
      }
    LayerDev& L = *h->layers[k];
    L.dense = false;
    L.drop_col_blocks();
    L.n_rows = h->nloc;
    L.unit = upload_rows(h->stream, 0, n_rows, indptr, indices, data, L.indptr, L.indices, L.data,
                         L.nnz);
    h->h2d_layer_bytes += 8 * (n_rows + 1) + (L.unit ? 4 : 8) * L.nnz;
    L.symmetric = true;
    L.loaded = true;
    h->have_embedding = false;
    return N2V2R_OK;
  });
}

// float32 column sums of layer k for all N nodes (row sums of the local rows of A^T, gathered)
int n2v2r_column_sums(n2v2r_handle* h, int k, float* out) {
  if (h && h->multi()) return multi_column_sums(h, k, out);
  return guarded(h, [&]() -> int {
    if (k < 0 || k >= h->K || !out || !h->layers[k]->loaded) return N2V2R_ERR_BAD_ARG;
    DevBuf o, g;
    o.ensure(sizeof(float) * h->npad);
    if (h->layers[k]->dense) {
      DevBuf ones;
      ones.ensure(sizeof(float) * h->n);
      std::vector<float> one(h->n, 1.f);
      HIPCHK(hipMemcpy(ones.p, one.data(), sizeof(float) * h->n, hipMemcpyHostToDevice));
      h->dense_apply(h->layers[k]->dense_at(), h->layers[k]->lda, ones.as<float>(), 1, 1,
                     o.as<float>(), 1, 0.f, nullptr);
    } else {
      HIPCHK(n2v2r_launch_row_sums(h->layers[k]->csr_t(), o.as<float>(), h->stream));
    }
    const float* src = o.as<float>();
    if (h->comm) {
      g.ensure(sizeof(float) * h->world * h->npad);
      h->comm->allgather(o.p, g.p, sizeof(float) * h->npad, h->stream);
      src = g.as<float>();
    }
    HIPCHK(hipMemcpyAsync(out, src, sizeof(float) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}

// Bipartite projection (replaces bipartite_to_unipartite_projection, preprocessing_utils.py:16-32,
// which network_transform applies to non-square layers, :130-132): out = W^T W (n x n,
// on_columns) or W W^T (m x m) for a host row-major m x n fp64 W, in fp64 as the reference's
// float64 np.matmul (syrk_f64_kernel: v_mfma_f64_16x16x4_f64, exactly symmetric output).
int n2v2r_project(n2v2r_handle* h, int64_t m, int64_t n, const double* W, int on_columns,
                  double* out) {
  if (h && h->multi()) h = h->ranks[0];  // no collective: rank 0's GPU
  return guarded(h, [&]() -> int {
    if (m < 1 || n < 1 || !W || !out) return N2V2R_ERR_BAD_ARG;
    DevBuf w, o;
    w.ensure(sizeof(double) * m * n);
    HIPCHK(hipMemcpyAsync(w.p, W, sizeof(double) * m * n, hipMemcpyHostToDevice, h->stream));
    // columns: X = W (k = row of W, i = column); rows: X = W^T (k = column, i = row)
    const int64_t r = on_columns ? n : m, kd = on_columns ? m : n;
    const int64_t sk = on_columns ? n : 1, si = on_columns ? 1 : n;
    o.ensure(sizeof(double) * r * r);
    HIPCHK(n2v2r_launch_syrk_f64(w.as<double>(), sk, si, kd, r, o.as<double>(), r, h->stream));
    HIPCHK(hipMemcpyAsync(out, o.p, sizeof(double) * r * r, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return N2V2R_OK;
  });
}

// Soft-threshold scan (soft_threshold.hip): E is uploaded whole and standardised as
// n2v2r_set_layer_corr does it, the scan kernel writes one partial per chunk and a second kernel
// adds them.  Every buffer is local to the call; nothing of the handle but its stream is used.
// chunks: 0 = n2v2r_soft_chunks(n); ms (optional): the scan kernel's time from one event pair.
static int soft_connectivity(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                             int kind, const double* powers, int n_powers, int chunks,
                             double* conn, int* chunks_used, double* ms,
                             int method = N2V2R_COR_PEARSON, int64_t* fallback = nullptr) {
  if (h && h->multi()) h = h->ranks[0];  // no collective: rank 0's GPU
  return guarded(h, [&]() -> int {
    if (!E || !powers || !conn || n < 1 || n > 0x7fffffffLL) {
      h->set_err("soft_connectivity: E, powers and conn must be given and 1 <= n < 2^31");
      return N2V2R_ERR_BAD_ARG;
    }
    if (samples < 2) {
      h->set_err("soft_connectivity: a correlation needs at least 2 samples, got %lld",
                 (long long)samples);
      return N2V2R_ERR_BAD_ARG;
    }
    if (n_powers < 1 || n_powers > 32) {
      h->set_err("soft_connectivity: between 1 and 32 powers per call, got %d", n_powers);
      return N2V2R_ERR_BAD_ARG;
    }
    for (int q = 0; q < n_powers; ++q)
      if (!std::isfinite(powers[q]) || powers[q] < 1.0) {
        h->set_err("soft_connectivity: power must be finite and >= 1, got %g (powers[%d])",
                   powers[q], q);
        return N2V2R_ERR_BAD_ARG;
      }
    if (kind == N2V2R_CORR_RAW) {
      h->set_err("soft_connectivity: a raw correlation takes no power (r may be negative): the "
                 "kinds are unsigned, signed and signed hybrid");
      return N2V2R_ERR_BAD_ARG;
    }
    if (kind != N2V2R_CORR_UNSIGNED && kind != N2V2R_CORR_SIGNED &&
        kind != N2V2R_CORR_SIGNED_HYBRID) {
      h->set_err("soft_connectivity: unknown correlation kind %d", kind);
      return N2V2R_ERR_BAD_ARG;
    }
    if (!corr_method_known(method)) {
      h->set_err("soft_connectivity: unknown correlation method %d", method);
      return N2V2R_ERR_BAD_ARG;
    }
    const int64_t nt = (n + 63) / 64, npad = nt * 64, sp = n2v2r_corr_spad(samples);
    if (chunks < 0 || chunks > nt || chunks > 65535) {
      h->set_err("soft_connectivity: chunks must lie in [0, %lld], got %d", (long long)nt, chunks);
      return N2V2R_ERR_BAD_ARG;
    }
    const int G = chunks ? chunks : n2v2r_soft_chunks(n);
    hipStream_t st = h->stream;
    DevBuf e, z, pw, flag, part, out;  // (the kernels write every element that is read)
    e.ensure_raw(sizeof(double) * n * samples);
    z.ensure_raw(sizeof(double) * npad * sp);
    pw.ensure_raw(sizeof(double) * 32);
    flag.ensure_raw(sizeof(unsigned) * 4);
    part.ensure_raw(sizeof(double) * G * n_powers * npad);
    out.ensure_raw(sizeof(double) * n_powers * n);
    HIPCHK(hipMemcpyAsync(e.p, E, sizeof(double) * n * samples, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pw.p, powers, sizeof(double) * n_powers, hipMemcpyHostToDevice, st));
    const CorrRows rows = corr_standardise_rows(st, e.as<double>(), n, samples, method,
                                                z.as<double>(), flag.as<unsigned>());
    if (rows.bad != 0xFFFFFFFFu) {
      h->set_err("soft_connectivity: row %u of the expression matrix holds a non-finite value or "
                 "is constant (zero variance): its correlations are undefined", rows.bad);
      return N2V2R_ERR_BAD_ARG;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms) {
      HIPCHK(hipEventCreate(&e0));
      const hipError_t ce = hipEventCreate(&e1);
      if (ce != hipSuccess) {
        (void)hipEventDestroy(e0);
        throw HipFail{ce, "hipEventCreate"};
      }
    }
    hipError_t err = hipSuccess;
    if (ms) err = hipEventRecord(e0, st);
    if (err == hipSuccess)
      err = n2v2r_launch_soft_conn(z.as<double>(), samples, n, kind, pw.as<double>(), n_powers, G,
                                   part.as<double>(), st);
    if (ms && err == hipSuccess) err = hipEventRecord(e1, st);
    if (err == hipSuccess)
      err = n2v2r_launch_soft_conn_sum(part.as<double>(), G, n_powers, n, out.as<double>(), st);
    if (err == hipSuccess)
      err = hipMemcpyAsync(conn, out.p, sizeof(double) * n_powers * n, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // the local buffers die here
    float t = 0.f;
    if (ms && err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
    if (ms) {
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
    }
    if (err != hipSuccess) throw HipFail{err, "soft_connectivity"};
    if (ms) *ms = (double)t;
    if (chunks_used) *chunks_used = G;
    if (fallback) std::copy(rows.fallback, rows.fallback + 2, fallback);
    return N2V2R_OK;
  });
}

int n2v2r_soft_connectivity(n2v2r_handle* h, int64_t n, int64_t samples, const double* E, int kind,
                            const double* powers, int n_powers, double* conn) {
  return soft_connectivity(h, n, samples, E, kind, powers, n_powers, 0, conn, nullptr, nullptr);
}

int n2v2r_soft_connectivity_method(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                                   int kind, const double* powers, int n_powers, int method,
                                   double* conn, int64_t* fallback) {
  return soft_connectivity(h, n, samples, E, kind, powers, n_powers, 0, conn, nullptr, nullptr,
                           method, fallback);
}

// diagnostics (n2v2r_diag.h): the row passes of the correlation methods apart from the tile
// product.  Buffers local to the call, rank 0's GPU on a multi handle (no collective).
int n2v2r_corr_ranks(n2v2r_handle* h, int64_t n, int64_t samples, const double* E, double* R) {
  if (h && h->multi()) h = h->ranks[0];
  return guarded(h, [&]() -> int {
    if (!E || !R || n < 1 || n > 0x7fffffffLL || samples < 2 || samples > 0x7fffffffLL) {
      h->set_err("corr_ranks: E and R must be given, 1 <= n < 2^31 and 2 <= samples < 2^31");
      return N2V2R_ERR_BAD_ARG;
    }
    hipStream_t st = h->stream;
    DevBuf e, r;
    e.ensure_raw(sizeof(double) * n * samples);
    r.ensure_raw(sizeof(double) * n * samples);
    HIPCHK(hipMemcpyAsync(e.p, E, sizeof(double) * n * samples, hipMemcpyHostToDevice, st));
    HIPCHK(n2v2r_launch_corr_ranks(e.as<double>(), n, samples, r.as<double>(), st));
    HIPCHK(hipMemcpyAsync(R, r.p, sizeof(double) * n * samples, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // e and r die here
    return N2V2R_OK;
  });
}

int n2v2r_corr_standardise(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                           int method, double* Z, int64_t* bad_row) {
  if (h && h->multi()) h = h->ranks[0];
  return guarded(h, [&]() -> int {
    if (!E || !Z || n < 1 || n > 0x7fffffffLL || samples < 2 || samples > 0x7fffffffLL) {
      h->set_err("corr_standardise: E and Z must be given, 1 <= n < 2^31 and 2 <= samples < "
                 "2^31");
      return N2V2R_ERR_BAD_ARG;
    }
    if (!corr_method_known(method)) {
      h->set_err("corr_standardise: unknown correlation method %d", method);
      return N2V2R_ERR_BAD_ARG;
    }
    hipStream_t st = h->stream;
    const int64_t npad = (n + 63) / 64 * 64, sp = n2v2r_corr_spad(samples);
    DevBuf e, z, flag;
    e.ensure_raw(sizeof(double) * n * samples);
    z.ensure_raw(sizeof(double) * npad * sp);
    flag.ensure_raw(sizeof(unsigned) * 4);
    HIPCHK(hipMemcpyAsync(e.p, E, sizeof(double) * n * samples, hipMemcpyHostToDevice, st));
    const CorrRows rows = corr_standardise_rows(st, e.as<double>(), n, samples, method,
                                                z.as<double>(), flag.as<unsigned>());
    HIPCHK(hipMemcpy2DAsync(Z, sizeof(double) * samples, z.p, sizeof(double) * sp,
                            sizeof(double) * samples, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // e and z die here
    if (bad_row) *bad_row = rows.bad == 0xFFFFFFFFu ? -1 : (int64_t)rows.bad;
    return N2V2R_OK;
  });
}

// the row kernel of a method alone, timed with HIP events (the flag words are not reset between
// the launches: their atomics run as in a build, their values are not read)
int n2v2r_bench_corr_rows(n2v2r_handle* h, int64_t n, int64_t samples, const double* E, int method,
                          int reps, double* ms) {
  if (h && h->multi()) h = h->ranks[0];
  return guarded(h, [&]() -> int {
    if (!E || !ms || reps < 1 || n < 1 || n > 0x7fffffffLL || samples < 2 ||
        samples > 0x7fffffffLL || !corr_method_known(method)) {
      h->err = "bench_corr_rows: E and ms, reps >= 1, 1 <= n < 2^31, 2 <= samples < 2^31 and a "
               "known method";
      return N2V2R_ERR_BAD_ARG;
    }
    hipStream_t st = h->stream;
    const int64_t npad = (n + 63) / 64 * 64, sp = n2v2r_corr_spad(samples);
    const bool ranks = method == N2V2R_COR_SPEARMAN;
    DevBuf e, o, flag;
    e.ensure_raw(sizeof(double) * n * samples);
    o.ensure_raw(sizeof(double) * (ranks ? n * samples : npad * sp));
    flag.ensure_raw(sizeof(unsigned) * 4);
    HIPCHK(hipMemcpyAsync(e.p, E, sizeof(double) * n * samples, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(flag.p, 0xFF, sizeof(unsigned) * 4, st));
    auto launch = [&]() {
      if (ranks) return n2v2r_launch_corr_ranks(e.as<double>(), n, samples, o.as<double>(), st);
      if (method == N2V2R_COR_BICOR)
        return n2v2r_launch_corr_bicor(e.as<double>(), n, samples, o.as<double>(),
                                       flag.as<unsigned>(), st);
      return n2v2r_launch_corr_standardise(e.as<double>(), n, samples, o.as<double>(),
                                           flag.as<unsigned>(), st);
    };
    HIPCHK(launch());  // warm-up
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    const hipError_t ce = hipEventCreate(&e1);
    if (ce != hipSuccess) {
      (void)hipEventDestroy(e0);
      throw HipFail{ce, "hipEventCreate"};
    }
    hipError_t err = hipSuccess;
    for (int r = 0; r < reps && err == hipSuccess; ++r) {
      err = hipEventRecord(e0, st);
      if (err == hipSuccess) err = launch();
      if (err == hipSuccess) err = hipEventRecord(e1, st);
      if (err == hipSuccess) err = hipEventSynchronize(e1);
      float t = 0.f;
      if (err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
      ms[r] = (double)t;
    }
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // the local buffers die here
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) throw HipFail{err, "bench_corr_rows"};
    return N2V2R_OK;
  });
}

// diagnostics (n2v2r_diag.h): the scan with the chunk count given, the scan kernel timed
int n2v2r_soft_connectivity_chunks(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                                   int kind, const double* powers, int n_powers, int chunks,
                                   double* conn, int* chunks_used, double* kernel_ms) {
  return soft_connectivity(h, n, samples, E, kind, powers, n_powers, chunks, conn, chunks_used,
                           kernel_ms);
}

}  // extern "C"
