/* n2v2r_diag.h -- diagnostic entry points of libn2v2r_hip.so (kernel timings and single solver
 * stages for tests and the roofline); not part of the drop-in API in n2v2r.h and with no
 * reference counterpart.  Same conventions as n2v2r.h. */
#ifndef N2V2R_DIAG_H
#define N2V2R_DIAG_H

#include "n2v2r.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SpMM kernel alone (tests + roofline): Y = A_k X (transpose = 0) or A_k^T X (1) for a host
 * N x b panel X (b = 8, 16, 32 or 64), timed with HIP events on the engine stream over `reps`
 * launches after one warm-up.  avg_ms = mean launch duration; algo_bytes = SURVEY 8(d) bytes
 * per launch (8 nnz + 4 (N+1) + 8 N b).  On a partitioned handle A_k means this rank's rows:
 * X is the global N x b panel, Y its n_local x b rows, bytes 8 nnz_loc + 4 (n_loc+1) +
 * 4 (N + n_loc) b.  Y may be NULL. */
int n2v2r_bench_spmm(n2v2r_handle* h, int k, int transpose, int b, int reps, const float* X,
                     float* Y, double* avg_ms, double* algo_bytes);
/* The flat-window tiled SpMM of layer k (A_k X, or A_k^T X) at panel width b = 8 with nb column
 * blocks (0: panel blocks of <= 2 MB, at most 32), one-GPU handles; Y (optional, n x 8) receives
 * the product.  N2V2R_ERR_BAD_ARG when b != 8 (the b = 16 tiled kernel was retired; the
 * parameter keeps the signature) or when the layer cannot take packed blocks. */
int n2v2r_bench_spmm_tiled(n2v2r_handle* h, int k, int transpose, int b, int nb, int reps,
                           const float* X, float* Y, double* avg_ms);

/* 1 when UASE (and n2v2r_bench_spmm) use a column-block SpMM at panel width b on this handle's
 * layers, else 0: b = 8 CSR panels beyond 8 MB (no upper bound) take the flat-window tiled form
 * (each layer's entries regrouped into column blocks of <= 2 MB of panel, 4..32 blocks chosen
 * automatically, one launch per SpMM stage walking the blocks in phases with LDS accumulators);
 * env N2V2R_SPMM_CB=1/0 forces / forbids column blocks. */
int n2v2r_spmm_col_blocks(const n2v2r_handle* h, int b);

/* Rayleigh-Ritz stage alone (tests): top-p eigenpairs of a host symmetric c x c fp64 matrix H
 * (3 <= c <= 768) through UASE's own path, all on the GPU (Householder tridiagonalisation,
 * bisection + inverse iteration on the tridiagonal, compact-WY back-transform).  w: p eigenvalues, descending; S: c x p
 * row-major fp32 eigenvectors (the Ritz coefficients UASE consumes). */
int n2v2r_rr_top(n2v2r_handle* h, int c, const double* H, int p, double* w, float* S);

/* One orthogonalisation pass at block width 8 alone (tests), through the solver's own launchers,
 * on a one-GPU handle.  Q: nq >= 1 basis blocks of n x 8 fp32, one after the other; Za (and Zb):
 * n x 8 fp32, orthogonalised in place.  tau: the selective threshold (PipPass skip_tol; 0: every
 * block); seed: of the refill deviates.
 *   Zb == NULL: the Gram [Q Za]^T Za and one fused pass of Za against Q; first: the pass is the
 *     block's first (a pivot the Gram cannot resolve is clamped and the column kept).
 *     gram: (nq + 1) x 8 x 8 fp64; R: the pass's R (8 x 8 fp64, the identity for a skipped pass).
 *   Zb != NULL (first must be 0): the solver's paired full pass, Za against Q and Zb against
 *     [Q Za'] from the two-block Gram, as three launches (form 0) or through the paired apply
 *     (form 1); Zb's pass draws with seed + 1.  gram: 2 x (nq + 2) x 8 x 8 fp64 (Za's Gram, then
 *     Zb's with its rows against Za rewritten against the corrected Za').  R is not written.
 * flags[8], any_flag: as the last pass left them.  skipped: nq + 1 (nq + 2) counters, [0] the
 * passes skipped whole, [1 + k] the times block k was applied (all zero when tau == 0).
 * N2V2R_ERR_BAD_ARG where a launcher refuses the shape (a basis past 768 columns, a plan that
 * does not fit with form 1) and on a partitioned or multi-GPU handle. */
int n2v2r_pip_pass(n2v2r_handle* h, int64_t n, int nq, const float* Q, float* Za, float* Zb,
                   float tau, int first, int form, uint64_t seed, double* gram, double* R,
                   int* flags, int* any_flag, int* skipped);

/* What one n2v2r_gram_apply launched, from the solver's own plan of that application. */
typedef struct n2v2r_gram_info {
  int form;       /* as n2v2r_eig_stats.spmm_form: 0 flat sum, 1 XCD-split, 4 dense, 5 tiled */
  int rs_form;    /* 1: stage 2 as the reduce-scatter of the rank's column share */
  int rs_chunks;  /* ... in this many row chunks (1: one launch; 0 without rs_form) */
  int split2;     /* 1: both stages split over the XCDs, W summed from per-layer partials */
  int tile_nb, tile_wb, tile_rows; /* tiled form: column blocks, window bits, rows per tile (else 0) */
  int rpw1, rpw2; /* rows per wave of the last row-kernel launch of stage 1 / stage 2 (the
                     launcher's rule on the arguments launched); 0: that stage ran no row kernel */
} n2v2r_gram_info;

/* One application W = M X = sum_k A_k (A_k^T X) at panel width b (8, 16, 32 or 64) alone (tests),
 * through the solver's own set-up steps and launches: whichever form a fit at this width would
 * take on this handle under the environment switches in force (flat, XCD-split, tiled, dense;
 * on a rank handle the gather or the reduce-scatter form).  X: the global N x b panel (a rank
 * handle uploads its own rows and gathers the rest from its peers: the call is collective, every
 * rank makes it with the same X).  W: this handle's n_local x b rows of M X.  Z (optional):
 * K x n_local x b, the stage-1 panels Z_k = A_k^T X.  Every row the application has to write --
 * W, the Z_k, the split form's partials, a rank handle's gathered panels -- is filled with NaN
 * bytes first, so a row no launch wrote shows in the result.  info (optional): what ran.  The
 * handle's embedding and ranking results are left alone, and a later fit is bit-identical to one
 * without the call.  N2V2R_ERR_BAD_ARG for another b, for missing layers and on a multi-GPU
 * parent handle (its ranks would each need the call). */
int n2v2r_gram_apply(n2v2r_handle* h, int b, const float* X, float* Z, float* W,
                     n2v2r_gram_info* info);

/* What one n2v2r_ritz_step launched, as the solver's ritz_vectors recorded it. */
typedef struct n2v2r_ritz_info {
  int fused;     /* 1: ritz_nn_kernel made X (and MX) in one launch; 0: ts_nn launches per slice */
  int launches;  /* product launches made: 1 when fused, else one per slice of <= 128 output
                    columns and product (X, and MX unless lean) */
  int lds_bytes; /* dynamic LDS of the fused launch (the launcher's rule), else 0 */
} n2v2r_ritz_info;

/* The step between a cycle's Rayleigh-Ritz and the next cycle alone (tests), through the solver's
 * own ritz_vectors and launch_residuals on an Eig whose plan is block width b (8, 16, 32 or 64),
 * keep kept Ritz vectors and a basis of nq blocks, with the fit's scratch sizing: X = Q S and
 * MX = W S (fused at b = 8, keep <= 96 while S fits 150 KB of LDS, else per slice of 128 output
 * columns), then res[j] = sum_r (MX[r][j] - theta[j] X[r][j])^2.  n = the handle's local row
 * count, from the layers set (any loaded layers; the step does not read them).
 * Q, W: nq blocks of n x b fp32, one after the other; S: (nq b) x keep fp32 row-major; theta: keep
 * fp64.  X, MX: keep / b blocks of n x b fp32; res: keep fp64.  lean != 0 (b = 8 only): X alone,
 * as a fit with lean images computes it; W, MX and res may be NULL and are not touched.  Every row
 * of X and MX the step has to write, and res, is filled with NaN bytes first.  On a rank handle
 * every rank makes the call with its own rows (collective unless lean) and res comes back summed
 * over the ranks, as the solver reads it.  info (optional): what ran.  The handle's embedding
 * and ranking results are left alone, and a later fit is bit-identical to one without the call.
 * N2V2R_ERR_BAD_ARG on a multi-GPU parent handle, without loaded layers, for another b, for
 * keep % b != 0, keep + b > nq b, nq b > 768, lean with b != 8, and for a NULL pointer the mode
 * needs. */
int n2v2r_ritz_step(n2v2r_handle* h, int b, int nq, int keep, int lean, const float* Q,
                    const float* W, const float* S, const double* theta, float* X, float* MX,
                    double* res, n2v2r_ritz_info* info);

/* What one n2v2r_block_gram or n2v2r_ortho_pass launched, from the launchers' own shape rules
 * (the functions the launchers call to decide). */
typedef struct n2v2r_pass_info {
  int gram_form;    /* the Gram kernel: 0 streaming (b = 8), 1 lines (b = 8), 2 narrow (one 8- or
                       16-wide right-hand block), 3 MFMA tiles */
  int gram_flush;   /* narrow form: 1 when the instantiation that flushes its fp32 sums ran */
  int64_t nchunks;  /* row chunks of the Gram (one fp64 partial each) */
  int64_t rows_per_chunk; /* rows of a chunk; its 4 waves take ceil(rows_per_chunk / 4) each */
  int stage;        /* pass, b > 8: 1 when pip_chol staged the Gram through LDS (b = 8: 0) */
  int nwg;          /* pass, b > 8: the workgroups F's rows were split over (b = 8: 0) */
  int apply_kernel; /* pass: 0 the fused b = 8 kernel, 8 / 16 ts_nn_rows_kernel<8> / <16>,
                       32 NT ts_nn_kernel<NT> */
  int reserved;
  uint64_t fill_seed; /* pass: the refill seed the pass drew (Eig::next_fill_seed) */
} n2v2r_pass_info;

/* G = [A]^T [B] alone (tests), through the solver's own Gram method (Eig::tn) on an Eig whose plan
 * is block width b (8, 16, 32 or 64) and a basis of max(na, nb) blocks, with the fit's scratch
 * sizing, so the partial buffer and with it the chunk plan are a fit's: the pass Gram
 * [Q Z]^T Z (nb = 1) and the projected matrix H = Q^T W of the dense Rayleigh-Ritz (na = nb).
 * n = the handle's local row count, from the layers set (any loaded layers; the call does not
 * read them).  A, B: na / nb blocks of n x b fp32, one after the other; G: (na b) x (nb b) fp64
 * row-major, filled with NaN bytes first, like the chunk partials.  info (optional): what ran.
 * The handle's embedding and ranking results are left alone, and a later fit is bit-identical to
 * one without the call.  One-GPU handles only: N2V2R_ERR_BAD_ARG on a rank or multi-GPU handle,
 * without loaded layers, for another b, for na < 1, nb < 1, na b > 768 or nb b > 768, and for a
 * NULL A, B or G. */
int n2v2r_block_gram(n2v2r_handle* h, int b, int na, int nb, const float* A, const float* B,
                     double* G, n2v2r_pass_info* info);

/* One orthogonalisation pass at block width b (8, 16, 32 or 64) alone (tests), through the
 * solver's own Eig::pip_pass on an Eig whose plan is b and a basis of nq + 1 blocks, with the
 * fit's scratch sizing: the Gram [Q Z]^T Z, then at b = 8 the fused pass, at wider blocks
 * pip_chol (P = Z^T Z - C^T C, its Cholesky factor's inverse, F = [-C R^{-1}; R^{-1}]) and the
 * apply Z' = [Q Z] F.  n = the handle's local row count, as for n2v2r_block_gram.
 * Q: nq >= 0 basis blocks of n x b fp32 (nq = 0: the start block's pass, Q may be NULL); Z: n x b
 * fp32, the block in and the result out.  in_place = 0: the pass reads a separate copy of Z and
 * writes a block filled with NaN bytes, as an expansion does from the image it orthogonalises.
 * first: as PipPass::first (a pivot the Gram cannot resolve is clamped and the column kept).
 * cond: -1 no condition word; 0 / 1: that value in a device word the pass is conditional on (the
 * third pass's gate; 0: nothing runs, the flags and any_flag are cleared).  seed: the Eig's seed,
 * from which the pass draws its refill seed (returned in info).
 * gram: (nq + 1) b x b fp64; xinv: b x b fp64 (R^{-1}, flagged columns zero; b = 8: not written,
 * the fused kernel keeps it in LDS); F: (nq + 1) b x b fp32 (b = 8: not written); flags[b],
 * any_flag.  The device buffers behind gram, xinv, F and the result block are filled with NaN
 * bytes before the pass and the flag words with a non-zero pattern, so what no launch wrote shows.
 * The handle's embedding and ranking results are left alone, and a later fit is bit-identical to
 * one without the call.  One-GPU handles only: N2V2R_ERR_BAD_ARG on a rank or multi-GPU handle,
 * without loaded layers, for another b, for nq < 0, (nq + 1) b > 768, cond outside -1 .. 1, and
 * for a NULL pointer the mode needs (Q with nq > 0, Z, gram, flags, any_flag; xinv and F at
 * b > 8). */
int n2v2r_ortho_pass(n2v2r_handle* h, int b, int nq, const float* Q, float* Z, int in_place,
                     int first, int cond, uint64_t seed, double* gram, double* xinv, float* F,
                     int* flags, int* any_flag, n2v2r_pass_info* info);

/* Banded Rayleigh-Ritz stage alone (tests; block width 8, c <= 512, kp + 8 <= 192): the
 * projected matrix of a Krylov-Schur cycle given as UASE keeps it.  Basis order [X (kp
 * columns, diagonal theta_prev), E, Z_2, ...] in 8-wide blocks; hband holds band column
 * j0 = kp/8 ([X E]^T M E, (kp+8) x 8 row-major) at offset 0, then for every later block j the
 * 16 x 8 matrix [Q_{j-1} Q_j]^T M Q_j.  Entries outside the band (half-bandwidth 8) are taken
 * as zero.  Same outputs as n2v2r_rr_top. */
int n2v2r_rr_band_top(n2v2r_handle* h, int c, int kp, const double* hband, int64_t hband_len,
                      const double* theta_prev, int p, double* w, float* S);

/* What one n2v2r_rr_stage ran. */
typedef struct n2v2r_rr_info {
  int form_ran;       /* 0 Sturm, 1 BandReduce, 2 DenseFromBand, 3 Dense: the form whose result is
                         returned (-1: the call was refused) */
  int sturm_err;      /* err[0] of the Sturm launch (a vector failed its residual check); -1: Sturm
                         did not run */
  int second_solves;  /* err[1]: vectors that took the second solve; -1 likewise */
  int reduce_err;     /* the reducing path's error word (the bulge chase gave up); -1: it did not
                         run */
  int tri_coop;       /* dense forms: 1 the multi-workgroup tridiagonalisation ran, 0 the
                         one-workgroup kernel (N2V2R_RR_TRI=1, no room for the grid, or after a
                         timed-out grid barrier); -1 n/a */
  int msect_points, msect_rounds; /* Sturm: points per eigenvalue per multisection round and the
                         rounds launched (the launcher's own rule); 0 otherwise */
  int reserved;
} n2v2r_rr_info;

/* One Rayleigh-Ritz of a Krylov-Schur projected matrix alone, in one chosen form (tests), through
 * the solver's launchers on buffers of its own.  c, kp, hband, hband_len, theta_prev, p, w, S: as
 * n2v2r_rr_band_top, within the launchers' own limits: 16 <= c <= 768, c % 8 == 0, kp % 8 == 0,
 * kp + 8 <= c, 1 <= p <= c.  form:
 *   -1  as a fit moves: the Sturm form, and when a vector fails its check (sturm_err) the form the
 *       solver takes next, by the solver's own rule at (kp, c): the reducing path while
 *       kp + 8 <= 192 and c <= 640, else the dense steps on H expanded from the band
 *       (env N2V2R_RR_STAGE_TEST_STURM_FAIL=1, tests: a good Sturm result is discarded and that
 *       form runs; sturm_err still reports the launch's own word);
 *    0  the Sturm form alone; its result is returned even when sturm_err != 0;
 *    1  the reducing path alone (kp + 8 <= 192);
 *    2  rr_band_expand_kernel into a c x c matrix, then the dense steps (tridiagonalisation,
 *       bisection + inverse iteration, back-transform).
 * Y (optional): c x p fp64 row-major, the eigenvectors in fp64 where the form holds them in H's
 * basis: the Sturm form does (its inverse iteration works on H itself).  The reducing path and the
 * dense steps hold fp64 vectors of their tridiagonal only and back-transform into fp32 S: Y comes
 * back as NaN bytes from them.  The device buffers behind w, S and Y are filled with NaN bytes
 * before each form runs, so a column no launch wrote shows (the first kp entries behind w hold
 * theta_prev on entry: the launchers read and write one buffer).  info (optional): what ran.  The
 * handle's embedding and ranking results are left alone, and a later fit is bit-identical to one
 * without the call.  N2V2R_ERR_BAD_ARG for a shape outside the limits above or one the form's
 * launcher refuses, a short hband_len, a NULL hband, w or S (theta_prev with kp > 0), and a form
 * outside -1 .. 2. */
int n2v2r_rr_stage(n2v2r_handle* h, int c, int kp, const double* hband, int64_t hband_len,
                   const double* theta_prev, int p, int form, double* w, float* S,
                   double* Y /* optional, c x p */, n2v2r_rr_info* info);

/* What one n2v2r_embed_step launched, from the launchers' own shape rules. */
typedef struct n2v2r_embed_info {
  int form;      /* the products' form in the n2v2r_eig_stats.spmm_form codes: 0 the CSR row kernels
                    (also on a handle whose applications take the XCD split: the embedding's
                    products never do), 4 dense, 5 tiled (-1: the call was refused) */
  int launches;  /* product launches: ldu / b row-kernel launches over all K layers, ldu / 8 tiled
                    launches over all K layers, K * ldu / 64 dense GEMMs */
  int ldu;       /* row stride of U and of every Y_k: 64 * ceil(d / 64) */
  int rpw;       /* row-kernel form: rows per wave of the last launch (the launcher's rule on the
                    arguments launched), else 0 */
  int64_t colmax_chunks; /* row chunks of the column-max pass over this handle's local rows */
  int64_t colmax_rows;   /* rows per chunk (the last chunk may be shorter) */
} n2v2r_embed_info;

/* The step that turns a converged fit into the embedding alone (tests), through the solver's own
 * build_embedding with a GramOp set up as a fit's at block width b (8, 16, 32 or 64): the sign
 * pass (every column of U flipped so that its entry of largest magnitude, the smallest global row
 * on ties, is positive; +1 for a zero entry), sigma = sqrt(max(theta, 0)) and Y_k = A_k^T U
 * sigma^(-1/2) (a zero column where sigma is 0) in whichever form a fit at this width would take
 * on this handle under the environment switches in force: the row kernels on strided panels, the
 * tiled SpMM on 8-column slices, the dense GEMMs; on a rank handle the same on the all-gathered
 * U, with the sign keys and signs all-reduced.  The products the final lean check of a fit may
 * have captured are not reachable through this entry.
 * U: the global N x d fp32 matrix, row-major (a rank handle uploads its own rows: the call is
 * collective, every rank makes it with the same U); theta: d fp64 Ritz values.  The rows go into
 * the handle's U at row stride ldu, padded rows and columns zeroed first, as n2v2r_uase zeroes
 * them.  The local rows of every Y_k, the column scales, the chunk keys and the winning keys are
 * filled with NaN bytes before the step, so what no launch wrote shows.  The result is installed
 * as the handle's embedding exactly as a fit installs it (U, Y, sigma, d, the row stride; the
 * ranking results cleared): read it with n2v2r_get_embedding, n2v2r_get_left_embedding and
 * n2v2r_get_singular_values.  info (optional): what ran.  A later fit is bit-identical to one
 * without the call.
 * N2V2R_ERR_BAD_ARG on a multi-GPU parent handle (its ranks would each need the call), without
 * loaded layers, for another b, for d outside [1, min(600, n - 1)] and for a NULL U or theta; the
 * handle's embedding and ranking results are then left alone. */
int n2v2r_embed_step(n2v2r_handle* h, int b, int d, const float* U, const double* theta,
                     n2v2r_embed_info* info);

/* Layer bytes each rank copied host -> device so far (one-GPU handle: one entry): row pointers,
 * column indices and values of every CSR layer ingest and the 8 n samples bytes of every
 * n2v2r_set_layer_corr (each rank uploads E whole), into per_rank[0 .. min(W, cap)).  Returns the
 * rank count W.  A multi-GPU handle slices layers on the host, so each rank's figure is about
 * 1/W of the layers' bytes (2/W for directed layers: rows of A and of A^T). */
int n2v2r_h2d_layer_bytes(const n2v2r_handle* h, int64_t* per_rank, int cap);

/* A dense layer (n2v2r_set_layer_dense, n2v2r_set_layer_corr) copied back to the host: A is
 * row-major n x n fp32.  A multi-GPU handle returns all N rows; a rank handle writes its local
 * rows at their global offset (rows [row0, row0 + n_local) of A) and leaves the rest alone.
 * N2V2R_ERR_BAD_ARG when layer k is not a loaded dense layer. */
int n2v2r_get_layer_dense(n2v2r_handle* h, int k, float* A /* n x n */);

/* A loaded CSR layer's local rows copied back to the host (layers that came in through
 * n2v2r_set_layer_csr / _rows or n2v2r_layers_to_csr): the thresholded network as an edge
 * structure, without an n x n host array.  transpose = 1 reads the A^T copy of a directed layer
 * (N2V2R_ERR_BAD_ARG for a symmetric one, which keeps none).  n2v2r_get_layer_csr_nnz gives the
 * entry count to size the buffers with.  indptr: n_local + 1 row pointers starting at 0; indices:
 * global columns; data: the values, 1.0f for an unweighted layer.  A rank handle returns its
 * n_local rows, a multi-GPU handle all N rows (the ranks' rows one after the other).
 * N2V2R_ERR_BAD_ARG when layer k is not a loaded CSR layer. */
int n2v2r_get_layer_csr_nnz(n2v2r_handle* h, int k, int transpose, int64_t* nnz);
int n2v2r_get_layer_csr(n2v2r_handle* h, int k, int transpose, int64_t* indptr, int32_t* indices,
                        float* data);

/* One kernel of n2v2r_layers_to_csr alone on the loaded dense layer k of a one-GPU handle
 * (tools/sparsify_probe.py): which = 0 dense_row_count_kernel, 1 dense_row_compact_kernel (into
 * scratch buffers; the layer stays dense), timed with one HIP event pair on the engine stream
 * around `reps` launches back to back after one warm-up.  avg_ms = the span / reps; bytes = the
 * layer bytes one launch reads (the compaction writes 8 B per stored entry besides, 4 B for an
 * unweighted layer). */
int n2v2r_bench_sparsify_pass(n2v2r_handle* h, int k, int which, int reps, double* avg_ms,
                              double* bytes);

/* One kernel of n2v2r_transform_layer alone on the loaded dense layer k of a one-GPU handle, timed
 * with one HIP event pair on the engine stream around `reps` launches back to back, after one
 * warm-up (the roofline of tools/layer_transform_probe.py).  which: 0..3 the radix-select
 * histogram pass of that index (its prefix = the digits of the layer's median alive key, so every
 * pass counts a real bucket), 4 the min pass above that key, 5 the apply pass with a cut of -inf
 * and no flag, which rewrites every entry with its own value (a -0 becomes +0, a NaN 0).
 * flags / threshold as n2v2r_transform_layer (BINARIZE ignored).  avg_ms = the span / reps;
 * bytes = the layer bytes one launch reads (the apply pass writes as many again). */
int n2v2r_bench_transform_pass(n2v2r_handle* h, int k, int which, int flags, double threshold,
                               int reps, double* avg_ms, double* bytes);

/* tom_tile_kernel of n2v2r_tom_layer alone on the loaded symmetric dense layer k of a one-GPU
 * handle (tools/tom_probe.py): the row sums once, one warm-up launch, then `reps` launches into
 * the handle's scratch buffer, each between its own HIP event pair on the engine stream; the
 * layer is left as it is.  ms[0 .. reps) = the launches' times; flop (optional) = what one launch
 * computes: 2 * 64 * 64 * lda for each of the nt (nt + 1) / 2 upper-triangle tiles, nt = lda / 64,
 * lda = 64 ceil(n / 64) (about n^3). */
int n2v2r_bench_tom_tiles(n2v2r_handle* h, int k, int type, int reps, double* ms, double* flop);

/* n2v2r_soft_connectivity with the chunk count given (tests, tools/soft_threshold_probe.py):
 * every tile row's tile columns are split into `chunks` contiguous chunks, one workgroup and one
 * partial sum each, added in ascending order (0: the count the call itself takes, a function of n
 * alone; at most ceil(n / 64)).  chunks_used (optional) = the count that ran; kernel_ms (optional)
 * = soft_conn_kernel's time, one HIP event pair on the engine stream around its one launch (the
 * upload, the standardisation and the chunk sum are outside it).  Errors as
 * n2v2r_soft_connectivity, and N2V2R_ERR_BAD_ARG for chunks outside [0, ceil(n / 64)]. */
int n2v2r_soft_connectivity_chunks(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                                   int kind, const double* powers, int n_powers, int chunks,
                                   double* conn, int* chunks_used, double* kernel_ms);

/* The row passes of the correlation methods (N2V2R_COR_*, n2v2r.h) apart from the tile product
 * (tests, tools/cor_method_probe.py).  Each call uploads E (n x samples, row-major fp64) into
 * buffers of its own on the engine stream and leaves the handle as it is; on a multi-GPU handle it
 * runs on rank 0's GPU, with no collective.  N2V2R_ERR_BAD_ARG: NULL E or output, n < 1,
 * samples < 2, an unknown method.
 * n2v2r_corr_ranks: R (n x samples) = the per-row average ranks corr_rank_kernel writes, exact
 * half-integers; a row that holds a non-finite value comes back as NaNs (the standardisation that
 * follows refuses it).
 * n2v2r_corr_standardise: Z (n x samples) = columns [0, samples) of rows [0, n) of the
 * standardised rows the tile product consumes, under `method`; bad_row (optional) = the smallest
 * row that holds a non-finite value or is constant, or -1.  A bad row is no error here: its Z is
 * zeros.
 * n2v2r_bench_corr_rows: the method's row kernel alone (N2V2R_COR_PEARSON: corr_standardise_kernel,
 * N2V2R_COR_SPEARMAN: corr_rank_kernel, N2V2R_COR_BICOR: corr_bicor_kernel), launched 1 + reps
 * times (the first is a warm-up), each between its own HIP event pair; ms[0 .. reps). */
int n2v2r_corr_ranks(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                     double* R /* n x samples */);
int n2v2r_corr_standardise(n2v2r_handle* h, int64_t n, int64_t samples, const double* E,
                           int method, double* Z /* n x samples */, int64_t* bad_row);
int n2v2r_bench_corr_rows(n2v2r_handle* h, int64_t n, int64_t samples, const double* E, int method,
                          int reps, double* ms);

#ifdef __cplusplus
}
#endif

#endif /* N2V2R_DIAG_H */
