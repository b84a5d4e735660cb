"""The step between a cycle's Rayleigh-Ritz and the next cycle on its own (``n2v2r_ritz_step``:
the solver's ``Eig::ritz_vectors`` and ``Eig::launch_residuals`` on host arrays) against
np.longdouble: the Ritz vectors X = Q S and images MX = W S from ``ritz_nn_kernel`` (fused, b = 8,
keep <= 96, S within 150 KB of LDS), ``ts_nn_kernel`` (per slice of 128 output columns) and
``ts_nn_rows_kernel`` (a last slice of <= 16 columns), and the squared residuals
res[j] = sum_r (MX[r][j] - theta[j] X[r][j])^2 from ``resid_kernel`` + the chunk fold (+ the
all-reduce on a rank handle).

Inputs (built in fp64, rounded to fp32 once; the references use the rounded arrays).  Q: the fp32
rounding of an orthonormal n x c factor, c = nq b (at n = 37 < c, of one with orthonormal rows);
S: of c x keep orthonormal columns; theta: keep distinct descending fp64 values in [1, 100];
W = Q (S diag(theta) S^T) + E with E ~ N(0, 1) * 1e-4 / sqrt(n), so MX is within ~1e-4 of
X diag(theta) and a residual is a cancellation of five to six digits, as near convergence.  The
handle carries one identity layer, only to fix n and the row partition.

Product bound (derived, not measured).  An output entry is an fp32 sum of ca = nq b products
accumulated by MFMA 32x32x2 instructions: with at most one rounding per product and one per
addition, in any order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1),
    |X - Q S| <= gamma32(2 ca) |Q| |S|,   gamma32(k) = k u / (1 - k u),   u = 2^-24,
entrywise, against Q32 @ S32 in np.longdouble (and MX against W32 @ S32).  |Q| |S| is formed in
fp64 (its own rounding, ca 2^-53 relative, is nine orders below the bound's).

Residual bound (derived).  The reference uses the X and MX the GPU returned, so the products'
rounding does not enter.  Each term v^2, v = MX - theta X, is formed in fp64 from fp32 inputs
with at most one rounding for v (one fused multiply-add, v_fma_f64 in the gfx950 code: separate
roundings of theta x and of the difference would leave ~1e-10 |v| and miss this bound) and one for
its square, and the terms, all non-negative, are added in fp64: at most n additions along any
path through the row loop, the workgroup fold and the chunk fold (and the ranks' sum), so
    |res - ref| <= gamma64(n + 16) ref,   u = 2^-53.
The reference has to resolve v better than that: theta x carries 77 significant bits, which one
np.longdouble product would round at 2^-64 |theta x| ~ 1e-13 |v|, above the bound at small n.  So
theta is split as hi + lo, hi its fp32 rounding: hi x (48 bits) and lo x (<= 53 bits) are exact in
np.longdouble, m - hi x is exact (both multiples of 2^-47 of their common magnitude), and
v = (m - hi x) - lo x carries one longdouble rounding, 2^-64 |v|.

Shapes: the smallest that take each branch (CASES); every case asserts what ran from
``n2v2r_ritz_info``.  n = 4,099 is prime: 3 rows in the last 32-row tile and in the last 256-row
workgroup.  Each case prints the largest fraction of its bounds it reached, and the largest so
far per kernel family (``pytest -s``).  On an MI355X the largest fractions were 0.084 (fused),
0.020 (ts_nn), 0.012 (ts_nn_rows) of the product bound and 0.11 (resid, at n = 37; 0.0008 at
n = 4,099) of the residual bound; the 22 cases take 11 s together."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import fixture_layers, load_fixture
from test_gpu_dist import _run_ranks
from test_gpu_pip_pass import _basis, _gamma, _ro, U32, U64

pytestmark = pytest.mark.gpu

N0 = 4099
LD = np.longdouble

# (b, keep, nq, fused, launches, what it reaches).  launches: 1 fused; else 2 (X and MX) per slice
# of 128 output columns.
CASES = [
    (8, 32, 5, 1, 1, "fused <1>; c = 40 < 64: first-chunk loads clamped to ca - 8"),
    (8, 32, 8, 1, 1, "fused <1>; exactly one k chunk"),
    (8, 32, 9, 1, 1, "fused <1>; chunk tail of one 8-group"),
    (8, 48, 24, 1, 1, "fused <2>; cb = 48, columns 48..63 staged as zero and masked"),
    (8, 88, 48, 1, 1, "fused <3>; 147,456 B of LDS, the cfg2 shape"),
    (8, 96, 50, 1, 1, "fused <3>; exactly 150 KB of LDS, the last that fits"),
    (8, 96, 51, 0, 2, "first past the LDS limit: one ts_nn_kernel<3> launch per product"),
    (8, 104, 20, 0, 2, "keep > 96: ts_nn_kernel<4>, cb = 104"),
    (8, 136, 24, 0, 4, "slices 128 + 8: ts_nn_rows_kernel<8>"),
    (8, 144, 24, 0, 4, "slices 128 + 16: ts_nn_rows_kernel<16> at A.width 8 (generic loop)"),
    (8, 184, 80, 0, 4, "slices 128 + 56, the cfg4 shape: coefficient slice at column 128"),
    (16, 144, 11, 0, 4, "slices 128 + 16: ts_nn_rows_kernel<16>, w == CB: two rounds + tail 3"),
    (32, 160, 7, 0, 4, "slices 128 + 32; k tail of 32; A.width 32"),
    (64, 192, 5, 0, 4, "slices 128 + 64; A.width 64"),
]
LEAN = [(32, 9), (48, 24), (88, 48)]  # (keep, nq) at b = 8, fused


def _lds(nq, keep):
    """Dynamic LDS of the fused launch: S padded to whole 32-column tiles."""
    return 4 * nq * 8 * 32 * -(-keep // 32)


def _rows_from(keep):
    """First column of the slice ts_nn_rows_kernel writes (a last slice of <= 16 columns after
    whole slices of 128), or None."""
    last = keep % 128
    return keep - last if keep > 128 and 0 < last <= 16 else None


# ----------------------------------------------------------------------------- inputs
def _build(n, b, nq, keep):
    """(Q, W as (nq, n, b) fp32, S (c, keep) fp32, theta fp64)."""
    c = nq * b
    if n >= c:
        q64, q32 = _basis(n, c, 1000 + c)
    else:  # (n = 37: fewer rows than columns, so orthonormal rows)
        q64, q32 = (np.ascontiguousarray(a.T) for a in _basis(c, n, 1000 + c))
    s64, s32 = _basis(c, keep, 2000 + 7 * c + keep)
    rng = np.random.default_rng(31 * n + 5 * c + keep)
    theta = np.sort(rng.uniform(1.0, 100.0, keep))[::-1].copy()
    assert (np.diff(theta) < 0).all() and theta[0] <= 100.0 and theta[-1] >= 1.0
    w64 = ((q64 @ s64) * theta) @ s64.T + rng.standard_normal((n, c)) * (1e-4 / np.sqrt(n))
    blocks = lambda a: np.ascontiguousarray(a.astype(np.float32).reshape(n, nq, b)
                                            .transpose(1, 0, 2))
    return _ro(blocks(q32), blocks(w64), s32, theta)


_case = functools.lru_cache(maxsize=None)(_build)  # (the n = 4,099 and n = 37 cases, shared)


def _flat(blocks):
    """(nblk, n, b) blocks -> (n, nblk b)."""
    return blocks.transpose(1, 0, 2).reshape(blocks.shape[1], -1)


def _identity(eng, n):
    eng.set_layers([sp.identity(n, dtype=np.float32, format="csr")])


# ----------------------------------------------------------------------------- the checks
_FRAC = {}  # kernel family -> largest fraction of its bound so far


def _note(family, frac):
    _FRAC[family] = max(_FRAC.get(family, 0.0), frac)
    return _FRAC[family]


def _check_product(what, family, A, S, got, rows_from=None):
    """got (blocks) against A S in np.longdouble, entrywise within gamma32(2 ca) |A| |S|; no NaN
    left.  Columns from rows_from on count for the ts_nn_rows family."""
    A, got = _flat(A), _flat(got)
    n, ca = A.shape
    assert got.shape == (n, S.shape[1]) and got.dtype == np.float32
    bad = np.flatnonzero(np.isnan(got).any(1))
    assert bad.size == 0, (what, "NaN left in rows", bad[:8], "of", n)
    g = LD(_gamma(2 * ca, U32))
    Sl, Sa = S.astype(LD), np.abs(S).astype(np.float64)
    frac = np.zeros(S.shape[1])
    for r0 in range(0, n, 32768):
        a = A[r0:r0 + 32768]
        ref = np.einsum("nk,kj->nj", a.astype(LD), Sl)
        mag = np.abs(a).astype(np.float64) @ Sa
        frac = np.maximum(frac, (np.abs(got[r0:r0 + 32768].astype(LD) - ref) / (g * mag)).max(0)
                          .astype(np.float64))
    parts = [(family, frac)] if rows_from is None else [(family, frac[:rows_from]),
                                                        ("ts_nn_rows", frac[rows_from:])]
    for fam, f in parts:
        print(f"ritz_step {what}: {fam} worst |got - ref| / bound = {f.max():.4f}"
              f" (family so far {_note(fam, float(f.max())):.4f})")
    assert frac.max() <= 1.0, (what, float(frac.max()), "column", int(frac.argmax()))


def _resid_ref(X, MX, theta):
    """sum_r (MX - theta X)^2 in np.longdouble, theta x formed exactly (module docstring)."""
    assert np.finfo(LD).nmant >= 63
    x, m = _flat(X).astype(LD), _flat(MX).astype(LD)
    hi = theta.astype(np.float32).astype(np.float64)
    lo = theta - hi
    v = (m - hi.astype(LD) * x) - lo.astype(LD) * x
    return (v * v).sum(0)


def _check_resid(what, ref, res, n):
    assert res.dtype == np.float64 and res.shape == ref.shape
    assert np.isfinite(res).all(), (what, res)
    frac = (np.abs(res.astype(LD) - ref) / (LD(_gamma(n + 16, U64)) * ref)).astype(np.float64)
    print(f"ritz_step {what}: resid worst |res - ref| / bound = {frac.max():.4f}"
          f" (family so far {_note('resid', float(frac.max())):.4f}); rms |v|"
          f" {float(np.sqrt((ref / n).max())):.1e} against theta_1 rms |x| {100 / np.sqrt(n):.1e}")
    assert frac.max() <= 1.0, (what, float(frac.max()), "column", int(frac.argmax()))


def _run(eng, what, inputs, b, nq, keep, fused, launches, n_total=None):
    """One non-lean step, every check; returns (X, MX, res, info)."""
    Q, W, S, theta = inputs
    X, MX, res, info = eng.ritz_step(Q, W, S, theta)
    print(f"ritz_step {what}: info {info}")
    assert (info["fused"], info["launches"]) == (fused, launches), info
    assert info["lds_bytes"] == (_lds(nq, keep) if fused else 0), info
    fam, rf = "fused" if info["fused"] else "ts_nn", _rows_from(keep)
    _check_product(what + " X", fam, Q, S, X, rf)
    _check_product(what + " MX", fam, W, S, MX, rf)
    if n_total is None:
        _check_resid(what, _resid_ref(X, MX, theta), res, Q.shape[1])
    return X, MX, res, info


def _run_lean(eng, what, inputs, nq, keep, X_full):
    Q, W, S, theta = inputs
    X, MX, res, info = eng.ritz_step(Q, None, S, theta, lean=True)
    assert MX is None and res is None
    assert (info["fused"], info["launches"], info["lds_bytes"]) == (1, 1, _lds(nq, keep)), info
    assert not np.isnan(X).any(), what
    assert np.array_equal(X.view(np.uint32), X_full.view(np.uint32)), (what, "lean X differs")


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("b,keep,nq,fused,launches,why", CASES,
                         ids=[f"b{c[0]}-keep{c[1]}-nq{c[2]}" for c in CASES])
def test_branches(engine, b, keep, nq, fused, launches, why):
    _identity(engine, N0)
    X, MX, res, info = _run(engine, f"b {b} keep {keep} nq {nq}", _case(N0, b, nq, keep), b, nq,
                            keep, fused, launches)
    if (keep, nq) == (96, 50):
        assert info["lds_bytes"] == 153600
    if (b, keep, nq) in [(8, k, q) for k, q in LEAN]:
        _run_lean(engine, f"lean keep {keep} nq {nq}", _case(N0, b, nq, keep), nq, keep, X)


@pytest.mark.parametrize("keep,nq,fused,launches", [(32, 5, 1, 1), (104, 20, 0, 2)])
def test_one_tile_and_five_rows(engine, keep, nq, fused, launches):
    """n = 37: one full 32-row tile and 5 rows; one residual chunk."""
    _identity(engine, 37)
    _run(engine, f"n 37 keep {keep}", _case(37, 8, nq, keep), 8, nq, keep, fused, launches)


def test_grid_stride_wraps(engine):
    """n = 70,001: 2,188 tiles for the fused launch's 2,048 waves, so the grid-stride loop wraps
    with one pass (lean) and with two; 69 residual chunks."""
    n = 70_001
    assert -(-n // 32) == 2188 and -(-n // 1024) == 69
    _identity(engine, n)
    inputs = _build(n, 8, 9, 32)
    X, MX, res, info = _run(engine, "n 70,001", inputs, 8, 9, 32, 1, 1)
    _run_lean(engine, "n 70,001 lean", inputs, 9, 32, X)


def test_residual_chunk_cap(engine):
    """n = 262,147: ceil(n / 1024) = 257 chunks are capped at 256, of 1,025 rows each."""
    n = 262_147
    assert -(-n // 1024) == 257 and -(-n // 256) == 1025 and -(-n // 1025) == 256
    _identity(engine, n)
    _run(engine, "n 262,147", _build(n, 8, 5, 32), 8, 5, 32, 1, 1)


@pytest.mark.parametrize("b,keep,nq,fused,launches", [(8, 48, 24, 1, 1), (32, 160, 7, 0, 4)])
def test_partitioned(b, keep, nq, fused, launches):
    """Three simulated ranks: each rank's rows of X and MX within the product bound, the same
    all-reduced res on every rank, within the residual bound of the reference over all rows."""
    Q, W, S, theta = _case(N0, b, nq, keep)

    def fn(eng, r):
        _identity(eng, N0)
        _, world, row0, nl = eng.dist_info()
        assert world == 3
        inputs = (Q[:, row0:row0 + nl], W[:, row0:row0 + nl], S, theta)
        return (row0, nl) + _run(eng, f"rank {r} b {b} keep {keep}", inputs, b, nq, keep, fused,
                                 launches, n_total=N0)

    out = _run_ranks(3, fn)
    assert [o[0] for o in out] == list(np.cumsum([0] + [o[1] for o in out[:-1]]))
    assert sum(o[1] for o in out) == N0
    X = np.concatenate([o[2] for o in out], axis=1)
    MX = np.concatenate([o[3] for o in out], axis=1)
    for o in out[1:]:
        assert np.array_equal(o[4].view(np.uint64), out[0][4].view(np.uint64)), "res differs"
    _check_resid(f"3 ranks b {b} keep {keep}", _resid_ref(X, MX, theta), out[0][4], N0)


# ----------------------------------------------------------------------------- the handle after
def test_handle_left_usable(engine):
    """A fit after the call gives the bits of a fit without it, and the results of the fit before
    it stay readable."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    d, seed = int(fx["dims"].max()), int(fx["seed"])
    engine.set_layers(layers)

    def fit():
        engine.uase(d, seed=seed)
        return engine.singular_values(), engine.embedding(), engine.left_embedding()

    fit()
    ref = fit()  # (a fit after a fit, as the one below is)
    n = layers[0].shape[0]
    _run(engine, "er_cfg1 fused", _build(n, 8, 9, 32), 8, 9, 32, 1, 1)
    _run(engine, "er_cfg1 slices", _build(n, 16, 11, 144), 16, 11, 144, 0, 4)
    after = (engine.singular_values(), engine.embedding(), engine.left_embedding())
    again = fit()
    for a, b, c in zip(ref, after, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bad_arguments(engine):
    """Every refusal is N2V2R_ERR_BAD_ARG, writes nothing, and leaves the handle working."""
    from node2vec2rank_amd import _lib
    n = 37
    _identity(engine, n)
    Q, W, S, theta = _case(n, 8, 5, 32)
    buf = lambda *shape: np.zeros(shape, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(eng, b, nq, keep, lean, q=Q, w=W, s=S, th=theta, x=True, mx=True, res=True):
        pb = max(1, keep // b)
        out = (buf(pb, n, b) if x else None, buf(pb, n, b) if mx else None,
               np.zeros(keep) if res else None)
        info = _lib.RitzInfo()
        st = eng.lib.n2v2r_ritz_step(eng.h, b, nq, keep, lean, ptr(q), ptr(w), ptr(s), ptr(th),
                                     ptr(out[0]), ptr(out[1]), ptr(out[2]), ctypes.byref(info))
        if st != _lib.OK:
            assert all(o is None or not o.any() for o in out), "a refused call wrote an output"
        return st

    big = buf(97 * n * 8)  # (room for every shape named below)
    sbig = buf(776 * 64)
    assert call(engine, 8, 5, 32, 0) == _lib.OK
    for b in (4, 12, 24, 128):                                   # b not in {8, 16, 32, 64}
        assert call(engine, b, 40, 32, 0, q=big, w=big, s=sbig) == _lib.ERR_BAD_ARG, b
    assert call(engine, 8, 5, 28, 0) == _lib.ERR_BAD_ARG         # keep % b
    assert call(engine, 16, 5, 40, 0, q=big, w=big, s=sbig) == _lib.ERR_BAD_ARG
    assert call(engine, 8, 5, 40, 0, s=sbig) == _lib.ERR_BAD_ARG  # keep + b > nq b
    assert call(engine, 8, 97, 32, 0, q=big, w=big, s=sbig) == _lib.ERR_BAD_ARG  # nq b > 768
    assert call(engine, 16, 5, 32, 1, q=big, s=sbig) == _lib.ERR_BAD_ARG  # lean, b != 8
    for miss in ("q", "w", "s", "th"):                           # a pointer the mode needs
        assert call(engine, 8, 5, 32, 0, **{miss: None}) == _lib.ERR_BAD_ARG, miss
    for miss in ("x", "mx", "res"):
        assert call(engine, 8, 5, 32, 0, **{miss: False}) == _lib.ERR_BAD_ARG, miss
    for miss in ("q", "s", "th"):
        assert call(engine, 8, 5, 32, 1, w=None, **{miss: None}) == _lib.ERR_BAD_ARG, miss
    assert call(engine, 8, 5, 32, 1, w=None, mx=False, res=False) == _lib.OK  # lean needs no more
    multi = _lib.Engine.multi([0, 0])                            # a multi-GPU parent handle
    try:
        _identity(multi, N0)
        assert call(multi, 8, 5, 32, 0) == _lib.ERR_BAD_ARG
    finally:
        multi.close()
    _run(engine, "after the refusals", (Q, W, S, theta), 8, 5, 32, 1, 1)
