"""The step from a converged fit's left vectors to the embedding on its own (``n2v2r_embed_step``:
the solver's ``build_embedding`` behind a ``GramOp`` set up as a fit's) in every form the products
take -- the CSR row kernels on strided panels with the ``colscale`` pointer offset per slice
(``spmm8_pipe_kernel<2|4|8>``, ``spmm_csr_panel_kernel<8|16|32|64, .>``), the tiled SpMM on
8-column slices followed by ``scale_cols_kernel``, ``dense_gemm_kernel<2>`` on 64-column slices
with the scale in the split-K fold, and on a row partition the packed keys, the two all-reduces
and the products on the gathered U -- read back through ``n2v2r_get_embedding``,
``n2v2r_get_left_embedding`` and ``n2v2r_get_singular_values``.  No ``align_signs`` anywhere: the
sign pass is what is under test.

Signs (exact).  s_j = the sign of U[r*, j], r* the smallest row among those that hold the
column's largest |u| (fp32 values, +1 for a zero entry); the signed U is U * s bit for bit,
``left_embedding()`` = fl32(U s fl32(sqrt sigma_j)) bit for bit (a -0 where sigma = 0 and the
signed entry is negative), ``singular_values()`` = sqrt(max(theta, 0)) exactly.  With one unit
permutation layer, Y[i, j] = fl32(U[p(i), j] s_j sc_j), sc_j = fl32(1 / sqrt(sigma_j)), exactly.
Every column carries one planted case, rows taken from the chunk length ``info`` reports: the
winner in row 0, in row n - 1, in the last row of chunk 0, the first of chunk 1, rows r0 + 7 and
r0 + 8 of a middle chunk (where the eight row lanes wrap), exact ties +a / -a inside a chunk and
across a chunk boundary in both orders, a column of one magnitude (row 0 negative), an all-zero
column, an all-subnormal column.  Every other entry of a column is <= 1/32 of its winner (asserted
on the CPU with the issue's factor 30) and has the sign opposite to the expected one, so a pass
that lands on any other row gives the wrong sign.  theta: ordinary values, and 0, -1e-12 (sigma =
scale = 0: a zero Y column) and 1e-30 (scale 3.2e7) in three columns.  n = 257 and 4,099 (prime)
with d around the 32-column tile and where ldu goes from 64 to 128; n = 262,147, the first size
past the 1,024-chunk cap (257 rows per chunk).

Products (derived bound, every element of every Y_k).  U = the fp32 rounding of an
fp64-orthonormal factor with the same planted columns (but the subnormal one: the bound below
assumes no underflow), K = 3 CSR layers (directed weighted; symmetric unit; weighted with 700-entry
hub rows and a hub column, rows 1000..1099 and every column = 3 mod 11 empty), d = 65, so that every
block width makes at least two slices.  Reference: ref = (A_k^T (U s)) sc in np.longdouble from the
fp32 arrays (sparse layers: each product in fp64, where an fp32 x fp32 product is exact, the sums
and the scale in np.longdouble; dense layers: a np.longdouble matrix product).
    |Y - ref| <= (gamma32(2 L + 2) + gamma64(L)) (|A_k|^T |U|)_ij sc_j
gamma_t(m) = m u_t / (1 - m u_t), u32 = 2^-24, u64 = 2^-53, L the entry count of that row of A_k^T
(n for a dense layer): two roundings per product (test_gpu_wide_pass.py's convention: it covers an
uncontracted multiply-add and the MFMA), two for the scale, and a gamma64(L) term for the
reference's own sums (generous where np.longdouble is wider than fp64, right where it is not).  An
empty row and a column with sigma = 0 must be exactly zero.  Every case asserts ``info``'s form,
launch count and, for the row kernels, rows per wave; U and sigma are checked exactly in every case.

Measured on an MI355X: 31 cases, about 5 s together (the slowest, test_row_kernels_b8
at mean degree 70, 0.5 s, most of it the np.longdouble reference on the host; test_signs_exact at
n = 262,147 0.3 s).  Largest fractions of the bound reached: spmm8_pipe_kernel<8> 0.461, <4>
0.161, <2> 0.042; spmm_csr_panel_kernel<8, 1> 0.027, <16, 8>, <32, 4> and <64, 2> 0.461 each (the
same U and layers as <8>: rows of one or two entries, where the bound is gamma32(4) against up to
two roundings); the tiled SpMM + scale_cols_kernel 0.465 with N2V2R_SPMM_VW=0 and =2 alike;
dense_gemm_kernel<2> 0.025; partitioned 0.479 (row kernels), 0.464 (tiled), 0.0032 (dense).  With
the same U bits every rank's signed rows are bit-equal to the one-GPU result: the sign pass itself
cannot disagree between a partitioned and a one-GPU run.  (Two fits still can: their U differ in
the last bits, so test_gpu_dist.py keeps its alignment.)

Kernel changes that must fail this file (each tried once on a scratch copy):
colmax_partial_kernel keyed by row instead of ~row, decoded likewise (30 of 31 cases fail: every tie
goes to the larger row); colmax_partial_kernel without row0 (the six partitioned cases);
colmax_sign_kernel with <= (30 cases: the all-zero column comes back as -0); the row path's
a.colscale without + q * b (every row-kernel case with d > 8); the dense path's colscale without
+ q * 64 (the four dense cases); the tiled path's a.Y[k] without + q * 8 (the six tiled cases);
scale_cols_kernel indexing s[e % (w / 2)] (test_signs_exact at d = 64 and 100 through the sign
pass's own scaling of U, and the tiled cases with ldu = 128); colmax_fold_kernel comparing only
the high words, in its loop and in its shuffle steps (19 cases: the ties across a middle chunk
boundary wherever there are more than two chunks, 7 | 8 of 17 and 509 | 510 of 1,021 among them;
with two chunks lane 0 keeps chunk 0's key on a tie and is right by accident).  Every one of
them is observable."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import fixture_layers, load_fixture
from test_gpu_dist import _run_ranks
from test_gpu_gram_apply import RPW_BY_MEAN, _same_bits
from test_gpu_pip_pass import _basis, _gamma, _ro, U32, U64
from test_gpu_spmm_prefetch import _layer as _er_layer

pytestmark = pytest.mark.gpu

N0 = 4099
NCASE = 14
HUB = 700
BAND = (1000, 1100)


# ----------------------------------------------------------------------------- inputs
def _theta(d, seed):
    """Ordinary Ritz values, and 0, 1e-30 and -1e-12 in columns 2, 5 and 8 where they exist."""
    th = np.random.default_rng(seed).uniform(0.5, 4.0, d)
    for j, v in ((2, 0.0), (5, 1e-30), (8, -1e-12)):
        if j < d:
            th[j] = v
    return _ro(th)


def _plant(base, rows, chunks, flip, subnormal=True):
    """Column j of `base` (n x d fp32) gets planted case j % 14 with a = 32 max |column|; returns
    (U, e), e the signs the cases are built to give.  flip: every other entry gets the sign
    opposite to e_j.  rows, chunks: the column-max pass's chunk length and count."""
    n, d = base.shape
    assert chunks >= 2 and rows * (chunks - 1) < n <= rows * chunks
    r0 = (chunks // 2) * rows
    assert r0 + 20 < n
    U = np.array(base, dtype=np.float32)
    e = np.ones(d, dtype=np.float32)
    for j in range(d):
        c = j % NCASE
        a = np.float32(32.0) * np.abs(U[:, j]).max()
        put = {0: {rows - 1: -a, rows: a},          # tie across chunks 0 | 1: the smaller row
               1: {0: a},
               2: {n - 1: -a},
               3: {rows - 1: -a},                   # last row of chunk 0
               4: {rows: -a},                       # first row of chunk 1
               5: {r0 + 7: -a},                     # the eight row lanes wrap between these two
               6: {r0 + 8: a},
               7: {r0 + 3: a, r0 + 20: -a},         # ties inside one chunk
               8: {r0 + 3: -a, r0 + 20: a},
               9: {r0 - 1: a, r0: -a},              # ties across a middle chunk boundary
               10: {r0 - 1: -a, r0: a},
               13: {n - 1: -a}}.get(c)
        if c == 11:      # one magnitude everywhere, row 0 negative
            U[:, j] = a
            U[0, j] = -a
            e[j] = -1
            continue
        if c == 12:      # all zero
            U[:, j] = 0
            continue
        if c == 13 and subnormal:  # all subnormal: the winner 2^-130, the rest <= 2^-135
            k = np.random.default_rng(j).integers(1, 2 ** 14 + 1, size=n)
            U[:, j] = (k * 2.0 ** -149).astype(np.float32)
            U[n - 1, j] = -np.float32(2.0 ** -130)
            assert np.abs(U[:, j]).max() < np.finfo(np.float32).tiny and (U[:, j] != 0).all()
            e[j] = -1
            continue
        e[j] = 1 if min(put.items())[1] > 0 else -1
        if flip:
            U[:, j] = -e[j] * np.abs(U[:, j])
        for r, v in put.items():
            U[r, j] = v
    return U, e


def _ref_signs(U):
    """The issue's reference on the fp32 values, after asserting that it is unambiguous: every
    entry that does not hold the column's largest magnitude bit for bit is below 1/30 of it."""
    a = np.abs(U)
    m = a.max(0)
    rest = np.where(a == m, np.float32(0), a).max(0)
    assert (m.astype(np.float64) >= 30.0 * rest.astype(np.float64)).all()
    r = (a == m).argmax(0)
    return np.where(U[r, np.arange(U.shape[1])] < 0, -1, 1).astype(np.float32), r


def _scales(theta):
    sigma = np.sqrt(np.maximum(theta, 0.0))
    with np.errstate(divide="ignore"):
        sc = np.where(sigma > 0, 1.0 / np.sqrt(sigma), 0.0).astype(np.float32)
    return sigma, sc


def _check_left(eng, U, theta, rows=slice(None)):
    """singular_values() and left_embedding() exactly; returns (U s, sc)."""
    s, _ = _ref_signs(U)
    sigma, sc = _scales(theta)
    sv = eng.singular_values()
    assert sv.dtype == np.float64 and np.array_equal(sv, sigma), (sv, sigma)
    Us = U * s
    X = eng.left_embedding()
    want = (Us * np.sqrt(sigma).astype(np.float32))[rows]
    assert X.dtype == np.float32 and X.shape == want.shape
    bad = np.flatnonzero((X.view(np.uint32) != want.view(np.uint32)).any(0))
    assert bad.size == 0, ("left_embedding differs in columns", bad, "signs", s[bad])
    return Us, sc


def _layers3(n, mean, seed):
    """K = 3: directed weighted; symmetric unit; weighted with two 700-entry hub rows and one hub
    column, rows 1000..1099 empty and every column = 3 mod 11 empty."""
    hub = min(HUB, n // 3)
    rng = np.random.default_rng(seed + 7)
    c = _er_layer(seed + 2, n, mean, "dw").tocoo()
    okc = np.flatnonzero(np.arange(n) % 11 != 3)
    okr = np.flatnonzero((np.arange(n) < BAND[0]) | (np.arange(n) >= BAND[1]))
    keep = ((c.row < BAND[0]) | (c.row >= BAND[1])) & (c.col % 11 != 3)
    rows, cols = [c.row[keep]], [c.col[keep]]
    for r in (5, n - 2):
        rows.append(np.full(hub, r))
        cols.append(rng.choice(okc, size=hub, replace=False))
    rows.append(rng.choice(okr, size=hub, replace=False))
    cols.append(np.full(hub, 7))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A2 = sp.csr_matrix((rng.uniform(0.5, 2.0, rows.size).astype(np.float32), (rows, cols)),
                       shape=(n, n))
    A2.sum_duplicates()
    assert A2[BAND[0]:BAND[1]].nnz == 0 and A2[:, 3::11].nnz == 0
    assert np.diff(A2.indptr)[5] >= hub and np.diff(A2.tocsc().indptr)[7] >= hub
    layers = [_er_layer(seed, n, mean, "dw"), _er_layer(seed + 1, n, mean, "su"), A2]
    assert abs(layers[0] - layers[0].T).nnz != 0 and abs(layers[1] - layers[1].T).nnz == 0
    assert (layers[1].data == 1).all()
    return layers


@functools.lru_cache(maxsize=None)
def _csr_layers(n, mean):
    return _layers3(n, mean, 40 * n + mean)


@functools.lru_cache(maxsize=None)
def _dense_layers(n):
    rng = np.random.default_rng(n)
    a, s = (rng.standard_normal((n, n)).astype(np.float32) for _ in range(2))
    return [a, s + s.T]


@functools.lru_cache(maxsize=None)
def _prod_u(n, d, rows, chunks):
    """The fp32 rounding of an fp64-orthonormal n x d factor with the planted columns."""
    U, e = _plant(_basis(n, d, 11 * n + d)[1], rows, chunks, flip=False, subnormal=False)
    assert np.array_equal(_ref_signs(U)[0], e)
    return _ro(U)


def _chunk_plan(eng, n, d, theta, b=8):
    """info of the step on an all-zero U (signs +1, U and every Y_k zero): the chunk length the
    planted rows are taken from."""
    info = eng.embed_step(np.zeros((n, d), np.float32), theta, b=b)
    assert not eng.left_embedding().any() and not eng.embedding().any()
    assert not np.signbit(eng.left_embedding()).any()
    return info


# ----------------------------------------------------------------------------- the product check
_REF = {}   # key -> per layer (A_k^T (U s), |A_k|^T |U|, L) in fp64, computed once
_FRAC = {}  # kernel family -> the largest fraction of the bound reached


def _ld_spmm(At, X64):
    """At X in np.longdouble for a CSR matrix and a panel that both hold fp32 values: each
    product is exact in fp64, the sums run in np.longdouble over each row's entries."""
    At = At.tocsr()
    out = np.zeros((At.shape[0], X64.shape[1]), dtype=np.longdouble)
    rows = np.flatnonzero(np.diff(At.indptr))
    if rows.size:
        v = At.data.astype(np.float64)[:, None]
        for j in range(0, X64.shape[1], 8):
            prod = (v * X64[At.indices, j:j + 8]).astype(np.longdouble)
            out[rows, j:j + 8] = np.add.reduceat(prod, At.indptr[:-1][rows], axis=0)
    return out


def _product_ref(key, layers, Us):
    if key not in _REF:
        out = []
        Us64 = Us.astype(np.float64)
        for A in layers:
            if sp.issparse(A):
                At = A.T.tocsr()
                L = np.diff(At.indptr).astype(np.float64)
                P, S = _ld_spmm(At, Us64), abs(At).astype(np.float64) @ np.abs(Us64)
            else:
                L = np.full(A.shape[0], float(A.shape[0]))
                P = A.T.astype(np.longdouble) @ Us.astype(np.longdouble)
                S = np.abs(A).T.astype(np.float64) @ np.abs(Us64)
            assert P.dtype == np.longdouble
            out.append(_ro(P, np.asarray(S), L))
        _REF[key] = out
    return _REF[key]


def _check_products(family, key, layers, Us, sc, Y):
    """Every element of every Y_k against the derived bound; returns the largest fraction."""
    n, d = Us.shape
    assert Y.dtype == np.float32 and Y.shape == (len(layers), n, d)
    assert not np.isnan(Y).any(), (family, "NaN in Y: rows", np.flatnonzero(np.isnan(Y).any((0, 2))))
    scl = sc.astype(np.longdouble)
    worst = 0.0
    for k, (P, S, L) in enumerate(_product_ref(key, layers, Us)):
        ref = P.astype(np.longdouble) * scl
        bound = ((_gamma(2 * L + 2, U32) + _gamma(L, U64))[:, None] * S).astype(np.longdouble) * scl
        err = np.abs(Y[k].astype(np.longdouble) - ref)
        zero = bound == 0
        assert not err[zero].any(), (family, k, "an element that must be exactly zero is not")
        frac = float((err[~zero] / bound[~zero]).max())
        i, j = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))),
                                err.shape)
        print(f"embed_step {family} layer {k}: fraction of the bound {frac:.4f} at ({i}, {j})")
        assert frac <= 1.0, (family, key, k, frac, (int(i), int(j)))
        worst = max(worst, frac)
    _FRAC[family] = max(_FRAC.get(family, 0.0), worst)
    print(f"embed_step {family}: largest fraction so far {_FRAC[family]:.4f}")
    return worst


def _ldu(d):
    return 64 * -(-d // 64)


# ----------------------------------------------------------------------------- signs, exactly
SIGN_SHAPES = [(257, 1)] + [(N0, d) for d in (1, 31, 32, 33, 64, 65, 100)] + [(262_147, 33)]


@pytest.mark.parametrize("n,d", SIGN_SHAPES)
def test_signs_exact(engine, monkeypatch, n, d):
    """One unit permutation layer: U s, sigma, the left embedding and Y all exact."""
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    rng = np.random.default_rng(1000 * n + d)
    p = rng.permutation(n)
    A = sp.csr_matrix((np.ones(n, np.float32), (p, np.arange(n))), shape=(n, n))  # A[p(i), i] = 1
    engine.set_layers([A])
    theta = _theta(d, n + d)
    info0 = _chunk_plan(engine, n, d, theta)
    rows, chunks = info0["colmax_rows"], info0["colmax_chunks"]
    if n == 262_147:
        assert (rows, chunks) == (257, 1021), info0  # past the 1,024-chunk cap
    noise = (rng.uniform(0.25, 1.0, (n, d)) * 1e-3).astype(np.float32)
    U, e = _plant(noise, rows, chunks, flip=True)
    s, win = _ref_signs(U)
    assert np.array_equal(s, e), "the planted cases and the reference disagree"
    info = engine.embed_step(U, theta)
    print("embed_step info", info)
    assert info == info0
    assert (info["form"], info["ldu"], info["launches"], info["rpw"]) == \
        (0, _ldu(d), _ldu(d) // 8, 8), info
    Us, sc = _check_left(engine, U, theta)
    Y = engine.embedding()
    assert Y.shape == (1, n, d) and not np.isnan(Y).any()
    want = Us[p] * sc
    bad = np.flatnonzero((Y[0] != want).any(0))
    assert bad.size == 0, ("Y differs in columns", bad)
    for j in (2, 8):
        if j < d:
            assert not Y[0, :, j].any() and s[j] == -1
    # again: the same bits
    assert engine.embed_step(U, theta) == info
    assert _same_bits(engine.embedding(), Y)


# ----------------------------------------------------------------------------- CSR row kernels
def _rows_case(engine, monkeypatch, family, mean, b, rpw):
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    n, d = N0, 65
    layers = _csr_layers(n, mean)
    engine.set_layers(layers)
    theta = _theta(d, mean)
    info0 = _chunk_plan(engine, n, d, theta, b=b)
    U = _prod_u(n, d, info0["colmax_rows"], info0["colmax_chunks"])
    info = engine.embed_step(U, theta, b=b)
    print("embed_step info", info)
    assert info == info0
    assert (info["form"], info["ldu"], info["launches"]) == (0, 128, 128 // b), info
    assert info["rpw"] == rpw, (mean, b, info)
    Us, sc = _check_left(engine, U, theta)
    _check_products(family, ("rows", mean), layers, Us, sc, engine.embedding())


@pytest.mark.parametrize("mean,rpw", RPW_BY_MEAN)
def test_row_kernels_b8(engine, monkeypatch, mean, rpw):
    """spmm8_pipe_kernel<8 | 4 | 2> and, at one row per wave, spmm_csr_panel_kernel<8, 1>:
    sixteen slices of a 128-float row, colscale + 8 q."""
    kern = "spmm_csr_panel_kernel<8,1>" if rpw == 1 else f"spmm8_pipe_kernel<{rpw}>"
    _rows_case(engine, monkeypatch, kern, mean, 8, rpw)


# rows per wave at mean row length 5 (auto_rpw with B / 4 lanes per panel row: the row group of
# 64 / rpw lanes shrinks while 64 / (2 rpw) >= B / 4 and >= (B / 4) mean / 3.5)
RPW_WIDE = {16: 8, 32: 4, 64: 2}


@pytest.mark.parametrize("b", [16, 32, 64])
def test_row_kernels_wide(engine, monkeypatch, b):
    _rows_case(engine, monkeypatch, f"spmm_csr_panel_kernel<{b},{RPW_WIDE[b]}>", 5, b, RPW_WIDE[b])


# ----------------------------------------------------------------------------- tiled form
@pytest.mark.parametrize("d", [8, 72])
@pytest.mark.parametrize("n", [2049, 4160])
def test_tiled(engine, monkeypatch, n, d):
    """8-column slices of U through the tiled SpMM into rows ldu floats apart, then
    scale_cols_kernel; the register-window form byte-equal to the LDS-only one."""
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    monkeypatch.setenv("N2V2R_SPMM_TILE_NB", "4")
    monkeypatch.delenv("N2V2R_SPMM_WBITS", raising=False)
    layers = _csr_layers(n, 3)
    engine.set_layers(layers)
    theta = _theta(d, n)
    out = {}
    for vw in (0, 2):
        monkeypatch.setenv("N2V2R_SPMM_VW", str(vw))
        info0 = _chunk_plan(engine, n, d, theta)
        U = _prod_u(n, d, info0["colmax_rows"], info0["colmax_chunks"])
        info = engine.embed_step(U, theta)
        print("embed_step info", info)
        assert info == info0
        assert (info["form"], info["ldu"], info["launches"], info["rpw"]) == \
            (5, _ldu(d), _ldu(d) // 8, 0), info
        Us, sc = _check_left(engine, U, theta)
        out[vw] = engine.embedding()
        _check_products(f"tiled VW={vw} + scale_cols_kernel", ("tiled", n, d), layers, Us, sc,
                        out[vw])
    assert _same_bits(out[0], out[2]), "Y differs between the LDS-only and register windows"


# ----------------------------------------------------------------------------- dense layers
@pytest.mark.parametrize("n", [257, 1037])
def test_dense(engine, n):
    """dense_gemm_kernel<2> on two 64-column slices (ldx = ldu = 128), colscale + 64 q in the
    split-K fold; lda is padded at n = 1,037.  K = 2, layer 0 directed."""
    d = 65
    layers = _dense_layers(n)
    engine.set_layers(layers, storage="dense", symmetric=-1)
    theta = _theta(d, n)
    info0 = _chunk_plan(engine, n, d, theta)
    U = _prod_u(n, d, info0["colmax_rows"], info0["colmax_chunks"])
    info = engine.embed_step(U, theta)
    print("embed_step info", info)
    assert info == info0
    assert (info["form"], info["ldu"], info["launches"], info["rpw"]) == (4, 128, 4, 0), info
    Us, sc = _check_left(engine, U, theta)
    _check_products("dense_gemm_kernel<2>", ("dense", n), layers, Us, sc, engine.embedding())


# ----------------------------------------------------------------------------- row partition
def _plant_ranks(base, world):
    """Winners in the last rank's rows (so every other rank takes the sign from its owner), ties
    across the boundary between ranks 0 and 1 and between the first and the last rank (the
    smaller global row decides), an all-zero column; every other entry has the sign opposite to
    the expected one."""
    n, d = base.shape
    R = -(-n // world)
    last0 = (world - 1) * R
    nl = n - last0
    assert nl > 8 and d > 8
    U = np.abs(np.array(base, dtype=np.float32))
    e = np.ones(d, dtype=np.float32)
    for j in range(d):
        a = np.float32(32.0) * U[:, j].max()
        put = {0: {n - 1: -a}, 1: {last0: a}, 2: {last0 + 5: -a},
               3: {R - 1: -a, R: a}, 4: {R - 1: a, R: -a},
               6: {3: -a, n - 2: a}, 7: {3: a, n - 2: -a}}.get(j)
        if j == 5:
            U[:, j] = 0
            continue
        if put is None:
            put = {last0 + (37 * j) % nl: -a if j % 3 else a}
        e[j] = 1 if min(put.items())[1] > 0 else -1
        U[:, j] *= -e[j]
        for r, v in put.items():
            U[r, j] = v
    assert np.array_equal(_ref_signs(U)[0], e)
    return _ro(U)


def _partition_case(engine, monkeypatch, world, family, key, layers, form, env, **set_kw):
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    n, d = layers[0].shape[0], 65
    U = _plant_ranks(_basis(n, d, n + world)[1], world)
    theta = _theta(d, n)
    # one GPU, the same U
    engine.set_layers(layers, **set_kw)
    one = engine.embed_step(U, theta)
    assert one["form"] == form, one
    Us, sc = _check_left(engine, U, theta)
    Xone, sone = engine.left_embedding(), engine.singular_values()
    _check_products(family + " (one GPU)", key, layers, Us, sc, engine.embedding())

    def fn(eng, r):
        eng.set_layers(layers, **set_kw)
        info = eng.embed_step(U, theta)
        return (eng.dist_info(), info, eng.embedding(), eng.left_embedding(),
                eng.singular_values())
    res = _run_ranks(world, fn)
    R = -(-n // world)
    for g, (di, info, Y, X, sv) in enumerate(res):
        assert di == (g, world, min(n, g * R), min(n, (g + 1) * R) - min(n, g * R)), di
        assert (info["form"], info["ldu"]) == (form, 128), info
        assert np.array_equal(sv, sone), (g, sv, sone)
        rows = slice(di[2], di[2] + di[3])
        bad = np.flatnonzero((X.view(np.uint32) != Xone[rows].view(np.uint32)).any(0))
        assert bad.size == 0, ("rank", g, "signed U differs from the one-GPU result in columns", bad)
    Y = np.concatenate([r[2] for r in res], axis=1)
    _check_products(family + " (partitioned)", key, layers, Us, sc, Y)


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rows(engine, monkeypatch, world):
    _partition_case(engine, monkeypatch, world, "rows b8", ("prows", world), _csr_layers(N0, 5), 0,
                    {"N2V2R_SPMM_CB": "0"})


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_tiled(engine, monkeypatch, world):
    _partition_case(engine, monkeypatch, world, "tiled", ("ptiled", world), _csr_layers(4160, 3),
                    5, {"N2V2R_SPMM_CB": "1", "N2V2R_SPMM_TILE_NB": "4"})


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_dense(engine, monkeypatch, world):
    _partition_case(engine, monkeypatch, world, "dense", ("pdense", world), _dense_layers(1037),
                    4, {}, storage="dense", symmetric=-1)


# ----------------------------------------------------------------------------- the handle after
def _fit(engine, fx):
    engine.uase(int(fx["dims"].max()), seed=int(fx["seed"]))
    return engine.singular_values(), engine.embedding(), engine.left_embedding()


def test_handle_left_usable(engine):
    """A fit after the step gives the bits of a fit without it."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    n = layers[0].shape[0]
    engine.set_layers(layers)
    _fit(engine, fx)
    ref = _fit(engine, fx)  # (a fit after a fit, as the one below is)
    d = 12
    theta = _theta(d, 3)
    info0 = _chunk_plan(engine, n, d, theta)
    U = _prod_u(n, d, info0["colmax_rows"], info0["colmax_chunks"])
    assert engine.embed_step(U, theta) == info0
    Us, sc = _check_left(engine, U, theta)
    _check_products("er_cfg1", ("er_cfg1",), layers, Us, sc, engine.embedding())
    again = _fit(engine, fx)
    for a, c in zip(ref, again):
        assert a.shape == c.shape and np.array_equal(a, c)


def test_bad_arguments(engine):
    """Every refused call returns N2V2R_ERR_BAD_ARG, reports form -1 and leaves the embedding of
    the fit before it readable."""
    from node2vec2rank_amd import _lib
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    n = layers[0].shape[0]
    engine.set_layers(layers)
    ref = _fit(engine, fx)
    U = np.random.default_rng(0).standard_normal((n, 4)).astype(np.float32)
    theta = np.ones(4)
    for b in (0, 4, 24, 128):
        with pytest.raises(ValueError):
            engine.embed_step(U, theta, b=b)
    wide = np.zeros((n, max(n, 601)), np.float32)
    for d in [0, n] + ([601] if n > 602 else []):   # d outside [1, min(600, n - 1)]
        with pytest.raises(ValueError):
            engine.embed_step(wide[:, :d], np.ones(d))
    ptr = ctypes.c_void_p
    for u, t in ((None, theta.ctypes.data_as(ptr)), (U.ctypes.data_as(ptr), None)):
        info = _lib.EmbedInfo()
        info.form = 7
        assert engine.lib.n2v2r_embed_step(engine.h, 8, 4, u, t, ctypes.byref(info)) == \
            _lib.ERR_BAD_ARG
        assert info.form == -1
    for a, c in zip(ref, (engine.singular_values(), engine.embedding(), engine.left_embedding())):
        assert np.array_equal(a, c)
    # the handle works: a good call, without info too
    assert engine.lib.n2v2r_embed_step(engine.h, 8, 4, U.ctypes.data_as(ptr),
                                       theta.ctypes.data_as(ptr), None) == _lib.OK
    assert engine.embed_step(U, theta)["form"] == 0
    # no layers
    bare = _lib.Engine(0)
    try:
        assert bare.lib.n2v2r_embed_step(bare.h, 8, 4, U.ctypes.data_as(ptr),
                                         theta.ctypes.data_as(ptr), None) == _lib.ERR_BAD_ARG
    finally:
        bare.close()
    # a multi-GPU parent handle: the call belongs to its ranks
    eng = _lib.Engine.multi([0, 0])
    try:
        eng.set_layers(layers)
        with pytest.raises(ValueError):
            eng.embed_step(U, theta)
    finally:
        eng.close()
