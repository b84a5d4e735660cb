"""The fp64 bipartite projection (``syrk_f64_kernel`` through ``n2v2r_project``,
``Engine.project`` and ``ingest.transform``) against numpy, past the one 64 x 64 tile and the
one 16-deep k chunk that the golden ingest fixtures (7 x 12) reach.

The shapes cover r = 1, the 63/64/65 boundaries and 2 to 5 tiles per side (the upper-triangle
tile decode, the mirror store, a partial last tile next to full ones), kd = 1, < 16, = 16, 17,
33 and 100 (a second and later k chunk, a partial one), each in both stride modes: W^T W reads W
with i contiguous (``si == 1``), W W^T with k contiguous (``sk == 1``).

Accuracy bound (derived, not measured): a length-kd fp64 dot product summed in any order, fused
or not, obeys |fl(x.y) - x.y| <= gamma_kd |x|.|y| with gamma_kd = kd u / (1 - kd u), u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The reference is the same
product in ``np.longdouble``.  Integer input makes every partial sum exactly representable, so
there the result must equal the int64 product bit for bit (a dropped or doubled term cannot hide
inside the bound)."""
import contextlib
import ctypes
import functools
import io
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SHAPES = [(7, 12), (3, 64), (17, 65), (33, 130), (100, 193), (16, 257), (1, 70), (70, 1)]
ONS = ["columns", "rows"]
CASES = [(m, n, on) for (m, n) in SHAPES for on in ONS]
U = 2.0 ** -53


def _x(W, on):
    """X with out = X^T X: W for columns, W^T for rows."""
    return W if on == "columns" else W.T


@functools.lru_cache(maxsize=None)
def _real_case(m, n):
    """W = standard_normal * 10^uniform(-3, 3) entrywise (fixed seed per shape)."""
    rng = np.random.default_rng(1000 * m + n)
    W = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-3.0, 3.0, (m, n))
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def _int_case(m, n):
    rng = np.random.default_rng(7000 * m + n)
    W = rng.integers(-8, 9, size=(m, n)).astype(np.float64)
    W.setflags(write=False)
    return W


def _longdouble_ref(X):
    """(X^T X, |X|^T |X|) in np.longdouble."""
    XL = np.asarray(X, dtype=np.longdouble)
    return XL.T @ XL, np.abs(XL).T @ np.abs(XL)


@functools.lru_cache(maxsize=None)
def _real_ref(m, n, on):
    ref, mag = _longdouble_ref(_x(_real_case(m, n), on))
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


def _gamma(kd):
    return kd * U / (1.0 - kd * U)


def _assert_within_bound(got, ref, mag, kd, where=None):
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = np.longdouble(_gamma(kd)) * mag
    if where is None:
        where = np.ones(got.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(where & (bound > 0), err / np.where(bound > 0, bound, 1), 0)
    print(f"kd = {kd}: worst |got - ref| / bound = {float(ratio.max()):.3f}")
    bad = where & ~(err <= bound)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), float(ratio.max()))


# ------------------------------------------------------------------- a. accuracy, real input
@pytest.mark.parametrize("m,n,on", CASES)
def test_project_real_within_dot_product_bound(engine, m, n, on):
    """Every entry of the r x r output (the device buffer is not zeroed: an unwritten tile is
    garbage) within gamma_kd (|X|^T |X|) of the longdouble product."""
    W = _real_case(m, n)
    X = _x(W, on)
    kd, r = X.shape
    got = engine.project(W, on)
    assert got.shape == (r, r) and got.dtype == np.float64
    assert np.isfinite(got).all()
    ref, mag = _real_ref(m, n, on)
    _assert_within_bound(got, ref, mag, kd)


# ------------------------------------------------------------------- b. exactness, integers
@pytest.mark.parametrize("m,n,on", CASES)
def test_project_integer_exact(engine, m, n, on):
    W = _int_case(m, n)
    Xi = _x(W, on).astype(np.int64)
    got = engine.project(W, on)
    np.testing.assert_array_equal(got, (Xi.T @ Xi).astype(np.float64))


# ------------------------------------------------------------------- c. symmetry, determinism
@pytest.mark.parametrize("m,n,on", CASES)
def test_project_symmetric_and_deterministic(engine, m, n, on):
    W = _real_case(m, n)
    a = engine.project(W, on)
    b = engine.project(W, on)
    assert np.array_equal(a, a.T)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------- d. input forms
@pytest.mark.parametrize("on", ONS)
def test_project_input_forms(engine, on):
    """float32, Fortran-ordered and non-contiguous inputs give the bits of their contiguous
    float64 copy."""
    rng = np.random.default_rng(5)
    big = rng.standard_normal((66, 260))
    forms = {
        "float32": big[:33, :130].astype(np.float32),
        "fortran": np.asfortranarray(big[:33, :130]),
        "slice": big[::2, 1::2],
        "transposed": big[:130, :33].T,
    }
    assert forms["fortran"].flags.f_contiguous and not forms["fortran"].flags.c_contiguous
    assert not forms["slice"].flags.c_contiguous and forms["slice"].shape == (33, 130)
    for name, W in forms.items():
        copy = np.ascontiguousarray(W, dtype=np.float64)
        got = engine.project(W, on)
        assert got.tobytes() == engine.project(copy, on).tobytes(), name
        ref, mag = _longdouble_ref(_x(copy, on))
        _assert_within_bound(got, ref, mag, _x(copy, on).shape[0])


# ------------------------------------------------------------------- e. non-finite values
def test_project_non_finite_positions(engine):
    """One NaN and one +inf in W (33 x 130, columns): NaN and +-inf land where numpy puts them;
    every finite entry still obeys the bound."""
    W = _real_case(33, 130).copy()
    W[5, 17] = np.nan      # tile 0
    W[20, 100] = np.inf    # tile 1, another row of W
    got = engine.project(W, "columns")
    with np.errstate(invalid="ignore", over="ignore"):
        ref64 = W.T @ W
        ref, mag = _longdouble_ref(W)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref64))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref64))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref64))
    # the expected pattern itself: NaN along row / column 17, inf along 100, NaN where they meet
    assert np.isnan(ref64[17]).all() and np.isnan(ref64[:, 17]).all()
    assert np.isinf(ref64[100, np.arange(130) != 17]).all() and ref64[100, 100] == np.inf
    fin = np.isfinite(ref64)
    assert fin.sum() == 128 * 128
    assert np.array_equal(got, got.T, equal_nan=True)
    with np.errstate(invalid="ignore"):
        _assert_within_bound(got, ref, mag, 33, where=fin)


# ------------------------------------------------------------------- f. other handle kinds
@pytest.mark.parametrize("on", ONS)
def test_project_multi_engine_same_bits(engine, on):
    from node2vec2rank_amd import _lib
    W = _real_case(33, 130)
    one = engine.project(W, on)
    eng = _lib.Engine.multi([0, 0])
    try:
        two = eng.project(W, on)
    finally:
        eng.close()
    assert one.tobytes() == two.tobytes()


def test_project_between_set_layers_and_uase_leaves_fit_alone(engine):
    """A projection on a handle that holds layers touches none of the fit's state: the singular
    values of the fit after it are those of a fit without it, bit for bit."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(4099, 6, 2)
    engine.set_layers(layers)
    engine.uase(8, seed=3)
    plain = engine.singular_values()
    engine.set_layers(layers)
    W = _int_case(33, 130)
    Xi = W.astype(np.int64)
    np.testing.assert_array_equal(engine.project(W, "columns"), (Xi.T @ Xi).astype(np.float64))
    engine.uase(8, seed=3)
    assert engine.singular_values().tobytes() == plain.tobytes()


# ------------------------------------------------------------------- g. ingest past one tile
class _NumpyEngine:
    """Stands in for the GPU engine in ``ingest.transform``: numpy's float64 matmul, as the
    reference's ``bipartite_to_unipartite_projection``."""

    def project(self, W, on="columns"):
        W = np.asarray(W, dtype=np.float64)
        return W.T @ W if on.casefold() == "columns" else W @ W.T


def _sparse_int_layer(m, n, seed):
    rng = np.random.default_rng(seed)
    vals = rng.integers(-8, 9, size=(m, n)).astype(np.float64)
    vals[rng.random((m, n)) >= 0.3] = 0.0
    return vals


@pytest.mark.parametrize("on,top,absolute,binarize",
                         list(itertools.product(ONS, [100, 30], [False, True], [False, True])))
def test_ingest_transform_matches_numpy_projection(engine, on, top, absolute, binarize):
    """40 x 150 integer-valued layer: the projection is exact, so the percentile cut, the
    surviving entries and their values are those of the numpy pipeline."""
    from node2vec2rank_amd import ingest
    vals = _sparse_int_layer(40, 150, 11)
    layer = ingest.Layer(sp.csr_matrix(vals), [f"r{i}" for i in range(40)],
                         [f"c{j}" for j in range(150)])
    kw = dict(top_percent_keep=top, absolute=absolute, binarize=binarize,
              project_unipartite_on=on)
    ours = ingest.transform(layer, engine=engine, **kw)
    ref = ingest.transform(layer, engine=_NumpyEngine(), **kw)
    side = 150 if on == "columns" else 40
    assert ours.shape == ref.shape == (side, side)
    assert ours.mat.dtype == np.float32 and ours.mat.nnz > 0
    np.testing.assert_array_equal(ours.mat.indptr, ref.mat.indptr)
    np.testing.assert_array_equal(ours.mat.indices, ref.mat.indices)
    np.testing.assert_array_equal(ours.mat.data, ref.mat.data)
    np.testing.assert_array_equal(ours.rows, ref.rows)
    np.testing.assert_array_equal(ours.cols, ref.cols)
    assert list(ours.rows) == list(layer.cols if on == "columns" else layer.rows)


def test_dataloader_bipartite_csv_matches_numpy_projection(engine, tmp_path):
    """Two 20 x 150 bipartite adjacency CSVs through ``DataLoader`` with the GPU engine and with
    the numpy stand-in."""
    import pandas as pd

    from node2vec2rank_amd import ingest
    rows = [f"g{i}" for i in range(20)]
    cols = [f"s{j}" for j in range(150)]
    names = []
    for k in range(2):
        f = tmp_path / f"bip{k}.csv"
        pd.DataFrame(_sparse_int_layer(20, 150, 21 + k).astype(np.int64), index=rows,
                     columns=cols).to_csv(f)
        names.append(f.name)
    cfg = dict(data_dir=str(tmp_path), graph_filenames=names, separator=",", is_edge_list=False,
               transpose=False, project_unipartite_on="columns", threshold=None,
               top_percent_keep=30, binarize=False, absolute=False)
    out = []
    for eng in (engine, _NumpyEngine()):
        with contextlib.redirect_stdout(io.StringIO()):
            out.append(ingest.DataLoader(cfg, engine=eng))
    ours, ref = out
    assert [str(x) for x in ours.get_nodes()] == cols == [str(x) for x in ref.get_nodes()]
    assert len(ours.get_graphs()) == 2
    for g, h in zip(ours.get_graphs(), ref.get_graphs()):
        assert g.shape == (150, 150) and g.dtype == np.float32 and g.nnz > 0
        np.testing.assert_array_equal(g.indptr, h.indptr)
        np.testing.assert_array_equal(g.indices, h.indices)
        np.testing.assert_array_equal(g.data, h.data)


# ------------------------------------------------------------------- h. argument errors
def test_project_argument_errors_leave_handle_usable(engine):
    from node2vec2rank_amd import _lib
    W = _int_case(17, 65)
    with pytest.raises(ValueError):
        engine.project(W, "diagonal")
    # the C entry point itself (the binding's typed signature would refuse a NULL array)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    raw = ctypes.CFUNCTYPE(ctypes.c_int, vp, i64, i64, vp, ctypes.c_int, vp)(
        ("n2v2r_project", engine.lib))
    out = np.empty((65, 65), dtype=np.float64)
    wp, op = W.ctypes.data_as(vp), out.ctypes.data_as(vp)
    assert raw(engine.h, 0, 65, wp, 1, op) == _lib.ERR_BAD_ARG
    assert raw(engine.h, 17, 0, wp, 1, op) == _lib.ERR_BAD_ARG
    assert raw(engine.h, 17, 65, wp, 1, None) == _lib.ERR_BAD_ARG
    assert raw(engine.h, 17, 65, None, 1, op) == _lib.ERR_BAD_ARG
    for on in ONS:
        Xi = _x(W, on).astype(np.int64)
        np.testing.assert_array_equal(engine.project(W, on), (Xi.T @ Xi).astype(np.float64))
