"""Spearman and biweight-midcorrelation co-expression layers on the GPU (corr_rank_kernel,
corr_bicor_kernel in csrc/corr.hip; n2v2r_set_layer_corr_method, n2v2r_soft_connectivity_method)
against scipy and the numpy references of tests/test_cor_methods.py, which checks those
references themselves and states the Z bound.

  * ranks: equal to ``scipy.stats.rankdata`` (exact half-integers);
  * Spearman: bit for bit the Pearson path applied to the rank matrix, at every stage;
  * bicor Z: |Z - longdouble reference| <= 2^-52 (s + 10 + 4 kappa_i) per entry;
  * bicor layers: the suite's layer bound |A - ref| <= 2^-24 |ref| + 1e-12 against fp64 numpy;
  * bicor connectivities: tests/test_gpu_soft_threshold.py's bound with (samples + 20) for its
    (samples + 10): the weights add a handful of roundings per element;
  * a zero-MAD row carries the Pearson kernel's bits and is counted.

S = 2048 is the longest row the kernels stage in LDS (CORR_ROW_LDS, csrc/corr.hip); (5, 2049)
takes the path that reads the row from global memory.
"""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

from oracle import n2v2r_oracle as orc
from test_cor_methods import (SMALL_SHAPES, SUITE_SHAPES, _bicor, _bicor_z, _expression, _tied,
                              _z_ratio)

pytestmark = pytest.mark.gpu

ROW_LDS = 2048
ALL_SHAPES = SUITE_SHAPES + SMALL_SHAPES + [(5, ROW_LDS + 1)]
KINDS = ["unsigned", "signed", "signed hybrid", "raw"]
KIND_POWER = [(k, p) for k in KINDS for p in (1.0, 6.0) if not (k == "raw" and p != 1.0)]
SCAN_KINDS = ["unsigned", "signed", "signed hybrid"]
DEFAULT = tuple(float(p) for p in (*range(1, 11), *range(12, 21, 2)))
INPUTS = ["expression", "tied"]

_E, _R = {}, {}


def _input(name, n, s):
    """The matrix of an input generator and a shape, made once and read-only."""
    if (name, n, s) not in _E:
        e = _expression(n, s, seed=1000 * n + s) if name == "expression" else \
            _tied(n, s, seed=n + s)
        e = np.ascontiguousarray(e)
        e.setflags(write=False)
        _E[(name, n, s)] = e
    return _E[(name, n, s)]


def _rank_matrix(name, n, s):
    if (name, n, s) not in _R:
        r = scipy.stats.rankdata(_input(name, n, s), axis=1)
        r.setflags(write=False)
        _R[(name, n, s)] = r
    return _R[(name, n, s)]


def _adjacency(r, kind, power, dtype=np.float64):
    t = {"unsigned": np.abs(r), "signed": (dtype(1) + r) * dtype(0.5),
         "signed hybrid": np.maximum(r, dtype(0)), "raw": r}[kind]
    return t ** dtype(power) if power != 1.0 else t


def _layer_reference(r, kind, power):
    t = _adjacency(r, kind, power).copy()
    np.fill_diagonal(t, 1.0)
    return t


def _check_layer(A, ref):
    err = np.abs(A.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12
    worst = float((err / bound).max())
    print(f"max |A - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst
    assert np.array_equal(A, A.T)  # bitwise
    assert np.all(np.diag(A) == np.float32(1.0))


# ---- 1. ranks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("n, s", ALL_SHAPES)
def test_ranks_equal_scipy(engine, n, s, name):
    got = engine.corr_ranks(_input(name, n, s))
    assert got.dtype == np.float64
    assert np.array_equal(got, _rank_matrix(name, n, s))


def test_signed_zeros_tie(engine):
    E = _tied(66, 9, seed=4)
    assert np.array_equal(np.signbit(E[1]), [False] * 4 + [True] * 4 + [False])
    assert np.array_equal(E[1], [0.0] * 8 + [1.0])
    R = engine.corr_ranks(E)
    assert np.array_equal(R[1], [4.5] * 8 + [9.0])
    assert np.array_equal(R[2], [9.0] + [4.5] * 8)
    assert np.array_equal(R, scipy.stats.rankdata(E, axis=1))


# ---- 2. Spearman is Pearson of the ranks, bit for bit -----------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("n, s", ALL_SHAPES)
def test_spearman_rows_are_the_pearson_rows_of_the_ranks(engine, n, s, name):
    E, R = _input(name, n, s), _rank_matrix(name, n, s)
    got, bad = engine.corr_standardise(E, "spearman", return_bad_row=True)
    assert bad == -1
    assert np.array_equal(got, engine.corr_standardise(R, "pearson"))
    assert np.abs((got * got).sum(axis=1) - 1.0).max() <= 1e-13


@pytest.mark.parametrize("kind, power", KIND_POWER)
@pytest.mark.parametrize("n, s", [(193, 7), (257, 200)])
def test_spearman_layer_is_the_pearson_layer_of_the_ranks(engine, n, s, kind, power):
    from node2vec2rank_amd import Coexpression
    E, R = _input("expression", n, s), _rank_matrix("expression", n, s)
    engine.set_layers([Coexpression(E, kind=kind, power=power, method="spearman")])
    got = engine.layer_dense(0)
    engine.set_layers([Coexpression(R, kind=kind, power=power)])
    assert np.array_equal(got.view(np.uint32), engine.layer_dense(0).view(np.uint32))
    # and independently of the Pearson path: numpy's correlation of scipy's ranks
    _check_layer(got, _layer_reference(np.corrcoef(R), kind, power))


@pytest.mark.parametrize("kind", SCAN_KINDS)
@pytest.mark.parametrize("n, s", [(193, 7), (257, 200)])
def test_spearman_connectivity_is_the_pearson_connectivity_of_the_ranks(engine, n, s, kind):
    E, R = _input("expression", n, s), _rank_matrix("expression", n, s)
    got = engine.soft_connectivity(E, kind=kind, powers=DEFAULT, method="spearman")
    assert np.array_equal(got, engine.soft_connectivity(R, kind=kind, powers=DEFAULT))


# ---- 3. bicor's standardised rows -------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("n, s", ALL_SHAPES)
def test_bicor_rows_match_longdouble(engine, n, s, name):
    E = _input(name, n, s)
    Z, bad = engine.corr_standardise(E, "bicor", return_bad_row=True)
    assert bad == -1 and Z.shape == (n, s) and np.isfinite(Z).all()
    worst = _z_ratio(Z, E)
    print(f"n={n} s={s} {name}: max |Z - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst


# ---- 4. bicor layers --------------------------------------------------------------------------
_BICOR = {}


def _bicor_r(n, s):
    if (n, s) not in _BICOR:
        _BICOR[(n, s)] = _bicor(_input("expression", n, s))
    return _BICOR[(n, s)]


@pytest.mark.parametrize("kind, power", KIND_POWER)
@pytest.mark.parametrize("n, s", SUITE_SHAPES)
def test_bicor_layer_matches_numpy(engine, n, s, kind, power):
    from node2vec2rank_amd import Coexpression
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no zero-MAD row here: no warning
        engine.set_layers([Coexpression(_input("expression", n, s), kind=kind, power=power,
                                        method="bicor")])
    assert engine.storage == "dense"
    _check_layer(engine.layer_dense(0), _layer_reference(_bicor_r(n, s), kind, power))


# ---- 5. bicor connectivities ------------------------------------------------------------------
_BICOR_LD = {}


def _bicor_r_longdouble(n, s):
    if (n, s) not in _BICOR_LD:
        z = _bicor_z(_input("expression", n, s), np.longdouble)
        _BICOR_LD[(n, s)] = np.clip(z @ z.T, np.longdouble(-1), np.longdouble(1))
    return _BICOR_LD[(n, s)]


@pytest.mark.parametrize("kind", SCAN_KINDS)
@pytest.mark.parametrize("n, s", SUITE_SHAPES + [(70, 2)])
def test_bicor_connectivity_matches_longdouble(engine, n, s, kind):
    r = _bicor_r_longdouble(n, s)
    off = ~np.eye(n, dtype=bool)
    ref = np.stack([np.where(off, _adjacency(r, kind, p, np.longdouble), np.longdouble(0))
                    .sum(axis=1) for p in DEFAULT])
    k = engine.soft_connectivity(_input("expression", n, s), kind=kind, powers=DEFAULT,
                                 method="bicor")
    assert k.dtype == np.float64 and k.shape == (len(DEFAULT), n)
    p = np.asarray(DEFAULT)[:, None]
    bound = 2.0 ** -53 * (n * (2.0 * p * (s + 20) + 4.0) + n * np.abs(ref.astype(np.float64)))
    worst = float((np.abs(k.astype(np.longdouble) - ref).astype(np.float64) / bound).max())
    print(f"n={n} s={s} {kind}: max |k - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst


# ---- 6. the zero-MAD fallback -----------------------------------------------------------------
def _zero_mad_matrix():
    E = _expression(130, 7, seed=21)
    E[3] = [1, 1, 1, 1, 2, 5, 1]
    E[40] = np.array([7, 2, 2, 2, -3, 2, 2]) * 1e-3 + 4.0
    return E


def _raw_set_layer(engine, E, kind, power, method, fallback=None):
    """n2v2r_set_layer_corr_method itself, past the checks Coexpression makes on the host."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    n, s = E.shape
    engine._check(engine.lib.n2v2r_set_num_layers(engine.h, 1, n), "set_num_layers")
    engine.n, engine.num_layers = n, 1
    fb = None if fallback is None else fallback.ctypes.data_as(ctypes.c_void_p)
    engine._check(engine.lib.n2v2r_set_layer_corr_method(
        engine.h, 0, n, s, E, int(kind), ctypes.c_double(power), int(method), fb), "layer 0")


def test_zero_mad_rows_take_the_pearson_row(engine):
    from node2vec2rank_amd import Coexpression, pick_soft_threshold
    E = _zero_mad_matrix()
    Z, bad = engine.corr_standardise(E, "bicor", return_bad_row=True)
    assert bad == -1
    P = engine.corr_standardise(E, "pearson")
    assert np.array_equal(Z[[3, 40]], P[[3, 40]])
    assert not np.array_equal(Z[4], P[4])
    worst = _z_ratio(Z, E)
    print(f"max |Z - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst

    message = r"2 rows have zero MAD \(first: row 3\); Pearson standardisation used for them"
    with pytest.warns(RuntimeWarning, match="layer 0: " + message):
        engine.set_layers([Coexpression(E, method="bicor")])
    _check_layer(engine.layer_dense(0), _layer_reference(_bicor(E), "unsigned", 1.0))
    with pytest.warns(RuntimeWarning, match=message):
        res = pick_soft_threshold(E, engine=engine, method="bicor")
    assert res.method == "bicor" and np.isfinite(res.connectivity).all()

    for method, want in ((2, [2, 3]), (1, [0, -1]), (0, [0, -1])):
        fb = np.array([-7, -7], dtype=np.int64)
        _raw_set_layer(engine, E, 0, 1.0, method, fb)
        assert fb.tolist() == want, method
        fb[:] = -7
        pw = np.array([1.0, 6.0])
        out = np.empty((2, 130))
        engine._check(engine.lib.n2v2r_soft_connectivity_method(
            engine.h, 130, 7, E, 0, pw, 2, method, out, fb.ctypes.data_as(ctypes.c_void_p)),
            "soft_connectivity")
        assert fb.tolist() == want, method
    _raw_set_layer(engine, E, 0, 1.0, 2, None)  # the counts are optional


# ---- 7. errors --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["pearson", "spearman", "bicor"])
def test_errors_leave_the_handle_usable(engine, method):
    from node2vec2rank_amd import Coexpression
    n, s = 130, 10
    good = _expression(n, s, seed=3)
    s_good = None

    def fits():
        nonlocal s_good
        engine.set_layers([Coexpression(good, method=method)])
        engine.uase(4, seed=2)
        sv = engine.singular_values()
        assert np.isfinite(sv).all() and sv[0] > 0
        if s_good is None:
            s_good = sv
        np.testing.assert_allclose(sv, s_good, rtol=1e-5)

    fits()
    const = good.copy()
    const[70] = 0.1
    nan = good.copy()
    nan[129, 4] = np.nan
    nan[128, 0] = np.nan
    pinf = good.copy()
    pinf[97, 0] = np.inf
    both = const.copy()
    both[97, 0] = np.inf
    both[5, 9] = -np.inf
    for E, row in ((const, 70), (nan, 128), (pinf, 97), (both, 5)):
        with pytest.raises(ValueError, match=rf"\brow {row}\b"):
            engine.set_layers([Coexpression(E, method=method)])
        with pytest.raises(ValueError):  # the layer is not loaded
            engine.layer_dense(0)
        with pytest.raises(ValueError, match=rf"\brow {row} "):
            engine.soft_connectivity(E, powers=[1.0, 6.0], method=method)
        Z, bad = engine.corr_standardise(E, method, return_bad_row=True)
        assert bad == row and not Z[row].any()  # no error here: the row is zeros
        fits()
    for code in (3, -1, 17):
        with pytest.raises(ValueError, match="method"):
            _raw_set_layer(engine, good, 0, 1.0, code)
        with pytest.raises(ValueError):
            engine.uase(4, seed=2)  # nothing loaded: refused, not a fit of stale data
        out = np.empty((1, n))
        with pytest.raises(ValueError, match="method"):
            engine._check(engine.lib.n2v2r_soft_connectivity_method(
                engine.h, n, s, good, 0, np.array([2.0]), 1, code, out, None), "soft")
        fits()
    with pytest.raises(ValueError, match="method"):
        engine.soft_connectivity(good, method="kendall")


# ---- 8. partitioned handles -------------------------------------------------------------------
def _method_layers(E):
    from node2vec2rank_amd import Coexpression
    return [Coexpression(E, method="spearman"),
            Coexpression(E, kind="signed", power=6.0, method="bicor")]


@pytest.fixture(scope="module")
def single_193(engine):
    E = _input("expression", 193, 37)
    engine.set_layers(_method_layers(E))
    return E, [engine.layer_dense(k) for k in range(2)]


def test_partitioned_rows_are_the_single_gpu_bits(single_193):
    from test_gpu_dist import _run_ranks
    E, whole = single_193

    def fn(eng, r):
        eng.set_layers(_method_layers(E))
        return eng.dist_info(), [eng.layer_dense(k) for k in range(2)]

    res = _run_ranks(2, fn)
    for k in range(2):
        got = np.zeros_like(whole[k])
        covered = 0
        for (_, _, row0, nl), layers in res:
            band = layers[k]
            assert not band[:row0].any() and not band[row0 + nl:].any()
            got[row0:row0 + nl] = band[row0:row0 + nl]
            covered += nl
        assert covered == 193
        np.testing.assert_array_equal(got, whole[k])


def test_multi_handle_rows_are_the_single_gpu_bits(single_193):
    from node2vec2rank_amd import _lib
    E, whole = single_193
    eng = _lib.Engine.multi([0, 0, 0])
    try:
        eng.set_layers(_method_layers(E))
        for k in range(2):
            np.testing.assert_array_equal(eng.layer_dense(k), whole[k])
        with pytest.warns(RuntimeWarning, match=r"layer 0: 2 rows have zero MAD \(first: row 3\)"):
            from node2vec2rank_amd import Coexpression
            eng.set_layers([Coexpression(_zero_mad_matrix(), method="bicor")])
    finally:
        eng.close()


# ---- 9. end to end ----------------------------------------------------------------------------
def test_fit_of_bicor_layers_matches_the_oracle(engine):
    from node2vec2rank_amd import Coexpression
    from node2vec2rank_amd.model import N2V2R
    n, K, s, d = 600, 2, 40, 8
    Es = [_expression(n, s, seed=70 + k) for k in range(K)]
    coex = [Coexpression(E, method="bicor") for E in Es]
    refs = [_layer_reference(_bicor(E), "unsigned", 1.0) for E in Es]
    _, s_ref, _ = orc.uase([sp.csr_matrix(a) for a in refs], d, seed=11)
    engine.set_layers(coex)
    engine.uase(d, seed=11)
    np.testing.assert_allclose(engine.singular_values(), s_ref, rtol=1e-5)

    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[4, 8], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=11, verbose=-1, save_dir=None)
    model = N2V2R(graphs=coex, nodes=nodes, config=dict(config))
    out = model.fit_transform_rank()
    agg = model.aggregate_transform()
    assert list(out) == ["1"]
    assert list(out["1"].index) == nodes
    assert out["1"].shape == (n, 4) and np.isfinite(out["1"].to_numpy()).all()
    assert list(agg["1"].columns) == ["borda_ranks"] and list(agg["1"].index) == nodes
    assert np.isfinite(agg["1"].to_numpy()).all()
