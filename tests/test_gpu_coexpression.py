"""Co-expression layers built on the GPU from expression matrices (n2v2r_set_layer_corr,
csrc/corr.hip) against numpy: ``r = np.corrcoef(E)``, the kind's transform and the power in fp64,
the diagonal set to 1.

Tolerance: the layer is ONE fp32 rounding of an fp64 value that differs from the reference's by
about (samples + 10) 2^-53 power (two fp64 evaluations of the same sums in different orders), so
every entry must satisfy |A - ref| <= 2^-24 |ref| + 1e-12."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import n2v2r_oracle as orc

pytestmark = pytest.mark.gpu

KINDS = ["unsigned", "signed", "signed hybrid", "raw"]
# one exact tile; ragged tiles; samples below, above and not a multiple of the 16-wide k chunk
SHAPES = [(64, 3), (193, 7), (130, 37), (257, 200)]
# every kind at power 1 and 6 (a raw layer may be negative: the entry point refuses a power for
# it, checked in test_errors_leave_the_handle_usable)
KIND_POWER = [(k, p) for k in KINDS for p in (1.0, 6.0) if not (k == "raw" and p != 1.0)]


def _expression(n, s, seed):
    """Rows on very different scales and offsets (standardisation must remove both)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    offset = rng.uniform(-5, 5, size=(n, 1)) * scale
    return rng.standard_normal((n, s)) * scale + offset


def _reference(E, kind, power):
    r = np.corrcoef(E)
    t = {"unsigned": np.abs(r), "signed": (1.0 + r) / 2.0, "signed hybrid": np.maximum(r, 0.0),
         "raw": r}[kind]
    if power != 1.0:
        t = t ** power
    np.fill_diagonal(t, 1.0)
    return t


_REF = {}


def _case(n, s):
    """The expression matrix of a shape and its fp64 references, computed once."""
    if (n, s) not in _REF:
        E = _expression(n, s, seed=1000 * n + s)
        _REF[(n, s)] = (E, {kp: _reference(E, *kp) for kp in KIND_POWER})
    return _REF[(n, s)]


def _check_layer(A, ref):
    err = np.abs(A.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12
    worst = float((err / bound).max())
    print(f"max |A - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst
    assert np.array_equal(A, A.T)  # bitwise
    assert np.all(np.diag(A) == np.float32(1.0))


@pytest.mark.parametrize("kind, power", KIND_POWER)
@pytest.mark.parametrize("n, s", SHAPES)
def test_layer_matches_numpy(engine, n, s, kind, power):
    from node2vec2rank_amd import Coexpression
    E, refs = _case(n, s)
    engine.set_layers([Coexpression(E, kind=kind, power=power)])
    assert engine.storage == "dense"
    _check_layer(engine.layer_dense(0), refs[(kind, power)])


def test_upload_is_the_expression_matrix(engine):
    from node2vec2rank_amd import Coexpression
    E, _ = _case(130, 37)
    before = engine.h2d_layer_bytes()[0]
    engine.set_layers([Coexpression(E), Coexpression(E, kind="signed")])
    assert engine.h2d_layer_bytes()[0] - before == 2 * 8 * 130 * 37


def _two_layers(E):
    from node2vec2rank_amd import Coexpression
    return [Coexpression(E), Coexpression(E, kind="signed", power=6.0)]


@pytest.fixture(scope="module")
def single_193(engine):
    E, _ = _case(193, 37)
    engine.set_layers(_two_layers(E))
    return E, [engine.layer_dense(k) for k in range(2)]


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rows_are_the_single_gpu_bits(single_193, world):
    """Rank bands are not tile-aligned (row0 = 97; 65, 130): every rank's rows carry the bits the
    one-GPU layer has there, and nothing outside its band is written."""
    from test_gpu_dist import _run_ranks
    E, whole = single_193

    def fn(eng, r):
        eng.set_layers(_two_layers(E))
        return eng.dist_info(), [eng.layer_dense(k) for k in range(2)]

    res = _run_ranks(world, fn)
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
        eng.set_layers(_two_layers(E))
        for k in range(2):
            np.testing.assert_array_equal(eng.layer_dense(k), whole[k])
        assert eng.h2d_layer_bytes() == [2 * 8 * 193 * 37] * 3
    finally:
        eng.close()


def test_fit_matches_dense_ingest_of_the_same_layers(engine):
    """n = 600, K = 3, samples = 40, d = 8: the fit from Coexpression layers and the fit from the
    read-back arrays through the existing dense ingest both meet tests/test_gpu_dense.py's bar
    against the oracle on the numpy reference layers."""
    from node2vec2rank_amd import Coexpression
    from node2vec2rank_amd.model import N2V2R
    n, K, s, d = 600, 3, 40, 8
    Es = [_expression(n, s, seed=50 + k) for k in range(K)]
    coex = [Coexpression(E) for E in Es]
    refs = [_reference(E, "unsigned", 1.0) for E in Es]
    _, s_ref, _ = orc.uase([sp.csr_matrix(a) for a in refs], d, seed=11)

    engine.set_layers(coex)
    engine.uase(d, seed=11)
    np.testing.assert_allclose(engine.singular_values(), s_ref, rtol=1e-5)
    for k in range(K):
        np.testing.assert_allclose(engine.column_sums(k), refs[k].sum(axis=0), rtol=1e-5)
    arrays = [engine.layer_dense(k) for k in range(K)]

    engine.set_layers(arrays, storage="dense")
    for k in range(K):  # the round trip keeps the bits
        np.testing.assert_array_equal(engine.layer_dense(k), arrays[k])
    engine.uase(d, seed=11)
    np.testing.assert_allclose(engine.singular_values(), s_ref, rtol=1e-5)
    for k in range(K):
        np.testing.assert_allclose(engine.column_sums(k), refs[k].sum(axis=0), rtol=1e-5)

    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[4, 8], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=11, verbose=-1, save_dir=None)
    frames = []
    for graphs in (coex, arrays):
        model = N2V2R(graphs=graphs, nodes=nodes, config=dict(config))
        out = model.fit_transform_rank()
        agg = model.aggregate_transform()
        dedi = model.degree_difference_ranking()
        frames.append((out, agg, dedi))
    (out_c, agg_c, dedi_c), (out_a, agg_a, dedi_a) = frames
    assert list(out_c) == list(out_a) == ["1", "2"]
    for key in out_c:
        assert list(out_c[key].columns) == list(out_a[key].columns)
        assert out_c[key].index.equals(out_a[key].index)
        assert list(out_c[key].index) == nodes
        assert out_c[key].shape == (n, 4) and np.isfinite(out_c[key].to_numpy()).all()
        assert list(agg_c[key].columns) == list(agg_a[key].columns) == ["borda_ranks"]
        assert agg_c[key].index.equals(agg_a[key].index)
        # the same layer bits either way: the same fp32 column sums
        np.testing.assert_array_equal(dedi_c[key].to_numpy(), dedi_a[key].to_numpy())


def _raw_corr(engine, E, kind, power):
    """n2v2r_set_layer_corr itself, past the checks Coexpression makes on the host."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    n, s = E.shape
    engine._check(engine.lib.n2v2r_set_num_layers(engine.h, 1, n), "set_num_layers")
    engine.n, engine.num_layers = n, 1
    engine._check(engine.lib.n2v2r_set_layer_corr(engine.h, 0, n, s, E, int(kind),
                                                  ctypes.c_double(power)), "layer 0")


def test_errors_leave_the_handle_usable(engine):
    from node2vec2rank_amd import Coexpression
    n, s = 130, 10
    good = _expression(n, s, seed=3)
    s_good = None

    def fits():
        nonlocal s_good
        engine.set_layers([Coexpression(good)])
        engine.uase(4, seed=2)
        sv = engine.singular_values()
        assert np.isfinite(sv).all() and sv[0] > 0
        if s_good is None:
            s_good = sv
        np.testing.assert_allclose(sv, s_good, rtol=1e-5)

    fits()
    const = good.copy()
    const[70] = 0.1  # (three tenths do not sum to 0.3: the mean of this row is not 0.1)
    with pytest.raises(ValueError, match=r"\brow 70\b"):
        engine.set_layers([Coexpression(const)])
    with pytest.raises(ValueError):  # the layer is not loaded
        engine.layer_dense(0)
    fits()
    nan = good.copy()
    nan[129, 4] = np.nan
    with pytest.raises(ValueError, match=r"\brow 129\b"):
        engine.set_layers([Coexpression(nan)])
    fits()
    both = const.copy()
    both[97, 0] = np.inf
    both[5, 9] = -np.inf
    with pytest.raises(ValueError, match=r"\brow 5\b"):  # the smallest bad row
        engine.set_layers([Coexpression(both)])
    fits()
    for E, kind, power, what in [(good[:, :1], 0, 1.0, "samples"), (good, 4, 1.0, "kind"),
                                 (good, -1, 1.0, "kind"), (good, 0, 0.5, "power"),
                                 (good, 1, float("nan"), "power"), (good, 3, 2.0, "raw")]:
        with pytest.raises(ValueError, match=what):
            _raw_corr(engine, E, kind, power)
        with pytest.raises(ValueError):
            engine.uase(4, seed=2)  # nothing loaded: refused, not a fit of stale data
        # a corrected call on the same handle, without starting over
        engine._check(engine.lib.n2v2r_set_layer_corr(engine.h, 0, n, s, good, 0,
                                                      ctypes.c_double(1.0)), "layer 0")
        engine.uase(4, seed=2)
        np.testing.assert_allclose(engine.singular_values(), s_good, rtol=1e-5)


def test_no_overwrite_between_ingest_forms():
    """A Coexpression layer over a handle that held larger dense layers, and dense arrays over a
    handle that held Coexpression layers: the fits agree with a fresh handle's within the
    suite's bar for two fp32 fits of one matrix (rtol 1e-5 on the singular values)."""
    from node2vec2rank_amd import Coexpression, _lib
    big = _expression(300, 24, seed=8)
    small = _expression(130, 12, seed=9)
    d = 6

    def sv(eng, layers, **kw):
        eng.set_layers(layers, **kw)
        eng.uase(d, seed=5)
        return eng.singular_values()

    fresh = _lib.Engine(0)
    try:
        s_coex = sv(fresh, [Coexpression(small), Coexpression(small, kind="signed")])
        arrays = [fresh.layer_dense(k) for k in range(2)]
    finally:
        fresh.close()
    fresh = _lib.Engine(0)
    try:
        s_dense = sv(fresh, arrays, storage="dense")
    finally:
        fresh.close()
    used = _lib.Engine(0)
    try:
        big_ref = [np.abs(np.corrcoef(big)).astype(np.float32)] * 3
        sv(used, big_ref, storage="dense")
        got = sv(used, [Coexpression(small), Coexpression(small, kind="signed")])
        np.testing.assert_allclose(got, s_coex, rtol=1e-5)
        sv(used, [Coexpression(big)] * 3)
        got = sv(used, arrays, storage="dense")
        np.testing.assert_allclose(got, s_dense, rtol=1e-5)
    finally:
        used.close()
