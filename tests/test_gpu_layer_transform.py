"""``n2v2r_transform_layer`` (csrc/transform.hip): threshold, top-percent cut and binarize of a
dense layer in place on the GPU, against ``ingest.transform`` on the layer's own stored values.

The oracle of every case is ``ingest.transform(Layer(csr_matrix(A0), ...)).mat.toarray()`` with
``A0`` the untransformed layer read back from the same handle; every comparison is bitwise
(``np.array_equal``): the cut depends only on two order statistics of the stored fp32 values,
which an integer radix select finds exactly, so there is nothing to tolerate."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import n2v2r_oracle as orc
from test_gpu_coexpression import _expression

pytestmark = pytest.mark.gpu

SHAPES = [(64, 3), (193, 7), (257, 200)]
# |r|; ((1 + r) / 2)^6; max(r, 0) (half the layer is zero); r itself (negative keys)
KIND_POWER = [("unsigned", 1.0), ("signed", 6.0), ("signed hybrid", 1.0), ("raw", 1.0)]
THRESHOLDS = [None, 0.1]
TOPS = [100, 37.5, 5, 0.1]


def _oracle(A0, **kw):
    from node2vec2rank_amd import ingest
    labels = np.arange(A0.shape[0])
    out = ingest.transform(ingest.Layer(sp.csr_matrix(A0), labels, labels), **kw).mat.toarray()
    assert out.dtype == np.float32
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


_E = {}


def _expr(n, s):
    if (n, s) not in _E:
        _E[(n, s)] = _expression(n, s, seed=1000 * n + s)
    return _E[(n, s)]


@pytest.mark.parametrize("kind, power", KIND_POWER)
@pytest.mark.parametrize("n, s", SHAPES)
def test_coexpression_layer_matches_ingest_transform(engine, n, s, kind, power):
    """At (64, 3) the layer has about 2,000 distinct values in 4,096 entries: ties straddle the
    cut.  (257, 200): more than one workgroup's worth of float4s and a ragged last tile."""
    from node2vec2rank_amd import Coexpression
    layer = Coexpression(_expr(n, s), kind=kind, power=power)
    engine.set_layers([layer])
    A0 = engine.layer_dense(0)
    first = True
    for thr in THRESHOLDS:
        alive = A0.astype(np.float64).ravel()  # (the threshold compares in fp64, as the oracle)
        alive = alive[(alive != 0) & ~(alive < (-np.inf if thr is None else thr))]
        for top in TOPS:
            for binarize in (False, True):
                if not first:
                    engine.set_layers([layer])
                first = False
                ref = _oracle(A0, threshold=thr, top_percent_keep=top, binarize=binarize)
                st = engine.transform_layer(0, threshold=thr, top_percent_keep=top,
                                            binarize=binarize)
                A = engine.layer_dense(0)
                what = (thr, top, binarize, st)
                assert _same_bits(A, ref), what
                assert np.array_equal(A, ref), what
                assert st["nonzero"] == alive.size, what
                assert st["kept"] == np.count_nonzero(ref), what
                assert _same_bits(A, A.T), what
                assert st["cut"] == np.percentile(alive, 100 - top), what


def test_set_layers_applies_the_coexpression_options(engine):
    from node2vec2rank_amd import Coexpression
    E = _expr(193, 7)
    engine.set_layers([Coexpression(E), Coexpression(E, kind="signed", power=6.0)])
    A0 = [engine.layer_dense(k) for k in range(2)]
    engine.set_layers([Coexpression(E, threshold=0.1, top_percent_keep=37.5),
                       Coexpression(E, kind="signed", power=6.0, top_percent_keep=5,
                                    binarize=True)])
    assert engine.storage == "dense"
    assert _same_bits(engine.layer_dense(0), _oracle(A0[0], threshold=0.1, top_percent_keep=37.5))
    assert _same_bits(engine.layer_dense(1), _oracle(A0[1], top_percent_keep=5, binarize=True))


def test_directed_dense_layer_with_heavy_ties(engine):
    """Six distinct values over 16,900 entries: both order statistics are the same value
    (x == y).  The layer is not symmetric, so the A^T copy is transformed as well; it is read
    through the column sums, exact in fp32 for these small integers."""
    n = 130
    rng = np.random.default_rng(7)
    P = rng.integers(0, 6, size=(n, n)).astype(np.float32)
    S = P * rng.choice(np.float32([-1.0, 1.0]), size=(n, n))
    assert not np.array_equal(P, P.T)
    for A0, absolute in ((P, False), (S, True), (S, False)):
        for top in (40, 0):
            for binarize in (False, True):
                engine.set_layers([A0], storage="dense")
                assert _same_bits(engine.layer_dense(0), A0)
                ref = _oracle(A0, top_percent_keep=top, binarize=binarize, absolute=absolute)
                st = engine.transform_layer(0, top_percent_keep=top, binarize=binarize,
                                            absolute=absolute)
                what = (absolute, top, binarize, st)
                assert _same_bits(engine.layer_dense(0), ref), what
                assert st["kept"] == np.count_nonzero(ref), what
                assert st["nonzero"] == np.count_nonzero(A0), what
                assert np.array_equal(engine.column_sums(0),
                                      ref.sum(axis=0, dtype=np.float32)), what


def _directed_193():
    """Integers 0..5, not symmetric: the handle keeps an A^T copy (read through the column sums,
    exact in fp32 for these values)."""
    return np.random.default_rng(11).integers(0, 6, size=(193, 193)).astype(np.float32)


def _three_layers(E):
    from node2vec2rank_amd import Coexpression
    return [Coexpression(E), Coexpression(E, kind="signed", power=6.0), _directed_193()]


_THREE = [dict(threshold=0.1, top_percent_keep=37.5), dict(top_percent_keep=5, binarize=True),
          dict(top_percent_keep=40)]


@pytest.fixture(scope="module")
def single_193(engine):
    E = _expression(193, 37, seed=1000 * 193 + 37)
    engine.set_layers(_three_layers(E))
    A0 = [engine.layer_dense(k) for k in range(3)]
    stats = [engine.transform_layer(k, **_THREE[k]) for k in range(3)]
    whole = [engine.layer_dense(k) for k in range(3)]
    for k in range(3):
        assert _same_bits(whole[k], _oracle(A0[k], **_THREE[k]))
    sums = engine.column_sums(2)
    assert np.array_equal(sums, whole[2].sum(axis=0, dtype=np.float32))
    return E, whole, stats, sums


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rows_are_the_single_gpu_bits(single_193, world):
    """Bands that are not tile-aligned (row0 = 97; 65, 130): the cut is global, every rank's rows
    carry the one-GPU bits (the directed layer's A^T rows too) and every rank reports the same
    stats."""
    from test_gpu_dist import _run_ranks
    E, whole, stats, sums = single_193

    def fn(eng, r):
        eng.set_layers(_three_layers(E))
        st = [eng.transform_layer(k, **_THREE[k]) for k in range(3)]
        return eng.dist_info(), st, [eng.layer_dense(k) for k in range(3)], eng.column_sums(2)

    res = _run_ranks(world, fn)
    for k in range(3):
        got = np.full_like(whole[k], np.nan)
        for (_, _, row0, nl), st, layers, cs in res:
            assert st[k] == stats[k]
            assert np.array_equal(cs, sums)
            band = layers[k]
            assert not band[:row0].any() and not band[row0 + nl:].any()
            got[row0:row0 + nl] = band[row0:row0 + nl]
        assert _same_bits(got, whole[k])


def test_multi_handle_rows_are_the_single_gpu_bits(single_193):
    from node2vec2rank_amd import Coexpression, _lib
    E, whole, stats, sums = single_193
    eng = _lib.Engine.multi([0, 0, 0])
    try:
        eng.set_layers(_three_layers(E))
        for k in range(3):
            assert eng.transform_layer(k, **_THREE[k]) == stats[k]
            assert _same_bits(eng.layer_dense(k), whole[k])
        assert np.array_equal(eng.column_sums(2), sums)
        # ... and through the Coexpression options
        eng.set_layers([Coexpression(E, **_THREE[0]),
                        Coexpression(E, kind="signed", power=6.0, **_THREE[1])])
        for k in range(2):
            assert _same_bits(eng.layer_dense(k), whole[k])
        with pytest.raises(ValueError, match="no non-zero"):
            eng.transform_layer(0, threshold=2.0)
        assert _same_bits(eng.layer_dense(0), whole[0])
    finally:
        eng.close()


def test_errors_leave_the_layer_as_it_was(engine):
    """A refused call writes nothing: the old bits are still there, and a fit runs.  (The layer
    with a planted NaN keeps its bits too; the fit after it runs on the handle once a clean layer
    replaces it, as no fit of a NaN layer is meaningful.)"""
    from node2vec2rank_amd import Coexpression
    E = _expr(193, 7)

    def fit():
        engine.uase(4, seed=2)
        sv = engine.singular_values()
        assert np.isfinite(sv).all() and sv[0] > 0
        return sv

    engine.set_layers([Coexpression(E)])
    A0 = engine.layer_dense(0)
    s0 = fit()
    with pytest.raises(ValueError, match="no non-zero entry left"):
        engine.transform_layer(0, threshold=2.0)
    assert _same_bits(engine.layer_dense(0), A0)
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)
    for bad in (101, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="top_percent_keep"):
            engine.transform_layer(0, top_percent_keep=bad)
    with pytest.raises(ValueError, match="threshold"):
        engine.transform_layer(0, threshold=float("nan"))
    with pytest.raises(ValueError, match="not loaded"):
        engine.transform_layer(1)
    st = engine.lib.n2v2r_transform_layer(engine.h, 0, 8, 0.0, 50.0, None)
    assert st == 1 and "flag" in engine._err()  # N2V2R_ERR_BAD_ARG
    assert _same_bits(engine.layer_dense(0), A0)
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)
    # the call can be repeated with good arguments (and with no stats asked for)
    assert engine.lib.n2v2r_transform_layer(engine.h, 0, 0, 0.0, 50.0, None) == 0
    assert _same_bits(engine.layer_dense(0), _oracle(A0, top_percent_keep=50))
    with pytest.raises(ValueError):  # the transform cleared the embedding
        engine.embedding()

    nan = A0.copy()
    nan[129, 4] = np.nan
    engine.set_layers([nan], storage="dense")
    with pytest.raises(ValueError, match="NaN"):
        engine.transform_layer(0, top_percent_keep=50)
    assert _same_bits(engine.layer_dense(0), nan)
    engine.set_layers([A0], storage="dense")
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)

    engine.set_layers([sp.csr_matrix(A0)], storage="csr")
    s_csr = fit()
    with pytest.raises(ValueError, match=r"ingest\.transform"):
        engine.transform_layer(0, top_percent_keep=50)
    np.testing.assert_allclose(fit(), s_csr, rtol=1e-5)


def test_fit_from_transformed_coexpression_layers(engine):
    """n = 600, K = 3, samples = 40, d = 8, top 20 percent kept: the fit from the Coexpression
    layers, the fit from their read-back arrays through the dense ingest and the oracle's on the
    oracle-transformed layers agree at rtol 1e-5 on the singular values (the suite's bar for two
    fp32 fits of one matrix, test_gpu_coexpression.test_no_overwrite_between_ingest_forms)."""
    from node2vec2rank_amd import Coexpression
    from node2vec2rank_amd.model import N2V2R
    n, K, s, d = 600, 3, 40, 8
    Es = [_expression(n, s, seed=50 + k) for k in range(K)]
    engine.set_layers([Coexpression(E) for E in Es])
    refs = [_oracle(engine.layer_dense(k), top_percent_keep=20) for k in range(K)]
    _, s_ref, _ = orc.uase([sp.csr_matrix(a) for a in refs], d, seed=11)

    coex = [Coexpression(E, top_percent_keep=20) for E in Es]
    engine.set_layers(coex)
    engine.uase(d, seed=11)
    s_coex = engine.singular_values()
    arrays = [engine.layer_dense(k) for k in range(K)]
    for k in range(K):
        assert _same_bits(arrays[k], refs[k])
    engine.set_layers(arrays, storage="dense")
    engine.uase(d, seed=11)
    np.testing.assert_allclose(s_coex, engine.singular_values(), rtol=1e-5)
    np.testing.assert_allclose(s_coex, s_ref, rtol=1e-5)

    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[4, 8], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=11, verbose=-1, save_dir=None)
    frames = []
    for graphs in (coex, arrays):
        model = N2V2R(graphs=graphs, nodes=nodes, config=dict(config))
        out = model.fit_transform_rank()
        agg = model.aggregate_transform()
        frames.append((out, agg, model.degree_difference_ranking()))
    (out_c, agg_c, dedi_c), (out_a, agg_a, dedi_a) = frames
    # The array run's DeDi, bitwise: from the arrays in DENSE storage, the storage the
    # Coexpression layers have.  (N2V2R itself stores arrays that are at most 1/4 non-zero, as
    # these are at 20 percent, as CSR, whose fp32 column sums add in another order.)
    engine.set_layers(arrays, storage="dense")
    sums = [engine.column_sums(k) for k in range(K)]
    assert list(out_c) == list(out_a) == ["1", "2"]
    for i, key in enumerate(out_c, start=1):
        assert out_c[key].shape == (n, 4) and np.isfinite(out_c[key].to_numpy()).all()
        assert list(out_c[key].columns) == list(out_a[key].columns)
        assert list(agg_c[key].columns) == list(agg_a[key].columns) == ["borda_ranks"]
        assert agg_c[key].index.equals(agg_a[key].index)
        assert list(dedi_c[key].columns) == list(dedi_a[key].columns) == ["DeDi", "absDeDi"]
        dedi = sums[i - 1] - sums[i]
        np.testing.assert_array_equal(dedi_c[key].to_numpy(), np.stack([dedi, np.abs(dedi)], 1))
        # ... and the CSR-stored array run agrees within the fp32 summation bound of both runs,
        # |fl(sum) - sum| <= n u sum for n non-negative terms, u = 2^-24
        bound = 2 * n * 2.0 ** -24 * (sums[i - 1] + sums[i]).astype(np.float64)
        err = np.abs(dedi_a[key]["DeDi"].to_numpy(dtype=np.float64) - dedi)
        assert (err <= bound).all(), float((err / bound).max())
