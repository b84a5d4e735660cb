"""Topological-overlap layers built on the GPU (n2v2r_tom_layer, csrc/tom.hip) against numpy.

The reference is ``tom()`` below (WGCNA's TOMsimilarity with TOMDenom = "min", in fp64) on the
adjacency read back from the same handle BEFORE the call, so both sides start from the same fp32
values.

Tolerance: the layer is ONE fp32 rounding of an fp64 value that differs from the reference's by a
reordered sum of n products, at most about (n + 4) 2^-53 <= 3e-14 at n = 257, so every entry must
satisfy |T - ref| <= 2^-24 |ref| + 1e-12 (the bound of test_gpu_coexpression.py; the worst ratio
observed on an MI355X is 0.9973 over the 16 cases of test_layer_matches_numpy and 0.9995 at
n = 600)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import n2v2r_oracle as orc
from test_gpu_coexpression import _expression

pytestmark = pytest.mark.gpu

# one exact tile; ragged tiles; k not a multiple of the tile
SHAPES = [(64, 3), (193, 7), (130, 37), (257, 200)]
# (kind, power, tom): |r|; ((1 + r) / 2)^6; max(r, 0) (half the layer zero); r itself (negative)
LAYERS = [("unsigned", 1.0, "unsigned"), ("signed", 6.0, "unsigned"),
          ("signed hybrid", 1.0, "unsigned"), ("raw", 1.0, "signed")]


def tom(A, kind):
    A = A.astype(np.float64).copy()
    np.fill_diagonal(A, 0.0)
    L = A @ A
    absA = np.abs(A) if kind == "signed" else A
    k = absA.sum(axis=1)
    num = L + A
    if kind == "signed":
        num = np.abs(num)
    den = np.minimum.outer(k, k) + 1.0 - absA
    T = num / den
    np.fill_diagonal(T, 1.0)
    return T


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


_E = {}


def _expr(n, s):
    if (n, s) not in _E:
        _E[(n, s)] = _expression(n, s, seed=1000 * n + s)
    return _E[(n, s)]


def _check_tom(T, ref):
    assert T.dtype == np.float32 and T.shape == ref.shape
    err = np.abs(T.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12
    worst = float((err / bound).max())
    print(f"max |T - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst
    assert _same_bits(T, T.T)
    assert np.all(np.diag(T) == np.float32(1.0))


def _differs(T, A):
    off = ~np.eye(A.shape[0], dtype=bool)
    return float(np.mean(np.abs(T.astype(np.float64) - A)[off] > 1e-3))


@pytest.mark.parametrize("kind, power, tk", LAYERS)
@pytest.mark.parametrize("n, s", SHAPES)
def test_layer_matches_numpy(engine, n, s, kind, power, tk):
    from node2vec2rank_amd import Coexpression
    engine.set_layers([Coexpression(_expr(n, s), kind=kind, power=power)])
    A0 = engine.layer_dense(0)
    ref = tom(A0, tk)
    engine.tom_layer(0, kind=tk)
    T = engine.layer_dense(0)
    _check_tom(T, ref)
    share = _differs(T, A0)
    print(f"off-diagonal entries that moved by more than 1e-3: {share:.3f}")
    assert share > 0.5, share  # (not a no-op)
    # ... and the same bits through the Coexpression option
    engine.set_layers([Coexpression(_expr(n, s), kind=kind, power=power, tom=tk)])
    assert _same_bits(engine.layer_dense(0), T)


def test_plain_dense_layer_and_its_diagonal_is_ignored(engine):
    """A symmetric array in [0, 1] through the dense ingest, with a zero and with a unit
    diagonal: the same overlap, because the stored diagonal is never read as a value."""
    n = 130
    rng = np.random.default_rng(5)
    U = np.triu(rng.uniform(0.0, 1.0, size=(n, n)), 1)
    zero = (U + U.T).astype(np.float32)
    unit = zero.copy()
    np.fill_diagonal(unit, 1.0)
    ref = tom(zero, "unsigned")
    got = []
    for A in (zero, unit):
        engine.set_layers([A], storage="dense")
        assert _same_bits(engine.layer_dense(0), A)
        engine.tom_layer(0)
        got.append(engine.layer_dense(0))
        _check_tom(got[-1], ref)
    assert _same_bits(got[0], got[1])
    # the signed overlap of a non-negative layer is the unsigned one
    engine.set_layers([unit], storage="dense")
    engine.tom_layer(0, kind="signed")
    assert _same_bits(engine.layer_dense(0), got[0])


def test_tom_comes_before_the_other_options(engine):
    """WGCNA's order (adjacency, overlap), then the reference's network_transform."""
    from node2vec2rank_amd import Coexpression
    from test_gpu_layer_transform import _oracle
    E = _expr(193, 7)
    engine.set_layers([Coexpression(E, tom="unsigned")])
    T = engine.layer_dense(0)
    engine.set_layers([Coexpression(E, tom="unsigned", top_percent_keep=37.5, binarize=True)])
    got = engine.layer_dense(0)
    assert _same_bits(got, _oracle(T, top_percent_keep=37.5, binarize=True))
    assert 0.3 < np.count_nonzero(got) / got.size < 0.45


def _two_layers(E):
    from node2vec2rank_amd import Coexpression
    return [Coexpression(E, tom="unsigned"), Coexpression(E, kind="raw", tom="signed")]


@pytest.fixture(scope="module")
def single_193(engine):
    from node2vec2rank_amd import Coexpression
    E = _expr(193, 37)
    engine.set_layers([Coexpression(E), Coexpression(E, kind="raw")])
    A0 = [engine.layer_dense(k) for k in range(2)]
    engine.set_layers(_two_layers(E))
    whole = [engine.layer_dense(k) for k in range(2)]
    for k, tk in enumerate(("unsigned", "signed")):
        _check_tom(whole[k], tom(A0[k], tk))
    return E, whole


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rows_are_the_single_gpu_bits(single_193, world):
    """Bands that are not tile-aligned (row0 = 97; 65, 130) and, at three ranks, a last band
    shorter than the others (63 rows of 65): every rank's rows carry the one-GPU bits and
    nothing outside its band shows in its read-back."""
    from test_gpu_dist import _run_ranks
    E, whole = single_193

    def fn(eng, r):
        eng.set_layers(_two_layers(E))
        return eng.dist_info(), [eng.layer_dense(k) for k in range(2)]

    res = _run_ranks(world, fn)
    for k in range(2):
        got = np.full_like(whole[k], np.nan)
        covered = 0
        for (_, _, row0, nl), layers in res:
            band = layers[k]
            assert not band[:row0].any() and not band[row0 + nl:].any()
            got[row0:row0 + nl] = band[row0:row0 + nl]
            covered += nl
        assert covered == 193
        assert _same_bits(got, whole[k])


def test_multi_handle_rows_are_the_single_gpu_bits(single_193):
    from node2vec2rank_amd import Coexpression, _lib
    E, whole = single_193
    eng = _lib.Engine.multi([0, 0, 0])
    try:
        eng.set_layers(_two_layers(E))
        for k in range(2):
            assert _same_bits(eng.layer_dense(k), whole[k])
        # every rank refuses alike, and the layer keeps its bits
        eng.set_layers([Coexpression(E, kind="raw")])
        raw = eng.layer_dense(0)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            eng.tom_layer(0, kind="unsigned")
        assert _same_bits(eng.layer_dense(0), raw)
        eng.tom_layer(0, kind="signed")
        assert _same_bits(eng.layer_dense(0), whole[1])
    finally:
        eng.close()


def test_errors_leave_the_layer_as_it_was(engine):
    """A refused call writes nothing: the old bits are still there, and a fit runs.  (The layer
    with a planted NaN keeps its bits too; the fit after it runs on the handle once a clean layer
    replaces it, as no fit of a NaN layer is meaningful.)"""
    from node2vec2rank_amd import Coexpression, _lib
    E = _expr(193, 7)

    def fit():
        engine.uase(4, seed=2)
        sv = engine.singular_values()
        assert np.isfinite(sv).all() and sv[0] > 0
        return sv

    engine.set_layers([Coexpression(E)])
    A0 = engine.layer_dense(0)
    s0 = fit()

    # a directed dense layer
    D = np.random.default_rng(11).uniform(0.0, 1.0, size=(193, 193)).astype(np.float32)
    engine.set_layers([D], storage="dense")
    s_d = fit()
    with pytest.raises(ValueError, match="directed"):
        engine.tom_layer(0)
    assert _same_bits(engine.layer_dense(0), D)
    np.testing.assert_allclose(fit(), s_d, rtol=1e-5)

    # CSR storage
    engine.set_layers([sp.csr_matrix(A0)], storage="csr")
    s_csr = fit()
    with pytest.raises(ValueError, match="CSR"):
        engine.tom_layer(0)
    np.testing.assert_allclose(fit(), s_csr, rtol=1e-5)

    # a layer that is not loaded; an unknown type (through the C call and through the wrapper)
    engine.set_layers([A0], storage="dense")
    with pytest.raises(ValueError, match="not loaded"):
        engine.tom_layer(1)
    assert engine.lib.n2v2r_tom_layer(engine.h, 0, 2) == _lib.ERR_BAD_ARG
    assert "type" in engine._err()
    assert engine.lib.n2v2r_tom_layer(engine.h, 0, -1) == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="kind"):
        engine.tom_layer(0, kind="mean")
    assert _same_bits(engine.layer_dense(0), A0)
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)

    # the unsigned overlap of a raw layer with negative entries: the message names the range
    # (37 samples: r itself has the rank of its samples, and the fit asks for 4 dimensions)
    E = _expr(193, 37)
    engine.set_layers([Coexpression(E, kind="raw")])
    raw = engine.layer_dense(0)
    assert (raw < 0).any()
    s_raw = fit()
    with pytest.raises(ValueError, match=r"\[0, 1\]") as info:
        engine.set_layers([Coexpression(E, kind="raw", tom="unsigned")])
    assert f"{np.count_nonzero(raw < 0)} entries" in str(info.value)
    assert _same_bits(engine.layer_dense(0), raw)
    np.testing.assert_allclose(fit(), s_raw, rtol=1e-5)

    # a planted NaN (symmetric = yes: a NaN never equals its mirror)
    nan = A0.copy()
    nan[129, 4] = nan[4, 129] = np.nan
    engine.set_layers([nan], symmetric=_lib.SYM_YES, storage="dense")
    with pytest.raises(ValueError, match="2 NaN"):
        engine.tom_layer(0)
    assert _same_bits(engine.layer_dense(0), nan)
    engine.set_layers([A0], storage="dense")
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)

    # a planted 1.5, and (signed) a planted -1.5
    for bad, kind, rng in ((1.5, "unsigned", r"\[0, 1\]"), (1.5, "signed", r"\[-1, 1\]"),
                           (-1.5, "signed", r"\[-1, 1\]")):
        big = A0.copy()
        big[7, 150] = big[150, 7] = bad
        engine.set_layers([big], storage="dense")
        s_big = fit()
        with pytest.raises(ValueError, match="2 entries outside the range " + rng):
            engine.tom_layer(0, kind=kind)
        assert _same_bits(engine.layer_dense(0), big)
        np.testing.assert_allclose(fit(), s_big, rtol=1e-5)

    # the call can be repeated with a good layer; a success clears the embedding
    engine.set_layers([A0], storage="dense")
    fit()
    engine.embedding()
    engine.tom_layer(0)
    with pytest.raises(ValueError):
        engine.embedding()
    _check_tom(engine.layer_dense(0), tom(A0, "unsigned"))
    fit()
    # ... and once more on the result (the scratch buffer and the layer change places again)
    T1 = engine.layer_dense(0)
    engine.tom_layer(0)
    _check_tom(engine.layer_dense(0), tom(T1, "unsigned"))


def test_fit_from_tom_layers(engine):
    """n = 600, K = 3, samples = 40, d = 8: the fit from Coexpression(tom="unsigned") layers
    against the oracle's on the numpy overlaps at rtol 1e-5 on the singular values (the suite's
    bar for two fp32 fits of one matrix), and the ranking frames of the model."""
    from node2vec2rank_amd import Coexpression
    from node2vec2rank_amd.model import N2V2R
    n, K, s, d = 600, 3, 40, 8
    Es = [_expression(n, s, seed=50 + k) for k in range(K)]
    engine.set_layers([Coexpression(E) for E in Es])
    refs = [tom(engine.layer_dense(k), "unsigned") for k in range(K)]
    _, s_ref, _ = orc.uase([sp.csr_matrix(a.astype(np.float32)) for a in refs], d, seed=11)

    coex = [Coexpression(E, tom="unsigned") for E in Es]
    engine.set_layers(coex)
    arrays = [engine.layer_dense(k) for k in range(K)]
    for k in range(K):
        _check_tom(arrays[k], refs[k])
    engine.uase(d, seed=11)
    np.testing.assert_allclose(engine.singular_values(), s_ref, rtol=1e-5)

    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[4, 8], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=11, verbose=-1, save_dir=None)
    frames = []
    for graphs in (coex, [a.astype(np.float32) for a in refs]):
        model = N2V2R(graphs=graphs, nodes=nodes, config=dict(config))
        out = model.fit_transform_rank()
        frames.append((out, model.aggregate_transform(), model.degree_difference_ranking()))
    (out_c, agg_c, dedi_c), (out_a, agg_a, dedi_a) = frames
    assert list(out_c) == list(out_a) == ["1", "2"]
    for key in out_c:
        assert list(out_c[key].columns) == list(out_a[key].columns)
        assert out_c[key].index.equals(out_a[key].index) and list(out_c[key].index) == nodes
        assert out_c[key].shape == (n, 4) and np.isfinite(out_c[key].to_numpy()).all()
        assert list(agg_c[key].columns) == list(agg_a[key].columns) == ["borda_ranks"]
        assert agg_c[key].index.equals(agg_a[key].index)
        assert list(dedi_c[key].columns) == list(dedi_a[key].columns) == ["DeDi", "absDeDi"]
