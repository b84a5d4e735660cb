"""Both forms of the distance kernel (``distances_kernel`` and the float4
``distances_seq_kernel`` of ``csrc/rank.hip``) against the fp64 oracle, on embeddings given to
the engine and on the layout a fit leaves behind (one GPU and row-partitioned).

``n2v2r_launch_distances`` takes the float4 sequential form when

    strategy == 0 && !corr && layer_i >= 1 && ldy % 4 == 0 &&
    ldy >= ((plan.dmax + 15) / 16) * 16 && Y 16-byte aligned

and the general form otherwise.  ``set_embedding`` stores rows ``ldy = d`` floats apart, so the
cases below pick d, the dims and the metrics to land on each side of every clause of that rule;
``_float4_form`` restates it and every case asserts the side it means to test.

The embedding is K = 5 layers of n = 700 rows (three workgroups of 256, the last one partial),
standard normal / 4 in float32, with four degenerate rows: row 3 zero in every layer (cosine and
correlation 0 / 0), row 5 zero in layer 2 only, row 9 the constant 0.5 everywhere (zero centred
norm: correlation 0 / 0, cosine of parallel vectors), row 11 identical across layers (distance
0).  The tolerance is the suite's own for distances from a given embedding (``rtol = 0``,
``atol = 1e-9``, NaN where the oracle has NaN); both sides work in fp64 on the same float32
values, so they differ by summation order only (~1e-15 at these sizes).  The Borda scores of the
GPU's own distances must equal the stable oracle's exactly."""
import functools

import numpy as np
import pytest

from oracle import n2v2r_oracle as orc

pytestmark = pytest.mark.gpu

K, N = 5, 700
DIMS = [1, 2, 15, 16, 17, 33, 64, 100, 128]
STRATEGIES = ["sequential", "one_vs_before", "one_vs_rest"]
ALL_METRICS = ["cosine", "euclidean", "correlation"]
COS_EUC = ["cosine", "euclidean"]


@functools.lru_cache(maxsize=None)
def _embedding(d):
    rng = np.random.default_rng(400 + d)
    Y = (rng.standard_normal((K, N, d)) / 4).astype(np.float32)
    Y[:, 3, :] = 0.0
    Y[2, 5, :] = 0.0
    Y[:, 9, :] = 0.5
    Y[:, 11, :] = Y[0, 11, :]
    Y.setflags(write=False)
    return Y


def _float4_form(strategy, metrics, ldy, dims):
    """The launcher's rule (device allocations are 16-byte aligned; layer_i >= 1 always holds
    for the sequential strategy)."""
    dmax = max(dims)
    return (strategy == "sequential" and "correlation" not in metrics and ldy % 4 == 0 and
            ldy >= (dmax + 15) // 16 * 16)


def _rank_vs_oracle(eng, Y, dims, metrics, strategy):
    """Rank on the engine's current embedding, compare every comparison's distance table with
    the oracle on Y (the same values in fp64) and its Borda with the oracle's on the GPU's own
    distances.  Returns the GPU tables and the column names."""
    ncmp, ncols = eng.rank(strategy, dims, metrics)
    ref = orc.rank_distances(np.asarray(Y, dtype=np.float64), dims, metrics, strategy)
    assert ncmp == len(ref) == (Y.shape[0] if strategy == "one_vs_rest" else Y.shape[0] - 1)
    tables, names = [], None
    worst = 0.0
    for c, (key, (cols, Dref)) in enumerate(ref.items()):
        D = eng.distances(c)
        assert D.shape == Dref.shape == (Y.shape[1], ncols)
        with np.errstate(invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.abs(D - Dref))))
        np.testing.assert_allclose(D, Dref, rtol=0, atol=1e-9, equal_nan=True,
                                   err_msg=f"{strategy} comparison {key}")
        np.testing.assert_array_equal(eng.borda(c), orc.borda(D, faithful=False))
        tables.append(np.array(D))
        names = cols
    print(f"{strategy}, {len(dims)} dims up to {max(dims)}, {list(metrics)}: "
          f"max |D - oracle| = {worst:.2e}")
    return tables, names


def _fit(dims, d):
    return [x for x in dims if x <= d]


# ------------------------------------------------------------------- a. general kernel
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("d", [128, 63])
def test_general_kernel_vs_oracle(engine, d, strategy):
    """All three metrics: a correlation column sends every strategy to ``distances_kernel``
    (``!corr`` fails).  At d = 63, ``ldy % 4 != 0`` fails as well."""
    Y = _embedding(d)
    dims = DIMS if d == 128 else _fit(DIMS, 63) + [63]
    assert not _float4_form(strategy, ALL_METRICS, d, dims)
    engine.set_embedding(Y)
    tables, names = _rank_vs_oracle(engine, Y, dims, ALL_METRICS, strategy)
    # the degenerate rows do what they are there for
    D = tables[-1]
    cos = [i for i, c in enumerate(names) if c.endswith("cosine")]
    cor = [i for i, c in enumerate(names) if c.endswith("correlation")]
    euc = [i for i, c in enumerate(names) if c.endswith("euclidean")]
    assert np.isnan(D[3, cos]).all() and np.isnan(D[3, cor]).all() and (D[3, euc] == 0).all()
    assert np.isnan(D[9, cor]).all() and (D[11, euc] == 0).all()
    assert np.isfinite(np.delete(D, [3, 5, 9], axis=0)[:, cos + euc]).all()


def test_general_kernel_sequential_without_correlation_unaligned_rows(engine):
    """d = 63, cosine and euclidean, sequential: only ``ldy % 4 == 0`` keeps the float4 form
    away (rows 252 B apart are not 16-byte aligned)."""
    Y = _embedding(63)
    dims = _fit(DIMS, 63) + [63]
    assert not _float4_form("sequential", COS_EUC, 63, dims)
    assert _float4_form("sequential", COS_EUC, 64, dims)
    engine.set_embedding(Y)
    _rank_vs_oracle(engine, Y, dims, COS_EUC, "sequential")


# ------------------------------------------------------------------- b. sequential float4 kernel
@pytest.mark.parametrize("d", [16, 48, 64, 128])
def test_float4_kernel_vs_oracle(engine, d):
    """``strategy == 0 && !corr && ldy % 4 == 0 && ldy >= ((dmax + 15) / 16) * 16`` holds with
    ldy = d a multiple of 16: ``distances_seq_kernel``, columns emitted at j + 1 = 1, 2, 15, 16
    (the last lane of a 16-wide group), 17 (the first of the next) ... as far as they fit."""
    Y = _embedding(d)
    dims = _fit(DIMS, d)
    assert dims[-1] in (16, 33, 64, 128)
    assert _float4_form("sequential", COS_EUC, d, dims)
    engine.set_embedding(Y)
    _rank_vs_oracle(engine, Y, dims, COS_EUC, "sequential")


def test_float4_kernel_tail_inside_wider_rows(engine):
    """d = 40, dims up to 32: ``ldy >= ((32 + 15) / 16) * 16 = 32`` and ``40 % 4 == 0``, so the
    float4 form runs on rows 160 B apart (16-byte aligned, not 64) and stops at
    ``j >= plan.dmax`` inside the row."""
    Y = _embedding(40)
    dims = [1, 15, 16, 17, 32]
    assert _float4_form("sequential", COS_EUC, 40, dims)
    engine.set_embedding(Y)
    _rank_vs_oracle(engine, Y, dims, COS_EUC, "sequential")


def test_float4_rule_falls_back_when_the_last_group_overruns_the_row(engine):
    """d = 40, dims = [33]: ``ldy >= ((33 + 15) / 16) * 16 = 48`` fails (the third 16-float
    group would read past the row), so the general form runs."""
    Y = _embedding(40)
    assert not _float4_form("sequential", COS_EUC, 40, [33])
    engine.set_embedding(Y)
    _rank_vs_oracle(engine, Y, [33], COS_EUC, "sequential")


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_float4_kernel_columns_in_request_order(engine, order):
    """The kernel emits by ascending dim; ``col_out`` puts every column back where the request
    (dims outer, metrics inner) has it."""
    Y = _embedding(128)
    if order == "reversed":
        dims = DIMS[::-1]
    else:
        dims = [int(x) for x in np.random.default_rng(2).permutation(DIMS)]
        assert dims != DIMS and dims != DIMS[::-1]
    assert _float4_form("sequential", COS_EUC, 128, dims)
    engine.set_embedding(Y)
    tables, names = _rank_vs_oracle(engine, Y, dims, COS_EUC, "sequential")
    assert names[0] == f"dim-{dims[0]}_distance-" + ("euclidean" if dims[0] == 1 else "cosine")
    # and they are the ascending request's columns, moved
    asc, asc_names = _rank_vs_oracle(engine, Y, DIMS, COS_EUC, "sequential")
    for c, name in enumerate(names):
        np.testing.assert_array_equal(tables[0][:, c], asc[0][:, asc_names.index(name)])


# ------------------------------------------------------------------- c. same arithmetic
def test_both_forms_give_the_same_bits(engine):
    """rank.hip: the float4 form takes "the same sums in the same order" as the general one.
    At d = 64 the cosine and euclidean columns of a run with correlation columns (general form)
    equal those of the run without (float4 form) bit for bit."""
    Y = _embedding(64)
    dims = _fit(DIMS, 64)
    assert not _float4_form("sequential", ALL_METRICS, 64, dims)
    assert _float4_form("sequential", COS_EUC, 64, dims)
    engine.set_embedding(Y)
    gen, gen_names = _rank_vs_oracle(engine, Y, dims, ALL_METRICS, "sequential")
    seq, seq_names = _rank_vs_oracle(engine, Y, dims, COS_EUC, "sequential")
    assert len(seq_names) == 2 * len(dims) - 1
    for cmp_ in range(K - 1):
        for c, name in enumerate(seq_names):
            g = gen[cmp_][:, gen_names.index(name)]
            np.testing.assert_array_equal(seq[cmp_][:, c], g, err_msg=f"{cmp_} {name}")


# ------------------------------------------------------------------- d, e. fitted layouts
FIT_DIMS = [1, 7, 16, 17, 24]


def _fitted_vs_oracle(eng):
    """Fit 3 ER layers of 1037 nodes at d = 24, then every strategy with all three metrics
    (general form) and the sequential strategy without correlation (float4 form: the fitted
    rows are padded) against the oracle on the embedding the engine returns."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(1037, 8, 3)
    eng.set_layers(layers)
    eng.uase(24, seed=5)
    Y = eng.embedding()
    assert Y.shape == (3, 1037, 24) and Y.dtype == np.float32 and np.isfinite(Y).all()
    for strategy in STRATEGIES:
        _rank_vs_oracle(eng, Y, FIT_DIMS, ALL_METRICS, strategy)
    _rank_vs_oracle(eng, Y, FIT_DIMS, COS_EUC, "sequential")
    _rank_vs_oracle(eng, Y, FIT_DIMS[::-1], COS_EUC, "sequential")


def test_fitted_layout_vs_oracle(engine):
    """One GPU after ``uase``: ``ldy`` padded, ``lrows = npad``."""
    _fitted_vs_oracle(engine)


def test_partitioned_fit_vs_oracle():
    """Three ranks: npad = ceil(1037 / 3) = 346, the last rank holds 345 rows.  Local columns
    go to ``Dloc`` with ``ldo = npad``, are all-gathered and cut to n."""
    from node2vec2rank_amd import _lib
    eng = _lib.Engine.multi([0, 0, 0])
    try:
        _fitted_vs_oracle(eng)
    finally:
        eng.close()


# ------------------------------------------------------------------- f. limits
def test_column_limit_and_dim_limit(engine):
    """256 ranking columns are accepted, 257 refused, a dim past d refused, and ``rank`` works
    afterwards.  (Cosine is skipped at dim 1, so 128 dims x {cosine, euclidean} is 255 columns;
    a repeated dim, which the reference allows, brings the float4 form to 256 and 257.)"""
    Y = _embedding(128)
    every = list(range(1, 129))
    engine.set_embedding(Y)
    # 128 dims x 2 metrics = 256 columns, general form
    tables, names = _rank_vs_oracle(engine, Y, every, ["euclidean", "correlation"], "sequential")
    assert len(names) == 256 and tables[0].shape == (N, 256)
    # 255 + 1 = 256 columns, float4 form
    assert _float4_form("sequential", COS_EUC, 128, every + [1])
    tables, names = _rank_vs_oracle(engine, Y, every + [1], COS_EUC, "sequential")
    assert len(names) == 256 and tables[0].shape == (N, 256)
    # 255 + 2 = 257
    with pytest.raises(ValueError):
        engine.rank("sequential", every + [2], COS_EUC)
    with pytest.raises(ValueError):
        engine.rank("sequential", every + [64], ["euclidean", "correlation"])  # 258
    with pytest.raises(ValueError):
        engine.rank("sequential", [4, 129], COS_EUC)
    with pytest.raises(ValueError):
        engine.rank("one_vs_rest", [129], ["euclidean"])
    _rank_vs_oracle(engine, Y, [1, 17, 128], COS_EUC, "sequential")
    _rank_vs_oracle(engine, Y, [1, 17, 128], ALL_METRICS, "one_vs_rest")
