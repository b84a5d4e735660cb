"""``n2v2r_layers_to_csr`` (csrc/sparsify.hip): dense-storage layers converted to CSR in HBM,
``Engine.to_csr`` / ``layer_csr`` and the ``sparsify`` option of ``set_layers``.

The oracle of the layout is ``scipy.sparse.csr_matrix(A)`` on the layer's own stored values: an
entry is stored when it is non-zero (a NaN is, -0.0 is not), columns ascend in every row.  The
conversion moves values and counts integers, so every comparison is bitwise unless stated
otherwise."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_coexpression import _expression

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_csr(a, b):
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and
            np.array_equal(a.indices, b.indices) and a.data.dtype == b.data.dtype == np.float32
            and np.array_equal(_bits(a.data), _bits(b.data)))


def _symmetric(n, count, seed):
    """A symmetric fp32 layer with exactly `count` non-zero entries (standard normal values)."""
    rng = np.random.default_rng(seed)
    pairs = n * (n - 1) // 2
    diag = min(n, count)
    if (count - diag) % 2:
        diag -= 1
    while (count - diag) // 2 > pairs:
        diag += 2
    assert 0 <= diag <= n and (count - diag) % 2 == 0
    vals = rng.standard_normal((n, n)).astype(np.float32)
    vals[vals == 0] = 1.0
    A = np.zeros((n, n), dtype=np.float32)
    iu = np.triu_indices(n, 1)
    pick = rng.choice(pairs, size=(count - diag) // 2, replace=False)
    A[iu[0][pick], iu[1][pick]] = vals[iu[0][pick], iu[1][pick]]
    A = A + A.T
    d = rng.choice(n, size=diag, replace=False)
    A[d, d] = vals[d, d]
    assert np.count_nonzero(A) == count and np.array_equal(A, A.T)
    return A


def _planted(n, seed):
    """About 10 percent dense, with an empty row, a full row, an entry in column n - 1 of the last
    row, -0.0 entries and one NaN (not symmetric: the handle keeps an A^T copy)."""
    rng = np.random.default_rng(seed)
    A = np.where(rng.random((n, n)) < 0.1, rng.standard_normal((n, n)), 0.0).astype(np.float32)
    A[0] = 0.0                                    # an empty row
    A[1] = np.float32(1.0) + np.arange(n, dtype=np.float32)  # a full row
    A[n - 1, n - 1] = 3.0
    A[2, ::2] = -0.0                              # -0.0 is zero: dropped
    A[2, 1] = np.nan                              # a NaN is non-zero: kept
    assert np.signbit(A[2, 0]) and A[2, 0] == 0
    return A


@pytest.mark.parametrize("n", [1, 63, 64, 65, 193, 257])
def test_layout_matches_scipy(engine, n):
    """n below, at and above the 64-column padding, and past one 256-column chunk (257).
    Densities 0 (next to non-empty layers), about 3 percent, exactly 25 percent (n even; the
    nearest count below it otherwise) and 100 percent, and the planted layer."""
    layers = [np.zeros((n, n), dtype=np.float32), _symmetric(n, round(0.03 * n * n), 1),
              _symmetric(n, n * n // 4, 2), _symmetric(n, n * n, 3)]
    if n >= 3:
        layers.append(_planted(n, 4))
    engine.set_layers(layers, storage="dense")
    assert engine.storage == "dense"
    assert engine.count_nonzeros() == [int(np.count_nonzero(A)) for A in layers]
    for k, A in enumerate(layers):  # (counting changed nothing)
        assert np.array_equal(_bits(engine.layer_dense(k)), _bits(A))
    counts = engine.to_csr()
    assert engine.storage == "csr"
    assert counts == [int(np.count_nonzero(A)) for A in layers]
    if n >= 3:
        assert counts[4] == sp.csr_matrix(layers[4]).nnz  # (the NaN counted, the -0.0 not)
    for k, A in enumerate(layers):
        ref = sp.csr_matrix(A)
        got = engine.layer_csr(k)
        assert got.shape == (n, n)
        assert _same_csr(got, ref), (n, k)
    with pytest.raises(ValueError, match="dense"):
        engine.layer_dense(0)
    if n >= 3:  # the planted layer is directed: its A^T copy came from the dense A^T
        assert _same_csr(engine.layer_csr(4, transpose=True),
                         sp.csr_matrix(np.ascontiguousarray(layers[4].T)))
    with pytest.raises(ValueError, match="symmetric"):
        engine.layer_csr(1, transpose=True)


def test_unit_layers(engine):
    """An all-ones pattern is an unweighted layer: data all 1.0f, and the column sums are those
    of the handle that ingested the same CSR."""
    from node2vec2rank_amd import Coexpression
    n = 193
    A = (_symmetric(n, 2001, 5) != 0).astype(np.float32)
    engine.set_layers([A], storage="dense")
    assert engine.to_csr() == [2001]
    got = engine.layer_csr(0)
    assert _same_csr(got, sp.csr_matrix(A))
    assert np.array_equal(_bits(got.data), np.full(2001, 0x3F800000, dtype=np.uint32))
    sums = engine.column_sums(0)
    engine.set_layers([sp.csr_matrix(A)])
    assert engine.storage == "csr"
    assert np.array_equal(sums, engine.column_sums(0))
    assert np.array_equal(sums, A.sum(axis=0, dtype=np.float32))
    # ... and the result of binarize=True
    layer = Coexpression(_expression(n, 37, seed=3), top_percent_keep=5, binarize=True)
    engine.set_layers([layer])
    B = engine.layer_dense(0)
    assert set(np.unique(B)) == {0.0, 1.0}
    assert engine.to_csr() == [int(np.count_nonzero(B))]
    got = engine.layer_csr(0)
    assert _same_csr(got, sp.csr_matrix(B)) and (got.data == 1.0).all()


def test_directed_layer(engine):
    """A 130 x 130 non-symmetric integer layer (six distinct values): the A^T copy is compacted
    from the dense A^T rows."""
    n = 130
    A = np.random.default_rng(7).integers(0, 6, size=(n, n)).astype(np.float32)
    assert not np.array_equal(A, A.T)
    engine.set_layers([A], storage="dense")
    assert engine.to_csr() == [int(np.count_nonzero(A))]
    assert _same_csr(engine.layer_csr(0), sp.csr_matrix(A))
    assert _same_csr(engine.layer_csr(0, transpose=True), sp.csr_matrix(np.ascontiguousarray(A.T)))
    sums = engine.column_sums(0)
    assert np.array_equal(sums, A.sum(axis=0, dtype=np.float32))  # (small integers: exact)
    engine.set_layers([sp.csr_matrix(A)])
    assert np.array_equal(sums, engine.column_sums(0))
    S = A + A.T
    engine.set_layers([S], storage="dense")
    engine.to_csr()
    with pytest.raises(ValueError, match="symmetric"):
        engine.layer_csr(0, transpose=True)


def _coex(E, **kw):
    from node2vec2rank_amd import Coexpression
    return [Coexpression(E, **kw), Coexpression(E, kind="signed", power=6.0, **kw)]


def test_same_state_as_the_csr_ingest_and_against_the_dense_fit(engine):
    """193 x 37, K = 2, top 5 percent: the converted handle and the handle that ingested the same
    layers as scipy CSR run the same kernels on the same CSR, so one Gram application (b = 8) and a
    fit from the same seed are bit-equal; the dense-storage fit of the same layers agrees on the
    singular values at rtol 1e-5 (the suite's bar for two fp32 fits of one matrix,
    test_gpu_layer_transform.test_fit_from_transformed_coexpression_layers)."""
    E = _expression(193, 37, seed=1000 * 193 + 37)
    X = np.random.default_rng(5).standard_normal((193, 8)).astype(np.float32)
    engine.set_layers(_coex(E, top_percent_keep=5))
    arrays = [engine.layer_dense(k) for k in range(2)]
    engine.uase(8, seed=11)
    s_dense = engine.singular_values()
    counts = engine.to_csr()
    assert counts == [int(np.count_nonzero(a)) for a in arrays]
    assert all(4 * c <= 193 * 193 for c in counts)
    W1, Z1, info1 = engine.gram_apply(X)
    engine.uase(8, seed=11)
    s1, Y1 = engine.singular_values(), engine.embedding()

    engine.set_layers([sp.csr_matrix(a) for a in arrays], storage="csr")
    for k in range(2):
        assert _same_csr(engine.layer_csr(k), sp.csr_matrix(arrays[k]))
    W2, Z2, info2 = engine.gram_apply(X)
    assert info1["form"] == info2["form"] and info1 == info2
    assert np.array_equal(_bits(W1), _bits(W2)) and np.array_equal(_bits(Z1), _bits(Z2))
    engine.uase(8, seed=11)
    assert np.array_equal(s1, engine.singular_values())
    assert np.array_equal(_bits(Y1), _bits(engine.embedding()))
    np.testing.assert_allclose(s1, s_dense, rtol=1e-5)


def test_set_layers_options(engine):
    E = _expression(193, 37, seed=1000 * 193 + 37)
    engine.set_layers(_coex(E, top_percent_keep=5), sparsify=True)
    assert engine.storage == "csr"
    first = engine.layer_csr(0)
    engine.set_layers(_coex(E, top_percent_keep=5), sparsify="auto")
    assert engine.storage == "csr" and _same_csr(engine.layer_csr(0), first)
    engine.set_layers(_coex(E), sparsify="auto")  # untransformed: every entry non-zero
    assert engine.storage == "dense"
    from node2vec2rank_amd import Coexpression
    engine.set_layers([Coexpression(E, top_percent_keep=5), Coexpression(E, top_percent_keep=50)],
                      sparsify="auto")  # one of the two above 1/4
    assert engine.storage == "dense"
    engine.set_layers(_coex(E, top_percent_keep=5))
    assert engine.storage == "dense"
    # dense arrays go the same way, counted on the GPU
    arrays = [engine.layer_dense(k) for k in range(2)]
    engine.set_layers(arrays, sparsify="auto")
    assert engine.storage == "csr" and _same_csr(engine.layer_csr(0), first)
    engine.set_layers([np.ones((5, 5), dtype=np.float32)], sparsify="auto")
    assert engine.storage == "dense"


def test_model_option_gives_the_default_run_s_frames():
    from node2vec2rank_amd.model import N2V2R
    n = 193
    E = _expression(n, 37, seed=1000 * 193 + 37)
    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[4, 8], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=11, verbose=-1, save_dir=None)
    frames = []
    for kw in ({}, dict(sparsify=True)):
        model = N2V2R(graphs=_coex(E, top_percent_keep=5), nodes=nodes, config=dict(config), **kw)
        out = model.fit_transform_rank()
        frames.append((out, model.aggregate_transform(), model.degree_difference_ranking()))
        assert model._eng.storage == ("csr" if kw else "dense")
    for a, b in zip(frames[0], frames[1]):
        assert list(a) == list(b) == ["1"]
        for key in a:
            assert list(a[key].columns) == list(b[key].columns)
            assert a[key].index.equals(b[key].index)
            assert a[key].shape == b[key].shape
            assert np.isfinite(b[key].to_numpy(dtype=np.float64)).all()


def _three_layers(E):
    """Two transformed co-expression layers (the second binarized: unit) and a directed one."""
    from node2vec2rank_amd import Coexpression
    D = np.random.default_rng(11).integers(0, 6, size=(193, 193)).astype(np.float32)
    return [Coexpression(E, threshold=0.1, top_percent_keep=37.5),
            Coexpression(E, kind="signed", power=6.0, top_percent_keep=5, binarize=True), D]


@pytest.fixture(scope="module")
def single_193(engine):
    E = _expression(193, 37, seed=1000 * 193 + 37)
    engine.set_layers(_three_layers(E))
    dense = [engine.layer_dense(k) for k in range(3)]
    counts = engine.to_csr()
    csr = [engine.layer_csr(k) for k in range(3)]
    for k in range(3):
        assert _same_csr(csr[k], sp.csr_matrix(dense[k]))
    csr_t = engine.layer_csr(2, transpose=True)
    assert _same_csr(csr_t, sp.csr_matrix(np.ascontiguousarray(dense[2].T)))
    return E, counts, csr, csr_t, engine.column_sums(2)


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rows_are_the_single_gpu_csr(single_193, world):
    """Bands that are not tile-aligned (row0 = 97; 65, 130): every rank converts its own rows
    (the directed layer's A^T rows too) and returns the global counts."""
    from test_gpu_dist import _run_ranks
    E, counts, csr, csr_t, sums = single_193

    def fn(eng, r):
        eng.set_layers(_three_layers(E))
        c = eng.to_csr()
        return (eng.dist_info(), c, eng.storage, [eng.layer_csr(k) for k in range(3)],
                eng.layer_csr(2, transpose=True), eng.column_sums(2))

    res = _run_ranks(world, fn)
    assert sorted(info[2] for info, *_ in res) == ([0, 97] if world == 2 else [0, 65, 130])
    for (_, _, row0, nl), c, storage, mats, mat_t, cs in res:
        assert c == counts and storage == "csr"
        for k in range(3):
            assert _same_csr(mats[k], csr[k][row0:row0 + nl]), (world, row0, k)
        assert _same_csr(mat_t, csr_t[row0:row0 + nl]), (world, row0)
        assert np.array_equal(cs, sums)


def test_multi_handle_returns_all_rows(single_193):
    from node2vec2rank_amd import _lib
    E, counts, csr, csr_t, sums = single_193
    eng = _lib.Engine.multi([0, 0, 0])
    try:
        eng.set_layers(_three_layers(E))
        assert eng.count_nonzeros() == counts
        assert eng.to_csr() == counts and eng.storage == "csr"
        for k in range(3):
            assert _same_csr(eng.layer_csr(k), csr[k])
        assert _same_csr(eng.layer_csr(2, transpose=True), csr_t)
        assert np.array_equal(eng.column_sums(2), sums)
        with pytest.raises(ValueError, match="already"):
            eng.to_csr()
        eng.set_layers(_coex(E, top_percent_keep=50), sparsify="auto")  # half the entries left
        assert eng.storage == "dense"
        eng.set_layers(_coex(E, top_percent_keep=5), sparsify="auto")
        assert eng.storage == "csr"
    finally:
        eng.close()


def test_refusals_leave_the_handle_alone(engine):
    from node2vec2rank_amd import _lib
    n = 193
    A = _symmetric(n, 3001, 9)

    def fit():
        engine.uase(4, seed=2)
        sv = engine.singular_values()
        assert np.isfinite(sv).all() and sv[0] > 0
        return sv

    # a handle whose layers are CSR already
    engine.set_layers([sp.csr_matrix(A)], storage="csr")
    s_csr = fit()
    with pytest.raises(ValueError, match="already"):
        engine.to_csr()
    with pytest.raises(ValueError, match="already"):
        engine.count_nonzeros()
    assert engine.storage == "csr" and _same_csr(engine.layer_csr(0), sp.csr_matrix(A))
    np.testing.assert_allclose(fit(), s_csr, rtol=1e-5)

    # a layer of the handle not loaded
    engine.set_layers([A], storage="dense")
    s0 = fit()
    assert engine.lib.n2v2r_set_num_layers(engine.h, 2, n) == _lib.OK
    assert engine.lib.n2v2r_set_layer_dense(engine.h, 0, n, A, _lib.SYM_DETECT) == _lib.OK
    engine.num_layers = 2
    with pytest.raises(ValueError, match="not loaded"):
        engine.to_csr()
    assert engine.storage == "dense"
    assert np.array_equal(_bits(engine.layer_dense(0)), _bits(A))
    # (the fit needs every layer: an all-zero second layer leaves the singular values of [A | 0])
    zeros = np.zeros((n, n), dtype=np.float32)
    assert engine.lib.n2v2r_set_layer_dense(engine.h, 1, n, zeros, _lib.SYM_DETECT) == _lib.OK
    np.testing.assert_allclose(fit(), s0, rtol=1e-5)

    # a successful call clears the embedding
    assert engine.to_csr() == [3001, 0]
    with pytest.raises(ValueError):
        engine.embedding()
