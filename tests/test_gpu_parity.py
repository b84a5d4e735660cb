"""HIP path vs the oracle and the reference's golden vectors (needs an MI355X)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import FIXTURES, fixture_layers, load_fixture
from oracle import n2v2r_oracle as orc

pytestmark = pytest.mark.gpu

# fixtures held to SURVEY 8(c)(4)'s end-to-end rank bar (tau >= 0.998, identical top set)
END_TO_END_STRICT = ("demo", "er_cfg1", "ties_nan", "directed_weighted")


# ----------------------------------------------------------------------------- SpMM
@pytest.mark.parametrize("b", [8, 16, 32, 64])
@pytest.mark.parametrize("name", ["er_cfg1", "directed_weighted", "demo"])
def test_spmm_matches_scipy(engine, name, b):
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    engine.set_layers(layers)
    rng = np.random.default_rng(b)
    X = rng.standard_normal((layers[0].shape[0], b)).astype(np.float32)
    for k, A in enumerate(layers):
        for tr in (False, True):
            Y, ms, by = engine.bench_spmm(k, X, transpose=tr, reps=2)
            M = A.T if tr else A
            ref = M.astype(np.float64) @ X.astype(np.float64)
            scale = np.abs(M).astype(np.float64) @ np.abs(X).astype(np.float64)
            assert np.all(np.abs(Y - ref) <= 1e-5 * scale + 1e-6), (name, k, tr)
            assert ms > 0 and by > 0


@pytest.mark.parametrize("name", ["er_cfg1", "directed_weighted", "demo"])
def test_spmm_column_blocks_matches_scipy(engine, name, monkeypatch):
    """The column-block SpMM (the flat-window tiled form), forced on, through n2v2r_bench_spmm."""
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    engine.set_layers(layers)
    assert engine.spmm_col_blocks(8) and not engine.spmm_col_blocks(16)
    X = np.random.default_rng(5).standard_normal((layers[0].shape[0], 8)).astype(np.float32)
    for k, A in enumerate(layers):
        for tr in (False, True):
            Y, ms, by = engine.bench_spmm(k, X, transpose=tr, reps=2)
            M = A.T if tr else A
            ref = M.astype(np.float64) @ X.astype(np.float64)
            scale = np.abs(M).astype(np.float64) @ np.abs(X).astype(np.float64)
            assert np.all(np.abs(Y - ref) <= 1e-5 * scale + 1e-6), (name, k, tr)
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    assert not engine.spmm_col_blocks(8)


@pytest.mark.parametrize("n,deg", [(1000, 4), (300_000, 16)])
@pytest.mark.parametrize("bad", [-1, "n"])
def test_set_layer_csr_rejects_out_of_range_columns(engine, n, deg, bad):
    """A column index outside [0, n) is refused at ingest (small layers: serial check; >= 2^22
    entries: the multi-threaded check), with the error text of the C-ABI."""
    nnz = n * deg
    indptr = np.arange(0, nnz + 1, deg, dtype=np.int64)
    indices = np.tile(np.arange(deg, dtype=np.int32), n)
    indices[nnz - 3] = -1 if bad == -1 else n
    data = np.ones(nnz, dtype=np.float32)
    engine._check(engine.lib.n2v2r_set_num_layers(engine.h, 1, n), "set_num_layers")
    st = engine.lib.n2v2r_set_layer_csr(engine.h, 0, n, nnz, indptr, indices, data, 1)
    with pytest.raises(Exception, match="out of range"):
        engine._check(st, "layer 0")


@pytest.mark.parametrize("n,deg", [(1000, 4), (300_000, 16)])
@pytest.mark.parametrize("fault", ["non_monotone", -1, "n"])
def test_set_layer_csr_rows_rejects_malformed_blocks(engine, n, deg, fault):
    """The rank-local ingest refuses a non-monotone indptr and out-of-range columns (either
    would hand the SpMM row spans / gathers outside its buffers)."""
    nnz = n * deg
    indptr = np.arange(0, nnz + 1, deg, dtype=np.int64)
    indices = np.tile(np.arange(deg, dtype=np.int32), n)
    if fault == "non_monotone":
        indptr[n // 2] = indptr[n // 2 + 1] + 1
    else:
        indices[nnz - 3] = -1 if fault == -1 else n
    data = np.ones(nnz, dtype=np.float32)
    engine._check(engine.lib.n2v2r_set_num_layers(engine.h, 1, n), "set_num_layers")
    st = engine.lib.n2v2r_set_layer_csr_rows(engine.h, 0, n, 0, n, nnz, indptr, indices, data)
    with pytest.raises(ValueError, match="monotone" if fault == "non_monotone" else "out of range"):
        engine._check(st, "layer 0 rows")


@pytest.mark.parametrize("symmetrise", [False, True])
def test_spmm_large_directed_host_transpose(engine, symmetrise):
    """Layers large enough (>= 2^22 entries) for the multi-threaded host transpose and symmetry
    check at ingest: A^T x through the stored transpose (or A itself when detected symmetric)
    matches scipy; an asymmetric layer wrongly detected symmetric would fail here."""
    n = 300_000
    rng = np.random.default_rng(11)
    A = sp.random(n, n, density=16.0 / n, format="csr", dtype=np.float32, random_state=rng)
    A.data = rng.integers(1, 5, A.nnz).astype(np.float32)
    if symmetrise:
        A = (A + A.T).tocsr()
    assert A.nnz >= 1 << 22
    engine.set_layers([A])
    X = rng.standard_normal((n, 8)).astype(np.float32)
    for tr in (False, True):
        Y, _, _ = engine.bench_spmm(0, X, transpose=tr, reps=1)
        M = A.T if tr else A
        ref = M.astype(np.float64) @ X.astype(np.float64)
        scale = np.abs(M).astype(np.float64) @ np.abs(X).astype(np.float64)
        assert np.all(np.abs(Y - ref) <= 1e-5 * scale + 1e-6), (symmetrise, tr)


@pytest.mark.parametrize("weighted", [False, True])
def test_spmm_b8_long_rows_and_empty_rows(engine, weighted):
    """The B = 8 pipelined kernel: rows longer than 32 (the non-pipelined remainder), empty
    rows, an odd row count, unit (unweighted) and weighted values."""
    rng = np.random.default_rng(11)
    n = 3001
    deg = rng.integers(0, 90, size=n)
    deg[::7] = 0
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, size=rows.size)
    vals = rng.standard_normal(rows.size).astype(np.float32) if weighted else np.ones(rows.size, np.float32)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    if not weighted:
        A.data[:] = 1.0
    engine.set_layers([A, A.T.tocsr()], symmetric=0)
    X = rng.standard_normal((n, 8)).astype(np.float32)
    for tr in (False, True):
        Y, _, _ = engine.bench_spmm(0, X, transpose=tr, reps=2)
        M = A.T if tr else A
        ref = M.astype(np.float64) @ X.astype(np.float64)
        scale = np.abs(M).astype(np.float64) @ np.abs(X).astype(np.float64)
        assert np.all(np.abs(Y - ref) <= 1e-5 * scale + 1e-6), tr


# ----------------------------------------------------------------------------- UASE
def _envelope(layers, d, seed):
    """The reference's own seed-to-seed deviation (ARPACK start vector seed vs seed+1)."""
    Ya, sa, _ = orc.uase(layers, d, seed=seed)
    Yb, sb, _ = orc.uase(layers, d, seed=seed + 1)
    Yb = orc.align_signs(Yb, Ya)
    return np.abs(Ya - Yb).max() / np.abs(Ya).max(), Yb


def _tau_envelope(Y_other, fx, strategy, key):
    """Kendall tau between the reference's Borda and the reference re-run from another ARPACK
    start vector (signs aligned, so correlation columns are comparable)."""
    from scipy.stats import kendalltau
    dims = [int(x) for x in fx["dims"]]
    metrics = [str(x) for x in fx["metrics"]]
    Ya = orc.align_signs(fx["Y"], Y_other)
    Da = orc.rank_distances(Ya, dims, metrics, strategy, faithful=True)[key][1]
    Db = orc.rank_distances(Y_other, dims, metrics, strategy, faithful=True)[key][1]
    return kendalltau(orc.borda(Da), orc.borda(Db)).statistic


ENV_SEEDS = 4


def _tau_envelope_unaligned(layers, fx, strategy):
    """The reference's envelope as a sign-arbitrary method sees it: Kendall tau between the
    reference's own Borda (quicksort ties, fx) and the reference's algorithm re-run from the
    ARPACK start vectors of seeds seed+1 .. seed+ENV_SEEDS with NO sign alignment (correlation
    distances depend on the per-column signs ARPACK leaves to its start vector), the minimum
    over those runs per comparison key."""
    from scipy.stats import kendalltau
    dims = [int(x) for x in fx["dims"]]
    metrics = [str(x) for x in fx["metrics"]]
    seed = int(fx["seed"])
    out = {}
    for s in range(seed + 1, seed + 1 + ENV_SEEDS):
        Y, _, _ = orc.uase(layers, max(dims), seed=s)
        for key, (_, D) in orc.rank_distances(Y, dims, metrics, strategy, faithful=True).items():
            t = kendalltau(orc.borda(D, faithful=True), fx[f"{strategy}/{key}/borda"]).statistic
            out[key] = min(out.get(key, 1.0), t)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_uase_matches_reference(engine, name):
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    d = int(fx["dims"].max())
    engine.set_layers(layers)
    st = engine.uase(d, seed=int(fx["seed"]))
    Y = engine.embedding().astype(np.float64)
    s = engine.singular_values()
    ref_Y, ref_s = fx["Y"], fx["sigma"]
    # singular values: fp32-level agreement
    np.testing.assert_allclose(s, ref_s, rtol=2e-5)
    env, _ = _envelope(layers, d, int(fx["seed"]))
    Ya = orc.align_signs(Y, ref_Y)
    err = np.abs(Ya - ref_Y).max() / np.abs(ref_Y).max()
    # SURVEY 8(c) contract: <= 5e-4 max|Y| on well-separated spectra; never tighter than 3x
    # the reference's own seed-to-seed deviation (near-degenerate columns).
    assert err <= max(5e-4, 3 * env), (name, err, env, st)


# ----------------------------------------------------------------------------- distances
@pytest.mark.parametrize("name", FIXTURES)
def test_distances_kernel_vs_oracle(engine, name):
    """Distances from a GIVEN embedding: fp64 arithmetic on the GPU vs the oracle."""
    fx = load_fixture(name)
    Y32 = fx["Y"].astype(np.float32)
    dims = [int(x) for x in fx["dims"]]
    metrics = [str(x) for x in fx["metrics"]]
    engine.set_embedding(Y32)
    for strategy in [str(x) for x in fx["strategies"]]:
        ncmp, ncols = engine.rank(strategy, dims, metrics)
        ref = orc.rank_distances(Y32.astype(np.float64), dims, metrics, strategy)
        assert ncmp == len(ref)
        for c, (key, (cols, Dref)) in enumerate(ref.items()):
            D = engine.distances(c)
            assert D.shape == Dref.shape
            np.testing.assert_allclose(D, Dref, rtol=0, atol=1e-9, equal_nan=True)
            # Borda on the GPU's own distances: bit-exact with the stable oracle
            np.testing.assert_array_equal(engine.borda(c), orc.borda(D, faithful=False))


@pytest.mark.parametrize("name", ["demo", "er_cfg1", "directed_weighted"])
def test_spectral_uase_seam(name):
    """``spectral.UASE`` -- the replacement of ``se.UASE(sparce_graphs, d)`` (model.py:53-55):
    ``(XA, YA)`` with YA of shape (K, N, d) indexed as model.py:75-84 indexes it, matching the
    reference's embedding to its seed envelope; XA = U diag(sqrt(sigma)), so that
    YA_k = A_k^T XA diag(sigma)^-1."""
    from node2vec2rank_amd import spectral
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    d = int(fx["dims"].max())
    XA, YA = spectral.UASE([sp.csc_matrix(A) for A in layers], d, seed=int(fx["seed"]))
    n = layers[0].shape[0]
    assert XA.shape == (n, d) and YA.shape == (len(layers), n, d)
    assert XA.dtype == np.float64 and YA.dtype == np.float64
    env, _ = _envelope(layers, d, int(fx["seed"]))
    Ya = orc.align_signs(YA, fx["Y"])
    assert np.abs(Ya - fx["Y"]).max() / np.abs(fx["Y"]).max() <= max(5e-4, 3 * env)
    sigma = np.linalg.norm(XA, axis=0) ** 2
    np.testing.assert_allclose(sigma, fx["sigma"], rtol=2e-5)
    for k, A in enumerate(layers):
        Yk = (A.T.astype(np.float64) @ XA) / sigma[None, :]
        assert np.abs(Yk - YA[k]).max() <= 1e-4 * np.abs(YA[k]).max()


def test_pairwise_seam(engine):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((500, 7))
    b = rng.standard_normal((500, 7))
    a[3] = 0.0
    for m in ("cosine", "euclidean", "correlation"):
        got = engine.pairwise_distances(a, b, m)
        ref = orc.distances_faithful(a, b, m)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True)
    with pytest.raises(NotImplementedError):
        engine.pairwise_distances(a, b, "manhattan")


# ----------------------------------------------------------------------------- Borda
def _has_ties(c):
    v = c[~np.isnan(c)]
    v = np.where(v == 0.0, 0.0, v)  # -0 == +0
    return len(np.unique(v)) < len(v)


@pytest.mark.parametrize("name", FIXTURES)
def test_borda_bit_exact_given_reference_distances(engine, name):
    """Given the reference's distance table: the stable GPU order equals the stable oracle, and
    the reference tie order (GPU tie flags + pandas' order for the tied columns,
    model.py:173-174) equals the REFERENCE's own Borda bit for bit, ties included."""
    fx = load_fixture(name)
    n_tied = 0
    for strategy in [str(x) for x in fx["strategies"]]:
        for key in [str(k) for k in fx[f"{strategy}/keys"]]:
            D = fx[f"{strategy}/{key}/D"]
            got, tied = engine.borda_columns(D, return_tied=True)
            np.testing.assert_array_equal(got, fx[f"{strategy}/{key}/borda_stable"])
            np.testing.assert_array_equal(tied, [_has_ties(c) for c in D.T])
            n_tied += int(tied.sum())
            ref = engine.borda_columns(D, tie_order="reference")
            # this host's numpy must order ties as the one that made the fixture (else the
            # comparison below is between two numpy builds, not between us and the reference)
            np.testing.assert_array_equal(orc.borda(D, faithful=True),
                                          fx[f"{strategy}/{key}/borda"])
            np.testing.assert_array_equal(ref, fx[f"{strategy}/{key}/borda"])
    print(f"{name}: {n_tied} tied columns")
    if name in ("demo", "ties_nan", "k4_strategies"):
        assert n_tied > 0  # the fixtures that hold exact ties exercise the tied path


def test_borda_given_orders_validated(engine):
    """n2v2r_borda_columns_ex refuses a given order that is not a permutation (the GPU scatters
    by it) and sums a valid one exactly."""
    import ctypes
    from node2vec2rank_amd import _lib
    rng = np.random.default_rng(2)
    n = 1000
    D = np.round(rng.random((n, 3)) * 20)  # heavy ties
    Dc = np.ascontiguousarray(D.T)
    out = np.empty(n, dtype=np.int64)
    tied = np.empty(3, dtype=np.int32)
    cols = np.array([1], dtype=np.int32)
    perm = rng.permutation(n).astype(np.int32)[None, :]
    lib = engine.lib
    st = lib.n2v2r_borda_columns_ex(engine.h, Dc, n, 3, cols.ctypes.data_as(ctypes.c_void_p), 1,
                                    perm.ctypes.data_as(ctypes.c_void_p), out, tied)
    assert st == _lib.OK
    pos = np.empty(n, dtype=np.int64)
    pos[perm[0]] = np.arange(n)
    stable = [orc._descending_order_pandas(D[:, j], "stable") for j in (0, 2)]
    want = n - pos
    for o in stable:
        p = np.empty(n, dtype=np.int64)
        p[o] = np.arange(n)
        want += n - p
    np.testing.assert_array_equal(out, want)
    assert tied.tolist() == [1, 1, 1]
    bad = perm.copy()
    bad[0, 5] = bad[0, 6]
    for b, c in ((bad, cols), (perm, np.array([3], dtype=np.int32))):
        st = lib.n2v2r_borda_columns_ex(engine.h, Dc, n, 3, c.ctypes.data_as(ctypes.c_void_p), 1,
                                        b.ctypes.data_as(ctypes.c_void_p), out, tied)
        assert st == _lib.ERR_BAD_ARG


def test_borda_large_with_ties_nans_and_negzero(engine):
    rng = np.random.default_rng(3)
    n, c = 300_000, 5
    D = rng.random((n, c))
    D[rng.random((n, c)) < 0.1] = 0.5          # heavy ties
    D[rng.random((n, c)) < 0.01] = np.nan      # NaNs last
    D[:100, 0] = -0.0
    D[100:200, 0] = 0.0
    D[:, 4] = np.round(D[:, 4] * 1000) / 1000  # many ties
    got = engine.borda_columns(D)
    np.testing.assert_array_equal(got, orc.borda(D, faithful=False))
    assert got.sum() == c * n * (n + 1) // 2   # every column is a permutation
    # the reference's tie order (pandas / numpy quicksort, model.py:173-174) on every column
    np.testing.assert_array_equal(engine.borda_columns(D, tie_order="reference"),
                                  orc.borda(D, faithful=True))


def test_borda_label_seam():
    from node2vec2rank_amd.model_utils import borda_aggregate_parallel
    labels = [f"g{i}" for i in range(50)]
    rng = np.random.default_rng(1)
    rankings = [list(np.array(labels)[rng.permutation(50)]) for _ in range(4)]
    got = borda_aggregate_parallel(rankings)
    idx = rankings[0]
    ref = np.array([[50 - r.index(node) for node in idx] for r in rankings]).sum(axis=0)
    assert list(got.index) == idx
    np.testing.assert_array_equal(got["borda_ranks"].to_numpy(), ref)


# ----------------------------------------------------------------------------- end to end
def _cfg(fx, strategy):
    return dict(embed_dimensions=[int(x) for x in fx["dims"]],
                distance_metrics=[str(x) for x in fx["metrics"]], seed=int(fx["seed"]),
                comp_strategy=strategy, verbose=-1, save_dir=None)


def eng_stable_borda(df):
    from node2vec2rank_amd import _lib
    return _lib.default_engine().borda_columns(df.to_numpy(dtype=np.float64), tie_order="stable")


@pytest.mark.parametrize("name", FIXTURES)
def test_model_end_to_end(name):
    from node2vec2rank_amd.model import N2V2R
    from scipy.stats import kendalltau
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    nodes = [str(x) for x in fx["nodes"]]
    d = int(fx["dims"].max())
    env, Y_other = _envelope(layers, d, int(fx["seed"]))
    env_unaligned = {}
    if name not in END_TO_END_STRICT:
        env_unaligned = {s: _tau_envelope_unaligned(layers, fx, s)
                         for s in [str(x) for x in fx["strategies"]]}
    for strategy in [str(x) for x in fx["strategies"]]:
        model = N2V2R(graphs=layers, nodes=nodes, config=_cfg(fx, strategy))
        ranks = model.fit_transform_rank()
        agg = model.aggregate_transform()
        keys = [str(k) for k in fx[f"{strategy}/keys"]]
        assert list(ranks) == keys and list(agg) == keys
        # correlation distances centre each embedding row, so unlike cosine/euclidean they
        # depend on the SVD's arbitrary per-column signs (ARPACK start vector in the
        # reference).  Their expected values are the reference embedding re-signed to ours.
        Y_al = orc.align_signs(fx["Y"], model.node_embeddings)
        ref_al = orc.rank_distances(Y_al, [int(x) for x in fx["dims"]],
                                    [str(x) for x in fx["metrics"]], strategy, faithful=True)
        for key in keys:
            df = ranks[key]
            cols = [str(c) for c in fx[f"{strategy}/{key}/cols"]]
            assert list(df.columns) == cols
            assert list(df.index) == nodes
            Dref = fx[f"{strategy}/{key}/D"].copy()
            corr = np.array(["correlation" in c for c in cols])
            Dref[:, corr] = ref_al[key][1][:, corr]
            D = df.to_numpy()
            np.testing.assert_array_equal(np.isnan(D), np.isnan(Dref))
            derr = np.nanmax(np.abs(D - Dref))
            # 1e-4 unless the reference's own seed envelope is wider
            assert derr <= max(1e-4, 20 * env), (name, strategy, key, derr, env)
            b = agg[key]["borda_ranks"].to_numpy()
            assert agg[key]["borda_ranks"].dtype == np.int64
            # aggregate_transform orders tied columns as the reference (pandas quicksort), so
            # the integer ranks compare with the reference's own Borda; correlation columns
            # against the reference's distances re-signed to ours, in the reference's order
            ref_b = (orc.borda(Dref, faithful=True) if corr.any()
                     else fx[f"{strategy}/{key}/borda"])
            tau = kendalltau(b, ref_b).statistic
            k = min(100, len(nodes) // 10)
            top = len(set(np.argsort(-b, kind="stable")[:k]) &
                      set(np.argsort(-ref_b, kind="stable")[:k]))
            exact = bool(np.array_equal(b, ref_b))
            print(f"{name}/{strategy}/{key}: Kendall tau {tau:.6f}, top-{k} overlap {top}, "
                  f"bit-exact {exact}")
            if name in END_TO_END_STRICT:
                # tau >= 0.998 and the identical top-100 set (top N/10 below
                # 1000 nodes)
                assert tau >= 0.998 and top == k, (name, strategy, key, tau, top)
            else:
                # k4_strategies (400-node SBM, dims 1..6, correlation columns): near-tied
                # distances make its ranks noise-level even for the reference.  Correlation
                # distances depend on the SVD's per-column signs, which the reference leaves to
                # ARPACK's start vector and the engine fixes (svd_flip), so no sign-arbitrary
                # method can match them; the bar is the reference's own envelope as such a
                # method sees it: tau of the reference's Borda against the reference re-run from
                # other start vectors, without sign alignment, the minimum over ENV_SEEDS runs
                # (and against the drop-in's own correlation-free-of-sign comparison above)
                # (a) the drop-in's output against the reference's output as they are
                tau_ref = kendalltau(b, fx[f"{strategy}/{key}/borda"]).statistic
                env_un = env_unaligned[strategy][key]
                # (b) with the signs aligned and both sides in the stable tie order (numpy
                # quicksort's order of the 0 / 2 ties of the 2-d correlation column changes with
                # any perturbation of the column, so only the stable order compares ties)
                tau_st = kendalltau(eng_stable_borda(df), orc.borda(Dref)).statistic
                env_al = _tau_envelope(Y_other, fx, strategy, key)
                print(f"    vs the reference's Borda as is: tau {tau_ref:.6f} (reference "
                      f"envelope, unaligned, min of {ENV_SEEDS}: {env_un:.6f}); signs aligned, "
                      f"stable ties: tau {tau_st:.6f} (envelope {env_al:.6f})")
                assert tau_ref >= min(0.998, env_un), (name, strategy, key, tau_ref, env_un)
                assert tau_st >= min(0.998, env_al - 0.01), (name, strategy, key, tau_st, env_al)
        Y = model.node_embeddings
        assert Y.shape == fx["Y"].shape


def test_model_errors():
    from node2vec2rank_amd.model import N2V2R
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    cfg = _cfg(fx, "sequential")
    m = N2V2R(graphs=layers, nodes=list(range(layers[0].shape[0])), config=cfg)
    with pytest.raises(ValueError):
        m.aggregate_transform()
    m.fit_transform_rank()
    with pytest.raises(NotImplementedError):
        m.aggregate_transform(method="mean")
    bad = dict(cfg, distance_metrics=["manhattan"])
    with pytest.raises(NotImplementedError):
        N2V2R(graphs=layers, nodes=list(range(layers[0].shape[0])), config=bad).fit_transform_rank()


def test_dedi_matches_reference():
    from node2vec2rank_amd.model import N2V2R
    fx = load_fixture("demo")
    layers = fixture_layers(fx)
    m = N2V2R(graphs=layers, nodes=[str(x) for x in fx["nodes"]], config=_cfg(fx, "sequential"))
    dd = m.degree_difference_ranking()
    np.testing.assert_array_equal(dd["1"]["DeDi"].to_numpy(), fx["dedi/1"])


def test_demo_recall_known_answer():
    """Quality pin: notebooks/node2vec2rank_demo.ipynb:176-177 (n2v2r 0.68, DeDi 0.0)."""
    import os
    from conftest import GOLDEN
    from node2vec2rank_amd.model import N2V2R
    fx = load_fixture("demo")
    layers = fixture_layers(fx)
    m = N2V2R(graphs=layers, nodes=[str(x) for x in fx["nodes"]], config=_cfg(fx, "sequential"))
    m.fit_transform_rank()
    b = m.aggregate_transform()["1"]["borda_ranks"].to_numpy()
    comm = np.load(os.path.join(GOLDEN, "demo_communities.npy"))
    rel = set(np.where(comm == 0)[0])
    top = np.argsort(-b, kind="stable")[:len(rel)]
    assert abs(len(rel & set(top)) / len(rel) - 0.68) <= 0.02


# ----------------------------------------------------------------------------- larger sizes
def test_uase_residuals_er_20k(engine):
    """Size-independent property at a mid size: every Ritz pair's true residual (recomputed
    on the host from the returned embedding) and sigma vs the oracle's ARPACK."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_000, 20, 2)
    d = 32
    engine.set_layers(layers)
    st = engine.uase(d, seed=42)
    assert st["converged"] == d
    assert st["rr_fallbacks"] == 0, st   # every Sturm Rayleigh-Ritz vector passed its check
    s = engine.singular_values()
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]   # U
    A = sp.hstack(layers).tocsr().astype(np.float64)
    MU = A @ (A.T @ X)
    res = np.linalg.norm(MU - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5
    np.testing.assert_allclose(X.T @ X, np.eye(d), atol=1e-5)
    _, s_ref, _ = orc.uase(layers, d, seed=42)
    np.testing.assert_allclose(s, s_ref, rtol=1e-5)


@pytest.fixture(scope="module")
def tiled_layer():
    """A directed weighted layer (N = 300,001) with hub rows of 5,000 entries (runs of many steps,
    rows spanning steps) and 100 empty rows, for the tiled SpMM tests."""
    from node2vec2rank_amd import synthetic
    n = 300_001
    rng = np.random.default_rng(3)
    A = sp.triu(synthetic.er_layers(n, 12, 1, seed_base=91)[0], k=1, format="coo")
    hubs = np.array([0, 77, 150_000, n - 1])
    hr = np.repeat(hubs, 5000)
    hc = np.concatenate([rng.choice(n, 5000, replace=False) for _ in hubs])
    keep = (A.row < 1000) | (A.row >= 1100)                  # rows 1000..1099 empty
    A = sp.coo_matrix((np.ones(keep.sum() + hr.size, np.float32),
                       (np.concatenate([A.row[keep], hr]), np.concatenate([A.col[keep], hc]))),
                      shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.data = rng.uniform(0.5, 2.0, A.nnz).astype(np.float32)  # weighted
    X = rng.standard_normal((n, 8)).astype(np.float32)
    refs = {}
    for tr in (False, True):
        M = (A.T if tr else A).tocsr().astype(np.float64)
        refs[tr] = (M @ X.astype(np.float64),
                    1e-5 * (abs(M) @ np.abs(X).astype(np.float64)) + 1e-6)
    return A, X, refs


@pytest.mark.parametrize("wbits", ["", "5", "6", "7"])
@pytest.mark.parametrize("nb", [0, 4, 32, 64])
def test_spmm_tiled_flat_blocks(engine, monkeypatch, tiled_layer, nb, wbits):
    """The flat-window tiled SpMM (b = 8) against scipy on every row, on a directed weighted layer
    (A and A^T) whose panel spans 4-64 column blocks (0: the fit's rule), windows of 32, 64 or
    128 rows ("": the fit's rule), hub rows, empty rows and an odd row count."""
    if wbits:
        monkeypatch.setenv("N2V2R_SPMM_WBITS", wbits)
    A, X, refs = tiled_layer
    engine.set_layers([A])
    for tr in (False, True):
        Y, ms = engine.bench_spmm_tiled(0, X, transpose=tr, nb=nb, reps=2)
        ref, bound = refs[tr]
        assert np.all(np.abs(Y - ref) <= bound), (nb, wbits, tr)


@pytest.mark.parametrize("nb", [4, 64])
def test_spmm_tiled_register_windows_bit_identical(engine, monkeypatch, tiled_layer, nb):
    """The flat kernel's register-window form (each wave also keeps one 64-row window's
    accumulators in VGPRs; the default for launches of more than one round of resident tiles,
    N2V2R_SPMM_VW=2 forces it at this size) is bit-identical to the LDS-only form: the same
    segment sums in the same order, handed to the rows' owners through the staging slot; both
    orientations, hub rows, empty rows, the partial last tile."""
    monkeypatch.setenv("N2V2R_SPMM_WBITS", "6")
    A, X, refs = tiled_layer
    engine.set_layers([A])
    for tr in (False, True):
        monkeypatch.setenv("N2V2R_SPMM_VW", "0")
        Y0, _ = engine.bench_spmm_tiled(0, X, transpose=tr, nb=nb, reps=1)
        monkeypatch.setenv("N2V2R_SPMM_VW", "2")
        Y1, _ = engine.bench_spmm_tiled(0, X, transpose=tr, nb=nb, reps=2)
        assert np.array_equal(Y0, Y1), (nb, tr)
        ref, bound = refs[tr]
        assert np.all(np.abs(Y1 - ref) <= bound), (nb, tr)


def test_fit_register_windows_bit_identical(engine, monkeypatch):
    """A whole fit on the tiled SpMM (both stages, the sum mode included) with every launch in
    the register-window form is bit-identical to the LDS-only form."""
    from node2vec2rank_amd import synthetic
    engine.set_layers(synthetic.er_layers(300_007, 16, 2, seed_base=31))
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    monkeypatch.setenv("N2V2R_SPMM_WBITS", "6")
    monkeypatch.setenv("N2V2R_SPMM_VW", "0")
    st0 = engine.uase(32, seed=8)
    s0, U0 = engine.singular_values(), engine.left_embedding()
    monkeypatch.setenv("N2V2R_SPMM_VW", "2")
    st1 = engine.uase(32, seed=8)
    assert st0["block_applications"] == st1["block_applications"] and st1["converged"] == 32
    assert np.array_equal(engine.singular_values(), s0)
    assert np.array_equal(engine.left_embedding(), U0)


@pytest.mark.parametrize("d", [60, 64, 100, 128])
def test_embedding_from_lean_check_bit_identical(engine, monkeypatch, d):
    """With the tiled SpMM on one GPU, the final lean check's stage-1 products A_k^T X of the d
    wanted Ritz vectors are kept as the embedding (sign and sigma^-1/2 folded into one column
    scale) instead of d/8 more SpMM launches: the same launch and summation order, so the
    embedding is bit-identical to the computed one (N2V2R_YCAP=0), and it matches
    A_k^T U diag(sigma)^-1/2 in fp64 on the host.  d = 60: the last kept block runs past d (its
    extra columns scaled by 0); d = 100: the d/8 blocks do not cover the padded width, so the
    embedding is computed (the same bar holds either way)."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(60_000, 18, 2, seed_base=23)
    engine.set_layers(layers)
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    monkeypatch.setenv("N2V2R_YCAP", "0")
    st0 = engine.uase(d, seed=42)
    assert st0["y_captured"] == 0, st0
    Y0 = engine.embedding().copy()
    monkeypatch.setenv("N2V2R_YCAP", "1")
    st = engine.uase(d, seed=42)
    assert st["converged"] == d and st["lean_checks"] >= 1, st
    # the capture ran where the d/8 blocks cover the padded width (d = 60, 64, 128), not at 100
    assert st["y_captured"] == (0 if d == 100 else 1), st
    Y1 = engine.embedding()
    assert np.array_equal(Y0, Y1)
    s = engine.singular_values()
    U = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    for k, A in enumerate(layers):
        ref = (A.T.astype(np.float64) @ U) / np.sqrt(s)[None, :]
        assert np.abs(Y1[k] - ref).max() <= 1e-5 * np.abs(ref).max(), k


@pytest.mark.parametrize("defer", ["1", "0"])
def test_uase_paired_full_passes(engine, monkeypatch, defer):
    """Paired full passes (the default with lean images) against one full pass per block
    (N2V2R_REORTH_DEFER=0): both meet the residual bar recomputed on the host, keep U
    orthonormal, and agree on sigma; the pairing changes neither the block applications nor the
    cycles by more than one cycle's worth."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(30_000, 16, 2, seed_base=31)
    d = 48
    engine.set_layers(layers)
    monkeypatch.setenv("N2V2R_REORTH_DEFER", "0")
    st0 = engine.uase(d, seed=7)
    s0 = engine.singular_values()
    monkeypatch.setenv("N2V2R_REORTH_DEFER", defer)
    st = engine.uase(d, seed=7)
    assert st["converged"] == d, st
    s = engine.singular_values()
    np.testing.assert_allclose(s, s0, rtol=1e-5)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 5e-6, res.max()
    np.testing.assert_allclose(X.T @ X, np.eye(d), atol=1e-5)
    assert abs(st["block_applications"] - st0["block_applications"]) <= 48, (st, st0)


@pytest.mark.parametrize("name", ["er_cfg1", "directed_weighted", "demo"])
def test_uase_column_blocks_golden(engine, name, monkeypatch):
    """The flat-window tiled column-block SpMM (forced on at fixture size; by default it runs
    for b = 8 panels beyond 8 MB) reproduces the reference embedding: symmetric, directed (A^T
    split) and weighted layers."""
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    d = int(fx["dims"].max())
    engine.set_layers(layers)
    engine.uase(d, seed=int(fx["seed"]), block=8)
    np.testing.assert_allclose(engine.singular_values(), fx["sigma"], rtol=2e-5)
    Ya = orc.align_signs(engine.embedding().astype(np.float64), fx["Y"])
    env, _ = _envelope(layers, d, int(fx["seed"]))
    err = np.abs(Ya - fx["Y"]).max() / np.abs(fx["Y"]).max()
    assert err <= max(5e-4, 3 * env), (name, err, env)


@pytest.mark.parametrize("nb", ["", "4", "64"])
def test_uase_column_blocks_er_20k(engine, monkeypatch, nb):
    """The flat-window tiled column-block SpMM vs the row SpMM on a 20k-node ER graph with a
    ragged column count (20,003: the last block is short), at the fit's block count and at 4 and
    64 blocks: same sigma within fp32 tolerance, true residuals, and run-to-run bit-identical
    embeddings (fixed summation order; the LDS adds of a row all come from one wave)."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_003, 20, 2)
    d = 32
    engine.set_layers(layers)
    if nb:
        monkeypatch.setenv("N2V2R_SPMM_TILE_NB", nb)
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    engine.uase(d, seed=42)
    s_row = engine.singular_values().copy()
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    st = engine.uase(d, seed=42)
    assert st["converged"] == d
    s = engine.singular_values()
    Y1 = engine.embedding().copy()
    np.testing.assert_allclose(s, s_row, rtol=1e-5)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5
    # the embedding images (the fit's SpMM form): Y_k = A_k^T U diag(sigma)^-1/2
    for k, Ak in enumerate(layers):
        Yk = (Ak.T.astype(np.float64) @ X) / np.sqrt(s)[None, :]  # X = U here
        assert np.abs(Y1[k] - Yk).max() <= 1e-5 * np.abs(Yk).max(), k
    engine.uase(d, seed=42)
    assert np.array_equal(engine.embedding(), Y1)
    assert st["spmm_form"] == 5, st["spmm_form"]


@pytest.mark.parametrize("layers_k", [2, 3])
def test_uase_split_stage2(engine, monkeypatch, layers_k):
    """XCD-split second SpMM stage (per-layer partials, W stored by the next Gram pass) vs the
    summed stage: same sigma within fp32 tolerance, true residuals, bit-identical reruns."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_003, 16, layers_k)
    d = 24
    engine.set_layers(layers)
    monkeypatch.setenv("N2V2R_SPMM_SPLIT", "0")
    engine.uase(d, seed=7)
    s_sum = engine.singular_values().copy()
    monkeypatch.setenv("N2V2R_SPMM_SPLIT", "1")
    st = engine.uase(d, seed=7)
    assert st["converged"] == d
    s = engine.singular_values()
    Y1 = engine.embedding().copy()
    np.testing.assert_allclose(s, s_sum, rtol=1e-5)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5
    engine.uase(d, seed=7)
    assert np.array_equal(engine.embedding(), Y1)


@pytest.mark.parametrize("mode", ["lean", "images_kept"])
def test_uase_lean_images_selective_reorth(engine, monkeypatch, mode):
    """Lean images (Krylov-Schur residual estimates, the true residuals checked before the fit
    ends) and selective reorthogonalisation (full passes apply only the blocks above tol/10)
    vs the fit with every image kept and every block of every full
    pass applied: same sigma within fp32 tolerance, true residuals and orthonormal U on the
    host, the engine's reported residual matching the host's, bit-identical reruns."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_003, 16, 2)
    d = 32
    engine.set_layers(layers)
    monkeypatch.setenv("N2V2R_LEAN_W", "0")
    monkeypatch.setenv("N2V2R_REORTH_TOL", "0")
    engine.uase(d, seed=11)
    s_ref = engine.singular_values().copy()
    monkeypatch.setenv("N2V2R_LEAN_W", "0" if mode == "images_kept" else "1")
    monkeypatch.delenv("N2V2R_REORTH_TOL")
    st = engine.uase(d, seed=11)
    assert st["converged"] == d and st["rr_fallbacks"] == 0, st
    s = engine.singular_values()
    Y1 = engine.embedding().copy()
    np.testing.assert_allclose(s, s_ref, rtol=1e-5)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5
    assert st["max_residual"] <= 1e-6
    # the reported residual is a true one (fp32 products on the GPU vs fp64 here)
    assert abs(st["max_residual"] - res.max()) < 0.5 * res.max() + 2e-7, (st["max_residual"], res.max())
    np.testing.assert_allclose(X.T @ X, np.eye(d), atol=1e-5)
    engine.uase(d, seed=11)
    assert np.array_equal(engine.embedding(), Y1)


@pytest.mark.parametrize("lean", ["1", "0"])
def test_uase_banded_rr_failure_fallbacks(engine, monkeypatch, lean):
    """Every banded Rayleigh-Ritz result forced to fail (test flag 8): the Sturm stage falls
    back to the reducing band path, that one to the dense Rayleigh-Ritz, and a lean-image fit
    (which cannot form the dense H) reruns with every image kept.  The embedding still matches
    the reference fixture."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    d = int(fx["dims"].max())
    engine.set_layers(layers)
    monkeypatch.setenv("N2V2R_LEAN_W", lean)
    st = engine.uase(d, seed=int(fx["seed"]), solver_flags=8)
    assert st["converged"] == d
    assert st["rr_fallbacks"] >= 1
    np.testing.assert_allclose(engine.singular_values(), fx["sigma"], rtol=2e-5)
    Ya = orc.align_signs(engine.embedding().astype(np.float64), fx["Y"])
    env, _ = _envelope(layers, d, int(fx["seed"]))
    err = np.abs(Ya - fx["Y"]).max() / np.abs(fx["Y"]).max()
    assert err <= max(5e-4, 3 * env), err


@pytest.mark.parametrize("block", [8, 16, 64])
@pytest.mark.parametrize("name", ["er_cfg1", "directed_weighted", "demo"])
def test_uase_block_widths(engine, name, block):
    """Every supported Krylov block width reproduces the reference embedding."""
    fx = load_fixture(name)
    layers = fixture_layers(fx)
    d = int(fx["dims"].max())
    engine.set_layers(layers)
    engine.uase(d, seed=int(fx["seed"]), block=block)
    np.testing.assert_allclose(engine.singular_values(), fx["sigma"], rtol=2e-5)
    Ya = orc.align_signs(engine.embedding().astype(np.float64), fx["Y"])
    env, _ = _envelope(layers, d, int(fx["seed"]))
    err = np.abs(Ya - fx["Y"]).max() / np.abs(fx["Y"]).max()
    assert err <= max(5e-4, 3 * env), (name, block, err, env)


# ----------------------------------------------------------------------------- Rayleigh-Ritz
@pytest.mark.parametrize("form", ["multi", "one"])
@pytest.mark.parametrize("c,p", [(40, 12), (256, 80), (300, 100), (512, 160), (600, 150),
                                 (737, 64), (768, 200)])
def test_rayleigh_ritz_stage(engine, monkeypatch, c, p, form):
    """GPU tridiagonalisation (the multi-workgroup form: 32 x 32 tiles in the LDS of PR x nt
    workgroups, one grid barrier per step; and the one-workgroup kernel, N2V2R_RR_TRI=1) +
    tridiagonal bisection / inverse iteration + GPU back-transform vs numpy eigh, including a
    tight cluster (gaps 1e-9 relative) and an exactly repeated eigenvalue."""
    if form == "one":
        monkeypatch.setenv("N2V2R_RR_TRI", "1")
    rng = np.random.default_rng(c)
    ev = np.sort(rng.random(c))[::-1] * 100.0
    ev[3:8] = ev[3] - 1e-7 * np.arange(5)
    ev[10] = ev[11]
    Q, _ = np.linalg.qr(rng.standard_normal((c, c)))
    H = (Q * ev) @ Q.T
    H = H + 1e-12 * rng.standard_normal((c, c))  # not exactly symmetric, as QtW is not
    w, S = engine.rr_top(H, p)
    ref = np.sort(np.linalg.eigvalsh(0.5 * (H + H.T)))[::-1][:p]
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10 * ref[0])
    S = S.astype(np.float64)
    assert np.abs(S.T @ S - np.eye(p)).max() < 5e-6
    Hs = 0.5 * (H + H.T)
    assert np.abs(Hs @ S - S * w).max() < 5e-6 * ref[0]


def _band_problem(c, kp, seed, cluster=False, decoupled=0):
    """A projected matrix with the Krylov-Schur structure (see n2v2r_rr_band_top) and its
    band columns as UASE saves them."""
    b = 8
    rng = np.random.default_rng(seed)
    nb, j0 = c // b, kp // b
    H = np.zeros((c, c))
    theta = None
    cols = []
    if kp:
        theta = np.sort(rng.random(kp))[::-1] * 50.0 + 10.0
        if cluster:
            theta[5:12] = theta[5] - 1e-9 * np.arange(7)  # a tight cluster of kept Ritz values
            theta[20] = theta[21]
        H[:kp, :kp] = np.diag(theta)
    for j in range(j0, nb):
        o = j * b
        D = rng.standard_normal((b, b)) * 3.0
        D = D + D.T
        H[o:o + b, o:o + b] = D
        Dn = D + 1e-13 * rng.standard_normal((b, b))  # Q^T W is not exactly symmetric
        if j == j0:
            if kp:
                BT = rng.standard_normal((kp, b))
                if decoupled:
                    BT[:decoupled] *= 1e-9  # converged Ritz vectors: tiny residual couplings
                H[:kp, o:o + b] = BT
                H[o:o + b, :kp] = BT.T
                cols.append(np.vstack([BT, Dn]))
            else:
                cols.append(Dn)
        else:
            R = np.triu(rng.standard_normal((b, b)))
            H[o:o + b, o - b:o] = R
            H[o - b:o, o:o + b] = R.T
            cols.append(np.vstack([R.T, Dn]))
    hband = np.concatenate([m.ravel() for m in cols])
    return H, hband, theta


@pytest.mark.parametrize("c,kp,p,cluster,decoupled", [
    (40, 0, 12, False, 0), (256, 0, 80, False, 0), (256, 80, 80, False, 0),
    (256, 80, 80, True, 30), (384, 160, 160, False, 0), (512, 184, 184, True, 100),
    (96, 80, 80, False, 0)])
@pytest.mark.parametrize("method", ["sturm", "band"])
def test_rayleigh_ritz_band_stage(engine, monkeypatch, c, kp, p, cluster, decoupled, method):
    """Banded Rayleigh-Ritz vs numpy eigh of the same structured matrix, both forms: "sturm"
    (Sturm-count multisection + inverse iteration on the unreduced arrow + band matrix, the
    default) and "band" (arrow reduction, bulge chasing, bisection, tridiagonal inverse
    iteration, back-transform)."""
    monkeypatch.setenv("N2V2R_RR", method)
    H, hband, theta = _band_problem(c, kp, seed=c + kp, cluster=cluster, decoupled=decoupled)
    w, S = engine.rr_band_top(hband, c, kp, theta, p)
    ref = np.sort(np.linalg.eigvalsh(H))[::-1][:p]
    scale = np.abs(ref).max()
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10 * scale)
    S = S.astype(np.float64)
    assert np.abs(S.T @ S - np.eye(p)).max() < 5e-6
    assert np.abs(H @ S - S * w).max() < 5e-6 * scale


def test_uase_rank_deficient_krylov(engine):
    """Disjoint cliques: M has two distinct eigenvalues per component size, so the block Krylov
    space breaks down after a few blocks and the orthogonalisation has to refill rank-deficient
    columns (random restarts inside the basis).  Singular values must still match scipy and U
    must be orthonormal with small residuals."""
    import scipy.sparse.linalg as sla
    rng = np.random.default_rng(5)
    sizes = [5] * 60 + [7] * 40 + [9] * 20 + [3] * 100  # 1,060 nodes, 4 clique sizes
    layers = []
    for k in range(2):
        perm = rng.permutation(sum(sizes))
        blocks = []
        off = 0
        for sz in sizes:
            blocks.append(np.full((sz, sz), 1.0) - np.eye(sz))
            off += sz
        A = sp.block_diag(blocks).tocsr().astype(np.float32)
        A = A[perm][:, perm]  # hide the block structure from the row order
        layers.append(sp.csr_matrix(A))
    d = 12
    engine.set_layers(layers)
    st = engine.uase(d, seed=3, raise_on_no_convergence=False)
    s = engine.singular_values()
    M = sum((A @ A.T).astype(np.float64) for A in layers)
    ev = np.sort(sla.eigsh(M, k=d + 4, which="LA")[0])[::-1][:d]
    np.testing.assert_allclose(s, np.sqrt(ev), rtol=1e-4)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]  # U sqrt(sigma) -> U
    assert np.abs(X.T @ X - np.eye(d)).max() < 1e-4
    R = M @ X - X * (s ** 2)[None, :]
    assert np.linalg.norm(R, axis=0).max() <= 1e-4 * s[0] ** 2, st


def test_uase_cycle_redo_path(engine):
    """The recovery after a rank-deficient second pass (the cycle expanded again with three
    passes) gives the same Ritz values as the normal path."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    engine.set_layers(layers)
    d = int(fx["dims"].max())
    engine.uase(d, seed=7)
    s0 = engine.singular_values()
    st = engine.uase(d, seed=7, solver_flags=4)
    np.testing.assert_allclose(engine.singular_values(), s0, rtol=1e-5)
    np.testing.assert_allclose(engine.singular_values(), fx["sigma"], rtol=2e-5)
    assert st["converged"] == d


@pytest.mark.parametrize("d", [320, 600])
def test_uase_large_dimension(engine, d):
    """Embedding dimensions above 256 (the reference has no limit; the engine's is 600, set by
    the Rayleigh-Ritz basis of 768 columns): singular values vs scipy's eigsh of M, true
    residuals and orthonormality on the host."""
    import scipy.sparse.linalg as sla
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(3000, 40, 2, seed_base=77)
    engine.set_layers(layers)
    st = engine.uase(d, seed=5)
    assert st["converged"] == d or (st["stagnated"] and st["max_residual"] <= st["stag_cap"]), st
    s = engine.singular_values()
    M = sum((A @ A.T).astype(np.float64) for A in layers)
    ev = np.sort(sla.eigsh(M, k=d + 10, which="LA")[0])[::-1][:d]
    np.testing.assert_allclose(s, np.sqrt(ev), rtol=1e-5)
    U = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    assert np.abs(U.T @ U - np.eye(d)).max() < 1e-5
    R = M @ U - U * (s ** 2)[None, :]
    assert np.linalg.norm(R, axis=0).max() <= 1e-5 * s[0] ** 2
    with pytest.raises(ValueError):
        engine.uase(601, seed=5)


@pytest.mark.parametrize("n,d", [(20_003, 24), (100_000, 64), (300_001, 40)])
def test_uase_sign_convention(engine, n, d):
    """Every column of U has its largest-magnitude entry positive (the svd_flip rule the engine
    fixes signs with), at sizes whose column-max pass runs over hundreds to a thousand row
    chunks, with d not a multiple of the 32-column tile."""
    from node2vec2rank_amd import synthetic
    engine.set_layers(synthetic.er_layers(n, 12, 2, seed_base=n % 97))
    st = engine.uase(d, seed=3)
    assert st["converged"] == d
    U = engine.left_embedding()[:, :d]
    r = np.abs(U).argmax(axis=0)
    assert (U[r, np.arange(d)] > 0).all()


def test_uase_sturm_failure_reducing_path_no_pool_growth(engine):
    """Only the Sturm stage forced to fail (test flag 32) under lean images: every cycle falls
    back to the reducing band path, which succeeds, so the fit stays lean; the restart block
    built before the fallback is reused, so the solver's block pool does not grow beyond the
    normal fit's (advisor round 2: the fallback used to take a second block per failure)."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_003, 16, 2)
    d = 32
    engine.set_layers(layers)
    st0 = engine.uase(d, seed=21)
    s0 = engine.singular_values()
    st = engine.uase(d, seed=21, solver_flags=32)
    assert st["converged"] == d and st["rr_fallbacks"] == st["restarts"], st
    assert st["pool_blocks"] <= st0["pool_blocks"], (st["pool_blocks"], st0["pool_blocks"])
    s = engine.singular_values()
    np.testing.assert_allclose(s[:d], s0[:d], rtol=1e-5)
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5


def test_uase_large_kept_set_sturm_failure_dense_from_band(engine):
    """A kept set past the reducing band path's 192-row arrow (keep 224) still takes the lean,
    Sturm Rayleigh-Ritz; forced to fail there (test flag 32), each cycle's fallback is the dense
    Rayleigh-Ritz on H expanded from the saved band (rr_band_expand_kernel), not a refit without
    lean images.  Both fits: every pair converged, the same singular values, host fp64
    residuals.  A third fit also discards the first multi-workgroup tridiagonalisation of that
    dense step (test flag 1024), so the step is retried from the band with the one-workgroup
    kernel: one tridiagonalisation fallback, the same values and residuals."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(60_001, 20, 2, seed_base=77)
    d = 128
    cols = [0, d // 2, d - 1]
    A = sp.hstack(layers).tocsr().astype(np.float64)

    def host_residuals(s):
        X = engine.left_embedding().astype(np.float64)[:, cols]
        X /= np.sqrt(s[cols])[None, :]
        return np.linalg.norm(A @ (A.T @ X) - X * (s[cols] ** 2)[None, :], axis=0) / s[0] ** 2

    engine.set_layers(layers)
    st0 = engine.uase(d, seed=5, keep=224)
    s0 = engine.singular_values()
    st = engine.uase(d, seed=5, keep=224, solver_flags=32)
    s = engine.singular_values()
    assert st0["converged"] == d and st0["rr_fallbacks"] == 0, st0
    assert st["converged"] == d and st["rr_fallbacks"] == st["restarts"], st
    assert st["lean_checks"] > 0 and st0["lean_checks"] > 0, (st0, st)
    np.testing.assert_allclose(s[:d], s0[:d], rtol=1e-5)
    res = host_residuals(s)
    assert res.max() < 1e-5, res
    st2 = engine.uase(d, seed=5, keep=224, solver_flags=32 | 1024)
    s2 = engine.singular_values()
    assert st2["converged"] == d and st2["tri_fallbacks"] == 1, st2
    assert st2["rr_fallbacks"] == st2["restarts"], st2
    np.testing.assert_allclose(s2[:d], s0[:d], rtol=1e-5)
    res2 = host_residuals(s2)
    assert res2.max() < 1e-5, res2


def test_uase_dense_rr_tridiag_timeout_retry_bit_identical(engine, monkeypatch):
    """Dense Rayleigh-Ritz (flag 2) whose first multi-workgroup tridiagonalisation is discarded
    (test flag 1024): the step is redone with the one-workgroup kernel, which every later cycle
    keeps.  The retry recomputes H from Q and W with fixed-order reductions, so the fit issues
    the launches of a fit that ran the one-workgroup kernel from the start (N2V2R_RR_TRI=1) on
    the same inputs: bit-identical singular values and left embedding."""
    from node2vec2rank_amd import synthetic
    d = 32
    engine.set_layers(synthetic.er_layers(20_003, 16, 2))
    st = engine.uase(d, solver_flags=2 | 1024)
    s, U = engine.singular_values(), engine.left_embedding()
    assert st["converged"] == d and st["tri_fallbacks"] == 1, st
    monkeypatch.setenv("N2V2R_RR_TRI", "1")
    st1 = engine.uase(d, solver_flags=2)
    assert st1["converged"] == d and st1["tri_fallbacks"] == 0, st1
    assert np.array_equal(engine.singular_values(), s)
    assert np.array_equal(engine.left_embedding(), U)


@pytest.mark.parametrize("keep,flags", [(168, 0), (168, 32), (256, 0)])
def test_uase_basis_768_fused_lean(engine, keep, flags):
    """Bases up to N2V2R_BAND_MAXC = 768 columns on the lean, fused, banded path (the fused PIP
    pass past 64 KB of LDS, block lists past 96 entries): converged, the singular values of a
    640-column fit, host fp64 residuals; flag 32 fails every cycle's Sturm stage: past
    640 columns the fallback is the dense Rayleigh-Ritz on H expanded from the band (the
    reducing band path stays at <= 640 columns)."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(60_001, 20, 2, seed_base=78)
    d = 128
    engine.set_layers(layers)
    engine.uase(d, seed=5, max_basis=640)
    s0 = engine.singular_values()
    st = engine.uase(d, seed=5, keep=keep, max_basis=768, solver_flags=flags)
    s = engine.singular_values()
    assert st["converged"] == d and st["basis"] == 768 and st["lean_checks"] > 0, st
    assert st["rr_fallbacks"] == (st["restarts"] if flags else 0), st
    np.testing.assert_allclose(s[:d], s0[:d], rtol=1e-5)
    cols = [0, d // 2, d - 1]
    X = engine.left_embedding().astype(np.float64)[:, cols] / np.sqrt(s[cols])[None, :]
    A = sp.hstack(layers).tocsr().astype(np.float64)
    res = np.linalg.norm(A @ (A.T @ X) - X * (s[cols] ** 2)[None, :], axis=0) / s[0] ** 2
    assert res.max() < 1e-5, res


def test_uase_loose_tolerance_keeps_orthogonality(engine):
    """A loose residual tolerance (1e-3) must not loosen the basis orthogonality: the selective
    reorthogonalisation threshold is capped at 1e-6 and a pass whose block Gram is off the
    identity runs (advisor round 2)."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_003, 16, 2)
    d = 32
    engine.set_layers(layers)
    st = engine.uase(d, seed=4, tol=1e-3)
    assert st["converged"] == d, st
    s = engine.singular_values()
    X = engine.left_embedding().astype(np.float64) / np.sqrt(s)[None, :]
    assert np.abs(X.T @ X - np.eye(d)).max() < 1e-5
