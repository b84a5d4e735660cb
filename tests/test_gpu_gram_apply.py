"""One application W = M X = sum_k A_k (A_k^T X) as the solver launches it (``n2v2r_gram_apply``:
a ``GramOp`` set up as a fit's, its own ``apply``) against fp64 products from scipy / numpy, in
every form the operator takes: the row kernels with all layers in one launch, sum mode and the
XCD split (K up to 8), the flat tiled form with K > 1, the dense GEMMs' accumulation over layers,
and on a row partition the gather form and the (chunked) reduce-scatter form.

Bars (the suite's elementwise ones, per stage):
    stage 1   |Z_k - A_k^T X|          <= bar(|A_k^T| |X|)
    stage 2   |W - sum_k A_k Z_k^gpu|  <= bar(sum_k |A_k| |Z_k^gpu|)    (fp64 on the GPU's own Z)
with bar(s) = 1e-5 s + 1e-6 for CSR layers (test_spmm_matches_scipy) and 2e-6 s + 1e-6 for dense
ones (test_dense_gemm_matches_numpy).  Every output row is NaN-filled before the application, so a
row no launch wrote fails the NaN check; every case also asserts that a second call returns the
same bits and that ``info`` names the form the case is about.

Inputs are seeded.  Row kernels: n = 3,001 (odd: the last wave and the last row group are
partial), rows of 0..90 entries, every 7th row empty, one row of 700 entries near the start and
one in the last 8 rows of every layer (a different row per layer, so no row's total over 8 layers
passes the 5,000 entries the tiled tests' hubs already carry), layers cycling through directed
weighted, symmetric, and unit directed with rows 1000..1099 empty.  Tiled form: n = 40,003 (tiles
of 96 or 128 rows on 256 CUs, a partial last tile), ER layers of mean degree 12 with 700-entry hub
rows and rows 1000..1099 empty.  Dense: n = 1,037 (no multiple of 128 or 4).

Each case prints the largest fraction of its bars it reached (``pytest -s``)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import fixture_layers, load_fixture
from test_gpu_dist import _run_ranks

pytestmark = pytest.mark.gpu

N_ROWS = 3001
N_TILE = 40_003
N_DENSE = 1037
HUB = 700
BAND = (1000, 1100)  # rows left empty in some layers


def _bar(scale, dense):
    return (2e-6 if dense else 1e-5) * scale + 1e-6


def _in_band(i):
    return (i >= BAND[0]) & (i < BAND[1])


# ----------------------------------------------------------------------------- inputs
def _rows_layer(seed, kind, hubs, n=N_ROWS, maxlen=90):
    """kind "dw": directed weighted; "sym": symmetric weighted; "unit": directed, all values 1,
    rows 1000..1099 empty.  Every 7th row empty, the rows `hubs` with 700 entries."""
    rng = np.random.default_rng(seed)
    sym = kind == "sym"
    deg = rng.integers(0, (maxlen // 2 if sym else maxlen) + 1, size=n)
    deg[::7] = 0
    if kind == "unit":
        deg[BAND[0]:BAND[1]] = 0
    deg[list(hubs)] = 0
    # a symmetric layer keeps its empty rows only if no entry names them as a column
    allowed = np.flatnonzero(np.arange(n) % 7 != 0) if sym else np.arange(n)
    rows = [np.repeat(np.arange(n), deg)]
    cols = [rng.choice(allowed, size=rows[0].size)]
    for r in hubs:
        rows.append(np.full(HUB, r))
        cols.append(rng.choice(allowed, size=HUB, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(rows.size).astype(np.float32)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    if sym:
        A = (A + A.T).tocsr()
        assert abs(A - A.T).nnz == 0
    if kind == "unit":
        A.data[:] = 1.0
    assert A[::7].nnz == 0 and (kind != "unit" or A[BAND[0]:BAND[1]].nnz == 0)
    lens = np.diff(A.indptr)
    assert all(lens[r] >= HUB for r in hubs)
    return A


@pytest.fixture(scope="module")
def row_layers():
    """Eight layers of the row-kernel family: directed weighted, symmetric, unit directed with
    the empty band, and again; each layer's hub rows are one of rows 3..11 and one of the last 8
    (never a 7th row, which stays empty; the last layer shares row n - 1 with the first)."""
    kinds = ["dw", "sym", "unit", "dw", "sym", "unit", "dw", "sym"]
    near = [3, 4, 5, 6, 8, 9, 10, 11]
    last = [N_ROWS - 1 - j for j in (0, 1, 2, 3, 5, 6, 7, 0)]
    hubs = list(zip(near, last))
    for h in hubs:
        assert all(r % 7 for r in h) and h[1] >= N_ROWS - 8, h
    layers = [_rows_layer(100 + k, kinds[k], hubs[k]) for k in range(8)]
    assert max(sum(np.diff(A.indptr) for A in layers)) <= 5000
    return layers


def _mean_layer(seed, mean, unit, n=N_ROWS):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 2 * mean + 1, size=n)
    rows = np.repeat(np.arange(n), deg)
    A = sp.csr_matrix((rng.standard_normal(rows.size).astype(np.float32),
                       (rows, rng.integers(0, n, size=rows.size))), shape=(n, n))
    A.sum_duplicates()
    if unit:
        A.data[:] = 1.0
    return A


def _er_layer(seed, kind, hubs, n=N_TILE, deg=12):
    """ER-like layer of mean degree 12 with 700-entry hub rows and rows 1000..1099 empty."""
    rng = np.random.default_rng(seed)
    sym = kind == "sym"
    m = n * deg // (2 if sym else 1)
    rows = [rng.integers(0, n, size=m)]
    cols = [rng.integers(0, n, size=m)]
    for r in hubs:
        rows.append(np.full(HUB, r))
        cols.append(rng.choice(n, size=HUB, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    keep = ~_in_band(rows)
    if sym:  # (its band rows are empty only if no entry names them as a column)
        keep &= ~_in_band(cols)
    rows, cols = rows[keep], cols[keep]
    A = sp.csr_matrix((rng.uniform(0.5, 2.0, rows.size).astype(np.float32), (rows, cols)),
                      shape=(n, n))
    A.sum_duplicates()
    if sym:
        A = (A + A.T).tocsr()
    if kind == "unit":
        A.data[:] = 1.0
    assert A[BAND[0]:BAND[1]].nnz == 0
    return A


@pytest.fixture(scope="module")
def tile_layers():
    """Eight layers of the tiled family; the first three (directed weighted, symmetric, unit
    directed) carry the hub rows, so a row's total over all eight stays under 5,000 entries."""
    hubs = (0, 77, 20_000, N_TILE - 1)
    kinds = ["dw", "sym", "unit", "dw", "sym", "unit", "dw", "sym"]
    layers = [_er_layer(300 + k, kinds[k], hubs if k < 3 else ()) for k in range(8)]
    assert max(sum(np.diff(A.indptr) for A in layers)) <= 5000
    return layers


@pytest.fixture(scope="module")
def dense_layers():
    rng = np.random.default_rng(41)
    a, b, s = (rng.standard_normal((N_DENSE, N_DENSE)).astype(np.float32) for _ in range(3))
    return [a, b, s + s.T]


def _panel(n, b, seed=0):
    return np.random.default_rng(1000 * b + seed).standard_normal((n, b)).astype(np.float32)


# ----------------------------------------------------------------------------- the check
_STAGE1 = {}   # (family, k, b) -> (A_k^T X, |A_k^T| |X|) in fp64, computed once
_FRAC = {}     # group -> [largest fraction of the bar in Z, in W]


def _f64(A):
    return A.astype(np.float64)


def _stage1_ref(family, k, A, X):
    key = (family, k, X.shape[1])
    if key not in _STAGE1:
        A64, X64 = _f64(A), X.astype(np.float64)
        ref, scale = A64.T @ X64, abs(A64).T @ np.abs(X64)
        ref.setflags(write=False)
        scale.setflags(write=False)
        _STAGE1[key] = (ref, scale)
    return _STAGE1[key]


def _check(group, family, layers, X, W, Z, dense=False):
    """Both stages against fp64; returns the largest fractions of the bars reached."""
    assert W.dtype == np.float32 and Z.dtype == np.float32
    assert Z.shape == (len(layers), X.shape[0], X.shape[1]) and W.shape == X.shape
    assert not np.isnan(Z).any(), (group, "NaN in Z: rows", np.flatnonzero(np.isnan(Z).any((0, 2))))
    assert not np.isnan(W).any(), (group, "NaN in W: rows", np.flatnonzero(np.isnan(W).any(1)))
    fz = 0.0
    for k, A in enumerate(layers):
        ref, scale = _stage1_ref(family, k, A, X)
        q = np.abs(Z[k] - ref) / _bar(scale, dense)
        fz = max(fz, float(q.max()))
    Zg = Z.astype(np.float64)
    ref = sum(_f64(A) @ Zg[k] for k, A in enumerate(layers))
    scale = sum(abs(_f64(A)) @ np.abs(Zg[k]) for k, A in enumerate(layers))
    q = np.abs(W - ref) / _bar(scale, dense)
    fw = float(q.max())
    f = _FRAC.setdefault(group, [0.0, 0.0])
    f[0], f[1] = max(f[0], fz), max(f[1], fw)
    print(f"gram_apply {group}: fraction of the bar Z {fz:.3f} W {fw:.3f}"
          f" (group so far Z {f[0]:.3f} W {f[1]:.3f})")
    assert fz <= 1.0, (group, "stage 1", fz)
    assert fw <= 1.0, (group, "stage 2", fw, "row", int(q.max(1).argmax()))
    return fz, fw


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _apply_twice(eng, X):
    W, Z, info = eng.gram_apply(X)
    W2, Z2, info2 = eng.gram_apply(X)
    assert _same_bits(W, W2) and _same_bits(Z, Z2), "second call differs"
    assert info == info2
    print("gram_apply info", info)
    return W, Z, info


# n2v2r_spmm_tile_rows at n = 40,003 on the MI355X's 256 CUs (two workgroups per CU, one round:
# ceil(40,003 / 512) = 79 rows, rounded up to whole windows): window bits -> rows per tile, i.e.
# 3, 2 and 1 windows per tile; 40,003 is a multiple of neither, so the last tile is partial
TILE_ROWS = {5: 96, 6: 128, 7: 128}


# ----------------------------------------------------------------------------- CSR row kernels
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_row_kernels_b8(engine, monkeypatch, row_layers, K, split):
    """b = 8: all K layers in one stage-1 launch, stage 2 summing the layers in one accumulator
    (form 0) or XCD-split into per-layer partials and summed (form 1; split_slot at K = 5, 8)."""
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    monkeypatch.setenv("N2V2R_SPMM_SPLIT", str(split))
    layers = row_layers[:K]
    engine.set_layers(layers)
    X = _panel(N_ROWS, 8)
    W, Z, info = _apply_twice(engine, X)
    want = 1 if split and K >= 2 else 0
    assert (info["form"], info["split2"], info["rs_form"]) == (want, want, 0), info
    assert info["rpw1"] in (1, 2, 4, 8) and info["rpw2"] in (1, 2, 4, 8), info
    _check(f"rows b8 {'split' if want else 'sum'}", "rows", layers, X, W, Z)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("b", [16, 32, 64])
def test_row_kernels_wide(engine, monkeypatch, row_layers, K, b):
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    layers = row_layers[:K]
    engine.set_layers(layers)
    X = _panel(N_ROWS, b)
    W, Z, info = _apply_twice(engine, X)
    assert (info["form"], info["split2"], info["rs_form"]) == (0, 0, 0), info
    assert info["rpw1"] >= 1 and info["rpw2"] >= 1 and info["tile_rows"] == 0, info
    _check(f"rows b{b}", "rows", layers, X, W, Z)


# mean row length -> rows per wave at b = 8 (auto_rpw: a row group of 64 / rpw lanes while
# 64 / (2 rpw) >= 2 mean / 3.5, i.e. 8 up to a mean of 14, 4 up to 28, 2 up to 56, then 1, where
# spmm_csr_panel_kernel<8, 1> runs instead of the pipelined kernel).  A retuned rule fails here
# and names the kernel that lost its case.
RPW_BY_MEAN = [(5, 8), (10, 8), (20, 4), (45, 2), (70, 1)]


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("mean,rpw", RPW_BY_MEAN)
def test_row_kernels_b8_rows_per_wave(engine, monkeypatch, mean, rpw, split):
    monkeypatch.setenv("N2V2R_SPMM_CB", "0")
    monkeypatch.setenv("N2V2R_SPMM_SPLIT", str(split))
    layers = [_mean_layer(7 * mean, mean, False), _mean_layer(7 * mean + 1, mean, True)]
    engine.set_layers(layers)
    X = _panel(N_ROWS, 8, seed=mean)
    W, Z, info = _apply_twice(engine, X)
    assert (info["rpw1"], info["rpw2"]) == (rpw, rpw), (mean, info)
    assert info["form"] == split, info
    _check(f"rows b8 rpw {rpw}", f"mean{mean}", layers, X, W, Z)


# ----------------------------------------------------------------------------- tiled form
def _tiled_case(engine, monkeypatch, layers, nb, wbits, vw=None):
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    for name, v in (("N2V2R_SPMM_TILE_NB", nb), ("N2V2R_SPMM_WBITS", wbits),
                    ("N2V2R_SPMM_VW", vw)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    X = _panel(N_TILE, 8)
    W, Z, info = _apply_twice(engine, X)
    wb = 6 if wbits is None else wbits
    assert info["form"] == 5 and info["tile_wb"] == wb and (info["rpw1"], info["rpw2"]) == (0, 0)
    assert info["tile_nb"] == (4 if nb is None else nb), info   # 1.28 MB of panel: 4 blocks
    assert info["tile_rows"] == TILE_ROWS[wb], info
    assert N_TILE % info["tile_rows"] != 0                      # a partial last tile
    return X, W, Z, info


TILED_CROSS = [(None, None), (None, 5), (None, 6), (None, 7), (4, 6), (64, 6)]


@pytest.mark.parametrize("nb,wbits", TILED_CROSS)
def test_tiled_k3(engine, monkeypatch, tile_layers, nb, wbits):
    """spmm8_flat_kernel with K = 3: stage 1 writing each layer after its phases, stage 2 carrying
    the LDS accumulators across the layers and writing once."""
    layers = tile_layers[:3]
    engine.set_layers(layers)
    X, W, Z, info = _tiled_case(engine, monkeypatch, layers, nb, wbits)
    _check("tiled K3", "tile", layers, X, W, Z)


def test_tiled_k3_register_windows_bit_identical(engine, monkeypatch, tile_layers):
    """The register-window form (N2V2R_SPMM_VW=2) against the LDS-only one (=0) at K = 3: the
    register accumulators live across the layers in sum mode."""
    layers = tile_layers[:3]
    engine.set_layers(layers)
    X, W0, Z0, _ = _tiled_case(engine, monkeypatch, layers, None, 6, vw=0)
    X, W2, Z2, _ = _tiled_case(engine, monkeypatch, layers, None, 6, vw=2)
    _check("tiled K3 register windows", "tile", layers, X, W2, Z2)
    assert _same_bits(Z0, Z2) and _same_bits(W0, W2)


@pytest.mark.parametrize("K", [1, 8])
def test_tiled_k1_k8(engine, monkeypatch, tile_layers, K):
    layers = tile_layers[:K]
    engine.set_layers(layers)
    X, W, Z, info = _tiled_case(engine, monkeypatch, layers, None, None)
    _check(f"tiled K{K}", "tile", layers, X, W, Z)


# ----------------------------------------------------------------------------- dense layers
@pytest.mark.parametrize("tn", [1, 0])
@pytest.mark.parametrize("b", [8, 32, 64])
def test_dense_k3(engine, monkeypatch, dense_layers, b, tn):
    """apply_M_dense: beta = 1 accumulation over the layers, the B-streaming (TN) and the
    LDS-staged GEMM."""
    monkeypatch.setenv("N2V2R_DENSE_TN", str(tn))
    engine.set_layers(dense_layers, storage="dense", symmetric=-1)
    X = _panel(N_DENSE, b)
    W, Z, info = _apply_twice(engine, X)
    assert info["form"] == 4 and (info["rpw1"], info["rpw2"], info["tile_rows"]) == (0, 0, 0), info
    _check(f"dense {'tn' if tn else 'lds'}", "dense", dense_layers, X, W, Z, dense=True)


def test_dense_k1(engine, dense_layers):
    layers = dense_layers[:1]
    engine.set_layers(layers, storage="dense", symmetric=-1)
    X = _panel(N_DENSE, 32)
    W, Z, info = _apply_twice(engine, X)
    assert info["form"] == 4, info
    _check("dense K1", "dense", layers, X, W, Z, dense=True)


# ----------------------------------------------------------------------------- row partition
def _ranks_apply(world, layers, X, **set_kw):
    def fn(eng, r):
        eng.set_layers(layers, **set_kw)
        return (eng.dist_info(),) + _apply_twice(eng, X)
    res = _run_ranks(world, fn)
    assert [r[0][2] for r in res] == [min(X.shape[0], g * -(-X.shape[0] // world))
                                      for g in range(world)]
    W = np.concatenate([r[1] for r in res], axis=0)
    Z = np.concatenate([r[2] for r in res], axis=1)
    return W, Z, [r[3] for r in res]


def _dist_env(monkeypatch, stage2, chunks=None, cb=0):
    monkeypatch.setenv("N2V2R_DIST_STAGE2", stage2)
    monkeypatch.setenv("N2V2R_SPMM_CB", str(cb))
    if chunks is None:
        monkeypatch.delenv("N2V2R_RS_CHUNKS", raising=False)
    else:
        monkeypatch.setenv("N2V2R_RS_CHUNKS", str(chunks))


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_gather(monkeypatch, row_layers, world):
    _dist_env(monkeypatch, "gather")
    layers, X = row_layers[:3], _panel(N_ROWS, 8)
    W, Z, infos = _ranks_apply(world, layers, X)
    for info in infos:
        assert (info["form"], info["rs_form"], info["split2"]) == (0, 0, 0), info
        assert info["rpw1"] >= 1 and info["rpw2"] >= 1, info
    _check("partition gather", "rows", layers, X, W, Z)


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rs_chunks_bit_identical(monkeypatch, row_layers, world):
    """stage2_rs: the column share's product in one launch, and in 4 row chunks over pointer-
    shifted row ranges with the whole share's rows per wave: the same bits."""
    layers, X = row_layers[:3], _panel(N_ROWS, 8)
    out = {}
    for chunks in (1, 4):
        _dist_env(monkeypatch, "rs", chunks)
        W, Z, infos = _ranks_apply(world, layers, X)
        for info in infos:
            assert (info["form"], info["rs_form"], info["rs_chunks"]) == (0, 1, chunks), info
            assert info["rpw1"] >= 1 and info["rpw2"] >= 1, info
        _check("partition rs", "rows", layers, X, W, Z)
        out[chunks] = (W, Z)
    assert _same_bits(out[1][1], out[4][1]), "Z differs between 1 and 4 chunks"
    assert _same_bits(out[1][0], out[4][0]), "W differs between 1 and 4 chunks"


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_rs_tiled_stage1(monkeypatch, row_layers, world):
    """Stage 1 tiled on the rank's rows (column blocks over the gathered panel), stage 2 the
    reduce-scatter form."""
    _dist_env(monkeypatch, "rs", cb=1)
    layers, X = row_layers[:3], _panel(N_ROWS, 8)
    W, Z, infos = _ranks_apply(world, layers, X)
    for info in infos:
        assert (info["form"], info["rs_form"]) == (5, 1) and info["rpw1"] == 0, info
        assert info["tile_rows"] > 0 and info["rpw2"] >= 1, info
    _check("partition rs tiled stage 1", "rows", layers, X, W, Z)


def test_partitioned_gather_b32(monkeypatch, row_layers):
    _dist_env(monkeypatch, "gather")
    layers, X = row_layers[:3], _panel(N_ROWS, 32)
    W, Z, infos = _ranks_apply(2, layers, X)
    assert all((i["form"], i["rs_form"]) == (0, 0) for i in infos), infos
    _check("partition gather b32", "rows", layers, X, W, Z)


def test_partitioned_dense(dense_layers):
    X = _panel(N_DENSE, 32)
    W, Z, infos = _ranks_apply(2, dense_layers, X, storage="dense", symmetric=-1)
    assert all((i["form"], i["rs_form"]) == (4, 0) for i in infos), infos
    _check("partition dense", "dense", dense_layers, X, W, Z, dense=True)


@pytest.mark.parametrize("stage2", ["rs", "gather"])
def test_rccl_world1(monkeypatch, row_layers, stage2):
    """The same application with every collective through RCCL at world size 1."""
    from node2vec2rank_amd import _lib
    _dist_env(monkeypatch, stage2)
    layers, X = row_layers[:3], _panel(N_ROWS, 8)
    eng = _lib.Engine.rccl(0, 0, 1, _lib.comm_unique_id())
    try:
        eng.set_layers(layers)
        W, Z, info = _apply_twice(eng, X)
    finally:
        eng.close()
    assert (info["form"], info["rs_form"]) == (0, int(stage2 == "rs")), info
    _check(f"rccl world 1 {stage2}", "rows", layers, X, W, Z)


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
    X = _panel(layers[0].shape[0], 8)
    W, Z, info = _apply_twice(engine, X)
    _check("er_cfg1", "er_cfg1", layers, X, W, Z)
    after = (engine.singular_values(), engine.embedding(), engine.left_embedding())
    again = fit()
    for a, b, c in zip(ref, after, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bad_arguments(engine, row_layers):
    engine.set_layers(row_layers[:1])
    with pytest.raises(ValueError):
        engine.gram_apply(_panel(N_ROWS, 8)[:, :4])  # b = 4
    with pytest.raises(ValueError):
        engine.gram_apply(np.zeros((N_ROWS, 24), np.float32))
    # a multi-GPU parent handle: the call belongs to its ranks
    from node2vec2rank_amd import _lib
    eng = _lib.Engine.multi([0, 0])
    try:
        eng.set_layers(row_layers[:1])
        with pytest.raises(ValueError):
            eng.gram_apply(_panel(N_ROWS, 8))
    finally:
        eng.close()
