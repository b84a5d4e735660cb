"""The soft-threshold scan on the GPU (n2v2r_soft_connectivity, csrc/soft_threshold.hip) against
an extended-precision host reference.

Reference: ``np.longdouble`` on the host, the same chain as the kernel's: standardise the rows
(mean, centre, divide by the centred 2-norm), r = clip(Z Z^T, -1, 1), the kind's map, the power,
the row sum with the diagonal excluded.

Bound per entry of k (derived, not tuned):

    |k - ref| <= 2^-53 (n (2 p (samples + 10) + 4) + n |ref|)

An r entry of the fp64 product differs from the exact one by about (samples + 10) 2^-53 (the
standardisation's and the dot product's roundings); pow passes on at most p times that (t <= 1,
d t^p / dt = p t^(p-1) <= p) plus its own rounding, doubled for slack, plus 4 for the clip and the
kind's map; the sum adds at most n roundings of its running value, which is <= |ref|.  numpy's own
fp64 evaluation of the chain has to sit at <= 0.03 of the bound (asserted below), which shows
that the bound does not rest on the code under test; an entry dropped or counted twice at p = 1
is about 1e7 bounds.  Observed on an MI355X: numpy's fp64 at most 0.026 of the bound, the kernel
at most 0.025 over the 48 cases of test_connectivity_matches_longdouble.

Inputs: rows that mix four latent factors plus noise, on per-row scales 10^U(-3, 3) with offsets,
so the correlations spread over [-1, 1] and high powers do not vanish.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one exact tile and ragged tiles; samples below, above and not a multiple of the 16-wide k round;
# n = 257 walks five tiles per workgroup
SHAPES = [(64, 3), (193, 7), (130, 37), (257, 200)]
KINDS = ["unsigned", "signed", "signed hybrid"]
DEFAULT = tuple(float(p) for p in (*range(1, 11), *range(12, 21, 2)))
POWERS = {"default15": DEFAULT, "one": (1.0,), "2.5": (2.5,),
          "32": tuple(float(p) for p in np.linspace(1.0, 20.0, 32))}


def _expression(n, s, seed):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((n, 4)) @ rng.standard_normal((4, s))
    x = mix + 0.5 * rng.standard_normal((n, s))
    scale = 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    return np.ascontiguousarray(x * scale + rng.uniform(-5, 5, size=(n, 1)) * scale)


_E, _R, _K = {}, {}, {}


def _expr(n, s):
    if (n, s) not in _E:
        e = _expression(n, s, seed=7000 * n + s)
        e.setflags(write=False)
        _E[(n, s)] = e
    return _E[(n, s)]


def _corr(n, s, dtype):
    """clip(Z Z^T, -1, 1) of the standardised rows, in ``dtype``; computed once per shape."""
    if (n, s, dtype) not in _R:
        e = _expr(n, s).astype(dtype)
        c = e - e.mean(axis=1, keepdims=True)
        z = c / np.sqrt((c * c).sum(axis=1, keepdims=True))
        r = np.clip(z @ z.T, dtype(-1), dtype(1))
        r.setflags(write=False)
        _R[(n, s, dtype)] = r
    return _R[(n, s, dtype)]


def _connectivity(n, s, kind, powers, dtype=np.longdouble):
    key = (n, s, kind, powers, dtype)
    if key not in _K:
        r = _corr(n, s, dtype)
        one, half = dtype(1), dtype(0.5)
        t = {"unsigned": np.abs(r), "signed": (one + r) * half,
             "signed hybrid": np.maximum(r, dtype(0))}[kind]
        off = ~np.eye(n, dtype=bool)
        k = np.stack([np.where(off, t ** dtype(p), dtype(0)).sum(axis=1) for p in powers])
        k.setflags(write=False)
        _K[key] = k
    return _K[key]


def _bound(n, s, powers, ref):
    p = np.asarray(powers, dtype=np.float64)[:, None]
    return 2.0 ** -53 * (n * (2.0 * p * (s + 10) + 4.0) + n * np.abs(ref.astype(np.float64)))


def _ratio(k, n, s, powers, ref):
    err = np.abs(k.astype(np.longdouble) - ref).astype(np.float64)
    return float((err / _bound(n, s, powers, ref)).max())


@pytest.mark.parametrize("pname", list(POWERS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n, s", SHAPES)
def test_connectivity_matches_longdouble(engine, n, s, kind, pname):
    powers = POWERS[pname]
    ref = _connectivity(n, s, kind, powers)
    k = engine.soft_connectivity(_expr(n, s), kind=kind, powers=powers)
    assert k.dtype == np.float64 and k.shape == (len(powers), n)
    worst = _ratio(k, n, s, powers, ref)
    print(f"n={n} s={s} {kind} {pname}: max |k - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n, s", SHAPES)
def test_bound_does_not_rest_on_the_code_under_test(n, s, kind):
    """numpy's fp64 evaluation of the chain (no GPU involved) sits at <= 0.03 of the bound."""
    ref = _connectivity(n, s, kind, DEFAULT)
    host = _connectivity(n, s, kind, DEFAULT, dtype=np.float64)
    worst = _ratio(host, n, s, DEFAULT, ref)
    print(f"n={n} s={s} {kind}: numpy fp64 max |k - ref| / bound = {worst:.4f}")
    assert worst <= 0.03, worst


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_counts(engine, kind):
    """Every chunk count is within the bound, and a count's result is reproducible bit for bit."""
    n, s = 257, 200
    ref = _connectivity(n, s, kind, DEFAULT)
    for chunks in (1, 2, 5):
        k, used, ms = engine.soft_connectivity_chunks(_expr(n, s), kind=kind, powers=DEFAULT,
                                                      chunks=chunks)
        assert used == chunks and ms > 0.0
        worst = _ratio(k, n, s, DEFAULT, ref)
        print(f"{kind} chunks={chunks}: max |k - ref| / bound = {worst:.4f}, kernel {ms:.3f} ms")
        assert worst <= 1.0, (chunks, worst)
        again, _, _ = engine.soft_connectivity_chunks(_expr(n, s), kind=kind, powers=DEFAULT,
                                                      chunks=chunks)
        assert np.array_equal(k, again), chunks
    auto, used, _ = engine.soft_connectivity_chunks(_expr(n, s), kind=kind, powers=DEFAULT)
    assert 1 <= used <= 5
    assert np.array_equal(auto, engine.soft_connectivity(_expr(n, s), kind=kind, powers=DEFAULT))
    with pytest.raises(ValueError, match="chunks"):
        engine.soft_connectivity_chunks(_expr(n, s), kind=kind, powers=DEFAULT, chunks=6)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n, s", [(193, 7), (257, 200)])
def test_scan_describes_the_layer_the_build_produces(engine, n, s, kind):
    """k(p) against the row sums of the fp32 layer Coexpression(E, kind, power=p) builds: one fp32
    rounding per entry, each entry <= 1, so at most n 2^-24 apart (the diagonal, exactly 1, taken
    off)."""
    from node2vec2rank_amd import Coexpression
    k = engine.soft_connectivity(_expr(n, s), kind=kind, powers=[1.0, 6.0])
    for q, p in enumerate((1.0, 6.0)):
        engine.set_layers([Coexpression(_expr(n, s), kind=kind, power=p)])
        rows = engine.layer_dense(0).astype(np.float64).sum(axis=1) - 1.0
        worst = float(np.abs(rows - k[q]).max())
        print(f"n={n} {kind} p={p:g}: max |layer row sum - k| = {worst:.3e}, "
              f"allowed {n * 2.0 ** -24:.3e}")
        assert worst <= n * 2.0 ** -24, (p, worst)


def test_the_handle_is_left_alone(engine):
    from node2vec2rank_amd import Coexpression
    n, s = 130, 37
    engine.set_layers([Coexpression(_expr(n, s), kind="signed", power=6),
                       Coexpression(_expr(n, s)[:, ::-1].copy(), kind="unsigned")])
    before = [engine.layer_dense(0), engine.layer_dense(1)]
    storage = engine.storage
    engine.soft_connectivity(_expr(257, 200), kind="signed hybrid", powers=DEFAULT)
    engine.soft_connectivity(_expr(n, s), kind="unsigned", powers=[2.0])
    for a, b in zip(before, [engine.layer_dense(0), engine.layer_dense(1)]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert engine.storage == storage == "dense"


def _bad(kind):
    e = _expr(130, 37).copy()
    if kind == "constant":
        e[77] = 3.5
        e[101] = -1.0
    else:
        e[41, 5] = np.nan
        e[90, 0] = np.nan
    return e


@pytest.mark.parametrize("args, word", [
    (dict(E=_bad("constant")), "row 77 "),
    (dict(E=_bad("nan")), "row 41 "),
    (dict(powers=list(range(1, 34))), "33"),
    (dict(powers=[1.0, 0.5]), "0.5"),
    (dict(kind="raw"), "raw"),
    (dict(E=_expr(130, 37)[:, :1].copy()), "2 samples"),
], ids=["constant-row", "nan-row", "33-powers", "power-0.5", "raw", "one-sample"])
def test_errors_name_the_cause_and_leave_the_handle_usable(engine, args, word):
    call = dict(E=_expr(130, 37), kind="signed", powers=[1.0, 6.0])
    good = dict(call)
    call.update(args)
    with pytest.raises(ValueError, match=word):
        engine.soft_connectivity(call["E"], kind=call["kind"], powers=call["powers"])
    k = engine.soft_connectivity(good["E"], kind=good["kind"], powers=good["powers"])
    ref = _connectivity(130, 37, "signed", (1.0, 6.0))
    assert _ratio(k, 130, 37, (1.0, 6.0), ref) <= 1.0


def test_pick_soft_threshold_end_to_end(engine):
    """(No connectivity of this input lies on a bin edge other than the minimum and the maximum,
    which the binning places by rule: the fit is then a smooth function of k.)"""
    from node2vec2rank_amd import pick_soft_threshold, scale_free_fit
    n, s = 257, 200
    res = pick_soft_threshold(_expr(n, s), kind="unsigned", engine=engine)
    cols = ["Power", "SFT.R.sq", "slope", "truncated.R.sq", "mean.k.", "median.k.", "max.k."]
    assert list(res.table.columns) == cols and len(res.table) == 15
    assert res.connectivity.shape == (15, n)
    assert np.array_equal(res.table["Power"].to_numpy(), np.array(DEFAULT))
    assert np.array_equal(res.table["mean.k."].to_numpy(), res.connectivity.mean(axis=1))
    assert np.array_equal(res.table["median.k."].to_numpy(), np.median(res.connectivity, axis=1))
    assert np.array_equal(res.table["max.k."].to_numpy(), res.connectivity.max(axis=1))
    ref = _connectivity(n, s, "unsigned", DEFAULT).astype(np.float64)
    fits = np.array([scale_free_fit(k) for k in ref])
    got = res.table[["SFT.R.sq", "slope", "truncated.R.sq"]].to_numpy()
    print("max |table - fit of the reference| =", float(np.abs(got - fits).max()))
    assert np.all(np.abs(got - fits) <= 1e-9 * np.maximum(1.0, np.abs(fits)))
    signed = -np.sign(fits[:, 1]) * fits[:, 0]
    want = min((p for p, v in zip(DEFAULT, signed) if v > 0.85), default=None)
    assert res.power_estimate == want
