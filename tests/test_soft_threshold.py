"""The host half of the soft-threshold scan (node2vec2rank_amd/soft_threshold.py): the scale-free
fit, the choice of the power and the argument checks.  No GPU: where a test goes through
``pick_soft_threshold`` the engine is a numpy stand-in.

``scale_free_fit`` is checked against a restatement that shares no code with it: ``pd.cut`` for
the bins (R's ``cut(k, nBreaks)``: equal-width right-closed bins, the outer edges moved out by
0.1 % of the range so the minimum lands in the first bin), ``np.polyfit`` for the line and the
normal equations for the three-regressor fit.  Both sides are fp64 evaluations of the same
formulas on at most 10 points, so they must agree to 1e-9."""
import math

import numpy as np
import pandas as pd
import pytest

from node2vec2rank_amd import Coexpression, pick_soft_threshold, scale_free_fit
from node2vec2rank_amd import soft_threshold as sth


def _restated_fit(k, nb):
    k = np.asarray(k, dtype=np.float64)
    codes = pd.cut(k, nb).codes
    edges = np.linspace(k.min(), k.max(), nb + 1)
    dk, p = np.empty(nb), np.empty(nb)
    for b in range(nb):
        inside = k[codes == b]
        mid = (edges[b] + edges[b + 1]) / 2
        dk[b] = inside.mean() if inside.size and inside.mean() != 0 else mid
        p[b] = inside.size / k.size
    x, y = np.log10(dk), np.log10(p + 1e-9)
    slope, icpt = np.polyfit(x, y, 1)
    tot = ((y - y.mean()) ** 2).sum()
    r2 = 1.0 - ((y - (slope * x + icpt)) ** 2).sum() / tot
    X = np.column_stack([np.ones(nb), x, dk])
    beta = np.linalg.solve(X.T @ X, X.T @ y)
    r2t = 1.0 - ((y - X @ beta) ** 2).sum() / tot
    return r2, slope, 1.0 - (1.0 - r2t) * (nb - 1) / (nb - 3)


def _pareto(n=20000, seed=0):
    # density ~ k^-2.5 on [3, 30] (a Pareto law cut at ten times its minimum, by inverse CDF), so
    # that every one of the equal-width bins is populated: an empty bin enters the fit as
    # log10(1e-9) and an untruncated tail is mostly empty bins
    u = np.random.default_rng(seed).uniform(0.0, 1.0, n)
    a, lo, hi = 1.5, 3.0, 30.0
    return lo * (1.0 - u * (1.0 - (lo / hi) ** a)) ** (-1.0 / a)


def _uniform(n=3000, seed=1):
    return np.random.default_rng(seed).uniform(2.0, 50.0, n)


def _gapped(seed=2):
    rng = np.random.default_rng(seed)  # two groups far apart: the bins between them are empty
    return np.concatenate([rng.uniform(1.0, 2.0, 500), rng.uniform(9.0, 10.0, 40)])


@pytest.mark.parametrize("make", [_pareto, _uniform, _gapped])
@pytest.mark.parametrize("nb", [10, 7])
def test_scale_free_fit_matches_restatement(make, nb):
    k = make()
    got, ref = scale_free_fit(k, nb), _restated_fit(k, nb)
    print(make.__name__, nb, got, ref)
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-9 * max(1.0, abs(r)), (got, ref)


def test_inputs_are_what_they_claim():
    """The empty-bin input does have empty bins, the others none."""
    for make, empty in ((_pareto, False), (_uniform, False), (_gapped, True)):
        codes = pd.cut(make(), 10).codes
        assert (np.bincount(codes, minlength=10) == 0).any() == empty


def test_pareto_is_scale_free_and_uniform_is_not():
    r2, slope, _ = scale_free_fit(_pareto())
    assert slope < 0 and r2 > 0.85, (r2, slope)
    r2u, _, _ = scale_free_fit(_uniform())
    assert r2u < 0.5, r2u


def test_constant_connectivity_is_nan_and_never_the_estimate():
    assert all(math.isnan(v) for v in scale_free_fit(np.full(50, 3.25)))
    conn = np.vstack([np.full(20000, 7.0), _pareto()])
    table = sth.fit_table([1.0, 2.0], conn)
    assert list(table.columns) == sth.COLUMNS
    assert table.loc[0, ["SFT.R.sq", "slope", "truncated.R.sq"]].isna().all()
    assert table.loc[0, "mean.k."] == 7.0 and table.loc[0, "max.k."] == 7.0
    assert sth.power_estimate(table, 0.0) == 2.0
    assert sth.power_estimate(table.iloc[:1], 0.0) is None


def _table(r2, slope):
    n = len(r2)
    return pd.DataFrame({"Power": np.arange(1.0, n + 1), "SFT.R.sq": r2, "slope": slope,
                         "truncated.R.sq": r2, "mean.k.": 1.0, "median.k.": 1.0, "max.k.": 2.0})


def test_power_estimate_selection():
    # the lowest power above the cut
    assert sth.power_estimate(_table([0.2, 0.86, 0.9, 0.99], [-1, -1, -2, -2]), 0.85) == 2.0
    # a positive slope makes the signed fit negative: power 2 does not qualify
    assert sth.power_estimate(_table([0.2, 0.95, 0.9, 0.99], [-1, 0.5, -2, -2]), 0.85) == 3.0
    # the cut itself is not exceeded
    assert sth.power_estimate(_table([0.85, 0.85], [-1, -1]), 0.85) is None
    # nothing qualifies
    assert sth.power_estimate(_table([0.2, 0.5, 0.84], [-1, -1, -1]), 0.85) is None
    assert sth.power_estimate(_table([0.99, 0.99], [1, 2]), 0.85) is None
    # another cut
    assert sth.power_estimate(_table([0.2, 0.5, 0.84], [-1, -1, -1]), 0.4) == 2.0


class _NumpyEngine:
    """Stands in for Engine.soft_connectivity with the formula itself (a small n x n array)."""

    def __init__(self):
        self.calls = []

    def soft_connectivity(self, E, kind="unsigned", powers=(6.0,)):
        self.calls.append((kind, tuple(powers)))
        r = np.clip(np.corrcoef(E), -1.0, 1.0)
        t = {"unsigned": np.abs(r), "signed": (1 + r) / 2, "signed hybrid": np.maximum(r, 0)}[kind]
        np.fill_diagonal(t, 0.0)
        return np.stack([(t ** p).sum(axis=1) for p in powers])


class _NoEngine:
    def soft_connectivity(self, *a, **k):
        raise AssertionError("the engine was reached: the check came too late")


def _expr(n=60, s=12, seed=3):
    return np.random.default_rng(seed).standard_normal((n, s))


def test_pick_soft_threshold_through_a_stand_in_engine():
    eng = _NumpyEngine()
    E = _expr()
    res = pick_soft_threshold(E, kind="signed", engine=eng)
    assert eng.calls == [("signed", sth.DEFAULT_POWERS)]
    assert sth.DEFAULT_POWERS == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20)
    assert res.connectivity.shape == (15, 60) and res.connectivity.dtype == np.float64
    assert list(res.table.columns) == sth.COLUMNS and len(res.table) == 15
    assert np.array_equal(res.table["Power"].to_numpy(), np.array(sth.DEFAULT_POWERS))
    assert np.array_equal(res.table["mean.k."].to_numpy(), res.connectivity.mean(axis=1))
    assert np.array_equal(res.table["median.k."].to_numpy(), np.median(res.connectivity, axis=1))
    assert np.array_equal(res.table["max.k."].to_numpy(), res.connectivity.max(axis=1))
    for q in range(15):
        fit = scale_free_fit(res.connectivity[q])
        assert np.array_equal(res.table.iloc[q, 1:4].to_numpy(dtype=np.float64), np.array(fit),
                              equal_nan=True)
    assert res.power_estimate == sth.power_estimate(res.table, 0.85)
    # a Coexpression's own kind wins, a DataFrame is taken as Coexpression takes it
    eng = _NumpyEngine()
    pick_soft_threshold(Coexpression(E, kind="signed hybrid", power=6), kind="unsigned",
                        powers=[2, 2.5], engine=eng)
    pick_soft_threshold(pd.DataFrame(E), powers=[3], engine=eng)
    assert eng.calls == [("signed hybrid", (2.0, 2.5)), ("unsigned", (3.0,))]


@pytest.mark.parametrize("kwargs, word", [
    (dict(expression=np.zeros(5)), "2-D"),
    (dict(expression=np.zeros((5, 1))), "2 samples"),
    (dict(expression="genes"), "expression"),
    (dict(kind="pearson"), "kind"),
    (dict(kind=3), "kind"),
    (dict(kind="raw"), "raw"),
    (dict(expression=Coexpression(_expr(), kind="raw")), "raw"),
    (dict(powers=[]), "powers"),
    (dict(powers=list(range(1, 34))), "33"),
    (dict(powers=[1, 0.5]), ">= 1"),
    (dict(powers=[1, math.nan]), "finite"),
    (dict(powers=[1, math.inf]), "finite"),
    (dict(powers=["six"]), "powers"),
    (dict(r2_cut="high"), "r2_cut"),
    (dict(r2_cut=1.5), "r2_cut"),
    (dict(r2_cut=math.nan), "r2_cut"),
    (dict(n_breaks=1), "n_breaks"),
    (dict(n_breaks=2.5), "n_breaks"),
    (dict(n_breaks=True), "n_breaks"),
])
def test_pick_soft_threshold_value_errors(kwargs, word):
    args = dict(expression=_expr(), engine=_NoEngine())
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        pick_soft_threshold(**args)


def test_scale_free_fit_value_errors():
    with pytest.raises(ValueError):
        scale_free_fit(_pareto(), 1)
    with pytest.raises(ValueError):
        scale_free_fit([])
    with pytest.raises(ValueError):
        scale_free_fit([1.0, math.nan, 2.0])
