"""Choosing the soft-threshold power of a ``Coexpression`` layer: WGCNA's ``pickSoftThreshold``
(hdWGCNA's ``TestSoftPowers``) without an N x N array.

``pick_soft_threshold`` gets the connectivities ``k_i(p) = sum_{j != i} t(r_ij) ** p`` of every
gene for every candidate power from the GPU (``Engine.soft_connectivity``,
``n2v2r_soft_connectivity``: fp64, nothing N x N on the host or in HBM, the engine's loaded layers
untouched) and fits the scale-free topology model to each power's connectivities on the host
(``scale_free_fit``, numpy fp64).

R is not a dependency of this package and WGCNA was not run against it: ``scale_free_fit`` and
the choice of ``power_estimate`` restate the formulas of WGCNA's ``scaleFreeFitIndex`` and
``pickSoftThreshold`` (parity by formula, not by comparison of outputs).
"""
from __future__ import annotations

import math

import numpy as np

from .coexpression import Coexpression, method_name

# WGCNA's default powerVector, c(1:10, seq(12, 20, 2))
DEFAULT_POWERS = tuple(float(p) for p in (*range(1, 11), *range(12, 21, 2)))
MAX_POWERS = 32  # per call of n2v2r_soft_connectivity
COLUMNS = ["Power", "SFT.R.sq", "slope", "truncated.R.sq", "mean.k.", "median.k.", "max.k."]
SCAN_KINDS = ("unsigned", "signed", "signed hybrid")


def _r_squared(y, X):
    """(R^2, coefficients) of the least-squares fit of y on the columns of X (X holds the
    intercept column)."""
    beta = np.linalg.lstsq(X, y, rcond=None)[0]
    res = y - X @ beta
    tot = y - y.mean()
    return 1.0 - float(res @ res) / float(tot @ tot), beta


def scale_free_fit(k, n_breaks: int = 10):
    """WGCNA's ``scaleFreeFitIndex(k, nBreaks)``: ``(R^2, slope, truncated R^2)`` of the
    scale-free topology fit of the connectivities k, in fp64.

    k is cut into ``n_breaks`` equal-width, right-closed bins over [min k, max k] (the minimum
    falls into the first bin); ``dk`` is a bin's mean of k, or its midpoint where the bin is empty
    or the mean is 0; ``p`` is the bin's share of the genes.  R^2 and slope are those of the
    least-squares line of ``log10(p + 1e-9)`` on ``log10(dk)``; the truncated R^2 is the adjusted
    R^2 of the same fit with ``dk`` as a third regressor (NaN with fewer than 4 bins).  Where
    max k = min k there is no distribution to fit: all three are NaN."""
    k = np.asarray(k, dtype=np.float64).reshape(-1)
    nb = int(n_breaks)
    if nb < 2:
        raise ValueError(f"n_breaks must be at least 2, got {n_breaks!r}")
    if k.size == 0 or not np.all(np.isfinite(k)):
        raise ValueError("k must be a non-empty array of finite connectivities")
    lo, hi = float(k.min()), float(k.max())
    if not hi > lo:
        return math.nan, math.nan, math.nan
    edges = np.linspace(lo, hi, nb + 1)
    # right-closed: k in (edges[b], edges[b + 1]] -> b; the minimum itself -> bin 0
    which = np.clip(np.searchsorted(edges, k, side="left") - 1, 0, nb - 1)
    count = np.bincount(which, minlength=nb).astype(np.float64)
    total = np.bincount(which, weights=k, minlength=nb)
    mids = 0.5 * (edges[:-1] + edges[1:])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / count
    dk = np.where((count == 0) | (mean == 0), mids, mean)
    p = count / k.size
    x, y = np.log10(dk), np.log10(p + 1e-9)
    one = np.ones(nb)
    r2, beta = _r_squared(y, np.column_stack([one, x]))
    trunc = math.nan
    if nb > 3:
        r2t, _ = _r_squared(y, np.column_stack([one, x, dk]))
        trunc = 1.0 - (1.0 - r2t) * (nb - 1) / (nb - 3)
    return r2, float(beta[1]), trunc


def fit_table(powers, connectivity, n_breaks: int = 10):
    """``pickSoftThreshold``'s ``fitIndices`` table from the P x n connectivities of P powers: a
    DataFrame with WGCNA's columns ``Power, SFT.R.sq, slope, truncated.R.sq, mean.k., median.k.,
    max.k.`` (``SFT.R.sq`` is the unsigned R^2, as in WGCNA)."""
    import pandas as pd
    powers = np.asarray(powers, dtype=np.float64).reshape(-1)
    conn = np.asarray(connectivity, dtype=np.float64)
    if conn.ndim != 2 or conn.shape[0] != powers.size:
        raise ValueError(f"connectivity must be (len(powers), n), got {conn.shape}")
    rows = []
    for p, k in zip(powers, conn):
        r2, slope, trunc = scale_free_fit(k, n_breaks)
        rows.append([p, r2, slope, trunc, float(np.mean(k)), float(np.median(k)),
                     float(np.max(k))])
    return pd.DataFrame(rows, columns=COLUMNS)


def power_estimate(table, r2_cut: float = 0.85):
    """``pickSoftThreshold``'s ``powerEstimate``: the lowest ``Power`` of ``table`` whose signed fit
    ``-sign(slope) * SFT.R.sq`` exceeds ``r2_cut``, or ``None`` when no power does.  A row whose
    fit is NaN (constant connectivities) never qualifies."""
    power = np.asarray(table["Power"], dtype=np.float64)
    signed = -np.sign(np.asarray(table["slope"], dtype=np.float64)) * \
        np.asarray(table["SFT.R.sq"], dtype=np.float64)
    ok = signed > float(r2_cut)  # (NaN compares false)
    return float(power[ok].min()) if ok.any() else None


class SoftThreshold:
    """What ``pick_soft_threshold`` returns: ``.connectivity`` (P x n float64, row q the
    connectivities at ``.powers[q]``), ``.table`` (``fit_table``'s DataFrame) and
    ``.power_estimate`` (``power_estimate`` of the table: a float or ``None``); ``.kind`` and
    ``.method`` are those of the network scanned."""

    def __init__(self, kind, powers, connectivity, table, estimate, r2_cut, method="pearson"):
        self.kind = kind
        self.method = method
        self.powers = powers
        self.connectivity = connectivity
        self.table = table
        self.power_estimate = estimate
        self.r2_cut = r2_cut

    def __repr__(self):
        method = "" if self.method == "pearson" else f"method={self.method!r}, "
        return (f"SoftThreshold(kind={self.kind!r}, {method}powers={len(self.powers)}, "
                f"n={self.connectivity.shape[1]}, power_estimate={self.power_estimate!r})")


def _validate(expression, kind, powers, r2_cut, n_breaks, method="pearson"):
    if isinstance(expression, Coexpression):
        layer = expression  # (its own kind and method are the ones scanned)
    else:
        layer = Coexpression(expression, kind=kind, method=method_name(method))
    if layer.kind not in SCAN_KINDS:
        raise ValueError(f"a {layer.kind!r} layer takes no power (r may be negative): the kinds "
                         f"to scan are {list(SCAN_KINDS)}")
    if powers is None:
        powers = DEFAULT_POWERS
    try:
        pw = np.array(powers, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"powers must be a sequence of numbers, got {powers!r}") from None
    if not 1 <= pw.size <= MAX_POWERS:
        raise ValueError(f"between 1 and {MAX_POWERS} powers per scan, got {pw.size}")
    if not np.all(np.isfinite(pw)) or np.any(pw < 1.0):
        raise ValueError(f"every power must be finite and >= 1, got {pw.tolist()}")
    try:
        cut = float(r2_cut)
    except (TypeError, ValueError):
        raise ValueError(f"r2_cut must be a number, got {r2_cut!r}") from None
    if not math.isfinite(cut) or not 0.0 <= cut <= 1.0:
        raise ValueError(f"r2_cut must lie in [0, 1], got {r2_cut!r}")
    if isinstance(n_breaks, (bool, np.bool_)) or not isinstance(n_breaks, (int, np.integer)) \
            or n_breaks < 2:
        raise ValueError(f"n_breaks must be an integer >= 2, got {n_breaks!r}")
    return layer, pw, cut, int(n_breaks)


def pick_soft_threshold(expression, kind: str = "unsigned", powers=None, r2_cut: float = 0.85,
                        n_breaks: int = 10, engine=None, method: str = "pearson") -> SoftThreshold:
    """WGCNA's ``pickSoftThreshold`` for the rows of ``expression``.

    expression: ``n x samples`` (an array or a DataFrame, as ``Coexpression`` takes it), or a
        ``Coexpression``, whose own ``kind`` and ``method`` are used (its power and options play
        no part).
    kind: ``"unsigned"``, ``"signed"`` or ``"signed hybrid"``.
    powers: up to 32 candidate exponents, each >= 1; default WGCNA's ``c(1:10, seq(12, 20, 2))``.
    r2_cut: the signed scale-free fit a power must exceed to be the estimate.
    n_breaks: bins of the connectivity histogram (``scaleFreeFitIndex``'s ``nBreaks``).
    engine: the ``Engine`` to run on (default: the process-wide engine of device 0); its loaded
        layers and embedding are left alone.
    method: ``"pearson"``, ``"spearman"`` or ``"bicor"``, as ``Coexpression`` takes it.  A bicor
        scan in which rows have zero MAD warns (``RuntimeWarning``) as ``Engine.set_layers`` does.

    Every violation of the above is a ``ValueError`` before any GPU work; rows the correlation is
    undefined for (constant, non-finite) are a ``ValueError`` from the engine, by row index.

    The formulas are WGCNA's, restated (see the module docstring): parity is by formula."""
    layer, pw, cut, nb = _validate(expression, kind, powers, r2_cut, n_breaks, method)
    if engine is None:
        from ._lib import default_engine
        engine = default_engine()
    if layer.method == "pearson":  # (an engine that knows no method keyword still serves)
        conn = engine.soft_connectivity(layer.expression, kind=layer.kind, powers=pw)
    else:
        conn = engine.soft_connectivity(layer.expression, kind=layer.kind, powers=pw,
                                        method=layer.method)
    table = fit_table(pw, conn, nb)
    return SoftThreshold(layer.kind, pw, conn, table, power_estimate(table, cut), cut,
                         layer.method)
