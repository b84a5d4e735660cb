"""``Coexpression``: a graph layer given by its expression matrix instead of its N x N network.

The engine builds the dense co-expression layer on the GPU (``n2v2r_set_layer_corr``,
include/n2v2r.h), so the N x N correlation matrix never exists on the host.  Nothing here
touches the GPU: the class only holds and validates the caller's data.
"""
from __future__ import annotations

import math

import numpy as np

# kind -> N2V2R_CORR_* (include/n2v2r.h); the names follow WGCNA's networkType
KINDS = {"unsigned": 0, "signed": 1, "signed hybrid": 2, "raw": 3}
# tom -> N2V2R_TOM_*; the names follow WGCNA's TOMType
TOMS = ("unsigned", "signed")
# method -> N2V2R_COR_* (include/n2v2r.h); the names follow R's cor(method=) and WGCNA's corFnc
METHODS = {"pearson": 0, "spearman": 1, "bicor": 2}


def method_name(method) -> str:
    """The case-folded name of a correlation method; ``ValueError`` for anything else."""
    if not isinstance(method, str) or method.casefold() not in METHODS:
        raise ValueError(f"unknown method {method!r}; options are {sorted(METHODS)}")
    return method.casefold()


class Coexpression:
    """One layer: ``t(np.corrcoef(expression)) ** power`` over the rows of ``expression`` (or
    the Spearman or biweight midcorrelation in ``np.corrcoef``'s place, see ``method``).

    expression: ``n x samples`` (n nodes / genes), any real dtype or a DataFrame; kept as a
        C-contiguous float64 array (``.expression``).
    kind: ``"unsigned"`` |r|, ``"signed"`` (1 + r) / 2, ``"signed hybrid"`` max(r, 0) or
        ``"raw"`` r itself.
    power: the soft-threshold exponent, >= 1 (``"raw"`` layers, which may be negative, take 1).
    tom: ``None`` (the adjacency itself), ``"unsigned"`` or ``"signed"``: the layer becomes the
        topological overlap matrix of the adjacency (WGCNA's ``TOMsimilarity`` with
        ``TOMDenom="min"``, hdWGCNA's ``GetTOM``), on the GPU (``n2v2r_tom_layer``), before the
        options below.  ``"unsigned"`` needs entries in [0, 1] (every kind but ``"raw"`` gives
        them); ``"signed"`` takes [-1, 1].  The engine checks the range when the layer is
        loaded: a ``"raw"`` layer that happens to be non-negative passes as ``"unsigned"``.
    threshold, top_percent_keep, binarize: the reference's ``network_transform``
        (``preprocessing_utils.py:116-141``) applied to the finished layer, on the GPU
        (``n2v2r_transform_layer``): entries below ``threshold`` are dropped, then only the top
        ``top_percent_keep`` percent of the non-zero entries stay (an ``np.percentile`` cut), and
        with ``binarize`` the survivors become 1.  The defaults (``None``, 100, ``False``) leave
        the layer as built.  There is no ``absolute`` option: ``kind="unsigned"`` is that.
    method: the correlation r, case-folded.  ``"pearson"`` (the default); ``"spearman"``, the
        Pearson correlation of the rows' average ranks (ties share their mean rank, as
        ``scipy.stats.rankdata``); ``"bicor"``, the biweight midcorrelation, WGCNA's
        ``corFnc = "bicor"`` with ``maxPOutliers = 1`` and ``pearsonFallback = "individual"``: a
        row whose MAD is zero is standardised by the Pearson formula, and the engine warns with
        the count of such rows.  Missing values, ``maxPOutliers < 1``, the other fallback modes
        and Kendall's tau are out of scope.

    Every violation is a ``ValueError`` here, before any GPU work; rows the correlation is
    undefined for (a non-finite value, zero variance) are reported by the engine when the layer
    is loaded, by row index."""

    def __init__(self, expression, kind: str = "unsigned", power: float = 1.0, threshold=None,
                 top_percent_keep=100, binarize: bool = False, tom=None,
                 method: str = "pearson"):
        values = getattr(expression, "values", expression)  # (a DataFrame's array)
        try:
            e = np.ascontiguousarray(np.asarray(values), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"expression must be a real n x samples array: {err}") from None
        if e.ndim != 2:
            raise ValueError(f"expression must be 2-D (n x samples), got {e.ndim}-D")
        if e.shape[0] < 1 or e.shape[1] < 2:
            raise ValueError("expression needs at least 1 row and 2 samples, got shape "
                             f"{e.shape}")
        if not isinstance(kind, str) or kind.replace("_", " ").casefold() not in KINDS:
            raise ValueError(f"unknown kind {kind!r}; options are {sorted(KINDS)}")
        try:
            p = float(power)
        except (TypeError, ValueError):
            raise ValueError(f"power must be a number, got {power!r}") from None
        if not math.isfinite(p) or p < 1.0:
            raise ValueError(f"power must be finite and >= 1, got {power!r}")
        self.kind = kind.replace("_", " ").casefold()
        if self.kind == "raw" and p != 1.0:
            raise ValueError("a raw correlation layer takes power 1 (r may be negative)")
        if threshold is not None:
            try:
                threshold = float(threshold)
            except (TypeError, ValueError):
                raise ValueError(f"threshold must be a number or None, got {threshold!r}") from None
            if not math.isfinite(threshold):
                raise ValueError(f"threshold must be finite, got {threshold!r}")
        try:
            top = float(top_percent_keep)
        except (TypeError, ValueError):
            raise ValueError("top_percent_keep must be a number, got "
                             f"{top_percent_keep!r}") from None
        if not math.isfinite(top) or not 0.0 <= top <= 100.0:
            raise ValueError(f"top_percent_keep must lie in [0, 100], got {top_percent_keep!r}")
        if not isinstance(binarize, (bool, np.bool_)):
            raise ValueError(f"binarize must be True or False, got {binarize!r}")
        if tom is not None and (not isinstance(tom, str) or tom.casefold() not in TOMS):
            raise ValueError(f"unknown tom {tom!r}; options are None, 'unsigned' and 'signed'")
        self.method = method_name(method)
        self.expression = e
        self.power = p
        self.threshold = threshold
        self.top_percent_keep = top
        self.binarize = bool(binarize)
        self.tom = None if tom is None else tom.casefold()

    @property
    def shape(self):
        """Shape of the layer (n x n), as a graph array's."""
        return (self.expression.shape[0], self.expression.shape[0])

    @property
    def kind_id(self) -> int:
        return KINDS[self.kind]

    @property
    def method_id(self) -> int:
        return METHODS[self.method]

    @property
    def filters(self) -> bool:
        """Whether any of threshold / top_percent_keep / binarize is set."""
        return self.threshold is not None or self.top_percent_keep != 100.0 or self.binarize

    @property
    def transforms(self) -> bool:
        """Whether the layer is changed after the correlation build: ``tom`` or any of
        threshold / top_percent_keep / binarize."""
        return self.tom is not None or self.filters

    def __repr__(self):
        n, s = self.expression.shape
        extra = ""
        if self.method != "pearson":
            extra = f", method={self.method!r}"
        if self.tom is not None:
            extra += f", tom={self.tom!r}"
        if self.filters:
            extra += (f", threshold={self.threshold!r}, top_percent_keep={self.top_percent_keep:g}"
                      f", binarize={self.binarize}")
        return (f"Coexpression(n={n}, samples={s}, kind={self.kind!r}, power={self.power:g}"
                f"{extra})")
