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


class Coexpression:
    """One layer: ``t(np.corrcoef(expression)) ** power`` over the rows of ``expression``.

    expression: ``n x samples`` (n nodes / genes), any real dtype or a DataFrame; kept as a
        C-contiguous float64 array (``.expression``).
    kind: ``"unsigned"`` |r|, ``"signed"`` (1 + r) / 2, ``"signed hybrid"`` max(r, 0) or
        ``"raw"`` r itself.
    power: the soft-threshold exponent, >= 1 (``"raw"`` layers, which may be negative, take 1).

    Every violation is a ``ValueError`` here, before any GPU work; rows the correlation is
    undefined for (a non-finite value, zero variance) are reported by the engine when the layer
    is loaded, by row index."""

    def __init__(self, expression, kind: str = "unsigned", power: float = 1.0):
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
        self.expression = e
        self.power = p

    @property
    def shape(self):
        """Shape of the layer (n x n), as a graph array's."""
        return (self.expression.shape[0], self.expression.shape[0])

    @property
    def kind_id(self) -> int:
        return KINDS[self.kind]

    def __repr__(self):
        n, s = self.expression.shape
        return f"Coexpression(n={n}, samples={s}, kind={self.kind!r}, power={self.power:g})"
