"""``Coexpression`` layers, host side: validation, the storage rule of ``Engine.set_layers`` and
the declared C-ABI.  CPU only (nothing here creates a handle)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import REPO


def _E(n=12, s=5, seed=0):
    return np.random.default_rng(seed).standard_normal((n, s))


def test_coexpression_holds_contiguous_float64():
    import node2vec2rank_amd
    from node2vec2rank_amd import Coexpression
    assert node2vec2rank_amd.Coexpression is Coexpression
    E = np.asfortranarray(_E().astype(np.float32))
    c = Coexpression(E)
    assert c.expression.dtype == np.float64 and c.expression.flags.c_contiguous
    np.testing.assert_array_equal(c.expression, E.astype(np.float64))
    assert (c.kind, c.power, c.shape) == ("unsigned", 1.0, (12, 12))
    assert Coexpression(_E(), kind="signed_hybrid", power=6).kind == "signed hybrid"
    assert Coexpression(_E(), kind="raw").kind_id == 3
    import pandas as pd
    assert Coexpression(pd.DataFrame(_E())).expression.shape == (12, 5)


@pytest.mark.parametrize("args, kwargs", [
    ((np.zeros(7),), {}),                        # 1-D
    ((np.zeros((3, 4, 5)),), {}),                # 3-D
    ((np.zeros((6, 1)),), {}),                   # one sample
    ((np.zeros((0, 4)),), {}),                   # no rows
    ((_E(),), dict(kind="pearson")),             # unknown kind
    ((_E(),), dict(kind=None)),
    ((_E(),), dict(power=0.5)),                  # power < 1
    ((_E(),), dict(power=float("nan"))),
    ((_E(),), dict(power=float("inf"))),
    ((_E(),), dict(power="six")),
    ((_E(),), dict(kind="raw", power=2.0)),      # raw only with power 1
    ((np.array([["a", "b"], ["c", "d"]]),), {}),  # not numbers
])
def test_coexpression_validation(args, kwargs):
    from node2vec2rank_amd import Coexpression
    with pytest.raises(ValueError):
        Coexpression(*args, **kwargs)


class _NoLibrary:
    """Stands in for the ctypes library: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called: set_layers must refuse before any library call")


def _stub_engine():
    from node2vec2rank_amd import _lib
    eng = object.__new__(_lib.Engine)
    eng.h = None  # (close() / __del__ then have nothing to destroy)
    eng.lib = _NoLibrary()
    return eng


def test_set_layers_refuses_sparse_or_csr_next_to_coexpression():
    from node2vec2rank_amd import Coexpression
    eng = _stub_engine()
    c = Coexpression(_E())
    with pytest.raises(ValueError, match="sparse"):
        eng.set_layers([c, sp.identity(12, format="csr", dtype=np.float32)])
    with pytest.raises(ValueError, match="sparse"):
        eng.set_layers([sp.identity(12, format="coo"), c], storage="dense")
    with pytest.raises(ValueError, match="csr"):
        eng.set_layers([c, c], storage="csr")
    with pytest.raises(ValueError, match="node set"):
        eng.set_layers([c, np.ones((11, 11), dtype=np.float32)])
    with pytest.raises(ValueError, match="node set"):
        eng.set_layers([c, Coexpression(_E(n=13))])


def test_as_layer_passes_coexpression_through():
    from node2vec2rank_amd import Coexpression
    from node2vec2rank_amd.model import _as_layer
    c = Coexpression(_E())
    assert _as_layer(c) is c


def test_new_symbols_are_declared():
    from node2vec2rank_amd import _lib
    main = open(os.path.join(REPO, "include", "n2v2r.h")).read()
    diag = open(os.path.join(REPO, "include", "n2v2r_diag.h")).read()
    assert re.search(r"int\s+n2v2r_set_layer_corr\s*\(\s*n2v2r_handle\s*\*\s*h,\s*int\s+k,\s*"
                     r"int64_t\s+n,\s*int64_t\s+samples,\s*const\s+double\s*\*\s*E[^)]*,\s*"
                     r"int\s+kind,\s*double\s+power\s*\)", main)
    for name, value in [("UNSIGNED", 0), ("SIGNED", 1), ("SIGNED_HYBRID", 2), ("RAW", 3)]:
        assert re.search(rf"N2V2R_CORR_{name}\s*=\s*{value}\b", main), name
    assert "np.corrcoef" in main
    assert re.search(r"int\s+n2v2r_get_layer_dense\s*\(\s*n2v2r_handle\s*\*\s*h,\s*int\s+k,\s*"
                     r"float\s*\*\s*A", diag)
    assert {"n2v2r_set_layer_corr", "n2v2r_get_layer_dense"} <= set(_lib.EXPORTED)
    from node2vec2rank_amd.coexpression import KINDS
    assert KINDS == {"unsigned": 0, "signed": 1, "signed hybrid": 2, "raw": 3}
