"""The ``sparsify`` option of ``Engine.set_layers``, host side, and the declared C-ABI of the
dense -> CSR conversion.  CPU only (nothing here creates a handle)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import REPO
from test_coexpression import _E, _stub_engine


@pytest.mark.parametrize("bad", ["yes", "AUTO", 1, 0, None, 2.5])
def test_unknown_sparsify_value_is_refused_before_any_library_call(bad):
    from node2vec2rank_amd import Coexpression
    eng = _stub_engine()
    with pytest.raises(ValueError, match="sparsify"):
        eng.set_layers([Coexpression(_E())], sparsify=bad)
    with pytest.raises(ValueError, match="sparsify"):
        eng.set_layers([np.ones((12, 12), dtype=np.float32)], storage="dense", sparsify=bad)


@pytest.mark.parametrize("sparsify", [True, "auto"])
def test_sparsify_with_nothing_to_convert_is_refused_before_any_library_call(sparsify):
    from node2vec2rank_amd import Coexpression
    eng = _stub_engine()
    dense = np.ones((12, 12), dtype=np.float32)
    with pytest.raises(ValueError, match="nothing to convert"):
        eng.set_layers([dense], storage="csr", sparsify=sparsify)
    with pytest.raises(ValueError, match="nothing to convert"):
        eng.set_layers([sp.identity(12, format="csr", dtype=np.float32)], sparsify=sparsify)
    with pytest.raises(ValueError, match="nothing to convert"):
        eng.set_layers([dense, sp.identity(12, format="coo")], storage="dense", sparsify=sparsify)
    # storage="csr" next to Coexpression layers stays an error
    with pytest.raises(ValueError, match="csr"):
        eng.set_layers([Coexpression(_E())], storage="csr", sparsify=sparsify)
    with pytest.raises(ValueError, match="csr"):
        eng.set_layers([Coexpression(_E())], storage="csr")


def test_model_passes_sparsify_to_set_layers():
    from node2vec2rank_amd.model import N2V2R
    config = dict(embed_dimensions=[2], distance_metrics=["cosine"], comp_strategy="sequential",
                  seed=1, verbose=-1, save_dir=None)
    graphs = [np.ones((3, 3), dtype=np.float32)] * 2
    seen = {}

    class Eng:
        def set_layers(self, layers, **kw):
            seen.update(kw)

    for value in (False, True, "auto"):
        model = N2V2R(graphs=graphs, nodes=list("abc"), config=dict(config), sparsify=value)
        model._eng = Eng()
        model._eng.h = object()
        import weakref
        model._eng._owner = weakref.ref(model)
        model._load_layers()
        assert seen == {"sparsify": value}
    assert N2V2R(graphs=graphs, nodes=list("abc"), config=dict(config))._sparsify is False


def test_new_symbols_are_declared():
    from node2vec2rank_amd import _lib
    main = open(os.path.join(REPO, "include", "n2v2r.h")).read()
    diag = open(os.path.join(REPO, "include", "n2v2r_diag.h")).read()
    assert re.search(r"int\s+n2v2r_layers_to_csr\s*\(\s*n2v2r_handle\s*\*\s*h,\s*"
                     r"int64_t\s*\*\s*nnz\s*(/\*[^)]*\*/\s*)?\)", main)
    assert re.search(r"int\s+n2v2r_get_layer_csr_nnz\s*\(\s*n2v2r_handle\s*\*\s*h,\s*int\s+k,\s*"
                     r"int\s+transpose,\s*int64_t\s*\*\s*nnz\s*\)", diag)
    assert re.search(r"int\s+n2v2r_get_layer_csr\s*\(\s*n2v2r_handle\s*\*\s*h,\s*int\s+k,\s*"
                     r"int\s+transpose,\s*int64_t\s*\*\s*indptr,\s*int32_t\s*\*\s*indices,\s*"
                     r"float\s*\*\s*data\s*\)", diag)
    assert {"n2v2r_layers_to_csr", "n2v2r_get_layer_csr_nnz", "n2v2r_get_layer_csr"} <= set(
        _lib.EXPORTED)
    lib = _lib.load()
    for name in ("n2v2r_layers_to_csr", "n2v2r_count_layer_nonzeros", "n2v2r_get_layer_csr_nnz",
                 "n2v2r_get_layer_csr", "n2v2r_bench_sparsify_pass"):
        assert hasattr(lib, name), name
    assert lib.n2v2r_layers_to_csr(None, None) == _lib.ERR_BAD_ARG


def test_scipy_stores_nan_and_drops_negative_zero():
    """The rule the conversion kernels follow is ``scipy.sparse.csr_matrix(dense)``'s: a NaN is
    non-zero and stored, -0.0 equals zero and is dropped."""
    A = np.zeros((3, 3), dtype=np.float32)
    A[0, 1] = np.nan
    A[1, 2] = -0.0
    A[2, 0] = 2.0
    m = sp.csr_matrix(A)
    assert m.nnz == 2 == np.count_nonzero(A)
    assert m.indices.tolist() == [1, 0] and m.indptr.tolist() == [0, 1, 1, 2]
    assert np.isnan(m.data[0]) and m.data[1] == 2.0
