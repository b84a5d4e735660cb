"""The threshold / top_percent_keep / binarize options of ``Coexpression`` and the declaration of
``n2v2r_transform_layer``.  CPU only: nothing here touches the GPU."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _E():
    return np.random.default_rng(0).standard_normal((5, 4))


def test_defaults_and_repr_unchanged():
    from node2vec2rank_amd import Coexpression
    c = Coexpression(_E())
    assert (c.threshold, c.top_percent_keep, c.binarize) == (None, 100.0, False)
    assert not c.transforms
    assert repr(c) == "Coexpression(n=5, samples=4, kind='unsigned', power=1)"
    assert repr(Coexpression(_E(), kind="signed", power=6)) == \
        "Coexpression(n=5, samples=4, kind='signed', power=6)"
    # explicit defaults are defaults
    c = Coexpression(_E(), threshold=None, top_percent_keep=100, binarize=False)
    assert not c.transforms and "threshold" not in repr(c)


def test_options_are_kept_and_shown():
    from node2vec2rank_amd import Coexpression
    c = Coexpression(_E(), threshold=0.1, top_percent_keep=37.5, binarize=True)
    assert (c.threshold, c.top_percent_keep, c.binarize) == (0.1, 37.5, True)
    assert c.transforms
    assert repr(c) == ("Coexpression(n=5, samples=4, kind='unsigned', power=1, threshold=0.1, "
                       "top_percent_keep=37.5, binarize=True)")
    for kw in (dict(threshold=0.0), dict(top_percent_keep=5), dict(binarize=True),
               dict(top_percent_keep=0)):
        c = Coexpression(_E(), **kw)
        assert c.transforms, kw
        assert "top_percent_keep=" in repr(c)
    assert Coexpression(_E(), top_percent_keep=np.float32(50)).top_percent_keep == 50.0
    assert Coexpression(_E(), threshold=np.float64(-0.5)).threshold == -0.5


@pytest.mark.parametrize("kw", [
    dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold="high"),
    dict(threshold=[0.1]),
    dict(top_percent_keep=101), dict(top_percent_keep=-0.5), dict(top_percent_keep=float("nan")),
    dict(top_percent_keep=float("inf")), dict(top_percent_keep=None), dict(top_percent_keep="5%"),
    dict(binarize=1), dict(binarize="yes"), dict(binarize=None),
])
def test_bad_options_are_value_errors(kw):
    from node2vec2rank_amd import Coexpression
    with pytest.raises(ValueError, match=next(iter(kw))):
        Coexpression(_E(), **kw)


def test_header_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "n2v2r.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+n2v2r_transform_layer\s*\(\s*n2v2r_handle\s*\*\s*h\s*,\s*int\s+k\s*,"
                     r"\s*int\s+flags\s*,\s*double\s+threshold\s*,\s*double\s+top_percent_keep\s*,"
                     r"\s*n2v2r_transform_stats\s*\*\s*stats\s*\)", code)
    assert re.search(r"N2V2R_TF_ABSOLUTE\s*=\s*1\s*,\s*N2V2R_TF_BINARIZE\s*=\s*2\s*,"
                     r"\s*N2V2R_TF_THRESHOLD\s*=\s*4", code)
    assert re.search(r"int64_t\s+nonzero\s*;\s*int64_t\s+kept\s*;\s*double\s+cut\s*;", code)
    from node2vec2rank_amd import _lib
    assert "n2v2r_transform_layer" in _lib.EXPORTED
    assert (_lib.TF_ABSOLUTE, _lib.TF_BINARIZE, _lib.TF_THRESHOLD) == (1, 2, 4)
