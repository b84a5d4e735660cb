"""The ``tom`` option of ``Coexpression`` (no GPU): validation in the constructor, ``__repr__``
and ``transforms``."""
import numpy as np
import pytest

from node2vec2rank_amd import Coexpression

E = np.random.default_rng(0).standard_normal((6, 5))


def test_default_is_the_adjacency():
    c = Coexpression(E)
    assert c.tom is None
    assert not c.transforms and "tom" not in repr(c)


@pytest.mark.parametrize("tom", ["unsigned", "signed", "Signed", "UNSIGNED"])
def test_tom_is_kept_shown_and_counts_as_a_transform(tom):
    c = Coexpression(E, kind="signed", power=6, tom=tom)
    assert c.tom == tom.casefold()
    assert c.transforms
    assert f"tom={tom.casefold()!r}" in repr(c)
    assert "threshold" not in repr(c)  # the other options are still at their defaults
    both = Coexpression(E, tom=tom, top_percent_keep=37.5, binarize=True)
    assert both.transforms
    assert f"tom={tom.casefold()!r}" in repr(both) and "top_percent_keep=37.5" in repr(both)


@pytest.mark.parametrize("tom", ["mean", "", "signed Nowick", 0, 1, True, False, b"signed",
                                 ["signed"]])
def test_anything_else_is_a_value_error(tom):
    with pytest.raises(ValueError, match="tom"):
        Coexpression(E, tom=tom)


def test_unsigned_tom_of_a_raw_layer_is_left_to_the_engine():
    """A raw layer may by chance be non-negative: the range is checked where the values are."""
    c = Coexpression(E, kind="raw", tom="unsigned")
    assert c.kind == "raw" and c.tom == "unsigned"
