"""The generators of the Borda radix-sort tests (borda_inputs.py), checked on the CPU against a
numpy twin of the GPU's sort key, so that the GPU cases exercise the digits, tile edges and tie
positions they name."""
import numpy as np
import pytest

import borda_inputs as bi
from oracle import n2v2r_oracle as orc


def test_key_twin_orders_as_the_oracle_on_every_key_class():
    """Stable ascending order of the twin keys == the oracle's stable descending order
    (pandas nargsort: NaN of any sign or payload last in row order, -0 == +0)."""
    col = bi.key_class_column()
    b = bi.bits(col)
    for pat in bi.key_class_values():            # every class is there, twice, bits intact
        assert int((b == pat).sum()) == 2, hex(int(pat))
    assert int(np.isnan(col).sum()) == 6
    assert np.signbit(col[np.isnan(col)]).sum() == 2
    order = np.argsort(bi.desc_key(col), kind="stable")
    np.testing.assert_array_equal(order, orc._descending_order_pandas(col, "stable"))
    assert bi.varying_bytes(col) == list(range(8))


def test_key_twin_on_known_values():
    k = bi.desc_key(np.array([np.inf, bi.DBL_MAX, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0,
                              -bi.DBL_MAX, -np.inf, np.nan]))
    assert k[4] == k[5]
    assert (np.diff(k[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]].astype(object)) > 0).all()
    assert k[10] == bi.ALL_ONES and k[0] == ~(bi.bits(np.array([np.inf]))[0] | bi.SIGN)


@pytest.mark.parametrize("p,negative", bi.ONE_BYTE_CASES)
def test_one_byte_columns_vary_in_exactly_that_byte(p, negative):
    col = bi.one_byte_column(p, negative)
    assert np.isfinite(col).all() and (col != 0.0).all()
    assert (np.signbit(col) == negative).all()
    assert bi.varying_bytes(col) == [p]
    assert np.unique(col).size > 100             # the pass has work to do
    # the bit patterns themselves differ in byte p only, too
    b = bi.bits(col)
    diff = int(np.bitwise_or.reduce(b) ^ np.bitwise_and.reduce(b))
    assert diff & ~(0xFF << (8 * p)) == 0
    if p == 7:                                   # digit 0 excluded: no +-0, no subnormal base
        assert ((b >> np.uint64(56)) & np.uint64(0x7F)).min() >= 1
        assert ((b >> np.uint64(56)) & np.uint64(0x7F)).max() <= 0x7E


@pytest.mark.parametrize("n,p", bi.TIE_CASES)
def test_tie_columns_hold_one_equal_pair_where_they_say(n, p):
    col = bi.tie_column(n, p)
    assert col.shape == (n,)
    assert bi.equal_adjacent_pairs(col) == [p]
    assert bi.equal_adjacent_pairs(bi.distinct_column(n, 9)) == []


def test_distribution_columns_are_what_they_are_called():
    cols = bi.distribution_columns()
    n = 2 * bi.TILE + 1
    assert all(c.shape == (n,) for c in cols.values())
    assert (np.diff(cols["ascending"]) > 0).all() and (np.diff(cols["descending"]) < 0).all()
    assert bi.varying_bytes(cols["all_equal"]) == [] and bi.varying_bytes(cols["all_nan"]) == []
    t = cols["tile_constant"]
    assert np.unique(t[:bi.TILE]).size == 1 and np.unique(t[bi.TILE:2 * bi.TILE]).size == 1
    assert np.unique(t).size == 3


def test_mixed_tables_hold_ties_nans_and_both_signs():
    D = bi.mixed_table(4097, 3)
    assert np.isnan(D).any() and (D < 0).any() and (D > 0).any()
    assert (D == -0.75).sum() > 3 * 4097 * 0.05


def test_chunk_case_reference_equals_the_oracle_on_a_prefix():
    m = 100_003
    v = bi.chunk_case_values(m)
    assert v.min() >= 0 and v.max() <= 1023 and np.unique(v).size == 1024
    assert bi.varying_bytes(v) == [5, 6, 7]      # three passes
    np.testing.assert_array_equal(bi.chunk_case_reference(v), orc.borda(v[:, None]))
    ntiles = -(-bi.N_CHUNKS_CASE // bi.TILE)
    assert ntiles == 8217 and -(-256 * ntiles // 2048) == 1028
