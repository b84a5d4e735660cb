"""The Borda radix sort (csrc/rank.hip, run_borda in csrc/ranking.cpp) on every key class, digit
and tile edge, against the oracle's stable Borda (``borda(D, faithful=False)``: descending, ties by
ascending row, NaN last in row order) and, for ``tie_order="reference"``, against
``borda(D, faithful=True)``.  Integers throughout: every comparison is exact.  Every call is
also checked to return one permutation per column (the sum of the scores) and to return the same
array when made again.  The inputs are those of borda_inputs.py, checked on the CPU by
test_borda_inputs.py."""
import time

import numpy as np
import pytest

import borda_inputs as bi
from node2vec2rank_amd import _lib
from oracle import n2v2r_oracle as orc

pytestmark = pytest.mark.gpu


def _check(eng, D, want=None, reference_order=False, **kw):
    """The stable GPU Borda of the n x C table D: equal to the oracle (or ``want``), a
    permutation per column, the same on a second call.  Returns what borda_columns returned."""
    D = np.asarray(D, dtype=np.float64)
    n, c = D.shape
    res = eng.borda_columns(D, **kw)
    got = res[0] if isinstance(res, tuple) else res
    assert got.dtype == np.int64 and got.shape == (n,)
    np.testing.assert_array_equal(got, orc.borda(D, faithful=False) if want is None else want)
    assert int(got.sum()) == c * n * (n + 1) // 2
    again = eng.borda_columns(D, **kw)
    np.testing.assert_array_equal(again[0] if isinstance(again, tuple) else again, got)
    if reference_order:
        ref = eng.borda_columns(D, tie_order="reference")
        np.testing.assert_array_equal(ref, orc.borda(D, faithful=True))
        assert int(ref.sum()) == c * n * (n + 1) // 2
        np.testing.assert_array_equal(eng.borda_columns(D, tie_order="reference"), ref)
    return res


# ---------------------------------------------------------------------------- (a) key classes
def _key_class_tables():
    col = bi.key_class_column()
    rng = np.random.default_rng(11)
    ordinary = np.abs(rng.standard_normal((col.size, 2)))
    return {"alone": col[:, None],
            "between_ordinary": np.column_stack([ordinary[:, 0], col, ordinary[:, 1]])}


@pytest.mark.parametrize("which", ["alone", "between_ordinary"])
def test_key_classes(engine, which):
    """+-inf, +-0, subnormals, +-DBL_MIN, +-DBL_MAX, one-ulp neighbours of +-1 and three kinds of
    NaN in one column of two tiles, every one twice."""
    D = _key_class_tables()[which]
    _, tied = _check(engine, D, reference_order=True, return_tied=True)
    assert tied[0 if which == "alone" else 1]


def test_key_classes_multi_engine(engine):
    """The same tables through a two-rank handle on one device: rank 0's sort, the same result."""
    multi = _lib.Engine.multi((0, 0))
    try:
        for D in _key_class_tables().values():
            np.testing.assert_array_equal(_check(multi, D, reference_order=True),
                                          engine.borda_columns(D))
    finally:
        multi.close()


# ---------------------------------------------------------------------------- (b) one byte
@pytest.mark.parametrize("p,negative", bi.ONE_BYTE_CASES)
def test_one_varying_byte_alone(engine, p, negative):
    """One radix pass, on digit p."""
    _check(engine, bi.one_byte_column(p, negative)[:, None])


def test_one_varying_byte_all_sixteen_together(engine):
    """All eight passes run; each is the identity on the fifteen columns constant in its digit."""
    D = np.column_stack([bi.one_byte_column(p, neg) for p, neg in bi.ONE_BYTE_CASES])
    _check(engine, D)


@pytest.mark.parametrize("negative", [False, True])
def test_lowest_and_highest_byte_pair(engine, negative):
    D = np.column_stack([bi.one_byte_column(0, negative), bi.one_byte_column(7, not negative)])
    _check(engine, D)
    _check(engine, D[:, ::-1])


# ---------------------------------------------------------------------------- (c) sizes
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", bi.SIZES)
def test_sizes_and_columns(engine, n, c):
    """Wave, workgroup, tile and scan-chunk edges (32768 keys: 256 * 8 tiles = one 2048-entry
    chunk; 32769: two, the second partial), one column and three."""
    _check(engine, bi.mixed_table(n, c), reference_order=n <= 4097)


def test_sixty_four_columns_at_a_tile_edge(engine):
    _check(engine, bi.rounded_table(4097, 64), reference_order=True)


# ---------------------------------------------------------------------------- (d) distributions
@pytest.mark.parametrize("name", ["ascending", "descending", "all_equal", "all_nan",
                                  "alternating", "tile_constant", "together"])
def test_distributions(engine, name):
    cols = bi.distribution_columns()
    D = np.column_stack(list(cols.values())) if name == "together" else cols[name][:, None]
    _check(engine, D)


# ---------------------------------------------------------------------------- (e) tie flags
@pytest.mark.parametrize("n", sorted({n for n, _ in bi.TIE_CASES}))
def test_tie_flag_at_wave_workgroup_and_tile_boundaries(engine, n):
    """One equal pair at sorted positions (p, p + 1), across lanes 63|64, workgroups 255|256,
    tiles 4095|4096 and at the very end of the column: flagged, and only there."""
    cols, want = [bi.distinct_column(n, 600 + n)], [False]
    for m, p in bi.TIE_CASES:
        if m == n:
            cols += [bi.tie_column(n, p), bi.distinct_column(n, 700 + n + p)]
            want += [True, False]
    _, tied = _check(engine, np.column_stack(cols), return_tied=True)
    assert tied.tolist() == want


def test_tie_flag_nan_and_signed_zero(engine):
    n = 300
    nan_only = bi.distinct_column(n, 801)
    nan_only[[3, 70, 299]] = np.nan
    zeros = bi.distinct_column(n, 802)
    zeros[5], zeros[260] = -0.0, 0.0
    _, tied = _check(engine, np.column_stack([nan_only, zeros, bi.distinct_column(n, 803)]),
                     return_tied=True)
    assert tied.tolist() == [False, True, False]


# ---------------------------------------------------------------------------- (f) label seam
def test_label_seam_at_size():
    """borda_aggregate_parallel encodes a ranking as -position (-0.0, -1, ..., -(n - 1)):
    negative keys over two tiles."""
    from node2vec2rank_amd.model_utils import borda_aggregate_parallel
    n = 5000
    rng = np.random.default_rng(21)
    labels = np.array([f"g{i}" for i in range(n)])
    perms = [rng.permutation(n) for _ in range(4)]
    got = borda_aggregate_parallel([list(labels[p]) for p in perms])
    total = np.zeros(n, dtype=np.int64)
    for p in perms:
        pos = np.empty(n, dtype=np.int64)
        pos[p] = np.arange(n)
        total += n - pos
    assert list(got.index) == list(labels[perms[0]])
    assert got["borda_ranks"].dtype == np.int64
    np.testing.assert_array_equal(got["borda_ranks"].to_numpy(), total[perms[0]])


# ---------------------------------------------------------------------------- (g) groups
def test_groups_of_columns_in_rank(engine):
    """rank() sorts every comparison's columns in one call (12 segments, 4 per group) and sums
    them per group."""
    rng = np.random.default_rng(31)
    engine.set_embedding(rng.standard_normal((3, 4097, 8)).astype(np.float32))
    ncmp, ncols = engine.rank("one_vs_rest", [2, 8], ["cosine", "euclidean"])
    assert (ncmp, ncols) == (3, 4)
    first = [engine.borda(c) for c in range(ncmp)]
    for c in range(ncmp):
        np.testing.assert_array_equal(first[c], orc.borda(engine.distances(c), faithful=False))
        assert int(first[c].sum()) == ncols * 4097 * 4098 // 2
    engine.rank("one_vs_rest", [2, 8], ["cosine", "euclidean"])
    for c in range(ncmp):
        np.testing.assert_array_equal(engine.borda(c), first[c])


# ---------------------------------------------------------------------------- (h) state
def test_no_state_between_calls(engine):
    big, small = bi.mixed_table(32769, 3), bi.mixed_table(65, 1)
    first = _check(engine, big)
    _check(engine, small)
    np.testing.assert_array_equal(engine.borda_columns(big), first)


# ---------------------------------------------------------------------------- (i) > 1024 chunks
def test_more_than_1024_scan_chunks(engine):
    """33,652,743 keys: 8217 tiles, 1028 chunks of the histogram scan, so the chunk-offset scan
    runs a second 1024-entry round with a carry.  Three passes (bytes 5..7).  The reference is a
    16-bit stable argsort (borda_inputs.chunk_case_reference, equal to the oracle on a prefix).

    The heaviest case of the file: 1.2 s on an MI355X, of which 0.46 s are the two GPU calls with
    their comparisons and the rest the input and the reference
    (test_borda_large_with_ties_nans_and_negzero: 0.21 s).  About 1.5 GB of device memory."""
    v = bi.chunk_case_values()
    want = bi.chunk_case_reference(v)
    t0 = time.perf_counter()
    _check(engine, v[:, None], want=want)
    print(f"two sorts of {v.size} keys with checks: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------- n > INT32_MAX
def test_row_count_beyond_int32_is_refused(engine):
    """The sort's payload is an int32 row index: both entry points refuse n = 2**31 before they
    read anything (D is one element)."""
    D = np.zeros((1, 1), dtype=np.float64)
    out = np.zeros(1, dtype=np.int64)
    tied = np.zeros(1, dtype=np.int32)
    lib = engine.lib
    assert lib.n2v2r_borda_columns(engine.h, D, 2 ** 31, 1, out) == _lib.ERR_BAD_ARG
    assert lib.n2v2r_borda_columns_ex(engine.h, D, 2 ** 31, 1, None, 0, None, out,
                                      tied) == _lib.ERR_BAD_ARG
    assert lib.n2v2r_borda_columns(engine.h, D, 1, 1, out) == _lib.OK and out[0] == 1
