"""What the CSR ingest leaves in HBM, entry by entry: the rows of A, the A^T copy and the symmetry
verdict, on the one-GPU handle (csrc/ingest.hip: the scan, the stable radix transpose, the
comparison), on rank handles (the same on the GPU, then row slices) and on the multi-GPU handle
(the host twin in csrc/layers.cpp: ``host_csr_symmetric``, ``host_transpose_rows``,
``host_all_ones``, ``host_indices_in_range``), read back with ``Engine.layer_csr``.

Oracles.  The stored A is the input's own ``(indptr, indices, data)``: the ingest neither sorts
nor sums.  The stored A^T is ``inp.tocsc()`` read as a CSR, on exactly the arrays handed in: the
stable counting sort by column, duplicates kept as separate entries in source-row order.  A
symmetric verdict shows as ``layer_csr(k, transpose=True)`` raising ``ValueError`` (no copy is
kept); a directed one as the copy being there.  Every comparison is bitwise; there are no
tolerances in this file (the column sums are of integers below 2^24: exact in any order).  The
unweighted flag does not show in a read-back (a unit layer's values are 1.0f either way); it is
read from the value-stream bytes ``bench_spmm`` reports (``test_unweighted_flag``).

The safe-direction rule.  For a -0.0 stored against a +0.0, a NaN stored against a NaN and a
symmetric layer with duplicate entries the paths legitimately differ (the GPU compares entry by
entry with float ==, the host hashes the bits of a multiset), so no exact verdict is asserted
there, only this, on every path: if the verdict is symmetric, the stored A equals the oracle's
A^T, where equal means == or both NaN, after ``sum_duplicates`` on both sides; if it is directed,
the kept copy is the oracle's, bitwise.  (As the code stands, the GPU paths and the dense ingest
take the +-0 pair for symmetric and the NaN pair and the duplicates for directed; the host path
of the multi-GPU handle the other way round.)

Out of scope: the radix scan's 1024-chunk carry loop, which needs more than 33.5 M entries."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import n2v2r_oracle as orc
from test_gpu_dist import _run_ranks
from test_gpu_ingest_device import _shuffle_rows
from test_gpu_sparsify import _bits, _same_csr, _symmetric

pytestmark = pytest.mark.gpu

SYM_DETECT, SYM_NO = -1, 0
ONE = 0x3F800000


# ---- inputs -----------------------------------------------------------------------------------
def _csr(n, counts, cols, vals, rows=None):
    """The CSR with these arrays as they are (scipy neither sorts nor sums them)."""
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return sp.csr_matrix((np.asarray(vals, dtype=np.float32), np.asarray(cols, dtype=np.int32),
                          indptr), shape=(n if rows is None else rows, n))


def _values(rng, nnz, weighted):
    return (rng.integers(1, 8, nnz) if weighted else np.ones(nnz)).astype(np.float32)


def _rand(n, mean, seed, weighted, colset=None, counts=None):
    """Rows of 0 .. 2 mean entries (or `counts`), columns drawn from `colset` (default: all):
    rows unsorted, duplicates as they fall."""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = rng.integers(0, 2 * mean + 1, n)
    nnz = int(np.sum(counts))
    cols = rng.integers(0, n, nnz) if colset is None else rng.choice(colset, nnz)
    return _csr(n, counts, cols, _values(rng, nnz, weighted))


def _rand_nnz(n, nnz, seed, weighted):
    rng = np.random.default_rng(seed)
    counts = np.bincount(rng.integers(0, n, nnz), minlength=n)
    return _csr(n, counts, rng.integers(0, n, nnz), _values(rng, nnz, weighted))


def _from_coo(n, r, c, v):
    """Entries in row order, ascending columns, equal (row, column) pairs in the order given."""
    order = np.lexsort((c, r))
    return _csr(n, np.bincount(r, minlength=n), np.asarray(c)[order], np.asarray(v)[order])


def _sym(n, mean, seed, weighted):
    """Canonical, finite, exactly symmetric (small integers, or all ones)."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=mean / (2.0 * n), format="csr", dtype=np.float32, random_state=rng)
    A.data = rng.integers(1, 4, A.nnz).astype(np.float32)
    S = (A + A.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    if not weighted:
        S.data[:] = 1.0
    assert (S != S.T).nnz == 0
    return sp.csr_matrix(S, dtype=np.float32)


def _copy(A, indices=None, data=None):
    return sp.csr_matrix(((A.data if data is None else data).astype(np.float32),
                          (A.indices if indices is None else indices).astype(np.int32),
                          A.indptr.astype(np.int64)), shape=A.shape)


def _ulp(A, p):
    data = A.data.copy()
    data[p] = np.nextafter(data[p], np.float32(np.inf))
    assert _bits(data[p:p + 1])[0] == _bits(A.data[p:p + 1])[0] + 1
    return _copy(A, data=data)


def _swap(A, p):
    """Entries p and p + 1 (of one row) change places: the same matrix, one descent."""
    ix, dv = A.indices.copy(), A.data.copy()
    assert ix[p] < ix[p + 1]
    ix[[p, p + 1]] = ix[[p + 1, p]]
    dv[[p, p + 1]] = dv[[p + 1, p]]
    return _copy(A, ix, dv)


def _row_of(A, p):
    return int(np.searchsorted(A.indptr, p, side="right") - 1)


def _long_row(n, seed):
    """Symmetric, weighted; row 7 holds exactly 130 ascending entries, the last row at least 2."""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < 0.01
    M[7, :] = M[:, 7] = False
    cols = np.sort(rng.choice(np.delete(np.arange(n), 7), 130, replace=False))
    M[7, cols] = True
    M[n - 1, [3, 8]] = True
    M = M | M.T
    V = np.triu(rng.integers(1, 4, (n, n)))
    V = V + np.triu(V, 1).T
    A = sp.csr_matrix((M * V).astype(np.float32))
    assert A.indptr[8] - A.indptr[7] == 130 and (A != A.T).nnz == 0
    return A


# ---- oracles and checks -----------------------------------------------------------------------
def _oracle_t(inp):
    """A^T as the ingest must store it: scipy's stable counting sort by column."""
    c = inp.tocsc()
    t = sp.csr_matrix((c.data, c.indices, c.indptr), shape=inp.shape)
    if inp.nnz <= 100_000:  # the same from first principles: a stable sort of the entries by column
        order = np.argsort(inp.indices, kind="stable")
        rows = np.repeat(np.arange(inp.shape[0]), np.diff(inp.indptr))
        assert np.array_equal(t.indices, rows[order])
        assert np.array_equal(_bits(t.data), _bits(inp.data[order]))
        assert np.array_equal(t.indptr[1:], np.cumsum(np.bincount(inp.indices,
                                                                  minlength=inp.shape[1])))
    return t


def _rows(m, row0, nl):
    p0, p1 = m.indptr[row0], m.indptr[row0 + nl]
    return sp.csr_matrix((m.data[p0:p1], m.indices[p0:p1],
                          (m.indptr[row0:row0 + nl + 1] - p0).astype(np.int64)),
                         shape=(nl, m.shape[1]))


def _read(eng, K):
    """[(stored A, stored A^T or None when the layer was judged symmetric)] of this handle."""
    out = []
    for k in range(K):
        try:
            t = eng.layer_csr(k, transpose=True)
        except ValueError as e:
            assert "symmetric" in str(e), e
            t = None
        out.append((eng.layer_csr(k), t))
    return out


def _check(read, layers, verdicts=None, row0=0, nl=None, tag=""):
    for k, (a, t) in enumerate(read):
        inp = layers[k]
        m = inp.shape[0] if nl is None else nl
        assert _same_csr(a, _rows(inp, row0, m)), (tag, k, "A")
        if t is not None:
            assert _same_csr(t, _rows(_oracle_t(inp), row0, m)), (tag, k, "A^T")
        if verdicts is not None:
            assert ("symmetric" if t is None else "directed") == verdicts[k], (tag, k)


def _canon_equal(a, b):
    a, b = a.copy(), b.copy()
    a.sum_duplicates()
    b.sum_duplicates()
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and
            bool(np.all((a.data == b.data) | (np.isnan(a.data) & np.isnan(b.data)))))


def _check_safe(read, layers, row0=0, nl=None, tag=""):
    """The safe-direction rule of the module docstring."""
    for k, (a, t) in enumerate(read):
        inp = layers[k]
        m = inp.shape[0] if nl is None else nl
        assert _same_csr(a, _rows(inp, row0, m)), (tag, k, "A")
        ref = _rows(_oracle_t(inp), row0, m)
        if t is None:
            assert _canon_equal(a, ref), (tag, k, "judged symmetric, A != A^T")
        else:
            assert _same_csr(t, ref), (tag, k, "A^T")


@pytest.fixture(scope="module")
def multi3():
    from node2vec2rank_amd import _lib
    eng = _lib.Engine.multi([0, 0, 0])
    yield eng
    eng.close()


def _on_ranks(world, layers, symmetric, sums=False):
    def fn(eng, r):
        eng.set_layers(layers, symmetric=symmetric)
        cs = [eng.column_sums(k) for k in range(len(layers))] if sums else None
        return eng.dist_info(), _read(eng, len(layers)), cs
    return _run_ranks(world, fn)


# ---- a. layout, one GPU, symmetric = SYM_NO ---------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65_536, 65_537, 262_149])
def test_layout_by_rows(engine, n, weighted):
    """The transpose's pass loop runs ceil(log2 n) column bits in 8-bit passes: one pass up to
    n = 256, two up to 65 536, three beyond; 262 149 rows is the first size past the scan's grid
    of 65 536 workgroups of 4 rows (its row loop's second stride).  About 3 entries per row."""
    A = _rand(n, 3, 100 + n, weighted, counts=np.full(n, 3) if n <= 2 else None)
    assert A.nnz > 0
    engine.set_layers([A], symmetric=SYM_NO)
    read = _read(engine, 1)
    assert read[0][1] is not None
    _check(read, [A], tag=n)
    if not weighted:
        for m in read[0]:
            assert np.array_equal(_bits(m.data), np.full(A.nnz, ONE, dtype=np.uint32))


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("nnz", [1, 4095, 4096, 4097, 32_769])
def test_layout_by_entries(engine, nnz, weighted):
    """Around the radix sort's tile of 4096 entries; 32 769 entries are 9 tiles, the first count
    whose 256 x 9 histogram needs a second 2048-element chunk of the scan."""
    A = _rand_nnz(1000, nnz, 200 + nnz, weighted)
    assert A.nnz == nnz
    engine.set_layers([A], symmetric=SYM_NO)
    _check(_read(engine, 1), [A], verdicts=["directed"], tag=nnz)


def _planted(weighted, n=300):
    """Seven layers at n = 300: the first 40 columns empty; the last 40; 260 consecutive empty
    columns in the middle (the row-pointer fill loops of csr_from_sorted_kernel, between two
    entries and behind the last one); empty rows (the first and the last among them); one row of
    130 entries; every entry in one column; every entry in one row."""
    w = weighted
    counts = np.random.default_rng(1).integers(0, 7, n)
    empty_rows = counts.copy()
    empty_rows[::2] = 0
    empty_rows[[0, n - 1]] = 0
    long_row = counts.copy()
    long_row[7] = 130
    one_col = np.ones(n, dtype=np.int64)
    one_col[::5] = 2
    one_row = np.zeros(n, dtype=np.int64)
    one_row[5] = 200
    return [_rand(n, 3, 11, w, colset=np.arange(40, n)),
            _rand(n, 3, 12, w, colset=np.arange(0, n - 40)),
            _rand(n, 3, 13, w, colset=np.r_[0:20, 280:n]),
            _rand(n, 3, 14, w, counts=empty_rows),
            _rand(n, 3, 15, w, counts=long_row),
            _rand(n, 3, 16, w, colset=np.array([17]), counts=one_col),
            _rand(n, 3, 17, w, counts=one_row)]


@pytest.mark.parametrize("weighted", [True, False])
def test_layout_planted(engine, weighted):
    layers = _planted(weighted)
    engine.set_layers(layers, symmetric=SYM_NO)
    _check(_read(engine, len(layers)), layers, verdicts=["directed"] * len(layers))


def _uncanonical(n=300):
    """Rows shuffled; duplicates kept as separate entries with different values, adjacent and
    not; a stored 0.0, a stored -0.0 and a stored NaN."""
    rng = np.random.default_rng(21)
    base = _sym(n, 6, 22, True)
    coo = base.tocoo()
    r = np.concatenate([coo.row, [3, 3, 3, 3, 10, 10, 10]])
    c = np.concatenate([coo.col, [9, 9, 4, 9, 1, 2, 3]])
    v = np.concatenate([coo.data, [1, 2, 3, 4, 0.0, -0.0, np.nan]]).astype(np.float32)
    order = np.argsort(r, kind="stable")  # row 3 ends ... 9, 9, 4, 9: adjacent and not
    special = _csr(n, np.bincount(r, minlength=n), c[order], v[order])
    tail = special.data[special.indptr[10]:special.indptr[11]][-3:]
    assert list(_bits(tail)) == [0x00000000, 0x80000000, 0x7FC00000]
    return [_shuffle_rows(base, rng), special, _shuffle_rows(special, rng)]


def test_layout_uncanonical(engine):
    layers = _uncanonical()
    engine.set_layers(layers, symmetric=SYM_NO)
    read = _read(engine, len(layers))
    _check(read, layers, verdicts=["directed"] * len(layers))
    for a, t in read[1:]:  # all three special values are still stored, on both copies
        for m in (a, t):
            bits = set(_bits(m.data).tolist())
            assert {0x00000000, 0x80000000, 0x7FC00000} <= bits


@pytest.mark.parametrize("symmetric", [SYM_NO, SYM_DETECT])
def test_empty_layers_next_to_others(engine, symmetric):
    n = 300
    E = sp.csr_matrix((n, n), dtype=np.float32)
    layers = [E, _rand(n, 3, 31, True), E, _rand(n, 3, 32, False), E]
    engine.set_layers(layers, symmetric=symmetric)
    read = _read(engine, len(layers))
    _check(read, layers)
    for k in (0, 2, 4):
        a, t = read[k]
        assert a.nnz == 0 and not a.indptr.any()
        if symmetric == SYM_NO:
            assert t is not None and t.nnz == 0 and not t.indptr.any()
        else:  # (an empty layer equals its transpose)
            assert t is None


def _unit_layers(n=300):
    """Unweighted; weighted; all ones except the very last value, an entry of column 7."""
    U = _rand(n, 5, 141, False)
    indices, data = U.indices.copy(), U.data.copy()
    indices[-1], data[-1] = 7, 2.0
    return [U, _rand(n, 5, 142, True), _copy(U, indices, data)]


def _spmm_bytes(eng, K, n, b=8):
    X = np.ones((n, b), dtype=np.float32)
    return [[eng.bench_spmm(k, X, transpose=tr, reps=1, want_y=False)[2] for tr in (False, True)]
            for k in range(K)]


def _expected_bytes(m, unit, b=8):
    """spmm_algo_bytes (csrc/engine.h): a unit CSR streams no values, 4 bytes an entry for 8."""
    nl, n = m.shape
    return (4.0 if unit else 8.0) * m.nnz + 8.0 * (nl + 1) + 4.0 * (n + nl) * b


def test_unweighted_flag(engine, multi3):
    """A unit layer reads back 1.0f whether or not the ingest saw that it is one, so the flag is
    read where it is reported: in the bytes ``bench_spmm`` counts for a product with the stored
    A and A^T.  One GPU and rank handles flag the whole layer; the multi handle flags each rank's
    rows of A and of A^T by themselves (``bench_spmm`` reports its rank 0)."""
    layers = _unit_layers()
    n = layers[0].shape[0]
    whole = [bool(np.all(A.data == 1.0)) for A in layers]
    assert whole == [True, False, False]
    engine.set_layers(layers, symmetric=SYM_NO)
    for k, A in enumerate(layers):
        assert _spmm_bytes(engine, 3, n)[k] == [_expected_bytes(A, whole[k]),
                                                _expected_bytes(_oracle_t(A), whole[k])], k

    def fn(eng, r):
        eng.set_layers(layers, symmetric=SYM_NO)
        return eng.dist_info(), _spmm_bytes(eng, 3, n)

    for (_, _, row0, nl), got in _run_ranks(2, fn):
        for k, A in enumerate(layers):
            assert got[k] == [_expected_bytes(_rows(A, row0, nl), whole[k]),
                              _expected_bytes(_rows(_oracle_t(A), row0, nl), whole[k])], (row0, k)
    multi3.set_layers(layers, symmetric=SYM_NO)
    got = _spmm_bytes(multi3, 3, n)
    for k, A in enumerate(layers):
        mine = [_rows(A, 0, 100), _rows(_oracle_t(A), 0, 100)]
        assert got[k] == [_expected_bytes(m, bool(np.all(m.data == 1.0))) for m in mine], k
    # (the 2.0 sits in the last row and in column 7: rank 0 holds it only in its rows of A^T)
    assert _rows(layers[2], 0, 100).data.max() == 1.0
    assert _rows(_oracle_t(layers[2]), 0, 100).data.max() == 2.0


# ---- b. the verdict of SYM_DETECT -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _verdict_cases(n=300):
    """(name, layer, exact verdict) for the clean inputs; the same list goes to every path."""
    rng = np.random.default_rng(41)
    W, U = _sym(n, 8, 42, True), _sym(n, 8, 43, False)
    L = _long_row(n, 44)
    nnz = W.nnz
    # one entry of the pattern moved inside its row (the row's last entry one column on: the
    # entry it mirrored has lost its partner), the row counts as they were
    p = next(int(W.indptr[r + 1] - 1) for r in range(n)
             if W.indptr[r + 1] > W.indptr[r] and W.indices[W.indptr[r + 1] - 1] < n - 1)
    moved = W.indices.copy()
    moved[p] += 1
    q = next(i for i in range(nnz // 2, nnz) if W.indices[i] != _row_of(W, i))
    counts = np.diff(W.indptr).copy()
    counts[_row_of(W, q)] -= 1
    last2 = int(L.indptr[n]) - 2
    assert L.indptr[n] - L.indptr[n - 1] >= 2
    return [
        ("sym weighted", W, "symmetric"),
        ("sym unit", U, "symmetric"),
        ("sym weighted, rows shuffled", _shuffle_rows(W, rng), "symmetric"),
        ("sym unit, rows shuffled", _shuffle_rows(U, rng), "symmetric"),
        ("one ulp, first entry", _ulp(W, 0), "directed"),
        ("one ulp, last entry", _ulp(W, nnz - 1), "directed"),
        ("one ulp, in the middle", _ulp(W, nnz // 2), "directed"),
        ("one entry moved", _copy(W, indices=moved), "directed"),
        ("one entry removed", _csr(n, counts, np.delete(W.indices, q), np.delete(W.data, q)),
         "directed"),
        ("symmetric pattern, all values differ",
         _copy(W, data=np.arange(1, nnz + 1, dtype=np.float32)), "directed"),
        ("row of 130, entries 63 and 64 swapped", _swap(L, int(L.indptr[7]) + 63), "symmetric"),
        ("the only descent in the last pair of the last row", _swap(L, last2), "symmetric"),
    ]


def _groups(cases, size=8):  # (a handle takes at most 8 layers)
    return [cases[i:i + size] for i in range(0, len(cases), size)]


def test_verdict_one_gpu(engine):
    """Lanes of csr_scan_kernel stride a row by 64: the descent between entries 63 and 64 of a
    row sits on that boundary.  A missed descent leaves the layer compared unsorted against its
    sorted transpose: judged directed."""
    for group in _groups(_verdict_cases()):
        layers = [c[1] for c in group]
        engine.set_layers(layers, symmetric=SYM_DETECT)
        _check(_read(engine, len(layers)), layers, verdicts=[c[2] for c in group],
               tag=[c[0] for c in group])


def test_verdict_one_ulp_beyond_one_workgroup(engine):
    """About 40 000 entries: csr_compare_kernel runs 20 workgroups of 256 threads, and entry
    30 000 is met in a later stride of its thread's loop."""
    S = _sym(2000, 20, 51, True)
    assert 36_000 < S.nnz < 44_000
    layers = [S, _ulp(S, 30_000), _ulp(S, S.nnz - 1), _ulp(S, 0)]
    engine.set_layers(layers, symmetric=SYM_DETECT)
    _check(_read(engine, 4), layers, verdicts=["symmetric"] + ["directed"] * 3)


@functools.lru_cache(maxsize=None)
def _safe_cases(n=300):
    """Inputs whose verdict may differ between the paths (module docstring)."""
    W = _sym(n, 8, 61, True)
    p = next(i for i in range(W.nnz) if W.indices[i] > _row_of(W, i))
    i, j = _row_of(W, p), int(W.indices[p])
    coo = W.tocoo()
    pq = next(k for k in range(W.nnz) if coo.row[k] == j and coo.col[k] == i)

    def pair(a, b):
        data = W.data.copy()
        data[p], data[pq] = a, b
        return _copy(W, data=data)

    keep = np.ones(W.nnz, dtype=bool)
    keep[[p, pq]] = False
    # (i, j) stored twice as 1, 2 and (j, i) twice as 2, 1: symmetric as a multiset and after
    # summing, not entry by entry
    dup = _from_coo(n, np.concatenate([coo.row[keep], [i, i, j, j]]),
                    np.concatenate([coo.col[keep], [j, j, i, i]]),
                    np.concatenate([coo.data[keep], [1, 2, 2, 1]]))
    return [pair(0.0, -0.0), pair(np.nan, np.nan), dup,
            _shuffle_rows(dup, np.random.default_rng(62))]


def test_safe_direction_one_gpu(engine):
    layers = _safe_cases()
    engine.set_layers(layers, symmetric=SYM_DETECT)
    _check_safe(_read(engine, len(layers)), layers, tag="one GPU")


def test_safe_direction_multi(multi3):
    layers = _safe_cases()
    multi3.set_layers(layers, symmetric=SYM_DETECT)
    _check_safe(_read(multi3, len(layers)), layers, tag="multi")


def test_safe_direction_ranks():
    layers = _safe_cases()
    for (_, _, row0, nl), read, _ in _on_ranks(2, layers, SYM_DETECT):
        _check_safe(read, layers, row0, nl, tag=("ranks", row0))


# ---- c. the other ingest paths ----------------------------------------------------------------
def _path_layers(n):
    """A directed and a symmetric layer, weighted and unit."""
    return [_rand(n, 5, 71, True), _rand(n, 5, 72, False), _sym(n, 8, 73, True),
            _sym(n, 8, 74, False)]


def _hollow(n, lo, hi, weighted, seed):
    """No entry in rows or columns [lo, hi): the rank that owns them gets nothing at all."""
    out = np.r_[0:lo, hi:n]
    counts = np.random.default_rng(seed).integers(0, 7, n)
    counts[lo:hi] = 0
    return _rand(n, 3, seed, weighted, colset=out, counts=counts)


@pytest.mark.parametrize("world,n", [(3, 193), (2, 1000), (3, 300)])
def test_rank_handles(world, n):
    """Every rank ingests the whole layer on its GPU and keeps rows [row0, row0 + nl) of A and
    of A^T.  n = 193 on 3 ranks: rows [65, 130) of the last two layers hold no entry at all.
    n = 300: the planted layers and the clean verdict cases."""
    if n == 300:
        cases = _verdict_cases()[:1] + _verdict_cases()[4:]
        sets = [(_planted(True), SYM_NO, ["directed"] * 7),
                (_planted(False)[:4] + _uncanonical(), SYM_NO, ["directed"] * 7),
                ([c[1] for c in cases[:8]], SYM_DETECT, [c[2] for c in cases[:8]])]
    else:
        layers = _path_layers(n)
        verdicts = ["directed", "directed", "symmetric", "symmetric"]
        if n == 193:
            layers += [_hollow(n, 65, 130, True, 75), _hollow(n, 65, 130, False, 76)]
            verdicts += ["directed", "directed"]
        sets = [(layers, SYM_DETECT, verdicts), (layers, SYM_NO, ["directed"] * len(layers))]
    for layers, symmetric, verdicts in sets:
        res = _on_ranks(world, layers, symmetric)
        R = -(-n // world)
        assert sorted(info[2] for info, _, _ in res) == [g * R for g in range(world)]
        assert sum(info[3] for info, _, _ in res) == n
        for (_, _, row0, nl), read, _ in res:
            _check(read, layers, verdicts, row0, nl, tag=(world, n, symmetric, row0))
            if n == 193 and row0 == 65:
                for a, t in read[4:]:
                    assert a.nnz == 0 and (t is None or t.nnz == 0)


@pytest.mark.parametrize("which", ["planted", "uncanonical", "n1000", "verdicts"])
def test_multi_handle(multi3, which):
    """The host twin: all N rows against the oracles, and the exact verdicts of the clean cases
    from ``host_csr_symmetric``."""
    if which == "verdicts":
        sets = [([c[1] for c in g], SYM_DETECT, [c[2] for c in g])
                for g in _groups(_verdict_cases())]
    elif which == "n1000":
        layers = _path_layers(1000)
        sets = [(layers, SYM_DETECT, ["directed", "directed", "symmetric", "symmetric"]),
                (layers, SYM_NO, ["directed"] * 4)]
    elif which == "planted":
        sets = [(_planted(w), SYM_NO, ["directed"] * 7) for w in (True, False)]
    else:
        E = sp.csr_matrix((300, 300), dtype=np.float32)
        sets = [(_uncanonical() + [E, _hollow(300, 100, 200, True, 77)], SYM_NO,
                 ["directed"] * 5)]
    for layers, symmetric, verdicts in sets:
        multi3.set_layers(layers, symmetric=symmetric)
        _check(_read(multi3, len(layers)), layers, verdicts, tag=(which, symmetric))


@functools.lru_cache(maxsize=None)
def _big_ones():
    """n = 65 537, 65 entries per row: 4 259 905 entries, just over 2^22, all ones except the
    very last value."""
    n, per = 65_537, 65
    rng = np.random.default_rng(81)
    vals = np.ones(n * per, dtype=np.float32)
    vals[-1] = 2.0
    A = _csr(n, np.full(n, per), rng.integers(0, n, n * per), vals)
    assert A.nnz > 1 << 22
    return A


def _check_big(eng):
    A = _big_ones()
    eng.set_layers([A], symmetric=SYM_NO)
    (a, t), = _read(eng, 1)
    assert _same_csr(a, A)
    assert _same_csr(t, _oracle_t(A))
    assert a.data[-1] == 2.0 and np.count_nonzero(_bits(a.data) != ONE) == 1
    assert np.count_nonzero(_bits(t.data) != ONE) == 1


def test_multi_handle_threaded_host_checks(multi3):
    """Above 2^22 entries ``host_indices_in_range`` runs in threads on the multi handle (every
    rank's own slice stays below the threshold of ``host_all_ones``); the one value that is not
    1.0 is the last one, so it reads back weighted."""
    _check_big(multi3)


def test_one_gpu_threaded_all_ones(engine):
    """The one-GPU ingest calls ``host_all_ones`` on the whole layer: above 2^22 entries the value
    that is not 1.0 lies in the last thread's chunk.  A layer taken for unweighted would read
    back 1.0 there."""
    _check_big(engine)


def test_multi_handle_threaded_symmetry(multi3):
    """Just over 2^20 entries ``host_csr_symmetric`` sums its hashes in threads: the clean layer
    is symmetric, and directed once its last entry's value is altered (the last thread's rows)."""
    S = _sym(20_000, 54, 91, True)
    assert 1 << 20 < S.nnz < 1.2 * (1 << 20)
    assert S.indices[-1] != _row_of(S, S.nnz - 1)  # (off the diagonal: its mirror stays as it was)
    data = S.data.copy()
    data[-1] += 1.0
    layers = [S, _copy(S, data=data)]
    multi3.set_layers(layers, symmetric=SYM_DETECT)
    _check(_read(multi3, 2), layers, verdicts=["symmetric", "directed"])


def test_set_layer_rows_block_comes_back():
    """``set_layer_rows``: the rank's block read back unchanged, the transpose refused (the
    caller declared the layers symmetric)."""
    n = 1000
    layers = [_sym(n, 8, 95, True), _sym(n, 8, 96, False)]

    def fn(eng, r):
        eng.set_layer_rows(n, 2, [])  # sets the partition first
        _, _, row0, nl = eng.dist_info()
        eng.set_layer_rows(n, 2, [A[row0:row0 + nl] for A in layers])
        return eng.dist_info(), _read(eng, 2), None

    for (_, _, row0, nl), read, _ in _run_ranks(2, fn):
        _check(read, layers, ["symmetric"] * 2, row0, nl, tag=row0)


# ---- d. column sums ---------------------------------------------------------------------------
def _directed(n):
    """Directed layers, unit and small-integer (sums far below 2^24: exact in any order)."""
    return [_rand(n, 5, 101, False), _rand(n, 5, 102, True), _planted(False)[2] if n == 300
            else _rand(n, 9, 103, False)]


def _column_sums(A):
    ref = np.bincount(A.indices, weights=A.data.astype(np.float64), minlength=A.shape[1])
    if np.all(A.data == 1.0):
        assert np.array_equal(ref, np.bincount(A.indices, minlength=A.shape[1]))
    assert ref.max() < 1 << 24
    return ref.astype(np.float32)


@pytest.mark.parametrize("n", [300, 1000])
def test_column_sums_one_gpu(engine, n):
    """The A^T copy of a directed unweighted layer keeps no value stream: csr_row_sums_kernel
    counts its entries (it read ``data`` there before: a null pointer on this handle)."""
    layers = _directed(n)
    engine.set_layers(layers)
    _check(_read(engine, 3), layers, verdicts=["directed"] * 3)
    for k, A in enumerate(layers):
        np.testing.assert_array_equal(engine.column_sums(k), _column_sums(A))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n", [300, 1000])
def test_column_sums_ranks(n, world):
    """(a rank's slice of a unit A^T copy allocated the value stream and copied nothing in)"""
    layers = _directed(n)
    for _, _, cs in _on_ranks(world, layers, SYM_DETECT, sums=True):
        for k, A in enumerate(layers):
            np.testing.assert_array_equal(cs[k], _column_sums(A))


@pytest.mark.parametrize("n", [300, 1000])
def test_column_sums_multi(multi3, n):
    layers = _directed(n)
    multi3.set_layers(layers)
    for k, A in enumerate(layers):
        np.testing.assert_array_equal(multi3.column_sums(k), _column_sums(A))


def test_column_sums_after_reloading_a_layer_as_unit(engine):
    """The raw library: a directed weighted layer into k = 0, then a directed unit layer into the
    same k without ``n2v2r_set_num_layers`` in between.  The weighted load's A^T values are still
    allocated; the sums are the unit layer's."""
    from node2vec2rank_amd import _lib
    n = 300
    W, U = _rand(n, 6, 111, True), _rand(n, 4, 112, False)
    assert U.nnz < W.nnz
    assert engine.lib.n2v2r_set_num_layers(engine.h, 1, n) == _lib.OK
    engine.n, engine.num_layers, engine.storage = n, 1, "csr"
    for A in (W, U):
        st = engine.lib.n2v2r_set_layer_csr(
            engine.h, 0, n, int(A.nnz), np.ascontiguousarray(A.indptr, dtype=np.int64),
            np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float32), _lib.SYM_DETECT)
        assert st == _lib.OK, engine._err()
        _check(_read(engine, 1), [A], verdicts=["directed"])
        np.testing.assert_array_equal(engine.column_sums(0), _column_sums(A))


def test_dedi_of_directed_unweighted_graphs():
    from node2vec2rank_amd.model import N2V2R
    n = 300
    graphs = [_rand(n, 5, 121, False), _rand(n, 5, 122, False)]
    config = dict(embed_dimensions=[4], distance_metrics=["cosine"], comp_strategy="sequential",
                  seed=1, verbose=-1, save_dir=None)
    model = N2V2R(graphs=graphs, nodes=[f"v{i}" for i in range(n)], config=config)
    out = model.degree_difference_ranking()
    dedi, absdedi = orc.degree_difference(graphs)["1"]
    assert dedi.dtype == np.float32 and np.any(dedi != 0)
    assert list(out) == ["1"]
    np.testing.assert_array_equal(out["1"]["DeDi"].to_numpy(), dedi)
    np.testing.assert_array_equal(out["1"]["absDeDi"].to_numpy(), absdedi)
    np.testing.assert_array_equal(dedi, _column_sums(graphs[0]) - _column_sums(graphs[1]))


# ---- e. the dense verdict, visible after to_csr() ---------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_dense_verdict(engine, n):
    """Symmetric except one entry at (n - 1, 0): directed, and the A^T copy compacted from the
    dense A^T is ``csr_matrix(A.T)``; the unmodified layer is symmetric.  A NaN diagonal and a
    -0.0 against a +0.0 follow the safe-direction rule (neither zero is stored)."""
    S = _symmetric(n, n * n // 10, 130 + n)
    D = S.copy()
    D[n - 1, 0] = D[n - 1, 0] + 1.0
    assert D[n - 1, 0] != D[0, n - 1] and D[n - 1, 0] != 0
    N = S.copy()
    N[5, 5] = np.nan
    Z = S.copy()
    Z[3, 7], Z[7, 3] = -0.0, 0.0
    layers = [S, D, N, Z]
    engine.set_layers(layers, storage="dense")
    engine.to_csr()
    read = _read(engine, 4)
    inputs = [sp.csr_matrix(A) for A in layers]
    transposed = [sp.csr_matrix(np.ascontiguousarray(A.T)) for A in layers]
    for k in range(4):
        assert _same_csr(read[k][0], inputs[k]), (n, k)
    assert read[0][1] is None
    assert read[1][1] is not None and _same_csr(read[1][1], transposed[1])
    for k in (2, 3):
        a, t = read[k]
        if t is None:
            assert _canon_equal(a, transposed[k]), (n, k)
        else:
            assert _same_csr(t, transposed[k]), (n, k)
