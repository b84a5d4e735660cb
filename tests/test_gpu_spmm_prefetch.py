"""The flat tiled SpMM's uniform words (a phase's block record, a window's two offsets) at the
shapes where fetching them can go wrong: one application W = sum_k A_k (A_k^T X) through
``n2v2r_gram_apply`` with the tiled form forced at small N, against fp64 products at
``test_gpu_gram_apply``'s bars (stage 1 against |A_k^T| |X|, stage 2 against the GPU's own Z;
1e-5 s + 1e-6 per element), and the register-window form (``N2V2R_SPMM_VW=2``) byte-equal to the
LDS-only one (``=0``).

* N = 2,049 and 4,160 at mean degree 3: most (window, block) runs are empty, 2,049 is no multiple
  of the 64 window rows (4,160 is 65 windows), every tile has fewer windows than its 16 waves,
  and the register-window form's last tile has waves without a window.
* N = 70,000 at mean degree 20 with 4 and with 64 column blocks, unit layers and weighted ones,
  the first layer directed (stage 1 walks the transposed blocks, stage 2 the plain ones), K = 1
  and K = 3: the last phase of a layer hands over to the first phase of the next, and stage 2
  sums the layers in one accumulator.
* all edges among the first, or the last, quarter of the nodes at 4 column blocks: the last
  three, or the first three, blocks of every window are empty.

Inputs are seeded; every case prints the fractions of its bars it reached (``pytest -s``)."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_gram_apply import _apply_twice, _check, _panel, _same_bits

pytestmark = pytest.mark.gpu


def _layer(seed, n, deg, kind, lo=0, hi=None):
    """ER-like layer of mean degree `deg` with every edge among the nodes lo .. hi - 1.
    kind: "d" directed or "s" symmetric, then "u" unit or "w" weighted."""
    hi = n if hi is None else hi
    rng = np.random.default_rng(seed)
    sym = kind[0] == "s"
    m = n * deg // (2 if sym else 1)
    rows, cols = rng.integers(lo, hi, size=m), rng.integers(lo, hi, size=m)
    A = sp.csr_matrix((rng.uniform(0.5, 2.0, m).astype(np.float32), (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    if sym:
        A = (A + A.T).tocsr()
    if kind[1] == "u":
        A.data[:] = 1.0
    return A


def _tiled_both(engine, monkeypatch, group, layers, nb):
    """The application in the LDS-only and in the register-window form: both named by `info`,
    the first checked against fp64, the second byte-equal to it."""
    n = layers[0].shape[0]
    monkeypatch.setenv("N2V2R_SPMM_CB", "1")
    monkeypatch.setenv("N2V2R_SPMM_TILE_NB", str(nb))
    monkeypatch.delenv("N2V2R_SPMM_WBITS", raising=False)
    engine.set_layers(layers)
    X = _panel(n, 8, seed=n % 97)
    out = {}
    for vw in (0, 2):
        monkeypatch.setenv("N2V2R_SPMM_VW", str(vw))
        W, Z, info = _apply_twice(engine, X)
        assert info["form"] == 5 and (info["rpw1"], info["rpw2"]) == (0, 0), info
        assert info["tile_nb"] == nb and info["tile_wb"] == 6 and info["tile_rows"] > 0, info
        out[vw] = (W, Z)
    _check(group, group, layers, X, *out[0])
    assert _same_bits(out[0][1], out[2][1]), "Z differs between the LDS-only and register windows"
    assert _same_bits(out[0][0], out[2][0]), "W differs between the LDS-only and register windows"


@pytest.mark.parametrize("n", [2049, 4160])
def test_sparse_small(engine, monkeypatch, n):
    layers = [_layer(500 + n, n, 3, "du"), _layer(501 + n, n, 3, "dw")]
    _tiled_both(engine, monkeypatch, f"prefetch n{n}", layers, 4)


_BIG = {}  # (nb) -> the three layers at N = 70,000, built once


def _big_layers(nb):
    if nb not in _BIG:
        vals = "u" if nb == 4 else "w"
        _BIG[nb] = [_layer(600 + 10 * nb + k, 70_000, 20, ("d" if k == 0 else "s") + vals)
                    for k in range(3)]
    return _BIG[nb]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("nb", [4, 64])
def test_layer_hand_over(engine, monkeypatch, nb, K):
    """nb = 4: unit layers; nb = 64: weighted ones.  Layer 0 is directed."""
    layers = _big_layers(nb)[:K]
    assert abs(layers[0] - layers[0].T).nnz != 0
    _tiled_both(engine, monkeypatch, f"prefetch nb{nb} K{K}", layers, nb)


@pytest.mark.parametrize("where", ["first", "last"])
def test_empty_edge_blocks(engine, monkeypatch, where):
    n, nb = 8_000, 4
    lo, hi = (0, n // nb) if where == "first" else (n - n // nb, n)
    layers = [_layer(700, n, 6, "du", lo, hi), _layer(701, n, 6, "sw", lo, hi)]
    for A in layers:  # nothing outside the quarter, as a row or as a column
        coo = A.tocoo()
        assert coo.row.min() >= lo and coo.row.max() < hi
        assert coo.col.min() >= lo and coo.col.max() < hi
    _tiled_both(engine, monkeypatch, f"prefetch edges {where}", layers, nb)
