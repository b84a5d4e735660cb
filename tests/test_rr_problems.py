"""The Krylov-Schur problem generator of the Rayleigh-Ritz stage tests (rr_problems.py), checked on
the CPU for the shapes test_gpu_rr_stage.py uses: what ``assemble`` drops of the dense projection
is rounding (<= 1e-12 ||H||), the assembled matrix has the prescribed spectrum (to 1e-12 ||H||),
and a prescribed gap ladder comes out within 5 % of the gaps set, down to 1e-11 tn."""
import numpy as np
import pytest

import rr_problems as rp


def _norm(H):
    return np.abs(np.linalg.eigvalsh(H)).max()


@pytest.mark.parametrize("c,kp", rp.SHAPES)
def test_assemble_drops_rounding_only_and_keeps_the_spectrum(c, kp):
    pr = rp.case("shape", c, kp)
    H = rp.assemble(pr["hband"], c, kp, pr["theta"])
    nh = _norm(H)
    assert np.array_equal(H, H.T)
    assert np.abs(H - pr["Hdense"]).max() <= 1e-12 * nh
    w = np.sort(np.linalg.eigvalsh(H))[::-1]
    assert np.abs(w - np.sort(pr["ev"])[::-1]).max() <= 1e-12 * nh
    tn = rp.gershgorin_norm(H)
    assert nh <= tn <= 3.0 * nh  # (the triage saw 1.3 .. 2.4)


def test_assemble_reads_the_layout_the_kernels_read():
    """Entry by entry against rs_band_entry / rr_band_expand_kernel, restated: an hband of
    distinct values, so a transposed or shifted read shows."""
    c, kp, W = 40, 16, 8
    n = rp.hband_len(c, kp)
    hb = np.arange(1.0, n + 1.0)
    theta = -np.arange(1.0, kp + 1.0)
    H = rp.assemble(hb, c, kp, theta)

    def entry(i, col):  # kp <= col <= i
        if i - col > W:
            return 0.0
        j, r = i // W, i % W
        if j == kp // W:
            cc = col - kp
            return 0.5 * (hb[(kp + r) * W + cc] + hb[(kp + cc) * W + r])
        G = hb[(kp + W) * W + (j - kp // W - 1) * 2 * W * W:]
        if col >= j * W:
            cc = col - j * W
            return 0.5 * (G[(W + r) * W + cc] + G[(W + cc) * W + r])
        cc = col - (j - 1) * W
        return G[cc * W + r] if r <= cc else 0.0

    for i in range(c):
        for j in range(c):
            lo, hi = min(i, j), max(i, j)
            if hi < kp:
                want = theta[i] if i == j else 0.0
            elif lo < kp:
                want = hb[lo * W + (hi - kp)] if hi < kp + W else 0.0
            else:
                want = entry(hi, lo)
            assert H[i, j] == want, (i, j)


@pytest.mark.parametrize("c,kp", rp.GAP_SHAPES)
@pytest.mark.parametrize("g", [1e-11, 1.1e-9, 1e-6])
def test_gap_ladder_is_reproduced(c, kp, g):
    pr = rp.case("gap", c, kp, g)
    H, w, _, tn = rp.case_reference("gap", c, kp, g)
    nh = np.abs(w).max()
    assert np.abs(H - pr["Hdense"]).max() <= 1e-12 * nh
    assert np.abs(w - np.sort(pr["ev"])[::-1]).max() <= 1e-12 * nh
    a, n = rp.LADDER
    gaps = -np.diff(w[a:a + n])
    assert np.abs(gaps / pr["gap"] - 1.0).max() <= 0.05, gaps / pr["gap"]
    assert abs(pr["gap"] / tn / g - 1.0) <= 0.05  # in units of the final matrix's tn
    # the ladder's neighbours stay far: the next gaps are the grid's
    assert min(w[a - 1] - w[a], w[a + n - 1] - w[a + n]) > 100 * pr["gap"]


@pytest.mark.parametrize("name", rp.EDGES + rp.ZEROS + rp.SPECTRA)
def test_variants(name):
    kind = "edge" if name in rp.EDGES else "zero" if name in rp.ZEROS else "spectrum"
    pr = rp.case(kind, name)
    c, kp, p = pr["c"], pr["kp"], pr["p"]
    H, w, V, tn = rp.case_reference(kind, name)
    nh = np.abs(w).max()
    if pr["ev"] is not None:
        assert np.abs(w - np.sort(pr["ev"])[::-1]).max() <= 1e-12 * nh
    if name == "triple_p":
        assert w[p - 2] - w[p] <= 1e-12 * nh < w[p - 3] - w[p - 2]
    if name == "cluster0":
        assert w[0] - w[2] <= 1e-12 * nh
    if name == "pair":
        assert w[20] - w[21] <= 1e-12 * nh
    if name == "fold24":
        k = np.nonzero(np.abs(w - pr["theta"][10]) <= 1e-12 * nh)[0]
        assert k.size == 24 and k[0] < p
    if name in ("R", "both"):
        assert not H[160:, :160].any()
    if name in ("G0", "both"):
        assert not H[:30, 30:].any()
    if name == "diag":
        assert not (H - np.diag(np.diag(H))).any()
        assert np.diff(np.sort(np.diag(H))).min() > 1e-6 * tn
    if name == "negative":
        assert w[0] < 0
    if name == "indefinite":
        assert w[0] > 0 > w[-1]
    if name == "graded":
        assert w[-1] > 0 and w[0] / w[-1] > 5e11
