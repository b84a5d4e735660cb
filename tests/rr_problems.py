"""Projected matrices of block Krylov-Schur cycles for the Rayleigh-Ritz stage tests
(test_rr_problems.py checks the generator on the CPU, test_gpu_rr_stage.py uses it).

``ks_problem`` runs the cycle itself on the host in fp64: a symmetric A with a prescribed
spectrum, block Lanczos at b = 8 with two full re-orthogonalisations per block, a restart that keeps
the top ``kp`` Ritz vectors X, and Lanczos again from the residual block E against X until the basis
has c = len(ev) columns.  What it returns is what the solver keeps of such a cycle -- the band
columns ``hband`` in the layout n2v2r_rr_band_top documents and the kept Ritz values -- so the
kept Ritz vectors are as converged, and their couplings to E as graded, as a real cycle makes them.

``assemble`` builds the matrix the kernels read from ``hband`` (rs_band_entry and
rr_band_expand_kernel in rr_sturm.hip): diagonal blocks symmetrised as 0.5 (G + G^T), only the upper
triangle of each coupling R_j, zero outside the arrow and the band.  That matrix, not A, is what a
reference has to decompose: the kernels see nothing else.

Gaps are given in units of ``tn``, the Gershgorin norm rr_sturm_prep_kernel computes (the largest
|centre| + radius over the rows of the assembled matrix; ``gershgorin_norm``): ``with_ladder``
builds once, reads tn, sets the ladder and builds again.
"""
import functools

import numpy as np

B = 8


def hband_len(c, kp):
    return (kp + B) * B + (c // B - kp // B - 1) * 2 * B * B


def _orth_block(W, Q):
    """W orthogonalised against the columns of Q twice, then QR: (block, R)."""
    for _ in range(2):
        if Q.shape[1]:
            W = W - Q @ (Q.T @ W)
    return np.linalg.qr(W)


def _lanczos(A, Q, upto):
    """Block Lanczos with full re-orthogonalisation: blocks A Q_last against all of Q until it
    has ``upto`` columns."""
    while Q.shape[1] < upto:
        Z, _ = _orth_block(A @ Q[:, -B:], Q)
        Q = np.hstack([Q, Z])
    return Q


def ks_problem(ev, kp, c1, seed):
    """The projected matrix of one Krylov-Schur cycle of A = V diag(ev) V^T, order c = len(ev).

    kp = 0: plain block Lanczos to c columns (a fit's first cycle; c1 is ignored).  kp > 0: Lanczos
    to c1 columns, host eigh of the projection, the top kp Ritz vectors X kept, E the next Lanczos
    block (orthogonal to the whole first basis), Lanczos from E against [X E ...] to c columns.
    Returns a dict: hband, theta (kp kept Ritz values, descending; None at kp = 0), H (the dense
    Q^T A Q, symmetrised), c, kp."""
    ev = np.asarray(ev, dtype=np.float64)
    c = ev.size
    assert c % B == 0 and kp % B == 0 and kp + B <= c
    rng = np.random.default_rng(seed)
    V, _ = np.linalg.qr(rng.standard_normal((c, c)))
    A = (V * ev) @ V.T
    A = 0.5 * (A + A.T)
    Q0, _ = np.linalg.qr(rng.standard_normal((c, B)))
    theta = None
    if kp == 0:
        Q = _lanczos(A, Q0, c)
    else:
        assert c1 % B == 0 and kp <= c1 and c1 + B <= c
        Q1 = _lanczos(A, Q0, c1)
        T = Q1.T @ A @ Q1
        tw, tz = np.linalg.eigh(0.5 * (T + T.T))
        top = np.argsort(tw)[::-1][:kp]
        X = Q1 @ tz[:, top]
        E, _ = _orth_block(A @ Q1[:, -B:], Q1)
        E, _ = _orth_block(E, X)  # (X is inside span(Q1): this only removes rounding)
        Q = _lanczos(A, np.hstack([X, E]), c)
        theta = np.einsum("ij,ij->j", X, A @ X)
    H = Q.T @ A @ Q
    H = 0.5 * (H + H.T)
    j0 = kp // B
    cols = [H[:kp + B, kp:kp + B]]
    for j in range(j0 + 1, c // B):
        cols.append(H[(j - 1) * B:(j + 1) * B, j * B:(j + 1) * B])
    hband = np.concatenate([m.ravel() for m in cols])
    assert hband.size == hband_len(c, kp)
    return {"hband": hband, "theta": theta, "H": H, "c": c, "kp": kp}


def assemble(hband, c, kp, theta):
    """The c x c matrix the Rayleigh-Ritz kernels read from the band columns."""
    hband = np.asarray(hband, dtype=np.float64)
    H = np.zeros((c, c))
    j0 = kp // B
    G0 = hband[:(kp + B) * B].reshape(kp + B, B)
    if kp:
        H[np.arange(kp), np.arange(kp)] = theta[:kp]
        H[:kp, kp:kp + B] = G0[:kp]
        H[kp:kp + B, :kp] = G0[:kp].T
    D = G0[kp:]
    H[kp:kp + B, kp:kp + B] = 0.5 * (D + D.T)
    off = (kp + B) * B
    for j in range(j0 + 1, c // B):
        G = hband[off:off + 2 * B * B].reshape(2 * B, B)
        off += 2 * B * B
        o = j * B
        D = G[B:]
        H[o:o + B, o:o + B] = 0.5 * (D + D.T)
        # G[:8] = Q_{j-1}^T M Q_j = R_j^T; H[o + r][o - 8 + cc] = G[cc][r] for r <= cc
        R = np.triu(G[:B].T)
        H[o:o + B, o - B:o] = R
        H[o - B:o, o:o + B] = R.T
    return H


def gershgorin_norm(H):
    """tn as rr_sturm_prep_kernel computes it: max over rows of |H_ii| + sum_{j != i} |H_ij|."""
    a = np.abs(H)
    return float(a.sum(axis=1).max())


def uniform_ev(c, lo=10.0, hi=100.0, seed=0):
    """c descending values on [lo, hi]: an even grid, each point moved by at most 15 % of the
    spacing, so no two values come closer than 70 % of it by accident."""
    rng = np.random.default_rng(1000 + seed)
    h = (hi - lo) / (c - 1)
    return np.linspace(hi, lo, c) + 0.3 * h * (rng.random(c) - 0.5)


def ladder_ev(ev, first, count, gap):
    """ev with ev[first + i] = ev[first] - i * gap for i < count."""
    ev = np.array(ev, dtype=np.float64)
    ev[first:first + count] = ev[first] - gap * np.arange(count)
    return ev


def with_ladder(ev, kp, c1, seed, first, count, g):
    """A problem whose eigenvalues first .. first + count - 1 are ``g * tn`` apart: built once to
    read tn, then again with the ladder set (and once more if the ladder moved tn by over 1 %:
    the basis, and with it the row sums, follow the spectrum).  Returns (problem, gap): the
    absolute gap set."""
    pr = ks_problem(ev, kp, c1, seed)
    for _ in range(3):
        tn = gershgorin_norm(assemble(pr["hband"], pr["c"], kp, pr["theta"]))
        gap = g * tn
        pr = ks_problem(ladder_ev(ev, first, count, gap), kp, c1, seed)
        tn2 = gershgorin_norm(assemble(pr["hband"], pr["c"], kp, pr["theta"]))
        if abs(tn2 - tn) <= 0.01 * tn:
            break
    return pr, gap


# ---- deliberately degenerate variants: edits of hband after generation -----------------------
def zero_coupling(hband, c, kp, j):
    """R_j = 0 for block j (kp / 8 < j < c / 8): the band splits between blocks j - 1 and j."""
    assert kp // B < j < c // B
    out = np.array(hband, dtype=np.float64)
    off = (kp + B) * B + (j - kp // B - 1) * 2 * B * B
    out[off:off + B * B] = 0.0
    return out


def scale_g0_rows(hband, rows, factor):
    """Rows ``rows`` of G0 (the couplings of those kept Ritz vectors to E) times ``factor``
    (0: exactly converged vectors)."""
    out = np.array(hband, dtype=np.float64)
    for r in rows:
        out[r * B:(r + 1) * B] *= factor
    return out


def diagonal_only(hband, c, kp):
    """Every coupling zero and every diagonal block reduced to its diagonal."""
    out = np.zeros_like(np.asarray(hband, dtype=np.float64))
    src = np.asarray(hband, dtype=np.float64)
    d = np.arange(B)
    o = kp * B
    out[o:o + B * B].reshape(B, B)[d, d] = src[o:o + B * B].reshape(B, B)[d, d]
    off = (kp + B) * B
    for _ in range(kp // B + 1, c // B):
        o = off + B * B
        out[o:o + B * B].reshape(B, B)[d, d] = src[o:o + B * B].reshape(B, B)[d, d]
        off += 2 * B * B
    return out


# ---- the reference -----------------------------------------------------------------------------
def matmul_ld(H, V):
    """H @ V accumulated in np.longdouble (each block of 8 rows over its non-zero columns only:
    H is an arrow + band matrix).  A residual H v - w v of an fp64 eigenpair sits at the rounding
    level of an fp64 product; this resolves it."""
    Hx, Vx = H.astype(np.longdouble), V.astype(np.longdouble)
    out = np.zeros((H.shape[0], V.shape[1]), dtype=np.longdouble)
    for o in range(0, H.shape[0], B):
        nz = np.flatnonzero(np.any(H[o:o + B] != 0, axis=0))
        out[o:o + B] = Hx[o:o + B][:, nz] @ Vx[nz]
    return out


def residuals(H, w, Y):
    """||H y_j - w_j y_j|| / ||y_j|| of fp64 pairs, evaluated in np.longdouble."""
    R = matmul_ld(H, Y) - Y.astype(np.longdouble) * w.astype(np.longdouble)
    return (np.sqrt((R * R).sum(axis=0)).astype(np.float64) / np.linalg.norm(Y, axis=0))


def groups(w, tn, p):
    """(a, b, gap): the runs [a, b) of descending eigenvalues w chained by gaps below 1e-6 tn that
    start among the first p, and each run's distance to the rest of the spectrum."""
    c = w.size
    cuts = np.nonzero(-np.diff(w) >= 1e-6 * tn)[0] + 1
    bounds = np.concatenate([[0], cuts, [c]])
    for a, b in zip(bounds[:-1], bounds[1:]):
        if a >= p:
            break
        gap = min(w[a - 1] - w[a] if a > 0 else np.inf, w[b - 1] - w[b] if b < c else np.inf)
        yield int(a), int(b), float(gap)


def refine(H, w, V, tn):
    """eigh's vectors with their first-order error against the other groups removed, as
    np.longdouble.  eigh leaves each v_i with a residual r_i of a few eps ||H||, so v_i is off its
    eigenvector by sum_k v_k (v_k^T r_i) / (w_i - w_k): about eps ||H|| / gap, 1e-10 at a gap of
    1e-6 tn -- as much as the vectors under test are allowed -- and rounding the corrected vector
    to fp64 would put eps ||H|| / gap back.  r_i comes from matmul_ld, the correction is applied
    for k outside i's group (``groups``), and each group is orthonormalised again (Gram-Schmidt,
    twice, in np.longdouble)."""
    ld = np.longdouble
    R = (matmul_ld(H, V) - V.astype(ld) * w.astype(ld)).astype(np.float64)
    C = V.T @ R                      # C[k, i] = v_k^T r_i
    D = w[None, :] - w[:, None]      # D[k, i] = w_i - w_k
    gid = np.zeros(w.size, dtype=np.int64)
    runs = list(groups(w, tn, w.size))
    for n, (a, b, _) in enumerate(runs):
        gid[a:b] = n
    other = gid[:, None] != gid[None, :]
    A = np.where(other, C / np.where(other, D, 1.0), 0.0)
    V2 = V.astype(ld) + (V @ A).astype(ld)  # (the correction is ~1e-10: fp64 carries it)
    for a, b, _ in runs:
        for j in range(a, b):
            for _ in range(2):
                if j > a:
                    V2[:, j] -= V2[:, a:j] @ (V2[:, a:j].T @ V2[:, j])
            V2[:, j] /= np.sqrt((V2[:, j] * V2[:, j]).sum())
    return V2


def reference(hband, c, kp, theta):
    """fp64 eigh of the assembled matrix, the vectors refined into np.longdouble (``refine``):
    (H, w descending, V columns to match, tn)."""
    H = assemble(hband, c, kp, theta)
    w, V = np.linalg.eigh(H)
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    tn = gershgorin_norm(H)
    return H, w, refine(H, w, V, tn), tn


def default_c1(c, kp):
    """Columns of the first basis: half-way between kp and c, a multiple of 8 with room for E
    (kp <= c1 <= c - 8).  At c = kp + 8 that leaves c1 = kp: every Ritz vector of the first basis
    is kept and the second holds nothing but [X E].  None at kp = 0."""
    if kp == 0:
        return None
    c1 = C1.get((c, kp), ((kp + c) // 2) // B * B)
    return min(max(c1, kp), c - B)


# ---- the cases of test_gpu_rr_stage.py (test_rr_problems.py checks the generator on them) ------
C1 = {(256, 80): 160, (512, 184): 256, (768, 600): 680, (96, 80): 88}
# (16, 8): the smallest c - kp = 8; kp = 8 with c - kp = 8 .. 72: the nine tail lengths of the
# 9-step elimination; (640, 184): the reducing path's last c; (768, 0): the largest LDS
SHAPES = ([(16, 0)] + [(8 + 8 * k, 8) for k in range(1, 10)] +
          [(96, 80), (256, 0), (256, 80), (384, 160), (512, 184), (520, 192), (640, 184),
           (768, 0), (768, 600), (768, 760)])
GAPS = [1e-11, 1e-10, 5e-10, 9e-10, 1.1e-9, 2e-9, 1e-8, 1e-7, 1e-6]
GAP_SHAPES = [(256, 80), (256, 0), (768, 600)]
LADDER = (4, 5)  # eigenvalues 4 .. 8
EDGES = ["triple_p", "cluster0", "pair", "fold24"]
ZEROS = ["R", "G0", "both", "diag"]
SPECTRA = ["indefinite", "negative", "graded"]
BASE = (256, 80)  # the shape of the edge, zero-coupling and spectrum cases


@functools.lru_cache(maxsize=2)
def case(kind, *args):
    """One test problem: a dict with hband, theta, c, kp, p = kp + 8 and, for the ladder and
    cluster cases, what was prescribed (ev, gap, group).  Cached: the forms of a case share it."""
    extra = {}
    if kind == "shape":
        c, kp = args
        ev = uniform_ev(c)
        pr = ks_problem(ev, kp, default_c1(c, kp), seed=c + kp)
    elif kind == "gap":
        c, kp, g = args
        ev0 = uniform_ev(c)
        pr, gap = with_ladder(ev0, kp, default_c1(c, kp), c + kp, LADDER[0], LADDER[1], g)
        ev = ladder_ev(ev0, LADDER[0], LADDER[1], gap)
        extra = {"gap": gap, "g": g}
    else:
        c, kp = BASE
        c1, seed = default_c1(c, kp), c + kp
        p = kp + B
        ev = uniform_ev(c)
        name, = args
        if kind == "edge":
            if name == "triple_p":  # a cluster that straddles the last wanted index p - 1
                ev[p - 1] = ev[p] = ev[p - 2]
            elif name == "cluster0":
                ev[1] = ev[2] = ev[0]
            elif name == "pair":
                ev[21] = ev[20]
            pr = ks_problem(ev, kp, 200 if name == "fold24" else c1, seed)
            if name == "fold24":
                # a band of half-width 8 cannot hold a multiplicity above 8: 24 equal kept Ritz
                # values of a converged first basis instead, their couplings scaled to 1e-12
                pr["theta"][10:34] = pr["theta"][10]
                pr["hband"] = scale_g0_rows(pr["hband"], range(10, 34), 1e-12)
                ev = None
        elif kind == "zero":
            pr = ks_problem(ev, kp, c1, seed)
            hb = pr["hband"]
            if name in ("R", "both"):
                hb = zero_coupling(hb, c, kp, 20)
            if name in ("G0", "both"):
                hb = scale_g0_rows(hb, range(30), 0.0)
            if name == "diag":
                hb = diagonal_only(hb, c, kp)
            pr["hband"] = hb
            ev = None
        elif kind == "spectrum":
            if name == "indefinite":
                ev = uniform_ev(c, -100.0, 100.0)
            elif name == "negative":
                ev = uniform_ev(c, -100.0, -10.0)
            else:
                ev = 100.0 * 10.0 ** (-12.0 * np.arange(c) / c)
            pr = ks_problem(ev, kp, c1, seed)
        else:
            raise KeyError(kind)
    out = {"hband": pr["hband"], "theta": pr["theta"], "c": pr["c"], "kp": pr["kp"],
           "p": pr["kp"] + B, "ev": ev, "Hdense": pr["H"]}
    out.update(extra)
    return out


@functools.lru_cache(maxsize=2)
def case_reference(kind, *args):
    """``reference`` of ``case(kind, *args)`` (cached likewise)."""
    pr = case(kind, *args)
    return reference(pr["hband"], pr["c"], pr["kp"], pr["theta"])
