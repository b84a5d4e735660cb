"""Every form of the Rayleigh-Ritz stage on its own (``n2v2r_rr_stage``) against fp64
``numpy.linalg.eigh`` of the matrix the kernels read, with a report of the form that ran.

The forms: 0 Sturm (rr_sturm.hip: multisection on Sturm counts + inverse iteration on the unreduced
arrow + band matrix), 1 BandReduce (rr_band.hip: arrow reduction, bulge chase, tridiagonal
bisection / inverse iteration, back-transform), 2 DenseFromBand (rr_band_expand_kernel + the dense
steps of rr.hip), and -1: Sturm, then what the solver takes after a failed Sturm result.  The
problems are projected matrices of host-run Krylov-Schur cycles (rr_problems.py), the reference is
eigh of ``assemble(hband)``: the kernels see nothing but hband.

Bounds (none is compared against the code under test).  ||H|| = the largest |reference
eigenvalue|, tn = the Gershgorin norm rr_sturm_prep_kernel computes, restated on the host,
eps = 2^-52.  The reference's own error is taken as e_ref = 8 c eps ||H|| (LAPACK's backward bound
with margin).  r_j = ||H y_j - w_j y_j|| / ||y_j|| is computed on the host from the fp64 vectors Y
where the form returns them (Sturm), else from the fp32 S (then r_j is about 1e-7 ||H||, and the
ceiling below is the eigenvalue bound that binds).  The products are accumulated in np.longdouble:
Sturm's residuals are a few eps ||H||, the rounding level of an fp64 product.  For the same
reason the reference's vectors are eigh's with their first-order error removed
(rr_problems.refine, kept in np.longdouble): eigh's own sit eps ||H|| / gap from the eigenvectors, which at a gap of
1e-6 tn is as much as the subspace bound allows the vectors under test (unrefined, the Sturm
vectors of the (256, 80) ladder at 1e-6 tn measured 1.6e-10 from eigh's against a bound of
1.0e-10, with residuals of 1.7e-14).
  * eigenvalues: |w_j - ref_j| <= r_j + e_ref (a Ritz value lies within its residual of an
    eigenvalue; the Sturm count fixes the index) and <= 1e-10 ||H|| (the ceiling the older stage
    tests hold);
  * contract: a Sturm result with sturm_err == 0 has r_j <= 1e-8 tn for every j (the kernel's own
    acceptance rule, so a wrong on-device residual shows);
  * max |S^T S - I| < 5e-6 and max |H S - S w| < 5e-6 ||H|| on the fp32 S (what the consumer
    needs; the older stage tests' figures), in every case, the gap sweep included;
  * subspaces: for every group of reference eigenvalues separated from the rest by
    gap_g >= 1e-6 tn, ||(I - V_g V_g^T) Y_g||_2 <= max_j r_j / gap_g + 64 c eps (Davis-Kahan);
    a group that straddles the last wanted index is compared through its wanted members;
  * Sturm's fp64 vectors have unit norm to 16 eps c.
A column no launch wrote is NaN (the entry fills its outputs with NaN bytes first) and fails these.

The Sturm form may give up (sturm_err = 1: the fallback exists for that).  A Sturm-only case
(form 0) that did skips its result assertions; ``test_zz_sturm_only_giveups`` caps such cases at
10 % of the Sturm-only cases run, and the shape sweep allows none at kp <= 184, the shape of every
ordinary cycle.  Under form -1 nothing is skipped.

Measured per case (not asserted): the worst r_j / (c eps tn) and the worst |Y^T Y - I| (Sturm's
fp64 vectors), kept in ``REPORT``; with N2V2R_RR_STAGE_REPORT=<path> the last test writes them as
JSON (profiles/rr_stage.json is such a run on an MI355X).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.linalg

import rr_problems as rp
from conftest import fixture_layers, load_fixture

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
AS_FIT, STURM, REDUCE, EXPAND = -1, 0, 1, 2
FORM_NAME = {AS_FIT: "fit", STURM: "sturm", REDUCE: "reduce", EXPAND: "expand"}

REPORT = {}        # case id -> measurements
STURM_ONLY = []    # ids of the Sturm-only cases run
GIVEUPS = []       # ... of those whose Sturm launch gave up


def after_failed_sturm(c, kp):
    """The solver's rule, restated: the reducing path while its arrow and chase admit the shape."""
    return REDUCE if kp + 8 <= 192 and c <= 640 else EXPAND


def forms_of(c, kp):
    return [AS_FIT, STURM] + ([REDUCE] if kp + 8 <= 192 and c <= 640 else []) + [EXPAND]


def check(cid, ref, p, w, S, Y, info, form, no_giveup=False, rec=None, discarded=False):
    """Every assertion of the module docstring on one result.  ref = (H, ref_w, V, tn)."""
    H, ref_w, V, tn = ref
    c = H.shape[0]
    nh = float(np.abs(ref_w).max())
    e_ref = 8 * c * EPS * nh
    rec = {} if rec is None else rec
    rec.update(form=FORM_NAME[form], c=c, p=p, **{k: info[k] for k in (
        "form_ran", "sturm_err", "second_solves", "reduce_err", "tri_coop", "msect_points",
        "msect_rounds")})
    REPORT[cid] = rec
    # ---- what ran
    if form == AS_FIT:
        assert info["sturm_err"] >= 0 and info["second_solves"] >= 0
        assert (info["form_ran"] == STURM) == (info["sturm_err"] == 0 and not discarded), info
        if info["sturm_err"] != 0 or discarded:
            assert info["form_ran"] == after_failed_sturm(c, rec["kp"]), info
    else:
        assert info["form_ran"] == form, info
        assert (info["sturm_err"] >= 0) == (form == STURM), info
    ran = info["form_ran"]
    assert (info["reduce_err"] >= 0) == (ran == REDUCE) and info["reduce_err"] <= 0, info
    assert (info["tri_coop"] >= 0) == (ran == EXPAND), info
    if form == STURM:
        STURM_ONLY.append(cid)
        if info["sturm_err"] != 0:
            assert not no_giveup, f"{cid}: the Sturm form gave up at an ordinary cycle's shape"
            GIVEUPS.append(cid)
            rec["gave_up"] = True
            return rec
    # ---- the vectors the residuals are read from
    S64 = S.astype(np.float64)
    assert np.isfinite(w).all() and np.isfinite(S64).all(), f"{cid}: a value no launch wrote"
    if ran == STURM:
        assert np.isfinite(Y).all(), f"{cid}: a column of Y no launch wrote"
        norms = np.linalg.norm(Y, axis=0)
        assert np.abs(norms - 1.0).max() <= 16 * EPS * c, (cid, np.abs(norms - 1.0).max())
        Yr = Y
        rec["ortho_Y"] = float(np.abs(Y.T @ Y - np.eye(p)).max())
    else:
        assert np.isnan(Y).all(), f"{cid}: Y from a form documented to return none"
        Yr = S64 / np.linalg.norm(S64, axis=0)
    r = rp.residuals(H, w, Yr)
    rec["r_over_c_eps_tn"] = float(r.max() / (c * EPS * tn))
    print(f"{cid}: ran {ran} err {info['sturm_err']} second {info['second_solves']} "
          f"max r/(c eps tn) {rec['r_over_c_eps_tn']:.3g} ortho_Y {rec.get('ortho_Y', -1):.3g}")
    # ---- eigenvalues
    dw = np.abs(w - ref_w[:p])
    assert (dw <= r + e_ref).all(), (cid, int(np.argmax(dw - r)), dw.max(), r.max(), e_ref)
    assert dw.max() <= 1e-10 * nh, (cid, dw.max() / nh)
    # ---- the kernel's acceptance rule, from the host
    if ran == STURM and info["sturm_err"] == 0:
        assert r.max() <= 1e-8 * tn, (cid, int(np.argmax(r)), r.max() / tn)
    # ---- what the consumer needs of S
    orth = np.abs(S64.T @ S64 - np.eye(p)).max()
    rec["ortho_S"] = float(orth)
    assert orth < 5e-6, (cid, orth)
    res = np.abs(H @ S64 - S64 * w).max()
    assert res < 5e-6 * nh, (cid, res / nh)
    # ---- subspaces
    worst = 0.0
    for a, b, gap in rp.groups(ref_w, tn, p):
        Yg, Vg = Yr[:, a:min(b, p)].astype(np.longdouble), V[:, a:b]
        out = np.linalg.norm((Yg - Vg @ (Vg.T @ Yg)).astype(np.float64), 2)
        bound = r[a:min(b, p)].max() / gap + 64 * c * EPS
        worst = max(worst, out / bound)
        assert out <= bound, (cid, a, b, out, bound)
    rec["subspace_of_bound"] = float(worst)
    return rec


def run(engine, cid, pr, ref, form, p=None, **kw):
    p = pr["p"] if p is None else p
    w, S, Y, info = engine.rr_stage(pr["hband"], pr["c"], pr["kp"], pr["theta"], p, form)
    rec = {"kp": pr["kp"]}
    for k in ("g", "gap"):
        if k in pr:
            rec[k] = pr[k]
    if "gap" in pr:
        rec["g_of_tn"] = pr["gap"] / ref[3]
    check(cid, ref, p, w, S, Y, info, form, rec=rec, **kw)
    return w, S, Y, info


def _ids(cases):
    return ["-".join(str(x) for x in k) + "-" + FORM_NAME[f] for k, f in cases]


# ----------------------------------------------------------------------------- 1 shapes
SHAPE_CASES = [(("shape", c, kp), f) for c, kp in rp.SHAPES for f in forms_of(c, kp)]


@pytest.mark.parametrize("key,form", SHAPE_CASES, ids=_ids(SHAPE_CASES))
def test_shape_sweep(engine, key, form):
    """Uniform spectrum on [10, 100], p = kp + 8, every form the shape admits: c - kp = 8 alone
    ((16, 8)), the nine tail lengths of the 9-step elimination (kp = 8, c - kp = 8 .. 72), the
    reducing path's last c (640), the largest inverse-iteration LDS ((768, 0)), kept sets past
    the reducing path's arrow ((520, 192), (768, 600), (768, 760))."""
    _, c, kp = key
    run(engine, f"shape {c} {kp} {FORM_NAME[form]}", rp.case(*key), rp.case_reference(*key),
        form, no_giveup=kp <= 184)


# ----------------------------------------------------------------------------- 2 multisection
@pytest.mark.parametrize("p", [1, 64, 65, 85, 86, 128, 129, 256, 257, 600, 768])
def test_multisection_boundaries(engine, p):
    """Both sides of every p at which the multisection's point count changes, at (768, 0)."""
    key = ("shape", 768, 0)
    _, _, _, info = run(engine, f"msect p {p}", rp.case(*key), rp.case_reference(*key), STURM,
                        p=p)
    M = 256 * min(max(256 // p, 1), 4)
    assert info["msect_points"] == M, info
    rounds, wdt = 1, 2.0 / (p * M + 1.0)  # the launcher's rule: brackets below 1e-10 of the span
    while wdt > 1e-10:
        rounds, wdt = rounds + 1, wdt / (M + 1)
    assert info["msect_rounds"] == rounds, info


# ----------------------------------------------------------------------------- 3 gaps
GAP_CASES = [(("gap", c, kp, g), f) for c, kp in rp.GAP_SHAPES for g in rp.GAPS
             for f in forms_of(c, kp)]


@pytest.mark.parametrize("key,form", GAP_CASES, ids=_ids(GAP_CASES))
def test_gap_sweep(engine, key, form):
    """Eigenvalues 4 .. 8 a ladder of gaps g tn, g from deep inside the inverse iterations'
    cluster threshold (1e-9 tn) to 1e-6 tn: just above the threshold nothing orthogonalises the
    ladder's vectors against each other, and the Sturm form's acceptance (residual <= 1e-8 tn) is
    looser than the threshold.  Among kept Ritz values (256, 80), in a pure band (256, 0) and past
    the reducing path (768, 600)."""
    _, c, kp, g = key
    run(engine, f"gap {c} {kp} {g:g} {FORM_NAME[form]}", rp.case(*key), rp.case_reference(*key),
        form)


@pytest.fixture(scope="module")
def dense_gap_unit():
    """The unit of the dense sweep's gaps: the Gershgorin norm of a Householder tridiagonal of the
    plain c = 256 matrix (rr_inviter_kernel's tn is that of the GPU's tridiagonal, which the
    host does not see; any orthogonal tridiagonalisation's lies within [1, 3] ||A||)."""
    A = _dense_matrix(rp.uniform_ev(256))
    T = scipy.linalg.hessenberg(A)
    return rp.gershgorin_norm(np.triu(np.tril(T, 1), -1))


def _dense_matrix(ev):
    rng = np.random.default_rng(256)
    V, _ = np.linalg.qr(rng.standard_normal((ev.size, ev.size)))
    A = (V * ev) @ V.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("tri", ["multi", "one"])
@pytest.mark.parametrize("g", rp.GAPS)
def test_gap_sweep_dense(engine, monkeypatch, dense_gap_unit, g, tri):
    """The same ladder through n2v2r_rr_top (the dense steps on A itself), both
    tridiagonalisation kernels, c = 256, p = 88."""
    if tri == "one":
        monkeypatch.setenv("N2V2R_RR_TRI", "1")
    c, p = 256, 88
    gap = g * dense_gap_unit
    A = _dense_matrix(rp.ladder_ev(rp.uniform_ev(c), rp.LADDER[0], rp.LADDER[1], gap))
    w, S = engine.rr_top(A, p)
    rw, V = np.linalg.eigh(A)
    rw, V = rw[::-1].copy(), V[:, ::-1].copy()
    ref = (A, rw, rp.refine(A, rw, V, dense_gap_unit), dense_gap_unit)
    info = dict(form_ran=EXPAND, sturm_err=-1, second_solves=-1, reduce_err=-1, tri_coop=0,
                msect_points=0, msect_rounds=0)  # (rr_top reports nothing: the dense steps)
    check(f"dense gap {g:g} {tri}", ref, p, w, S, np.full((c, p), np.nan), info, EXPAND,
          rec={"kp": 0, "g": g, "gap": gap})


# ----------------------------------------------------------------------------- 4 5 6 variants
VARIANTS = ([("edge", n) for n in rp.EDGES] + [("zero", n) for n in rp.ZEROS] +
            [("spectrum", n) for n in rp.SPECTRA])
VARIANT_CASES = [(k, f) for k in VARIANTS for f in forms_of(*rp.BASE)]


@pytest.mark.parametrize("key,form", VARIANT_CASES, ids=_ids(VARIANT_CASES))
def test_variants(engine, key, form):
    """At (256, 80), p = 88.  Clusters at the edges: an exact triple that straddles the last
    wanted index, one that starts at index 0, an exactly repeated pair, 24 equal kept Ritz
    values (couplings 1e-12); clustered groups are compared as subspaces.  Zero couplings: one
    R_j = 0 (the band splits), G0 rows 0 .. 29 exactly zero, both, and a diagonal H (S a signed
    permutation to 5e-6).  Spectra: indefinite, all negative, graded over twelve decades."""
    pr, ref = rp.case(*key), rp.case_reference(*key)
    cid = f"{key[0]} {key[1]} {FORM_NAME[form]}"
    w, S, Y, info = run(engine, cid, pr, ref, form)
    if key == ("zero", "diag") and not REPORT[cid].get("gave_up"):
        d = np.diag(ref[0])
        order = np.argsort(d)[::-1][:pr["p"]]
        assert np.array_equal(w, d[order]) or np.abs(w - d[order]).max() <= 8 * EPS * ref[3]
        P = np.zeros(S.shape)
        P[order, np.arange(pr["p"])] = 1.0
        assert np.abs(np.abs(S.astype(np.float64)) - P).max() <= 5e-6


@pytest.mark.parametrize("form", forms_of(*rp.BASE), ids=lambda f: FORM_NAME[f])
@pytest.mark.parametrize("e", [-60, 60])
def test_scaled(engine, form, e):
    """H times 2^-60 and 2^+60: every bound holds in the scaled units, w scales, and |S| is the
    unscaled run's within 5e-6.  Whether the scaled run is bit-identical is recorded."""
    key = ("shape",) + rp.BASE
    pr, ref = rp.case(*key), rp.case_reference(*key)
    s = 2.0 ** e
    spr = dict(pr, hband=pr["hband"] * s, theta=pr["theta"] * s)
    sref = (ref[0] * s, ref[1] * s, ref[2], ref[3] * s)  # (powers of two: exact)
    cid = f"scaled 2^{e} {FORM_NAME[form]}"
    w0, S0, Y0, i0 = engine.rr_stage(pr["hband"], pr["c"], pr["kp"], pr["theta"], pr["p"], form)
    w1, S1, Y1, i1 = run(engine, cid, spr, sref, form)
    if form == STURM and (i0["sturm_err"] or i1["sturm_err"]):
        return
    nh = np.abs(ref[1]).max()
    assert np.abs(w1 / s - w0).max() <= 2e-10 * nh
    assert np.abs(np.abs(S1.astype(np.float64)) - np.abs(S0.astype(np.float64))).max() <= 5e-6
    REPORT[cid]["bit_identical_to_unscaled"] = bool(
        np.array_equal(w1 / s, w0) and np.array_equal(S1, S0))


# ----------------------------------------------------------------------------- 7 the path
def test_expand_matches_reduce(engine):
    """(256, 80): the dense steps on the expanded H and the reducing path agree on w within the
    eigenvalue ceiling (each is held to the reference by the shape sweep)."""
    key = ("shape", 256, 80)
    pr, ref = rp.case(*key), rp.case_reference(*key)
    w1 = run(engine, "path reduce", pr, ref, REDUCE)[0]
    w2, _, _, info = run(engine, "path expand", pr, ref, EXPAND)
    assert np.abs(w2 - w1).max() <= 1e-10 * np.abs(ref[1]).max()
    assert info["tri_coop"] in (0, 1)


def test_expand_one_workgroup_kernel(engine, monkeypatch):
    """(768, 600), where the reducing path cannot run: DenseFromBand with the one-workgroup
    tridiagonalisation passes every assertion too, and the report names the kernel."""
    monkeypatch.setenv("N2V2R_RR_TRI", "1")
    key = ("shape", 768, 600)
    info = run(engine, "path expand one-wg", rp.case(*key), rp.case_reference(*key), EXPAND)[3]
    assert info["tri_coop"] == 0


@pytest.mark.parametrize("c,kp", [(256, 80), (640, 184), (520, 192), (768, 600)])
def test_fallback_after_a_discarded_sturm_result(engine, monkeypatch, c, kp):
    """The Sturm form gives up in none of this module's cases, so the step after a failed result
    is taken with a good one discarded (N2V2R_RR_STAGE_TEST_STURM_FAIL, as a fit's
    N2V2R_EIG_TEST_STURM_FAIL): form -1 then returns the form the rule names -- the reducing path
    up to (640, 184), past it the dense steps on H expanded with the kept Ritz values the Sturm
    assembly copied -- with the bits of that form run alone."""
    monkeypatch.setenv("N2V2R_RR_STAGE_TEST_STURM_FAIL", "1")
    key = ("shape", c, kp)
    pr, ref = rp.case(*key), rp.case_reference(*key)
    w, S, Y, info = run(engine, f"discarded {c} {kp}", pr, ref, AS_FIT, discarded=True)
    assert info["form_ran"] == after_failed_sturm(c, kp) and info["sturm_err"] == 0
    monkeypatch.delenv("N2V2R_RR_STAGE_TEST_STURM_FAIL")
    w1, S1, _, _ = engine.rr_stage(pr["hband"], c, kp, pr["theta"], pr["p"], info["form_ran"])
    assert np.array_equal(w, w1) and np.array_equal(S, S1)


def test_shared_rule():
    """The restated rule at the corners the cases sit on."""
    assert after_failed_sturm(640, 184) == REDUCE and after_failed_sturm(520, 192) == EXPAND
    assert after_failed_sturm(648, 184) == EXPAND and after_failed_sturm(768, 600) == EXPAND
    assert REDUCE not in forms_of(520, 192) and REDUCE in forms_of(640, 184)


# ----------------------------------------------------------------------------- 8 repeat, handle
@pytest.mark.parametrize("c,kp", [(256, 80), (768, 600)])
def test_repeatable(engine, c, kp):
    pr = rp.case("shape", c, kp)
    for form in forms_of(c, kp):
        a = engine.rr_stage(pr["hband"], c, kp, pr["theta"], pr["p"], form)
        b = engine.rr_stage(pr["hband"], c, kp, pr["theta"], pr["p"], form)
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes(), (c, kp, form)
        assert a[3] == b[3]


def test_handle_left_usable(engine):
    """A fit after the calls gives the bits of a fit without them, and the results of the fit
    before them stay readable."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    d, seed = int(fx["dims"].max()), int(fx["seed"])
    engine.set_layers(layers)

    def fit():
        engine.uase(d, seed=seed)
        return engine.singular_values(), engine.embedding(), engine.left_embedding()

    fit()
    ref = fit()  # (a fit after a fit, as the one below is)
    pr = rp.case("shape", 256, 80)
    for form in forms_of(256, 80):
        engine.rr_stage(pr["hband"], 256, 80, pr["theta"], pr["p"], form)
    after = (engine.singular_values(), engine.embedding(), engine.left_embedding())
    again = fit()
    for a, b, c in zip(ref, after, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ----------------------------------------------------------------------------- 9 arguments
def test_bad_arguments(engine):
    """Every refusal is N2V2R_ERR_BAD_ARG, writes nothing, and leaves the handle working."""
    from node2vec2rank_amd import _lib
    pr = rp.case("shape", 256, 80)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    hb256 = pr["hband"]

    def call(c=256, kp=80, p=88, form=AS_FIT, hband=hb256, hlen=None, theta=pr["theta"],
             w=True, S=True, Y=True, h=None):
        n = max(c, 1) * max(p, 1)
        out = (np.zeros(max(p, 1)) if w else None, np.zeros(n, np.float32) if S else None,
               np.zeros(n) if Y else None)
        info = _lib.RrInfo()
        st = engine.lib.n2v2r_rr_stage(
            engine.h if h is None else h, c, kp, ptr(hband),
            (0 if hband is None else hband.size) if hlen is None else hlen, ptr(theta), p, form,
            ptr(out[0]), ptr(out[1]), ptr(out[2]), ctypes.byref(info))
        if st != _lib.OK:
            assert all(o is None or not o.any() for o in out), "a refused call wrote an output"
            assert info.form_ran == -1 or h is not None
        return st

    big = np.zeros(rp.hband_len(768, 0))
    bad = _lib.ERR_BAD_ARG
    for form in (AS_FIT, STURM, EXPAND):
        assert call(c=8, kp=0, p=8, form=form, hband=big, theta=None) == bad  # below the launchers'
    assert call(c=20, kp=0, p=8, hband=big, theta=None) == bad        # c % 8
    assert call(c=776, kp=0, p=8, hband=big, theta=None) == bad       # past 768 columns
    assert call(c=256, kp=84) == bad                                   # kp % 8
    assert call(c=16, kp=16, p=8, hband=big) == bad                    # kp + 8 > c
    assert call(c=88, kp=88, p=8, hband=big) == bad
    assert call(c=256, kp=192, form=REDUCE, hband=big, theta=np.zeros(192)) == bad  # the arrow
    assert call(hlen=hb256.size - 1) == bad                            # a short hband
    assert call(p=0) == bad and call(p=257) == bad
    assert call(hband=None, hlen=hb256.size) == bad
    assert call(theta=None) == bad                                     # kp > 0 needs theta_prev
    assert call(w=False) == bad and call(S=False) == bad
    assert call(form=-2) == bad and call(form=3) == bad
    assert call(h=ctypes.c_void_p(None)) == bad
    assert call(Y=False) == _lib.OK                                    # Y is optional
    assert call() == _lib.OK
    # the handle still works
    key = ("shape", 256, 80)
    run(engine, "after refusals", rp.case(*key), rp.case_reference(*key), AS_FIT)


# ----------------------------------------------------------------------------- the give-up cap
def test_zz_sturm_only_giveups():
    """Of the Sturm-only cases this session ran, at most 10 % gave up (the last test of the
    module: it counts the ones before it).  Writes the measurements where asked to."""
    path = os.environ.get("N2V2R_RR_STAGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"sturm_only_cases": len(STURM_ONLY), "sturm_only_giveups": GIVEUPS,
                       "cases": REPORT}, f, indent=1, sort_keys=True)
    print(f"Sturm-only: {len(GIVEUPS)} of {len(STURM_ONLY)} gave up: {GIVEUPS}")
    assert len(GIVEUPS) <= 0.10 * len(STURM_ONLY), GIVEUPS
