"""The orthogonalisation pass at block widths 16, 32 and 64 and the block Grams on their own
(``n2v2r_ortho_pass``: the solver's ``Eig::pip_pass``; ``n2v2r_block_gram``: its ``Eig::tn``)
against np.longdouble / fp64: the Gram kernels ``ts_tn_narrow_kernel<16, .>`` (b = 16, one
right-hand block) and ``ts_tn_kernel`` (MFMA; b = 32 / 64 and every many-block right-hand side:
H = Q^T W of the dense Rayleigh-Ritz), ``pip_chol_kernel`` in every form (P staged / chunked, the
register and the wave-0 factorisation, F over 1 .. 6 workgroups, both F writers) and the apply
``ts_nn_rows_kernel<16>`` / ``ts_nn_kernel<1>`` / ``<2>`` with the cond, flags and refill
arguments.  Every case asserts the branch it took from ``n2v2r_pass_info``, which the entries fill
from the launchers' own shape rules.  The handle carries one identity layer, only to fix n.

Inputs.  Pass: Q is the fp32 rounding of an fp64-orthonormal factor, Z = Q_S A + W with b columns,
built as in test_gpu_pip_pass.py (W orthogonalised against Q in fp64, columns of norm 1 .. 2,
|A_ij| = (1 .. 2) 1e-2 ||w_j||); every case asserts on the CPU that cond_2(P) < 10 for
P = sym(Z^T Z) - C^T C from the fp64 Gram of the fp32 arrays.  n = 4,099 is prime: the last chunk
and the last wave are ragged and the MFMA kernel's two-row tail step ends on an odd row.  Gram:
N(0, 1) arrays with planted rows scaled by 30 -- the last row, the last row of every wave's span
(ceil(rows_per_chunk / 4) apart within a chunk, from info), and rows 1023, 1024, 1025 of a wave's
span where it is that long -- so a dropped, doubled or misplaced row moves entries by far more
than the bound.

Bounds (gamma_t(k) = k u_t / (1 - k u_t), u32 = 2^-24, u64 = 2^-53).
  Gram (derived): |G - ref| <= (gamma32(2 m) + gamma64(n + 8)) |A|^T |B| with
    m = min(ceil(rows_per_chunk / 4), TN_FLUSH + 8) from info: one fp32 span per wave between
    flushes and two roundings per product (the convention of test_gpu_ritz_step.py for
    mfma_f32_32x32x2; it covers an uncontracted multiply-add in the narrow kernel), then fp64
    additions over the flushes, waves and chunks.  Reference in np.longdouble up to 2e7
    multiply-adds, fp64 BLAS past that with its own gamma64(n) |A|^T |B| added.
  F (derived): against -C X (rows < c) and X (rows >= c) in np.longdouble from the returned Gram
    and xinv, |F - ref| <= u32 |ref| + gamma64(b + 1) |C| |X|; flagged columns exactly 0.
  Z' (derived): against [Q Z] F in np.longdouble from the returned fp32 F, the product bound of
    test_gpu_ritz_step.py, gamma32(2 (c + b)) |[Q Z]| |F| (the same kernels).
  xinv (measured constant): against the inverse of the Cholesky factor of P^ (np.longdouble, from
    the returned Gram, by the kernel's pivot rule): err <= XINV_C b u64 cond_2(P^) max |X_ref|.

The refill deviates of a flagged column are compared bit for bit with the column
``n2v2r_pip_pass`` refills at b = 8 with the same refill seed and column index (both use
counter_normal(seed, row * 64 + col)), and the b = 8 pass through the new entry bit for bit with
``n2v2r_pip_pass`` given the reported refill seed.

A non-finite entry in one column of Z (test_non_finite_column): before this file the flagged
column's entries of R above the diagonal stayed non-finite and the back substitution multiplied
them by the zeros of the flagged row of R^{-1} (NaN x 0), so every column of xinv came out NaN, in
both factorisation forms; F summed NaN x 0 over the flagged column of C, and the apply multiplied
the non-finite entry by the zero coefficients of its column.  pip_chol_kernel now skips a flagged
column in the substitution and in F's sums, and the apply kernels read a flagged column of the
block being replaced as zeros; with finite input every output keeps its bits.  The fused b = 8
kernel (pip_factor / pip_finish) has the same flaw and is left as it is: through the new entry,
one NaN entry in column 3 at n = 4,099, nq = 1 and 5, flags column 3 alone and refills it, and
every other column comes back NaN in all rows.

On an MI355X: 64 cases, 8.3 s together (the slowest, test_narrow_flush at n = 4,198,407, 1.5 s).
Largest fractions of the bounds reached: Gram 0.0059 (ts_tn_kernel), 0.0053
(ts_tn_narrow_kernel), 0.0036 (the streaming kernel at b = 8); F 0.9965 (pip_chol_kernel: the
bound's first term is the fp32 rounding of F itself); Z' 0.067 (ts_nn_rows_kernel<16>), 0.047
(ts_nn_kernel<1>), 0.028 (ts_nn_kernel<2>); the xinv ratio between 7.9e-3 and 0.21 (5e-10 .. 4e-9
on the clamped duplicates, cond_2 4e6).

Kernel changes that must fail this file (each tried once on a scratch copy): the last F
workgroup's fend one row short; ts_tn_narrow_kernel without its scalar tail loop; ts_tn_kernel's
tail step adding row r1 - 1 again for the odd row, its output row map with the 4 and the 8
swapped, its flush without zeroing acc; the register-form pivot reading zzd[ej]; ts_nn_kernel
refilling by flags[col ^ 1].  Not observable by any shape: the odd last row of the chunked P loop
(`if (k < kr)`), since kr = min(4096 / b, c - k0) is even for every c that is a multiple of b."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import fixture_layers, load_fixture
from test_gpu_pip_pass import SINGLE, _basis, _gamma, _ro, _single_case, U32, U64

pytestmark = pytest.mark.gpu

N0 = 4099
LD = np.longdouble
TN_FLUSH = 1024
PIP_CANCEL = 1e-6
STREAM, LINES, NARROW, MFMA = 0, 1, 2, 3
# max |xinv - X_ref| / (b u64 cond_2(P^) max |X_ref|) over the pass and pivot cases below.
# Measured on an MI355X: 7.9e-3 .. 0.21 (5e-10 for the clamped duplicates, whose cond_2 is 4e6);
# 10 x the largest for other seeds.
XINV_C = 2.1


def _identity(eng, n):
    eng.set_layers([sp.identity(n, dtype=np.float32, format="csr")])


def _flat(blocks):
    """(nblk, n, b) blocks -> (n, nblk b)."""
    return blocks.transpose(1, 0, 2).reshape(blocks.shape[1], -1)


_FRAC = {}  # kernel family -> largest fraction of its bound so far


def _note(family, frac):
    _FRAC[family] = max(_FRAC.get(family, 0.0), frac)
    return _FRAC[family]


def _report(what, family, kind, frac):
    print(f"wide_pass {what}: {family} {kind} worst / bound = {frac:.4g}"
          f" (family so far {_note(family + ' ' + kind, frac):.4g})")


GRAM_NAME = {STREAM: "ts_tn_stream", LINES: "ts_tn_lines", NARROW: "ts_tn_narrow", MFMA: "ts_tn"}


def _apply_name(k):
    return {0: "pip_fused", 8: "ts_nn_rows<8>", 16: "ts_nn_rows<16>"}.get(k, f"ts_nn<{k // 32}>")


# ----------------------------------------------------------------------------- references
def _gram_ref(A, B):
    """(A^T B, |A|^T |B|, gamma of the reference's own error) for fp32 (n, ca), (n, cb): in
    np.longdouble up to 2e7 multiply-adds, else fp64 BLAS.  Non-finite inputs give non-finite
    reference entries in the positions they reach."""
    n = A.shape[0]
    mag = np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)
    if n * A.shape[1] * B.shape[1] <= 2e7:
        return np.einsum("ni,nj->ij", A.astype(LD), B.astype(LD)), mag, 0.0
    return (A.astype(np.float64).T @ B.astype(np.float64)).astype(LD), mag, _gamma(n, U64)


def _check_gram(what, G, ref, mag, gref, info, n):
    per_wave = -(-info["rows_per_chunk"] // 4)
    m = min(per_wave, TN_FLUSH + 8)
    bound = LD(_gamma(2 * m, U32) + _gamma(n + 8, U64) + gref) * mag
    ok = np.isfinite(ref.astype(np.float64))
    assert not np.isnan(G[ok]).any(), (what, "NaN left in the Gram")
    err = np.abs(G.astype(LD) - ref)
    zero = ok & (bound == 0)  # (a zero column: nothing to round)
    assert (err[zero] == 0).all(), (what, "a Gram entry of a zero column is not zero")
    ok &= ~zero
    frac = float((err[ok] / bound[ok]).max())
    _report(what, GRAM_NAME[info["gram_form"]], "Gram", frac)
    assert frac <= 1.0, (what, frac)


def _factor_ref(gram, b, first):
    """(X, R, bad) in np.longdouble from a returned Gram ((c + b) x b) by pip_chol_kernel's pivot
    rule: P = sym(Z^T Z) - C^T C = R^T R, a pivot not above PIP_CANCEL of the column's squared
    norm clamped to it and the row decoupled (first) or the column flagged (later passes), zero and
    non-finite columns flagged (unit row); X = R^{-1} with flagged columns zero."""
    g = gram.astype(LD)
    c = g.shape[0] - b
    C, ZZ = g[:c], g[c:]
    A = (ZZ + ZZ.T) / 2 - C.T @ C
    zz = np.diag(ZZ).copy()
    floor = LD(1e-30) * np.nanmax(zz)
    R = np.zeros((b, b), LD)
    bad = []
    for k in range(b):
        d = A[k, k]
        cn = not d > LD(PIP_CANCEL) * zz[k]
        if (not zz[k] > floor) or d != d or (cn and not first):
            bad.append(k)
            R[k, k] = 1
            continue
        if cn:
            R[k, k] = np.sqrt(LD(PIP_CANCEL) * zz[k])
            continue
        R[k, k] = np.sqrt(d)
        R[k, k + 1:] = A[k, k + 1:] / R[k, k]
        A[k + 1:, k + 1:] -= np.outer(R[k, k + 1:], R[k, k + 1:])
    for j in bad:
        R[:j, j] = 0
    X = np.zeros((b, b), LD)
    for j in range(b - 1, -1, -1):
        e = np.zeros(b, LD)
        e[j] = 1
        X[j] = (e - R[j, j + 1:] @ X[j + 1:]) / R[j, j]
    X[:, bad] = 0
    return X, R, bad


def _check_xinv(what, out, b, first):
    """Returns the flagged columns of the reference factorisation."""
    X, R, bad = _factor_ref(out["gram"], b, first)
    kappa = float(np.linalg.cond(R.astype(np.float64))) ** 2
    assert not np.isnan(out["xinv"]).any(), (what, "NaN in xinv")
    assert not np.tril(out["xinv"], -1).any() and not out["xinv"][:, bad].any()
    err = float(np.abs(out["xinv"].astype(LD) - X).max())
    ratio = err / (b * U64 * kappa * float(np.abs(X).max()))
    print(f"wide_pass {what}: xinv error / (b u64 cond max|X|) = {ratio:.4g}"
          f" (so far {_note('xinv ratio', ratio):.4g}; cond {kappa:.3g})")
    assert ratio <= XINV_C, (what, ratio)
    return bad


def _check_F(what, out, b, flagged):
    g, X = out["gram"].astype(LD), out["xinv"].astype(LD)
    c = g.shape[0] - b
    C = g[:c].copy()
    C[:, flagged] = 0  # (a flagged column of C may be non-finite; its coefficients are zero)
    ref = np.vstack([-(C @ X), X])
    mag = np.vstack([np.abs(C) @ np.abs(X), np.zeros((b, b), LD)])
    F = out["F"]
    assert F.dtype == np.float32 and not np.isnan(F).any(), (what, "NaN in F")
    assert not F[:, flagged].any(), (what, "a flagged column of F is not zero")
    bound = LD(U32) * np.abs(ref) + LD(_gamma(b + 1, U64)) * mag
    err = np.abs(F.astype(LD) - ref)
    nz = bound > 0
    assert (err[~nz] == 0).all()
    frac = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    _report(what, "pip_chol", "F", frac)
    assert frac <= 1.0, (what, frac)


def _check_apply(what, out, Q, zin, b, flagged):
    """Z' against [Q Z] F (the returned fp32 F) on the columns not flagged; no NaN anywhere."""
    A = np.concatenate([_flat(Q), zin], axis=1) if Q.shape[0] else zin.copy()
    A[:, A.shape[1] - b + np.asarray(flagged, dtype=int)] = 0  # (read as zeros: their F rows are)
    n, ca = A.shape
    F, Z = out["F"], out["Z"]
    bad = np.flatnonzero(np.isnan(Z).any(1))
    assert bad.size == 0, (what, "NaN left in rows", bad[:8], "of", n)
    keep = np.setdiff1d(np.arange(b), flagged)
    g = LD(_gamma(2 * ca, U32))
    Fl, Fa = F.astype(LD), np.abs(F).astype(np.float64)
    frac = 0.0
    for r0 in range(0, n, 32768):
        a = A[r0:r0 + 32768]
        ref = np.einsum("nk,kj->nj", a.astype(LD), Fl)
        mag = np.abs(a).astype(np.float64) @ Fa
        f = np.abs(Z[r0:r0 + 32768].astype(LD) - ref)[:, keep] / (g * mag[:, keep])
        frac = max(frac, float(f.max()))
    _report(what, _apply_name(out["info"]["apply_kernel"]), "Z'", frac)
    assert frac <= 1.0, (what, frac)


def _check_refill(col):
    assert np.isfinite(col).all()
    assert abs(float(col.mean())) < 5.0 / np.sqrt(col.size) and 0.9 < float(col.std()) < 1.1


def _check_pass(what, out, Q, zin, b, first=0, flagged=()):
    """Every check of one pass at b > 8: the Gram, xinv, F and Z' within their bounds."""
    n = zin.shape[0]
    A = np.concatenate([_flat(Q), zin], axis=1) if Q.shape[0] else zin
    ref, mag, gref = _gram_ref(A, zin)
    _check_gram(what, out["gram"], ref, mag, gref, out["info"], n)
    bad = _check_xinv(what, out, b, first)
    assert bad == list(flagged) and np.flatnonzero(out["flags"]).tolist() == list(flagged), what
    _check_F(what, out, b, list(flagged))
    _check_apply(what, out, Q, zin, b, list(flagged))
    for j in flagged:
        _check_refill(out["Z"][:, j])
    return ref


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _pass_case(b, nq, n=N0):
    """(Q as (nq, n, b) fp32, Z (n, b) fp32): Z = Q_S A + W, S the first, the middle and the last
    block."""
    rng = np.random.default_rng(11 * n + 97 * b + nq)
    w = rng.standard_normal((n, b)) / np.sqrt(n)
    if nq == 0:
        return _ro(np.zeros((0, n, b), np.float32), (w * rng.uniform(1.0, 2.0, b)).astype(np.float32))
    q64, q32 = _basis(n, b * nq, 300 + b + nq)
    for _ in range(2):
        w = w - q64 @ (q64.T @ w)
    w = w * rng.uniform(1.0, 2.0, b)
    z, wn = w.copy(), np.linalg.norm(w, axis=0)
    for k in sorted({0, nq // 2, nq - 1}):
        a = rng.uniform(1.0, 2.0, (b, b)) * rng.choice([-1.0, 1.0], (b, b)) * 1e-2 * wn
        z += q64[:, b * k:b * k + b] @ a
    Q = np.ascontiguousarray(q32.reshape(n, nq, b).transpose(1, 0, 2))
    return _ro(Q, z.astype(np.float32))


def _assert_well_conditioned(ref, b):
    """cond_2(P) < 10 from the fp64 Gram of the fp32 arrays."""
    g = ref.astype(np.float64)
    c = g.shape[0] - b
    p = (g[c:] + g[c:].T) / 2 - g[:c].T @ g[:c]
    assert np.linalg.cond(p) < 10, np.linalg.cond(p)


# (b, nq, stage, nwg, what it reaches)
PASS = [
    (16, 0, 1, 1, "the start block; bb > 64 staged P; register factorisation"),
    (16, 1, 1, 1, "one basis block"),
    (16, 7, 1, 1, "c + b = 128: the last shape with one F workgroup"),
    (16, 8, 1, 2, "c + b = 144: two F workgroups"),
    (16, 16, 1, 3, "c + b = 272 over 3 workgroups of 91: the last one short"),
    (16, 27, 1, 4, "c = 432: the last staged c"),
    (16, 28, 0, 4, "c = 448: the first unstaged c; chunked P (256 + 192 rows), chunked F"),
    (16, 47, 0, 6, "c + b = 768: the largest basis"),
    (32, 0, 1, 1, "the start block"),
    (32, 1, 1, 1, "one basis block"),
    (32, 3, 1, 1, "c + b = 128"),
    (32, 4, 1, 2, "c + b = 160: two F workgroups"),
    (32, 6, 1, 2, "c = 192: the last staged c"),
    (32, 7, 0, 2, "c = 224: the first unstaged c; chunked P (128 + 96 rows)"),
    (32, 9, 0, 3, "c + b = 320 over 3 workgroups of 107: the last one short"),
    (32, 23, 0, 6, "c + b = 768: the largest basis, the cfg3 shape"),
    (64, 0, 1, 1, "the start block: the only staged c; wave-0 factorisation"),
    (64, 1, 0, 1, "c + b = 128: one F workgroup, unstaged"),
    (64, 2, 0, 2, "c + b = 192: two F workgroups"),
    (64, 4, 0, 3, "c + b = 320 over 3 workgroups of 107"),
    (64, 11, 0, 6, "c + b = 768: the largest basis"),
]
GRAM_OF = {16: NARROW, 32: MFMA, 64: MFMA}
APPLY_OF = {16: 16, 32: 32, 64: 64}


def _assert_branch(info, b, nq, stage, nwg):
    assert info["gram_form"] == GRAM_OF[b] and info["gram_flush"] == 0, info
    assert (info["stage"], info["nwg"], info["apply_kernel"]) == (stage, nwg, APPLY_OF[b]), info
    c = nq * b
    assert stage == int((c + b) * b * 8 <= 56 * 1024) and nwg == min(8, (c + b + 127) // 128)
    assert -(-N0 // info["rows_per_chunk"]) == info["nchunks"]


# ----------------------------------------------------------------------------- the pass
@pytest.mark.parametrize("b,nq,stage,nwg,why", PASS, ids=[f"b{c[0]}-nq{c[1]}" for c in PASS])
def test_pass_branches(engine, b, nq, stage, nwg, why):
    _identity(engine, N0)
    Q, z = _pass_case(b, nq)
    out = engine.ortho_pass(Q, z, seed=5)
    what = f"b {b} nq {nq}"
    print(f"wide_pass {what}: info {out['info']}")
    _assert_branch(out["info"], b, nq, stage, nwg)
    assert out["any_flag"] == 0
    ref = _check_pass(what, out, Q, z, b)
    _assert_well_conditioned(ref, b)


@pytest.mark.parametrize("b,nq", [(16, 1), (32, 7), (64, 2)])
def test_out_of_place_is_bit_identical(engine, b, nq):
    """in_place = 0 (a separate input block, the result into a NaN-filled one, as expand_one does
    from W_from) gives the bits of the in-place pass."""
    _identity(engine, N0)
    Q, z = _pass_case(b, nq)
    a = engine.ortho_pass(Q, z, in_place=True, first=1, seed=5)
    o = engine.ortho_pass(Q, z, in_place=False, first=1, seed=5)
    assert not np.isnan(o["Z"]).any()
    for key in ("Z", "gram", "xinv", "F", "flags"):
        assert a[key].tobytes() == o[key].tobytes(), key
    assert a["any_flag"] == o["any_flag"] == 0 and a["info"] == o["info"]


@pytest.mark.parametrize("n,nq,S", [SINGLE[1], SINGLE[2]], ids=["nq5", "nq70"])
def test_b8_is_the_earlier_entry(engine, n, nq, S):
    """b = 8 through Eig::pip_pass: Z, Gram and flags are the bits n2v2r_pip_pass (the launchers
    called directly) gives with the refill seed the pass reports."""
    _identity(engine, n)
    Q, z = _single_case(n, nq, S)
    z = z.copy()
    z[:, 5] = 0.0  # (a refilled column, so the seed matters)
    out = engine.ortho_pass(Q, z, seed=77)
    info = out["info"]
    assert (info["gram_form"], info["apply_kernel"], info["stage"], info["nwg"]) == (STREAM, 0, 0, 0)
    assert info["fill_seed"] == 77 ^ (0xABCD + 1) and out["xinv"] is None and out["F"] is None
    old = engine.pip_pass(Q, z, tau=0.0, first=0, seed=info["fill_seed"])
    assert out["flags"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and out["any_flag"] == 1
    assert out["Z"].tobytes() == old["Za"].tobytes()
    assert out["gram"].tobytes() == old["gram"].tobytes()
    assert out["flags"].tobytes() == old["flags"].tobytes() and old["any_flag"] == 1
    ref, mag, gref = _gram_ref(np.concatenate([_flat(Q), z], axis=1), z)
    _check_gram(f"b 8 nq {nq}", out["gram"], ref, mag, gref, info, n)


# ----------------------------------------------------------------------------- the pivot rule
# (b, nq): nq = 1 and one unstaged c; b = 16 / 32 the register form, 64 the wave-0 form
PIVOT = [(16, 1), (16, 28), (32, 1), (32, 7), (64, 1)]
pivot_cases = pytest.mark.parametrize("b,nq", PIVOT, ids=[f"b{b}-nq{q}" for b, q in PIVOT])


def _b8_refill(engine, seed, j):
    """Column j < 8 as n2v2r_pip_pass refills it at b = 8 with refill seed `seed`."""
    n, nq, S = SINGLE[0]
    assert n == N0
    Q, z = _single_case(n, nq, S)
    z = z.copy()
    z[:, j] = 0.0
    out = engine.pip_pass(Q, z, tau=0.0, first=0, seed=seed)
    assert out["flags"][j] == 1
    return out["Za"][:, j]


@pivot_cases
@pytest.mark.parametrize("first", [0, 1])
def test_zero_column(engine, b, nq, first):
    _identity(engine, N0)
    Q, z0 = _pass_case(b, nq)
    z = z0.copy()
    z[:, 3] = 0.0
    out = engine.ortho_pass(Q, z, first=first, seed=9)
    _check_pass(f"zero column b {b} nq {nq} first {first}", out, Q, z, b, first, flagged=(3,))
    assert out["flags"].tolist() == [int(j == 3) for j in range(b)] and out["any_flag"] == 1
    assert out["Z"][:, 3].tobytes() == _b8_refill(engine, out["info"]["fill_seed"], 3).tobytes()


@pivot_cases
def test_duplicate_column(engine, b, nq):
    """A column that copies another: its pivot cancels.  The block's first pass clamps the pivot
    to PIP_CANCEL of the column's squared norm and keeps the column (flag clear, any_flag set); a
    later pass flags and refills it."""
    _identity(engine, N0)
    Q, z0 = _pass_case(b, nq)
    z = z0.copy()
    z[:, 6] = z[:, 2]
    a = engine.ortho_pass(Q, z, first=1, seed=9)
    assert not a["flags"].any() and a["any_flag"] == 1
    _check_pass(f"duplicate b {b} nq {nq} first 1", a, Q, z, b, first=1)
    o = engine.ortho_pass(Q, z, first=0, seed=9)
    assert o["flags"].tolist() == [int(j == 6) for j in range(b)] and o["any_flag"] == 1
    _check_pass(f"duplicate b {b} nq {nq} first 0", o, Q, z, b, first=0, flagged=(6,))


@pivot_cases
def test_condition_word(engine, b, nq):
    """cond = 0: nothing runs (Z bit for bit, the flags and any_flag cleared, Gram, xinv and F
    still NaN-filled); cond = 1 is the pass without a condition word."""
    _identity(engine, N0)
    Q, z = _pass_case(b, nq)
    off = engine.ortho_pass(Q, z, cond=0, seed=9)
    assert off["Z"].tobytes() == z.tobytes()
    assert not off["flags"].any() and off["any_flag"] == 0
    for key in ("gram", "xinv", "F"):
        assert np.isnan(off[key]).all(), key
    on, plain = engine.ortho_pass(Q, z, cond=1, seed=9), engine.ortho_pass(Q, z, cond=-1, seed=9)
    for key in ("Z", "gram", "xinv", "F", "flags"):
        assert on[key].tobytes() == plain[key].tobytes(), key
    assert on["any_flag"] == plain["any_flag"] == 0 and on["info"] == plain["info"]
    assert not np.isnan(on["Z"]).any()


@pivot_cases
def test_non_finite_column(engine, b, nq):
    """One NaN entry in column 3: only that column is flagged and refilled; every other output
    column is finite and within its bound (module docstring)."""
    _identity(engine, N0)
    Q, z0 = _pass_case(b, nq)
    z = z0.copy()
    z[5, 3] = np.nan
    out = engine.ortho_pass(Q, z, first=0, seed=9)
    assert out["flags"].tolist() == [int(j == 3) for j in range(b)] and out["any_flag"] == 1
    _check_pass(f"NaN entry b {b} nq {nq}", out, Q, z, b, first=0, flagged=(3,))
    # the rest of the block is what the pass makes of Z with that column zero
    zz = z0.copy()
    zz[:, 3] = 0.0
    same = engine.ortho_pass(Q, zz, first=0, seed=9)
    assert out["Z"].tobytes() == same["Z"].tobytes() and out["F"].tobytes() == same["F"].tobytes()


# ----------------------------------------------------------------------------- block Grams
def _planted(n, info):
    """The rows to scale: the last row, the last row of every wave's span, rows 1023 .. 1025 of a
    span where it is that long."""
    rpc = info["rows_per_chunk"]
    pw = -(-rpc // 4)
    rows = {n - 1}
    for c0 in range(0, n, rpc):
        c1 = min(c0 + rpc, n)
        for w in range(4):
            r0, r1 = c0 + w * pw, min(c0 + (w + 1) * pw, c1)
            if r0 >= r1:
                continue
            rows.add(r1 - 1)
            rows.update(r for r in (r0 + 1023, r0 + 1024, r0 + 1025) if r < r1)
    return np.array(sorted(rows))


def _gram_case(engine, what, n, b, na, nb, form, last_block=False):
    """N(0, 1) blocks with planted rows through block_gram, checked; returns info.  last_block:
    B is A's last block (the pass Gram)."""
    _identity(engine, n)
    rng = np.random.default_rng(1000 * b + 10 * na + nb)
    A = rng.standard_normal((na, n, b), dtype=np.float32)
    B = A[-1:] if last_block else rng.standard_normal((nb, n, b), dtype=np.float32)
    _, info = engine.block_gram(A, B)  # (the plan the rows are planted for)
    rows = _planted(n, info)
    A[:, rows] *= 30
    if not last_block:
        B[:, rows] *= 30
    G, info2 = engine.block_gram(A, B)
    print(f"wide_pass {what}: info {info2}; {rows.size} planted rows")
    assert info2 == info and info["gram_form"] == form, info2
    ref, mag, gref = _gram_ref(_flat(A), _flat(B))
    _check_gram(what, G, ref, mag, gref, info, n)
    return info


@pytest.mark.parametrize("b,form", [(8, STREAM), (16, NARROW), (32, MFMA), (64, MFMA)])
def test_pass_gram(engine, b, form):
    """nb = 1, B = A's last block: the Gram of a pass."""
    info = _gram_case(engine, f"pass Gram b {b}", N0, b, 5, 1, form, last_block=True)
    assert info["gram_flush"] == 0


# (b, nq, what it reaches)
H_SHAPES = [
    (8, 5, "c = 40: a tile edge inside a 32-wide tile"),
    (16, 11, "c = 176"),
    (32, 7, "c = 224"),
    (64, 5, "c = 320"),
    (32, 24, "c = 768: one chunk, 1,026 rows per wave > TN_FLUSH"),
]


@pytest.mark.parametrize("b,nq,why", H_SHAPES, ids=[f"b{s[0]}-nq{s[1]}" for s in H_SHAPES])
def test_projected_matrix(engine, b, nq, why):
    """na = nb = nq: H = Q^T W of the dense Rayleigh-Ritz, ts_tn_kernel with many tiles."""
    info = _gram_case(engine, f"H b {b} nq {nq}", N0, b, nq, nq, MFMA)
    if (b, nq) == (32, 24):
        assert info["nchunks"] == 1 and -(-info["rows_per_chunk"] // 4) == 1026 > TN_FLUSH


def test_projected_matrix_several_long_chunks(engine):
    """c = 256 at n = 70,001: 16 chunks, every wave past TN_FLUSH."""
    info = _gram_case(engine, "H b 32 nq 8 n 70,001", 70_001, 32, 8, 8, MFMA)
    assert info["nchunks"] > 1 and -(-info["rows_per_chunk"] // 4) > TN_FLUSH + 8


def test_narrow_flush(engine):
    """ts_tn_narrow_kernel<16, true>: the launcher takes it when rows_per_chunk / 4 (rounded
    down) > TN_FLUSH, from rows_per_chunk = 4,100 on: n > 1024 * 4,099."""
    n = 1024 * 4099 + 1031
    info = _gram_case(engine, "narrow flush", n, 16, 2, 1, NARROW, last_block=True)
    assert info["gram_flush"] == 1 and info["nchunks"] == 1024 and info["rows_per_chunk"] == 4101


# ----------------------------------------------------------------------------- the handle after
def test_handle_left_usable(engine):
    """A fit after either call gives the bits of a fit without it, and the results of the fit
    before it stay readable."""
    fx = load_fixture("er_cfg1")
    layers = fixture_layers(fx)
    d, seed = int(fx["dims"].max()), int(fx["seed"])
    engine.set_layers(layers)

    def fit():
        engine.uase(d, seed=seed)
        return engine.singular_values(), engine.embedding(), engine.left_embedding()

    def results():
        return engine.singular_values(), engine.embedding(), engine.left_embedding()

    fit()
    ref = fit()  # (a fit after a fit, as the ones below are)
    n = layers[0].shape[0]
    rng = np.random.default_rng(3)
    A = rng.standard_normal((3, n, 32), dtype=np.float32)
    calls = [lambda: engine.block_gram(A, A),
             lambda: engine.ortho_pass(A[:2] / np.float32(np.sqrt(n)), A[2], seed=4),
             lambda: engine.ortho_pass(A[:2, :, :8] / np.float32(np.sqrt(n)), A[2, :, :8], seed=4)]
    for call in calls:
        call()
        for a, b in zip(ref, results()):
            assert np.array_equal(a, b)
        for a, b in zip(ref, fit()):
            assert np.array_equal(a, b)


def test_bad_arguments(engine):
    """Every refusal is N2V2R_ERR_BAD_ARG, writes nothing, and leaves the handle working."""
    from node2vec2rank_amd import _lib
    n = 37
    _identity(engine, n)
    big = np.zeros(97 * n * 64, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def gram(eng, b, na, nb, a=big, bb=big, g=True):
        G = np.zeros((776 * 64) ** 2 // 4096, np.float64) if g else None
        st = eng.lib.n2v2r_block_gram(eng.h, b, na, nb, ptr(a), ptr(bb), ptr(G), None)
        assert st == _lib.OK or G is None or not G.any(), "a refused call wrote an output"
        return st

    def opass(eng, b, nq, q=big, cond=-1, **miss):
        outs = {"z": np.zeros(n * 64, np.float32), "gram": np.zeros(776 * 64),
                "xinv": np.zeros(64 * 64), "F": np.zeros(776 * 64, np.float32),
                "flags": np.zeros(64, np.int32), "any_flag": np.zeros(1, np.int32)}
        outs.update(miss)
        st = eng.lib.n2v2r_ortho_pass(eng.h, b, nq, ptr(q), ptr(outs["z"]), 1, 0, cond, 1,
                                      ptr(outs["gram"]), ptr(outs["xinv"]), ptr(outs["F"]),
                                      ptr(outs["flags"]), ptr(outs["any_flag"]), None)
        if st != _lib.OK:
            assert all(o is None or not o.any() for o in outs.values()), "a refused call wrote"
        return st

    assert gram(engine, 16, 3, 2) == _lib.OK and opass(engine, 16, 3) == _lib.OK
    for b in (4, 12, 24, 128):
        assert gram(engine, b, 2, 2) == _lib.ERR_BAD_ARG and opass(engine, b, 2) == _lib.ERR_BAD_ARG
    assert gram(engine, 8, 97, 1) == _lib.ERR_BAD_ARG and gram(engine, 64, 1, 13) == _lib.ERR_BAD_ARG
    assert gram(engine, 16, 0, 1) == _lib.ERR_BAD_ARG and gram(engine, 16, 1, 0) == _lib.ERR_BAD_ARG
    assert opass(engine, 8, 96) == _lib.ERR_BAD_ARG and opass(engine, 32, 24) == _lib.ERR_BAD_ARG
    assert opass(engine, 16, -1) == _lib.ERR_BAD_ARG
    assert opass(engine, 16, 3, cond=2) == _lib.ERR_BAD_ARG
    assert opass(engine, 16, 3, cond=-2) == _lib.ERR_BAD_ARG
    for miss in ("a", "bb"):
        assert gram(engine, 16, 2, 2, **{miss: None}) == _lib.ERR_BAD_ARG, miss
    assert gram(engine, 16, 2, 2, g=False) == _lib.ERR_BAD_ARG
    assert opass(engine, 16, 3, q=None) == _lib.ERR_BAD_ARG
    for miss in ("z", "gram", "xinv", "F", "flags", "any_flag"):
        assert opass(engine, 16, 3, **{miss: None}) == _lib.ERR_BAD_ARG, miss
    assert opass(engine, 8, 3, xinv=None, F=None) == _lib.OK      # b = 8 writes neither
    assert opass(engine, 16, 0, q=None) == _lib.OK                # the start block has no basis
    multi = _lib.Engine.multi([0, 0])                             # a multi-GPU parent handle
    try:
        _identity(multi, N0)
        assert gram(multi, 16, 2, 2) == _lib.ERR_BAD_ARG and opass(multi, 16, 3) == _lib.ERR_BAD_ARG
    finally:
        multi.close()
    fresh = _lib.Engine()                                         # no layers set
    try:
        assert gram(fresh, 16, 2, 2) == _lib.ERR_BAD_ARG and opass(fresh, 16, 3) == _lib.ERR_BAD_ARG
    finally:
        fresh.close()
    assert gram(engine, 16, 3, 2) == _lib.OK and opass(engine, 16, 3) == _lib.OK
