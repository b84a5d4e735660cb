"""One orthogonalisation pass at block width 8 on its own (``n2v2r_pip_pass``: the solver's
launchers ``n2v2r_launch_ts_tn`` + ``n2v2r_launch_pip_fused``, or for a pair
``n2v2r_launch_ts_tn2`` and the three-launch / paired-apply forms) against numpy.

Inputs.  Q is the fp32 rounding of an fp64 QR factor (nq blocks of n x 8).  Z = Q_S A + W: S is
a chosen set of blocks, A has entries of (1 .. 2) * 1e-2 * ||w_j|| so that
max_ij |C_ij| / ||z_j|| ~ 2e-2 on S, and W (columns of norm 1 .. 2) is orthogonalised against all
of Q in fp64 before the rounding, which leaves ~1e-7 on the other blocks.  With tau = 1e-4 the
selective decision then sits orders of magnitude from either side; every case checks on the CPU,
from the fp64 Gram of the fp32 arrays, that each block is at least 100 x away from tau.

Gram bound (derived, not measured).  The streaming Gram kernels give every lane at most
TS_MAX_CHUNK / 32 = 256 rows of a chunk: an fp32 FMA chain s <- fl32(s + x z) of m <= 256 exact
products, which obeys |s - sum| <= gamma32_m sum |x||z|, gamma32_m = m u32 / (1 - m u32),
u32 = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: one rounding per
term).  The lane sums are converted to fp64 exactly and added in fp64 (the reduce-scatter over
the 32 row lanes, then the chunks): at most n further additions in total, a factor
(1 + gamma64_n), u64 = 2^-53.  Together
    |G - X^T Z| <= (gamma32_256 + gamma64_n + gamma32_256 gamma64_n) |X|^T |Z|
against the same product in np.longdouble, the form of bound tests/test_gpu_project.py uses
with the fp32 term in front.

Output bound.  An output entry is an fp32 chain of 8 |S| subtractions and up to 8 products with
R^{-1}, on fp32 roundings of C and R^{-1}: with k = 8 |S| + 16
    |Z' - (Z - Q_S C_S) R^{-1}| <= gamma32_k (|Z| + |Q_S| |C_S|) |R^{-1}|,
both sides in np.longdouble from the returned Gram's coefficients rounded to fp32 and the
returned R (for a pair, whose R is not returned: numpy's Cholesky factor of the returned Gram,
which the single-pass tests show equal to the GPU's to R_RTOL).

Shapes: the smallest at which each branch is taken.  n = 4,099 is prime, so the last 256-row
workgroup holds 3 rows; nq = 1 a single block; 5 one batch of QB = 4 blocks and a tail block;
70 blocks past the first 64-wide ballot round; 81 (c = 648) the largest basis whose LDS stays
within 64 KB and 82 the first past it (the attribute path: 8 ((c + 8) 8 + 256) + 4 (8 c + 64) +
16 + 4 max(c / 8, 64) bytes is 65,364 at c = 648 and 66,136 at c = 656); n = 2^19 + 3 the
512-row workgroups (NU = 4, QB = 2)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAU = 1e-4
U32 = 2.0 ** -24
U64 = 2.0 ** -53
N0 = 4099
NBIG = 2 ** 19 + 3
# |R - chol(P)^T|_max / |R|_max.  Measured on an MI355X over the single-pass cases below: between
# 1.1e-16 and 2.6e-16 (a few fp64 roundings on an 8 x 8 factor with cond(P) < 10); 10 x the largest
# for other seeds.
R_RTOL = 2.6e-15

# (n, nq, S): S the blocks Z is coupled to
SINGLE = [(N0, 1, (0,)), (N0, 5, (1, 4)), (N0, 70, (0, 3, 63, 64, 69)), (N0, 81, (2, 64, 80)),
          (N0, 82, (2, 64, 81)), (NBIG, 5, (0, 2, 4))]
PAIR_SHAPES = [(N0, 5), (N0, 70), (NBIG, 5)]


def _gamma(k, u):
    return k * u / (1.0 - k * u)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _basis(n, ncol, seed):
    """(Q64, Q32): the fp64 QR factor of a random n x ncol matrix (by Cholesky QR, twice: the
    same factor as Householder's up to signs, orthonormal to fp64 rounding, in two BLAS calls
    per round) and its fp32 rounding."""
    q64 = np.random.default_rng(seed).standard_normal((n, ncol))
    for _ in range(2):
        q64 = np.linalg.solve(np.linalg.cholesky(q64.T @ q64), q64.T).T
    assert np.abs(q64.T @ q64 - np.eye(ncol)).max() < 1e-13
    return q64, q64.astype(np.float32)


def _orth_against(w, *bases):
    for _ in range(2):
        for q in bases:
            w = w - q @ (q.T @ w)
    return w


def _coupled(rng, q64, w, S):
    """Q_S A + W in fp64, |A_ij| = (1 .. 2) * 1e-2 * ||w_j||."""
    z = w.copy()
    wn = np.linalg.norm(w, axis=0)
    for k in S:
        a = rng.uniform(1.0, 2.0, (8, 8)) * rng.choice([-1.0, 1.0], (8, 8)) * 1e-2 * wn
        z += q64[:, 8 * k:8 * k + 8] @ a
    return z


@functools.lru_cache(maxsize=None)
def _single_case(n, nq, S):
    """(Q as (nq, n, 8) fp32, Z fp32)."""
    q64, q32 = _basis(n, 8 * nq, 100 + nq)
    rng = np.random.default_rng(7 * n + nq)
    w = _orth_against(rng.standard_normal((n, 8)) / np.sqrt(n), q64) * rng.uniform(1.0, 2.0, 8)
    z = _coupled(rng, q64, w, S).astype(np.float32)
    Q = np.ascontiguousarray(q32.reshape(n, nq, 8).transpose(1, 0, 2))
    return _ro(Q, z)


def _gram64(blocks, z):
    """fp64 Gram of the fp32 arrays: (len(blocks), 8, 8)."""
    z64 = z.astype(np.float64)
    return np.stack([b.astype(np.float64).T @ z64 for b in blocks])


def _applied_on_cpu(g64, tau):
    """The blocks a selective pass applies, from the fp64 Gram g64 = [Q Z]^T Z; asserts that
    every block's max_ij |C_ij| / ||z_j|| is at least 100 x away from tau."""
    zn = np.sqrt(np.diag(g64[-1]))
    ratio = np.array([(np.abs(c) / zn).max() for c in g64[:-1]])
    assert ((ratio >= 100 * tau) | (ratio <= tau / 100)).all(), ratio
    return tuple(int(k) for k in np.flatnonzero(ratio > tau))


def _longdouble_gram(blocks, z):
    """([X]^T Z, |X|^T |Z|) in np.longdouble, one 8 x 8 per block."""
    zl = z.astype(np.longdouble)
    ref = np.stack([np.einsum("ni,nj->ij", b.astype(np.longdouble), zl) for b in blocks])
    mag = np.stack([np.einsum("ni,nj->ij", np.abs(b).astype(np.longdouble), np.abs(zl))
                    for b in blocks])
    return ref, mag


@functools.lru_cache(maxsize=None)
def _single_ref(n, nq, S):
    Q, z = _single_case(n, nq, S)
    return _ro(*_longdouble_gram(list(Q) + [z], z))


def _assert_gram(got, ref, mag, n, what):
    g32, g64 = _gamma(256, U32), _gamma(n, U64)
    bound = np.longdouble(g32 + g64 + g32 * g64) * mag
    err = np.abs(got.astype(np.longdouble) - ref)
    frac = float((err / bound).max())
    print(f"{what}: Gram worst |got - ref| / bound = {frac:.4f}")
    assert (err <= bound).all(), frac


def _mm(a, b):
    """a @ b in np.longdouble (einsum: numpy's longdouble matmul is several times slower)."""
    return np.einsum("nk,kj->nj", a, b)


def _p_of(gram, applied):
    """P = Z^T Z - C_S^T C_S in np.longdouble from a Gram (nblk + 1, 8, 8), applied rows only."""
    gl = gram.astype(np.longdouble)
    p = (gl[-1] + gl[-1].T) / 2
    for k in applied:
        p = p - gl[k].T @ gl[k]
    return p


def _assert_output(zout, blocks, z, gram, applied, R, what):
    """|Z' - (Z - Q_S C_S) R^{-1}| <= gamma32_k (|Z| + |Q_S| |C_S|) |R^{-1}|, k = 8 |S| + 16."""
    rinv = np.linalg.inv(R).astype(np.float32).astype(np.longdouble)
    num = z.astype(np.longdouble)
    mag = np.abs(num)
    for k in applied:
        cf = gram[k].astype(np.float32).astype(np.longdouble)
        ql = blocks[k].astype(np.longdouble)
        num = num - _mm(ql, cf)
        mag = mag + _mm(np.abs(ql), np.abs(cf))
    ref = _mm(num, rinv)
    bound = np.longdouble(_gamma(8 * len(applied) + 16, U32)) * _mm(mag, np.abs(rinv))
    err = np.abs(zout.astype(np.longdouble) - ref)
    frac = float((err / bound).max())
    print(f"{what}: output worst |got - ref| / bound = {frac:.4f}")
    assert (err <= bound).all(), frac


def _r_error(R, p):
    ref = np.linalg.cholesky(np.asarray(p, dtype=np.float64)).T
    assert np.array_equal(np.tril(R, -1), np.zeros((8, 8)))
    return float(np.abs(R - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------- a. one pass against numpy
@pytest.mark.parametrize("tau", [TAU, 0.0])
@pytest.mark.parametrize("n,nq,S", SINGLE)
def test_single_pass_against_numpy(engine, n, nq, S, tau):
    Q, z = _single_case(n, nq, S)
    g64 = _gram64(list(Q) + [z], z)
    assert _applied_on_cpu(g64, TAU) == S
    applied = S if tau > 0 else tuple(range(nq))
    assert np.linalg.cond(np.asarray(_p_of(g64, applied), dtype=np.float64)) < 10
    out = engine.pip_pass(Q, z, tau=tau, first=0, seed=5)
    what = f"n {n} nq {nq} tau {tau:g}"
    # the applied set, read from the histogram (not counted when every block is applied)
    hist = out["skipped"]
    assert hist[0] == 0
    assert tuple(np.flatnonzero(hist[1:])) == (S if tau > 0 else ())
    assert (hist[1:] <= 1).all()
    assert not out["flags"].any() and out["any_flag"] == 0
    ref, mag = _single_ref(n, nq, S)
    _assert_gram(out["gram"], ref, mag, n, what)
    err = _r_error(out["R"], _p_of(out["gram"], applied))
    print(f"{what}: R error {err:.3e}")
    assert err <= R_RTOL, err
    _assert_output(out["Za"], Q, z, out["gram"], applied, out["R"], what)


def test_skipped_pass_leaves_block_untouched(engine):
    """S empty and Z orthonormal: nothing to apply.  R = I, Z bit for bit, skipped[0] counted."""
    n, nq = N0, 5
    q64, q32 = _basis(n, 8 * nq + 8, 31)
    Q = np.ascontiguousarray(q32[:, :8 * nq].reshape(n, nq, 8).transpose(1, 0, 2))
    z = np.ascontiguousarray(q32[:, 8 * nq:])
    assert _applied_on_cpu(_gram64(list(Q) + [z], z), TAU) == ()
    assert np.abs(_gram64([z], z)[0] - np.eye(8)).max() < TAU / 100
    out = engine.pip_pass(Q, z, tau=TAU, first=0, seed=5)
    assert np.array_equal(out["R"], np.eye(8))
    assert out["Za"].tobytes() == z.tobytes()
    assert out["skipped"].tolist() == [1] + [0] * nq
    assert not out["flags"].any() and out["any_flag"] == 0


# ------------------------------------------------------------------- b. breakdown columns
@pytest.mark.parametrize("first", [0, 1])
def test_zero_column_is_flagged_and_refilled(engine, first):
    n, nq, S = SINGLE[1]
    Q, z0 = _single_case(n, nq, S)
    z = z0.copy()
    z[:, 3] = 0.0
    a = engine.pip_pass(Q, z, tau=TAU, first=first, seed=11)
    b = engine.pip_pass(Q, z, tau=TAU, first=first, seed=11)
    c = engine.pip_pass(Q, z, tau=TAU, first=first, seed=12)
    assert a["flags"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and a["any_flag"] == 1
    assert not a["R"][3].any()
    assert np.isfinite(a["Za"][:, 3]).all()
    assert a["Za"][:, 3].tobytes() == b["Za"][:, 3].tobytes()
    assert not np.array_equal(a["Za"][:, 3], c["Za"][:, 3])
    # the refill is N(0, 1) deviates, not a constant
    assert 0.9 < a["Za"][:, 3].std() < 1.1
    # the other columns do not depend on the seed
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert a["Za"][:, keep].tobytes() == c["Za"][:, keep].tobytes()


def test_duplicate_column_is_clamped_then_refilled(engine):
    """A column that copies another: its pivot cancels.  The block's first pass clamps the pivot
    and keeps the column (flag clear, any_flag set); a later pass flags and refills it."""
    n, nq, S = SINGLE[1]
    Q, z0 = _single_case(n, nq, S)
    z = z0.copy()
    z[:, 6] = z[:, 2]
    a = engine.pip_pass(Q, z, tau=TAU, first=1, seed=11)
    assert not a["flags"].any() and a["any_flag"] == 1
    assert np.isfinite(a["Za"]).all()
    b = engine.pip_pass(Q, z, tau=TAU, first=0, seed=11)
    assert b["flags"].tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and b["any_flag"] == 1
    assert not b["R"][6].any()
    assert 0.9 < b["Za"][:, 6].std() < 1.1
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert a["Za"][:, keep].tobytes() == b["Za"][:, keep].tobytes()


# ------------------------------------------------------------------- c. the pair, both forms
def _pair_sets(nq):
    """(S_a, S_b): the old blocks Za and Zb are coupled to."""
    last = nq - 1
    return ((0, last), (1, last)) if nq <= 5 else ((0, 3, 64, last), (3, 63, 65, last))


@functools.lru_cache(maxsize=None)
def _pair_case(n, nq, kind):
    """(Q, Za, Zb).  kind 'both': both blocks coupled to Q, Zb also to Za; 'a_done': Za already
    orthonormal against Q; 'b_done': Zb already orthonormal against [Q Za']."""
    q64, q32 = _basis(n, 8 * nq + 16, 200 + nq)
    qo, wa, wb = q64[:, :8 * nq], q64[:, 8 * nq:8 * nq + 8], q64[:, 8 * nq + 8:]
    rng = np.random.default_rng(13 * n + nq)
    sa, sb = _pair_sets(nq)
    za = wa if kind == "a_done" else _coupled(rng, qo, wa * rng.uniform(1.0, 2.0, 8), sa)
    if kind == "b_done":
        zb = wb
    else:
        w = wb * rng.uniform(1.0, 2.0, 8)
        mix = rng.uniform(1.0, 2.0, (8, 8)) * rng.choice([-1.0, 1.0], (8, 8)) * 1e-2
        zb = _coupled(rng, qo, w, sb) + wa @ (mix * np.linalg.norm(w, axis=0))
    Q = np.ascontiguousarray(q32[:, :8 * nq].reshape(n, nq, 8).transpose(1, 0, 2))
    return _ro(Q, za.astype(np.float32), zb.astype(np.float32))


def _run_pair(engine, n, nq, kind, tau=TAU):
    Q, za, zb = _pair_case(n, nq, kind)
    f0 = engine.pip_pass(Q, za, zb, tau=tau, form=0, seed=21)
    f1 = engine.pip_pass(Q, za, zb, tau=tau, form=1, seed=21)
    for key in ("Za", "Zb", "flags", "skipped", "gram"):
        assert f0[key].tobytes() == f1[key].tobytes(), key
    assert f0["any_flag"] == f1["any_flag"]
    return Q, za, zb, f1


def _check_pair(Q, za, zb, out, n, nq, kind, tau=TAU):
    what = f"pair {kind} n {n} nq {nq} tau {tau:g}"
    sa, sb = _pair_sets(nq)
    sa = () if kind == "a_done" else sa
    sb = () if kind == "b_done" else sb + (nq,)
    blocks_a, blocks_b = list(Q), list(Q) + [out["Za"]]
    assert _applied_on_cpu(_gram64(blocks_a + [za], za), TAU) == sa
    assert _applied_on_cpu(_gram64(blocks_b + [zb], zb), TAU) == sb
    hist = out["skipped"]
    want = np.zeros(nq + 2, dtype=np.int64)
    want[0] = (kind == "a_done") + (kind == "b_done")
    if tau > 0:
        for k in sa + sb:
            want[1 + k] += 1
    assert hist.tolist() == want.tolist()
    assert not out["flags"].any() and out["any_flag"] == 0
    if kind == "a_done":
        assert out["Za"].tobytes() == za.tobytes()
    if kind == "b_done":
        assert out["Zb"].tobytes() == zb.tobytes()
        return
    # Zb' against the reference built from [Q Za'], Za' as the GPU returned it
    gb = out["gram"][1]  # rows: Q, Za' (the corrected rows), Zb's own
    applied = sb if tau > 0 else tuple(range(nq + 1))
    p = np.asarray(_p_of(gb, applied), dtype=np.float64)
    assert np.linalg.cond(p) < 10
    _assert_output(out["Zb"], blocks_b, zb, gb, applied, np.linalg.cholesky(p).T, what)


@pytest.mark.parametrize("n,nq", PAIR_SHAPES)
def test_pair_forms_bit_equal_and_within_bound(engine, n, nq):
    Q, za, zb, out = _run_pair(engine, n, nq, "both")
    _check_pair(Q, za, zb, out, n, nq, "both")


def test_pair_every_block_applied(engine):
    n, nq = PAIR_SHAPES[0]
    Q, za, zb, out = _run_pair(engine, n, nq, "both", tau=0.0)
    _check_pair(Q, za, zb, out, n, nq, "both", tau=0.0)


@pytest.mark.parametrize("kind", ["a_done", "b_done"])
def test_pair_with_one_pass_skipped(engine, kind):
    """Za already orthonormal to Q while Zb is not (pass a skipped whole, Zb still takes Za from
    memory), and the reverse (pass b skipped whole): skip_a, skip_b and b_za of the paired apply."""
    n, nq = PAIR_SHAPES[0]
    Q, za, zb, out = _run_pair(engine, n, nq, kind)
    _check_pair(Q, za, zb, out, n, nq, kind)
