"""The paired apply (needs an MI355X): a pair's two selective passes planned by one small launch
and applied in one read of the basis (dense.hip, pip_pair_kernel; N2V2R_PAIR_APPLY=fused, the
default from 2^19 rows on) against the three-launch path (split: apply, fixup, apply).  Every output element goes through
the same operations in the same order on both paths and the fit is a function of the launches'
outputs alone, so the singular values, the left embedding and the application count must be
equal bit for bit: any difference is a bug.  The switch is read at every fit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(eng, d, fused, **kw):
    os.environ["N2V2R_PAIR_APPLY"] = "fused" if fused else "split"
    try:
        st = eng.uase(d, **kw)
    finally:
        os.environ.pop("N2V2R_PAIR_APPLY", None)
    return eng.singular_values(), eng.left_embedding(), st


def _same(eng, layers, d, min_restarts=0, **kw):
    """Fit twice, fused and split; the fits must agree bit for bit."""
    eng.set_layers(layers)
    s1, x1, st1 = _fit(eng, d, True, **kw)
    s0, x0, st0 = _fit(eng, d, False, **kw)
    print(f"n {layers[0].shape[0]} d {d}: {st1['restarts']} cycles, "
          f"{st1['block_applications']} applications, lean checks {st1['lean_checks']}")
    assert st1["converged"] == d and st1["lean_checks"] > 0, st1
    assert st1["restarts"] >= min_restarts, st1
    for k in ("restarts", "block_applications", "converged", "basis", "lean_checks"):
        assert st1[k] == st0[k], (k, st1, st0)
    assert np.array_equal(s1, s0)
    assert np.array_equal(x1, x0)
    assert np.isfinite(x1).all()
    return st1


def check_padded(eng, d):
    """N = 4,099 (prime: the last 256-row workgroup holds 3 rows), a basis small enough that
    the fit restarts: pairs with and without kept Ritz blocks in front of them."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(4099, 6, 2, seed_base=311)
    _same(eng, layers, d, min_restarts=2, seed=3, max_basis=max(64, 3 * d), keep=max(16, d + d // 2))


@pytest.mark.parametrize("d", [8, 64])
def test_padded_last_workgroup(engine, d):
    check_padded(engine, d)


def test_512_row_workgroups(engine):
    """From 2^19 rows on a workgroup takes 512 rows (4 per lane); 3 rows past a multiple."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers((1 << 19) + 3, 4, 2, seed_base=312)
    _same(engine, layers, 8, seed=3)


def test_basis_768(engine):
    """A basis past 512 columns: the plan's largest block lists and LDS footprint."""
    from node2vec2rank_amd import synthetic
    layers = synthetic.er_layers(20_000, 20, 2, seed_base=313)
    st = _same(engine, layers, 128, seed=5, keep=168, max_basis=768)
    assert st["basis"] == 768, st


def test_row_partitioned():
    """Two thread ranks on device 0: the all-reduced Grams feed the same launches."""
    from node2vec2rank_amd import _lib, synthetic
    layers = synthetic.er_layers(4099, 6, 2, seed_base=311)
    eng = _lib.Engine.multi([0, 0])
    try:
        _same(eng, layers, 8, min_restarts=2, seed=3, max_basis=64, keep=16)
    finally:
        eng.close()


def test_refill_and_cancellation(engine):
    """Exactly rank-deficient blocks (the lowrank_exact layers: rank 8): columns are refilled by
    counter deviates and the sticky flag re-expands cycles; both must match the split path."""
    import scipy.sparse as sp
    from test_oracle_golden import lowrank_exact_layers
    fx = load_fixture("lowrank_exact")
    layers = [sp.csr_matrix(a) for a in lowrank_exact_layers(fx)]
    d = int(fx["dims"].max())
    engine.set_layers(layers)
    s1, x1, st1 = _fit(engine, d, True, seed=int(fx["seed"]))
    s0, x0, st0 = _fit(engine, d, False, seed=int(fx["seed"]))
    print(f"lowrank_exact: {st1['restarts']} cycles, {st1['block_applications']} applications")
    for k in ("restarts", "block_applications", "converged", "basis", "stagnated"):
        assert st1[k] == st0[k], (k, st1, st0)
    assert np.array_equal(s1, s0)
    assert np.array_equal(x1, x0)


CHILD = r"""
import sys
sys.path.insert(0, "tests")
import test_gpu_pair_apply as t
from node2vec2rank_amd import _lib
eng = _lib.Engine(0)
for d in (8, 64):
    t.check_padded(eng, d)
print("PAIR_POISON_OK")
"""


def test_poisoned_lds():
    """The padded-workgroup fits with LDS and scratch poisoned before every solver stage: the
    plan and the apply read nothing they did not write."""
    env = dict(os.environ, N2V2R_POISON="1", N2V2R_DEBUG_FINITE="1")
    env.pop("N2V2R_PAIR_APPLY", None)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "PAIR_POISON_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
