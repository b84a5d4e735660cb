"""bench.py's plain and --full runs and --dump-outputs.

CPU: the writer behind --dump-outputs (names, dtypes, the seeded row sample of outputs over the
budget).  GPU: the smallest configuration (cfg1) through the command line: a plain run prints the
headline keys and none of the --full legs, two runs with the same arguments dump identical arrays,
and --full adds the legs beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ["metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"]
FULL_ONLY = ["device_resident", "cpu_baseline"]


def _bench():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def test_dump_outputs_whole_arrays(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(0)
    arrays = {"distances_1": rng.random((1000, 10)), "borda_ranks_1": np.arange(1000.0)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["borda_ranks_1.npy", "distances_1.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, a)


def test_dump_outputs_sample_is_seeded_and_within_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 96 * 101)  # 101 rows of 88 + 8 bytes
    arrays = {"distances_1": np.arange(5000.0).reshape(500, 10), "borda_ranks_1": np.arange(500.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 101
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 500
    idx = rows.astype(np.int64)
    total = 0
    for name in ("distances_1", "borda_ranks_1", "sample_rows"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
        total += a.nbytes
        if name != "sample_rows":
            np.testing.assert_array_equal(a, arrays[name][idx])
    assert total <= 96 * 101


def _run(*extra):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config",
                        "cfg1", "--steps", "2", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run("--dump-outputs", a)
    _run("--dump-outputs", b)
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "nodes/s"
    assert line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["full"] is False and line["roofline"] is None
    for k in FULL_ONLY:
        assert k not in line, k
    # cfg1: 1000 nodes, one comparison, dim 8 x {cosine, euclidean}
    assert sorted(os.listdir(a)) == ["borda_ranks_1.npy", "distances_1.npy"]
    D = np.load(os.path.join(a, "distances_1.npy"))
    r = np.load(os.path.join(a, "borda_ranks_1.npy"))
    assert D.shape == (1000, 2) and D.dtype == np.float64
    assert r.shape == (1000,) and r.dtype == np.float64
    for f in os.listdir(a):
        np.testing.assert_array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f)))


@pytest.mark.gpu
def test_full_run_adds_the_legs():
    line = _run("--full", "--cpu-sample", "300")
    for k in HEADLINE + FULL_ONLY:
        assert k in line, k
    assert line["full"] is True
    assert line["roofline"]["achieved"] > 0
    assert line["device_resident"]["ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0
