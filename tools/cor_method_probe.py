"""What a Spearman or bicor co-expression layer costs beside the Pearson layer.

    python tools/cor_method_probe.py [--shapes 20000x200,20000x1000,5000x2000] [--reps 10]
                                     [--call-reps 5] [--no-host] [--out profiles/cor_methods.json]

For every shape N x samples, on one GPU and in one process:

  * the row kernels alone (n2v2r_bench_corr_rows: one HIP event pair per launch, median of
    ``--reps`` after a warm-up): ``corr_standardise_kernel`` (the Pearson row pass, for scale),
    ``corr_rank_kernel`` and ``corr_bicor_kernel``;
  * ``Engine.set_layers`` of one ``Coexpression`` layer under each method (upload, row pass, tile
    product; host clock around the call and a synchronise, median of ``--call-reps`` after one
    warm-up, the methods interleaved);
  * ``pick_soft_threshold`` with WGCNA's 15 default powers under each method, timed the same way;
  * the host route the GPU path replaces, one run each (BLAS threads recorded):
    ``scipy.stats.rankdata`` + ``np.corrcoef``, and bicor in numpy (medians, weights, one matmul).

``row_pass_share`` is a method's row kernel time over the Pearson layer build of the same shape.
The Pearson path runs the same kernels in the same order as before the methods existed.
Prints one JSON line and writes it to ``--out`` when given.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from node2vec2rank_amd import Coexpression, _lib, pick_soft_threshold  # noqa: E402

METHODS = ("pearson", "spearman", "bicor")


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _summary(v):
    return {"median_ms": round(statistics.median(v), 3), "runs_ms": [round(x, 3) for x in v]}


def _numpy_bicor(E):
    c = E - np.median(E, axis=1, keepdims=True)
    mad = np.median(np.abs(c), axis=1, keepdims=True)
    u = c / (9.0 * mad)
    a = c * np.where(np.abs(u) < 1.0, (1.0 - u * u) ** 2, 0.0)
    z = a / np.sqrt((a * a).sum(axis=1, keepdims=True))
    return z @ z.T


def _host(E):
    import scipy.stats
    out = {}
    t0 = time.perf_counter()
    r = np.corrcoef(scipy.stats.rankdata(E, axis=1))
    out["rankdata_corrcoef_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    del r
    t0 = time.perf_counter()
    r = _numpy_bicor(E)
    out["numpy_bicor_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    del r
    out["blas_threads"] = os.environ.get("OMP_NUM_THREADS") or os.environ.get(
        "OPENBLAS_NUM_THREADS") or "default"
    return out


def _shape(eng, n, s, reps, call_reps, host):
    E = np.random.default_rng(n + s).standard_normal((n, s))
    out = {"n": n, "samples": s}
    out["row_kernel"] = {m: _summary(eng.bench_corr_rows(E, m, reps).tolist()) for m in METHODS}

    layers = {m: [Coexpression(E, method=m)] for m in METHODS}

    def build(m):
        eng.set_layers(layers[m])
        eng.synchronize()

    ms = {m: [] for m in METHODS}
    for rep in range(call_reps + 1):  # rep 0 warms up (allocations, first launches)
        for m in METHODS:
            t = _timed(lambda: build(m))
            if rep:
                ms[m].append(t)
    out["set_layers"] = {m: _summary(v) for m, v in ms.items()}

    ms = {m: [] for m in METHODS}
    for rep in range(call_reps + 1):
        for m in METHODS:
            t = _timed(lambda: pick_soft_threshold(E, engine=eng, method=m))
            if rep:
                ms[m].append(t)
    out["pick_soft_threshold"] = {m: _summary(v) for m, v in ms.items()}

    base = out["set_layers"]["pearson"]["median_ms"]
    out["row_pass_share"] = {m: round(out["row_kernel"][m]["median_ms"] / base, 4)
                             for m in ("spearman", "bicor")}
    out["set_layers_over_pearson"] = {m: round(out["set_layers"][m]["median_ms"] / base, 3)
                                      for m in ("spearman", "bicor")}
    if host:
        out["host"] = _host(E)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x200,20000x1000,5000x2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--call-reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = _lib.Engine(0)
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")]
    out = {"reps": args.reps, "call_reps": args.call_reps,
           "shapes": [_shape(eng, n, s, args.reps, args.call_reps, not args.no_host)
                      for n, s in shapes]}
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
