"""Topological-overlap (TOM) layers on the GPU against the host route they replace.

    python tools/tom_probe.py [--n 20000] [--samples 200] [--reps 5] [--skip-host]
                              [--out profiles/tom_layer.json]

At BASELINE cfg3's size (N = 20k, 200 samples; the expression generator of
tools/corr_ingest_probe.py) it records, on one GPU, each figure the median of ``--reps`` runs
after a warm-up:

  * ``tom_tile_kernel`` alone (n2v2r_bench_tom_tiles: one HIP event pair per launch) and the fp64
    FLOP/s it reaches, over the flop of the upper-triangle tiles it computes (about n^3), beside
    the ~79 TFLOP/s fp64 peak SURVEY.md App. B lists;
  * one whole ``Engine.tom_layer`` call (validation, row sums, tiles, the synchronise at its end;
    a host clock around a call that ends in a device synchronise);
  * ``Engine.set_layers`` of one ``Coexpression`` layer with and without ``tom="unsigned"``;
  * the host route on the same box: ``layer_dense`` (read-back), the numpy fp64 ``tom()`` of
    tests/test_gpu_tom.py, ``set_layers`` of the float32 result.  The BLAS thread count is
    printed with it (threadpoolctl when it is installed, else the environment's).

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

from node2vec2rank_amd import Coexpression, _lib  # noqa: E402

PEAK_FP64_TFLOPS = 79.0


def tom(A, kind="unsigned"):
    A = A.astype(np.float64)
    np.fill_diagonal(A, 0.0)
    L = A @ A
    absA = np.abs(A) if kind == "signed" else A
    k = absA.sum(axis=1)
    L += A
    if kind == "signed":
        np.abs(L, out=L)
    den = np.minimum.outer(k, k)
    den += 1.0
    den -= absA
    L /= den
    np.fill_diagonal(L, 1.0)
    return L


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return {"source": "threadpoolctl",
                "pools": [{"api": p.get("internal_api"), "threads": p.get("num_threads")}
                          for p in threadpool_info()]}
    except ImportError:
        return {"source": "environment",
                "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"),
                "OPENBLAS_NUM_THREADS": os.environ.get("OPENBLAS_NUM_THREADS"),
                "MKL_NUM_THREADS": os.environ.get("MKL_NUM_THREADS"),
                "cpu_count": os.cpu_count()}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _summary(v):
    return {"median_ms": round(statistics.median(v), 3), "runs_ms": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, reps = args.n, args.samples, args.reps
    plain = Coexpression(np.random.default_rng(0).standard_normal((n, s)))
    with_tom = Coexpression(plain.expression, tom="unsigned")
    eng = _lib.Engine(0)

    def load(layer):
        eng.set_layers([layer])
        eng.synchronize()

    load(plain)
    kernel_ms, flop = eng.bench_tom_tiles(0, reps=reps)  # (its own warm-up launch inside)
    kernel = _summary(list(kernel_ms))
    kernel["flop"] = flop
    kernel["TFLOP_per_s"] = round(flop / kernel["median_ms"] / 1e9, 2)
    kernel["peak_fp64_TFLOP_per_s"] = PEAK_FP64_TFLOPS
    kernel["frac_of_peak"] = round(kernel["TFLOP_per_s"] / PEAK_FP64_TFLOPS, 3)

    call, loads = [], {"plain": [], "tom_unsigned": []}
    for rep in range(reps + 1):  # rep 0 warms up
        load(plain)
        t = _timed(lambda: eng.tom_layer(0))  # (synchronises before it returns)
        if rep:
            call.append(t)
    for rep in range(reps + 1):
        for name, layer in (("plain", plain), ("tom_unsigned", with_tom)):
            t = _timed(lambda: load(layer))
            if rep:
                loads[name].append(t)

    out = {"n": n, "samples": s, "reps": reps, "layer_bytes": 4 * n * n,
           "tom_tile_kernel": kernel, "tom_layer_call": _summary(call),
           "set_layers": {k: _summary(v) for k, v in loads.items()}}

    if not args.skip_host:
        # no warm-up run here: a numpy pass over fresh arrays has nothing to warm, and one run
        # takes tens of seconds
        host = {"read_back": [], "numpy_tom": [], "set_layers_array": [], "total": []}
        worst = None
        print("host BLAS threads:", json.dumps(_blas_threads()), flush=True)
        for rep in range(reps):
            load(plain)
            box = {}
            t0 = _timed(lambda: box.update(A=eng.layer_dense(0)))
            t1 = _timed(lambda: box.update(T=tom(box["A"]).astype(np.float32)))

            def up():
                eng.set_layers([box["T"]], storage="dense", symmetric=_lib.SYM_YES)
                eng.synchronize()
            t2 = _timed(up)
            for key, t in zip(host, (t0, t1, t2, t0 + t1 + t2)):
                host[key].append(t)
            print(f"host route run {rep}: {t0:.0f} + {t1:.0f} + {t2:.0f} ms", flush=True)
            if worst is None:  # the GPU result against the host's, once
                load(with_tom)
                worst = float(np.abs(eng.layer_dense(0).astype(np.float64) - box["T"]).max())
        out["host_route"] = {k: _summary(v) for k, v in host.items()}
        out["host_route"]["blas_threads"] = _blas_threads()
        out["host_route"]["max_abs_diff_gpu_vs_host_fp32"] = worst
        gpu_ms = (out["set_layers"]["tom_unsigned"]["median_ms"] -
                  out["set_layers"]["plain"]["median_ms"])
        out["host_route_over_gpu_tom"] = round(out["host_route"]["total"]["median_ms"] / gpu_ms, 1)
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
