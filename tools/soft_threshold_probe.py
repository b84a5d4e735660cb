"""The soft-threshold scan on the GPU against the two routes it replaces.

    python tools/soft_threshold_probe.py [--n 20000] [--samples 200] [--reps 5] [--host-reps 1]
                                         [--skip-host] [--out profiles/soft_threshold.json]

At BASELINE cfg3's size (N = 20k, 200 samples; rows that mix 8 latent factors plus noise, so the
correlations spread and high powers do not vanish) with WGCNA's 15 default powers it records, on
one GPU, each figure the median of ``--reps`` runs after a warm-up:

  * ``soft_conn_kernel`` alone (n2v2r_soft_connectivity_chunks: one HIP event pair around its
    launch), the pow() evaluations per second it reaches (n^2 P / time) and its chunk count;
  * the same with the single power 1, which takes no pow() at all: the tile product, the pass
    through LDS and the row sums.  The 15 powers run as two groups of <= 8, each with a product of
    its own, so the product's share of the 15-power launch is 2 x that time over the launch's;
  * one whole ``Engine.soft_connectivity`` call (upload, standardise, scan, chunk sum, download)
    and ``pick_soft_threshold`` (the call plus the host fits);
  * route (a), the host: ``np.corrcoef`` and, per power, ``(t ** p).sum(axis=1)`` in fp64, in
    row blocks of 2,000 so that the powers need no second N x N array.  The BLAS thread count is
    printed with it (threadpoolctl when it is installed, else the environment's).  One run per
    ``--host-reps``, no warm-up: a numpy pass over fresh arrays has nothing to warm;
  * route (b), the engine without the scan: per power ``set_layers([Coexpression(E, power=p)])``
    and ``column_sums(0)`` (fp32 sums of the fp32 layer, diagonal included; it replaces the
    handle's layers).

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
from node2vec2rank_amd.soft_threshold import DEFAULT_POWERS  # noqa: E402


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


def _expression(n, s, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 8)) @ rng.standard_normal((8, s))
    return x + rng.standard_normal((n, s))


def host_connectivity(E, powers, block=2000):
    """Route (a): numpy fp64, unsigned kind, diagonal excluded."""
    t = np.abs(np.clip(np.corrcoef(E), -1.0, 1.0))
    np.fill_diagonal(t, 0.0)
    out = np.empty((len(powers), E.shape[0]))
    for r0 in range(0, E.shape[0], block):
        rows = t[r0:r0 + block]
        for q, p in enumerate(powers):
            out[q, r0:r0 + block] = (rows if p == 1.0 else rows ** p).sum(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, reps = args.n, args.samples, args.reps
    powers = list(DEFAULT_POWERS)
    P = len(powers)
    E = _expression(n, s)
    eng = _lib.Engine(0)

    kern, kern1, call, pick = [], [], [], []
    chunks = None
    conn = None
    for rep in range(reps + 1):  # rep 0 warms up
        conn, chunks, ms = eng.soft_connectivity_chunks(E, powers=powers)
        _, _, ms1 = eng.soft_connectivity_chunks(E, powers=[1.0])
        t = _timed(lambda: eng.soft_connectivity(E, powers=powers))  # (ends in a synchronise)
        tp = _timed(lambda: pick_soft_threshold(E, powers=powers, engine=eng))
        if rep:
            kern.append(ms)
            kern1.append(ms1)
            call.append(t)
            pick.append(tp)
    kernel = _summary(kern)
    kernel["chunks"] = chunks
    kernel["pow_evaluations"] = float(n) * n * (P - 1)  # (power 1 takes none)
    kernel["entries_times_powers"] = float(n) * n * P
    kernel["G_pow_per_s"] = round(kernel["pow_evaluations"] / kernel["median_ms"] / 1e6, 2)
    kernel["G_entry_powers_per_s"] = round(kernel["entries_times_powers"] /
                                           kernel["median_ms"] / 1e6, 2)
    product = _summary(kern1)
    groups = (P + 7) // 8
    product["groups_in_full_launch"] = groups
    product["share_of_full_launch"] = round(groups * product["median_ms"] / kernel["median_ms"], 4)
    out = {"n": n, "samples": s, "reps": reps, "powers": powers, "kind": "unsigned",
           "soft_conn_kernel": kernel, "soft_conn_kernel_power_1_only": product,
           "soft_connectivity_call": _summary(call), "pick_soft_threshold": _summary(pick),
           "bytes_uploaded": 8 * n * s, "bytes_downloaded": 8 * P * n}

    # route (b): what the engine offered before the scan
    route_b, kb = [], None
    for rep in range(reps + 1):
        def per_power():
            sums = []
            for p in powers:
                eng.set_layers([Coexpression(E, power=p)])
                sums.append(eng.column_sums(0))
            return np.stack(sums)
        box = {}
        t = _timed(lambda: box.update(k=per_power()))
        kb = box["k"]
        if rep:
            route_b.append(t)
    out["route_b_layer_per_power"] = _summary(route_b)
    out["route_b_layer_per_power"]["layer_bytes_written_and_read"] = 2 * P * 4 * n * n
    rel_b = np.abs((kb.astype(np.float64) - 1.0) - conn) / np.maximum(conn, 1e-300)
    out["route_b_layer_per_power"]["max_rel_diff_vs_scan"] = float(rel_b.max())
    out["route_b_over_scan_call"] = round(out["route_b_layer_per_power"]["median_ms"] /
                                          out["soft_connectivity_call"]["median_ms"], 2)

    if not args.skip_host:
        print("host BLAS threads:", json.dumps(_blas_threads()), flush=True)
        host, kh = [], None
        for rep in range(args.host_reps):
            box = {}
            t = _timed(lambda: box.update(k=host_connectivity(E, powers)))
            kh = box["k"]
            host.append(t)
            print(f"host route run {rep}: {t:.0f} ms", flush=True)
        out["route_a_host_numpy"] = _summary(host)
        out["route_a_host_numpy"]["blas_threads"] = _blas_threads()
        out["route_a_host_numpy"]["corr_bytes"] = 8 * n * n
        rel_a = np.abs(kh - conn) / np.maximum(np.abs(kh), 1e-300)
        out["route_a_host_numpy"]["max_rel_diff_vs_scan"] = float(rel_a.max())
        out["route_a_over_scan_call"] = round(out["route_a_host_numpy"]["median_ms"] /
                                              out["soft_connectivity_call"]["median_ms"], 1)
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
