"""Ingest of co-expression layers: expression matrices against N x N arrays.

    python tools/corr_ingest_probe.py [--n 20000] [--samples 200] [--layers 4] [--d 256]
                                      [--reps 5] [--out profiles/corr_ingest.json]

At BASELINE cfg3's size (N = 20k, 200 samples, K = 4) it times, on one GPU and in one process:

  * ``Engine.set_layers`` of K ``Coexpression`` layers (n2v2r_set_layer_corr: 8 N samples bytes
    up, the layer built in HBM), and
  * ``Engine.set_layers`` of the same K layers as dense float32 N x N arrays
    (n2v2r_set_layer_dense: 4 N^2 bytes of pageable host memory up per layer), with the
    defaults ``N2V2R`` uses and, as the array path's floor, with ``symmetric=SYM_YES``,

median of ``--reps`` runs each after one warm-up, the two forms interleaved; and the whole
``N2V2R(...).fit_transform_rank()`` call both ways (a fresh model per run, same seed).  The
dense arrays are the Coexpression layers read back with ``Engine.layer_dense``, so both forms
load the same bits; the host-side cost of building such arrays with numpy is not in either
figure.  Prints one JSON line and writes it to ``--out`` when given.
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
from node2vec2rank_amd.model import N2V2R  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, K = args.n, args.samples, args.layers
    coex = [Coexpression(np.random.default_rng(k).standard_normal((n, s))) for k in range(K)]
    eng = _lib.Engine(0)
    eng.set_layers(coex)
    arrays = [eng.layer_dense(k) for k in range(K)]

    def load_coex():
        eng.set_layers(coex)
        eng.synchronize()

    def load_dense():  # as N2V2R loads arrays: storage chosen by density, symmetry detected
        eng.set_layers(arrays)
        eng.synchronize()

    def load_dense_sym():  # the cheapest form of the array path: no A^T, no comparison
        eng.set_layers(arrays, storage="dense", symmetric=_lib.SYM_YES)
        eng.synchronize()

    forms = {"coexpression": load_coex, "dense_arrays": load_dense,
             "dense_arrays_sym_yes": load_dense_sym}
    ms = {name: [] for name in forms}
    for rep in range(args.reps + 1):  # rep 0 warms up (allocations, first launches)
        for name, fn in forms.items():
            t = _timed(fn)
            if rep:
                ms[name].append(t)
    eng.close()

    nodes = [f"g{i}" for i in range(n)]
    config = dict(embed_dimensions=[args.d], distance_metrics=["cosine", "euclidean"],
                  comp_strategy="sequential", seed=7, verbose=-1)
    api = {"coexpression": [], "dense_arrays": []}
    for rep in range(args.reps + 1):
        for name, graphs in (("coexpression", coex), ("dense_arrays", arrays)):
            model = N2V2R(graphs, nodes, dict(config))
            t = _timed(model.fit_transform_rank)
            if rep:
                api[name].append(t)
            del model

    def summary(v):
        return {"median_ms": round(statistics.median(v), 2), "runs_ms": [round(x, 2) for x in v]}

    out = {"n": n, "samples": s, "layers": K, "d": args.d, "reps": args.reps,
           "upload_bytes": {"coexpression": 8 * n * s * K, "dense": 4 * n * n * K},
           "set_layers": {k: summary(v) for k, v in ms.items()},
           "fit_transform_rank": {k: summary(v) for k, v in api.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
