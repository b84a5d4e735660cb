"""Threshold / top-percent / binarize of a co-expression layer on the GPU.

    python tools/layer_transform_probe.py [--n 20000] [--samples 200] [--layers 4] [--reps 5]
                                          [--top 5] [--ceiling tools/stream_ceiling]
                                          [--out profiles/layer_transform.json]

At BASELINE cfg3's size (N = 20k, 200 samples, K = 4; the expression generator of
tools/corr_ingest_probe.py) it records, on one GPU:

  * every kernel of ``n2v2r_transform_layer`` alone on one layer (n2v2r_bench_transform_pass:
    HIP events, mean of 20 launches): the four histogram passes of the radix select, the min
    pass and the apply pass, in ms and GB/s (the apply pass reads and writes the layer), and as
    a fraction of the streaming ceiling measured in the same run by ``tools/stream_ceiling``
    (``hipcc --offload-arch=gfx950 -O3 -o tools/stream_ceiling tools/stream_ceiling.hip``; its
    best plain and best non-temporal dwordx4 read figures) when that program is there;
  * the first histogram pass on the co-expression layer against the same pass on a layer of
    the same size whose fp32 bit patterns are uniformly random (NaN and infinity patterns
    excluded), i.e. on keys spread over all 256 top digits: the cost of bin contention;
  * ``Engine.set_layers`` of the K layers with ``top_percent_keep=--top`` against the plain
    load (median of ``--reps`` runs after a warm-up, interleaved), and one whole
    ``transform_layer`` call.

Prints one JSON line and writes it to ``--out`` when given.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from node2vec2rank_amd import Coexpression, _lib  # noqa: E402

PASSES = ["hist0", "hist1", "hist2", "hist3", "min", "apply"]


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _ceiling(path):
    """Best plain and best non-temporal dwordx4 read rate of tools/stream_ceiling, in GB/s."""
    if not path or not os.path.exists(path):
        return None
    out = subprocess.run([path], check=True, capture_output=True, text=True, timeout=120).stdout
    best = {}
    for line in out.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            form = r["form"].split()[0]
            best[form] = max(best.get(form, 0.0), float(r["GB_per_s"]))
    return {"plain_GB_per_s": best.get("plain"), "nt_GB_per_s": best.get("nt")}


def _passes(eng, ceil):
    out = {}
    for which, name in enumerate(PASSES):
        ms, by = eng.bench_transform_pass(0, which, reps=20)
        moved = by * (2 if name == "apply" else 1)
        rec = {"ms": round(ms, 4), "GB_per_s": round(moved / ms / 1e6, 1)}
        if ceil:  # reads are non-temporal; the apply pass loads plainly
            ref = ceil["plain_GB_per_s"] if name == "apply" else ceil["nt_GB_per_s"]
            if ref:
                rec["frac_of_ceiling"] = round(rec["GB_per_s"] / ref, 3)
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top", type=float, default=5.0)
    ap.add_argument("--ceiling", default=os.path.join(REPO, "tools", "stream_ceiling"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, K = args.n, args.samples, args.layers
    ceil = _ceiling(args.ceiling)
    coex = [Coexpression(np.random.default_rng(k).standard_normal((n, s))) for k in range(K)]
    cut = [Coexpression(c.expression, top_percent_keep=args.top) for c in coex]
    eng = _lib.Engine(0)

    eng.set_layers(coex[:1])
    passes = _passes(eng, ceil)
    eng.transform_layer(0, top_percent_keep=args.top)  # warm-up
    eng.set_layers(coex[:1])
    eng.synchronize()
    stats = {}
    call_ms = _timed(lambda: stats.update(eng.transform_layer(0, top_percent_keep=args.top)))

    # uniformly random fp32 bit patterns: exponent 255 (infinities, NaNs) folded onto 127
    bits = np.random.default_rng(99).integers(0, 2 ** 32, size=(n, n), dtype=np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
    eng.set_layers([bits.view(np.float32)], storage="dense", symmetric=_lib.SYM_YES)
    del bits
    uniform = _passes(eng, ceil)

    def load(layers):
        eng.set_layers(layers)
        eng.synchronize()

    forms = {"plain": coex, f"top_percent_keep_{args.top:g}": cut}
    ms = {name: [] for name in forms}
    for rep in range(args.reps + 1):  # rep 0 warms up
        for name, layers in forms.items():
            t = _timed(lambda: load(layers))
            if rep:
                ms[name].append(t)
    eng.close()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 2), "runs_ms": [round(x, 2) for x in v]}

    out = {"n": n, "samples": s, "layers": K, "reps": args.reps, "layer_bytes": 4 * n * n,
           "stream_ceiling": ceil,
           "passes_coexpression": passes, "passes_uniform_keys": uniform,
           "hist0_contention_ratio": round(passes["hist0"]["ms"] / uniform["hist0"]["ms"], 3),
           "transform_layer_call": {"ms": round(call_ms, 3), **stats},
           "set_layers": {k: summary(v) for k, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
