"""Dense layers converted to CSR in HBM after a top-percent cut.

    python tools/sparsify_probe.py [--n 20000] [--samples 200] [--layers 4] [--d 256]
                                   [--tops 25,10,5,1] [--ceiling tools/stream_ceiling]
                                   [--out profiles/sparsify.json]

One BASELINE cfg3 layer set (N = 20k, K = 4, 200 samples; the expression generator of
tools/layer_transform_probe.py) and, for every ``top_percent_keep``, on one GPU:

  * ``Engine.to_csr()``: the host time of the whole call (counts, scan, allocations, compaction
    of the K layers, release of the dense copies), ending in a device synchronise;
  * the count and the compaction kernel alone on one layer (n2v2r_bench_sparsify_pass: HIP
    events around 20 launches), in ms and GB/s of the 4 N^2 layer bytes each reads, and as a
    fraction of the non-temporal dwordx4 read ceiling measured in the same run by
    ``tools/stream_ceiling`` (``hipcc --offload-arch=gfx950 -O3 -o tools/stream_ceiling
    tools/stream_ceiling.hip``) when that program is there;
  * the device-resident ``uase`` (d = --d) on the same layers in dense storage and after the
    conversion: the solver's own ms_total and block applications of the second fit from one seed
    (the first fit of each storage warms up and builds the one-off forms), and the largest
    relative difference of the singular values of the two fits;
  * the HBM in use on the device with the layers dense and after the conversion (hipMemGetInfo;
    the handle's solver workspace is in both), and the layers' own bytes from their shapes.

Prints one JSON line and writes it to ``--out`` when given.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from node2vec2rank_amd import Coexpression, _lib  # noqa: E402


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


def _hbm_used():
    """Bytes in use on the current device (every allocation of the process and of others)."""
    hip = None
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            pass
    if hip is None:
        return None
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        return None
    return int(total.value - free.value)


def _fit(eng, d, seed):
    eng.uase(d, seed=seed, raise_on_no_convergence=False)  # warm-up, one-off layer forms
    eng.synchronize()
    t0 = time.perf_counter()
    st = eng.uase(d, seed=seed, raise_on_no_convergence=False)
    eng.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return {"ms_total": round(st["ms_total"], 2), "wall_ms": round(wall, 2),
            "ms_spmm": round(st["ms_spmm"], 2), "block_applications": st["block_applications"],
            "restarts": st["restarts"], "converged": st["converged"],
            "spmm_form": st["spmm_form"]}, eng.singular_values()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--tops", default="25,10,5,1")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--ceiling", default=os.path.join(REPO, "tools", "stream_ceiling"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, K, d = args.n, args.samples, args.layers, args.d
    ceil = _ceiling(args.ceiling)
    E = [np.random.default_rng(k).standard_normal((n, s)) for k in range(K)]
    eng = _lib.Engine(0)
    lda = (n + 63) // 64 * 64
    runs = []
    for top in [float(t) for t in args.tops.split(",")]:
        eng.set_layers([Coexpression(e, top_percent_keep=top) for e in E])
        eng.synchronize()
        rec = {"top_percent_keep": top, "hbm_used_dense": _hbm_used(),
               "layer_bytes_dense": 4 * n * lda * K}
        kernels = {}
        for which, name in enumerate(["count", "compact"]):
            ms, by = eng.bench_sparsify_pass(0, which, reps=20)
            k = {"ms": round(ms, 4), "GB_per_s": round(by / ms / 1e6, 1)}
            if ceil and ceil.get("nt_GB_per_s"):
                k["frac_of_nt_ceiling"] = round(k["GB_per_s"] / ceil["nt_GB_per_s"], 3)
            kernels[name] = k
        rec["kernels_one_layer"] = kernels
        rec["uase_dense"], s_dense = _fit(eng, d, args.seed)
        eng.synchronize()
        t0 = time.perf_counter()
        nnz = eng.to_csr()
        eng.synchronize()
        rec["to_csr_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["nnz"] = nnz
        rec["density"] = [round(c / (n * n), 5) for c in nnz]
        rec["hbm_used_csr"] = _hbm_used()
        rec["layer_bytes_csr"] = sum(8 * c + 8 * (n + 1) for c in nnz)
        rec["uase_csr"], s_csr = _fit(eng, d, args.seed)
        rec["hbm_used_csr_after_fit"] = _hbm_used()  # (with the column-block forms, if built)
        rec["singular_values_max_rel_diff"] = float(np.max(np.abs(s_csr - s_dense) /
                                                           np.abs(s_dense)))
        rec["csr_over_dense_ms_total"] = round(rec["uase_csr"]["ms_total"] /
                                               rec["uase_dense"]["ms_total"], 3)
        runs.append(rec)
        line = json.dumps({"n": n, "samples": s, "layers": K, "d": d, "seed": args.seed,
                           "stream_ceiling": ceil, "runs": runs})
        print(json.dumps(rec), flush=True)
        if args.out:  # (rewritten after every cut: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    eng.close()
    print(line)


if __name__ == "__main__":
    main()
