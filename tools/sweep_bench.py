"""Concurrent rho sweep against the sequential one, measured in one process on one GPU.

    python tools/sweep_bench.py [--rows a,b,c] [--steps 20] [--warmup 3] [--out FILE]

Rows (every timed step includes the set-up from the raw shards -- Gram + inverses -- like bench.py's
headline; a step ends in a stream sync; min / median / max over the steps):

  a  sequential: ``chain_admm(refresh=True)`` at rho = 3, 5, 7 to 1e-8, the sum of the three per step
     (run it with GADMM_NATIVE_LIB=<another build> too: the single solve's A/B);
  b  concurrent: ``chain_admm_sweep(refresh=True)`` of the same three in one launch;
  c  co-running penalty: K = 1, 2, 4, 8 members all at rho = 3; time per step over the K = 1 time.

``--rows b`` alone is the run to put under ``rocprofv3 --kernel-trace --stats`` (row d of
profiles/sweep/README.md): one chain_blocked_sweep_kernel, one Gram and one inverse launch per step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gadmm_amd.algorithms import chain_admm, chain_admm_sweep  # noqa: E402
from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.ops import native  # noqa: E402


def timed(step, steps, warmup, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b,c")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    rows = [r for r in a.rows.split(",") if r]
    native.require()
    dev = torch.device("cuda", 0)
    ds = linear_synthetic(24)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    obj0 = model.optimum()
    ids = list(range(24))
    rhos = (3.0, 5.0, 7.0)
    opts = {"refresh": True, "state": False, "residual": False}
    results = []

    def emit(rec):
        rec["native_lib"] = native.library_path()
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        results.append(line)

    if "a" in rows:
        def seq():
            return [chain_admm(model, ids, 24, rho, obj0, a.tol, 3000, engine_opts=opts) for rho in rhos]
        ms, rs = timed(seq, a.steps, a.warmup, dev)
        emit({"row": "a", "what": "sequential rho sweep (sum of 3 solves per step)", "rhos": rhos,
              "iters": [int(r.iters) for r in rs], "engine": [r.extra.get("engine") for r in rs], **stats(ms)})
        single = {}
        for rho in rhos:  # each solve alone: the slowest is what a perfect side-by-side sweep costs
            m1, r1 = timed(lambda: chain_admm(model, ids, 24, rho, obj0, a.tol, 3000, engine_opts=opts),
                           a.steps, a.warmup, dev)
            single[rho] = stats(m1)
            emit({"row": "a1", "what": "single solve", "rho": rho, "iters": int(r1.iters), **single[rho]})
    if "b" in rows:
        def con():
            return chain_admm_sweep(model, ids, 24, rhos, obj0, a.tol, 3000, engine_opts=opts)
        ms, rs = timed(con, a.steps, a.warmup, dev)
        emit({"row": "b", "what": "concurrent rho sweep (one launch per step)", "rhos": rhos,
              "iters": [int(r.iters) for r in rs], "fallback": rs[0].extra.get("sweep_fallback"),
              "kernel": (rs[0].extra.get("sweep") or {}).get("kernel"),
              "placed": [(r.extra.get("sweep") or {}).get("placed") for r in rs],
              "own_wall_ms": [round(r.wall_s * 1e3, 4) for r in rs], **stats(ms)})
    if "c" in rows:
        base = None
        for K in (1, 2, 4, 8):
            ms, rs = timed(lambda: chain_admm_sweep(model, ids, 24, (3.0,) * K, obj0, a.tol, 3000, engine_opts=opts),
                           a.steps, a.warmup, dev)
            st = stats(ms)
            base = st["median_ms"] if K == 1 else base
            emit({"row": "c", "what": "co-running members, all at rho = 3", "K": K,
                  "iters": [int(r.iters) for r in rs], "fallback": rs[0].extra.get("sweep_fallback"),
                  "placed": [(r.extra.get("sweep") or {}).get("placed") for r in rs],
                  "ratio_to_K1": round(st["median_ms"] / base, 4), **st})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(results) + "\n")


if __name__ == "__main__":
    main()
