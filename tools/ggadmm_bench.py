"""GGADMM on the persistent graph kernel over five graphs, next to ``chain_admm``'s two chain kernels,
measured in one process on one GPU.

    python tools/ggadmm_bench.py [--steps 20] [--warmup 3] [--tols 1e-4,1e-8] [--out FILE]

E1 (N = 24, d = 50, rho = 3). Per tolerance, seven configurations run ALTERNATELY (one solve of each per
round, so drift of the box hits all of them alike): the graphs chain, ring, grid:4x6, star:0 and kbip on
``NativeGraphEngine``, and the identity chain on ``NativeChainEngine``'s per-worker persistent kernel
(``GADMM_BLOCKED=0``) and on its default blocked kernel. A timed step is one solve on a cached engine --
reset, launch, read-back, stream sync -- bracketed by device synchronisations; min / median / max over
the steps. There is no speed gate: these are first measurements of a graph solve on the device. One
JSON line per row: iterations, the times, microseconds per iteration, ``placed`` and the kernel's name;
a last line compares the chain graph on the new kernel with the per-worker chain kernel (same
iterations, traces equal or not, ratio of the medians).
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

from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.engine.chain_engine import NativeChainEngine  # noqa: E402
from gadmm_amd.engine.graph_engine import NativeGraphEngine  # noqa: E402
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.parallel.topology import Placement, parse_graph  # noqa: E402

GRAPHS = ["chain", "ring", "grid:4x6", "star:0", "kbip"]


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tols", default="1e-4,1e-8")
    ap.add_argument("--workers", type=int, default=24)
    ap.add_argument("--rho", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ggadmm_bench: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    N = a.workers
    ds = linear_synthetic(N)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    obj0 = model.optimum()
    ids = list(range(N))
    pre = (model.A, model.b, model.yy)
    lines = []
    for tol in (float(t) for t in a.tols.split(",")):
        graphs = {s: parse_graph(s if s != "grid:4x6" else "grid:4x%d" % (N // 4), N) for s in GRAPHS}
        engines = {}
        for s, g in graphs.items():
            engines["graph/" + s] = NativeGraphEngine(model.X, model.y, g, a.rho, obj0, tol, 3000, precomputed=pre)
        for cfg in ("chain-per-worker", "chain-blocked"):
            eng = NativeChainEngine(model.X, model.y, ids, N, "linear", rho=a.rho, obj0=obj0, tol=tol, max_iter=3000,
                                    precomputed=pre, residual=True)
            eng.set_path(ids, Placement.contiguous(N, 1), 0)
            engines[cfg] = eng
        torch.cuda.synchronize(dev)

        def solve(cfg):
            eng = engines[cfg]
            if cfg.startswith("graph/"):
                eng.reset()
                return eng, eng.run(fetch_trace=True)
            if cfg == "chain-per-worker":
                os.environ["GADMM_BLOCKED"] = "0"
            else:
                os.environ.pop("GADMM_BLOCKED", None)
            try:
                eng.reset()
                return eng, eng.run_persistent(fetch_trace=True)
            finally:
                os.environ.pop("GADMM_BLOCKED", None)

        cfgs = list(engines)
        ms = {c: [] for c in cfgs}
        last = {}
        for k in range(a.warmup + a.steps):
            for c in cfgs:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng, r = solve(c)
                torch.cuda.synchronize(dev)
                if k >= a.warmup:
                    ms[c].append((time.perf_counter() - t0) * 1e3)
                last[c] = (r, eng.traces(r.iters)[0].copy(), int(eng.last_placed), eng.last_kernel)
        for c in cfgs:
            r, tr, placed, kernel = last[c]
            st = stats(ms[c])
            g = graphs.get(c[6:]) if c.startswith("graph/") else graphs["chain"]
            rec = {"config": c, "N": N, "d": model.d, "rho": a.rho, "tol": tol, "edges": len(g.edges),
                   "max_degree": g.max_degree, "iters": int(r.iters), "converged": r.done == 1, "placed": placed,
                   "kernel": kernel, "final_gap": float(abs(tr[-1] - obj0)),
                   "us_per_iter_median": round(1e3 * st["median_ms"] / int(r.iters), 4),
                   "device": torch.cuda.get_device_name(0), **st}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        rg, rc = last["graph/chain"], last["chain-per-worker"]
        cmp_ = {"compare": "graph/chain vs chain-per-worker", "tol": tol, "iters": [int(rg[0].iters), int(rc[0].iters)],
                "trace_equal": bool(np.array_equal(rg[1], rc[1])),
                "median_ratio": round(float(np.median(ms["graph/chain"]) / np.median(ms["chain-per-worker"])), 4),
                "min_ratio": round(float(np.min(ms["graph/chain"]) / np.min(ms["chain-per-worker"])), 4)}
        line = json.dumps(cmp_)
        print(line, flush=True)
        lines.append(line)
        for eng in engines.values():
            eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
