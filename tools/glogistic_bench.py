"""Logistic GGADMM on the persistent graph kernel over five graphs, next to ``chain_admm(local_solver="gd")``'s
one-wave chain kernel, measured in one process on one GPU.

    python tools/glogistic_bench.py [--steps 20] [--warmup 3] [--out FILE]

E3 (N = 24, 50 x 50 shards, lam = 1e-5, gd_step = 2.2, max_inner = 100, inner_tol = 1e-4, rho = 2e-4, gap
1e-4). Six configurations run ALTERNATELY (one solve of each per round, so drift of the box hits all of them
alike): the graphs chain, ring, grid:4x6, star:0 and kbip on ``NativeGraphLogisticEngine``, and the identity
chain on ``NativeChainEngine``'s persistent logistic kernel under ``GADMM_LOGISTIC_ZREC=0`` (set here for the
whole process): one wave per worker, the same worker layout as the graph kernel. A timed step is one solve on
a cached engine -- reset, launch, read-back, stream sync -- bracketed by device synchronisations; min /
median / max over the steps. There is no speed gate. One JSON line per row: iterations, the times,
microseconds per iteration, ``placed`` and the kernel's name; a last line compares the chain graph with the
chain kernel (same iterations, traces equal or not, ratio of the medians and of the per-iteration times).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

os.environ["GADMM_LOGISTIC_ZREC"] = "0"  # the one-wave chain kernel, read by the launcher at every launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gadmm_amd.config import get_preset  # noqa: E402
from gadmm_amd.data import logistic_synthetic  # noqa: E402
from gadmm_amd.engine.chain_engine import NativeChainEngine  # noqa: E402
from gadmm_amd.engine.graph_logistic_engine import NativeGraphLogisticEngine  # noqa: E402
from gadmm_amd.models import LogisticRegression  # noqa: E402
from gadmm_amd.parallel.topology import Placement, parse_graph  # noqa: E402


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("glogistic_bench: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    cfg = get_preset("LogisticRegression_Topologies")
    N, rho, tol, mi = cfg.num_workers, cfg.rhos[0], cfg.acc, cfg.gadmm_iters
    ds = logistic_synthetic(N)
    model = LogisticRegression(ds.X.to(dev), ds.y.to(dev), cfg.lam)
    obj0 = model.optimum()
    ids = list(range(N))
    graphs = {s: parse_graph(s, N) for s in cfg.graphs}
    engines = {"graph/" + s: NativeGraphLogisticEngine(model.X, model.y, g, rho, obj0, tol, mi, cfg.lam, cfg.gd_step,
                                                       cfg.max_inner, 1e-4) for s, g in graphs.items()}
    chain = NativeChainEngine(model.X, model.y, ids, N, "logistic", rho=rho, obj0=obj0, tol=tol, max_iter=mi,
                              lam=cfg.lam, step=cfg.gd_step, max_inner=cfg.max_inner, inner_tol=1e-4,
                              local_solver="gd", residual=True)
    chain.set_path(ids, Placement.contiguous(N, 1), 0)
    engines["chain-one-wave"] = chain
    torch.cuda.synchronize(dev)

    def solve(c):
        eng = engines[c]
        eng.reset()
        return eng.run(fetch_trace=True) if c.startswith("graph/") else eng.run_persistent(fetch_trace=True)

    ms = {c: [] for c in engines}
    last = {}
    for k in range(a.warmup + a.steps):
        for c, eng in engines.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = solve(c)
            torch.cuda.synchronize(dev)
            if k >= a.warmup:
                ms[c].append((time.perf_counter() - t0) * 1e3)
            last[c] = (r, eng.traces(r.iters)[0].copy(), int(eng.last_placed), eng.last_kernel)
    lines = []
    for c in engines:
        r, tr, placed, kernel = last[c]
        st = stats(ms[c])
        g = graphs[c[6:]] if c.startswith("graph/") else graphs["chain"]
        lines.append(json.dumps({
            "config": c, "N": N, "m": model.m, "d": model.d, "rho": rho, "tol": tol, "edges": len(g.edges),
            "max_degree": g.max_degree, "iters": int(r.iters), "converged": r.done == 1, "placed": placed,
            "kernel": kernel, "final_gap": float(abs(tr[-1] - obj0)),
            "us_per_iter_median": round(1e3 * st["median_ms"] / int(r.iters), 4),
            "device": torch.cuda.get_device_name(0), **st}))
    rg, rc = last["graph/chain"], last["chain-one-wave"]
    mg, mc = float(np.median(ms["graph/chain"])), float(np.median(ms["chain-one-wave"]))
    lines.append(json.dumps({
        "compare": "graph/chain vs chain-one-wave", "iters": [int(rg[0].iters), int(rc[0].iters)],
        "trace_equal": bool(np.array_equal(rg[1], rc[1])),
        "trace_max_rel_diff": (float(np.max(np.abs(rg[1] - rc[1]) / np.abs(rc[1])))
                               if len(rg[1]) == len(rc[1]) else None),
        "median_ratio": round(mg / mc, 4),
        "us_per_iter": [round(1e3 * mg / int(rg[0].iters), 4), round(1e3 * mc / int(rc[0].iters), 4)]}))
    print("\n".join(lines), flush=True)
    for eng in engines.values():
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
