"""Q-GGADMM on the persistent graph kernel with a quantized exchange (csrc/kernels/graph_quant.hip) next to
the unquantized graph kernel, measured in one process on one GPU.

    python tools/qggadmm_bench.py [--steps 20] [--warmup 3] [--tols 1e-4,1e-8] [--bits 4,8] [--out FILE]

E1 (N = 24, d = 50, rho = 3). Per tolerance, the five graphs chain, ring, grid:4x6, star:0 and kbip
(maximum degree 2, 2, 4, 23, 12) each run unquantized and at every bit width of ``--bits`` on
``NativeGraphEngine``; the configurations run ALTERNATELY (one solve of each per round, so drift of the box
hits all of them alike). A timed step is one solve on a cached engine -- reset, launch, read-back, stream
sync -- bracketed by device synchronisations; min / median / max over the steps. There is no speed gate:
these are first measurements of a quantized solve on a graph. One JSON line per row: kernel, iterations,
the times, microseconds per iteration, payload bits and ``placed``; then one line per graph and bit width
with the ratio of the microseconds per iteration to the unquantized kernel's.
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

from gadmm_amd.algorithms.quantize import payload_bits  # noqa: E402
from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.engine.graph_engine import NativeGraphEngine  # noqa: E402
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.parallel.topology import parse_graph  # noqa: E402

GRAPHS = ["chain", "ring", "grid:4x6", "star:0", "kbip"]


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tols", default="1e-4,1e-8")
    ap.add_argument("--bits", default="4,8")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--workers", type=int, default=24)
    ap.add_argument("--rho", type=float, default=3.0)
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qggadmm_bench: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    N = a.workers
    ds = linear_synthetic(N)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    obj0 = model.optimum()
    pre = (model.A, model.b, model.yy)
    widths = [int(b) for b in a.bits.split(",") if b]
    lines = []
    for tol in (float(t) for t in a.tols.split(",")):
        graphs = {s: parse_graph(s if s != "grid:4x6" else "grid:4x%d" % (N // 4), N) for s in GRAPHS}
        engines = {}
        for s, g in graphs.items():
            for b in [0] + widths:
                engines[(s, b)] = NativeGraphEngine(model.X, model.y, g, a.rho, obj0, tol, a.max_iter, precomputed=pre,
                                                    quant=(b, a.seed) if b else None)
        torch.cuda.synchronize(dev)
        cfgs = list(engines)
        ms = {c: [] for c in cfgs}
        last = {}
        for k in range(a.warmup + a.steps):
            for c in cfgs:
                eng = engines[c]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.reset()
                r = eng.run(fetch_trace=True)
                torch.cuda.synchronize(dev)
                if k >= a.warmup:
                    ms[c].append((time.perf_counter() - t0) * 1e3)
                last[c] = (r, eng.traces(r.iters)[0].copy(), int(eng.last_placed), eng.last_kernel)
        per_iter = {}
        for c in cfgs:
            s, b = c
            r, tr, placed, kernel = last[c]
            st = stats(ms[c])
            g = graphs[s]
            per_iter[c] = 1e3 * st["median_ms"] / int(r.iters)
            rec = {"graph": s, "bits": b, "N": N, "d": model.d, "rho": a.rho, "tol": tol, "edges": len(g.edges),
                   "max_degree": g.max_degree, "kernel": kernel, "iters": int(r.iters), "converged": r.done == 1,
                   "us_per_iter_median": round(per_iter[c], 4),
                   "payload_bits": int(r.iters) * N * (payload_bits(model.d, b) if b else 64 * model.d),
                   "placed": placed, "final_gap": float(abs(tr[-1] - obj0)), "device": torch.cuda.get_device_name(0),
                   **st}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        for s in GRAPHS:
            for b in widths:
                line = json.dumps({"compare": "Q(b=%d) / unquantized" % b, "graph": s, "tol": tol,
                                   "max_degree": graphs[s].max_degree,
                                   "us_per_iter_ratio": round(per_iter[(s, b)] / per_iter[(s, 0)], 4),
                                   "iters": [last[(s, b)][0].iters, last[(s, 0)][0].iters]})
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
