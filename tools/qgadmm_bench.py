"""Q-GADMM's packed hand-off against the full-precision one, measured in one process on one GPU.

    python tools/qgadmm_bench.py [--steps 20] [--warmup 3] [--tol 1e-8] [--out FILE]

E1 (N = 24, d = 50, rho = 3) to ``--tol``. Configurations, run ALTERNATELY (one solve of each per
round, so drift of the box hits all of them alike); a timed step is one solve on a cached engine
(Gram and inverses are set up once, outside the timing, for every configuration) and ends in a stream
sync; min / median / max over the steps:

  q4, q8, q16   ``chain_admm(quantize=(b, 1234))``: the persistent Q kernel, G = ceil(50 b / 64) + 1
                granules per message;
  per-worker    unquantized GADMM on the per-worker persistent kernel (``GADMM_BLOCKED=0``), 50
                granules per message: the same schedule and hand-off discipline as the Q kernel;
  blocked       unquantized GADMM on the default (temporally blocked) kernel.

Each line also carries the iterations, the payload bits and the wire bytes (16-byte granules).
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

from gadmm_amd.algorithms import chain_admm  # noqa: E402
from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.ops import native  # noqa: E402


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--workers", type=int, default=24)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    native.require()
    dev = torch.device("cuda", 0)
    N = a.workers
    ds = linear_synthetic(N)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    d = model.d
    obj0 = model.optimum()
    ids = list(range(N))
    plain = {"state": False, "residual": False}

    def solve(cfg):
        if cfg.startswith("q"):
            return chain_admm(model, ids, N, 3.0, obj0, a.tol, 3000, quantize=(int(cfg[1:]), 1234), name="Q-GADMM")
        os.environ["GADMM_BLOCKED"] = "0" if cfg == "per-worker" else "1"
        try:
            return chain_admm(model, ids, N, 3.0, obj0, a.tol, 3000, engine_opts=plain)
        finally:
            os.environ.pop("GADMM_BLOCKED", None)

    cfgs = ["q4", "q8", "q16", "per-worker", "blocked"]
    ms = {c: [] for c in cfgs}
    last = {}
    for k in range(a.warmup + a.steps):
        for c in cfgs:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = solve(c)
            torch.cuda.synchronize(dev)
            if k >= a.warmup:
                ms[c].append((time.perf_counter() - t0) * 1e3)
            eng = r.extra.get("engine_obj")  # the engine is shared by the unquantized rows: read it now
            last[c] = (r, getattr(eng, "last_kernel", None), int(getattr(eng, "last_placed", -1)))
    lines = []
    for c in cfgs:
        r, kernel, placed = last[c]
        ex = r.extra
        q = c.startswith("q")
        rec = {"config": c, "N": N, "d": d, "tol": a.tol, "iters": int(r.iters), "converged": bool(r.converged),
               "engine": ex.get("engine"), "kernel": kernel, "placed": placed,
               "payload_bits": int(ex["payload_bits"]) if q else int(r.iters) * N * 64 * d,
               "granules_per_message": int(ex["q_granules"]) if q else d,
               "wire_bytes": int(ex["q_wire_bytes"]) if q else int(r.iters) * N * d * 16,
               "comm_units": float(r.comm_units[-1]), "final_gap": float(r.loss[-1]),
               "device": torch.cuda.get_device_name(0), **stats(ms[c])}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
