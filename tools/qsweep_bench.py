"""Concurrent Q-GADMM solves (one launch, one solve per XCD) against the sequential loop, measured in
one process on one GPU.

    python tools/qsweep_bench.py [--steps 20] [--warmup 3] [--tol 1e-8] [--out FILE]

E1 shards (N = 24, d = 50) to ``--tol``, every engine cached (Gram and inverses are set up once, outside
the timing). Configurations, run ALTERNATELY (one of each per round, so drift of the box hits all of
them alike); a timed step ends in a device sync; min / median / max over the steps:

  seq6          the loop of ``chain_admm(quantize=(b, 1234))`` over bits {4, 8} x rho {3, 5, 7}: six
                launches of the persistent Q kernel, one after the other (what an entry runs today);
                ``members`` holds each solve's own statistics, ``slowest_member`` the largest median;
  con6          ``quantized_group_admm_sweep`` of the same six: one launch, K = 6;
  k1 k2 k4 k8   ``quantized_group_admm_sweep`` of K members (rho 3, b = 8, seed k), k = 1..K;
  single        ``chain_admm(quantize=(8, 1))`` at rho 3: the single solve that k1 is a sweep of one of.

Each line also carries the iterations of its members and, for the sweeps, the kernel and placements.
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

from gadmm_amd.algorithms import chain_admm, quantized_group_admm_sweep  # noqa: E402
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
    obj0 = model.optimum()
    ids = list(range(N))
    six = [(rho, bits, 1234) for bits in (4, 8) for rho in (3.0, 5.0, 7.0)]
    same = {K: [(3.0, 8, k) for k in range(1, K + 1)] for K in (1, 2, 4, 8)}
    member_ms = [[] for _ in six]

    def single(cfg):
        rho, bits, seed = cfg
        return chain_admm(model, ids, N, rho, obj0, a.tol, 3000, quantize=(bits, seed), name="Q-GADMM")

    def run(c, timed):
        if c == "seq6":
            out = []
            for j, cfg in enumerate(six):
                t0 = time.perf_counter()
                out.append(single(cfg))
                torch.cuda.synchronize(dev)
                if timed:
                    member_ms[j].append((time.perf_counter() - t0) * 1e3)
            return out
        if c == "con6":
            return quantized_group_admm_sweep(model, six, obj0, a.tol, 3000)
        if c == "single":
            return [single(same[1][0])]
        return quantized_group_admm_sweep(model, same[int(c[1:])], obj0, a.tol, 3000)

    cfgs = ["seq6", "con6", "k1", "k2", "k4", "k8", "single"]
    ms = {c: [] for c in cfgs}
    last = {}
    for k in range(a.warmup + a.steps):
        for c in cfgs:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rs = run(c, k >= a.warmup)
            torch.cuda.synchronize(dev)
            if k >= a.warmup:
                ms[c].append((time.perf_counter() - t0) * 1e3)
            last[c] = rs
    lines = []
    for c in cfgs:
        rs = last[c]
        rec = {"config": c, "N": N, "d": model.d, "tol": a.tol, "K": len(rs), "iters": [int(r.iters) for r in rs],
               "converged": all(bool(r.converged) for r in rs),
               "kernel": rs[0].extra.get("sweep_kernel", rs[0].extra.get("kernel")),
               "placed": [int(r.extra.get("placed", -1)) for r in rs],
               "fallback": rs[0].extra.get("sweep_fallback"),
               "device": torch.cuda.get_device_name(0), **stats(ms[c])}
        if c == "seq6":
            rec["members"] = [dict(rho=cfg[0], bits=cfg[1], **stats(m)) for cfg, m in zip(six, member_ms)]
            rec["slowest_member"] = max(rec["members"], key=lambda m: m["median_ms"])
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
