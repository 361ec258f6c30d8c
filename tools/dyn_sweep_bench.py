"""Concurrent D-GADMM coherence sweep against the sequential loop, measured in one process on one GPU.

    python tools/dyn_sweep_bench.py [--sets e7,e5] [--rows a,b] [--steps 20] [--warmup 3] [--out FILE]

Sets: ``e7`` = N 24, rho 1, coherences {1, 10, 50} (LinearRegression_gadmm_vs_admm); ``e5`` = N 50,
rho 3, coherences {1e9, 1, 10, 50, 100} (Dynamic_LinearRegression_Synthetic, part 2). Every timed
step includes the set-up from the raw shards (Gram + inverses + padded image) like bench.py's
headline, and ends in a stream sync; min / median / max over the steps.

  a   sequential: ``dynamic_group_admm(refresh=True)`` per coherence, the sum per step, with the
      single solve's own kernel choice (coherence 1 and 2: the per-worker kernel);
  a1  each member alone: the slowest is what a perfect side-by-side sweep costs;
  b   concurrent: ``dynamic_group_admm_sweep(refresh=True)`` of the same members; with the host share
      from ``utils/timing.host_stamp``: ``host_ahead_ms`` = host time serially ahead of the launches
      (chain draws, epoch staging, argument set-up of every member and round), ``host_after_ms`` =
      decoding and result assembly after the last read-back.
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

from gadmm_amd.algorithms import dynamic_group_admm, dynamic_group_admm_sweep  # noqa: E402
from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.ops import native  # noqa: E402
from gadmm_amd.parallel import topology as T  # noqa: E402
from gadmm_amd.utils import timing  # noqa: E402

SETS = {
    "e7": dict(n=24, rho=1.0, cohs=(1, 10, 50), max_iter=20000, seed=lambda c: 1234 + int(c), path="findPath2"),
    "e5": dict(n=50, rho=3.0, cohs=(1e9, 1, 10, 50, 100), max_iter=5000, seed=lambda c: 1234 + int(min(c, 1e6)),
               path="findPath"),
}


def timed(step, steps, warmup, dev, each=None):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    ms, out = [], None
    for _ in range(steps):
        if each is not None:
            each(None)
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
        if each is not None:
            each(out)
    return ms, out


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def host_share(stamps):
    """(ahead, after) ms of one sweep call's stamps: host time before each round's launch returned plus
    the set-up before the first round; host time after the last round's sync."""
    t = {}
    ahead, last_sync, begin, end = 0.0, None, None, None
    for label, v in stamps:
        if label == "dsw:begin":
            begin = v
        elif label == "dsw:round":
            t["round"] = v
            if begin is not None:
                ahead += v - begin
                begin = None
        elif label == "dsw:launched":
            ahead += v - t["round"]
        elif label == "dsw:synced":
            last_sync = v
        elif label == "dsw:end":
            end = v
    after = (end - last_sync) if (end is not None and last_sync is not None) else 0.0
    return ahead * 1e3, after * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="e7,e5")
    ap.add_argument("--rows", default="a,b")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    rows = [r for r in a.rows.split(",") if r]
    native.require()
    dev = torch.device("cuda", 0)
    opts = {"refresh": True, "state": False, "residual": False}
    results = []

    def emit(rec):
        rec["native_lib"] = native.library_path()
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        results.append(line)

    for name in [s for s in a.sets.split(",") if s]:
        cfg = SETS[name]
        n, rho, cohs, mi = cfg["n"], cfg["rho"], cfg["cohs"], cfg["max_iter"]
        seeds = [cfg["seed"](c) for c in cohs]
        ds = linear_synthetic(n)
        model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
        obj0 = model.optimum()
        rng = np.random.default_rng(1234)
        path, cost = (T.find_path2(n, rng) if cfg["path"] == "findPath2" else T.find_path(n, rng))[:2]

        def one(c, s):
            return dynamic_group_admm(model, rho, obj0, a.tol, mi, path, cost, c, seed=s, engine_opts=opts)

        seq_med = slow = None
        if "a" in rows:
            ms, rs = timed(lambda: [one(c, s) for c, s in zip(cohs, seeds)], a.steps, a.warmup, dev)
            st = stats(ms)
            seq_med = st["median_ms"]
            emit({"set": name, "row": "a", "what": "sequential coherence loop (sum of %d solves per step)" % len(cohs),
                  "coherences": cohs, "iters": [int(r.iters) for r in rs],
                  "engine": [r.extra.get("engine") for r in rs], **st})
            slow = 0.0
            for c, s in zip(cohs, seeds):
                m1, r1 = timed(lambda: one(c, s), a.steps, a.warmup, dev)
                s1 = stats(m1)
                slow = max(slow, s1["median_ms"])
                emit({"set": name, "row": "a1", "what": "single solve", "coherence": c, "iters": int(r1.iters),
                      "kernel": getattr(r1.extra.get("engine_obj"), "last_kernel", None), **s1})
        if "b" in rows:
            shares = []

            def each(out):
                if out is None:
                    timing.HOST_STAMPS = []
                else:
                    shares.append(host_share(timing.HOST_STAMPS))
                    timing.HOST_STAMPS = None

            ms, rs = timed(lambda: dynamic_group_admm_sweep(model, rho, obj0, a.tol, mi, path, cost, cohs, seeds,
                                                            engine_opts=opts), a.steps, a.warmup, dev, each=each)
            st = stats(ms)
            rec = {"set": name, "row": "b", "what": "concurrent coherence sweep", "coherences": cohs,
                   "iters": [int(r.iters) for r in rs], "fallback": rs[0].extra.get("sweep_fallback"),
                   "kernel": (rs[0].extra.get("sweep") or {}).get("kernel"),
                   "placed": [(r.extra.get("sweep") or {}).get("placed") for r in rs],
                   "launches": [(r.extra.get("sweep") or {}).get("launches") for r in rs],
                   "own_wall_ms": [round(r.wall_s * 1e3, 4) for r in rs],
                   "host_ahead_ms": round(float(np.median([s[0] for s in shares])), 4),
                   "host_after_ms": round(float(np.median([s[1] for s in shares])), 4), **st}
            if seq_med:
                rec["vs_sequential_sum"] = round(st["median_ms"] / seq_med, 4)
                rec["vs_slowest_member_alone"] = round(st["median_ms"] / slow, 4)
            emit(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(results) + "\n")


if __name__ == "__main__":
    main()
