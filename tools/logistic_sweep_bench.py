"""Concurrent logistic (inner-GD) sweep against the sequential one, measured on one GPU.

    python tools/logistic_sweep_bench.py [--repeats 15] [--warmup 3] [--ab-lib OTHER.so] [--out FILE]

Rows (E3: 24 workers, d = m = 50, step 2.2, lam 1e-5, to the 1e-4 gap; every timed step ends in a stream
sync; the variants of a row are timed in turn within each repeat, so drift hits them alike; min / median /
max over the repeats):

  a  E3's rho in {3e-4, 2e-4}: ``logistic_admm_sweep`` (one launch) against the two ``chain_admm`` solves
     one after the other, and each solve alone (the slowest is what a perfect side-by-side launch costs);
  b  K = 1, 2, 4, 8 members at rho = 2e-4: one launch against K solves one after the other;
  c  a sweep of ONE against ``chain_admm`` (what the sweep path itself costs);
  d  ``--ab-lib``: the single solve, and a launch of ``--ab-members`` members at rho = 2e-4, on this build
     against another build of the library (``GADMM_NATIVE_LIB``), alternately, each in a fresh child process
     (a process loads one library).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gadmm_amd.algorithms import chain_admm, logistic_admm_sweep  # noqa: E402
from gadmm_amd.data import logistic_synthetic  # noqa: E402
from gadmm_amd.models import LogisticRegression  # noqa: E402
from gadmm_amd.ops import native  # noqa: E402

N, STEP, TOL, CAP = 24, 2.2, 1e-4, 400
OPTS = {"state": False, "residual": False}


def interleaved(variants, repeats, warmup, dev):
    """``{name: [ms]}`` and each variant's last result; the variants run in turn within every repeat."""
    ms = {k: [] for k in variants}
    out = {}
    for rep in range(warmup + repeats):
        for k, fn in variants.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out[k] = fn()
            torch.cuda.synchronize(dev)
            if rep >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms, out


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "repeats": len(ms)}


def problem(dev):
    ds = logistic_synthetic(N)
    model = LogisticRegression(ds.X.to(dev).contiguous(), ds.y.to(dev).contiguous(), lam=1e-5)
    return model, model.optimum(None, n_total=N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ab-lib", default=None, help="row d: another build of the native library")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-members", type=int, default=8, help="row d: members of the timed launch (0: single solve only)")
    ap.add_argument("--single", action="store_true", help="(row d's child) time the single solve and the launch of "
                    "--ab-members members, print one JSON line")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    rows = [r for r in a.rows.split(",") if r]
    native.require()
    dev = torch.device("cuda", 0)
    model, obj0 = problem(dev)
    ids = list(range(N))
    results = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        results.append(line)

    def single(rho):
        return chain_admm(model, ids, N, rho, obj0, TOL, CAP, local_solver="gd", step=STEP, engine_opts=OPTS)

    def sweep(members):
        return logistic_admm_sweep(model, ids, N, members, obj0, TOL, CAP, step=STEP, engine_opts=OPTS)

    def sweep_fields(rs):
        return {"iters": [int(r.iters) for r in rs], "fallback": rs[0].extra.get("sweep_fallback"),
                "kernel": rs[0].extra.get("sweep_kernel"), "placed": [(r.extra.get("sweep") or {}).get("placed") for r in rs]}

    if a.single:
        variants = {"single": lambda: single(2e-4)}
        if a.ab_members > 0:  # (0: the other build has no sweep kernel)
            variants["sweep"] = lambda: sweep([2e-4] * a.ab_members)
        ms, out = interleaved(variants, a.repeats, a.warmup, dev)
        rec = {"lib": native.library_path(), "iters": int(out["single"].iters), **stats(ms["single"])}
        if a.ab_members > 0:
            rec.update(sweep_members=a.ab_members, sweep_median_ms=stats(ms["sweep"])["median_ms"],
                       sweep_kernel=out["sweep"][0].extra.get("sweep_kernel"))
        print(json.dumps(rec), flush=True)
        return
    if "a" in rows:
        rhos = [3e-4, 2e-4]
        ms, out = interleaved({"concurrent": lambda: sweep(rhos), "sequential": lambda: [single(r) for r in rhos],
                               "alone_3e-4": lambda: single(3e-4), "alone_2e-4": lambda: single(2e-4)},
                              a.repeats, a.warmup, dev)
        slowest = max(np.median(ms["alone_3e-4"]), np.median(ms["alone_2e-4"]))
        emit({"row": "a", "what": "E3 rho sweep {3e-4, 2e-4}", **sweep_fields(out["concurrent"]),
              "concurrent": stats(ms["concurrent"]), "sequential": stats(ms["sequential"]),
              "alone": {"3e-4": stats(ms["alone_3e-4"]), "2e-4": stats(ms["alone_2e-4"])},
              "sequential_over_concurrent": round(float(np.median(ms["sequential"]) / np.median(ms["concurrent"])), 4),
              "concurrent_over_slowest_alone": round(float(np.median(ms["concurrent"]) / slowest), 4)})
    if "b" in rows:
        for K in (1, 2, 4, 8):
            ms, out = interleaved({"concurrent": lambda: sweep([2e-4] * K),
                                   "sequential": lambda: [single(2e-4) for _ in range(K)],
                                   "alone": lambda: single(2e-4)}, a.repeats, a.warmup, dev)
            emit({"row": "b", "what": "K members at rho = 2e-4", "K": K, **sweep_fields(out["concurrent"]),
                  "concurrent": stats(ms["concurrent"]), "sequential": stats(ms["sequential"]), "alone": stats(ms["alone"]),
                  "sequential_over_concurrent": round(float(np.median(ms["sequential"]) / np.median(ms["concurrent"])), 4),
                  "concurrent_over_alone": round(float(np.median(ms["concurrent"]) / np.median(ms["alone"])), 4)})
    if "c" in rows:
        ms, out = interleaved({"sweep_of_one": lambda: sweep([2e-4]), "chain_admm": lambda: single(2e-4)},
                              a.repeats, a.warmup, dev)
        emit({"row": "c", "what": "a sweep of ONE against chain_admm", **sweep_fields(out["sweep_of_one"]),
              "sweep_of_one": stats(ms["sweep_of_one"]), "chain_admm": stats(ms["chain_admm"]),
              "ratio": round(float(np.median(ms["sweep_of_one"]) / np.median(ms["chain_admm"])), 4)})
    if "d" in rows and a.ab_lib:
        libs = {"this": native.library_path(), "other": os.path.abspath(a.ab_lib)}
        med = {k: [] for k in libs}
        swp = {k: [] for k in libs}
        for _ in range(a.ab_rounds):
            for k, lib in libs.items():  # alternately, a fresh child each (a failing child ends the row)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--single", "--repeats", str(a.repeats),
                                    "--warmup", str(a.warmup), "--ab-members", str(a.ab_members)], env=dict(os.environ, GADMM_NATIVE_LIB=lib),
                                   capture_output=True, text=True, timeout=240, check=True)
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                assert rec["lib"] == lib
                med[k].append(rec["median_ms"])
                swp[k].append(rec.get("sweep_median_ms", float("nan")))
                emit({"row": "d1", "lib": k, **rec})
        emit({"row": "d", "what": "single solve and a launch of %d members, this build against another (medians of "
              "each child)" % a.ab_members,
              "sweep_this_ms": swp["this"], "sweep_other_ms": swp["other"],
              "sweep_ratio_of_medians": round(float(np.median(swp["this"]) / np.median(swp["other"])), 4),
              "this_ms": med["this"], "other_ms": med["other"],
              "ratio_of_medians": round(float(np.median(med["this"]) / np.median(med["other"])), 4),
              "spread_this": round(float((max(med["this"]) - min(med["this"])) / np.median(med["this"])), 4),
              "spread_other": round(float((max(med["other"]) - min(med["other"])) / np.median(med["other"])), 4)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(results) + "\n")


if __name__ == "__main__":
    main()
