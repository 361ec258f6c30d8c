"""Concurrent logistic GGADMM solves (one launch, one solve per XCD) against the sequential loop, measured in
one process on one GPU.

    python tools/glogistic_sweep_bench.py [--steps 10] [--warmup 2] [--out FILE]
    python tools/glogistic_sweep_bench.py --singles-only           # chain and ring alone (what --ab runs)
    python tools/glogistic_sweep_bench.py --ab OTHER_LIB [--ab-rounds 3] [--out FILE]

E3 (N = 24, 50 x 50 shards, lam = 1e-5, gd_step = 2.2, max_inner = 100, inner_tol = 1e-4, rho = 2e-4, gap 1e-4),
every engine cached (set up once, outside the timing). Configurations, run ALTERNATELY (one of each per round,
so drift of the box hits all of them alike); a timed step ends in a device sync; min / median / max over the
steps:

  seq5          the loop of ``graph_admm_logistic`` over chain, ring, 4 x 6 grid, star and complete bipartite:
                five launches of the persistent logistic graph kernel, one after the other (what the topology
                entry runs); ``members`` holds each solve's own statistics, ``slowest_member`` the largest median;
  con5          ``graph_admm_logistic_sweep`` of the same five: one launch, K = 5;
  k1 k2 k4 k8   ``graph_admm_logistic_sweep`` of K ring members;
  ring          ``graph_admm_logistic`` on the ring: the single solve that k1 is a sweep of one of.

Each line also carries the iterations of its members and, for the sweeps, the kernel and placements.

``--ab OTHER_LIB``: the single solves on the chain and on the ring on this build and on another build of the
native library, in fresh child processes run alternately (this, other, this, ...; ``GADMM_NATIVE_LIB`` names the
library a child loads), ``--ab-rounds`` of each. A child that fails ends the run. One line per child, then a
summary: per graph the medians of every round of either build.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def emit(lines, out):
    for line in lines:
        print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def ab(a):
    """The chain and ring single solves on this build and on ``a.ab``, alternately, each in a fresh child process."""
    rounds = {"this": [], "other": []}
    lines = []
    for k in range(a.ab_rounds):
        for which in ("this", "other"):
            env = dict(os.environ)
            env.pop("GADMM_NATIVE_LIB", None)
            if which == "other":
                env["GADMM_NATIVE_LIB"] = os.path.abspath(a.ab)
            cmd = [sys.executable, os.path.abspath(__file__), "--singles-only", "--steps", str(a.steps), "--warmup",
                   str(a.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit("child (%s build, round %d) failed with %d:\n%s" % (which, k, p.returncode,
                                                                                   p.stdout[-2000:] + p.stderr[-2000:]))
            recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
            rounds[which].append({r["config"]: r for r in recs})
            lines += [json.dumps(dict(r, build=which, round=k)) for r in recs]
    summary = {"config": "ab-summary", "other": os.path.abspath(a.ab), "rounds": a.ab_rounds}
    for cfg in ("chain", "ring"):
        summary[cfg] = {w: [r[cfg]["median_ms"] for r in rounds[w]] for w in rounds}
    emit(lines + [json.dumps(summary)], a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--singles-only", action="store_true", help="the chain and ring single solves only (no sweep)")
    ap.add_argument("--ab", default=None, help="another build of the native library to alternate with")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    if a.ab:
        return ab(a)

    import torch
    from gadmm_amd.algorithms import graph_admm_logistic
    from gadmm_amd.config import get_preset
    from gadmm_amd.data import logistic_synthetic
    from gadmm_amd.models import LogisticRegression
    from gadmm_amd.ops import native
    from gadmm_amd.parallel.topology import parse_graph

    if not torch.cuda.is_available():
        raise SystemExit("glogistic_sweep_bench: needs a HIP device (a CPU run measures nothing)")
    native.require()
    dev = torch.device("cuda", 0)
    cfg = get_preset("LogisticRegression_Topologies")
    N, rho, tol, cap = cfg.num_workers, cfg.rhos[0], cfg.acc, cfg.gadmm_iters
    ds = logistic_synthetic(N)
    model = LogisticRegression(ds.X.to(dev), ds.y.to(dev), cfg.lam)
    obj0 = model.optimum()
    specs = list(cfg.graphs)
    graphs = [parse_graph(s, N) for s in specs]
    chain, ring = graphs[specs.index("chain")], graphs[specs.index("ring")]
    member_ms = [[] for _ in graphs]

    def single(g):
        return graph_admm_logistic(model, g, rho, obj0, tol, cap, cfg.gd_step, max_inner=cfg.max_inner, backend="native")

    def sweep(members):
        from gadmm_amd.algorithms import graph_admm_logistic_sweep
        return graph_admm_logistic_sweep(model, members, obj0, tol, cap, cfg.gd_step, max_inner=cfg.max_inner)

    def run(c, timed):
        if c == "seq5":
            out = []
            for j, g in enumerate(graphs):
                t0 = time.perf_counter()
                out.append(single(g))
                torch.cuda.synchronize(dev)
                if timed:
                    member_ms[j].append((time.perf_counter() - t0) * 1e3)
            return out
        if c == "con5":
            return sweep([(g, rho) for g in graphs])
        if c in ("chain", "ring"):
            return [single(chain if c == "chain" else ring)]
        return sweep([(ring, rho)] * int(c[1:]))

    cfgs = ["chain", "ring"] if a.singles_only else ["seq5", "con5", "k1", "k2", "k4", "k8", "ring"]
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
        rec = {"config": c, "N": N, "m": model.m, "d": model.d, "rho": rho, "tol": tol, "K": len(rs),
               "iters": [int(r.iters) for r in rs], "converged": all(bool(r.converged) for r in rs),
               "kernel": rs[0].extra.get("sweep_kernel", rs[0].extra.get("kernel")),
               "placed": [int(r.extra.get("placed", -1)) for r in rs],
               "fallback": rs[0].extra.get("sweep_fallback"), "library": native.library_path(),
               "device": torch.cuda.get_device_name(0), **stats(ms[c])}
        if c == "seq5":
            rec["members"] = [dict(graph=s, **stats(m)) for s, m in zip(specs, member_ms)]
            rec["slowest_member"] = max(rec["members"], key=lambda m: m["median_ms"])
        lines.append(json.dumps(rec))
    emit(lines, a.out)


if __name__ == "__main__":
    main()
