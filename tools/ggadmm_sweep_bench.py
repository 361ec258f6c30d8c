"""Concurrent GGADMM / Q-GGADMM solves (one launch, one solve per XCD) against the sequential loop, measured
in one process on one GPU.

    python tools/ggadmm_sweep_bench.py [--steps 20] [--warmup 3] [--tol 1e-4] [--out FILE]
    python tools/ggadmm_sweep_bench.py --singles-only            # the single solves alone (what --ab runs)
    python tools/ggadmm_sweep_bench.py --ab OTHER_LIB [--ab-rounds 3] [--ab-other-first] [--out FILE]

E1 shards (N = 24, d = 50), rho = 3, to ``--tol``, every engine cached (Gram and inverses are set up once,
outside the timing). Configurations, run ALTERNATELY (one of each per round, so drift of the box hits all
of them alike); a timed step ends in a device sync; min / median / max over the steps:

  seq5          the loop of ``graph_admm`` over chain, ring, 4 x 6 grid, star and complete bipartite: five
                launches of the persistent graph kernel, one after the other (what the topology entry runs);
                ``members`` holds each solve's own statistics, ``slowest_member`` the largest median;
  con5          ``graph_admm_sweep`` of the same five: one launch, K = 5;
  chain         ``graph_admm`` on the chain alone: the member that decides the batch's time;
  k1 k2 k4 k8   ``graph_admm_sweep`` of K ring members;
  ring          ``graph_admm`` on the ring: the single solve that k1 is a sweep of one of;
  qseq5 qcon5 qchain   the same as seq5 / con5 / chain for Q-GGADMM, b = 8, seed 1234.

Each line also carries the iterations of its members and, for the sweeps, the kernel and placements.

``--ab OTHER_LIB``: the single solves (``seq5`` and ``qseq5`` with their members) on this build and on
another build of the native library, in fresh child processes run alternately (this, other, this, ...;
``GADMM_NATIVE_LIB`` names the library a child loads), ``--ab-rounds`` of each. A child that fails ends
the run. One line per child, then a summary: per member the medians of every round of either build.
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

GRAPHS = ("chain", "ring", "grid:4x6", "star:0", "kbip")


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
    """The single solves on this build and on ``a.ab``, alternately, each in a fresh child process."""
    rounds = {"this": [], "other": []}
    lines = []
    for k in range(a.ab_rounds):
        for which in (("other", "this") if a.ab_other_first else ("this", "other")):
            env = dict(os.environ)
            env.pop("GADMM_NATIVE_LIB", None)
            if which == "other":
                env["GADMM_NATIVE_LIB"] = os.path.abspath(a.ab)
            cmd = [sys.executable, os.path.abspath(__file__), "--singles-only", "--steps", str(a.steps), "--warmup",
                   str(a.warmup), "--tol", repr(a.tol), "--workers", str(a.workers)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("child (%s build, round %d) failed with %d:\n%s" % (which, k, p.returncode,
                                                                                   p.stdout[-2000:] + p.stderr[-2000:]))
            recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
            rounds[which].append({r["config"]: r for r in recs})
            lines += [json.dumps(dict(r, build=which, round=k)) for r in recs]
    summary = {"config": "ab-summary", "other": os.path.abspath(a.ab), "rounds": a.ab_rounds}
    for cfg in ("seq5", "qseq5"):
        for j, spec in enumerate(GRAPHS):
            summary["%s/%s" % (cfg, spec)] = {w: [r[cfg]["members"][j]["median_ms"] for r in rounds[w]] for w in rounds}
        summary[cfg] = {w: [r[cfg]["median_ms"] for r in rounds[w]] for w in rounds}
    emit(lines + [json.dumps(summary)], a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--workers", type=int, default=24)
    ap.add_argument("--singles-only", action="store_true", help="seq5 and qseq5 only (no sweep is built)")
    ap.add_argument("--ab", default=None, help="another build of the native library to alternate with")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-other-first", action="store_true", help="each round runs the other build first")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    if a.ab:
        return ab(a)

    import torch
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.ops import native
    from gadmm_amd.parallel.topology import parse_graph

    native.require()
    dev = torch.device("cuda", 0)
    N, rho, quant = a.workers, 3.0, (8, 1234)
    ds = linear_synthetic(N)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    obj0 = model.optimum()
    graphs = [parse_graph(s, N) for s in GRAPHS]
    ring = graphs[1]
    member_ms = {"seq5": [[] for _ in graphs], "qseq5": [[] for _ in graphs]}

    def single(g, q=None):
        return graph_admm(model, g, rho, obj0, a.tol, 3000, backend="native", quantize=q)

    def sweep(members):
        from gadmm_amd.algorithms import graph_admm_sweep
        return graph_admm_sweep(model, members, obj0, a.tol, 3000)

    def run(c, timed):
        if c in ("seq5", "qseq5"):
            out = []
            for j, g in enumerate(graphs):
                t0 = time.perf_counter()
                out.append(single(g, quant if c == "qseq5" else None))
                torch.cuda.synchronize(dev)
                if timed:
                    member_ms[c][j].append((time.perf_counter() - t0) * 1e3)
            return out
        if c == "con5":
            return sweep([(g, rho) for g in graphs])
        if c == "qcon5":
            return sweep([(g, rho) + quant for g in graphs])
        if c == "chain":
            return [single(graphs[0])]
        if c == "qchain":
            return [single(graphs[0], quant)]
        if c == "ring":
            return [single(ring)]
        return sweep([(ring, rho)] * int(c[1:]))

    cfgs = ["seq5", "qseq5"] if a.singles_only else ["seq5", "con5", "chain", "k1", "k2", "k4", "k8", "ring", "qseq5",
                                                     "qcon5", "qchain"]
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
               "fallback": rs[0].extra.get("sweep_fallback"), "library": native.library_path(),
               "device": torch.cuda.get_device_name(0), **stats(ms[c])}
        if c in member_ms:
            rec["members"] = [dict(graph=s, **stats(m)) for s, m in zip(GRAPHS, member_ms[c])]
            rec["slowest_member"] = max(rec["members"], key=lambda m: m["median_ms"])
        lines.append(json.dumps(rec))
    emit(lines, a.out)


if __name__ == "__main__":
    main()
