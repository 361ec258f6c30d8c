"""CQ-GADMM's censored hand-off next to Q-GADMM's, and the Q kernel next to the parent build's, measured
in one process on one GPU.

    python tools/cqgadmm_bench.py --parent-lib PATH/libgadmm_native.so [--steps 20] [--warmup 3]
                                  [--tol 1e-8] [--censor 1,0.98] [--out FILE]

E1 (N = 24, d = 50, rho = 3, b = 8, seed 1234) to ``--tol``. Three configurations, run ALTERNATELY (one
solve of each per round, so drift of the box hits all of them alike); a timed step is one solve on a
cached engine -- reset, launch, read-back, stream sync -- through the SAME host code for all three, only
the launch entry differs; min / median / max over the steps:

  q8          the persistent Q kernel of this build;
  q8-parent   the persistent Q kernel of the library given by ``--parent-lib`` (a build of the parent
              commit), loaded next to this build's with its own symbols bound first. Its PersistArgs has
              no censor fields, so the arguments are copied field by name into that layout;
  cq8         the persistent CQ kernel of this build under ``--censor``.

The gate is q8 against q8-parent: this build must leave the Q solve within the run-to-run noise of the
parent's, i.e. the median of q8 no higher than the slowest of the parent's own steps in the same call, and the two
objective traces equal (``q_vs_parent_median``, ``gate_ok``); the tool exits 1 otherwise. cq8 is reported next to them with its
time per iteration: what it adds per iteration is the censoring sum (one more 64-lane reduction on the
path from the solve to the publication) and the header test in the receivers' wait; what it saves is
the transmissions.
"""
import argparse
import ctypes
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
from gadmm_amd.models import LinearRegression  # noqa: E402
from gadmm_amd.ops import native  # noqa: E402
from gadmm_amd.parallel.topology import Placement  # noqa: E402

_CENSOR_FIELDS = ("c_thr2", "c_sent")


class ParentPersistArgs(ctypes.Structure):
    """PersistArgs as the parent commit has it: this build's without the censor fields."""
    _fields_ = [f for f in native.PersistArgs._fields_ if f[0] not in _CENSOR_FIELDS]


def to_parent(pa: native.PersistArgs) -> ParentPersistArgs:
    out = ParentPersistArgs()
    for name, _ in ParentPersistArgs._fields_:
        setattr(out, name, getattr(pa, name))
    return out


def stats(ms):
    return {"min_ms": round(float(np.min(ms)), 4), "median_ms": round(float(np.median(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libgadmm_native.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--workers", type=int, default=24)
    ap.add_argument("--censor", default="1,0.98")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file too")
    a = ap.parse_args()
    lib = native.require()
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    buf = (ctypes.c_longlong * 16)()
    k = parent.gadmm_quant_abi_layout(buf, 16)
    if buf[k - 1] != ctypes.sizeof(ParentPersistArgs) or buf[5] != ParentPersistArgs.qg.offset:
        raise SystemExit("--parent-lib: its PersistArgs is not this build's without the censor fields")
    parent.gadmm_chain_persistent_q_launch.restype = ctypes.c_int
    parent.gadmm_chain_persistent_q_launch.argtypes = [ctypes.POINTER(ParentPersistArgs), ctypes.c_void_p]
    censor = tuple(float(x) for x in a.censor.split(","))
    dev = torch.device("cuda", 0)
    N = a.workers
    ds = linear_synthetic(N)
    model = LinearRegression(ds.X.to(dev), ds.y.to(dev))
    d = model.d
    obj0 = model.optimum()
    ids = list(range(N))

    def engine(cen):
        eng = NativeChainEngine(model.X, model.y, ids, N, "linear", rho=3.0, obj0=obj0, tol=a.tol, max_iter=3000,
                                precomputed=(model.A, model.b, model.yy), quant=(8, 1234), censor=cen)
        eng.set_path(ids, Placement.contiguous(N, 1), 0)
        return eng

    eng_q, eng_c = engine(None), engine(censor)
    torch.cuda.synchronize(dev)

    def solve(cfg):
        eng = eng_c if cfg == "cq8" else eng_q
        eng.reset()
        pa = eng.prepare_persistent_q()
        if cfg == "q8":
            rc = lib.gadmm_chain_persistent_q_launch(ctypes.byref(pa), eng.stream.cuda_stream)
        elif cfg == "q8-parent":
            ppa = to_parent(pa)
            rc = parent.gadmm_chain_persistent_q_launch(ctypes.byref(ppa), eng.stream.cuda_stream)
        else:
            rc = lib.gadmm_chain_persistent_cq_launch(ctypes.byref(pa), eng.stream.cuda_stream)
        if rc != 0:
            raise SystemExit("%s: launch refused (rc=%d)" % (cfg, rc))
        fetch = eng._queue_readback(True)
        eng.stream.synchronize()
        return eng, eng.finish_persistent_q(0.0, fetch, cfg)

    cfgs = ["q8", "q8-parent", "cq8"]
    ms = {c: [] for c in cfgs}
    last = {}
    for k in range(a.warmup + a.steps):
        for c in cfgs:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng, r = solve(c)
            if k >= a.warmup:
                ms[c].append((time.perf_counter() - t0) * 1e3)
            if r.done == 4:
                raise SystemExit("%s: hand-off timeout" % c)
            tr = eng.objective_trace(r.iters)
            last[c] = (r, tr.copy(), int(eng.last_placed), eng.sent_trace(r.iters) if c == "cq8" else None)
    lines = []
    q_same = bool(np.array_equal(last["q8"][1], last["q8-parent"][1]))
    for c in cfgs:
        r, tr, placed, sent = last[c]
        st = stats(ms[c])
        tx = int(sent.sum()) if sent is not None else int(r.iters) * N
        rec = {"config": c, "N": N, "d": d, "tol": a.tol, "iters": int(r.iters), "converged": r.done == 1,
               "placed": placed, "transmissions": tx, "transmission_share": round(tx / (int(r.iters) * N), 4),
               "final_gap": float(abs(tr[-1] - obj0)), "us_per_iter_median": round(1e3 * st["median_ms"] / int(r.iters), 4),
               "device": torch.cuda.get_device_name(0), **st}
        if c == "cq8":
            rec["censor"] = list(censor)
        if c == "q8-parent":
            rec["trace_equals_q8"] = q_same
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    gate = {"gate": "q8 vs q8-parent", "q_vs_parent_median": round(float(np.median(ms["q8"]) / np.median(ms["q8-parent"])), 4),
            "q_vs_parent_min": round(float(np.min(ms["q8"]) / np.min(ms["q8-parent"])), 4),
            "parent_spread_max_over_min": round(float(np.max(ms["q8-parent"]) / np.min(ms["q8-parent"])), 4),
            "trace_equal": q_same}
    gate["gate_ok"] = bool(q_same and np.median(ms["q8"]) <= np.max(ms["q8-parent"]))
    line = json.dumps(gate)
    print(line, flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not gate["gate_ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
