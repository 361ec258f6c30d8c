"""NumPy prototype of CQ-GADMM, independent of the censoring code of the package: the source of the known
answers in tests/golden/cqgadmm_prototype.json.

    python tools/cqgadmm_prototype.py [--out tests/golden/cqgadmm_prototype.json]

It takes from the package only what Q-GADMM's own tests already hold to known answers -- the data set,
the counter-based uniforms and the quantizer (``quantize.u01`` / ``quantize_rows``) -- and does the rest
itself in plain Python floats: the thresholds by repeated product, ``s`` by its own 64-lane butterfly,
the decision, the chain schedule (heads, then tails, then the duals, all on public models) and the
objective of the true iterates. Every run is made twice, with the local solves by ``numpy.linalg.solve``
and by a product with the explicit inverse: the two roundings agree on every censoring decision of the
first 80 iterations (recorded: cumulative transmissions after 20 / 40 / 60 / 80 iterations, and the number
of iterations in which every worker / no worker sends) and part later, so their counts at the stop differ
(recorded per variant, to show the spread; tests pin none of them).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gadmm_amd.algorithms import quantize as Q  # noqa: E402  (u01, quantize_rows only)
from gadmm_amd.data import linear_synthetic  # noqa: E402
from gadmm_amd.oracle.reference import opt_linear  # noqa: E402


def butterfly_sum(v):
    v = [float(x) for x in v]
    nc = (len(v) + 63) // 64
    v = v + [0.0] * (nc * 64 - len(v))
    tot = 0.0
    for c in range(nc):
        x = v[c * 64:(c + 1) * 64]
        for off in (32, 16, 8, 4, 2, 1):
            x = [x[i] + x[i ^ off] for i in range(64)]
        tot = tot + x[0]
    return tot


def run(N, censor, tol, solve, max_iter, bits=8, seed=1234, rho=3.0):
    ds = linear_synthetic(N)
    Xf, yf = ds.stacked()
    X, y = ds.X.numpy(), ds.y.numpy()
    d = X.shape[2]
    obj0 = opt_linear(Xf.numpy(), yf.numpy())
    A = np.einsum("nmi,nmj->nij", X, X)
    b = np.einsum("nmi,nm->ni", X, y)
    deg = [(w > 0) + (w < N - 1) for w in range(N)]
    Mi = [np.linalg.inv(A[w] + deg[w] * rho * np.eye(d)) for w in range(N)] if solve == "inverse" else None
    thr = [float(censor[0])]
    for _ in range(max_iter):
        thr.append(thr[-1] * float(censor[1]))
    hat, th, mu = np.zeros((N, d)), np.zeros((N, d)), np.zeros((N, d))
    sent = []
    for it in range(1, max_iter + 1):
        row = np.zeros(N, bool)
        for ws in (list(range(0, N, 2)), list(range(1, N, 2))):
            for w in ws:
                r = b[w] - mu[w]
                if w > 0:
                    r = r + rho * hat[w - 1]
                if w < N - 1:
                    r = r + rho * hat[w + 1]
                th[w] = Mi[w] @ r if Mi is not None else np.linalg.solve(A[w] + deg[w] * rho * np.eye(d), r)
            cand = Q.quantize_rows(th[ws], hat[ws], bits, Q.u01(seed, it, N, ws, d))[2]
            for k, w in enumerate(ws):
                s = butterfly_sum([(float(c) - float(h)) * (float(c) - float(h)) for c, h in zip(cand[k], hat[w])])
                if s >= thr[it] * thr[it]:
                    hat[w] = cand[k]
                    row[w] = True
        for w in range(N):
            m = mu[w]
            if w > 0:
                m = m - rho * (hat[w - 1] - hat[w])
            if w < N - 1:
                m = m + rho * (hat[w] - hat[w + 1])
            mu[w] = m
        sent.append(row)
        f = sum(0.5 * np.sum((X[w] @ th[w] - y[w]) ** 2) for w in range(N))
        if abs(f - obj0) < tol:
            break
    return it, np.array(sent)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = []
    for N, censor, tol in ((8, (1.0, 0.9), 1e-8), (24, (1.0, 0.98), 1e-4)):
        first = {}
        stop = {}
        for solve in ("solve", "inverse"):
            _, tr = run(N, censor, 0.0, solve, 80)
            first[solve] = tr
            it, full = run(N, censor, tol, solve, 3000)
            stop[solve] = [int(it), int(full.sum())]
        assert np.array_equal(first["solve"], first["inverse"])
        tr = first["solve"]
        cases.append({"N": N, "d": 50, "bits": 8, "seed": 1234, "rho": 3.0, "censor": list(censor),
                      "cumulative_transmissions_20_40_60_80": [int(tr[:k].sum()) for k in (20, 40, 60, 80)],
                      "iterations_everybody_sends": int(tr.all(axis=1).sum()),
                      "iterations_nobody_sends": int((~tr.any(axis=1)).sum()),
                      "tol": tol, "iterations_transmissions_at_stop": stop})
    out = {"produced_by": "tools/cqgadmm_prototype.py", "cases": cases}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
