"""High-precision reference of logistic GGADMM (``graph_admm_logistic``, gadmm_amd/algorithms/ggadmm.py) in
EDGE-DUAL form, NumPy only: one multiplier ``lam_e`` per edge ``e = (h, t)``, heads take ``+sum lam_e`` and
tails ``-sum lam_e`` into the frozen shift, ``lam_e += rho (theta_h - theta_t)`` (as ``hp_ggadmm.ggadmm_run``),
with the inner GD, its strict stop, the step counts and the stop margin of ``hp_reference.gadmm_logistic_gd``.
The bounds are ``hp_reference.bound`` unchanged, nothing fitted to a kernel. A helper module, not a conftest.
"""
import numpy as np

from hp_ggadmm import GraphReference, _adjacency, _star_leaf_heads
from hp_reference import K_ITERS, LD, MAX_INNER, Reference, _cached, _freeze, bound, make_logistic, seed_of

from gadmm_amd.parallel import topology as T


def glogistic_run(X, y, rho, lam, step, K, max_inner, inner_tol, edges, heads, dtype=LD):
    """K iterations from theta = 0, lam_e = 0: ``(theta (K, N, d), per-worker dual aggregates (K, N, d), objectives
    (K,), inner step counts (K, N), margin)``; ``margin`` as in ``hp_reference.gadmm_logistic_gd``."""
    N, m, d = np.asarray(X).shape
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    rho, lam, step, tol = (np.asarray(v, dtype=dtype) for v in (rho, lam, step, inner_tol))
    one, half = np.asarray(1.0, dtype=dtype), np.asarray(0.5, dtype=dtype)
    hs, nb = _adjacency(N, edges, heads)
    E = [(a, b) if a in hs else (b, a) for a, b in ((int(u), int(v)) for u, v in edges)]
    at = [[e for e, (h, t) in enumerate(E) if w in (h, t)] for w in range(N)]
    th = np.zeros((N, d), dtype=dtype)
    lam_e = np.zeros((len(E), d), dtype=dtype)
    thetas, mus = np.zeros((K, N, d), dtype=dtype), np.zeros((K, N, d), dtype=dtype)
    obj, inner, margin = np.zeros((K,), dtype=dtype), np.zeros((K, N), dtype=np.int64), np.inf
    for k in range(K):
        for w in sorted(hs) + [w for w in range(N) if w not in hs]:
            s = np.zeros(d, dtype=dtype)
            for e in at[w]:
                s = s + lam_e[e] if w in hs else s - lam_e[e]
            for j in nb[w]:
                s = s + rho * (th[w] - th[j])
            x = th[w].copy()
            for _ in range(int(max_inner)):
                g = -(X[w].T @ (y[w] / (one + np.exp(y[w] * (X[w] @ x))))) + lam * x + s
                x_new = x - step * g
                dx = np.max(np.abs(x_new - x))
                x = x_new
                inner[k, w] += 1
                if tol > 0:
                    margin = min(margin, float(abs(dx / tol - one)))
                if dx < tol:
                    break
            th[w] = x
        for e, (h, t) in enumerate(E):
            lam_e[e] = lam_e[e] + rho * (th[h] - th[t])
        thetas[k] = th
        for w in range(N):
            agg = sum((lam_e[e] for e in at[w]), np.zeros(d, dtype=dtype))
            mus[k, w] = agg if w in hs else -agg
            obj[k] = obj[k] + (lam * half * (th[w] @ th[w]) + np.sum(np.log1p(np.exp(-y[w] * (X[w] @ th[w])))))
    return thetas, mus, obj, inner, margin


class GLReference(GraphReference):
    """``GraphReference`` with the bounds of ``Reference(..., m_logistic=m)``; ``extra = (step counts, margin)``."""

    def __init__(self, ld, f64, rho, d, m, edges, heads):
        GraphReference.__init__(self, ld, f64, rho, d, edges, heads)
        Reference.__init__(self, ld, f64, rho, d, m_logistic=m, residual=False)
        self.b_res_w = bound(self.e_res_w, d, m)


# name: (graph, rows per shard m, d, inner_tol), each the smallest shape at which its thing can break
CASES = {
    "edge-m5-d3": (lambda: T.chain_graph(2), 5, 3, 0.0),                         # the smallest graph
    "ring4-m30-d20": (lambda: T.ring_graph(4), 30, 20, 0.0),                     # no degree-1 worker
    "k23-m40-d52": (lambda: T.complete_bipartite_graph(2, 3), 40, 52, 0.0),      # top of QT = 13 through d; class 4
    "grid2x3-m52-d20": (lambda: T.grid_graph(2, 3), 52, 20, 0.0),                # top of QT = 13 through m
    "k44-m40-d53": (lambda: T.complete_bipartite_graph(4, 4), 40, 53, 0.0),      # first of QT = 16 through d
    "star8-m64-d64": (lambda: T.star_graph(8, 0), 64, 64, 0.0),                  # full lanes; degree 7, class 8
    "star12hub5-m53-d20": (lambda: _star_leaf_heads(12, 5), 53, 20, 0.0),        # QT = 16 through m; a 2nd poll group
    "star20-m12-d7": (lambda: T.star_graph(20, 0), 12, 7, 0.0),                  # degree 19: a third poll group
    "grid2x3-m52-d20-live": (lambda: T.grid_graph(2, 3), 52, 20, 1e-3),          # the live inner stop rule
}
LIVE = "grid2x3-m52-d20-live"


def case_data(name):
    """``(graph, X, y, rho = 0.2 / (step * max_degree), lam, step, inner_tol)`` on ``make_logistic`` data."""
    def build():
        make, m, d, tol = CASES[name]
        g = make()
        X, y, _, lam, step = make_logistic(g.n, m, d, seed_of(g.n, m, d) + 7919 * len(g.edges))
        _freeze(X, y)
        return g, X, y, 0.2 / (step * g.max_degree), lam, step, tol
    return _cached(("glogistic-data", name), build)


def case(name, K=K_ITERS):
    """``case_data(name)`` + the ``GLReference`` of ``K`` iterations (``MAX_INNER`` inner steps)."""
    def build():
        g, X, y, rho, lam, step, tol = data = case_data(name)
        ld, f64 = ((h[0], h[1][-1], h[2], h[3], h[4]) for h in (
            glogistic_run(X, y, rho, lam, step, K, MAX_INNER, tol, g.edges, g.heads, t) for t in (LD, np.float64)))
        return data + (GLReference(ld, f64, rho, X.shape[2], X.shape[1], g.edges, g.heads),)
    return _cached(("glogistic-case", name, K), build)
