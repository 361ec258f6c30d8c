"""High-precision reference of GGADMM (gadmm_amd/algorithms/ggadmm.py) in EDGE-DUAL form, NumPy only.

The code under test keeps one aggregated dual per worker. This reference keeps one multiplier
``lam_e`` per edge ``e = (h, t)``, as the paper writes the algorithm (Ben Issaid et al.,
arXiv:2009.06459, for the constraint ``theta_h = theta_t`` on every edge):

    heads:  theta_h = (A_h + rho deg_h I)^{-1} (b_h - sum_{e at h} lam_e + rho sum_{t in N(h)} theta_t)
    tails:  theta_t = (A_t + rho deg_t I)^{-1} (b_t + sum_{e at t} lam_e + rho sum_{h in N(t)} theta_h)
    edges:  lam_e   = lam_e + rho (theta_h - theta_t)

so it shares no dual bookkeeping with the per-worker form: a wrong sign, a missed neighbour or a
stale read in the per-worker update shows as a difference. What is compared is theta, the objective,
the K4 rows and the per-worker aggregate ``mu_h = sum_{e at h} lam_e``, ``mu_t = -sum_{e at t} lam_e``.

Every function does all of its arithmetic in ``dtype`` (long double: the reference; float64: the noise
of the recurrence, ``hp_reference.noise_level``). The bounds are ``hp_reference.bound`` unchanged: the
float64 run of this very recurrence sums the same ``deg`` neighbour terms per right-hand side, so the
(deg - 2) further roundings of ``rho max|theta|`` that a right-hand side of degree ``deg`` has over a
chain's are already in the measured noise ``e64``; no term is added for them, and none is fitted to a
kernel.

This is a helper module, not a conftest: test modules import it as ``import hp_ggadmm``.
"""
import numpy as np

from hp_reference import K_ITERS, LD, Reference, _cached, _freeze, _own_or_largest, bound, make_linear, noise_level, \
    seed_of, spd_inverse

from gadmm_amd.parallel import topology as T

MUTANTS = ("drop-edge", "stale", "deg-1")
OVERRUN = 16  # a persistent kernel stops at most this many iterations past K (lag + slack, as hp_reference)


def _adjacency(n, edges, heads):
    hs = set(int(h) for h in heads)
    nb = [[] for _ in range(n)]
    for a, b in edges:
        a, b = int(a), int(b)
        assert (a in hs) != (b in hs), "every edge joins a head to a tail"
        nb[a].append(b)
        nb[b].append(a)
    return hs, [sorted(v) for v in nb]


def ggadmm_run(X, y, rho, K, edges, heads, dtype=LD, mutant=None):
    """K iterations from theta = 0, lam = 0. ``edges``: pairs of worker ids, ``heads``: one colour class.
    ``mutant`` names a wrong implementation, applied at the first worker of degree >= 3 (ascending id; one
    must exist): ``"drop-edge"`` leaves its last neighbour out of its right-hand side, ``"stale"`` reads
    that neighbour one iteration stale there, ``"deg-1"`` builds its inverse with ``deg - 1``.
    Returns ``(theta (K, N, d), mu (K, N, d) per-worker aggregates after each iteration, objectives (K,))``."""
    X = np.asarray(X)
    N, m, d = X.shape
    assert mutant is None or mutant in MUTANTS
    Xd, yd = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    A = np.einsum("nmi,nmj->nij", Xd, Xd)
    b = np.einsum("nmi,nm->ni", Xd, yd)
    yy = np.einsum("nm,nm->n", yd, yd)
    rho = np.asarray(rho, dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    hs, nb = _adjacency(N, edges, heads)
    E = [(a, b_) if a in hs else (b_, a) for a, b_ in ((int(u), int(v)) for u, v in edges)]
    at = [[e for e, (h, t) in enumerate(E) if w in (h, t)] for w in range(N)]
    victim = None
    if mutant is not None:
        victim = next(w for w in range(N) if len(nb[w]) >= 3)
    Minv = [spd_inverse(A[w] + (len(nb[w]) - (1 if (mutant == "deg-1" and w == victim) else 0)) * rho * eye, dtype)
            for w in range(N)]
    th = np.zeros((N, d), dtype=dtype)
    prev = th.copy()
    lam = np.zeros((len(E), d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    mus = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    order = sorted(hs) + [w for w in range(N) if w not in hs]
    for k in range(K):
        before = th.copy()  # theta^{k-1} of every worker (what a head reads of its tails)
        for w in order:
            sgn = -1 if w in hs else 1
            r = b[w].copy()
            for e in at[w]:
                r = r + sgn * lam[e]
            for j in nb[w]:
                if w == victim and j == nb[w][-1]:
                    if mutant == "drop-edge":
                        continue
                    if mutant == "stale":
                        # one iteration older than what the worker should read: a head should read its
                        # tails' theta^{k-1} (gets k-2), a tail its heads' theta^{k} (gets k-1)
                        r = r + rho * (prev[j] if w in hs else before[j])
                        continue
                r = r + rho * th[j]
            th[w] = Minv[w] @ r
        for e, (h, t) in enumerate(E):
            lam[e] = lam[e] + rho * (th[h] - th[t])
        prev = before
        thetas[k] = th
        for w in range(N):
            agg = np.zeros(d, dtype=dtype)
            for e in at[w]:
                agg = agg + lam[e]
            mus[k, w] = agg if w in hs else -agg
        tot = np.zeros((), dtype=dtype)
        for w in range(N):
            tot = tot + (half * (th[w] @ (A[w] @ th[w])) - b[w] @ th[w] + half * yy[w])
        obj[k] = tot
    return thetas, mus, obj


def ggadmm_linear(X, y, rho, K, edges, heads, dtype=LD, mutant=None):
    """``(theta (K, N, d), mu (N, d) per-worker aggregates after iteration K, objectives (K,))``."""
    th, mus, obj = ggadmm_run(X, y, rho, K, edges, heads, dtype, mutant)
    return th, mus[-1], obj


def graph_residual(theta_hist, edges, heads, dtype=LD):
    """K4 rows (K, N): a tail's entry is ``sum_{h in N(t)} |theta_h - theta_t|^2`` after each iteration
    (each edge once, its tail owns it); a head's is 0."""
    th = np.asarray(theta_hist, dtype=dtype)
    K, N, d = th.shape
    hs, nb = _adjacency(N, edges, heads)
    out = np.zeros((K, N), dtype=dtype)
    for k in range(K):
        for t in range(N):
            if t in hs:
                continue
            tot = np.zeros((), dtype=dtype)
            for h in nb[t]:
                tot = tot + np.sum((th[k, h] - th[k, t]) ** 2)
            out[k, t] = tot
    return out


class GraphReference(Reference):
    """``hp_reference.Reference`` of a GGADMM case (theta, dual, objective and their bounds) plus the K4
    rows over the graph's edges: ``res_w`` (K, N), ``tails`` (K, N) bool, the noise ``e_res_w`` of the
    float64 history (each entry over its own reference value, as ``Reference``), ``b_res_w``."""

    def __init__(self, ld, f64, rho, d, edges, heads):
        Reference.__init__(self, ld, f64, rho, d, residual=False)
        K, N = self.theta.shape[:2]
        hs = set(int(h) for h in heads)
        self.tails = np.tile(np.asarray([w not in hs for w in range(N)]), (K, 1))
        self.res_w = graph_residual(self.theta, edges, heads, LD)
        res64 = graph_residual(np.asarray(f64[0], dtype=np.float64), edges, heads, np.float64)
        self.res_w_scale = _own_or_largest(self.res_w)
        self.e_res_w = self.err_res_w(res64)
        self.b_res_w = bound(self.e_res_w, d)
        _freeze(self.tails, self.res_w, self.res_w_scale)

    def err_res_w(self, rows):
        k = len(rows)
        diff = np.abs(self.res_w[:k] - np.asarray(rows, dtype=LD)) / self.res_w_scale[:k]
        diff = diff[self.tails[:k]]
        return float(np.max(diff)) if diff.size else 0.0


def _star_leaf_heads(n, hub):
    return T.BipartiteGraph(n, [(hub, w) for w in range(n) if w != hub], heads=[w for w in range(n) if w != hub])


# (name, graph, rows per shard m, d): the smallest shapes at which each thing can break
# (tests/test_gpu_ggadmm.py says what each exercises)
CASES = {
    "edge-d1": (lambda: T.chain_graph(2), 3, 1),
    "edge-d50": (lambda: T.chain_graph(2), 60, 50),
    "ring4-d7": (lambda: T.ring_graph(4), 12, 7),
    "grid2x3-d50": (lambda: T.grid_graph(2, 3), 60, 50),
    "k23-d52": (lambda: T.complete_bipartite_graph(2, 3), 60, 52),
    "k44-d53": (lambda: T.complete_bipartite_graph(4, 4), 70, 53),
    "star8-d64": (lambda: T.star_graph(8, 0), 40, 64),
    "star12hub5-d50": (lambda: _star_leaf_heads(12, 5), 60, 50),
    "grid4x6-d50": (lambda: T.grid_graph(4, 6), 60, 50),
    "star40-d7": (lambda: T.star_graph(40, 0), 12, 7),
}


def case_graph(name):
    return _cached(("ggadmm-graph", name), CASES[name][0])


def case_data(name):
    """``(graph, X, y, rho)``: ``make_linear`` data seeded by the shape and the edge count."""
    def build():
        g = case_graph(name)
        _, m, d = CASES[name]
        X, y, rho = make_linear(g.n, m, d, seed_of(g.n, m, d) + 7919 * len(g.edges))
        _freeze(X, y)
        return g, X, y, rho
    return _cached(("ggadmm-data", name), build)


def _history(name, K, dtype):
    """One run of the recurrence per (case, arithmetic), long enough for every ``last`` a test asks for."""
    run = K_ITERS if K <= K_ITERS else K_ITERS + OVERRUN
    assert K <= run

    def build():
        g, X, y, rho = case_data(name)
        out = ggadmm_run(X, y, rho, run, g.edges, g.heads, dtype)
        _freeze(*out)
        return out
    return _cached(("ggadmm-run", name, run, np.dtype(dtype).name), build)


def case(name, K=K_ITERS):
    """``(graph, X, y, rho, GraphReference)`` of ``K`` iterations of case ``name``."""
    def build():
        g, X, y, rho = case_data(name)
        th, mus, obj = _history(name, K, LD)
        th64, mus64, obj64 = _history(name, K, np.float64)
        ref = GraphReference((th[:K], mus[K - 1], obj[:K]), (th64[:K], mus64[K - 1], obj64[:K]), rho,
                             CASES[name][2], g.edges, g.heads)
        return g, X, y, rho, ref
    return _cached(("ggadmm-case", name, K), build)


def mutant_factors(name, K=K_ITERS):
    """``{mutant: max over (theta, dual, objective) of err / bound}`` of the float64 mutants of case
    ``name`` against its reference: how far above the bound each wrong implementation lands."""
    g, X, y, rho, ref = case(name, K)
    out = {}
    for mut in MUTANTS:
        th, mu, obj = ggadmm_linear(X, y, rho, K, g.edges, g.heads, np.float64, mutant=mut)
        out[mut] = max(ref.err_theta(th[-1], K) / ref.b_theta, ref.err_dual(mu) / ref.b_dual,
                       ref.err_obj(obj) / ref.b_obj)
    return out


__all__ = ["ggadmm_linear", "ggadmm_run", "graph_residual", "GraphReference", "CASES", "case", "case_data",
           "case_graph", "mutant_factors", "MUTANTS", "noise_level"]
