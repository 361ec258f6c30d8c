"""High-precision reference of Q-GGADMM (the quantized recurrence of gadmm_amd/algorithms/ggadmm.py),
NumPy only, written from that module's docstring:

    heads, all at once:  r = b_n - mu_n;  for k in N(n) ascending: r = r + rho hat_k   (tails' hat^{it-1})
                         theta_n = (A_n + rho deg_n I)^{-1} r                           (the TRUE iterate)
                         (R, q, hat_n) = quantizer line(theta_n, hat_n, bits, u(seed, it, N, n, d))
    tails, all at once:  the same with the heads' hat^{it}
    every worker:        for k in N(n) ascending: mu_n = mu_n + rho (hat_n - hat_k)     (public models)
    objective            of the TRUE theta; K4 residual over the edges on the public models

It is built on ``hp_ggadmm``'s adjacency and case data and on ``hp_reference.q_line`` / ``q_uniforms`` (the
quantizer line and the counter formula restated in Python integers) and shares no code with ggadmm.py or
quantize.py. Every function does all of its arithmetic in ``dtype`` (long double: the reference;
float64: the noise of the recurrence). Bounds are ``hp_reference.bound`` unchanged.

A quantized case is comparable under the project's own condition (``hp_reference.QGADMM_MARGIN``): the
long-double and the float64 run produce identical codes, and the smallest flip margin is at least
QGADMM_MARGIN b_theta over the longest run a test asks for. ``SEEDS`` records, per case, the first quantizer
seed of 1234..1297 that qualifies; ``DROPPED`` the cases none serves (none).

This is a helper module, not a conftest: test modules import it as ``import hp_qggadmm``.
"""
import numpy as np

import hp_ggadmm as G
from hp_reference import LD, QGADMM_FIRST_SEED, QGADMM_LAST_SEED, QGADMM_MARGIN, Reference, _cached, _freeze, _gram, \
    _gram_objective, _own_or_largest, bound, make_linear, noise_level, q_line, q_uniforms, seed_of, spd_inverse

from gadmm_amd.parallel import topology as T

OVERRUN = G.OVERRUN   # a persistent kernel stops at most this many iterations past its cap
CAP = 8               # the cap of the class test (no stop rule)
RUN = CAP + OVERRUN   # the longest run the class test asks of a case
BITS = (4, 8, 16)
MUTANTS = ("dual-true", "rhs-true", "obj-hat", "twice", "stale", "u-slot")


def _dequant(hat, R, q, bits, dtype):
    """A receiver's line: ``hat + (q delta - R)``, ``delta = 2R / L``; ``hat`` at ``R == 0``."""
    if R == 0:
        return hat.copy()
    L = np.asarray((1 << int(bits)) - 1, dtype=dtype)
    delta = (np.asarray(2.0, dtype=dtype) * R) / L
    return hat + (np.asarray(q, dtype=dtype) * delta - R)


def qggadmm_run(X, y, rho, K, edges, heads, bits, seed, dtype=LD, mutant=None):
    """K iterations from theta = hat = mu = 0. Returns ``(theta (K, N, d) true iterates, hat (K, N, d),
    mu (K, N, d), objectives (K,), codes (K, N, d) int64, R (K, N), K4 rows (K, N) -- a tail's entry is the
    squared distance of the public models over its edges, a head's 0 --, margin (K,) the smallest flip
    margin up to each iteration)``; a run to k is a prefix of a longer one.

    ``mutant`` names a wrong implementation. ``"dual-true"``: the duals read true iterates; ``"rhs-true"``:
    the right-hand sides read the neighbours' true iterates; ``"obj-hat"``: the objective of the public
    models; ``"u-slot"``: the uniforms indexed by launch slot (heads in ascending id, then tails) instead
    of worker id. Two act on ONE copy, that of the last neighbour held by the first worker of degree >= 3
    (ascending id; one must exist): ``"twice"`` applies every message to it twice, ``"stale"`` leaves it
    one message behind."""
    X = np.asarray(X)
    N, m, d = X.shape
    assert mutant is None or mutant in MUTANTS
    hs, nb = G._adjacency(N, edges, heads)
    A, b, yy = _gram(X, y, dtype)
    rho = np.asarray(rho, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    Minv = [spd_inverse(A[w] + len(nb[w]) * rho * eye, dtype) for w in range(N)]
    groups = (sorted(hs), [w for w in range(N) if w not in hs])
    slot = {w: i for i, w in enumerate(groups[0] + groups[1])}
    victim = src = None
    if mutant in ("twice", "stale"):
        victim = next(w for w in range(N) if len(nb[w]) >= 3)
        src = nb[victim][-1]
    th = np.zeros((N, d), dtype=dtype)
    hat = np.zeros((N, d), dtype=dtype)
    mu = np.zeros((N, d), dtype=dtype)
    wrong = np.zeros(d, dtype=dtype)   # the victim's copy of hat[src] under "twice" / "stale"
    out_th = np.zeros((K, N, d), dtype=dtype)
    out_hat = np.zeros((K, N, d), dtype=dtype)
    out_mu = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    codes = np.zeros((K, N, d), dtype=np.int64)
    Rs = np.zeros((K, N), dtype=dtype)
    rows = np.zeros((K, N), dtype=dtype)
    margins = np.zeros((K,), dtype=np.float64)
    margin = np.inf

    def public(w, j):  # what worker w holds of neighbour j's public model
        return wrong if (w == victim and j == src) else hat[j]

    for k in range(1, K + 1):
        for group in groups:
            for w in group:
                r = b[w] - mu[w]
                for j in nb[w]:
                    r = r + rho * (th[j] if mutant == "rhs-true" else public(w, j))
                th[w] = Minv[w] @ r
                u = q_uniforms(seed, k, N, slot[w] if mutant == "u-slot" else w, d)
                before = hat[w].copy()
                Rs[k - 1, w], codes[k - 1, w], hat[w], mg = q_line(th[w], hat[w], u, bits, dtype)
                margin = min(margin, mg)
                if w == src:
                    if mutant == "twice":
                        wrong = _dequant(_dequant(wrong, Rs[k - 1, w], codes[k - 1, w], bits, dtype), Rs[k - 1, w],
                                         codes[k - 1, w], bits, dtype)
                    elif mutant == "stale":
                        wrong = before
        new_mu = mu.copy()
        for w in range(N):
            v = mu[w]
            own = th[w] if mutant == "dual-true" else hat[w]
            for j in nb[w]:
                v = v + rho * (own - (th[j] if mutant == "dual-true" else public(w, j)))
            new_mu[w] = v
        mu = new_mu
        out_th[k - 1], out_hat[k - 1], out_mu[k - 1] = th, hat, mu
        obj[k - 1] = _gram_objective(A, b, yy, hat if mutant == "obj-hat" else th)
        for t in groups[1]:
            tot = np.zeros((), dtype=dtype)
            for h in nb[t]:
                e = hat[h] - hat[t]
                tot = tot + e @ e
            rows[k - 1, t] = tot
        margins[k - 1] = margin
    return out_th, out_hat, out_mu, obj, codes, Rs, rows, margins


class QGraphReference(Reference):
    """``hp_reference.Reference`` of a Q-GGADMM case: ``theta`` (K, N, d) the TRUE iterates, ``dual`` the
    per-worker duals after K, ``obj``; plus ``hat`` (N, d) the public models after K, ``codes`` (K, N, d),
    ``R`` (K, N), ``res_w`` (K, N) the K4 rows on the public models with ``tails`` (K, N), ``margin`` the
    run's smallest flip margin, ``codes_agree`` (the float64 run produced the same codes), ``seed``, and
    the bounds ``b_hat`` / ``b_R`` (errors over ``scale_theta``) and ``b_res_w`` (each tail entry over its
    own value, as ``GraphReference``)."""

    def __init__(self, ld, f64, rho, d, heads, seed, bits):
        th, hats, mus, obj, codes, Rs, rows, margins = ld
        Reference.__init__(self, (th, mus[-1], obj), (f64[0], f64[2][-1], f64[3]), rho, d, residual=False)
        K, N = th.shape[:2]
        self.seed, self.bits = seed, bits
        self.hat, self.codes, self.R, self.margin = hats[-1], codes, Rs, float(margins[-1])
        self.codes_agree = bool(np.array_equal(codes, f64[4]))
        hs = set(int(h) for h in heads)
        self.tails = np.tile(np.asarray([w not in hs for w in range(N)]), (K, 1))
        self.res_w = rows
        self.res_w_scale = _own_or_largest(rows)
        self.e_hat = noise_level(hats, f64[1], self.scale_theta)
        self.e_R = noise_level(Rs, f64[5], self.scale_theta)
        self.e_res_w = self.err_res_w(f64[6])
        self.b_hat, self.b_R, self.b_res_w = bound(self.e_hat, d), bound(self.e_R, d), bound(self.e_res_w, d)

    def err_hat(self, hat):
        return noise_level(self.hat, hat, self.scale_theta)

    def err_R(self, R):
        """``R`` (N,) of every worker's last message against the reference's last iteration."""
        return noise_level(self.R[-1], R, self.scale_theta)

    def err_res_w(self, rows):
        k = len(rows)
        diff = np.abs(self.res_w[:k] - np.asarray(rows, dtype=LD)) / self.res_w_scale[:k]
        diff = diff[self.tails[:k]]
        return float(np.max(diff)) if diff.size else 0.0


def _star_leaf_heads(n, hub):
    return T.BipartiteGraph(n, [(hub, w) for w in range(n) if w != hub], heads=[w for w in range(n) if w != hub])


# hp_ggadmm's data of K(4, 4), d = 53 (m = 70) has no qualifying seed in 1234..1297 at b = 16, nor have ten
# other data seeds or m = 55 .. 160: the dense graph converges so fast that after 24 iterations R is 1e-6
# and a 16-bit step 1e-10 of the iterate, which leaves the smallest of 10^4 flip margins at 1e-14, below
# b_theta. The shape stays and m goes to 30 (rows < d: a slower solve, R = 4e-5 at 24 iterations), with data
# of its own at every bit width.
#
# name -> (graph, rows per shard m, d, the bit widths it runs at): tests/test_gpu_qggadmm.py says what each
# exercises. A name of hp_ggadmm.CASES takes that case's graph and data.
CASES = {
    "edge-d1": (None, 3, 1, BITS),
    "edge-d16": (lambda: T.chain_graph(2), 30, 16, (4,)),   # b = 4: the last code word full ...
    "edge-d17": (lambda: T.chain_graph(2), 30, 17, (4,)),   # ... then one code in a new word
    "edge-d8": (lambda: T.chain_graph(2), 20, 8, (8,)),
    "edge-d9": (lambda: T.chain_graph(2), 20, 9, (8,)),
    "edge-d4": (lambda: T.chain_graph(2), 20, 4, (16,)),
    "edge-d5": (lambda: T.chain_graph(2), 20, 5, (16,)),
    "ring4-d7": (None, 12, 7, BITS),
    "grid2x3-d50": (None, 60, 50, BITS),
    "k23-d52": (None, 60, 52, BITS),
    "k44-d53": (lambda: T.complete_bipartite_graph(4, 4), 30, 53, BITS),
    "star8-d64": (None, 40, 64, BITS),
    "star12hub5-d50": (None, 60, 50, (8,)),
    "star20-d7": (lambda: T.star_graph(20, 0), 12, 7, BITS),          # degree 19: two poll groups, the hub a head
    "star20tail-d7": (lambda: _star_leaf_heads(20, 0), 12, 7, (8,)),  # ... and the hub a tail
}
# The runs to the 1e-4 stop (E1's shape: d = 50, 50 rows per shard; b = 8): name -> (graph, m, d, rho).
# A run must stay comparable to its stop + OVERRUN. With make_linear's rho = 0.5 m = 25 the stop comes after
# 91 .. 125 iterations, by when R has fallen to 1e-8 and the smallest flip margin to 1e-14, below b_theta: at
# every seed tried the float64 codes part from the long-double ones before the run ends. At rho = 200 the
# quantization noise keeps R up and the stop comes after 54 .. 68 iterations; STOP_SEEDS holds the first
# seed that qualifies over STOP_RUN = (its iterations to the stop) + OVERRUN, found on the CPU.
STOP_CASES = {
    "stop-grid4x6": (lambda: T.grid_graph(4, 6), 50, 50, 200.0),
    "stop-star20tail": (lambda: _star_leaf_heads(20, 0), 50, 50, 200.0),
}
STOP_TOL = 1e-4
STOP_MAX_ITER = 2000
STOP_SEEDS = {"stop-grid4x6": 1243, "stop-star20tail": 1235}   # 1234 gives margin / b_theta = 2.92 and 1.51
STOP_RUN = {"stop-grid4x6": 66 + OVERRUN, "stop-star20tail": 54 + OVERRUN}

# (case, bits) -> the quantizer seed: the first of 1234, 1235, ... at which the long-double and the float64
# run produce identical codes and the smallest flip margin is >= QGADMM_MARGIN b_theta over RUN iterations
# (the stop cases: over the iterations to their stop + OVERRUN). Found once by a search on the CPU
# (``find_seed``); only the cases that 1234 does not serve are listed. tests/test_qggadmm_cpu.py asserts
# the condition for every case.
SEEDS = {
    ("ring4-d7", 16): 1235,   # 1234: margin / b_theta = 0.92 at 24 iterations
    ("k23-d52", 16): 1241,    # 1234: 3.06
}
DROPPED = ()


def cases():
    """Every ``(name, bits)`` of the class test."""
    return [(name, b) for name, c in CASES.items() for b in c[3]]


def case_graph(name):
    spec = CASES.get(name) or STOP_CASES[name]
    if spec[0] is None:
        return G.case_graph(name)
    return _cached(("qggadmm-graph", name), spec[0])


def case_data(name):
    """``(graph, X, y, rho)``: hp_ggadmm's data where the case is one of its own, else ``make_linear``
    seeded the same way (by the shape and the edge count)."""
    spec = CASES.get(name) or STOP_CASES[name]
    if spec[0] is None:
        assert G.CASES[name][1:] == spec[1:3]
        return G.case_data(name)

    def build():
        g = case_graph(name)
        X, y, rho = make_linear(g.n, spec[1], spec[2], seed_of(g.n, spec[1], spec[2]) + 7919 * len(g.edges))
        _freeze(X, y)
        return g, X, y, (spec[3] if name in STOP_CASES else rho)
    return _cached(("qggadmm-data", name), build)


def seed_for(name, bits):
    return SEEDS.get((name, bits), QGADMM_FIRST_SEED)


def _history(name, bits, seed, run, dtype, mutant=None):
    def build():
        g, X, y, rho = case_data(name)
        out = qggadmm_run(X, y, rho, run, g.edges, g.heads, bits, seed, dtype, mutant)
        _freeze(*out)
        return out
    return _cached(("qggadmm-run", name, bits, seed, run, np.dtype(dtype).name, mutant), build)


def reference(name, bits, K, seed=None, run=RUN):
    """``(graph, X, y, rho, QGraphReference)`` of the first ``K`` iterations of a ``run``-iteration run."""
    seed = seed_for(name, bits) if seed is None else seed
    assert K <= run

    def build():
        g, X, y, rho = case_data(name)
        ld = _history(name, bits, seed, run, LD)
        f64 = _history(name, bits, seed, run, np.float64)
        d = X.shape[2]
        return g, X, y, rho, QGraphReference(tuple(a[:K] for a in ld), tuple(a[:K] for a in f64), rho, d, g.heads,
                                             seed, bits)
    return _cached(("qggadmm-case", name, bits, K, seed, run), build)


def case(name, bits, K=RUN):
    return reference(name, bits, K)


def condition(name, bits, run=RUN, seed=None):
    """``(codes of the long-double and the float64 run identical, margin / b_theta)`` over ``run``
    iterations; the case qualifies when the first holds and the second is >= QGADMM_MARGIN."""
    ref = reference(name, bits, run, seed, run)[4]
    return ref.codes_agree, ref.margin / ref.b_theta


def find_seed(name, bits, run=RUN):
    """The first seed of QGADMM_FIRST_SEED..QGADMM_LAST_SEED that qualifies over ``run`` iterations, or None."""
    for seed in range(QGADMM_FIRST_SEED, QGADMM_LAST_SEED + 1):
        agree, ratio = condition(name, bits, run, seed)
        if agree and ratio >= QGADMM_MARGIN:
            return seed
    return None


def mutant_factors(name, bits, K=RUN):
    """``{mutant: max over (theta, hat, dual, objective) of err / bound}`` of the float64 mutants of a
    case against its reference; ``None`` for a mutant that IS the recurrence on this graph (``"u-slot"``
    where the launch order is the identity: star_graph(n, 0) with the hub a head, whose hub comes first
    in both orders)."""
    g, X, y, rho, ref = reference(name, bits, K)
    out = {}
    for mut in MUTANTS:
        if mut == "u-slot" and list(g.order) == list(range(g.n)):
            out[mut] = None
            continue
        th, hats, mus, obj = _history(name, bits, ref.seed, K, np.float64, mut)[:4]
        out[mut] = max(ref.err_theta(th[-1], K) / ref.b_theta, ref.err_hat(hats[-1]) / ref.b_hat,
                       ref.err_dual(mus[-1]) / ref.b_dual, ref.err_obj(obj) / ref.b_obj)
    return out


__all__ = ["qggadmm_run", "QGraphReference", "CASES", "STOP_CASES", "STOP_SEEDS", "STOP_RUN", "cases", "case", "case_data", "case_graph",
           "reference", "condition", "find_seed", "seed_for", "mutant_factors", "MUTANTS", "SEEDS", "DROPPED"]
