"""Plain high-precision references of the solvers the HIP kernels implement (CPU, NumPy only).

Every function takes ``dtype`` (``np.longdouble`` or ``np.float64``) and does all of its arithmetic in
that dtype: the long-double run is the reference a kernel is held against, the float64 run of the very
same recurrence measures how far two correct float64 implementations may sit apart
(``noise_level``). The recurrences follow gadmm_amd/oracle/reference.py (the executable
specification), in the form the kernels evaluate them:

* the closed-form local solve applies an explicit inverse of ``A_n + deg rho I`` (the kernels cache
  it); NumPy has no long-double solve, so the long-double inverse is the float64 one refined by
  three Newton-Schulz steps ``X <- X (2 I - M X)`` (quadratic: 1e-13 -> 1e-26 -> below 2^-63);
* the linear objective is the Gram form ``1/2 th'A th - b'th + 1/2 y'y``;
* chain duals are the per-worker aggregates ``mu_n = lam_n - lam_{n-1}`` (D-GADMM form);
* D-GADMM (``dgadmm_linear``) is that recurrence over a list of chains: neighbours, roles and the
  degree's inverse follow the chain of the iteration; ``dgadmm_chains`` prescribes the chains;
* the K4 primal residual (``chain_residual``) is a function of a run's theta history and its chains: the
  tails' ``|th_l - th|^2 + |th - th_r|^2`` per (iteration, worker), what the chain kernels emit beside
  theta, the duals and the objective; ``Reference`` holds it for every chain case;
* Q-GADMM (``qgadmm_linear``) is ``gadmm_linear`` over a static chain whose theta table holds the public
  models th_hat; its quantizer line restates gadmm_amd/algorithms/quantize.py and is held against it bit
  for bit, the run against the torch path, by tests/test_hp_reference_cpu.py;
* the exact logistic prox (``gadmm_logistic_newton``) has no oracle counterpart: it follows the header
  of csrc/kernels/chain_newton.hip and is held against the torch path (models/logistic.py:newton_prox)
  by tests/test_hp_reference_cpu.py. Its long-double run is the converged prox (stop tolerance 1e-17);
  the float64 run stops as the kernels do (1e-13), optionally under their chord rule;
* the first-order baselines (``first_order``) follow the torch path (algorithms/baselines.py,
  dual_averaging.py), quirks included, with the scalar inputs (step, Hmax_n^2, LAG's threshold factor,
  IAG's schedule) computed once in float64 and shared with the engines;
* the set-up kernels (Grams, inverses) have exact references at the end of this file: integer data whose
  Gram is known exactly (``exact_gram``, ``image_gram``) and the long-double inverse, with the kernels'
  Gauss-Jordan recurrences in float64 (``gauss_jordan_inverse``) as the noise measure;
* the block-packed symmetric GEMV of the large-d engines (csrc/include/sym_gemv.h) is held to the integer
  product of integer data (``symv_int_data``), exact in float64 in any order; ``symv_packed_model`` is its
  block structure in NumPy (stored blocks, direct and transposed partials, the grouped row reduction),
  with the mistakes the GPU test must catch as mutants.

This is a helper module, not a conftest: test modules import it as ``import hp_reference``.
"""
import numpy as np

# x86 long double: 64-bit mantissa. Anything narrower is no reference for float64 kernels.
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, \
    "hp_reference needs an extended-precision long double (eps %g)" % np.finfo(np.longdouble).eps

LD = np.longdouble
FACTOR = 8.0  # kernel error <= FACTOR * max(float64 noise of the recurrence, dot-product floor)


def spd_inverse(M, dtype):
    """Explicit inverse of the SPD matrix ``M`` in ``dtype``."""
    M = np.asarray(M, dtype=dtype)
    if np.dtype(dtype) == np.float64:
        return np.linalg.inv(M)
    X = np.linalg.inv(M.astype(np.float64)).astype(dtype)
    two_i = 2 * np.eye(M.shape[0], dtype=dtype)
    for _ in range(3):
        X = X @ (two_i - M @ X)
    return X


def _gram(X, y, dtype):
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    A = np.einsum("nmi,nmj->nij", X, X)
    b = np.einsum("nmi,nm->ni", X, y)
    yy = np.einsum("nm,nm->n", y, y)
    return A, b, yy


def _gram_objective(A, b, yy, th):
    half = np.asarray(0.5, dtype=th.dtype)
    tot = np.zeros((), dtype=th.dtype)
    for n in range(th.shape[0]):
        tot = tot + (half * (th[n] @ (A[n] @ th[n])) - b[n] @ th[n] + half * yy[n])
    return tot


def gadmm_linear(X, y, rho, K, dtype=LD):
    """Per-worker-dual GADMM on the identity chain (``oracle.reference.dgadmm_linear`` without
    re-chaining): heads, tails, then every worker's ``mu``. ``X`` (N, m, d), ``y`` (N, m).
    Returns ``(theta (K, N, d), mu (N, d) after iteration K, objectives (K,))``."""
    N, m, d = X.shape
    A, b, yy = _gram(X, y, dtype)
    rho = np.asarray(rho, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    deg = [(n > 0) + (n < N - 1) for n in range(N)]
    Minv = [spd_inverse(A[n] + deg[n] * rho * eye, dtype) for n in range(N)]
    th = np.zeros((N, d), dtype=dtype)
    mu = np.zeros((N, d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    for k in range(K):
        for phase in (0, 1):
            for n in range(phase, N, 2):
                r = b[n] - mu[n]
                if n > 0:
                    r = r + rho * th[n - 1]
                if n < N - 1:
                    r = r + rho * th[n + 1]
                th[n] = Minv[n] @ r
        for n in range(N):
            upd = np.zeros(d, dtype=dtype)
            if n < N - 1:
                upd = upd + rho * (th[n] - th[n + 1])
            if n > 0:
                upd = upd - rho * (th[n - 1] - th[n])
            mu[n] = mu[n] + upd
        thetas[k] = th
        obj[k] = _gram_objective(A, b, yy, th)
    return thetas, mu, obj


def chain_tables(chains):
    """What every worker is in every epoch of ``chains`` (a list of ``(first_iteration, path)``, ``path``
    position -> worker), by plain loops over the chains: a list, one entry per epoch, of
    ``(first_iteration, {worker: (position, left, right)})`` with neighbours as worker ids (None at an
    end). A worker at an even position is a head; its degree is the number of its neighbours."""
    out = []
    for first, path in chains:
        path = [int(w) for w in path]
        n = len(path)
        assert sorted(path) == list(range(n)), "a chain is a permutation of the workers"
        out.append((int(first), {w: (p, path[p - 1] if p > 0 else None, path[p + 1] if p < n - 1 else None)
                                 for p, w in enumerate(path)}))
    assert all(a[0] < b[0] for a, b in zip(out, out[1:])), "epochs start at increasing iterations"
    return out


def flush_pairs(chains):
    """Per epoch e, ``{worker: (old left, old right)}`` of the workers that were HEADS of epoch e - 1's
    chain: their dual update of the last iteration before the re-chain is still pending there and must
    be applied with these, the OLD chain's, neighbours. Epoch 0: empty."""
    tabs = chain_tables(chains)
    out = [{}]
    for (_, old), _ in zip(tabs, tabs[1:]):
        out.append({w: (l, r) for w, (p, l, r) in old.items() if p % 2 == 0})
    return out


DGADMM_MUTANTS = ("ignore", "flush-new", "old-degree")


def _dgadmm_run(X, y, rho, K, chains, dtype, mutant=None):
    """The recurrence of ``dgadmm_linear`` with the duals of EVERY iteration (K, N, d): a run to
    iteration k is a prefix of a longer one over the same chains."""
    N, m, d = X.shape
    assert mutant is None or mutant in DGADMM_MUTANTS
    if mutant == "ignore":
        chains = chains[:1]
    tabs = chain_tables(chains)
    assert tabs[0][0] == 1 and len(tabs[0][1]) == N
    A, b, yy = _gram(X, y, dtype)
    rho = np.asarray(rho, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    Minv = [{g: spd_inverse(A[n] + g * rho * eye, dtype) for g in (1, 2)} for n in range(N)]
    th = np.zeros((N, d), dtype=dtype)
    mu = np.zeros((N, d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    mus = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    e = 0
    for k in range(1, K + 1):
        first_of_epoch = e + 1 < len(tabs) and tabs[e + 1][0] == k
        if first_of_epoch:
            e += 1
        tab = tabs[e][1]
        order = sorted(tab, key=lambda w: tab[w][0])  # workers by chain position
        for phase in (0, 1):
            for w in order[phase::2]:
                _, l, r = tab[w]
                rhs = b[w] - mu[w]
                if l is not None:
                    rhs = rhs + rho * th[l]
                if r is not None:
                    rhs = rhs + rho * th[r]
                src = tabs[e - 1][1] if (mutant == "old-degree" and first_of_epoch) else tab
                deg = (src[w][1] is not None) + (src[w][2] is not None)
                th[w] = Minv[w][deg] @ rhs
        last_of_epoch = e + 1 < len(tabs) and tabs[e + 1][0] == k + 1
        for w in order:
            p, l, r = tab[w]
            if mutant == "flush-new" and last_of_epoch and p % 2 == 0:
                _, l, r = tabs[e + 1][1][w]  # a head's pending update, applied with the NEW neighbours
            upd = np.zeros(d, dtype=dtype)
            if r is not None:
                upd = upd + rho * (th[w] - th[r])
            if l is not None:
                upd = upd - rho * (th[l] - th[w])
            mu[w] = mu[w] + upd
        thetas[k - 1] = th
        mus[k - 1] = mu
        obj[k - 1] = _gram_objective(A, b, yy, th)
    return thetas, mus, obj


def dgadmm_linear(X, y, rho, K, chains, dtype=LD, mutant=None):
    """D-GADMM (``oracle.reference.dgadmm_linear``): GADMM with per-worker duals whose chain changes.
    ``chains``: a list of ``(first_iteration, path)``, ``path`` position -> worker, the first at
    iteration 1 (what ``NativeChainEngine.run_persistent(epochs=...)`` takes). Iteration k runs on the
    chain of the last epoch that started at or before k: the workers at even positions (heads), then
    the others (tails), each applying the cached inverse of ``A_n + g rho I`` for ITS degree g in
    {1, 2} on THAT chain, then every worker's ``mu`` with the neighbours of that chain (so the update of
    the last iteration before a re-chain uses the old chain). On the single epoch ``(1, identity)`` the
    operations and their order are ``gadmm_linear``'s.
    ``mutant`` names a wrong implementation (tests/test_hp_reference_cpu.py measures how far each sits
    from the reference): ``"ignore"`` never re-chains; ``"flush-new"`` applies the heads' dual update of
    the last iteration before a re-chain with the NEW chain's neighbours; ``"old-degree"`` takes, in
    the first iteration after a re-chain, the inverse of each worker's degree on the OLD chain.
    Returns ``(theta (K, N, d), mu (N, d) after iteration K, objectives (K,))``."""
    th, mus, obj = _dgadmm_run(np.asarray(X), y, rho, K, chains, dtype, mutant)
    return th, mus[-1], obj


RESIDUAL_MUTANTS = ("one-edge", "stale-head", "pre-update", "lanes-64", "old-chain", "by-position")


def _chain_at(tabs, it):
    """The table of the chain in force at iteration ``it`` (1-based) of ``chain_tables`` output."""
    e = 0
    while e + 1 < len(tabs) and tabs[e + 1][0] <= it:
        e += 1
    return tabs[e][1]


def tail_mask(chains, K, N):
    """(K, N) bool: worker w is a tail (odd 0-based chain position) of the chain in force at iteration
    k + 1. ``chains`` None: the identity chain."""
    tabs = chain_tables([(1, list(range(N)))] if chains is None else chains)
    mask = np.zeros((K, N), dtype=bool)
    for it in range(1, K + 1):
        for w, (p, _, _) in _chain_at(tabs, it).items():
            mask[it - 1, w] = p % 2 == 1
    return mask


def chain_residual(theta_hist, chains=None, dtype=LD, mutant=None):
    """The K4 primal residual the chain kernels emit beside theta, the duals and the objective, from a
    theta history (K, N, d): entry ``[it - 1, w]`` of a worker w that is a TAIL (odd 0-based position) of
    the chain in force at iteration ``it`` is

        sum((th[it, left] - th[it, w])^2) + sum((th[it, w] - th[it, right])^2)

    over the edges it has (every chain edge has exactly one tail end), all thetas those after iteration
    ``it``; a head's entry is 0. Indexed by worker id; ``chains`` as ``dgadmm_linear`` takes them (None:
    the identity chain). Plain NumPy in ``dtype``.
    ``mutant`` names a mistake a kernel's residual branch could make (tests/test_hp_reference_cpu.py
    measures how far each sits from the reference): ``"one-edge"`` drops the right edge; ``"stale-head"``
    reads the heads' theta of iteration ``it - 1`` (0 before the first); ``"pre-update"`` the tail's own
    theta of ``it - 1``; ``"lanes-64"`` sums the coordinates < 64 only; ``"old-chain"`` takes the chain
    of ``it - 1``; ``"by-position"`` writes a tail's entry at its chain position instead of its id."""
    assert mutant is None or mutant in RESIDUAL_MUTANTS
    th = np.asarray(theta_hist, dtype=dtype)
    K, N, d = th.shape
    tabs = chain_tables([(1, list(range(N)))] if chains is None else chains)
    assert len(tabs[0][1]) == N and tabs[0][0] == 1
    out = np.zeros((K, N), dtype=dtype)
    start = np.zeros((N, d), dtype=dtype)
    cols = slice(0, 64) if mutant == "lanes-64" else slice(None)
    for it in range(1, K + 1):
        tab = _chain_at(tabs, max(it - 1, 1) if mutant == "old-chain" else it)
        cur = th[it - 1]
        prev = th[it - 2] if it > 1 else start
        nbr = prev if mutant == "stale-head" else cur
        for w, (p, l, r) in tab.items():
            if p % 2 == 0:
                continue
            own = prev[w] if mutant == "pre-update" else cur[w]
            tot = np.zeros((), dtype=dtype)
            if l is not None:
                tot = tot + np.sum(((nbr[l] - own)[cols]) ** 2)
            if r is not None and mutant != "one-edge":
                tot = tot + np.sum(((own - nbr[r])[cols]) ** 2)
            out[it - 1, p if mutant == "by-position" else w] = tot
    return out


def star_admm_linear(X, y, rho, K, dtype=LD):
    """Star ADMM, the hub is worker N - 1 and holds a shard (``oracle.reference.std_admm_linear``).
    Returns ``(theta (K, N, d), lam (N, d) after iteration K (the hub's row stays 0), objectives)``."""
    N, m, d = X.shape
    A, b, yy = _gram(X, y, dtype)
    rho = np.asarray(rho, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    hub = N - 1
    Minv = [spd_inverse(A[n] + (rho if n != hub else (N - 1) * rho) * eye, dtype) for n in range(N)]
    th = np.zeros((N, d), dtype=dtype)
    lam = np.zeros((N, d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    for k in range(K):
        for n in range(hub):
            th[n] = Minv[n] @ (b[n] - lam[n] + rho * th[hub])
        c1 = np.zeros(d, dtype=dtype)
        s1 = np.zeros(d, dtype=dtype)
        for n in range(hub):
            c1 = c1 + lam[n]
            s1 = s1 + th[n]
        th[hub] = Minv[hub] @ (b[hub] + c1 + rho * s1)
        for n in range(hub):
            lam[n] = lam[n] + rho * (th[n] - th[hub])
        thetas[k] = th
        obj[k] = _gram_objective(A, b, yy, th)
    return thetas, lam, obj


def gadmm_logistic_gd(X, y, rho, lam, step, K, max_inner, inner_tol, dtype=LD):
    """GADMM logistic regression with the inexact inner gradient descent
    (``oracle.reference.gadmm_logistic_gd`` / ``logreg_gd``): the prox terms are frozen at the
    pre-update iterate, an inner solve takes at most ``max_inner`` steps and stops after the first
    step with all ``|dx| < inner_tol`` (strict). Returns ``(theta (K, N, d), mu (N, d) per-worker
    duals after iteration K, objectives (K,), inner step counts (K, N), margin)``; ``margin`` is the
    smallest relative distance ``|max|dx| / inner_tol - 1|`` of any stop test from its threshold
    (inf when ``inner_tol`` is 0: no test can pass)."""
    N, m, d = X.shape
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    rho, lam, step, tol = (np.asarray(v, dtype=dtype) for v in (rho, lam, step, inner_tol))
    one = np.asarray(1.0, dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    th = np.zeros((N, d), dtype=dtype)
    dual = np.zeros((N, d), dtype=dtype)  # edge duals; row N - 1 stays 0
    thetas = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    inner = np.zeros((K, N), dtype=np.int64)
    margin = [np.inf]
    z = np.zeros(d, dtype=dtype)

    def update(n, k):
        c1 = dual[n - 1] if n > 0 else z
        t1 = rho * (th[n] - th[n - 1]) if n > 0 else z
        c2 = dual[n] if n < N - 1 else z
        t2 = rho * (th[n] - th[n + 1]) if n < N - 1 else z
        H, Y = X[n], y[n]
        x = th[n].copy()
        steps = 0
        for _ in range(int(max_inner)):
            g = -(H.T @ (Y / (one + np.exp(Y * (H @ x))))) + lam * x - c1 + c2 + t1 + t2
            x_new = x - step * g
            dx = np.max(np.abs(x_new - x))
            x = x_new
            steps += 1
            if tol > 0:
                margin[0] = min(margin[0], float(abs(dx / tol - one)))
            if dx < tol:
                break
        th[n] = x
        inner[k, n] = steps

    for k in range(K):
        for n in range(0, N, 2):
            update(n, k)
        for n in range(1, N, 2):
            update(n, k)
        for n in range(N - 1):
            dual[n] = dual[n] + rho * (th[n] - th[n + 1])
        thetas[k] = th
        tot = np.zeros((), dtype=dtype)
        for n in range(N):
            tot = tot + (lam * half * (th[n] @ th[n]) + np.sum(np.log1p(np.exp(-y[n] * (X[n] @ th[n])))))
        obj[k] = tot
    mu = dual.copy()
    mu[1:] = mu[1:] - dual[:-1]
    return thetas, mu, obj, inner, margin[0]


NEWTON_MAX = 50      # step cap of a local Newton solve (chain_newton.hip NEWTON_MAX, newton_prox iters)
NEWTON_TOL = 1e-13   # the kernels' stop tolerance (NEWTON_TOL / NTOL)
NEWTON_TOL_LD = 1e-17  # the long-double reference's: the converged prox


def _newton_run(X, y, rho, lam, K, dtype, tol, chord):
    """The recurrence of ``gadmm_logistic_newton`` with the duals of EVERY iteration (K, N, d): a run
    to iteration k is a prefix of a longer one, so one run serves every ``k <= K``."""
    N, m, d = X.shape
    if chord > 0 and np.dtype(dtype) != np.float64:
        raise ValueError("the chord rule is the float64 kernels': dtype=float64 only")
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    rho, lam, tol = (np.asarray(v, dtype=dtype) for v in (rho, lam, tol))
    one = np.asarray(1.0, dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    th = np.zeros((N, d), dtype=dtype)
    mu = np.zeros((N, d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    mus = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    steps = np.zeros((K, N), dtype=np.int64)
    cache = [None] * N  # chord > 0: the inverse of the worker's last refresh, kept across iterations

    def solve(n, k):
        deg = (n > 0) + (n < N - 1)
        shift = lam + deg * rho
        c = mu[n].copy()
        if n > 0:
            c = c - rho * th[n - 1]
        if n < N - 1:
            c = c - rho * th[n + 1]
        A, Y = X[n], y[n]
        x = th[n].copy()
        Hinv = cache[n] if chord > 0 else None
        refresh = Hinv is None
        prev = None
        for s in range(NEWTON_MAX):
            p = one / (one + np.exp(Y * (A @ x)))  # sigma(-y z)
            g = -(A.T @ (Y * p)) + shift * x + c
            if refresh:
                Hinv = spd_inverse((A.T * (p * (one - p))) @ A + shift * eye, dtype)
                if chord > 0:
                    cache[n] = Hinv
            dx = Hinv @ g
            x = x - dx
            mdx = np.max(np.abs(dx))
            steps[k, n] = s + 1
            if mdx < tol * max(one, np.max(np.abs(x))):
                break
            # chord steps reuse the inverse while they contract by at least `chord` per step; the step
            # after a refresh is always a chord step (as the kernel: its contraction is not tested)
            refresh = bool(chord <= 0 or (not refresh and prev is not None and mdx > chord * prev))
            prev = mdx
        th[n] = x

    for k in range(K):
        for phase in (0, 1):
            for n in range(phase, N, 2):
                solve(n, k)
        for n in range(N):
            upd = np.zeros(d, dtype=dtype)
            if n < N - 1:
                upd = upd + rho * (th[n] - th[n + 1])
            if n > 0:
                upd = upd - rho * (th[n - 1] - th[n])
            mu[n] = mu[n] + upd
        thetas[k] = th
        mus[k] = mu
        tot = np.zeros((), dtype=dtype)
        for n in range(N):
            tot = tot + (lam * half * (th[n] @ th[n]) + np.sum(np.log1p(np.exp(-y[n] * (X[n] @ th[n])))))
        obj[k] = tot
    return thetas, mus, obj, steps


def gadmm_logistic_newton(X, y, rho, lam, K, dtype=LD, tol=NEWTON_TOL_LD, chord=0.0):
    """GADMM logistic regression with EXACT local solves (header of csrc/kernels/chain_newton.hip;
    the stop rule of models/logistic.py:newton_prox): heads, tails, then every worker's ``mu``. Worker n
    minimises ``f_n(x) + mu_n'x + rho/2 sum_nbr |x - th_nbr|^2`` by Newton steps

        g = -X'(y . sigma(-y . Xx)) + (lam + deg rho) x + mu - rho (th_l + th_r)
        H = X' diag(w) X + (lam + deg rho) I,  w = sigma (1 - sigma);   dx = H^-1 g;   x <- x - dx

    from its own last iterate, at most 50 of them, and stops after the first step with
    ``max|dx| < tol * max(1, max|x|)`` (strict). ``H^-1`` is ``spd_inverse``'s explicit inverse.
    ``chord = c > 0`` (float64 only) is the kernels' chord rule: a worker keeps the inverse of its last
    refresh across iterations, and a step refreshes only when none is cached or when the previous
    step, itself a chord step, contracted by less than c (``|dx_k| > c |dx_{k-1}|``); the stop rule
    and the fixed point are unchanged.
    Returns ``(theta (K, N, d), mu (N, d) per-worker duals after iteration K, objectives (K,),
    Newton step counts (K, N))``."""
    th, mus, obj, steps = _newton_run(np.asarray(X), y, rho, lam, K, dtype, tol, chord)
    return th, mus[-1], obj, steps


def edge_to_worker_duals(lam_edge):
    """Per-worker aggregate ``mu_n = lam_n - lam_{n-1}`` of edge duals (N, d) whose last row is 0."""
    mu = np.array(lam_edge, copy=True)
    mu[1:] = mu[1:] - lam_edge[:-1]
    return mu


def make_linear(n, m, d, seed):
    """Gaussian shards with noise-dominated labels ``y = X th* + N(0, 1)``, ``|th*| = 1``: the final
    objective stays a fixed fraction of ``1/2 y'y``, so the Gram-form objective does not cancel and a
    relative tolerance means something. Returns ``(X (n, m, d), y (n, m), rho = 0.5 m)``."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m, d))
    ts = rng.standard_normal(d)
    ts = ts / np.linalg.norm(ts)
    y = X @ ts + rng.standard_normal((n, m))
    return X, y, 0.5 * m


def make_logistic(n, m, d, seed):
    """Gaussian shards ``/ sqrt(d)``, labels +-1. Returns ``(X, y, rho, lam, step)`` with
    ``lam = 1e-3``, ``step = 1 / max_n(lambda_max(X_n'X_n) / 4 + lam)`` and ``rho = 0.1 / step``."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m, d)) / np.sqrt(d)
    y = np.where(rng.standard_normal((n, m)) > 0, 1.0, -1.0)
    lam = 1e-3
    L = max(0.25 * float(np.linalg.eigvalsh(X[i].T @ X[i])[-1]) + lam for i in range(n))
    step = 1.0 / L
    return X, y, 0.1 / step, lam, step


def noise_level(ref_ld, ref_f64, scale):
    """Largest absolute difference of two runs, divided by ``scale`` (a scalar, or per value)."""
    diff = np.abs(np.asarray(ref_ld, dtype=LD) - np.asarray(ref_f64, dtype=LD)) / np.asarray(scale, dtype=LD)
    return float(np.max(diff)) if diff.size else 0.0


def _own_or_largest(ref):
    """The scale of a trace that decays over many orders: each entry's own magnitude where that exceeds
    1e-20 of the trace's largest, the largest elsewhere (as ``QReference.res_scale``)."""
    mag = np.abs(np.asarray(ref, dtype=LD))
    top = np.max(mag) if mag.size else np.asarray(0.0, dtype=LD)
    return np.where(mag > 1e-20 * top, mag, top)


def bound(e64, d, m_logistic=0, truncation=0.0, n=0):
    """``FACTOR * max(e64, max(d, m_logistic, n, 16) * 2^-53, truncation)``: the float64 noise of the
    recurrence, with the standard dot-product bound as the floor for runs that happen to round luckily.
    ``truncation``: what a stop rule of the kernel admits beyond rounding (``chord_truncation``); ``n``:
    the worker count where a step sums n rows (the first-order server step), 0 elsewhere."""
    return FACTOR * max(float(e64), max(int(d), int(m_logistic), int(n), 16) * 2.0 ** -53, float(truncation))


def chord_truncation(chord, scale_theta):
    """``tau(c) / max|theta|``, ``tau(c) = c / (1 - c) NEWTON_TOL max(1, max|x|)``: a chord-accepted last
    step contracted by at most c, so the iterate it leaves can sit that far from the prox (the
    geometric tail ``sum_{j >= 1} c^j`` of a step below the stop threshold). 0 at ``chord = 0``: exact
    Newton converges quadratically and its stop rule leaves nothing above rounding."""
    if chord <= 0:
        return 0.0
    return chord / (1.0 - chord) * NEWTON_TOL * max(1.0, scale_theta) / scale_theta


class Reference:
    """A case's long-double run, the float64 noise of the same recurrence, and the bounds from them.

    ``theta`` (K, N, d), ``dual`` (N, d), ``obj`` (K,) in long double; ``rho``; ``scale_theta`` =
    max |theta| over the run; ``b_theta`` / ``b_dual`` / ``b_obj``: the bounds of the three relative
    errors ``err_theta`` / ``err_dual`` / ``err_obj`` measure.

    Chain references (``residual=True``; ``f64[0]`` is then the float64 theta history (K, N, d)) also hold
    the K4 primal residual of the long-double history over ``chains`` (``chain_residual``): ``res_w``
    (K, N) per worker, ``res`` (K,) its row sums, ``tails`` (K, N) which entries are tails'. Their noise
    ``e_res_w`` / ``e_res`` is the distance of the same function of the float64 history, in float64; each
    entry is taken over its own reference value where that exceeds 1e-20 of the trace's largest, over
    the largest below that, and of ``res_w`` the tails' entries only (a head's is exactly 0). Bounds
    ``b_res_w`` / ``b_res`` and errors ``err_res_w`` / ``err_res`` as for the other quantities."""

    def __init__(self, ld, f64, rho, d, m_logistic=0, chord=0.0, chains=None, residual=True):
        self.theta, self.dual, self.obj = ld[0], ld[1], ld[2]
        self.extra = ld[3:]
        self.rho = float(rho)
        self.scale_theta = float(np.max(np.abs(self.theta)))
        self.e_theta = noise_level(self.theta, f64[0], self.scale_theta)
        self.e_dual = noise_level(self.dual, f64[1], self.rho * self.scale_theta)
        self.e_obj = noise_level(self.obj, f64[2], np.abs(self.obj))
        self.truncation = chord_truncation(chord, self.scale_theta)  # Newton cases with a chord rule only
        self.b_theta = bound(self.e_theta, d, m_logistic, self.truncation)
        self.b_dual = bound(self.e_dual, d, m_logistic, self.truncation)
        self.b_obj = bound(self.e_obj, d, m_logistic, self.truncation)
        if residual:
            K, N = self.theta.shape[:2]
            self.chains = chains
            self.theta64 = f64[0]  # the float64 history: what the residual's power is measured on
            self.tails = tail_mask(chains, K, N)
            self.res_w = chain_residual(self.theta, chains, LD)
            self.res = self.res_w.sum(axis=1)
            res64 = chain_residual(np.asarray(f64[0], dtype=np.float64), chains, np.float64)
            self.res_w_scale, self.res_scale = _own_or_largest(self.res_w), _own_or_largest(self.res)
            self.e_res_w = self._tails_level(self.res_w, res64)
            self.e_res = noise_level(self.res, res64.sum(axis=1), self.res_scale)
            self.b_res_w, self.b_res = bound(self.e_res_w, d, m_logistic), bound(self.e_res, d, m_logistic)
            _freeze(self.tails, self.res_w, self.res, self.res_w_scale, self.res_scale)

    def _tails_level(self, ref, rows):
        k = len(rows)
        diff = np.abs(ref[:k] - np.asarray(rows, dtype=LD)) / self.res_w_scale[:k]
        diff = diff[self.tails[:k]]
        return float(np.max(diff)) if diff.size else 0.0

    def err_res_w(self, rows):
        """``rows`` (k, N), the per-worker residual of iterations 1..k, against the reference's first k
        rows: the tails' entries only."""
        return self._tails_level(self.res_w, rows)

    def err_res(self, res):
        res = np.asarray(res)
        return noise_level(self.res[:len(res)], res, self.res_scale[:len(res)])

    def err_theta(self, theta, k=None):
        """``theta`` (N, d) against the reference after iteration ``k`` (1-based; None: the last)."""
        ref = self.theta[-1 if k is None else k - 1]
        return noise_level(ref, theta, self.scale_theta)

    def err_dual(self, dual, ref=None):
        return noise_level(self.dual if ref is None else ref, dual, self.rho * self.scale_theta)

    def err_obj(self, obj):
        obj = np.asarray(obj)
        return noise_level(self.obj[:len(obj)], obj, np.abs(self.obj[:len(obj)]))


# ------------------------------------------------------------------------------------------------
# The shapes of tests/test_gpu_dispatch_classes.py (why each is there is written next to the
# parameter lists of that file) and their references, built once per process and shared.
K_ITERS = 20
MAX_INNER = 6

LINEAR_SHAPES = [(2, 3, 1), (3, 7, 3), (5, 40, 32), (4, 40, 33), (5, 60, 52), (5, 70, 53), (4, 40, 64),
                 (3, 80, 65), (4, 150, 128), (3, 150, 129), (3, 280, 256), (3, 280, 257)]
LOGISTIC_SHAPES = [(3, 5, 3), (4, 30, 20), (3, 40, 52), (3, 52, 20), (3, 40, 53), (3, 64, 64), (3, 100, 20),
                   (2, 60, 128), (3, 200, 30), (3, 250, 40), (3, 100, 100)]
STAR_SHAPES = [(3, 7, 3), (4, 60, 52), (4, 70, 53), (3, 40, 64), (2, 8, 6), (5, 8, 6), (26, 60, 53),
               (3, 80, 65), (2, 70, 66), (4, 80, 65), (4, 150, 128), (3, 150, 129), (3, 280, 256), (3, 280, 257)]
assert all(n - 1 < max(d, 16) for n, _, d in STAR_SHAPES)  # the hub's sum of n - 1 rows is under the floor's size
LIVE_STOP = ((4, 30, 20), 1e-3)  # the one logistic case with a live inner stop rule

_CACHE = {}


def seed_of(n, m, d):
    return 1000003 * n + 1009 * m + d


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _freeze(*arrs):
    for a in arrs:
        a.setflags(write=False)


def linear_case(n, m, d, K=K_ITERS):
    """``(X, y, rho, Reference)`` of ``gadmm_linear`` on ``make_linear(n, m, d, seed_of(n, m, d))``."""
    def build():
        X, y, rho = make_linear(n, m, d, seed_of(n, m, d))
        _freeze(X, y)
        return X, y, rho, Reference(gadmm_linear(X, y, rho, K, LD), gadmm_linear(X, y, rho, K, np.float64), rho, d)
    return _cached(("lin", n, m, d, K), build)


RESIDUAL_PATHS = {(4, 40, 33): (3, 2, 1, 0), (5, 40, 33): (2, 0, 4, 1, 3)}  # the permuted static chains


def linear_path_case(n, m, d, path, K=K_ITERS):
    """``(X, y, rho, Reference)`` of GADMM on the static chain ``path`` (position -> worker) over the
    data of ``linear_case``: ``gadmm_linear`` on the shards in chain order (``X[path]``, ``y[path]``), its
    theta history and duals mapped back to worker ids, and the K4 residual over that chain."""
    path = [int(w) for w in path]
    assert sorted(path) == list(range(n))

    def build():
        X, y, rho = make_linear(n, m, d, seed_of(n, m, d))
        _freeze(X, y)

        def run(dtype):
            th_p, mu_p, obj = gadmm_linear(X[path], y[path], rho, K, dtype)
            th, mu = np.zeros_like(th_p), np.zeros_like(mu_p)
            th[:, path] = th_p
            mu[path] = mu_p
            return th, mu, obj
        return X, y, rho, Reference(run(LD), run(np.float64), rho, d, chains=[(1, path)])
    return _cached(("lin-path", n, m, d, tuple(path), K), build)


def star_case(n, m, d, K=K_ITERS):
    """As ``linear_case`` for ``star_admm_linear`` (the same data). The size behind the dot-product floor
    of the bounds is d, although the hub's right-hand side sums n - 1 rows: at every shape of
    ``STAR_SHAPES`` n - 1 < max(d, 16), so the longer sum would not move a bound there, and at n = 66,
    d = 6 (tests/test_gpu_stop_rule.py) it would only widen one that the kernel meets as it is."""
    def build():
        X, y, rho = make_linear(n, m, d, seed_of(n, m, d))
        _freeze(X, y)
        return X, y, rho, Reference(star_admm_linear(X, y, rho, K, LD), star_admm_linear(X, y, rho, K, np.float64),
                                    rho, d, residual=False)
    return _cached(("star", n, m, d, K), build)


def logistic_case(n, m, d, K=K_ITERS, max_inner=MAX_INNER, inner_tol=0.0):
    """``(X, y, rho, lam, step, Reference)`` of ``gadmm_logistic_gd``; ``Reference.extra`` holds the
    inner step counts (K, N) and the decision margin."""
    def build():
        X, y, rho, lam, step = make_logistic(n, m, d, seed_of(n, m, d))
        _freeze(X, y)
        ld = gadmm_logistic_gd(X, y, rho, lam, step, K, max_inner, inner_tol, LD)
        f64 = gadmm_logistic_gd(X, y, rho, lam, step, K, max_inner, inner_tol, np.float64)
        return X, y, rho, lam, step, Reference(ld, f64, rho, d, m)
    return _cached(("log", n, m, d, K, max_inner, inner_tol), build)


# The shapes of tests/test_gpu_newton_classes.py (the edge each one sits on is written there).
NEWTON_GRAPH_SHAPES = [(2, 1, 1), (3, 5, 3), (3, 7, 5), (4, 17, 16), (3, 15, 17), (5, 36, 34), (3, 52, 52),
                       (3, 40, 53), (3, 53, 40), (4, 7, 61), (2, 3, 64), (3, 63, 63), (3, 64, 64)]
NEWTON_PERSISTENT_SHAPES = [(2, 1, 1), (3, 5, 3), (3, 7, 5), (4, 17, 16), (3, 15, 17), (5, 36, 34), (4, 12, 49),
                            (3, 40, 52), (3, 52, 20), (3, 52, 52)]
NEWTON_SHAPES = NEWTON_GRAPH_SHAPES + [s for s in NEWTON_PERSISTENT_SHAPES if s not in NEWTON_GRAPH_SHAPES]
NEWTON_CHORDS = (0.0, 0.02, 0.3)  # exact Newton, the graph engine's default, the persistent kernels'
PERSISTENT_OVERRUN = 16           # a persistent kernel stops at most this many iterations past K


def _newton_history(n, m, d, K, dtype, tol, chord):
    """One run of the recurrence per (case, arithmetic), long enough for every iteration count the
    tests ask for: K_ITERS for the graph engine and the CPU tests, up to PERSISTENT_OVERRUN more for
    the iteration a persistent kernel happens to stop at."""
    run = K_ITERS if K <= K_ITERS else max(K, K_ITERS + PERSISTENT_OVERRUN)

    def build():
        X, y, rho, lam, _ = make_logistic(n, m, d, seed_of(n, m, d))
        out = _newton_run(X, y, rho, lam, run, dtype, tol, chord)
        _freeze(X, y, *out)
        return (X, y, rho, lam) + out
    return _cached(("newton-run", n, m, d, run, np.dtype(dtype).name, tol, chord), build)


def newton_case(n, m, d, K=K_ITERS, chord=0.0):
    """The ``Reference`` of ``gadmm_logistic_newton`` on ``make_logistic(n, m, d, seed_of(n, m, d))``
    (the data of ``logistic_case``; ``step`` is not used). The reference is the long-double run with
    ``tol = 1e-17`` and no chord rule, the converged prox; its noise ``e_*`` is the distance of the
    float64 run with the kernels' ``tol = 1e-13`` and the chord threshold ``chord`` (e64 at 0, e_chord
    above), and at ``chord > 0`` the bounds also admit ``chord_truncation``. Beside the fields of
    ``Reference``: ``X``, ``y``, ``lam``, ``chord``; ``extra[0]`` the long-double run's Newton step
    counts (K, N) and ``steps64`` the float64 run's."""
    def build():
        X, y, rho, lam, th, mus, obj, steps = _newton_history(n, m, d, K, LD, NEWTON_TOL_LD, 0.0)
        _, _, _, _, th64, mus64, obj64, steps64 = _newton_history(n, m, d, K, np.float64, NEWTON_TOL, float(chord))
        ref = Reference((th[:K], mus[K - 1], obj[:K], steps[:K]), (th64[:K], mus64[K - 1], obj64[:K]), rho, d, m,
                        chord=float(chord))
        ref.X, ref.y, ref.lam, ref.chord, ref.steps64 = X, y, lam, float(chord), steps64[:K]
        return ref
    return _cached(("newton", n, m, d, K, float(chord)), build)


# ------------------------------------------------------------------------------------------------
# First-order baselines (tests/test_gpu_first_order_classes.py): GD, DGD, LAG-PS, LAG-WK, IAG and dual
# averaging as gadmm_amd/algorithms/baselines.py and dual_averaging.py run them (the torch path, which
# follows GD_DGD_LAG.m and dual_averaging.m), every operation in ``dtype``.
FO_K = 80  # > ring + 3 = 67 IAG table slots and > 64 objective-ring slots; LAG decides from iteration 11
FO_ALGS = ("GD", "DGD", "LAG-PS", "LAG-WK", "cIAG", "R-IAG", "DualAvg", "DualAvg-J")
FO_TRIGGERSLOT = 10


def _fo_eval(kind, X, y, lam, dtype):
    """``ev(TH) -> (f (N,), g (N, d))``: every worker's objective and gradient at its row of ``TH``.
    Linear: the Gram form, Gram formed in ``dtype``; logistic: softplus / sigmoid on the shard."""
    half = np.asarray(0.5, dtype=dtype)
    if kind == "linear":
        A, b, yy = _gram(X, y, dtype)

        def ev(TH):
            At = np.einsum("nij,nj->ni", A, TH)
            return half * np.sum(At * TH, axis=1) - np.sum(b * TH, axis=1) + half * yy, At - b
        return ev
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    lam = np.asarray(lam, dtype=dtype)
    one = np.asarray(1.0, dtype=dtype)

    def ev(TH):
        z = np.einsum("nmd,nd->nm", X, TH)
        f = np.sum(np.log1p(np.exp(-y * z)), axis=1) + lam * half * np.sum(TH * TH, axis=1)
        return f, -np.einsum("nmd,nm->nd", X, y / (one + np.exp(y * z))) + lam * TH
    return ev


def first_order(alg, X, y, K, step, kind="linear", lam=0.0, thrd=0.0, hsq=None, sched=None, jacobi=False,
                faithful=True, dtype=LD, scale_history=None, ev=None):
    """``K`` iterations of ``alg`` in GD, DGD, LAG-PS, LAG-WK, IAG, DualAvg from theta = 0. ``step`` is
    the step the update applies (what ``engine.run`` takes: alpha, alpha / 100 for DGD, alpha / N for
    IAG); ``thrd`` / ``hsq`` LAG's threshold factor and Hmax_n^2; ``sched`` IAG's refreshing worker per
    iteration. The quirks of the torch path: the server table (and DGD's gradients when ``faithful``)
    start as ones; ``faithful`` GD's first step is ones (linear) or worker 0's gradient (logistic);
    ``faithful`` LAG-PS refreshes worker 0 every iteration > 1 without counting an upload; LAG decides
    nothing before iteration 11. ``scale_history = (it, c)`` multiplies LAG's recorded
    ``|theta^it - theta^{it-1}|^2`` by c (a wrong entry of the kernels' step ring). ``ev``: a prebuilt
    ``_fo_eval`` of the same data and dtype.
    Returns a dict: ``obj`` (K,), ``theta`` after iteration K ((d,) server algorithms, (N, d) DGD and
    dual averaging), ``scale`` = max |theta| over the run, and for LAG ``cnt`` (K,) uploads per
    iteration, ``mask`` (K, N), ``margin`` = the smallest ``|lhs - rhs| / max(|lhs|, |rhs|)`` of any
    trigger decision (0 / 0 skipped)."""
    N, m, d = np.shape(X)
    if ev is None:
        ev = _fo_eval(kind, X, y, lam, dtype)
    step = np.asarray(step, dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    out = {"obj": obj}
    scale = 0.0
    ones_t = np.ones((N, d), dtype=dtype)

    def rows(theta):
        return np.broadcast_to(theta, (N, d))

    if alg == "GD":
        theta = np.zeros(d, dtype=dtype)
        for it in range(1, K + 1):
            f, G = ev(rows(theta))
            if it == 1 and faithful:
                g = np.ones(d, dtype=dtype) if kind == "linear" else G[0]
            else:
                g = np.sum(G, axis=0)
            obj[it - 1] = np.sum(f)
            theta = theta - step * g
            scale = max(scale, float(np.max(np.abs(theta))))
    elif alg == "DGD":
        theta = np.zeros((N, d), dtype=dtype)
        G = ones_t.copy() if faithful else np.zeros((N, d), dtype=dtype)
        half, third = np.asarray(0.5, dtype=dtype), np.asarray(1.0, dtype=dtype) / np.asarray(3.0, dtype=dtype)
        for it in range(1, K + 1):
            f, g = ev(theta)
            if it > 1 or not faithful:
                G = g
            obj[it - 1] = np.sum(f)
            new = np.empty_like(theta)
            for w in range(N):
                if N == 1:
                    new[w] = theta[w] - step * G[w]
                elif w == 0:
                    new[w] = theta[w] - half * step * (G[w] + G[w + 1])
                elif w == N - 1:
                    new[w] = theta[w] - half * step * (G[w] + G[w - 1])
                else:
                    new[w] = theta[w] - third * step * (G[w] + G[w + 1] + G[w - 1])
            theta = new
            scale = max(scale, float(np.max(np.abs(theta))))
    elif alg in ("LAG-PS", "LAG-WK"):
        ps = alg == "LAG-PS"
        thrd = np.asarray(thrd, dtype=dtype)
        hloc = np.asarray(hsq, dtype=dtype)
        table, G = ones_t.copy(), ones_t.copy()
        theta_hat = np.zeros((N, d), dtype=dtype)
        theta = np.zeros(d, dtype=dtype)
        dl = {}  # |theta^k - theta^{k-1}|^2, k = 1 .. (the kernels' ring of the last ten)
        cnt = np.zeros((K,), dtype=np.float64)
        masks = np.zeros((K, N), dtype=bool)
        margin = np.inf
        for it in range(1, K + 1):
            f, g = ev(rows(theta))
            mask = np.zeros(N, dtype=bool)
            if it > FO_TRIGGERSLOT:
                trig = np.zeros((), dtype=dtype)
                for k in range(1, FO_TRIGGERSLOT + 1):
                    trig = trig + dl[it - k]
                lhs = hloc * np.sum((theta_hat - theta) ** 2, axis=1) if ps else np.sum((g - G) ** 2, axis=1)
                rhs = thrd * trig
                mask = lhs > rhs
                big = np.maximum(np.abs(lhs), np.abs(rhs))
                live = big > 0
                if np.any(live):
                    margin = min(margin, float(np.min(np.abs(lhs - rhs)[live] / big[live])))
            G[mask] = g[mask]
            if ps:
                theta_hat[mask] = theta
            upd = mask.copy()
            if ps and faithful and it > 1:  # the forced refresh of worker 0: no upload counted
                G[0] = g[0]
                upd[0] = True
            table[upd] = G[upd]
            cnt[it - 1] = int(mask.sum())
            masks[it - 1] = mask
            obj[it - 1] = np.sum(f)
            new = theta - step * np.sum(table, axis=0)
            dl[it] = np.sum((new - theta) ** 2)
            if scale_history is not None and scale_history[0] == it:
                dl[it] = dl[it] * np.asarray(scale_history[1], dtype=dtype)
            theta = new
            scale = max(scale, float(np.max(np.abs(theta))))
        out.update(cnt=cnt, mask=masks, margin=margin)
    elif alg == "IAG":
        table = ones_t.copy()
        theta = np.zeros(d, dtype=dtype)
        for it in range(1, K + 1):
            f, g = ev(rows(theta))
            w = int(sched[it - 1])
            if it > 1:
                table[w] = g[w]
            obj[it - 1] = np.sum(f)
            theta = theta - step * np.sum(table, axis=0)
            scale = max(scale, float(np.max(np.abs(theta))))
    elif alg == "DualAvg":
        theta = np.zeros((N, d), dtype=dtype)
        Z = np.zeros((N, d), dtype=dtype)
        half = np.asarray(0.5, dtype=dtype)
        for it in range(1, K + 1):
            _, g = ev(theta)
            Zp = Z.copy()
            for w in range(N):
                left = None if w == 0 else (Zp[w - 1] if jacobi else Z[w - 1])
                right = None if w == N - 1 else Zp[w + 1]
                if left is None and right is None:
                    zn = g[w].copy()
                elif left is None:
                    zn = right + g[w]
                elif right is None:
                    zn = left + g[w]
                else:
                    zn = half * right + half * left + g[w]
                Z[w] = zn
            theta = -step * Z
            obj[it - 1] = np.sum(ev(theta)[0])
            scale = max(scale, float(np.max(np.abs(theta))))
    else:
        raise ValueError("first_order: unknown algorithm %r" % (alg,))
    out.update(theta=theta, scale=scale)
    return out


def fo_constants(kind, X, y, lam):
    """The scalar inputs of a first-order run, once, in float64 (``baselines.global_constants`` /
    ``model.hmax``): ``(step = 1 / Hmax_all, hmax (N,))``. The very same values go to the reference and
    to the engines, which take them as arguments: no eigenvalue solver stands between the two."""
    G = np.einsum("nmi,nmj->nij", X, X)
    ev_all = float(np.linalg.eigvalsh(G.sum(0))[-1])
    ev_loc = np.array([float(np.linalg.eigvalsh(G[i])[-1]) for i in range(G.shape[0])])
    if kind == "linear":
        return 1.0 / ev_all, ev_loc
    return 1.0 / (0.25 * ev_all + lam), 0.25 * np.abs(ev_loc) + lam


def fo_run_args(alg, n, K, step, hmax):
    """``(engine algorithm, keyword arguments)`` of variant ``alg`` (one of ``FO_ALGS``) for both
    ``first_order`` and ``engine.run``: the step as the update applies it, LAG's ``thrd`` (as
    ``baselines.lag``) and ``hsq``, IAG's schedule (``baselines.iag_schedule``, seed 7), ``jacobi``."""
    if alg == "GD":
        return "GD", {"step": step}
    if alg == "DGD":
        return "DGD", {"step": step / 100.0}
    if alg in ("LAG-PS", "LAG-WK"):
        thrd = (10.0 if alg == "LAG-PS" else 1.0) / (step ** 2 * n ** 2) / FO_TRIGGERSLOT
        return alg, {"step": step, "thrd": thrd, "hsq": hmax ** 2}
    if alg in ("cIAG", "R-IAG"):
        import torch
        from gadmm_amd.algorithms.baselines import iag_schedule
        sched = iag_schedule(n, K, "cyclic" if alg == "cIAG" else "random", torch.from_numpy(np.array(hmax)), 7)
        return "IAG", {"step": step / n, "sched": sched}
    if alg in ("DualAvg", "DualAvg-J"):
        return "DualAvg", {"step": step, "jacobi": alg == "DualAvg-J"}
    raise ValueError(alg)


def _fo_data(kind, n, m, d, seed_offset):
    """Data, constants and the two ``_fo_eval`` closures of a shape, shared by its eight algorithms."""
    def build():
        seed = seed_of(n, m, d) + seed_offset
        if kind == "linear":
            X, y, _ = make_linear(n, m, d, seed)
            lam = 0.0
        else:
            X, y, _, lam, _ = make_logistic(n, m, d, seed)
        _freeze(X, y)
        step, hmax = fo_constants(kind, X, y, lam)
        _freeze(hmax)
        return X, y, lam, step, hmax, _fo_eval(kind, X, y, lam, LD), _fo_eval(kind, X, y, lam, np.float64)
    return _cached(("fo-data", kind, n, m, d, seed_offset), build)


class FoCase:
    """One first-order case: the data, the run arguments, the long-double run (``ld``), the float64
    run of the same recurrence (``f64``) and the bounds from them. ``theta`` / ``obj`` / ``cnt`` /
    ``mask`` / ``margin`` are the long-double run's; ``e_obj`` (relative per trace entry) and
    ``e_theta`` (over ``scale_theta`` = max |theta| of the run) the float64 noise; ``b_obj`` /
    ``b_theta`` = ``bound(e64, d, m_logistic, n=n)``."""

    def __init__(self, kind, alg, n, m, d, K, faithful, seed_offset):
        X, y, lam, step, hmax, ev_ld, ev_64 = _fo_data(kind, n, m, d, seed_offset)
        self.kind, self.variant, self.n, self.m, self.d, self.K, self.faithful = kind, alg, n, m, d, K, faithful
        self.X, self.y, self.lam, self.step0, self.hmax = X, y, lam, step, hmax
        self.alg, self.args = fo_run_args(alg, n, K, step, hmax)
        kw = dict(self.args, kind=kind, lam=lam, faithful=faithful)
        self.ld = first_order(self.alg, X, y, K, dtype=LD, ev=ev_ld, **kw)
        self.f64 = first_order(self.alg, X, y, K, dtype=np.float64, ev=ev_64, **kw)
        for r in (self.ld, self.f64):
            _freeze(*[v for v in r.values() if isinstance(v, np.ndarray)])
        self.obj, self.theta, self.scale_theta = self.ld["obj"], self.ld["theta"], self.ld["scale"]
        self.cnt, self.mask, self.margin = self.ld.get("cnt"), self.ld.get("mask"), self.ld.get("margin")
        self.uploads = None if self.cnt is None else float(self.cnt.sum())
        self.e_obj = noise_level(self.obj, self.f64["obj"], np.abs(self.obj))
        self.e_theta = noise_level(self.theta, self.f64["theta"], self.scale_theta)
        ml = m if kind == "logistic" else 0
        self.b_obj, self.b_theta = bound(self.e_obj, d, ml, n=n), bound(self.e_theta, d, ml, n=n)

    def err_obj(self, obj):
        obj = np.asarray(obj)
        return noise_level(self.obj[:len(obj)], obj, np.abs(self.obj[:len(obj)]))

    def err_theta(self, theta):
        """``theta`` (d,) or (N, d) (a server algorithm's replicated rows: each against the one
        reference row) over ``scale_theta``."""
        return noise_level(np.broadcast_to(self.theta, np.shape(theta)), theta, self.scale_theta)


# Per-shape seed offsets, changed only when a case misses the noise cap or a LAG condition of
# tests/test_hp_reference_cpu.py (none widened; every change is recorded here with its reason).
FO_SEED_OFFSET = {}


def first_order_case(kind, alg, n, m, d, K=FO_K, faithful=True):
    """The cached ``FoCase`` of variant ``alg`` (one of ``FO_ALGS``) on ``make_linear`` /
    ``make_logistic(n, m, d, seed_of(n, m, d))`` (``lam = 1e-3`` as ``make_logistic`` returns it)."""
    off = FO_SEED_OFFSET.get((kind, n, m, d), 0)
    return _cached(("fo", kind, alg, n, m, d, K, bool(faithful), off),
                   lambda: FoCase(kind, alg, n, m, d, K, bool(faithful), off))


# The shapes of tests/test_gpu_first_order_classes.py (why each is there is written next to that
# file's parameter lists).
FO_LINEAR_SHAPES = [(2, 3, 1), (3, 7, 3), (5, 70, 64), (4, 80, 65), (3, 150, 128), (1, 5, 3), (33, 8, 4), (65, 6, 3),
                    (253, 4, 2), (256, 4, 2)]
FO_LINEAR_WIDE = (257, 4, 2)  # DGD and dual averaging only: the server algorithms stop at n = 256
FO_LOGISTIC_SHAPES = [(3, 5, 3), (3, 64, 20), (3, 65, 20), (3, 128, 64), (4, 70, 60), (3, 129, 20), (2, 60, 65),
                      (2, 66, 128), (2, 130, 70), (33, 6, 3)]
FO_BIG_SHAPES = [(1, 140, 129), (3, 140, 129), (3, 270, 256), (3, 270, 257), (3, 60, 50)]
FO_LIVE_STOP_AT = 40
# (variant, n, m, d, faithful) of the live stop rule: the persistent engine's monitor at (3, 7, 3) and
# the large-d engine's device stop rule at d = 129. GD and DGD run with faithful=False: the faithful
# first step along ones moves AWAY from the optimum, and the stop rule's gaps must decrease from the
# start (dual averaging has no such quirk).
FO_LIVE_STOP = [("GD", 3, 7, 3, False), ("DGD", 3, 7, 3, False), ("DualAvg", 3, 7, 3, True),
                ("GD", 3, 140, 129, False)]


def fo_algs(n):
    """The variants run at worker count ``n``. LAG-WK is left out at n = 1: its trigger compares a
    gradient change of the one worker with its own step history, the run is a feedback loop on a single
    comparison and its float64 noise (theta: 2.8e-9 at linear (1, 5, 3)) is far above the 1e-12 cap.
    At n >= 65 the randomized schedule stands for IAG: in 80 iterations the cyclic one never reaches a
    row beyond 80."""
    return [a for a in FO_ALGS if not (n == 1 and a == "LAG-WK") and not (n >= 65 and a == "cIAG")]


def fo_live_stop(case):
    """``(obj0, tol, gaps)`` of a live stop rule on ``case``: ``obj0`` the long-double objective after
    the last iteration, ``tol`` the midpoint of the gaps ``|obj_k - obj0|`` at iterations 39 and 40."""
    gaps = np.abs(case.obj - case.obj[-1])
    k = FO_LIVE_STOP_AT
    return float(case.obj[-1]), float((gaps[k - 2] + gaps[k - 1]) / 2), gaps


# ------------------------------------------------------------------------------------------------
# Set-up kernels (tests/test_gpu_setup_kernels.py): the three Grams (csrc/kernels/gram.hip,
# gram_ozaki.hip, gram_crt.hip) against EXACT integer Grams, the inverses (spd_inverse.hip,
# spd_inverse_blocked.hip) against the long-double inverse with the float64 Gauss-Jordan recurrence of
# the kernels as the noise measure.
CRT_NMOD = 16   # moduli of gram_crt.hip: Garner's Horner evaluation rounds at most once per modulus
IMAGE_BITS = 49  # bits of the int8 schemes' integer images (gram_crt.hip KB; 7 digits of 7 bits)


def column_exponents(cols):
    """The int8 Grams' documented column-exponent rule on the augmented columns ``cols`` (..., m, D):
    the smallest e with ``max|x| <= 127/128 * 2^e`` (``frexp``, incremented when the fraction is above
    127/128), and 0 for an all-zero column. Returns int64 (..., D)."""
    mx = np.max(np.abs(np.asarray(cols, dtype=np.float64)), axis=-2)
    f, e = np.frexp(mx)
    e = np.where(f > 127.0 / 128.0, e + 1, e)
    return np.where(mx > 0, e, 0).astype(np.int64)


def _int_gram(N):
    """``sum_i N_ia N_ib`` of int64 ``N`` (shards, m, D) as Python integers (object array): the values are
    split into halves of at most 25 bits so that every int64 partial Gram is exact (asserted)."""
    N = np.asarray(N, dtype=np.int64)
    hi = (N + (1 << 24)) >> 25  # nearest: N = hi 2^25 + lo, |lo| <= 2^24
    lo = N - (hi << 25)
    big = max(int(np.max(np.abs(hi))), int(np.max(np.abs(lo))), 1)
    assert N.shape[1] * big * big < 2 ** 63
    g = lambda a, b: np.einsum("nmi,nmj->nij", a, b).astype(object)  # noqa: E731
    return g(hi, hi) * (1 << 50) + (g(hi, lo) + g(lo, hi)) * (1 << 25) + g(lo, lo)


class ExactGram:
    """``X`` (shards, m, d), ``y`` (shards, m) float64; ``G`` the exact augmented Gram as Python integers
    (object, shards x D x D); ``shift`` (shards, D) with ``x_ij = N_ij 2^shift_j``; ``image`` the float64
    image ``G_ab 2^(shift_a + shift_b)`` (exact when every ``|G_ab| < 2^53``, else None); ``A``, ``b``,
    ``yy`` its blocks; ``e`` the column exponents the int8 kernels must derive; ``N`` the integers."""

    def __init__(self, N, shift, need_image):
        N = np.asarray(N, dtype=np.int64)
        shift = np.broadcast_to(np.asarray(shift, dtype=np.int64), (N.shape[0], N.shape[2]))
        aug = np.ldexp(N.astype(np.float64), shift[:, None, :])   # exact: |N| < 2^53, a power-of-two scale
        self.N, self.shift = N, np.array(shift)
        self.X, self.y = np.ascontiguousarray(aug[:, :, :-1]), np.ascontiguousarray(aug[:, :, -1])
        self.m, self.d = N.shape[1], N.shape[2] - 1
        self.G = _int_gram(N)
        self.e = column_exponents(aug)
        self.pair_shift = self.shift[:, :, None] + self.shift[:, None, :]
        self.image = self.A = self.b = self.yy = None
        if need_image:
            assert max(abs(int(v)) for v in self.G.reshape(-1)) < 2 ** 53   # the float64 image is exact
            self.image = np.ldexp(self.G.astype(np.float64), self.pair_shift)
            d = self.d
            self.A, self.b, self.yy = self.image[:, :d, :d], self.image[:, d, :d], self.image[:, d, d]
            _freeze(self.image)
        _freeze(self.N, self.shift, self.X, self.y, self.e, self.pair_shift)

    def unscale(self, A, b, yy):
        """Kernel outputs (shards, d, d), (shards, d), (shards,) as the augmented (shards, D, D) matrix in
        units of the integer Gram (an exact power-of-two scaling of every entry)."""
        n, d = self.N.shape[0], self.d
        out = np.empty((n, d + 1, d + 1), dtype=np.float64)
        out[:, :d, :d], out[:, d, :d], out[:, :d, d], out[:, d, d] = A, b, b, yy
        return np.ldexp(out, -self.pair_shift)


def exact_gram(N_int, s):
    """Integer data ``N_int`` (shards, m, d + 1; the last column is y) with per-column power-of-two
    exponents ``s`` ((d + 1,) or (shards, d + 1)): ``X = N_int 2^s`` and the exact Gram with its float64
    image, which is exact because every ``|G_ab| < 2^53`` (asserted). See ``ExactGram``."""
    return ExactGram(N_int, s, True)


def image_gram(N49, e):
    """Full 49-bit images ``|N| < 2^49``, ``x = N 2^(e_j - 49)``: the exact integer Gram (Python integers)
    and the column exponents the kernels derive from the data, which must be the intended ``e`` (the
    generator pins each column's maximum; asserted). See ``ExactGram`` (``image`` is None)."""
    N49 = np.asarray(N49, dtype=np.int64)
    assert int(np.max(np.abs(N49))) < 2 ** IMAGE_BITS
    e = np.broadcast_to(np.asarray(e, dtype=np.int64), (N49.shape[0], N49.shape[2]))
    g = ExactGram(N49, e - IMAGE_BITS, False)
    assert np.array_equal(g.e, e), "a column's maximum does not pin the intended exponent"
    return g


def gram_errors(g, A, b, yy, lower_only=False):
    """Entrywise ``|out - exact| / (2^-53 |exact|)`` of kernel outputs against the exact integer Gram, in
    exact rational arithmetic: ``(largest ratio over the entries with exact != 0, number of entries
    with exact == 0 and out != 0)``. Integer-valued outputs compare as Python integers."""
    U = g.unscale(A, b, yy)
    worst, nonzero_at_zero = 0.0, 0
    from fractions import Fraction
    for n in range(U.shape[0]):
        Un, Gn = U[n], g.G[n]
        whole = Un == np.rint(Un)
        for a in range(Un.shape[0]):
            for c in range(a + 1 if lower_only else Un.shape[1]):
                ex = Gn[a, c]
                v = float(Un[a, c])
                if ex == 0:
                    nonzero_at_zero += v != 0.0
                    continue
                if not np.isfinite(v):
                    return float("inf"), nonzero_at_zero
                err = abs(int(v) - ex) if whole[a, c] else abs(Fraction(v) - ex)
                worst = max(worst, float(Fraction(err * 2 ** 53, abs(ex))))
    return worst, int(nonzero_at_zero)


def range_statistic(g):
    """``max_j colmax_j / sqrt(G_jj / m)`` per shard over the augmented columns with ``G_jj > 0`` (the
    accuracy gate's statistic, linalg.gram), in long double from the exact Gram."""
    out = np.zeros(g.N.shape[0], dtype=LD)
    aug = np.abs(np.concatenate([g.X, g.y[:, :, None]], axis=2)).max(axis=1)
    for n in range(g.N.shape[0]):
        for j in range(g.d + 1):
            gjj = int(g.G[n, j, j])
            if gjj > 0:
                ajj = np.ldexp(LD(gjj), int(2 * g.shift[n, j]))   # exact: G_jj < 2^53
                out[n] = max(out[n], LD(aug[n, j]) / np.sqrt(ajj / LD(g.m)))
    return out


def integer_gram_case(shards, m, d, amp, seed=0):
    """The integer-exact data family, cached: ``N_int`` uniform in ``[-amp, amp]`` with, as far as the
    d + 1 columns allow (D >= 6: all; D = 4: the first four; D = 2: the first two), in this order

    * a column whose largest magnitude is exactly ``127 2^k`` (the exponent rule's edge: not
      incremented), the extreme NEGATIVE;
    * one at ``255 2^k`` (incremented);
    * an all-zero column;
    * one at ``2^k``;
    * two orthogonal columns, ``v = (u_1, -u_0, u_3, -u_2, ...)`` (a last odd row: 0): products that
      cancel to an exact 0;

    on the columns 0, D - 1 (y), D - 2 (the last feature), 1, 2, D - 3, rotated by the shard index, so
    that the second shard of a call has them elsewhere (a stale exponent or maximum of the previous
    shard shows). Column scales ``2^s``, s uniform in [-30, 30] per shard and column. ``k`` is the
    largest with ``255 2^k <= amp``. ``m amp^2 < 2^53``: every partial sum in any order is exact."""
    def build():
        assert amp >= 255 and m * amp * amp < 2 ** 53 and amp <= 2 ** 20
        rng = np.random.default_rng([seed, shards, m, d, amp])
        D = d + 1
        N = rng.integers(-amp, amp + 1, size=(shards, m, D), dtype=np.int64)
        N[:, 0, :] = np.where(N[:, 0, :] == 0, 1, N[:, 0, :])   # no accidental all-zero column at m = 1
        s = rng.integers(-30, 31, size=(shards, D), dtype=np.int64)
        k = int(np.floor(np.log2(amp / 255.0)))
        pos = [0, D - 1, D - 2, 1, 2, D - 3] if D >= 6 else list(range(D))
        kinds = ["e127", "e255", "zero", "pow2", "orth"] if D >= 6 else ["e127", "e255", "zero", "pow2"][:D]
        for n in range(shards):
            p = pos[n % len(pos):] + pos[:n % len(pos)]
            row = int(rng.integers(0, m))
            for kind, c in zip(kinds, p):
                if kind == "zero":
                    N[n, :, c] = 0
                elif kind == "orth":
                    u = N[n, :, p[5]].copy()
                    v = np.zeros_like(u)
                    h = m // 2 * 2
                    v[0:h:2], v[1:h:2] = u[1:h:2], -u[0:h:2]
                    N[n, :, c] = v
                else:
                    top = {"e127": 127, "e255": 255, "pow2": 1}[kind] << k
                    N[n, :, c] = np.clip(N[n, :, c], -top + 1, top - 1)
                    N[n, row, c] = -top if kind == "e127" else top
        return exact_gram(N, s)
    return _cached(("int-gram", shards, m, d, amp, seed), build)


def image_case(shards, m, d, seed=0):
    """Full 49-bit images, cached: column j has the intended exponent ``e_j`` uniform in [-20, 20] and
    holds ``+T``, ``-T`` (the largest image the exponent rule admits at that exponent, ``T = 127 2^42``:
    ``max|x| = 127/128 2^e`` exactly, where the rule does not increment) and 0 when m >= 3, the rest
    uniform in ``[-T, T]``."""
    def build():
        assert m >= 3
        rng = np.random.default_rng([seed, shards, m, d, 49])
        T = 127 << 42
        D = d + 1
        N = rng.integers(-T, T + 1, size=(shards, m, D), dtype=np.int64)
        e = rng.integers(-20, 21, size=(shards, D), dtype=np.int64)
        for n in range(shards):
            for j in range(D):
                r = rng.choice(m, size=3, replace=False)
                N[n, r[0], j], N[n, r[1], j], N[n, r[2], j] = T, -T, 0
        return image_gram(N, e)
    return _cached(("image-gram", shards, m, d, seed), build)


def _gj_plain(W):
    """In place: Gauss-Jordan without pivoting in the kernels' operation order (spd_inverse.hip):
    ``p = 1 / m_kk``; row k scaled; rank-1 update off row and column k; column k = ``-a_ik p``."""
    d = W.shape[0]
    for k in range(d):
        p = 1.0 / W[k, k]
        row = W[k, :] * p
        col = W[:, k].copy()
        row[k] = 0.0
        col[k] = 0.0
        W -= np.outer(col, row)
        W[k, :] = row
        W[:, k] = -col * p
        W[k, k] = p
    return W


def _gj_blocked(W, nb):
    """In place on the lower triangle, the scheme in the header of spd_inverse_blocked.hip: per pivot
    block K the panel C (``W_iK`` below, ``-W_Ki'`` left of it), ``Pi = W_KK^-1`` (a block wider than 64
    recurses with 64-blocks), the residual-corrected ``Lc0 = C Pi``, ``R0 = C - Lc0 P``,
    ``Lc = Lc0 + R0 Pi``, ``R = C - Lc P``, the signed lower update
    ``W_IJ -= sgn_J (Lc_I C_J' + R_I Lc_J')`` as one product of ``[Lc | R]`` and ``[C | Lc]``, the cross; then
    the mirror."""
    d = W.shape[0]
    for k0 in range(0, d, nb):
        b = min(nb, d - k0)
        k1 = k0 + b
        C = np.zeros((d, b))
        C[:k0] = -W[k0:k1, :k0].T
        C[k1:] = W[k1:, k0:k1]
        P = np.tril(W[k0:k1, k0:k1])
        P = P + np.tril(P, -1).T
        Pi = gauss_jordan_inverse(P) if b <= 64 else _gj_blocked(P.copy(), 64)
        Lc = C @ Pi
        Lc = Lc + (C - Lc @ P) @ Pi
        R = C - Lc @ P
        sgn = np.where(np.arange(d) < k0, -1.0, 1.0)
        W -= (np.hstack([Lc, R]) @ np.hstack([C, Lc]).T) * sgn[None, :]   # rows and columns of K: C is 0 there
        W[k1:, k0:k1] = -Lc[k1:]
        W[k0:k1, :k0] = -Lc[:k0].T
        W[k0:k1, k0:k1] = Pi
    L = np.tril(W)
    W[:] = L + np.tril(L, -1).T
    return W


def gauss_jordan_inverse(M, nb=None):
    """float64 NumPy inverse of the symmetric ``M`` by the kernels' recurrence: the noise measure of the
    inverse tests, never their reference. ``nb = None``: spd_inverse.hip (plain Gauss-Jordan, then
    ``0.5 (W + W')``); ``nb`` 64 or 128: spd_inverse_blocked.hip."""
    W = np.array(M, dtype=np.float64)
    with np.errstate(all="ignore"):
        if nb is None:
            _gj_plain(W)
            return 0.5 * (W + W.T)
        assert nb in (64, 128)
        return _gj_blocked(W, nb)


INVERSE_KINDS = ("well", "ill")
_WELL_SHIFTS = (0.05, 0.11, 0.23, 0.4, 0.7, 1.3)   # times d: distinct per (worker, variant)
_ILL_KAPPA = (3e6, 6e6, 1e7, 1.7e7, 3e7, 5e7)      # target condition numbers, distinct likewise


class InverseMatrix:
    """One shifted Gram ``M = fl(A + s I)`` (what the kernels form), its long-double inverse ``ref``,
    ``kappa`` (2-norm, ``eigvalsh``), and per recurrence (``nb`` None / 64 / 128) the float64 noise
    ``e64(nb) = max|gauss_jordan_inverse(M, nb) - ref| / max|ref|`` and the bound
    ``FACTOR * max(e64, d 2^-53 kappa)``: the project's factor over the noise of the same recurrence,
    floored by the forward error of a backward-stable inversion."""

    def __init__(self, A, s):
        d = A.shape[0]
        self.d, self.A, self.s = d, A, float(s)
        self.M = A + self.s * np.eye(d)
        ev = np.linalg.eigvalsh(self.M)
        assert ev[0] > 0
        self.kappa = float(ev[-1] / ev[0])
        self.ref = spd_inverse(self.M, LD)
        self.scale = float(np.max(np.abs(self.ref)))
        self._e64 = {}
        _freeze(self.M, self.ref)

    def err(self, X):
        return noise_level(self.ref, X, self.scale)

    def e64(self, nb=None):
        if nb not in self._e64:
            self._e64[nb] = self.err(gauss_jordan_inverse(self.M, nb))
        return self._e64[nb]

    def bound(self, nb=None):
        return FACTOR * max(self.e64(nb), self.d * 2.0 ** -53 * self.kappa)

    def self_error(self):
        """The reference's own first-order error estimate ``max|X (M X - I)| / max|X|`` (long double)."""
        X, M = self.ref, self.M.astype(LD)
        return float(np.max(np.abs(X @ (M @ X - np.eye(self.d, dtype=LD)))) / LD(self.scale))


def _inverse_gram(kind, d, seed, n):
    def build():
        rng = np.random.default_rng([seed, d, n, INVERSE_KINDS.index(kind)])
        Z = rng.standard_normal((2 * d if kind == "well" else d // 2, d))
        A = Z.T @ Z
        A = 0.5 * (A + A.T)
        _freeze(A)
        return A, (float(np.linalg.eigvalsh(A)[-1]) if Z.shape[0] else 0.0)
    return _cached(("inv-gram", kind, d, seed, n), build)


def inverse_matrix(kind, d, seed, n, v, variants):
    """The cached ``InverseMatrix`` of worker ``n``, variant ``v``. ``well``: ``Z'Z`` of 2d Gaussian rows
    plus ``d * _WELL_SHIFTS[n variants + v]`` (kappa <= 100). ``ill``: the Gram of d // 2 rows, singular,
    plus ``lambda_max / _ILL_KAPPA[...]``, so 1e6 <= kappa_2 <= 1e8 (asserted; d >= 2: a 1 x 1 matrix
    has kappa 1)."""
    def build():
        A, lmax = _inverse_gram(kind, d, seed, n)
        i = (n * variants + v) % len(_WELL_SHIFTS)
        if kind == "well":
            c = InverseMatrix(A, d * _WELL_SHIFTS[i])
            assert c.kappa <= 100
        else:
            assert d >= 2
            c = InverseMatrix(A, lmax / _ILL_KAPPA[i])
            assert 1e6 <= c.kappa <= 1e8, c.kappa
        return c
    return _cached(("inv", kind, d, seed, n, v, variants), build)


class InverseCase:
    """``A`` (workers, d, d), ``shifts`` (workers, variants), ``mats[n][v]`` the ``InverseMatrix``."""

    def __init__(self, kind, d, seed, workers, variants):
        self.kind, self.d = kind, d
        self.mats = [[inverse_matrix(kind, d, seed, n, v, variants) for v in range(variants)] for n in range(workers)]
        self.A = np.stack([row[0].A for row in self.mats])
        self.shifts = np.array([[c.s for c in row] for row in self.mats])

    def ratios(self, out, nb=None, skip=()):
        """``err / bound`` of every matrix of ``out`` (workers, variants, d, d) not in ``skip``."""
        return {"n%dv%d" % (n, v): c.err(out[n, v]) / c.bound(nb)
                for n, row in enumerate(self.mats) for v, c in enumerate(row) if (n, v) not in skip}


def inverse_case(kind, d, seed=0, workers=3, variants=2):
    """The cached inverse case of family ``kind`` (``well`` / ``ill``) at size ``d``: ``workers`` Grams
    with ``variants`` distinct shifts each. A smaller case shares its matrices with a larger one of the
    same ``variants`` (the long-double inverse is computed once per matrix)."""
    return _cached(("inv-case", kind, d, seed, workers, variants),
                   lambda: InverseCase(kind, d, seed, workers, variants))


def non_spd_matrix(d, bad, seed=0, nan=False):
    """A symmetric ``L D L'`` (unit lower-triangular L with small entries, D = 1 .. 2 except
    ``D[bad] = -1``): the pivots of Gauss-Jordan without pivoting are D's entries (up to rounding, all
    far from 0), so the first non-positive one is at index ``bad``. ``nan``: instead a well-conditioned
    SPD matrix whose entry (bad, bad) is NaN."""
    rng = np.random.default_rng([seed, d, bad, int(nan)])
    L = np.tril(rng.uniform(-1, 1, (d, d)) / (2 * d), -1) + np.eye(d)
    D = rng.uniform(1, 2, d)
    if not nan:
        D[bad] = -1.0
    M = (L * D) @ L.T
    M = 0.5 * (M + M.T)
    if nan:
        M[bad, bad] = np.nan
    return M


# The shapes of tests/test_gpu_setup_kernels.py (the edge each one sits on is written there).
GRAM_AMP = 2 ** 20 - 1   # m amp^2 < 2^53 up to m = 8191; at most 3 non-zero base-128 digits per value
GRAM_AMP_LONG = 1000     # the cases of more than one chunk
GRAM_F64_D = (1, 62, 63, 64, 126, 127, 128, 129, 255)
GRAM_F64_M = (1, 15, 16, 17, 33)
GRAM_F64_SPLIT = ((40, 3), (33, 4), (512, 2), (513, 2))   # (m, ksplit)
GRAM_F64_SPLIT_D = (3, 70)                                # both tile sizes
GRAM_F64_AUTO = (2, 1025, 70)
GRAM_OZ_D = (1, 62, 63, 64, 129)
GRAM_OZ_M = (1, 31, 32, 33)
GRAM_OZ_LONG = (8191, 8192, 8193, 16385)    # d = 3, 2 shards, amp 1000
GRAM_CRT_D = (1, 254, 255, 256)
GRAM_CRT_M = (1, 33, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321)
GRAM_CRT_LONG = (32768, 32769, 65537)       # d = 3, 2 shards, amp 1000
GRAM_IMAGE = ((300, 5), (65, 255), (257, 256))
INV_SMALL_D = (1, 2, 7, 8, 9, 63, 64)
INV_GENERAL_D = (32, 33, 65, 90, 91, 127, 128)
INV_BLOCKED_D = (129, 192, 193, 257)


def gram_int_case(m, d):
    """The integer case of shape (m, d) shared by the three kernels' tests: 2 shards; amplitude
    ``GRAM_AMP`` while ``m amp^2 < 2^53``, else ``GRAM_AMP_LONG``."""
    return integer_gram_case(2, m, d, GRAM_AMP if m * GRAM_AMP ** 2 < 2 ** 53 else GRAM_AMP_LONG)


def gram_int_shapes():
    """Every (m, d) at which tests/test_gpu_setup_kernels.py runs an integer case."""
    out = {(m, d) for d in GRAM_F64_D for m in GRAM_F64_M} | {(m, d) for d in GRAM_F64_SPLIT_D for m, _ in GRAM_F64_SPLIT}
    out |= {GRAM_F64_AUTO[1:]} | {(m, d) for d in GRAM_OZ_D for m in GRAM_OZ_M} | {(m, 3) for m in GRAM_OZ_LONG}
    out |= {(m, d) for d in GRAM_CRT_D for m in GRAM_CRT_M} | {(m, 3) for m in GRAM_CRT_LONG}
    return sorted(out)


# ------------------------------------------------------------------------------------------------
# D-GADMM (tests/test_gpu_dgadmm_classes.py): prescribed chains, the cases and their references.
DGADMM_MOVES = ("reverse", "rotate", "same", "random")


def dgadmm_chains(n, K, coherence):
    """The prescribed chains of a D-GADMM case: ``[(first_iteration, path), ...]``, deterministic, no
    ``find_path2`` draw. The initial chain is a seeded permutation that is not the identity (worker id !=
    chain position != local index); at every re-chain iteration (``rechain_iterations(K, coherence)``)
    the next move of the cycle ``DGADMM_MOVES`` is applied to the current chain:

    * reverse: left and right swap; at even n every head becomes a tail;
    * rotate by one: every role flips (but the wrapped worker's at odd n), the first worker, an end,
      goes to the other end, its neighbour becomes an end and the old last worker an interior one;
    * the same chain again;
    * a new seeded random permutation.

    The cycle starts at "reverse" for even n and at "rotate" for odd n: the reversal of an odd chain
    leaves every worker its role and its pair of neighbours, so a case whose only re-chain it were
    (coherence K) would not notice a kernel that ignores re-chains."""
    from gadmm_amd.parallel.topology import rechain_iterations
    rng = np.random.default_rng([int(n), int(coherence), 7919])
    path = [int(v) for v in rng.permutation(n)]
    if path == list(range(n)):
        path = path[::-1]
    chains = [(1, list(path))]
    step = n % 2
    for it in rechain_iterations(K, coherence):
        move = DGADMM_MOVES[step % len(DGADMM_MOVES)]
        step += 1
        if move == "reverse":
            path = path[::-1]
        elif move == "rotate":
            path = path[1:] + path[:1]
        elif move == "random":
            path = [int(v) for v in rng.permutation(n)]
        chains.append((int(it), list(path)))
    assert len(chains) == 1 or any(a[1] != b[1] for a, b in zip(chains, chains[1:])), "no re-chain changes the chain"
    return chains


def _chains_key(chains):
    return tuple((int(f), tuple(int(w) for w in p)) for f, p in chains)


def _dgadmm_history(n, m, d, chains, K, dtype, mutant=None):
    """One run of the recurrence per (case, chains, arithmetic), K_ITERS long for the tests that stop
    at the cap and PERSISTENT_OVERRUN longer for the iteration a persistent kernel happens to stop at
    (the chains end at the cap: the kernels re-chain at none of the iterations past it)."""
    run = K if K <= K_ITERS else max(K, K_ITERS + PERSISTENT_OVERRUN)

    def build():
        X, y, rho = make_linear(n, m, d, seed_of(n, m, d))
        out = _dgadmm_run(X, y, rho, run, chains, dtype, mutant)
        _freeze(X, y, *out)
        return (X, y, rho) + out
    return _cached(("dgadmm-run", n, m, d, _chains_key(chains), run, np.dtype(dtype).name, mutant), build)


def dgadmm_case(n, m, d, coherence, K=K_ITERS, chains=None):
    """``(X, y, rho, chains, Reference)`` of ``dgadmm_linear`` on ``make_linear(n, m, d, seed_of(n, m,
    d))`` over ``dgadmm_chains(n, min(K, K_ITERS), coherence)`` (or the explicit ``chains``), K iterations
    long: the long-double run, and the float64 run of the same recurrence as the noise measure. A
    ``K > K_ITERS`` is the iteration a persistent kernel stopped at, past a cap of K_ITERS."""
    if chains is None:
        chains = dgadmm_chains(n, min(K, K_ITERS), coherence)
    chains = [(int(f), [int(w) for w in p]) for f, p in chains]

    def build():
        X, y, rho, th, mus, obj = _dgadmm_history(n, m, d, chains, K, LD)
        _, _, _, th64, mus64, obj64 = _dgadmm_history(n, m, d, chains, K, np.float64)
        return X, y, rho, chains, Reference((th[:K], mus[K - 1], obj[:K]), (th64[:K], mus64[K - 1], obj64[:K]), rho, d,
                                            chains=chains)
    return _cached(("dgadmm", n, m, d, _chains_key(chains), K), build)


def dgadmm_matrices(chains):
    """``(path_matrix (E, n), cost_matrix (E, n - 1) of ones)`` of ``chains`` for
    ``dynamic_group_admm_v0`` / ``PathSchedule(kind="matrix")``: row e is the chain of epoch e."""
    P = np.asarray([p for _, p in chains], dtype=np.int64)
    return P, np.ones((P.shape[0], max(P.shape[1] - 1, 0)))


# (n, m, d) -> coherences of tests/test_gpu_dgadmm_classes.py (why each shape is there is written next
# to that file's parameter lists; the d of the LDS thresholds are derived from the kernels' LDS formula
# there and asserted to be these).
DGADMM_SMALL = [(2, 3, 1), (3, 7, 3), (5, 40, 32), (4, 40, 33), (5, 60, 52)]
DGADMM_REG16 = [(5, 70, 53), (4, 40, 64)]
DGADMM_LDS_EXACT = [(3, 80, 65), (3, 100, 81)]
DGADMM_LDS_IDENTITY = [(3, 100, 82), (3, 120, 99)]
DGADMM_INELIGIBLE = (3, 120, 100)
DGADMM_MULTI_WG = [(13, 20, 8), (25, 12, 5), (13, 60, 52)]
DGADMM_GRAPH = [(3, 7, 3), (3, 80, 65), (3, 150, 129), (3, 280, 257)]
DGADMM_SWEEP = [((2, 40, 33), 1), ((3, 40, 33), 3), ((5, 40, 33), 7), ((13, 40, 33), 3)]


def dgadmm_cases():
    """Every ``(n, m, d, coherence)`` a GPU test of D-GADMM runs, sorted."""
    out = set()
    for s in DGADMM_SMALL + DGADMM_REG16 + DGADMM_LDS_EXACT + DGADMM_LDS_IDENTITY + DGADMM_MULTI_WG:
        out |= {s + (1,), s + (3,)}
    for s in [(5, 60, 52), (13, 20, 8)]:
        out |= {s + (7,), s + (K_ITERS,)}
    out |= {DGADMM_INELIGIBLE + (3,), (3, 80, 65, 1)} | {s + (3,) for s in DGADMM_GRAPH}
    out |= {s + (c,) for s, c in DGADMM_SWEEP}
    return sorted(out)


# ------------------------------------------------------------------------------------------------
# Q-GADMM (tests/test_gpu_qgadmm_classes.py): the quantized recurrence, the cases and their seeds.
QGADMM_MUTANTS = ("dual-true", "rhs-true", "obj-hat", "u-position", "no-clamp")
_M64 = (1 << 64) - 1


def q_uniforms(seed, it, n_workers, w, d):
    """The ``d`` uniforms of worker id ``w`` at iteration ``it`` (1-based): the counter formula of the
    gadmm_amd/algorithms/quantize.py docstring restated in Python integers mod 2^64 (no code shared with
    ``quantize.u01``): ``x = seed + 0x9e3779b97f4a7c15 * (((it * N + w) * d + i) + 1)``, the splitmix64
    finaliser, ``u = (z >> 11) * 2^-53``. float64 (d,): 53-bit integers times a power of two, exact."""
    out = np.empty(d, dtype=np.float64)
    for i in range(d):
        z = (int(seed) + 0x9e3779b97f4a7c15 * ((int(it) * int(n_workers) + int(w)) * int(d) + i + 1)) & _M64
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
        z ^= z >> 31
        out[i] = float(z >> 11) * 2.0 ** -53
    return out


def q_line(theta, hat, u, bits, dtype=LD, clamp=True):
    """The quantizer line on one worker's row, every operation in ``dtype``: ``R = max|theta - hat|``,
    ``delta = 2R / L``, ``q = clamp(floor((diff + R) / delta + u), 0, L)``, ``hat + (q delta - R)``; at
    ``R == 0`` every code is 0 and ``hat`` stays. Returns ``(R, q (d,) int64, new hat (d,), margin)``;
    the margin is ``min(frac, 1 - frac) * delta / max|theta|`` over the coordinates with ``|diff| < R``
    (``frac`` the fractional part of ``(diff + R) / delta + u``), inf when there is none."""
    theta = np.asarray(theta, dtype=dtype)
    hat = np.asarray(hat, dtype=dtype)
    u = np.asarray(u, dtype=dtype)
    L = np.asarray((1 << int(bits)) - 1, dtype=dtype)
    diff = theta - hat
    R = np.max(np.abs(diff))
    if R == 0:
        return R, np.zeros(theta.shape, dtype=np.int64), hat.copy(), np.inf
    delta = (np.asarray(2.0, dtype=dtype) * R) / L
    s = (diff + R) / delta + u
    fl = np.floor(s)
    q = np.minimum(np.maximum(fl, np.asarray(0.0, dtype=dtype)), L) if clamp else fl
    new = hat + (q * delta - R)
    inner = np.abs(diff) < R
    top = np.max(np.abs(theta))
    margin = np.inf
    if np.any(inner) and top > 0:
        frac = (s - fl)[inner]
        margin = float(np.min(np.minimum(frac, np.asarray(1.0, dtype=dtype) - frac)) * delta / top)
    return R, q.astype(np.int64), new, margin


def _qgadmm_run(X, y, rho, K, bits, seed, path, dtype, mutant=None):
    """The recurrence of ``qgadmm_linear`` with the state of EVERY iteration: ``(theta (K, N, d),
    th_hat (K, N, d), mu (K, N, d), objectives (K,), codes (K, N, d) int64, R (K, N), residual (K,),
    margin (K,) the smallest flip margin up to each iteration)``; a run to k is a prefix of a longer one."""
    N, m, d = X.shape
    assert mutant is None or mutant in QGADMM_MUTANTS
    path = list(range(N)) if path is None else [int(w) for w in path]
    tab = chain_tables([(1, path)])[0][1]
    assert len(tab) == N and N >= 2
    A, b, yy = _gram(X, y, dtype)
    rho = np.asarray(rho, dtype=dtype)
    eye = np.eye(d, dtype=dtype)
    Minv = [spd_inverse(A[w] + ((tab[w][1] is not None) + (tab[w][2] is not None)) * rho * eye, dtype)
            for w in range(N)]
    th = np.zeros((N, d), dtype=dtype)    # the true iterates
    hat = np.zeros((N, d), dtype=dtype)   # the public models: what neighbours hold
    mu = np.zeros((N, d), dtype=dtype)
    thetas = np.zeros((K, N, d), dtype=dtype)
    hats = np.zeros((K, N, d), dtype=dtype)
    mus = np.zeros((K, N, d), dtype=dtype)
    obj = np.zeros((K,), dtype=dtype)
    codes = np.zeros((K, N, d), dtype=np.int64)
    Rs = np.zeros((K, N), dtype=dtype)
    res = np.zeros((K,), dtype=dtype)
    margins = np.zeros((K,), dtype=np.float64)
    margin = np.inf
    seen = th if mutant == "rhs-true" else hat   # what a solve reads of its neighbours
    dual = th if mutant == "dual-true" else hat  # what the dual update reads
    for k in range(1, K + 1):
        for phase in (0, 1):
            for w in path[phase::2]:
                p, l, r = tab[w]
                rhs = b[w] - mu[w]
                if l is not None:
                    rhs = rhs + rho * seen[l]
                if r is not None:
                    rhs = rhs + rho * seen[r]
                th[w] = Minv[w] @ rhs
                u = q_uniforms(seed, k, N, p if mutant == "u-position" else w, d)
                Rs[k - 1, w], codes[k - 1, w], hat[w], mg = q_line(th[w], hat[w], u, bits, dtype,
                                                                   clamp=mutant != "no-clamp")
                margin = min(margin, mg)
        for w in path:
            _, l, r = tab[w]
            v = mu[w]
            if l is not None:
                v = v - rho * (dual[l] - dual[w])
            if r is not None:
                v = v + rho * (dual[w] - dual[r])
            mu[w] = v
        thetas[k - 1] = th
        hats[k - 1] = hat
        mus[k - 1] = mu
        obj[k - 1] = _gram_objective(A, b, yy, hat if mutant == "obj-hat" else th)
        tot = np.zeros((), dtype=dtype)
        for a_, b_ in zip(path, path[1:]):   # K4 on public models: every chain edge once
            e = hat[a_] - hat[b_]
            tot = tot + e @ e
        res[k - 1] = tot
        margins[k - 1] = margin
    return thetas, hats, mus, obj, codes, Rs, res, margins


def qgadmm_linear(X, y, rho, K, bits, seed, path=None, dtype=LD, mutant=None):
    """Q-GADMM (header of csrc/kernels/chain_quant.hip; specification gadmm_amd/algorithms/quantize.py)
    on the static chain ``path`` (position -> worker; None: the identity): GADMM whose theta table holds
    the public models ``th_hat``. Heads (even positions), then tails: worker w solves with the cached
    inverse of ``A_w + deg rho I`` from ``b_w - mu_w + rho (th_hat_l + th_hat_r)``, then quantizes
    ``theta_w - th_hat_w`` (``q_line``) with the uniforms of ``(iteration, worker ID w)`` -- not its chain
    position -- and moves ``th_hat_w``; then every worker's ``mu`` from ``th_hat`` of itself and its
    neighbours. The objective reads the true theta, the K4 residual (sum over chain edges of
    ``|th_hat_a - th_hat_b|^2``) the public models. All arithmetic in ``dtype``.
    ``mutant`` names a wrong implementation (tests/test_hp_reference_cpu.py measures how far each sits
    from the reference): ``"dual-true"`` the duals read true theta; ``"rhs-true"`` the right-hand side
    reads the neighbours' true theta; ``"obj-hat"`` the objective of ``th_hat``; ``"u-position"`` the
    uniforms indexed by chain position; ``"no-clamp"`` no clamp of the code.
    Returns ``(theta (K, N, d) true iterates, th_hat (N, d) after K, mu (N, d) after K, objectives (K,),
    codes (K, N, d), R (K, N), K4 residual (K,), the run's smallest flip margin)``."""
    th, hats, mus, obj, codes, Rs, res, margins = _qgadmm_run(np.asarray(X), y, rho, K, bits, seed, path, dtype, mutant)
    return th, hats[-1], mus[-1], obj, codes, Rs, res, float(margins[-1])


# The shapes of tests/test_gpu_qgadmm_classes.py (the edge each one sits on is written there).
QGADMM_BITS = (4, 8, 16)
QGADMM_GRAPH_SHAPES = [(2, 3, 1), (3, 7, 3), (3, 20, 4), (3, 20, 5), (3, 20, 8), (3, 20, 9), (4, 30, 16), (3, 30, 17),
                       (4, 40, 64), (3, 80, 65), (4, 150, 128), (3, 150, 129), (3, 280, 256)]
QGADMM_PERSISTENT_SHAPES = [(2, 3, 1), (3, 20, 4), (3, 20, 5), (3, 20, 8), (3, 20, 9), (4, 30, 16), (3, 30, 17),
                            (5, 40, 32), (4, 40, 33), (5, 60, 52), (5, 70, 53), (4, 40, 64)]
QGADMM_PERSISTENT_K = 8     # the cap of the persistent runs; the kernel stops up to PERSISTENT_OVERRUN later
QGADMM_PERSISTENT_RUN = QGADMM_PERSISTENT_K + PERSISTENT_OVERRUN
QGADMM_PATHS = {(5, 40, 33): (2, 0, 4, 1, 3), (4, 30, 16): (3, 2, 1, 0)}   # the permuted static chains (b = 8)
QGADMM_FIRST_SEED, QGADMM_LAST_SEED = 1234, 1297
QGADMM_MARGIN = 4.0         # a case is comparable while its smallest flip margin >= this many b_theta


def _qgadmm_history(n, m, d, bits, seed, path, run, dtype, mutant=None, data=0):
    def build():
        X, y, rho = make_linear(n, m, d, seed_of(n, m, d) + data)
        out = _qgadmm_run(X, y, rho, run, bits, seed, path, dtype, mutant)
        _freeze(X, y, *out)
        return (X, y, rho) + out
    return _cached(("qgadmm-run", n, m, d, bits, seed, path, run, np.dtype(dtype).name, mutant, data), build)


class QReference(Reference):
    """``Reference`` of a Q-GADMM case (``theta`` the TRUE iterates (K, N, d), ``dual`` = mu after K,
    ``obj``) plus ``hat`` (N, d) the public models after K, ``codes`` (K, N, d), ``R`` (K, N),
    ``res`` (K,) the K4 residual, ``margin`` the run's smallest flip margin, ``seed``, ``path``, and
    the bounds ``b_hat`` / ``b_R`` (errors over ``scale_theta``) and ``b_res`` (each entry over its own
    value where that exceeds 1e-20 of the trace's largest, over the largest below that). Its residual is
    the recurrence's own, on the PUBLIC models: ``Reference``'s (``res_w`` and the rest, a function of the
    true theta history) is not built here, and ``res`` / ``e_res`` / ``b_res`` / ``err_res`` are this
    class's."""

    def __init__(self, ld, f64, rho, d, seed, path):
        th, hats, mus, obj, codes, Rs, res, margins = ld
        super().__init__((th, mus[-1], obj), (f64[0], f64[2][-1], f64[3]), rho, d, residual=False)
        self.seed, self.path = seed, path
        self.hat, self.codes, self.R, self.res, self.margin = hats[-1], codes, Rs, res, float(margins[-1])
        self.codes_agree = bool(np.array_equal(codes, f64[4]))
        top = np.max(np.abs(res))
        self.res_scale = np.where(np.abs(res) > 1e-20 * top, np.abs(res), top)
        self.e_hat = noise_level(hats, f64[1], self.scale_theta)
        self.e_R = noise_level(Rs, f64[5], self.scale_theta)
        self.e_res = noise_level(res, f64[6], self.res_scale)
        self.b_hat, self.b_R, self.b_res = bound(self.e_hat, d), bound(self.e_R, d), bound(self.e_res, d)

    def err_hat(self, hat):
        return noise_level(self.hat, hat, self.scale_theta)

    def err_R(self, R):
        """``R`` (N,) of every worker's last message against the reference's iteration-K values."""
        return noise_level(self.R[-1], R, self.scale_theta)

    def err_res(self, res):
        res = np.asarray(res)
        return noise_level(self.res[:len(res)], res, self.res_scale[:len(res)])


def qgadmm_condition(n, m, d, bits, run, path=None, seed=QGADMM_FIRST_SEED):
    """The condition on the reference alone that makes a quantized run comparable, at ``run``
    iterations: ``(codes of the long-double and the float64 run identical, margin / b_theta)``; the
    case qualifies when the first holds and the second is >= QGADMM_MARGIN."""
    ref = _qgadmm_reference(n, m, d, bits, run, path, seed)[3]
    return ref.codes_agree, ref.margin / ref.b_theta


def _qgadmm_reference(n, m, d, bits, K, path, seed, run=None, data=0):
    path = None if path is None else tuple(int(w) for w in path)
    run = K if run is None else run
    assert K <= run

    def build():
        ld = _qgadmm_history(n, m, d, bits, seed, path, run, LD, data=data)
        f64 = _qgadmm_history(n, m, d, bits, seed, path, run, np.float64, data=data)
        return ld[:3] + (QReference(tuple(a[:K] for a in ld[3:]), tuple(a[:K] for a in f64[3:]), ld[2], d, seed, path),)
    return _cached(("qgadmm", n, m, d, bits, K, path, seed, run, data), build)


# (n, m, d, bits, path) -> the quantizer seed of the case: the first of 1234, 1235, ... at which the
# long-double and the float64 run produce identical codes and the smallest flip margin is
# >= QGADMM_MARGIN b_theta over the longest run a test asks for (``qgadmm_run_length``). Found once by
# a search on the CPU; only the cases that 1234 does not serve are listed, each with what 1234 gave.
# tests/test_hp_reference_cpu.py asserts the condition for every case and that an earlier seed fails.
QGADMM_SEEDS = {
    (3, 20, 5, 16, None): 1235,   # 1234: margin / b_theta = 0.75 at 20 iterations
    (2, 3, 2, 16, None): 1235,    # (a CPU-only case, qgadmm_power_cases) 1234: 1.63 at 24 iterations
}
# (shape, bits) pairs of QGADMM_PERSISTENT_SHAPES that no seed up to QGADMM_LAST_SEED serves over
# QGADMM_PERSISTENT_RUN iterations (they would be left out of the persistent tests): none.
QGADMM_DROPPED = ()


def qgadmm_run_length(d):
    """The longest run a test asks of a case: the persistent kernel (d <= 64) stops up to
    PERSISTENT_OVERRUN iterations past its cap of QGADMM_PERSISTENT_K; above it K_ITERS on the graph
    engine. The flip margin only falls as a run goes on, so a seed that serves it serves every prefix."""
    return max(K_ITERS, QGADMM_PERSISTENT_RUN) if d <= 64 else K_ITERS


def qgadmm_seed(n, m, d, bits, path=None):
    """``(seed, run length it is good for)`` of a case."""
    path = None if path is None else tuple(int(w) for w in path)
    return QGADMM_SEEDS.get((n, m, d, bits, path), QGADMM_FIRST_SEED), qgadmm_run_length(d)


def qgadmm_case(n, m, d, bits, K, path=None):
    """``(X, y, rho, QReference)`` of ``qgadmm_linear`` on ``make_linear(n, m, d, seed_of(n, m, d))`` with
    the case's seed (``QReference.seed``), K iterations long: the long-double run, and the float64 run of
    the same recurrence as the noise measure. Every K of a case is a prefix of one cached run."""
    seed, run = qgadmm_seed(n, m, d, bits, path)
    return _qgadmm_reference(n, m, d, bits, K, path, seed, run)


def qgadmm_power_cases():
    """The cases on which tests/test_hp_reference_cpu.py measures how far wrong variants of the
    recurrence land: ``qgadmm_cases()`` with the data of (2, 3, 1) replaced by (2, 3, 2). With ONE
    coordinate the difference is always extremal, its code is 0 or L and ``th_hat + (q delta - R)`` is
    theta itself up to rounding: th_hat == theta whatever the data, and a variant that reads the one
    for the other computes the recurrence. Two coordinates are the fewest at which one is interior."""
    return [((2, 3, 2) if c[:3] == (2, 3, 1) else c[:3]) + c[3:] for c in qgadmm_cases()]


def qgadmm_cases():
    """Every ``(n, m, d, bits, path)`` a GPU test of Q-GADMM runs."""
    shapes = QGADMM_GRAPH_SHAPES + [s for s in QGADMM_PERSISTENT_SHAPES if s not in QGADMM_GRAPH_SHAPES]
    return [s + (b, None) for s in shapes for b in QGADMM_BITS] + [s + (8, p) for s, p in QGADMM_PATHS.items()]


# ------------------------------------------------------------------------------------------------
# Cases for the sensitivity of the bound to a MISSING CLAMP. With ``|diff| <= R`` the code
# ``floor((diff + R) / delta + u)`` is in [0, L] already; the clamp acts only on an extremal coordinate
# with ``diff = +R`` whose ``c = L`` and whose draw is so close to 1 that ``c + u`` ROUNDS up to L + 1
# (``u > 1 - 2^-50`` at b = 4, ``> 1 - 2^-38`` at b = 16): no seed 1234, 1235, ... gets there in a short
# run. The counter formula is a bijection of the seed, though, so a seed can be SOLVED for: the one at
# which a chosen (iteration, worker, coordinate) draws the largest uniform there is, ``1 - 2^-53``.
_QM1, _QM2, _QGOLD = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb, 0x9e3779b97f4a7c15


def q_seed_drawing_top(low, it, n_workers, w, d, i):
    """The seed at which ``q_uniforms(seed, it, n_workers, w, d)[i] == 1 - 2^-53``: the splitmix64
    finaliser inverted (each xor-shift and each odd multiplier is a bijection mod 2^64) on
    ``z = (2^53 - 1) << 11 | low``; ``low`` in 0 .. 2047 are the bits the uniform drops, so there are
    2048 such seeds, which differ in every other draw."""
    assert 0 <= int(low) < 2048
    z = (((1 << 53) - 1) << 11) | int(low)
    z ^= (z >> 31) ^ (z >> 62)
    z = (z * pow(_QM2, -1, 1 << 64)) & _M64
    z ^= (z >> 27) ^ (z >> 54)
    z = (z * pow(_QM1, -1, 1 << 64)) & _M64
    z ^= (z >> 30) ^ (z >> 60)
    return (z - _QGOLD * ((int(it) * int(n_workers) + int(w)) * int(d) + int(i) + 1)) & _M64


QGADMM_CLAMP_K = 8   # iterations of a missing-clamp case: the clamp acts in the first


def qgadmm_clamp_case(n, m, d, bits, path=None):
    """``(X, y, rho, QReference, (data offset, worker, coordinate, low))`` of the missing-clamp case of a
    shape: data and seed chosen so that IN THE FIRST ITERATION the clamp of a head acts. A head's first
    solve, ``Minv_w b_w``, depends on no draw; the case needs a head whose largest coordinate is positive
    (``diff = +R``) and whose ``c`` is L exactly in float64, so that ``c + (1 - 2^-53)`` rounds to L + 1
    (about every third head: it turns on how ``2R / L`` rounds). The data is
    ``make_linear(n, m, d, seed_of(n, m, d) + t)`` for the first t = 0, 1, ... that has such a head (the
    first along the chain), the seed ``q_seed_drawing_top(low, 1, n, w, d, i)`` for the first ``low``
    at which the case is comparable (identical codes in long double and float64, margin >=
    QGADMM_MARGIN b_theta) over QGADMM_CLAMP_K iterations. The long-double run needs no clamp there
    (``L + 1 - 2^-53`` is a long double: its floor is L), the float64 run does, and both give L."""
    path_l = list(range(n)) if path is None else [int(w) for w in path]
    top = np.float64(1.0) - 2.0 ** -53

    def build():
        for t in range(64):
            X, y, rho = make_linear(n, m, d, seed_of(n, m, d) + t)
            A, b, _ = _gram(X, y, np.float64)
            for pos in range(0, n, 2):
                w = path_l[pos]
                th = spd_inverse(A[w] + ((pos > 0) + (pos < n - 1)) * rho * np.eye(d), np.float64) @ b[w]
                i = int(np.argmax(np.abs(th)))
                u = np.zeros(d)
                u[i] = top
                if th[i] > 0 and q_line(th, np.zeros(d), u, bits, np.float64, clamp=False)[1][i] == (1 << bits):
                    for low in range(2048):
                        seed = q_seed_drawing_top(low, 1, n, w, d, i)
                        out = _qgadmm_reference(n, m, d, bits, QGADMM_CLAMP_K, path, seed, data=t)
                        if out[3].codes_agree and out[3].margin >= QGADMM_MARGIN * out[3].b_theta:
                            return out + ((t, w, i, low),)
        raise AssertionError("no missing-clamp case for %r" % ((n, m, d, bits, path),))
    return _cached(("qgadmm-clamp", n, m, d, bits, None if path is None else tuple(path_l)), build)


# ------------------------------------------------------------------------------------------------
# The block-packed symmetric GEMV (csrc/include/sym_gemv.h; tests/test_gpu_symv_exact.py). Integer
# data: M symmetric and x with entries in [-2^19, 2^19], so every partial sum of every product of up to
# 8193 terms stays below 8193 * 2^38 < 2^53 -- every FMA and every addition of a float64 evaluation is
# exact IN ANY ORDER, and the kernel's output must equal the int64 product bit for bit.
SYMV_B = 128      # block edge (symv::B)
SYMV_RG = 8       # groups of partials per block row (symv::RG)
SYMV_LOADS = 8    # partials a reduce_row thread loads per trip of its loop
SYMV_AMP = 2 ** 19
SYMV_MAX_D = 8193  # SYMV_MAX_D * SYMV_AMP^2 < 2^53
# d -> what it is the smallest d to reach (tests/test_gpu_symv_exact.py)
SYMV_SHAPES = (1, 127, 128, 129, 255, 256, 257, 1024, 1025, 8193)
SYMV_MUTANTS = ("drop-transposed", "clip-8", "wrong-x-block")
assert SYMV_MAX_D * SYMV_AMP ** 2 < 2 ** 53


def symv_int_data(d, seed=0, count=1):
    """``(M (count, d, d) int32 symmetric, x (count, d) int64, y (count, d) int64 = M x)``, entries of M
    and x uniform in [-SYMV_AMP, SYMV_AMP]; the product is formed in int64, row chunk by row chunk."""
    assert 1 <= d <= SYMV_MAX_D
    rng = np.random.default_rng(7919 * d + seed)
    M = rng.integers(-SYMV_AMP, SYMV_AMP + 1, size=(count, d, d), dtype=np.int32)
    for c in range(count):
        low = np.tril(M[c], -1)
        M[c] = np.tril(M[c])
        M[c] += low.T
    x = rng.integers(-SYMV_AMP, SYMV_AMP + 1, size=(count, d), dtype=np.int64)
    y = np.zeros((count, d), dtype=np.int64)
    for c in range(count):
        for r0 in range(0, d, 1024):
            y[c, r0:r0 + 1024] = M[c, r0:r0 + 1024].astype(np.int64) @ x[c]
    return M, x, y


def symv_packed_model(M, x, mutant=None):
    """``M x`` (float64, (d,)) of one symmetric matrix the way sym_gemv.h forms it. Only the blocks (I, J),
    J <= I, of the B x B tiling are read (a diagonal block as the mirror of its lower half, the rest zero
    padded); block (I, J) gives the direct partial ``P[I][J] = M_IJ x_J`` and, off the diagonal, the
    transposed one ``P[J][I] = M_IJ' x_I``; block row t of the result is the sum of ``P[t][s]`` over s as
    ``reduce_row`` takes it: RG groups of ``per = ceil(nb / RG)`` consecutive s (the last one clipped at
    nb, later ones empty), each summed in trips of eight, then the group sums in group order. A partial
    nothing wrote is NaN, as in the GPU test's pre-filled work buffer.
    ``mutant`` names a mistake of the kernel (tests/test_hp_reference_cpu.py shows each one changes the
    result on the GPU test's data): ``"drop-transposed"`` the transposed product of the last stored
    off-diagonal block is never written; ``"clip-8"`` a group sums its first eight partials only (no
    second trip of the loop); ``"wrong-x-block"`` the direct product of block (1, 0) takes x's block 1
    instead of block 0."""
    assert mutant is None or mutant in SYMV_MUTANTS
    B = SYMV_B
    d = len(x)
    nb = (d + B - 1) // B
    xp = np.zeros(nb * B, dtype=np.float64)
    xp[:d] = x

    def stored(I, J):
        blk = np.zeros((B, B), dtype=np.float64)
        sub = M[I * B:(I + 1) * B, J * B:(J + 1) * B]
        blk[:sub.shape[0], :sub.shape[1]] = sub
        if I == J:
            blk = np.tril(blk) + np.tril(blk, -1).T
        return blk

    P = np.full((nb, nb, B), np.nan, dtype=np.float64)
    for I in range(nb):
        for J in range(I + 1):
            blk = stored(I, J)
            src = I if (mutant == "wrong-x-block" and (I, J) == (1, 0)) else J
            P[I, J] = blk @ xp[src * B:(src + 1) * B]
            if I != J and not (mutant == "drop-transposed" and (I, J) == (nb - 1, nb - 2)):
                P[J, I] = blk.T @ xp[I * B:(I + 1) * B]
    per = (nb + SYMV_RG - 1) // SYMV_RG
    out = np.zeros(nb * B, dtype=np.float64)
    for t in range(nb):
        y = np.zeros(B, dtype=np.float64)
        for g in range(SYMV_RG):
            s0, s1 = g * per, min(g * per + per, nb)
            acc = np.zeros(B, dtype=np.float64)
            for s in range(s0, s1, SYMV_LOADS):
                for u in range(SYMV_LOADS):
                    if s + u < s1:
                        acc = acc + P[t, s + u]
                if mutant == "clip-8":
                    break
            y = y + acc
        out[t * B:(t + 1) * B] = y
    return out[:d]
