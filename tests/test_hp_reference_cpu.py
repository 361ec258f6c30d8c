"""CPU tests of tests/hp_reference.py, the long-double reference of tests/test_gpu_dispatch_classes.py,
tests/test_gpu_dgadmm_classes.py, tests/test_gpu_newton_classes.py, tests/test_gpu_first_order_classes.py,
tests/test_gpu_setup_kernels.py, tests/test_gpu_qgadmm_classes.py and tests/test_gpu_symv_exact.py.

The helper is only worth trusting if its float64 / long-double runs reproduce the committed oracle
(gadmm_amd/oracle/reference.py) on every shape the GPU tests use: here the oracle stands where a
kernel stands there, held to the same bound ``8 * max(e64, max(d, m, 16) * 2^-53)``. The exact-prox
recurrence, which the oracle does not have, is held against the torch Newton path instead."""
import numpy as np
import pytest

import hp_reference as H
from gadmm_amd.oracle import reference as R

K = H.K_ITERS


def _check(tag, ref, theta, dual, obj):
    rt, rd, ro = ref.err_theta(theta) / ref.b_theta, ref.err_dual(dual) / ref.b_dual, ref.err_obj(obj) / ref.b_obj
    print("%s: err/bound theta %.3f dual %.3f objective %.3f (e64 %.2e %.2e %.2e)"
          % (tag, rt, rd, ro, ref.e_theta, ref.e_dual, ref.e_obj))
    assert rt <= 1.0 and rd <= 1.0 and ro <= 1.0, (tag, rt, rd, ro)


def _oracle_logistic(monkeypatch, X, y, rho, lam, step, iters, max_inner, inner_tol):
    """The oracle's own GADMM loop and inner solver, with the inner solver's cap and tolerance (its
    ``gadmm_logistic_gd`` does not forward them) set to the case's."""
    inner = R.logreg_gd
    monkeypatch.setattr(R, "logreg_gd", lambda *a: inner(*a, max_inner=max_inner, tol=inner_tol))
    return R.gadmm_logistic_gd(X, y, rho, iters, 0.0, lam, 0.0, step)


@pytest.mark.parametrize("n,m,d", H.LINEAR_SHAPES)
def test_gadmm_linear_reproduces_oracle(n, m, d):
    X, y, rho, ref = H.linear_case(n, m, d)
    o = R.gadmm_linear(X, y, rho, K, 0.0, 0.0)
    assert o.iters == K and len(o.obj) == K
    _check("linear %s" % ((n, m, d),), ref, o.theta, H.edge_to_worker_duals(o.dual), o.obj)
    # the per-worker form of the oracle (no re-chaining) is the same recurrence
    o2 = R.dgadmm_linear(X, y, rho, K, 0.0, 0.0, list(range(n)), np.zeros(max(n - 1, 0)), 0)
    _check("linear (per-worker duals) %s" % ((n, m, d),), ref, o2.theta, o2.dual, o2.obj)


@pytest.mark.parametrize("n,m,d", H.STAR_SHAPES)
def test_star_admm_reproduces_oracle(n, m, d):
    X, y, rho, ref = H.star_case(n, m, d)
    o = R.std_admm_linear(X, y, rho, K, 0.0, 0.0)
    assert np.all(ref.dual[n - 1] == 0)
    _check("star %s" % ((n, m, d),), ref, o.theta, o.dual, o.obj)


@pytest.mark.parametrize("n,m,d", H.LOGISTIC_SHAPES)
def test_gadmm_logistic_reproduces_oracle(n, m, d, monkeypatch):
    X, y, rho, lam, step, ref = H.logistic_case(n, m, d)
    inner, margin = ref.extra
    assert np.all(inner == H.MAX_INNER) and margin == np.inf  # inner_tol = 0: no test can pass
    o = _oracle_logistic(monkeypatch, X, y, rho, lam, step, K, H.MAX_INNER, 0.0)
    _check("logistic %s" % ((n, m, d),), ref, o.theta, H.edge_to_worker_duals(o.dual), o.obj)


def test_logistic_live_stop_margin(monkeypatch):
    """Every logistic case with ``inner_tol > 0``: no stop test of the long-double run comes within
    1e-6 (relative) of its threshold, so a correct float64 kernel takes the same decisions. A seed that
    fails this is replaced, the margin is not loosened."""
    (n, m, d), tol = H.LIVE_STOP
    X, y, rho, lam, step, ref = H.logistic_case(n, m, d, inner_tol=tol)
    inner, margin = ref.extra
    print("live stop %s: margin %.3e, inner steps of the last iteration %s" % ((n, m, d), margin, inner[-1]))
    assert margin > 1e-6
    assert inner.min() < H.MAX_INNER and inner.max() == H.MAX_INNER  # the rule is live, and so is the cap
    f64 = H.gadmm_logistic_gd(X, y, rho, lam, step, K, H.MAX_INNER, tol, np.float64)
    assert np.array_equal(f64[3], inner)
    o = _oracle_logistic(monkeypatch, X, y, rho, lam, step, K, H.MAX_INNER, tol)
    _check("logistic live stop", ref, o.theta, H.edge_to_worker_duals(o.dual), o.obj)


def test_fixtures_reproduce_oracle(lin24, log24):
    """The suite's own fixtures (N = 24, m = d = 50), 30 iterations, the oracle's default inner solver
    (100 steps, 1e-4)."""
    X, y = lin24.numpy()
    rho = 5.0
    ref = H.Reference(H.gadmm_linear(X, y, rho, 30, H.LD), H.gadmm_linear(X, y, rho, 30, np.float64), rho, 50)
    o = R.gadmm_linear(X, y, rho, 30, 0.0, 0.0)
    _check("lin24", ref, o.theta, H.edge_to_worker_duals(o.dual), o.obj)
    ref = H.Reference(H.star_admm_linear(X, y, 1.0, 30, H.LD), H.star_admm_linear(X, y, 1.0, 30, np.float64), 1.0, 50)
    o = R.std_admm_linear(X, y, 1.0, 30, 0.0, 0.0)
    _check("lin24 star", ref, o.theta, o.dual, o.obj)
    X, y = log24.numpy()
    args = (X, y, 2e-4, 1e-5, 2.2, 30, 100, 1e-4)
    ld, f64 = H.gadmm_logistic_gd(*args, H.LD), H.gadmm_logistic_gd(*args, np.float64)
    ref = H.Reference(ld, f64, 2e-4, 50, 50)
    assert ld[4] > 1e-6 and np.array_equal(ld[3], f64[3])
    o = R.gadmm_logistic_gd(X, y, 2e-4, 30, 0.0, 1e-5, 0.0, 2.2)
    _check("log24", ref, o.theta, H.edge_to_worker_duals(o.dual), o.obj)


# ------------------------------------------------------------------------------------------------
# Exact local solves (tests/test_gpu_newton_classes.py). The oracle has no exact-prox variant
# (gadmm_amd/oracle/reference.py: inner gradient descent only), so the project's own torch path
# stands where a kernel stands: it solves H dx = g by LU where the reference applies an explicit
# inverse, and batches a phase's workers (all of them step until the slowest has converged).
@pytest.mark.parametrize("n,m,d", H.NEWTON_SHAPES)
def test_gadmm_logistic_newton_reproduces_torch_path(n, m, d):
    import torch
    from gadmm_amd.algorithms import chain_admm
    from gadmm_amd.models import LogisticRegression
    ref = H.newton_case(n, m, d)
    model = LogisticRegression(torch.from_numpy(np.array(ref.X)), torch.from_numpy(np.array(ref.y)), lam=ref.lam)
    a = chain_admm(model, list(range(n)), n, ref.rho, 0.0, 1e-300, K, local_solver="newton", backend="torch")
    assert a.extra["backend"] == "torch" and a.iters == K and len(a.obj) == K
    theta, mu, nxt = a.extra["state"]
    assert nxt == K + 1
    _check("newton %s" % ((n, m, d),), ref, theta.numpy(), mu.numpy(), a.obj)


@pytest.mark.parametrize("n,m,d", H.NEWTON_SHAPES)
def test_newton_reference_noise_and_steps(n, m, d):
    """The bound means something only while the noise under it is small: e64 of every quantity stays
    below 64 * 2^-53 * max(d, m, 16) (measured 1.5e-16 .. 1.1e-15, profiles/newton_classes). Exact
    Newton from the worker's last iterate takes 3 .. 7 steps; no solve, at any tested chord threshold,
    comes near the cap of 50, where the kernels would report inner_fail."""
    ref = H.newton_case(n, m, d)
    lim = 64 * 2.0 ** -53 * max(d, m, 16)
    print("newton %s: e64 theta %.2e dual %.2e objective %.2e (limit %.2e), steps %d..%d (float64 %d..%d)"
          % ((n, m, d), ref.e_theta, ref.e_dual, ref.e_obj, lim, ref.extra[0].min(), ref.extra[0].max(),
             ref.steps64.min(), ref.steps64.max()))
    assert ref.e_theta <= lim and ref.e_dual <= lim and ref.e_obj <= lim
    assert ref.truncation == 0.0 and ref.b_theta == H.bound(ref.e_theta, d, m)
    for steps in (ref.extra[0], ref.steps64):
        assert steps.shape == (K, n) and 2 <= steps.min() and steps.max() <= 12
    for c in H.NEWTON_CHORDS[1:]:
        rc = H.newton_case(n, m, d, chord=c)
        print("  chord %.2f: e_chord theta %.2e dual %.2e objective %.2e, truncation %.2e, steps %d..%d"
              % (c, rc.e_theta, rc.e_dual, rc.e_obj, rc.truncation, rc.steps64.min(), rc.steps64.max()))
        assert rc.steps64.min() >= 1 and rc.steps64.max() < H.NEWTON_MAX
        assert rc.theta is ref.theta or np.array_equal(rc.theta, ref.theta)  # one long-double run serves all
        assert rc.truncation >= c / (1 - c) * H.NEWTON_TOL and rc.b_theta >= 8 * rc.truncation
        assert max(rc.b_theta, rc.b_dual, rc.b_obj) < 1e-12  # still ten orders below an indexing mistake


@pytest.mark.parametrize("n,m,d", [(2, 1, 1), (5, 36, 34), (3, 64, 64)])
def test_newton_bound_catches_one_wrong_coordinate(n, m, d):
    """One coordinate of one worker's theta off by 1e-9 of max|theta| lands above the chord-0 bound,
    off by 1e-10 above the (wider) bound at chord 0.3; the float64 runs themselves, correct by
    construction, land below 1/8 of it."""
    X, y, rho, lam, _ = H.make_logistic(n, m, d, H.seed_of(n, m, d))
    for c, off in ((0.0, 1e-9), (0.3, 1e-10)):
        ref = H.newton_case(n, m, d, chord=c)
        th64 = H.gadmm_logistic_newton(X, y, rho, lam, K, np.float64, H.NEWTON_TOL, c)[0][-1]
        assert ref.err_theta(th64) <= ref.b_theta / 8
        bad = np.array(th64)
        bad[n - 1, d - 1] += off * ref.scale_theta
        ratio = ref.err_theta(bad) / ref.b_theta
        print("newton %s chord %.1f: one coordinate off by %.0e -> err / bound %.1f" % ((n, m, d), c, off, ratio))
        assert ratio > 1.0


def test_newton_reference_api():
    X, y, rho, lam, _ = H.make_logistic(3, 5, 3, 1)
    th, mu, ob, steps = H.gadmm_logistic_newton(X, y, rho, lam, 4)
    assert th.dtype == mu.dtype == ob.dtype == H.LD and th.shape == (4, 3, 3) and mu.shape == (3, 3)
    assert ob.shape == (4,) and steps.shape == (4, 3)
    assert np.max(np.abs(mu.sum(axis=0))) < 1e-17 * float(np.max(np.abs(mu)) + 1)  # the duals sum to zero
    with pytest.raises(ValueError):
        H.gadmm_logistic_newton(X, y, rho, lam, 2, H.LD, 1e-17, 0.3)
    # a run to iteration k is a prefix of a longer one: what newton_case(K = last) relies on
    a, b = H.newton_case(3, 5, 3, K + 3), H.newton_case(3, 5, 3)
    assert np.array_equal(a.theta[:K], b.theta) and np.array_equal(a.obj[:K], b.obj) and a.theta.shape[0] == K + 3
    th2, mu2, _, _ = H.gadmm_logistic_newton(b.X, b.y, b.rho, b.lam, K)
    assert np.array_equal(th2, b.theta) and np.array_equal(mu2, b.dual)
    assert H.bound(0.0, 3, 5, 1e-14) == 8e-14 and H.chord_truncation(0.0, 2.0) == 0.0
    assert abs(H.chord_truncation(0.3, 0.5) - 0.3 / 0.7 * 1e-13 / 0.5) < 1e-28


@pytest.mark.parametrize("d", [1, 64, 256])
def test_newton_schulz_inverse(d):
    rng = np.random.default_rng(d)
    Z = rng.standard_normal((2 * d, d))
    M = (Z.T @ Z + 0.5 * d * np.eye(d)).astype(H.LD)
    Xi = H.spd_inverse(M, H.LD)
    assert Xi.dtype == H.LD
    resid = float(np.max(np.abs(np.eye(d, dtype=H.LD) - M @ Xi)))
    print("d=%d: |I - M X|_max = %.3e (bound %.3e)" % (d, resid, d * 2.0 ** -60))
    assert resid <= d * 2.0 ** -60
    assert H.spd_inverse(M.astype(np.float64), np.float64).dtype == np.float64


def test_dtypes_and_noise_level():
    X, y, rho = H.make_linear(3, 7, 3, 1)
    for fn in (H.gadmm_linear, H.star_admm_linear):
        for dt in (np.float64, H.LD):
            th, du, ob = fn(X, y, rho, 3, dt)
            assert th.dtype == du.dtype == ob.dtype == np.dtype(dt) and th.shape == (3, 3, 3)
    X, y, rho, lam, step = H.make_logistic(3, 5, 3, 1)
    assert set(np.unique(y)) <= {-1.0, 1.0} and lam == 1e-3 and abs(rho * step - 0.1) < 1e-15
    th, du, ob, inner, margin = H.gadmm_logistic_gd(X, y, rho, lam, step, 2, 4, 0.0, H.LD)
    assert th.dtype == H.LD and inner.shape == (2, 3) and np.all(inner == 4) and margin == np.inf
    assert H.noise_level(np.array([1.0, 2.0]), np.array([1.0, 2.5]), 2.0) == 0.25
    assert H.noise_level(np.array([1.0, 2.0]), np.array([1.5, 2.5]), np.array([1.0, 2.0])) == 0.5
    assert H.bound(0.0, 3) == 8 * 16 * 2.0 ** -53 and H.bound(0.0, 40, 250) == 8 * 250 * 2.0 ** -53
    assert H.bound(1e-15, 257) == 8 * 257 * 2.0 ** -53 and H.bound(1e-13, 257) == 8e-13


@pytest.mark.parametrize("n,m,d", [(2, 3, 1), (5, 60, 52), (3, 280, 257)])
def test_bound_catches_what_a_wrong_kernel_does(n, m, d):
    """The bound is far below anything an indexing or tail mistake produces: one theta coordinate off
    by 1e-11 relative (the suite's older rtol), or a solve whose last shard column of one worker is
    wrong in the ninth digit, both land above it in every quantity; the float64 run of the recurrence
    itself, a correct implementation by construction, lands below."""
    X, y, rho, ref = H.linear_case(n, m, d)
    th64, mu64, ob64 = H.gadmm_linear(X, y, rho, K, np.float64)
    assert ref.err_theta(th64[-1]) <= ref.b_theta / 8 and ref.err_obj(ob64) <= ref.b_obj / 8
    off = np.array(th64[-1])
    off[0, d - 1] += 1e-11 * ref.scale_theta
    assert ref.err_theta(off) > ref.b_theta
    Xb = np.array(X)
    Xb[0, :, d - 1] *= 1.0 + 1e-9  # the last column of worker 0's shard, nine digits in
    thb, mub, obb = H.gadmm_linear(Xb, y, rho, K, np.float64)
    assert ref.err_theta(thb[-1]) > ref.b_theta and ref.err_dual(mub) > ref.b_dual and ref.err_obj(obb) > ref.b_obj


# ------------------------------------------------------------------------------------------------
# D-GADMM (tests/test_gpu_dgadmm_classes.py): the re-chaining recurrence against the static one, the
# oracle and the torch path over the same prescribed chains; the host's epoch tables against the
# neighbours, roles and flush pairs the reference derives; and the power of the bound against three
# wrong re-chains.
DGADMM_CASES = H.dgadmm_cases()
DGADMM_POWER = 1000.0


@pytest.mark.parametrize("n,m,d", [(2, 3, 1), (5, 60, 52), (3, 80, 65)])
def test_dgadmm_single_identity_epoch_is_gadmm(n, m, d):
    """One epoch on the identity chain: the operations of ``gadmm_linear`` in its order, bit for bit."""
    X, y, rho = H.make_linear(n, m, d, H.seed_of(n, m, d))
    for dtype in (H.LD, np.float64):
        a = H.dgadmm_linear(X, y, rho, K, [(1, list(range(n)))], dtype)
        b = H.gadmm_linear(X, y, rho, K, dtype)
        assert all(u.dtype == dtype and np.array_equal(u, v) for u, v in zip(a, b))


def test_dgadmm_chains_are_prescribed():
    from gadmm_amd.parallel.topology import rechain_iterations
    for n, _, _, coh in DGADMM_CASES:
        chains = H.dgadmm_chains(n, K, coh)
        assert chains == H.dgadmm_chains(n, K, coh)  # deterministic
        assert [f for f, _ in chains] == [1] + [int(v) for v in rechain_iterations(K, coh)]
        assert all(sorted(p) == list(range(n)) for _, p in chains) and chains[0][1] != list(range(n))
        assert any(a[1] != b[1] for a, b in zip(chains, chains[1:]))
    # the cycle at even and at odd n, and what each move does to the roles
    c4, c5 = H.dgadmm_chains(4, K, 3), H.dgadmm_chains(5, K, 3)
    assert c4[1][1] == c4[0][1][::-1] and c4[2][1] == c4[1][1][1:] + c4[1][1][:1] and c4[3][1] == c4[2][1]
    assert c5[1][1] == c5[0][1][1:] + c5[0][1][:1] and c5[2][1] == c5[1][1] and c5[4][1] == c5[3][1][::-1]
    t = H.chain_tables(c5[:2])
    first = c5[0][1][0]
    assert t[0][1][first][:2] == (0, None) and t[1][1][first][0] == 4 and t[1][1][first][2] is None
    assert all((t[0][1][w][0] + t[1][1][w][0]) % 2 == 1 for w in range(5) if w != first)  # every other role flips
    assert H.flush_pairs(c5[:2])[1] == {w: v[1:] for w, v in t[0][1].items() if v[0] % 2 == 0}


@pytest.mark.parametrize("n,m,d,coh", DGADMM_CASES)
def test_dgadmm_reproduces_oracle_and_torch_path(n, m, d, coh):
    """The oracle's D-GADMM, fed the prescribed chains through its ``rechain`` callback, and the torch
    path, fed them as a path matrix, are within the case's bound of the long-double run."""
    import torch
    from gadmm_amd.algorithms import dynamic_group_admm_v0
    from gadmm_amd.models import LinearRegression
    X, y, rho, chains, ref = H.dgadmm_case(n, m, d, coh)
    assert ref.theta.dtype == H.LD and ref.theta.shape == (K, n, d) and ref.obj.shape == (K,)
    by_it = {f: p for f, p in chains}
    ones = np.ones(max(n - 1, 0))
    o = R.dgadmm_linear(X, y, rho, K, 0.0, 0.0, chains[0][1], ones, coh, lambda it: (by_it[it], ones))
    assert o.iters == K and len(o.obj) == K
    _check("D-GADMM oracle %s coh %s" % ((n, m, d), coh), ref, o.theta, o.dual, o.obj)
    P, C = H.dgadmm_matrices(chains)
    model = LinearRegression(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(y)))
    a = dynamic_group_admm_v0(model, rho, 0.0, 0.0, K, P, C, coh, faithful_initial_cost=False, backend="torch")
    theta, mu, nxt = a.extra["state"]
    assert a.extra["backend"] == "torch" and a.iters == K and nxt == K + 1 and len(a.obj) == K
    _check("D-GADMM torch %s coh %s" % ((n, m, d), coh), ref, theta.numpy(), mu.numpy(), a.obj)


def _epoch_expectation(chains):
    """(slots (E, n, 4), positions (E, n), flush (E, n, 2)) in the layout of ``epoch_tables_numpy`` (local
    workers 0..n-1) and ``epoch_flush_table`` from the reference's own tables, by plain loops."""
    tabs, fl = H.chain_tables(chains), H.flush_pairs(chains)
    E, n = len(tabs), len(tabs[0][1])
    slots = np.zeros((E, n, 4), dtype=np.int32)
    pos = np.zeros((E, n), dtype=np.int32)
    flush = np.full((E, n, 2), -1, dtype=np.int32)
    for e, (_, tab) in enumerate(tabs):
        for w, (p, l, r) in tab.items():
            slots[e, w] = (w, w, -1 if l is None else l, -1 if r is None else r)
            pos[e, w] = p
            if w in fl[e]:
                flush[e, p] = [-1 if v is None else v for v in fl[e][w]]
    return slots, pos, flush


@pytest.mark.parametrize("n,coh", sorted({(c[0], c[3]) for c in DGADMM_CASES}))
def test_epoch_tables_agree_with_the_reference(n, coh):
    """The tables the dynamic kernels read (engine/chain_engine.py: ``epoch_tables_numpy``,
    ``epoch_flush_table``; csrc/runtime/topology.cpp: ``gadmm_epoch_tables``,
    ``gadmm_epoch_tables_blocked`` where the library is already built) against the neighbours, roles and
    old-chain flush pairs of the reference's chains."""
    from gadmm_amd.engine.chain_engine import epoch_flush_table, epoch_tables_numpy
    from gadmm_amd.ops import native
    chains = H.dgadmm_chains(n, K, coh)
    slots, pos, flush = _epoch_expectation(chains)
    P = np.ascontiguousarray(H.dgadmm_matrices(chains)[0])
    E = len(chains)
    loc = np.arange(n, dtype=np.int64)
    s_np, p_np = epoch_tables_numpy(P, loc)
    assert np.array_equal(s_np, slots) and np.array_equal(p_np, pos)
    assert np.array_equal(epoch_flush_table(P), flush)
    sub = loc[::2].copy()  # a rank that holds every other worker
    s_sub, p_sub = epoch_tables_numpy(P, sub)
    assert np.array_equal(s_sub[:, :, 1:], slots[:, ::2, 1:]) and np.array_equal(p_sub, pos[:, ::2])
    assert np.array_equal(s_sub[:, :, 0], np.broadcast_to(np.arange(len(sub)), (E, len(sub))))
    lib = native.load(build_if_missing=False)
    if lib is None or getattr(lib, "gadmm_epoch_tables_blocked", None) is None:
        return  # the native builders are held to the same tables wherever the library is built
    es, pp = np.empty((E * n * 4,), dtype=np.int32), np.empty((E * n,), dtype=np.int32)
    assert lib.gadmm_epoch_tables(P.ctypes.data, E, n, loc.ctypes.data, n, es.ctypes.data, pp.ctypes.data) == 0
    assert np.array_equal(es.reshape(E, n, 4), slots) and np.array_equal(pp.reshape(E, n), pos)
    fl = np.empty((E * n * 2,), dtype=np.int32)
    assert lib.gadmm_epoch_tables_blocked(P.ctypes.data, E, n, es.ctypes.data, pp.ctypes.data, fl.ctypes.data) == 0
    # the blocked tables are in chain-position order: slot p is the worker at position p
    by_pos = np.take_along_axis(slots, P[:, :, None].astype(np.int64), axis=1)
    assert np.array_equal(es.reshape(E, n, 4), by_pos) and np.array_equal(pp.reshape(E, n), pos)
    assert np.array_equal(fl.reshape(E, n, 2), flush)


@pytest.mark.parametrize("n,m,d,coh", DGADMM_CASES)
def test_dgadmm_bound_rejects_a_wrong_rechain(n, m, d, coh):
    """Power of the GPU tests, as a condition on the reference alone: a float64 run that ignores the
    re-chains, one that applies the heads' pending dual with the NEW chain's neighbours, and one that
    takes the OLD degree's inverse in the first solve after a re-chain each sit at least 1000 bounds
    from the reference in some compared quantity (the last two are defined from three workers on: with
    two, every chain has the same neighbours and degrees). The float64 run itself sits below 1/8."""
    X, y, rho, chains, ref = H.dgadmm_case(n, m, d, coh)

    def ratios(run):
        th, mu, ob = run
        return (ref.err_theta(th[-1]) / ref.b_theta, ref.err_dual(mu) / ref.b_dual, ref.err_obj(ob) / ref.b_obj)

    assert max(ratios(H.dgadmm_linear(X, y, rho, K, chains, np.float64))) <= 1.0 / 8
    for mutant in H.DGADMM_MUTANTS if n >= 3 else H.DGADMM_MUTANTS[:1]:
        r = ratios(H.dgadmm_linear(X, y, rho, K, chains, np.float64, mutant=mutant))
        print("D-GADMM %s coh %s mutant %-10s: err/bound theta %.2e dual %.2e objective %.2e"
              % ((n, m, d), coh, mutant, *r))
        assert max(r) >= DGADMM_POWER, (mutant, r)


# ------------------------------------------------------------------------------------------------
# First-order baselines (tests/test_gpu_first_order_classes.py). The references follow the torch path
# (gadmm_amd/algorithms/baselines.py, dual_averaging.py), so the torch path on the CPU stands where a
# kernel stands; dual averaging is also held against the oracle. Then the conditions on the inputs
# that entitle the GPU tests to what they assert: LAG decisions far from a tie and of every kind,
# float64 noise small enough for the bound to reject anything, and bounds that do reject.
FO_CASES = [("linear",) + s for s in H.FO_LINEAR_SHAPES + [H.FO_LINEAR_WIDE] + H.FO_BIG_SHAPES] + \
           [("logistic",) + s for s in H.FO_LOGISTIC_SHAPES]
FO_UNFAITHFUL = [("linear", 3, 7, 3), ("logistic", 3, 5, 3)]
FO_ALL = [c + (True,) for c in FO_CASES] + [c + (False,) for c in FO_UNFAITHFUL]
FO_NOISE_CAP = 1e-12
FO_MARGIN = 1e-9


def _fo_torch(case):
    """The torch path on the CPU with the case's own constants: ``(objective trace, per-iteration
    upload counts or None, uploads or None)``."""
    import torch
    from gadmm_amd.algorithms import gradient_descent, decentralized_gd, lag, iag, dual_averaging
    from gadmm_amd.models import LinearRegression, LogisticRegression
    X, y = torch.from_numpy(np.array(case.X)), torch.from_numpy(np.array(case.y))
    model = LinearRegression(X, y) if case.kind == "linear" else LogisticRegression(X, y, lam=case.lam)
    n, K, s, f = case.n, case.K, case.step0, case.faithful
    ids, hmax, v = list(range(n)), torch.from_numpy(np.array(case.hmax)), case.variant
    if v == "GD":
        r = gradient_descent(model, ids, n, K, 0.0, s, faithful=f, backend="torch")
    elif v == "DGD":
        r = decentralized_gd(model, ids, n, K, 0.0, s, faithful=f, backend="torch")
    elif v.startswith("LAG"):
        r = lag(model, ids, n, K, 0.0, s, hmax, v[4:], faithful=f, backend="torch")
        comm = r.comm_units - np.arange(1, K + 1)  # 1 + the running upload count (no quiet unit: K < 1000)
        return r.obj, np.diff(np.concatenate([[1.0], comm])), r.extra["uploads"]
    elif v.endswith("IAG"):
        r = iag(model, ids, n, K, 0.0, s, "cyclic" if v == "cIAG" else "random", hmax, 7, faithful=f, backend="torch")
    else:
        r = dual_averaging(model, ids, n, s, 0.0, 0.0, K, jacobi=v.endswith("-J"), backend="torch")
    return r.obj, None, None


@pytest.mark.parametrize("kind,n,m,d,faithful", FO_ALL)
def test_first_order_reproduces_torch_path(kind, n, m, d, faithful):
    for alg in H.fo_algs(n):
        c = H.first_order_case(kind, alg, n, m, d, faithful=faithful)
        obj, cnt, uploads = _fo_torch(c)
        assert len(obj) == c.K == H.FO_K
        r_ld = c.err_obj(obj) / c.b_obj
        r_64 = H.noise_level(c.f64["obj"], obj, np.abs(c.obj)) / c.b_obj
        print("%s %s %s faithful=%d: torch path err/bound objective %.3f (float64 run %.3f)"
              % (kind, (n, m, d), alg, faithful, r_ld, r_64))
        assert r_ld <= 1.0 and r_64 <= 1.0, (alg, r_ld, r_64)
        if cnt is not None:
            assert np.array_equal(cnt, c.f64["cnt"]) and np.array_equal(cnt, c.cnt), alg
            assert uploads == c.uploads == float(c.f64["cnt"].sum()), alg
    if n >= 2:  # the oracle's sweep reads Z[1]: no n = 1
        c = H.first_order_case(kind, "DualAvg", n, m, d, faithful=faithful)
        o = R.dual_averaging(np.array(c.X), np.array(c.y), c.K, 0.0, 0.0, c.step0,
                             logistic_eta=c.lam if kind == "logistic" else None)
        ro, rt = c.err_obj(np.asarray(o.obj)) / c.b_obj, c.err_theta(o.theta) / c.b_theta
        print("%s %s DualAvg: oracle err/bound objective %.3f theta %.3f" % (kind, (n, m, d), ro, rt))
        assert len(o.obj) == c.K and ro <= 1.0 and rt <= 1.0, (ro, rt)


@pytest.mark.parametrize("kind,n,m,d,faithful", FO_ALL)
def test_first_order_inputs_entitle_the_assertions(kind, n, m, d, faithful):
    """Conditions on the inputs, not measurements. Every case: the float64 noise of every quantity is at
    most 1e-12 (above that a bound rejects nothing; LAG-WK at n = 1 is left out for this, see
    ``hp_reference.fo_algs``). Every LAG case: (a) the long-double and the float64 run take identical
    masks, (b) no decision of the long-double run comes within 1e-9 (relative) of its threshold, so a
    correct float64 kernel takes the same decisions and the GPU test may ask for equal counts, (c) after
    iteration 10 some iteration uploads nothing and some uploads, (d) at n >= 33 some iteration uploads a
    proper subset of the workers. A case that fails gets another seed offset
    (``hp_reference.FO_SEED_OFFSET``), nothing is widened."""
    for alg in H.fo_algs(n):
        c = H.first_order_case(kind, alg, n, m, d, faithful=faithful)
        print("%s %s %s faithful=%d: e64 objective %.2e theta %.2e%s"
              % (kind, (n, m, d), alg, faithful, c.e_obj, c.e_theta,
                 "" if c.cnt is None else ", margin %.2e, uploads %d" % (c.margin, c.uploads)))
        assert c.e_obj <= FO_NOISE_CAP and c.e_theta <= FO_NOISE_CAP, (alg, c.e_obj, c.e_theta)
        assert c.obj.dtype == H.LD and c.theta.dtype == H.LD and c.f64["obj"].dtype == np.float64
        assert c.theta.shape == ((n, d) if alg in ("DGD", "DualAvg", "DualAvg-J") else (d,))
        if c.cnt is None:
            continue
        assert np.array_equal(c.mask, c.f64["mask"]), alg                         # (a)
        assert c.margin >= FO_MARGIN, (alg, c.margin)                              # (b)
        assert np.all(c.cnt[:10] == 0)
        late = c.cnt[10:]
        assert np.any(late == 0) and np.any(late > 0), alg                         # (c)
        if n >= 33:
            assert np.any((late > 0) & (late < n)), alg                            # (d)


def test_first_order_lag_wk_single_worker_is_left_out():
    """Linear (1, 5, 3) LAG-WK misses the noise cap by orders of magnitude: it is not in ``fo_algs(1)``."""
    assert "LAG-WK" not in H.fo_algs(1) and "LAG-WK" in H.fo_algs(2) and len(H.fo_algs(2)) == 8
    assert "cIAG" not in H.fo_algs(65) and "R-IAG" in H.fo_algs(65) and "cIAG" in H.fo_algs(33)
    c = H.first_order_case("linear", "LAG-WK", 1, 5, 3)
    print("linear (1, 5, 3) LAG-WK: e64 objective %.2e theta %.2e" % (c.e_obj, c.e_theta))
    assert max(c.e_obj, c.e_theta) > FO_NOISE_CAP


@pytest.mark.parametrize("kind,alg,n,m,d", [("linear", "GD", 5, 70, 64), ("logistic", "LAG-WK", 4, 70, 60),
                                            ("linear", "DualAvg", 3, 150, 128)])
def test_first_order_bounds_reject_a_wrong_kernel(kind, alg, n, m, d):
    """The float64 run, correct by construction, sits below 1/8 of the bounds; one coordinate of the
    final theta, or one trace entry, off by 1e-9 relative lands above them; a step-history entry of LAG
    off by a factor 2 (a stale or overwritten slot of the kernels' ring) changes the upload counts."""
    c = H.first_order_case(kind, alg, n, m, d)
    th, obj = np.array(c.f64["theta"]), np.array(c.f64["obj"])
    assert c.err_theta(th) <= c.b_theta / 8 and c.err_obj(obj) <= c.b_obj / 8
    th.reshape(-1)[-1] += 1e-9 * c.scale_theta
    obj[c.K // 2] *= 1.0 + 1e-9
    rt, ro = c.err_theta(th) / c.b_theta, c.err_obj(obj) / c.b_obj
    print("%s %s %s: off by 1e-9 -> err/bound theta %.1f objective %.1f" % (kind, (n, m, d), alg, rt, ro))
    assert rt > 1.0 and ro > 1.0
    if c.cnt is not None:
        bad = H.first_order(c.alg, c.X, c.y, c.K, kind=kind, lam=c.lam, dtype=np.float64, scale_history=(20, 2.0),
                            **c.args)
        assert np.array_equal(bad["cnt"][:20], c.cnt[:20]) and not np.array_equal(bad["cnt"], c.cnt)


@pytest.mark.parametrize("alg,n,m,d,faithful", H.FO_LIVE_STOP)
def test_first_order_live_stop_is_decided(alg, n, m, d, faithful):
    """The live stop rule of the GPU tests (``fo_live_stop``): the gaps to the last objective decrease
    strictly up to iteration 40, the two gaps around the tolerance differ by more than 1e-6 relative, and
    the tolerance sits further from both than the objective bound reaches, so ``|obj - obj0| < tol`` first
    holds at iteration 40 in any run within the bound. (GD and DGD run with ``faithful=False``: the
    faithful first step along ones moves away from the optimum, the gap of iteration 2 is above that of 1.)"""
    c = H.first_order_case("linear", alg, n, m, d, faithful=faithful)
    obj0, tol, gaps = H.fo_live_stop(c)
    k = H.FO_LIVE_STOP_AT
    assert np.all(np.diff(gaps[:k]) < 0)
    assert gaps[k - 1] < tol < gaps[k - 2] and (gaps[k - 2] - gaps[k - 1]) / gaps[k - 2] > 1e-6
    reach = 2 * c.b_obj * float(np.max(np.abs(c.obj[k - 2:k])))  # err_obj is relative per trace entry
    assert min(gaps[k - 2] - tol, tol - gaps[k - 1]) > reach
    g64 = np.abs(c.f64["obj"] - obj0)
    assert int(np.nonzero(g64 < tol)[0][0]) + 1 == k


def test_first_order_reference_api():
    assert H.bound(0.0, 3, n=256) == 8 * 256 * 2.0 ** -53 and H.bound(0.0, 3, n=5) == H.bound(0.0, 3)
    assert H.bound(1e-13, 2, 0, 0.0, 256) == 8e-13 and H.bound(0.0, 40, 250, n=33) == 8 * 250 * 2.0 ** -53
    c = H.first_order_case("logistic", "LAG-PS", 3, 5, 3)
    assert c is H.first_order_case("logistic", "LAG-PS", 3, 5, 3) and c.lam == 1e-3 and c.alg == "LAG-PS"
    assert c.args["thrd"] == 10.0 / (c.step0 ** 2 * 9) / 10 and np.array_equal(c.args["hsq"], c.hmax ** 2)
    assert c.mask.shape == (H.FO_K, 3) and np.array_equal(c.mask.sum(1), c.cnt)
    u = H.first_order_case("logistic", "LAG-PS", 3, 5, 3, faithful=False)
    assert not np.array_equal(u.obj, c.obj)  # the forced refresh of worker 0 is a quirk of faithful runs
    i = H.first_order_case("linear", "cIAG", 3, 7, 3)
    assert i.alg == "IAG" and np.array_equal(i.args["sched"][:4], [1, 2, 0, 1]) and i.args["step"] == i.step0 / 3
    with pytest.raises(ValueError):
        H.first_order("SGD", i.X, i.y, 2, 0.1)


# ------------------------------------------------------------------------------------------------
# Set-up kernels (tests/test_gpu_setup_kernels.py): the exact Grams and the inverse references, checked
# here without a device, so that a failure there is the kernel's.
import math  # noqa: E402
from fractions import Fraction  # noqa: E402

import test_gram_crt_math as CRT  # noqa: E402  (the slicer / Garner emulation; not copied)

OZ_SL, OZ_KC = 7, 8192          # gram_ozaki.hip: digits per value, samples per chunk
CRT_KC = 32768                  # gram_crt.hip: samples per chunk
NMOD = H.CRT_NMOD


def test_kernel_constants_match_the_sources():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "kernels")
    oz, crt = open(os.path.join(src, "gram_ozaki.hip")).read(), open(os.path.join(src, "gram_crt.hip")).read()
    assert int(re.search(r"constexpr int SL = (\d+);", oz).group(1)) == OZ_SL
    assert int(re.search(r"constexpr int KC = (\d+);", oz).group(1)) == OZ_KC
    assert int(re.search(r"constexpr int KC = (\d+);", crt).group(1)) == CRT_KC
    assert int(re.search(r"constexpr int NMOD = (\d+);", crt).group(1)) == NMOD == len(CRT._tables()[0])
    assert int(re.search(r"constexpr int KB = (\d+);", crt).group(1)) == H.IMAGE_BITS == 7 * OZ_SL


@pytest.mark.parametrize("m,d", H.gram_int_shapes())
def test_exact_gram_agrees_with_long_double_and_torch(m, d):
    """The exact image equals the long-double Gram bit for bit (every sum is below 2^53, nothing
    rounds), and, where the rows are few, the torch float64 Gram too. The family's edge columns are
    where the docstring of ``integer_gram_case`` puts them."""
    import torch
    from gadmm_amd.ops import linalg
    g = H.gram_int_case(m, d)
    assert g.X.shape == (2, m, d) and g.image.shape == (2, d + 1, d + 1) and np.abs(g.shift).max() <= 30
    A, b, yy = H._gram(g.X, g.y, H.LD)
    assert np.array_equal(A, g.A.astype(H.LD)) and np.array_equal(b, g.b.astype(H.LD))
    assert np.array_equal(yy, g.yy.astype(H.LD))
    if m <= 64:
        At, bt, yyt = linalg.gram_torch(torch.from_numpy(np.array(g.X)), torch.from_numpy(np.array(g.y)))
        assert np.array_equal(At.numpy(), g.A) and np.array_equal(bt.numpy(), g.b) and np.array_equal(yyt.numpy(), g.yy)
    assert np.array_equal(g.image, g.image.transpose(0, 2, 1)) and not np.array_equal(g.N[0], g.N[1])
    if d + 1 >= 6:
        D, k = d + 1, int(np.floor(np.log2(np.abs(g.N).max() / 255.0)))
        pos = [0, D - 1, D - 2, 1, 2, D - 3]
        for n in range(2):
            e127, e255, zero, pow2, orth, u = pos[n:] + pos[:n]
            top = np.abs(g.N[n]).max(axis=0)
            assert top[e127] == 127 << k and g.N[n, :, e127].min() == -(127 << k)   # a negative extreme
            assert top[e255] == 255 << k and top[zero] == 0 and top[pow2] == 1 << k
            assert g.e[n, e127] == k + 7 + g.shift[n, e127]        # 127 2^k = 127/128 2^(k + 7): the edge
            assert g.e[n, e255] == k + 9 + g.shift[n, e255]        # 255/256 > 127/128: incremented
            assert g.e[n, pow2] == k + 1 + g.shift[n, pow2] and g.e[n, zero] == 0
            assert g.G[n, orth, u] == 0 and g.image[n, orth, u] == 0.0
            assert m < 2 or np.count_nonzero(g.N[n, :, orth] * g.N[n, :, u]) >= 2   # products that cancel


def _digit_gram(g):
    """gram_ozaki.hip on the CPU: the round-to-nearest base-128 digits of ``x 2^-e`` (the residual after
    7 digits must be 0 on this family), the exact int32 level sums of the digit pairs with p + q <= 8 per
    chunk, the recombination ``v = fma(level, 2^(-7 (L + 2)), v)`` smallest level first (the product is
    a power-of-two scaling, so the fma is one rounded addition), ``C += ldexp(v, e_a + e_b)`` per
    chunk. Integer arithmetic on integers (int64 NumPy, bounds asserted), floats where the kernel has floats."""
    aug = np.concatenate([g.X, g.y[:, :, None]], axis=2)
    out = np.zeros_like(g.image)
    digits_used = 0
    for n in range(aug.shape[0]):
        v = np.ldexp(aug[n], -g.e[n][None, :])
        assert np.abs(v).max() <= 127.0 / 128.0
        dig = np.zeros((OZ_SL,) + v.shape, dtype=np.int64)
        for p in range(OZ_SL):
            v = v * 128.0
            q = np.rint(v)
            v = v - q
            dig[p] = q.astype(np.int64)
            assert np.abs(q).max() <= (127 if p == 0 else 64)
            if np.any(q != 0):
                digits_used = max(digits_used, p + 1)
        assert not np.any(v), "a value of the integer family has more than 7 digits"
        for c0 in range(0, g.m, OZ_KC):
            chunk = dig[:, c0:c0 + OZ_KC]
            lev = np.zeros((OZ_SL,) + g.image.shape[1:], dtype=np.int64)
            for p in range(OZ_SL):
                for q in range(OZ_SL - p):
                    lev[p + q] += chunk[p].T @ chunk[q]
            assert np.abs(lev).max() < 2 ** 31
            acc = np.zeros(g.image.shape[1:])
            for L in range(OZ_SL - 1, -1, -1):
                acc = lev[L].astype(np.float64) * math.ldexp(1.0, -7 * (L + 2)) + acc
            out[n] += np.ldexp(acc, g.e[n][:, None] + g.e[n][None, :])
    return out, digits_used


@pytest.mark.parametrize("m,d", [(m, d) for d in H.GRAM_OZ_D for m in H.GRAM_OZ_M] + [(m, 3) for m in H.GRAM_OZ_LONG])
def test_digit_scheme_emulation_is_bit_exact_on_the_integer_family(m, d):
    """What entitles the GPU test to ``torch.equal``: on this family the scheme's own arithmetic, done
    correctly, reproduces the exact image bit for bit (at most 3 non-zero digits per value: no digit
    pair is dropped and every partial sum is exact)."""
    g = H.gram_int_case(m, d)
    out, used = _digit_gram(g)
    print("digits (m %d, d %d): %d digits used, %d mismatches" % (m, d, used, int(np.sum(out != g.image))))
    assert used <= 3 and np.array_equal(out, g.image)


def _crt_entry(Na, Nb, mods, inv, chunk):
    """One Gram entry by gram_crt.hip's arithmetic (tests/test_gram_crt_math.py): int8 residues, chunk
    sums reduced mod p into the balanced range, Garner, Horner in doubles."""
    res = []
    for p in mods:
        ra = [CRT._residue(float(v), p) for v in Na]
        rb = ra if Nb is Na else [CRT._residue(float(v), p) for v in Nb]
        acc = 0
        for c0 in range(0, len(ra), chunk):
            acc = int(math.fmod(acc + sum(x * y for x, y in zip(ra[c0:c0 + chunk], rb[c0:c0 + chunk])), p))
            hm = p >> 1
            acc = acc - p if acc > hm else acc + p if acc < -hm else acc
        res.append(acc)
    return CRT._garner(res, mods, inv)[0]


def _crt_emulation(g, rows=24, cols=6):
    """The emulation on a subsample of ``g``: the rows that hold each column's extremes first, then the
    leading ones, at most ``rows``; the family's edge columns, at most ``cols``. Per entry
    ``(|val - exact| / (2^-53 |exact|), val != 0 at exact == 0)`` against the subsample's own exact Gram."""
    mods, inv, kb, _ = CRT._tables()
    D = g.d + 1
    cs = sorted(set([0, D - 1, D - 2, 1, 2, D - 3][:cols]) & set(range(D)))
    worst, bad_zero = 0.0, 0
    for n in range(g.N.shape[0]):
        img = g.N[n].astype(object) * np.array([2 ** int(kb - (g.e[n, j] - g.shift[n, j])) for j in range(D)], dtype=object)
        assert max(abs(int(v)) for v in img.reshape(-1)) < 2 ** kb   # integers: e - shift <= 49 on both families
        top = list(dict.fromkeys(int(i) for i in np.argmax(np.abs(g.N[n][:, cs]), axis=0)))
        rs = (top + [i for i in range(g.m) if i not in top])[:rows]
        for ia, a in enumerate(cs):
            for c in cs[:ia + 1]:
                Na, Nb = [int(img[i, a]) for i in rs], [int(img[i, c]) for i in rs]
                exact = sum(x * y for x, y in zip(Na, Nb))
                val = _crt_entry(Na, Na if a == c else Nb, mods, inv, 7)
                if exact == 0:
                    bad_zero += val != 0.0
                else:
                    worst = max(worst, float(abs(Fraction(val) - exact) * 2 ** 53 / abs(exact)))
    return worst, bad_zero


@pytest.mark.parametrize("m,d", [(m, d) for d in H.GRAM_CRT_D for m in H.GRAM_CRT_M] + [(m, 3) for m in H.GRAM_CRT_LONG])
def test_crt_emulation_meets_the_gpu_bound_on_the_integer_family(m, d):
    """The CRT scheme's own arithmetic on the GPU file's data (a subsample: the emulation is Python per
    value and modulus) stays within NMOD 2^-53 |exact| entrywise and gives exactly 0 at an exact 0."""
    worst, bad_zero = _crt_emulation(H.gram_int_case(m, d))
    print("crt emulation (m %d, d %d): err / (2^-53 |exact|) %.2f of %d" % (m, d, worst, NMOD))
    assert worst <= NMOD and bad_zero == 0


@pytest.mark.parametrize("m,d", H.GRAM_IMAGE)
def test_image_gram_and_its_crt_emulation(m, d):
    g = H.image_case(2, m, d)
    T = 127 << 42
    assert g.image is None and np.all(np.abs(g.N).max(axis=1) == T) and np.all(np.abs(g.N).min(axis=1) == 0)
    assert np.all(g.N.max(axis=1) == T) and np.all(g.N.min(axis=1) == -T) and np.all(g.shift == g.e - H.IMAGE_BITS)
    assert int(g.G[1, d, 0]) == sum(int(a) * int(b) for a, b in zip(g.N[1, :, d], g.N[1, :, 0]))
    worst, bad_zero = _crt_emulation(g)
    print("crt emulation, 49-bit images (m %d, d %d): err / (2^-53 |exact|) %.2f of %d" % (m, d, worst, NMOD))
    assert worst <= NMOD and bad_zero == 0


def test_column_exponent_rule():
    cols = np.array([[0.0, 127.0, 127.5, 128.0, -255.0, 1.0, 2.0 ** -40 * 127 / 128]]).repeat(3, axis=0)
    cols[1] *= 0.5
    assert list(H.column_exponents(cols)) == [0, 7, 8, 8, 9, 1, -40]
    with pytest.raises(AssertionError):   # a maximum past 127/128 2^e does not pin the intended exponent
        H.image_gram(np.array([[[2 ** 49 - 1, 5]]]), np.array([[3, 3]]))
    with pytest.raises(AssertionError):   # an image Gram entry of 2^53 or more has no exact float64 image
        H.exact_gram(np.full((1, 2, 2), 2 ** 26), np.zeros(2, dtype=np.int64))


@pytest.mark.parametrize("m,d", [(33, 64), (1, 1), (8193, 3)])
def test_gram_bounds_reject_a_wrong_kernel(m, d):
    """The exact comparison rejects one entry off by one unit of its last place; the CRT bound, which
    admits NMOD roundings by construction, rejects an entry off by one unit of the INTEGER Gram (every
    ``|G| < 2^49`` on this family: one unit is above 16 * 2^-53 relative) and a value at an exact 0; both
    reject a dropped row. The exact image itself passes both."""
    g = H.gram_int_case(m, d)
    assert H.gram_errors(g, g.A, g.b, g.yy) == (0.0, 0)
    assert max(abs(int(v)) for v in g.G.reshape(-1)) < 2 ** 49
    A = np.array(g.A)
    j = int(np.argmax(np.abs(A[1]).max(axis=1) > 0))
    A[1, j, j] = np.nextafter(A[1, j, j], np.inf)
    assert not np.array_equal(A, g.A) and 1.0 <= H.gram_errors(g, A, g.b, g.yy)[0] <= 2.0
    A[1, j, j] = g.A[1, j, j] + np.ldexp(1.0, int(2 * g.shift[1, j]))
    worst, _ = H.gram_errors(g, A, g.b, g.yy)
    print("gram (m %d, d %d): one integer unit on a diagonal entry -> %.1f x 2^-53 relative" % (m, d, worst))
    assert worst > NMOD
    zeros = np.argwhere(g.A[0] == 0.0)
    if len(zeros):
        A = np.array(g.A)
        A[0, zeros[0][0], zeros[0][1]] = 2.0 ** -300
        assert H.gram_errors(g, A, g.b, g.yy) == (0.0, 1)
    # one row dropped (a tail the kernel never reads)
    Ad, bd, yyd = H._gram(g.X[:, :-1], g.y[:, :-1], np.float64)
    assert not np.array_equal(bd, g.b) or not np.array_equal(Ad, g.A) or not np.array_equal(yyd, g.yy)
    assert H.gram_errors(g, Ad, bd, yyd)[0] > NMOD
    r = H.range_statistic(g)
    assert r.dtype == H.LD and np.all(r >= 1.0)


# The inverse cases of the GPU file: (kind, d, workers, variants, recurrences).
INV_CASES = [(k, d, 3, 2, (None,)) for d in H.INV_SMALL_D + H.INV_GENERAL_D for k in H.INVERSE_KINDS if (k, d) != ("ill", 1)]
INV_CASES += [(k, d, w, v, (64, 128)) for d in H.INV_BLOCKED_D for k in H.INVERSE_KINDS for w, v in ((1, 1), (2, 2))]
INV_CASES += [("well", 9, 3, 1, (None,)), ("well", 64, 3, 1, (None,)), ("well", 200, 3, 1, (64, 128))]   # status tests


@pytest.mark.parametrize("kind,d,workers,variants,nbs", INV_CASES)
def test_inverse_cases_and_gauss_jordan_reference(kind, d, workers, variants, nbs):
    """Per matrix: kappa in the family's range (asserted when the case is built) and distinct shifts;
    ``gauss_jordan_inverse`` (plain, nb = 64 and nb = 128: all three, whatever the GPU test uses) agrees
    with ``np.linalg.inv`` to the bound of its recurrence; the long-double reference's own first-order
    error estimate is at most 1/64 of the smallest bound."""
    case = H.inverse_case(kind, d, workers=workers, variants=variants)
    assert case.A.shape == (workers, d, d) and len(set(case.shifts.reshape(-1))) == workers * variants
    for n, row in enumerate(case.mats):
        for v, c in enumerate(row):
            assert np.array_equal(c.M, case.A[n] + case.shifts[n, v] * np.eye(d)) and c.ref.dtype == H.LD
            inv = np.linalg.inv(c.M)
            for nb in (None, 64, 128):
                X = H.gauss_jordan_inverse(c.M, nb)
                assert np.array_equal(X, X.T)
                assert H.noise_level(X, inv, c.scale) <= c.bound(nb), (n, v, nb)
            smallest = min(c.bound(nb) for nb in (None, 64, 128))
            assert smallest >= H.FACTOR * d * 2.0 ** -53 * c.kappa
            se = c.self_error()
            print("inverse %s d %d n%d v%d: kappa %.3g, e64 plain %.2e nb64 %.2e nb128 %.2e, reference's own error %.2e"
                  " (%.1e of the smallest bound)" % (kind, d, n, v, c.kappa, c.e64(None), c.e64(64), c.e64(128), se,
                                                     se / smallest))
            assert se <= smallest / 64
    assert set(nbs) <= {None, 64, 128}


def test_blocked_reference_follows_the_recursion():
    """nb = 128 at d = 193 has a 65-wide last block, which recurses with 64-blocks: the result differs
    in rounding from nb = 64 and from the plain recurrence, and all three invert the matrix."""
    c = H.inverse_case("well", 193, workers=1, variants=1).mats[0][0]
    Xp, X64, X128 = (H.gauss_jordan_inverse(c.M, nb) for nb in (None, 64, 128))
    assert not np.array_equal(X64, X128) and not np.array_equal(Xp, X64)
    for X in (Xp, X64, X128):
        assert np.max(np.abs(X @ c.M - np.eye(193))) < 1e-12
    with pytest.raises(AssertionError):
        H.gauss_jordan_inverse(c.M, 32)


@pytest.mark.parametrize("d,nb", [(9, None), (64, None), (128, None), (193, 128), (257, 64)])
def test_inverse_bounds_reject_a_wrong_kernel(d, nb):
    """A ``well`` inverse with one entry moved by 1e-9 relative, and an ``ill`` inverse with one row
    taken from the neighbouring variant, land above the bound; the float64 recurrence lands below."""
    well = H.inverse_case("well", d, workers=2, variants=2) if d > 128 else H.inverse_case("well", d)
    c = well.mats[1][1]
    X = H.gauss_jordan_inverse(c.M, nb)
    assert c.err(X) <= c.bound(nb) / H.FACTOR
    X[d - 1, 0] += 1e-9 * c.scale
    assert c.err(X) > c.bound(nb)
    ill = H.inverse_case("ill", d, workers=2, variants=2) if d > 128 else H.inverse_case("ill", d)
    c, nbr = ill.mats[1][0], ill.mats[1][1]
    X = H.gauss_jordan_inverse(c.M, nb)
    X[d // 2] = H.gauss_jordan_inverse(nbr.M, nb)[d // 2]
    print("ill d %d: one row of the neighbouring variant -> err / bound %.3g" % (d, c.err(X) / c.bound(nb)))
    assert c.err(X) > c.bound(nb)
    out = np.stack([[H.gauss_jordan_inverse(m.M, nb) for m in row] for row in ill.mats])
    assert all(r <= 1.0 / H.FACTOR + 1e-12 for r in ill.ratios(out, nb).values())
    assert set(ill.ratios(out, nb)) - set(ill.ratios(out, nb, skip={(1, 0)})) == {"n1v0"}


@pytest.mark.parametrize("d,bad", [(9, 0), (9, 4), (9, 8), (64, 32), (200, 150)])
def test_non_spd_matrix_first_bad_pivot(d, bad):
    """The pivots of Gauss-Jordan without pivoting on ``non_spd_matrix(d, bad)`` are positive before
    index ``bad`` and negative at it, far from 0 (the kernels' rounding cannot move the index)."""
    M = d * H.non_spd_matrix(d, bad)
    assert np.array_equal(M, M.T)
    W = M.copy()
    piv = []
    for k in range(d):
        piv.append(W[k, k])
        W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], W[k, k + 1:]) / W[k, k]
    piv = np.array(piv) / d
    assert np.all(piv[:bad] > 0.9) and piv[bad] < -0.9
    Mn = H.non_spd_matrix(d, bad, nan=True)
    assert np.isnan(Mn[bad, bad]) and np.isnan(Mn).sum() == 1
    Mn[bad, bad] = 1.5
    assert np.linalg.eigvalsh(Mn)[0] > 0.5


# ------------------------------------------------------------------------------------------------
# Q-GADMM (tests/test_gpu_qgadmm_classes.py). A quantized run is comparable only while no rounding
# decision can flip: the condition on the reference alone for every case the GPU file uses, the
# quantizer line against the specification bit for bit, the float64 reference against the torch path,
# and the power of the bound against five wrong variants of the recurrence.
QGADMM_CASES = H.qgadmm_cases()
QGADMM_POWER_CASES = H.qgadmm_power_cases()   # (2, 3, 1) replaced by (2, 3, 2): see there
QGADMM_ALL_CASES = QGADMM_CASES + [c for c in QGADMM_POWER_CASES if c not in QGADMM_CASES]
QGADMM_POWER = 100.0


def _q_qualifies(n, m, d, bits, run, path, seed):
    agree, ratio = H.qgadmm_condition(n, m, d, bits, run, path, seed)
    return agree and ratio >= H.QGADMM_MARGIN, agree, ratio


@pytest.mark.parametrize("n,m,d,bits,path", QGADMM_ALL_CASES)
def test_qgadmm_case_is_comparable(n, m, d, bits, path):
    """At the longest run a GPU test asks of the case the long-double and the float64 run produce
    identical codes in every iteration and the smallest flip margin is >= 4 b_theta; the case's seed is
    the first from 1234 on of which that is true."""
    seed, run = H.qgadmm_seed(n, m, d, bits, path)
    assert H.QGADMM_FIRST_SEED <= seed <= H.QGADMM_LAST_SEED
    assert run == (H.K_ITERS if d > 64 else H.QGADMM_PERSISTENT_K + H.PERSISTENT_OVERRUN) and run >= H.K_ITERS
    ok, agree, ratio = _q_qualifies(n, m, d, bits, run, path, seed)
    ref = H.qgadmm_case(n, m, d, bits, run, path)[3]
    print("Q-GADMM %s b=%d chain %s seed %d, %d iterations: codes agree %s, margin %.3g = %.3g b_theta"
          % ((n, m, d), bits, path, seed, run, agree, ref.margin, ratio))
    assert ok and ref.seed == seed and ref.codes.shape == (run, n, d) and ref.theta.dtype == H.LD
    for earlier in range(H.QGADMM_FIRST_SEED, seed):
        ok, agree, ratio = _q_qualifies(n, m, d, bits, run, path, earlier)
        print("   seed %d: codes agree %s, margin / b_theta %.3g" % (earlier, agree, ratio))
        assert not ok
    # a shorter run of the case is a prefix of this one, and its margin is no smaller
    short = H.qgadmm_case(n, m, d, bits, H.QGADMM_PERSISTENT_K, path)[3]
    assert np.array_equal(short.codes, ref.codes[:H.QGADMM_PERSISTENT_K]) and short.margin >= ref.margin


def test_qgadmm_dropped_pairs():
    """No (shape, 16-bit) pair of the persistent tests is dropped; the rule for one that were: at most
    two, none at d in {16, 17, 52, 53, 64}, and truly no seed in 1234..1297 that serves 24 iterations."""
    dropped = H.QGADMM_DROPPED
    assert len(dropped) <= 2
    for (n, m, d), bits in dropped:
        assert bits == 16 and (n, m, d) in H.QGADMM_PERSISTENT_SHAPES and d not in (16, 17, 52, 53, 64)
        assert not any(_q_qualifies(n, m, d, bits, H.QGADMM_PERSISTENT_RUN, None, s)[0]
                       for s in range(H.QGADMM_FIRST_SEED, H.QGADMM_LAST_SEED + 1))
    assert set(H.QGADMM_SEEDS) <= set(QGADMM_ALL_CASES)


def test_qgadmm_uniforms_restate_the_counter_formula():
    from gadmm_amd.algorithms import quantize as Q
    for seed, it, n, w, d in [(1234, 1, 3, 0, 1), (1235, 24, 5, 4, 64), (7, 20, 4, 2, 256), (2 ** 64 - 1, 3, 2, 1, 9)]:
        u = H.q_uniforms(seed, it, n, w, d)
        assert u.dtype == np.float64 and np.all((u >= 0) & (u < 1))
        assert np.array_equal(u, Q.u01(seed, it, n, w, d))
    assert not np.array_equal(H.q_uniforms(1234, 2, 5, 1, 8), H.q_uniforms(1234, 2, 5, 3, 8))


@pytest.mark.parametrize("bits", H.QGADMM_BITS)
def test_qgadmm_quantizer_line_is_the_specification(bits):
    """On hand-picked (theta, hat, u) the float64 quantizer line of the reference equals
    ``quantize.quantize_rows`` bit for bit: a generic row, R == 0, and a row whose first two coordinates
    are extremal (diff = +R with u = 1 - 2^-53, diff = -R with u = 0; R = L / 8, so delta = 1 / 4 and
    c = L are exact and c + u rounds to L + 1: the one place where the clamp is live)."""
    from gadmm_amd.algorithms import quantize as Q
    L = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    hat = rng.standard_normal(9)
    rows = [(hat + 0.3 * rng.standard_normal(9), hat, rng.random(9)),
            (hat.copy(), hat, rng.random(9)),
            (np.zeros(9), np.zeros(9), rng.random(9))]
    R = L / 8.0
    step = np.array([R, -R, 0.0, 0.25 * R, -0.5 * R, R / 3, -R / 7, 0.999 * R, -0.999 * R])
    base = np.arange(9.0) / 4 - 1.0   # multiples of 1/4: base + step is exact, so diff = step exactly
    u = np.concatenate([[1.0 - 2.0 ** -53, 0.0], rng.random(7)])
    rows.append((base + step, base, u))
    for i, (theta, h, u) in enumerate(rows):
        Rq, q, new, _ = Q.quantize_rows(theta[None], h[None], bits, u[None])
        r64, q64, new64, margin = H.q_line(theta, h, u, bits, np.float64)
        assert r64.dtype == np.float64 and new64.dtype == np.float64
        assert np.array_equal(np.float64(r64).view(np.uint64), Rq[0].view(np.uint64)), i
        assert np.array_equal(q64, q[0]) and np.array_equal(new64.view(np.uint64), new[0].view(np.uint64)), i
        if i in (1, 2):
            assert r64 == 0 and not q64.any() and np.array_equal(new64, h) and margin == np.inf
        rld, qld, newld, _ = H.q_line(theta, h, u, bits, H.LD)
        assert newld.dtype == H.LD and (i != 0 or np.array_equal(qld, q64))
    assert np.array_equal(theta - h, step) and q64[0] == L and q64[1] == 0
    assert np.array_equal(new64[:2], theta[:2])   # both ends land on theta: L delta - R = R exactly here
    loose = H.q_line(theta, h, u, bits, np.float64, clamp=False)[1]
    assert loose[0] == L + 1 and np.array_equal(loose[1:], q64[1:])


@pytest.mark.parametrize("bits", H.QGADMM_BITS)
@pytest.mark.parametrize("n,m,d", [(3, 7, 3), (4, 30, 16), (3, 80, 65)])
def test_qgadmm_reproduces_torch_path(n, m, d, bits):
    """The torch path (``quantized_group_admm`` on CPU tensors, identity chain) stands where a kernel
    stands: true theta, th_hat (any flipped code moves it by a whole delta, >= 4 b_theta), the duals and
    the objectives are within the case's bounds of the long-double run, the residual within its own."""
    import torch
    from gadmm_amd.algorithms import quantized_group_admm
    from gadmm_amd.models import LinearRegression
    X, y, rho, ref = H.qgadmm_case(n, m, d, bits, K)
    model = LinearRegression(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(y)))
    a = quantized_group_admm(model, rho, 0.0, 0.0, K, bits, seed=ref.seed)
    hat, mu, nxt = a.extra["state"]
    assert a.extra["backend"] == "torch" and a.iters == K and nxt == K + 1 and len(a.obj) == K
    _check("Q-GADMM torch %s b=%d" % ((n, m, d), bits), ref, a.extra["theta_true"].numpy(), mu.numpy(), a.obj)
    rh, rr = ref.err_hat(hat.numpy()) / ref.b_hat, ref.err_res(a.primal_res) / ref.b_res
    print("   th_hat %.3f residual %.3f; torch margin %.3g, reference %.3g" % (rh, rr, a.extra["min_flip_margin"], ref.margin))
    assert rh <= 1.0 and rr <= 1.0


def _q_distances(n, m, d, bits, path, mutant):
    """(theta, objective) err / bound of the float64 run of ``mutant`` (None: the recurrence itself)."""
    seed, run = H.qgadmm_seed(n, m, d, bits, path)
    X, y, rho, ref = H.qgadmm_case(n, m, d, bits, run, path)
    out = H.qgadmm_linear(X, y, rho, run, bits, seed, path, np.float64, mutant)
    return ref.err_theta(out[0][-1]) / ref.b_theta, ref.err_obj(out[3]) / ref.b_obj


@pytest.mark.parametrize("n,m,d,bits,path", QGADMM_POWER_CASES)
def test_qgadmm_bound_rejects_a_wrong_variant(n, m, d, bits, path):
    """Power of the GPU tests, as a condition on the reference alone: a float64 run whose duals read the
    true theta, one whose right-hand side reads the neighbours' true theta, one that evaluates the
    objective of th_hat and (on a permuted chain; on the identity chain it is the recurrence itself) one
    that indexes the uniforms by chain position each sit at least 100 bounds from the reference in theta
    or in the objective. The float64 run itself sits below 1/8.

    The cases are those of the GPU file, but for (2, 3, 1), whose data is replaced by (2, 3, 2): with one
    coordinate th_hat == theta up to rounding whatever the data (``qgadmm_power_cases``), and every
    variant sat at 2.5e-3 / 2.2e-2 bounds, the distance of the recurrence itself. Measured: >= 2.3e6
    bounds in the objective everywhere (and, obj-hat aside, >= 80 in theta, >= 2.6e3 from d = 3 on);
    the table is in profiles/qgadmm_classes/README.md."""
    assert max(_q_distances(n, m, d, bits, path, None)) <= 1.0 / 8
    for mutant in H.QGADMM_MUTANTS[:4] if path is not None else H.QGADMM_MUTANTS[:3]:
        r = _q_distances(n, m, d, bits, path, mutant)
        print("Q-GADMM %s b=%d chain %s mutant %-10s: err/bound theta %.2e objective %.2e"
              % ((n, m, d), bits, path, mutant, *r))
        assert max(r) >= QGADMM_POWER, (mutant, r)
    if path is not None:
        X, y, rho, ref = H.qgadmm_case(n, m, d, bits, K)
        same = H.qgadmm_linear(X, y, rho, K, bits, ref.seed, None, np.float64, "u-position")
        assert np.array_equal(same[0], H.qgadmm_linear(X, y, rho, K, bits, ref.seed, None, np.float64)[0])


def test_qgadmm_seed_solved_for_a_draw():
    """``q_seed_drawing_top`` inverts the counter formula: the chosen draw is 1 - 2^-53, under both
    statements of the formula, and its 2048 solutions differ elsewhere."""
    from gadmm_amd.algorithms import quantize as Q
    for low, it, n, w, d, i in [(0, 1, 2, 0, 1, 0), (5, 1, 3, 2, 9, 4), (2047, 7, 5, 3, 256, 255)]:
        seed = H.q_seed_drawing_top(low, it, n, w, d, i)
        assert 0 <= seed < 2 ** 64
        for u in (H.q_uniforms(seed, it, n, w, d), Q.u01(seed, it, n, w, d)):
            assert u[i] == 1.0 - 2.0 ** -53 and (d == 1 or np.sum(u == u[i]) == 1)
    a, b = (H.q_uniforms(H.q_seed_drawing_top(low, 1, 3, 2, 9, 4), 1, 3, 2, 9) for low in (0, 1))
    assert a[4] == b[4] and not np.array_equal(a, b)


@pytest.mark.parametrize("n,m,d,bits,path", QGADMM_CASES)
def test_qgadmm_bound_rejects_a_missing_clamp(n, m, d, bits, path):
    """The fifth variant, no clamp of the code, held to the same 100 bounds on every shape of the GPU
    file. With the seeds 1234, 1235, ... the variant IS the recurrence (it sat at 0.02 .. 0.125 bounds
    in every case): with ``|diff| <= R`` the code is in [0, L] before the clamp, which acts only when
    ``c = L`` and ``c + u`` rounds up to L + 1, and no such draw comes up. So the data of every case is
    replaced (``qgadmm_clamp_case``): the first data seed with a head whose first difference has
    ``c = L`` exactly, and the quantizer seed SOLVED from the counter formula so that this coordinate
    draws 1 - 2^-53 in iteration 1. The case is comparable (asserted), the float64 recurrence with the
    clamp sits below 1/8, and the variant's code L + 1 moves th_hat by a whole delta: measured
    >= 1.7e6 bounds in theta and >= 3.9e6 in the objective."""
    X, y, rho, ref, (t, w, i, low) = H.qgadmm_clamp_case(n, m, d, bits, path)
    Kc, L = H.QGADMM_CLAMP_K, (1 << bits) - 1
    assert ref.codes_agree and ref.margin >= H.QGADMM_MARGIN * ref.b_theta and ref.codes.shape == (Kc, n, d)
    assert ref.seed == H.q_seed_drawing_top(low, 1, n, w, d, i) and ref.codes[0, w, i] == L
    out = {}
    for mutant in (None, "no-clamp"):
        run = H.qgadmm_linear(X, y, rho, Kc, bits, ref.seed, path, np.float64, mutant)
        out[mutant] = (ref.err_theta(run[0][-1]) / ref.b_theta, ref.err_obj(run[3]) / ref.b_obj, run[4])
    print("Q-GADMM %s b=%d chain %s (data +%d, worker %d coordinate %d, low %d, margin %.3g b_theta) mutant no-clamp: "
          "err/bound theta %.2e objective %.2e" % ((n, m, d), bits, path, t, w, i, low, ref.margin / ref.b_theta,
                                                   *out["no-clamp"][:2]))
    assert max(out[None][:2]) <= 1.0 / 8 and np.array_equal(out[None][2], ref.codes)
    assert out["no-clamp"][2][0, w, i] == L + 1   # the clamp is what the float64 recurrence relied on
    assert max(out["no-clamp"][:2]) >= QGADMM_POWER, out["no-clamp"][:2]


# ------------------------------------------------------------------------------------------------
# K4 primal residual (the "K4 primal residual" sections of tests/test_gpu_dispatch_classes.py and
# tests/test_gpu_newton_classes.py, and every solve of tests/test_gpu_dgadmm_classes.py): a function of
# the theta history the references already hold (``chain_residual``). The condition that entitles the
# GPU tests to their bound, the power of that bound against six wrong residual branches, and the torch
# path, the yardstick of the suite's older d = 50 residual test, held to the same reference.
RES_OVER = K + H.PERSISTENT_OVERRUN   # the longest run a persistent kernel's test may ask for
RES_BLOCKED_MULTI = (13, 20, 8)       # the static blocked kernel with several owned positions per workgroup
RES_POWER = 100.0
RES_CASES = (
    [("linear", s, None, RES_OVER if s[2] <= 128 else K) for s in H.LINEAR_SHAPES + [RES_BLOCKED_MULTI]]
    + [("path", s, p, RES_OVER) for s, p in H.RESIDUAL_PATHS.items()]
    + [("logistic", s, None, RES_OVER if max(s[1:]) <= 64 else K) for s in H.LOGISTIC_SHAPES]
    + [("live-stop", H.LIVE_STOP[0], H.LIVE_STOP[1], K)]
    + [("newton", s, None, RES_OVER if s in H.NEWTON_PERSISTENT_SHAPES else K) for s in H.NEWTON_SHAPES]
    + [("dgadmm", c[:3], c[3], RES_OVER if c[2] <= 99 else K) for c in DGADMM_CASES])


def _res_reference(kind, shape, arg, run):
    n, m, d = shape
    if kind == "linear":
        return H.linear_case(n, m, d, run)[3]
    if kind == "path":
        return H.linear_path_case(n, m, d, arg, run)[3]
    if kind == "logistic":
        return H.logistic_case(n, m, d, run)[5]
    if kind == "live-stop":
        return H.logistic_case(n, m, d, run, inner_tol=arg)[5]
    if kind == "newton":
        return H.newton_case(n, m, d, run, 0.0)
    return H.dgadmm_case(n, m, d, arg, run)[4]


def _res_ratios(ref, mutant=None):
    """(rows, sum) err / bound of ``chain_residual`` of the float64 history in float64."""
    rows = H.chain_residual(ref.theta64, ref.chains, np.float64, mutant)
    return ref.err_res_w(rows) / ref.b_res_w, ref.err_res(rows.sum(axis=1)) / ref.b_res


def _roles_change(chains):
    """Some re-chain gives a worker another role or another set of neighbours."""
    tabs = H.chain_tables(chains)
    view = [{w: (p % 2, frozenset((l, r))) for w, (p, l, r) in tab.items()} for _, tab in tabs]
    return any(a != b for a, b in zip(view, view[1:]))


def _res_live_mutants(ref):
    n, d = ref.theta.shape[1:]
    chains = [(1, list(range(n)))] if ref.chains is None else ref.chains
    live = ["stale-head", "pre-update"]
    if n > 2:
        live.append("one-edge")
    if d > 64:
        live.append("lanes-64")
    if _roles_change(chains):
        live.append("old-chain")
    if any(list(p) != list(range(n)) for _, p in chains):
        live.append("by-position")
    return live


@pytest.mark.parametrize("kind,shape,arg,run", RES_CASES)
def test_residual_reference_condition_and_power(kind, shape, arg, run):
    """On every case a GPU test compares a K4 residual on, over the longest run it may ask for: the
    bounds are finite, the trace is positive on the tails and exactly 0 on the heads, the float64 history
    sits within 1/8 of them (by construction; this guards the plumbing), and every wrong residual branch
    that changes the value at the case -- a dropped right edge (n > 2), the heads' or the tail's own
    theta of the iteration before, the first 64 coordinates only (d > 64), the chain of the iteration
    before (where a re-chain changes roles or neighbours), the row indexed by chain position (any chain
    but the identity) -- sits at least 100 bounds away in the rows or in their sum. An inert variant IS
    the function. Measured: profiles/residual_classes/README.md."""
    ref = _res_reference(kind, shape, arg, run)
    n = shape[0]
    assert ref.res_w.shape == (run, n) and ref.res.shape == (run,) and ref.res_w.dtype == H.LD
    assert np.isfinite(ref.b_res_w) and np.isfinite(ref.b_res) and ref.b_res_w > 0 and ref.b_res > 0
    assert np.all(ref.res_w[~ref.tails] == 0) and np.all(ref.res_w[ref.tails] > 0)
    assert np.all(ref.tails.sum(axis=1) == n // 2)
    own = _res_ratios(ref)
    live = _res_live_mutants(ref)
    print("residual %s %s %s run %d: e64 rows %.2e sum %.2e; float64 err/bound rows %.3f sum %.3f; "
          "smallest/largest %.1e" % (kind, shape, arg, run, ref.e_res_w, ref.e_res, own[0], own[1],
                                     float(ref.res.min() / ref.res.max())))
    assert max(own) <= 1.0 / 8
    for mutant in H.RESIDUAL_MUTANTS:
        if mutant in live:
            r = _res_ratios(ref, mutant)
            print("   mutant %-11s: err/bound rows %.2e sum %.2e" % (mutant, *r))
            assert max(r) >= RES_POWER, (mutant, r)
        else:
            assert np.array_equal(H.chain_residual(ref.theta, ref.chains, H.LD, mutant), ref.res_w), mutant


def test_residual_reference_api():
    """``chain_residual`` by hand on a tiny history, the identity default, and prefixes."""
    th = np.zeros((2, 3, 2))
    th[0] = [[1.0, 0.0], [3.0, 0.0], [0.0, 4.0]]
    th[1] = [[1.0, 1.0], [1.0, 2.0], [2.0, 2.0]]
    r = H.chain_residual(th, None, np.float64)
    assert r.dtype == np.float64 and np.array_equal(r, [[0.0, 4.0 + 25.0, 0.0], [0.0, 1.0 + 1.0, 0.0]])
    assert np.array_equal(H.chain_residual(th, [(1, [0, 1, 2])], np.float64), r)
    assert np.array_equal(H.chain_residual(th, None, np.float64, "one-edge"), [[0.0, 4.0, 0.0], [0.0, 1.0, 0.0]])
    # re-chained at iteration 2 to (1, 0, 2): worker 0 is the tail, its neighbours 1 and 2
    r2 = H.chain_residual(th, [(1, [0, 1, 2]), (2, [1, 0, 2])], H.LD)
    assert r2.dtype == H.LD and np.array_equal(r2, [[0.0, 29.0, 0.0], [1.0 + 2.0, 0.0, 0.0]])
    assert np.array_equal(H.chain_residual(th, [(1, [0, 1, 2]), (2, [1, 0, 2])], H.LD, "old-chain"), r)
    assert np.array_equal(H.chain_residual(th, [(1, [1, 0, 2])], H.LD, "by-position")[1], [0.0, 3.0, 0.0])
    mask = H.tail_mask([(1, [0, 1, 2]), (2, [1, 0, 2])], 2, 3)
    assert np.array_equal(mask, [[False, True, False], [True, False, False]])
    a, b = H.linear_case(3, 7, 3, K + 3)[3], H.linear_case(3, 7, 3)[3]
    assert np.array_equal(a.res_w[:K], b.res_w) and np.array_equal(a.res[:K], b.res) and a.err_res(b.res) == 0.0
    assert a.err_res_w(np.asarray(b.res_w, dtype=np.float64)) <= 2.0 ** -52
    q = H.qgadmm_case(3, 7, 3, 8, K)[3]   # the quantized reference keeps its own residual, on the public models
    assert q.res.shape == (K,) and not hasattr(q, "res_w")


@pytest.mark.parametrize("n,m,d", [(3, 7, 3), (4, 40, 33), (3, 80, 65)])
def test_residual_of_the_torch_path(n, m, d):
    """``chain_admm(backend="torch")`` is what tests/test_gpu.py holds the native residual to at d = 50;
    here its ``primal_res`` is held to the reference under the case's bound."""
    import torch
    from gadmm_amd.algorithms import chain_admm
    from gadmm_amd.models import LinearRegression
    X, y, rho, ref = H.linear_case(n, m, d)
    model = LinearRegression(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(y)))
    a = chain_admm(model, list(range(n)), n, rho, 0.0, 0.0, K, backend="torch")
    assert a.extra["backend"] == "torch" and a.iters == K and len(a.primal_res) == K
    ratio = ref.err_res(np.asarray(a.primal_res)) / ref.b_res
    print("torch path %s: residual err/bound %.3f (e64 %.2e)" % ((n, m, d), ratio, ref.e_res))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------
# The block-packed symmetric GEMV (tests/test_gpu_symv_exact.py): the NumPy model of its block structure
# equals the integer product, and each mistake the GPU test is there to catch changes the result on the
# very data that test uses.
@pytest.mark.parametrize("d", [129, 1025, 8193])
def test_symv_packed_model_and_its_mutants(d):
    """d = 129: nb = 2, the first transposed product; 1025: nb = 9, per = 2, a clipped last group and
    empty ones; 8193: nb = 65, per = 9, a second, masked trip of the eight-loads loop. A mutant differs at
    every d that has the path it breaks: "clip-8" needs per > 8, so only d = 8193 can see it -- at 129 and
    1025 it IS the product, which is why the GPU test runs d = 8193."""
    M, x, y = H.symv_int_data(d)
    M, x, y = M[0], x[0], y[0]
    assert np.array_equal(M, M.T) and np.abs(M).max() <= H.SYMV_AMP and np.abs(x).max() <= H.SYMV_AMP
    if d == 129:  # the int64 product against Python integers
        assert [int(v) for v in y] == [sum(int(a) * int(b) for a, b in zip(row, x)) for row in M]
    good = H.symv_packed_model(M, x)
    assert good.dtype == np.float64 and np.all(np.isfinite(good))
    assert np.array_equal(good.astype(np.int64), y) and np.array_equal(good, y.astype(np.float64))
    nb = -(-d // H.SYMV_B)
    per = -(-nb // H.SYMV_RG)
    for mutant in H.SYMV_MUTANTS:
        bad = H.symv_packed_model(M, x, mutant)
        live = per > H.SYMV_LOADS if mutant == "clip-8" else nb >= 2
        wrong = int(np.sum(~(bad == good)))  # a NaN (a partial nothing wrote) counts as wrong
        print("symv model d=%d %s: %d of %d entries differ" % (d, mutant, wrong, d))
        assert (wrong > 0) == live, (d, mutant, wrong)
    # the dropped transposed product surfaces as NaN: the partial is read and was never written
    assert np.isnan(H.symv_packed_model(M, x, "drop-transposed")).any()


def test_symv_packed_model_smallest_shapes():
    """d = 1, 127, 128 (one diagonal block, read as the mirror of its lower half) and 1024 (per = 1, every
    group one block): the model is the product there too."""
    for d in (1, 127, 128, 1024):
        M, x, y = H.symv_int_data(d)
        assert np.array_equal(H.symv_packed_model(M[0], x[0]), y[0].astype(np.float64))
    # the upper half of a diagonal block is never read: garbage there changes nothing
    M, x, y = H.symv_int_data(127)
    G = M[0].copy()
    G[np.triu_indices(127, 1)] = 12345
    assert np.array_equal(H.symv_packed_model(G, x[0]), y[0].astype(np.float64))
