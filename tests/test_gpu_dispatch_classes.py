"""Every kernel dispatch class of the chain, logistic and star solvers against a long-double reference.

The kernels dispatch on d (and on m for logistic) into separately instantiated templates; the rest of
the suite solves end to end at d = 50 almost only, and holds the odd shapes against another kernel,
not against an independent reference. Here each class runs K = 20 iterations of a tiny problem with no
stop rule (tol = 0, obj0 = 0, max_iter = K: the comparisons in the kernels are strict, nothing stops
early, no discrete decision can tie) and theta, the duals and the objectives are compared with
tests/hp_reference.py (plain NumPy in long double). The tolerance is not a fixed rtol: per case,

    err_kernel <= 8 * max(e64, max(d, m_logistic, 16) * 2^-53)

where e64 is the distance of the SAME recurrence run in float64 NumPy from its long-double run (taken
separately for theta / max|theta|, the dual / (rho max|theta|) and each objective value), and the
second term is the dot-product bound, the floor for runs that round luckily. The factor 8 pays for a
different summation order, FMA contraction and the ~2 ulp of the fast sigmoid; an indexing, tail or
stale-LDS mistake moves theta by ~1/d relative, eleven orders of magnitude above the bound.
Each test prints err / bound; profiles/dispatch_classes/README.md records the measured table.

The "K4 primal residual" section runs the chain classes once more with ``residual=True`` (the setting of
every solve a user runs) and holds the K residual sums and the per-worker rows behind them to
hp_reference.chain_residual under the same rule (profiles/residual_classes/README.md).

The star section runs the streaming engine (star_big.hip) past its first block and block row, with the
hub in the middle of the local order and with the device stop rule firing inside a block of enqueued
iterations, and the persistent star kernel over the hub's row layout (one, two and nine rows per helper
wave), where the hub's copies of the duals must be the workers' duals one step on, bit for bit
(profiles/star_classes/README.md).

Each parameter list names the dispatch condition that puts its d in its class: if a threshold moves,
the list next to it is the one to revisit.

Run with: pytest -m gpu tests/test_gpu_dispatch_classes.py -s
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = H.K_ITERS
BLOCK = 4  # iterations per graph replay: divides K, so the graph engine replays every iteration
assert K % BLOCK == 0


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _report(tag, ratios):
    """Print err / bound of every quantity, then assert all of them <= 1."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------
# Linear chain
def _linear_engine(n, m, d, residual=False, **kw):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, rho, _ = H.linear_case(n, m, d)
    eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "linear", rho=rho, obj0=0.0, tol=0.0, max_iter=K,
                            obj_mode="exact", block=BLOCK, residual=residual, **kw)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def _state_ratios(eng, ref, last, prefix=""):
    """theta after iteration ``last`` and, once the heads' lazy last dual update is applied
    (flush_duals; header of csrc/kernels/chain_small.hip), mu after it."""
    th = _host(eng.local_theta())
    eng.flush_duals()
    eng.stream.synchronize()
    mu = _host(eng.mu)
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(mu))
    return {prefix + "theta": ref.err_theta(th, last) / ref.b_theta, prefix + "dual": ref.err_dual(mu) / ref.b_dual}


def _residual_rows(eng, ref):
    """err / bound of the per-worker K4 rows of iterations 1..K (``eng.rres``, (K, n) by worker id) against
    ``ref`` (which may run past K: a persistent kernel's; ``max_iter = K``, so no row past K exists).
    Every head's entry is exactly 0.0 -- nothing writes it, ``reset()`` zeroed it -- and every tail's is
    finite and positive."""
    n = eng.n_total
    eng.stream.synchronize()
    assert eng.rres is not None and eng.rres.numel() >= K * n
    rows = _host(eng.rres[:K * n].view(K, n))
    tails = ref.tails[:K]
    assert np.all(rows[~tails] == 0.0), ("a head's row is not 0", rows)
    assert np.all(np.isfinite(rows[tails])) and np.all(rows[tails] > 0), rows
    return ref.err_res_w(rows) / ref.b_res_w


def _residual_ratios(eng, ref):
    """The K4 primal residual of an engine built with ``residual=True``: the K sums ``primal_residual``
    returns and the per-worker rows behind them (``_residual_rows``)."""
    rows = _residual_rows(eng, ref)
    return {"residual": ref.err_res(eng.primal_residual(K)) / ref.b_res, "residual rows": rows}


def run_linear_graph(n, m, d, use_graph=True, residual=False):
    """The phase kernels (chain_small.hip chain_phase_linear<NC>, chain_big.hip), replayed as a graph
    or launched eagerly: K iterations, then theta, mu and the K objectives (``residual``: and the K4
    primal residual, ``_residual_ratios``)."""
    ref = H.linear_case(n, m, d)[3]
    eng = _linear_engine(n, m, d, residual=residual)
    r = eng.run(stop_iter=K, use_graph=use_graph)
    assert r.iters == K and eng.ctl_state()["iter"] == K + 1, (r.iters, r.done, eng.ctl_state())
    # (a block shorter than the captured one is enqueued kernel by kernel: BLOCK divides K, none is)
    assert r.replays == K // BLOCK and (eng.graph_ok() or not use_graph) and eng.obj_mode_name == "exact"
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj}
    out.update(_state_ratios(eng, ref, K))
    if residual:
        out.update(_residual_ratios(eng, ref))
    eng.close()
    return out


def run_linear_persistent(n, m, d, family, residual=False, eng=None, case=None):
    """One persistent launch (``family``: "per-worker" or "blocked(", chosen by the environment the
    caller set). The kernel learns the cap's stop decision ``lag`` iterations late and stops after
    iteration ctl.iter - 1: theta and mu are compared with the reference run that far. ``eng``: an
    engine of the caller's (it stays open) in place of a fresh one; ``case``: ``last -> Reference`` of
    what that engine solves, in place of ``linear_case``."""
    own = eng is None
    if own:
        eng = _linear_engine(n, m, d, residual=residual)
    assert eng.persistent_eligible()
    if family == "blocked(":
        assert eng.blocked_plan() is not None
    r = eng.run_persistent()
    assert eng.last_kernel.startswith(family), eng.last_kernel
    last = eng.ctl_state()["iter"] - 1
    assert r.iters == K and K <= last <= K + 16, (r.iters, r.done, last)
    ref = H.linear_case(n, m, d, last)[3] if case is None else case(last)
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj}
    out.update(_state_ratios(eng, ref, last))
    if residual:
        out.update(_residual_ratios(eng, ref))
    kern = eng.last_kernel
    if own:
        eng.close()
    return out, kern


# d -> class of the graph phases: gadmm_chain_phase (chain_small.hip) sends d > 256 to
# gadmm_chain_phase_big (chain_big.hip) and switches on nc = (d + 63) / 64 between
# chain_phase_linear<1> (d <= 64), <2> (65..128) and <4> (129..256).
LINEAR_GRAPH = [
    (2, 3, 1),       # <1>: the smallest possible; every worker has degree 1 (one inverse variant)
    (3, 7, 3),       # <1>: odd n, the last worker is a head
    (5, 40, 32),     # <1>
    (4, 40, 33),     # <1>
    (5, 60, 52),     # <1>
    (5, 70, 53),     # <1>
    (4, 40, 64),     # <1>: the top of nc = 1; m < d, the Gram is rank-deficient and the shift makes it SPD
    (3, 80, 65),     # <2>: the first nc = 2 shape
    (4, 150, 128),   # <2>: the top of nc = 2
    (3, 150, 129),   # <4>: the first
    (3, 280, 256),   # <4>: the top
    (3, 280, 257),   # chain_big: the first d > 256
]
assert LINEAR_GRAPH == H.LINEAR_SHAPES


@pytest.mark.parametrize("n,m,d", LINEAR_GRAPH)
def test_linear_graph_engine(n, m, d):
    _report("linear graph %s" % ((n, m, d),), run_linear_graph(n, m, d))


# the same kernels launched one by one (run(use_graph=False)): one shape per phase-kernel family
@pytest.mark.parametrize("n,m,d", [(2, 3, 1), (3, 80, 65), (3, 280, 257)])
def test_linear_eager_phases(n, m, d):
    _report("linear eager %s" % ((n, m, d),), run_linear_graph(n, m, d, use_graph=False))


# per-worker persistent kernel: pick_variant (chain_persistent.hip) takes the register kernel at
# d <= DREG = 64 -- QT = 13 at d <= 52, QT = 16 above -- and the LDS kernel with NC = 2 at 65..128;
# gadmm_chain_persistent_lds returns 0 (not eligible) at d > 128.
LINEAR_PER_WORKER = [
    (2, 3, 1), (3, 7, 3), (5, 40, 32), (4, 40, 33),
    (5, 60, 52),     # REG QT = 13: the top
    (5, 70, 53),     # REG QT = 16: the first
    (4, 40, 64),     # REG QT = 16: the top
    (3, 80, 65),     # LDS NC = 2: the first
    (4, 150, 128),   # LDS NC = 2: the top, and the top of the persistent kernel
]


@pytest.mark.parametrize("n,m,d", LINEAR_PER_WORKER)
def test_linear_per_worker_persistent(n, m, d, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED", "0")
    out, kern = run_linear_persistent(n, m, d, "per-worker")
    assert kern == "per-worker"
    _report("linear per-worker %s" % ((n, m, d),), out)


def test_linear_persistent_not_eligible_above_128():
    eng = _linear_engine(3, 150, 129)
    assert not eng.persistent_eligible() and eng.blocked_plan() is None
    eng.close()


# blocked kernel: gadmm_chain_blocked_plan2 (chain_blocked.hip) returns no plan at d > 52; the launcher
# takes chain_blocked_kernel<32> at d <= 32 and <52> at 33..52 (gadmm_chain_blocked_pad_dim), and
# chain_blocked_pair_kernel<DB> under GADMM_BLOCK_PW=2.
LINEAR_BLOCKED = [
    (2, 3, 1, 1), (3, 7, 3, 1),
    (5, 40, 32, 1),  # DB = 32: the top
    (4, 40, 33, 1),  # DB = 52: the first
    (5, 60, 52, 1),  # DB = 52: the top
    (5, 60, 52, 2),  # DB = 52, a head + tail pair per wave
]


@pytest.mark.parametrize("n,m,d,pw", LINEAR_BLOCKED)
def test_linear_blocked_persistent(n, m, d, pw, monkeypatch):
    monkeypatch.delenv("GADMM_BLOCKED", raising=False)
    if pw != 1:
        monkeypatch.setenv("GADMM_BLOCK_PW", str(pw))
    out, kern = run_linear_persistent(n, m, d, "blocked(")
    assert ("pw=%d" % pw) in kern, kern
    _report("linear blocked pw=%d %s" % (pw, (n, m, d)), out)


def test_blocked_kernel_stops_at_52(monkeypatch):
    monkeypatch.delenv("GADMM_BLOCKED", raising=False)
    eng = _linear_engine(5, 70, 53)
    assert eng.blocked_plan() is None and eng.persistent_eligible()
    eng.close()


# D-GADMM on the per-worker kernel's dynamic mode (GADMM_BLOCKED_DYN=0): pick_variant's `dyn` branch,
# register kernel with both degree variants resident (NV = 2), QT = 13 at d <= 52 and 16 at 53..64
@pytest.mark.parametrize("n,m,d", [(5, 60, 52), (5, 70, 53)])
def test_dgadmm_per_worker_dynamic(n, m, d, monkeypatch):
    """Coherence 3 for K iterations over the chains tests/test_gpu_dyn_sweep.py uses (find_path2 drawn
    from the schedule's seed), against the long-double run of the re-chaining recurrence over those
    very chains (hp_reference.dgadmm_case with explicit chains) under its own bound; the float64 oracle
    (oracle.reference.dgadmm_linear), fed them through its callback, is held to the same reference.
    The kernel stops ``lag`` iterations after the cap and re-chains at none of them.
    tests/test_gpu_dgadmm_classes.py covers the other dynamic classes over prescribed chains."""
    from gadmm_amd.algorithms import dynamic_group_admm
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.oracle import reference as R
    from gadmm_amd.parallel import topology as T
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "0")
    X, y, rho, _ = H.linear_case(n, m, d)
    model = LinearRegression(_dev(X), _dev(y))
    p0, c0, _ = T.find_path(n, np.random.default_rng(5))
    a = dynamic_group_admm(model, rho, 0.0, 0.0, K, p0, c0, 3, seed=99, engine_opts={"cache": False})
    eng = a.extra["engine_obj"]
    assert a.extra["engine"] == "persistent-dynamic" and eng.last_kernel == "per-worker", (a.extra["engine"],
                                                                                            eng.last_kernel)
    theta, mu, nxt = a.extra["state"]
    last = nxt - 1
    assert a.iters == K and len(a.obj) == K and K <= last <= K + 16, (a.iters, last)
    rng = np.random.default_rng(99)
    seq = {}
    cur = [(list(p0), c0)]

    def rechain(it):
        if it > K:  # the solve draws no chain past its cap
            return cur[0]
        if it not in seq:
            p, c, _, _, _ = T.find_path2(n, rng)
            seq[it] = cur[0] = (p, c)
        return seq[it]

    o = R.dgadmm_linear(X, y, rho, last, 0.0, 0.0, p0, c0, 3, rechain)
    assert len(seq) == len([it for it in range(2, K + 1) if it % 3 == 0])
    chains = [(1, list(p0))] + [(it, list(seq[it][0])) for it in sorted(seq)]
    assert any(a_[1] != b_[1] for a_, b_ in zip(chains, chains[1:]))
    ref = H.dgadmm_case(n, m, d, 3, last, chains=chains)[4]
    out = {"objective": ref.err_obj(a.obj) / ref.b_obj, "theta": ref.err_theta(_host(theta), last) / ref.b_theta,
           "dual": ref.err_dual(_host(mu)) / ref.b_dual, "residual": ref.err_res(a.primal_res) / ref.b_res,
           "oracle objective": ref.err_obj(np.asarray(o.obj)) / ref.b_obj,
           "oracle theta": ref.err_theta(o.theta, last) / ref.b_theta, "oracle dual": ref.err_dual(o.dual) / ref.b_dual}
    out["residual rows"] = _residual_rows(eng, ref)
    eng.close()
    _report("D-GADMM per-worker dynamic %s" % ((n, m, d),), out)


# ------------------------------------------------------------------------------------------------
# Logistic, inner gradient descent: max_inner = 6, inner_tol = 0 (every local solve takes 6 steps)
def _logistic_engine(n, m, d, inner_tol=0.0, residual=False):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, rho, lam, step, _ = H.logistic_case(n, m, d, inner_tol=inner_tol)
    eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "logistic", rho=rho, obj0=0.0, tol=0.0, max_iter=K,
                            lam=lam, step=step, max_inner=H.MAX_INNER, inner_tol=inner_tol, block=BLOCK,
                            residual=residual)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def run_logistic_graph(n, m, d, inner_tol=0.0, residual=False):
    ref = H.logistic_case(n, m, d, inner_tol=inner_tol)[5]
    eng = _logistic_engine(n, m, d, inner_tol, residual=residual)
    r = eng.run(stop_iter=K)
    assert r.iters == K and eng.graph_ok() and eng.ctl_state()["iter"] == K + 1, (r.iters, r.done)
    assert r.replays == K // BLOCK
    inner = _host(eng.inner_iters)[:n]
    assert np.array_equal(inner, ref.extra[0][K - 1]), (inner, ref.extra[0][K - 1])
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj}
    out.update(_state_ratios(eng, ref, K))
    if residual:
        out.update(_residual_ratios(eng, ref))
    eng.close()
    return out


def run_logistic_persistent(n, m, d, residual=False):
    eng = _logistic_engine(n, m, d, residual=residual)
    assert eng.persistent_eligible()
    r = eng.run_persistent()
    assert eng.last_kernel == "per-worker-logistic", eng.last_kernel
    last = eng.ctl_state()["iter"] - 1
    assert r.iters == K and K <= last <= K + 16, (r.iters, r.done, last)
    ref = H.logistic_case(n, m, d, last)[5]
    assert np.all(_host(eng.inner_iters)[:n] == H.MAX_INNER)
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj}
    out.update(_state_ratios(eng, ref, last))
    if residual:
        out.update(_residual_ratios(eng, ref))
    eng.close()
    return out


# gadmm_chain_phase (chain_small.hip), logistic branch: ldsx = m d <= 8192 && m <= 256; under ldsx,
# dm = max(d, m) <= 64 takes chain_phase_logistic_quad<8> (dm <= 32), <13> (<= 52), <16> (<= 64), a
# larger dm chain_phase_logistic_wave<cmax>, cmax = max(ceil(d / 64), ceil(m / 64)) -> 1 / 2 / 4;
# without ldsx, chain_phase_logistic<1, 4, false> at d <= 64 and <4, 4, false> above.
LOGISTIC_GRAPH = [
    (3, 5, 3),       # quad<8>
    (4, 30, 20),     # quad<8>
    (3, 40, 52),     # quad<13> through d
    (3, 52, 20),     # quad<13> through m
    (3, 40, 53),     # quad<16>: the first
    (3, 64, 64),     # quad<16>: the top, full register rows
    (3, 100, 20),    # wave<2> through mc = 2
    (2, 60, 128),    # wave<2> through nc = 2 (m d = 7680)
    (3, 200, 30),    # wave<4> (mc = 4)
    (3, 250, 40),    # non-LDSX <1, 4> (m d = 10000)
    (3, 100, 100),   # non-LDSX <4, 4>
]
assert LOGISTIC_GRAPH == H.LOGISTIC_SHAPES


@pytest.mark.parametrize("n,m,d", LOGISTIC_GRAPH)
def test_logistic_graph_engine(n, m, d):
    _report("logistic graph %s" % ((n, m, d),), run_logistic_graph(n, m, d))


def test_logistic_live_stop_rule():
    """(4, 30, 20) with inner_tol = 1e-3: the inner solves of the last iterations stop early, each at
    the reference's step (tests/test_hp_reference_cpu.py holds every stop test 1e-6 off its threshold)."""
    (n, m, d), tol = H.LIVE_STOP
    ref = H.logistic_case(n, m, d, inner_tol=tol)[5]
    assert ref.extra[0][K - 1].min() < H.MAX_INNER
    _report("logistic graph live stop %s" % ((n, m, d),), run_logistic_graph(n, m, d, inner_tol=tol))


# logi_variant (chain_persistent_logistic.hip): mx = max(d, m) <= 64 only; QT = 13 at mx <= 52, 16
# above; GADMM_LOGISTIC_ZREC=0 the one-wave kernel, otherwise (default) the margins-recursion kernel
LOGISTIC_PERSISTENT = [
    (3, 5, 3), (4, 30, 20),
    (3, 40, 52),     # QT = 13: the top, through d
    (3, 52, 20),     # QT = 13: the top, through m
    (3, 40, 53),     # QT = 16: the first
    (3, 64, 64),     # QT = 16: the top
]


@pytest.mark.parametrize("zrec", ["0", "1"])
@pytest.mark.parametrize("n,m,d", LOGISTIC_PERSISTENT)
def test_logistic_persistent_kernel(n, m, d, zrec, monkeypatch):
    monkeypatch.setenv("GADMM_LOGISTIC_ZREC", zrec)
    _report("logistic persistent zrec=%s %s" % (zrec, (n, m, d)), run_logistic_persistent(n, m, d))


# ------------------------------------------------------------------------------------------------
# K4 primal residual (residual=True, what every solve a user runs has on): each tail writes
# |th_l - th|^2 + |th - th_r|^2 of iteration it into rres[(it - 1) n + worker], a hand-written branch of
# its own at every kernel family (tail mask, reduction, row index, `it - 1 < max_iter` guard). The
# same runs as above with the branch on: the K sums and the per-worker rows against
# hp_reference.chain_residual of the long-double theta history, under the bound rule of this file with
# each entry over its own reference value; heads' rows exactly 0. The objective, theta and the duals
# stay in the report: a residual branch that disturbs the iterates (the scratch buffer it shares with
# the objective's block sum in chain_small.hip) fails there. tests/test_hp_reference_cpu.py shows that a
# dropped edge, a stale theta, a 64-lane sum or a row indexed by chain position lands >= 100 bounds away.
@pytest.mark.parametrize("n,m,d", LINEAR_GRAPH)
def test_residual_linear_graph(n, m, d):
    _report("K4 linear graph %s" % ((n, m, d),), run_linear_graph(n, m, d, residual=True))


def test_residual_linear_eager_phases():
    _report("K4 linear eager (3, 80, 65)", run_linear_graph(3, 80, 65, use_graph=False, residual=True))


@pytest.mark.parametrize("n,m,d", LINEAR_PER_WORKER)
def test_residual_linear_per_worker_persistent(n, m, d, monkeypatch):
    """REG QT = 13 / 16, and the LDS kernel NC = 2, whose `lane + 64 c < d` mask has a partial second
    chunk at d = 65 and a full one at 128."""
    monkeypatch.setenv("GADMM_BLOCKED", "0")
    out, kern = run_linear_persistent(n, m, d, "per-worker", residual=True)
    assert kern == "per-worker"
    _report("K4 linear per-worker %s" % ((n, m, d),), out)


@pytest.mark.parametrize("n,m,d,pw", LINEAR_BLOCKED)
def test_residual_linear_blocked_persistent(n, m, d, pw, monkeypatch):
    monkeypatch.delenv("GADMM_BLOCKED", raising=False)
    if pw != 1:
        monkeypatch.setenv("GADMM_BLOCK_PW", str(pw))
    out, kern = run_linear_persistent(n, m, d, "blocked(", residual=True)
    assert ("pw=%d" % pw) in kern, kern
    _report("K4 linear blocked pw=%d %s" % (pw, (n, m, d)), out)


@pytest.mark.parametrize("pw", [1, 2])
def test_residual_blocked_several_owned_positions(pw, monkeypatch):
    """(13, 20, 8) with three owned positions per workgroup (GADMM_BLOCK_L=3): five worker workgroups
    and two objective workgroups. A workgroup also computes the halo positions around its own; their
    tails' residuals are computed from values that are wrong after k iterations and must not reach
    the owner's row."""
    n, m, d = 13, 20, 8
    monkeypatch.delenv("GADMM_BLOCKED", raising=False)
    monkeypatch.delenv("GADMM_BLOCK_K", raising=False)
    monkeypatch.setenv("GADMM_BLOCK_L", "3")
    monkeypatch.setenv("GADMM_BLOCK_PW", str(pw))
    eng = _linear_engine(n, m, d, residual=True)
    plan = eng.blocked_plan()
    assert plan is not None and plan[1] == 3 and plan[2] == 5 and plan[3] == pw, plan
    out, kern = run_linear_persistent(n, m, d, "blocked(", residual=True, eng=eng)
    eng.close()
    assert ("pw=%d" % pw) in kern and "L=3" in kern, kern
    _report("K4 linear blocked L=3 pw=%d %s" % (pw, (n, m, d)), out)


# a permuted static chain, and a second solve on the same engine: worker id != chain position, and every
# head of the first solve is a tail of the second (its row, 0 after the first solve, must be written)
# and the other way round (its row, non-zero after the first solve, must read exactly 0).
RESIDUAL_PATHS = [((4, 40, 33), (3, 2, 1, 0)), ((5, 40, 33), (2, 0, 4, 1, 3))]
assert dict(RESIDUAL_PATHS) == H.RESIDUAL_PATHS


@pytest.mark.parametrize("family", ["per-worker", "blocked("])
@pytest.mark.parametrize("shape,path", RESIDUAL_PATHS)
def test_residual_permuted_chain_second_solve(shape, path, family, monkeypatch):
    from gadmm_amd.parallel.topology import Placement
    n, m, d = shape
    if family == "per-worker":
        monkeypatch.setenv("GADMM_BLOCKED", "0")
    else:
        monkeypatch.delenv("GADMM_BLOCKED", raising=False)
    eng = _linear_engine(n, m, d, residual=True)
    out1, kern1 = run_linear_persistent(n, m, d, family, residual=True, eng=eng)
    first = H.linear_case(n, m, d)[3]
    eng.set_path(list(path), Placement.contiguous(n, 1), 0)
    eng.reset()
    out2, kern2 = run_linear_persistent(n, m, d, family, residual=True, eng=eng,
                                        case=lambda last: H.linear_path_case(n, m, d, path, last)[3])
    eng.close()
    second = H.linear_path_case(n, m, d, path)[3]
    assert np.any(first.tails[0] & ~second.tails[0]) and np.any(second.tails[0] & ~first.tails[0])
    if path == (3, 2, 1, 0):
        assert np.array_equal(second.tails[0], ~first.tails[0])  # every role flips
    _report("K4 linear %s identity chain %s" % (kern1, shape), out1)
    _report("K4 linear %s chain %s, second solve %s" % (kern2, path, shape), out2)


@pytest.mark.parametrize("n,m,d", LOGISTIC_GRAPH)
def test_residual_logistic_graph(n, m, d):
    _report("K4 logistic graph %s" % ((n, m, d),), run_logistic_graph(n, m, d, residual=True))


def test_residual_logistic_live_stop_rule():
    (n, m, d), tol = H.LIVE_STOP
    _report("K4 logistic graph live stop %s" % ((n, m, d),), run_logistic_graph(n, m, d, inner_tol=tol, residual=True))


@pytest.mark.parametrize("zrec", ["0", "1"])
@pytest.mark.parametrize("n,m,d", LOGISTIC_PERSISTENT)
def test_residual_logistic_persistent_kernel(n, m, d, zrec, monkeypatch):
    monkeypatch.setenv("GADMM_LOGISTIC_ZREC", zrec)
    _report("K4 logistic persistent zrec=%s %s" % (zrec, (n, m, d)), run_logistic_persistent(n, m, d, residual=True))


# ------------------------------------------------------------------------------------------------
# Star ADMM: star_variant (star_persistent.hip) takes QT = 13 at d <= 52 and 16 at 53..64
STAR_PERSISTENT = [
    (3, 7, 3),
    (4, 60, 52),     # QT = 13: the top
    (4, 70, 53),     # QT = 16: the first
    (3, 40, 64),     # QT = 16: the top; m < d
    # the hub's row layout: helper wave v of HW - 1 = 3 owns the upload rows q = v - 1, v + 2, ...
    (2, 8, 6),       # one upload row: helper waves 2 and 3 own nothing and still pass both barriers
    (5, 8, 6),       # the first n at which a helper (wave 1: rows 0 and 3) owns two rows
    (26, 60, 53),    # QT = 16 at 25 rows: wave 1 owns 9, its poll takes a second batch of SB = 8 with one
                     # wanted slot and seven masked ones (bit 8 of `got`)
]
# standard_admm (algorithms/std_admm.py) sends d > 64 to the streaming engine (star_big.hip): 256-thread
# blocks over d in sb_rhs / sb_sum / sb_hubrhs, 128-element block rows in sb_post / sb_sym_reduce /
# sb_local_obj, nb (nb + 1) / 2 stored blocks in sb_sym_part (sym_gemv.h)
STAR_BIG = [
    (3, 80, 65),     # the first d; odd d: the scalar path of wave_rows_dot in sb_obj
    (2, 70, 66),     # n = 2, one worker and the hub; even d: the double2 path of wave_rows_dot
    (4, 80, 65),     # the shape of the permuted case below, in worker order
    (4, 150, 128),   # d = B exactly
    (3, 150, 129),   # nb = 2: a transposed product inside a star solve; block row 1 with one live lane
    (3, 280, 256),   # nb = 2 full; the top of one 256-thread block
    (3, 280, 257),   # nb = 3; the second 256-thread block of sb_rhs / sb_sum / sb_hubrhs, one live thread
]
assert STAR_PERSISTENT + STAR_BIG == H.STAR_SHAPES
STAR_PERSISTENT_ORDER = ((5, 8, 6), (3, 4, 0, 2, 1))   # local order: the hub (worker 4) is workgroup 1
STAR_BIG_ORDER = ((4, 80, 65), (2, 3, 0, 1))           # the hub (worker 3) is local worker 1
STAR_STOP_AT = 11   # test_star_big_stops_in_mid_block: inside the second block of 8 iterations


def _fma(a, b, c):
    """round(a * b + c), one rounding, elementwise on float64 arrays: through exact rationals (a float
    of a Fraction is correctly rounded)."""
    from fractions import Fraction
    flat = [float(Fraction(x) * Fraction(y) + Fraction(z))
            for x, y, z in zip(np.ravel(a).tolist(), np.ravel(b).tolist(), np.ravel(c).tolist())]
    return np.asarray(flat, dtype=np.float64).reshape(np.shape(c))


def _mirror_state(lam_hub, lam, theta, hub, rho):
    """The hub keeps its own copies of the workers' duals ("same arithmetic, bit-identical",
    star_persistent.hip). When the kernel leaves they differ from the workers' own by the one step a
    worker applies lazily: lam_hub[q] = lam[q] + rho * (theta[q] - theta[hub]), in float64 in the kernel's
    operand order. Rows by worker id. Returns (entries that differ from the two-rounding evaluation,
    entries that differ from the fused one (the product unrounded into the sum), largest distance from
    the first in units of ulp(rho max|theta|))."""
    rows = [q for q in range(theta.shape[0]) if q != hub]
    diff = theta[rows] - theta[hub]
    plain = lam[rows] + rho * diff
    fused = _fma(np.full_like(diff, rho), diff, lam[rows])
    got = lam_hub[rows]
    ulp = np.spacing(rho * np.max(np.abs(theta)))
    return int(np.sum(got != plain)), int(np.sum(got != fused)), float(np.max(np.abs(got - plain)) / ulp)


def run_star_persistent(n, m, d, order=None):
    """``order``: the local order of the workers (workgroup b runs worker order[b]); None: by id."""
    from gadmm_amd.engine.star_engine import StarEngine
    X, y, rho, _ = H.star_case(n, m, d)
    order = list(range(n)) if order is None else [int(w) for w in order]
    assert sorted(order) == list(range(n))
    eng = StarEngine(_dev(X[order]), _dev(y[order]), order, n, rho, 0.0, 0.0, K)
    assert eng.eligible() and eng.last_kernel == "star-persistent"
    iters, done, _ = eng.run()
    last = int(eng.ctl.cpu()[0]) - 1  # the workers leave `lag` iterations after the cap's decision
    assert iters == K and K <= last <= K + 16, (iters, done, last)
    ref = H.star_case(n, m, d, last)[3]
    lam_hub = _host(eng.lam_hub)[: n - 1]  # the hub's copies, by worker id: updated through iteration `last`
    theta, lam = np.zeros((n, d)), np.zeros((n, d))  # by worker id
    theta[order], lam[order] = _host(eng.theta), _host(eng.lam)
    # a worker's own dual is lazy: the update of iteration `last` would come with the next broadcast
    th_l, rho_l = ref.theta[last - 1], np.asarray(rho, dtype=H.LD)
    lam_prev = ref.dual[: n - 1] - rho_l * (th_l[: n - 1] - th_l[n - 1])
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj,
           "theta": ref.err_theta(theta, last) / ref.b_theta,
           "dual": ref.err_dual(lam_hub, ref.dual[: n - 1]) / ref.b_dual,
           "worker_dual": ref.err_dual(lam[: n - 1], lam_prev) / ref.b_dual}
    assert np.all(lam[n - 1] == 0)
    # the hub's copies are the workers' duals one step on, bit for bit, in the kernel's arithmetic: both
    # sides compile to one subtraction and one FMA, so the product goes unrounded into the sum. The
    # two-rounding evaluation of the same expression is printed (on this data it agrees at every entry,
    # profiles/star_classes/README.md) and held to 2 ulp of rho max|theta|
    plain, fused, ulps = _mirror_state(lam_hub, lam, theta, n - 1, float(rho))
    print("star persistent %s%s: hub's duals against the workers' one step on: %d of %d entries differ unfused, "
          "%d fused, at most %.2f ulp(rho max|theta|)" % ((n, m, d), "" if order == list(range(n)) else " order %s" % (order,),
                                                       plain, (n - 1) * d, fused, ulps))
    assert fused == 0 and ulps <= 2.0, (plain, fused, ulps)
    return out


@pytest.mark.parametrize("n,m,d", STAR_PERSISTENT)
def test_star_persistent_kernel(n, m, d):
    _report("star persistent %s" % ((n, m, d),), run_star_persistent(n, m, d))


def test_star_persistent_hub_not_last_workgroup():
    """(5, 8, 6) in the local order (3, 4, 0, 2, 1): the hub is workgroup 1, every worker's table row and
    objective slot is its id, not its workgroup."""
    shape, order = STAR_PERSISTENT_ORDER
    _report("star persistent %s order %s" % (shape, order), run_star_persistent(*shape, order=order))


def _star_big(n, m, d, exact, order=None, max_iter=K, obj0=0.0, tol=0.0):
    """One solve of the streaming engine over the data of ``star_case`` in the local order ``order``
    (None: by id). Returns (the result, theta by worker id, lam by worker id)."""
    from gadmm_amd.algorithms import standard_admm
    from gadmm_amd.models import LinearRegression
    X, y, rho, _ = H.star_case(n, m, d)
    order = list(range(n)) if order is None else [int(w) for w in order]
    assert sorted(order) == list(range(n))
    model = LinearRegression(_dev(X[order]), _dev(y[order]))
    a = standard_admm(model, order, n, rho, obj0, tol, max_iter, engine_opts={"exact_objective": exact})
    assert a.extra["backend"] == "native" and a.extra["engine"].startswith("star-big"), a.extra
    assert a.extra["engine"] == "star-big(%s objective)" % ("exact" if exact else "identity")
    eng = a.extra["engine_obj"]
    assert eng.local == order and eng.hub_li == order.index(n - 1)
    theta, lam = np.zeros((n, d)), np.zeros((n, d))
    theta[order], lam[order] = _host(eng.theta), _host(eng.lam)
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(lam)) and np.all(lam[n - 1] == 0)
    return a, theta, lam


def _star_big_ratios(a, theta, lam, ref, k):
    return {"objective": ref.err_obj(a.obj) / ref.b_obj, "theta": ref.err_theta(theta, k) / ref.b_theta,
            "dual": ref.err_dual(lam) / ref.b_dual}


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n,m,d", STAR_BIG)
def test_star_big_kernel(n, m, d, exact):
    """The streaming star engine with its default objective (the identity A th = r - shift th of the
    solve) and with the exact one (a second GEMV by the Gram)."""
    ref = H.star_case(n, m, d)[3]
    a, theta, lam = _star_big(n, m, d, exact)
    assert a.iters == K and len(a.obj) == K
    _report("star-big %s %s" % ("exact" if exact else "identity", (n, m, d)), _star_big_ratios(a, theta, lam, ref, K))


@pytest.mark.parametrize("exact", [False, True])
def test_star_big_hub_not_last_local_worker(exact):
    """(4, 80, 65) in the local order (2, 3, 0, 1): hub_li = 1, so the `s == hub_li` skips of sb_rhs,
    sb_sum and sb_sym_* fall inside the worker loop and objp[gid[s]] scatters out of order."""
    (n, m, d), order = STAR_BIG_ORDER
    ref = H.star_case(n, m, d)[3]
    a, theta, lam = _star_big(n, m, d, exact, order=order)
    assert a.iters == K and len(a.obj) == K and a.extra["engine_obj"].hub_li == 1
    _report("star-big %s %s order %s" % ("exact" if exact else "identity", (n, m, d), order),
            _star_big_ratios(a, theta, lam, ref, K))


def test_star_big_stops_in_mid_block():
    """(3, 150, 129), identity objective, the default block of 8 iterations per host look, stopped by the
    device rule at iteration 11: obj0 is the reference's objective of iteration 11 and tol half the
    smallest gap of the ten before it (as tests/test_gpu_stop_rule.py; 0.396 = 2.5e-3 |obj0|, every
    earlier gap >= 2 tol: no engine's rounding moves the stop). The host has enqueued 16 iterations when
    it looks; the five behind the stop must be no-ops: theta and the duals are those of iteration 11."""
    n, m, d = 3, 150, 129
    full = np.asarray(H.star_case(n, m, d)[3].obj, dtype=np.float64)
    obj0 = float(full[STAR_STOP_AT - 1])
    tol = 0.5 * float(np.min(np.abs(full[:STAR_STOP_AT - 1] - obj0)))
    assert tol > 1e-6 * abs(obj0) and K > STAR_STOP_AT > 8 and STAR_STOP_AT % 8 != 0, (tol, obj0)
    ref = H.star_case(n, m, d, STAR_STOP_AT)[3]
    assert np.array_equal(ref.obj, H.star_case(n, m, d)[3].obj[:STAR_STOP_AT])
    a, theta, lam = _star_big(n, m, d, False, max_iter=K, obj0=obj0, tol=tol)
    eng = a.extra["engine_obj"]
    ctl = eng.ctl.cpu().tolist()
    trace = _host(eng.trace)
    print("star-big stop in mid-block %s: obj0 %.6f tol %.3f, iterations %d, converged %s, ctl (iter, done, conv) %s"
          % ((n, m, d), obj0, tol, a.iters, a.converged, ctl[:3]))
    assert a.iters == STAR_STOP_AT and a.converged and ctl[:3] == [STAR_STOP_AT + 1, 1, STAR_STOP_AT], (a.iters, ctl)
    assert len(a.obj) == STAR_STOP_AT and len(trace) == K and np.array_equal(trace[:STAR_STOP_AT], a.obj)
    assert np.all(np.isnan(trace[STAR_STOP_AT:])), trace
    _report("star-big stop in mid-block %s" % ((n, m, d),), _star_big_ratios(a, theta, lam, ref, STAR_STOP_AT))


# ------------------------------------------------------------------------------------------------
# Variants behind switches that are read once per process (static const in the launchers):
# GADMM_PERSIST_LDS takes pick_variant's LDS kernel with NC = 1 at d <= 64, GADMM_LOGISTIC_QUAD=0
# takes chain_phase_logistic_wave<1> at max(d, m) <= 64. monkeypatch cannot reach them.
ONCE_LINEAR = [(3, 7, 3), (5, 70, 53), (4, 40, 64)]
ONCE_LOGISTIC = [(3, 5, 3), (3, 64, 64)]


def child_main():
    """Runs in the fresh child process of test_variants_read_once_per_process: one JSON line."""
    from gadmm_amd.ops import native
    assert os.environ.get("GADMM_PERSIST_LDS") and os.environ.get("GADMM_LOGISTIC_QUAD") == "0"
    os.environ["GADMM_BLOCKED"] = "0"
    res = {}
    for s in ONCE_LINEAR:
        native.poison_lds()
        out, kern = run_linear_persistent(*s, "per-worker")
        res["linear per-worker LDS NC=1 %s" % (s,)] = out
    for s in ONCE_LOGISTIC:
        native.poison_lds()
        res["logistic graph wave<1> %s" % (s,)] = run_logistic_graph(*s)
    print("RATIOS " + json.dumps(res), flush=True)


def test_variants_read_once_per_process():
    env = dict(os.environ, GADMM_PERSIST_LDS="1", GADMM_LOGISTIC_QUAD="0",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_dispatch_classes as t; t.child_main()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RATIOS ")][-1]
    res = json.loads(line[len("RATIOS "):])
    assert len(res) == len(ONCE_LINEAR) + len(ONCE_LOGISTIC)
    for tag, ratios in res.items():
        _report(tag, ratios)
