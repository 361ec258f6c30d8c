"""Every kernel and engine that re-chains (D-GADMM) against a long-double reference of the re-chaining
recurrence.

The rest of the suite holds one D-GADMM kernel against another bit for bit, almost only at N = 24,
d = 50, over find_path2 draws: a mistake the kernels share with the epoch tables they all read passes.
Here every dispatch class that can run a re-chain -- the per-worker kernel's dynamic mode (register
kernel QT = 13 / 16 with both degree variants resident, LDS kernel NC = 2 with the exact and with the
identity objective, LDS kernel NC = 1), the blocked kernel's dynamic mode (DB = 32 / 52, one and several
workgroups, temporal depths), epoch chunks (hard stop + continuation), the epoch-by-epoch engine on the
phase kernels, and the dynamic sweep -- runs K = 20 iterations of a tiny problem over PRESCRIBED chains
(tests/hp_reference.py: dgadmm_chains; a reversal, a rotation that flips every role and moves the
ends, the same chain again, a random permutation, from an initial chain that is not the identity) with
no stop rule (tol = 0, obj0 = 0). theta, the duals and every objective value are compared with
hp_reference.dgadmm_linear in long double under the bound of tests/test_gpu_dispatch_classes.py,

    err_kernel <= 8 * max(e64, max(d, 16) * 2^-53),

e64 being the distance of the float64 run of the same re-chaining recurrence from its long-double run.
tests/test_hp_reference_cpu.py shows, on these very cases, that ignoring a re-chain, flushing a
head's pending dual with the new chain, or taking the old degree's inverse lands >= 1000 bounds away.
A persistent kernel stops ``last - K <= 16`` iterations after the cap and re-chains at none of them:
the reference runs to ``last`` over chains that end at K.
These solves run with the K4 primal residual on (the algorithm's default): the K sums the solve returns
and the per-worker rows of the engine are held to hp_reference.chain_residual over the case's chains -- a
worker's row is non-zero exactly in the iterations in which it is a tail, and is indexed by worker id,
not by chain position (profiles/residual_classes/README.md).
Each test prints err / bound; profiles/dgadmm_classes/README.md records the measured table.

Each parameter list names the dispatch condition that puts its shape in its class: if a threshold
moves, the list next to it is the one to revisit.

Run with: pytest -m gpu tests/test_gpu_dgadmm_classes.py -s
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hp_reference as H
from test_gpu_dispatch_classes import _dev, _host, _report, _residual_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = H.K_ITERS


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _count_launches(monkeypatch):
    """Counts the persistent launches of the solves that follow (``run_persistent`` calls)."""
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    calls = []
    inner = NativeChainEngine.run_persistent

    def counted(self, *a, **kw):
        calls.append(kw.get("hard_stop", 0))
        return inner(self, *a, **kw)

    monkeypatch.setattr(NativeChainEngine, "run_persistent", counted)
    return calls


def solve(n, m, d, coh, engine, **opts):
    """``dynamic_group_admm_v0`` over the prescribed chains of the case: ``(ratios, engine object)``.
    ``engine``: the ``extra["engine"]`` the solve must report. The state is after iteration ``last``:
    K exactly on the epoch-by-epoch engine, up to 16 later on a persistent kernel."""
    from gadmm_amd.algorithms import dynamic_group_admm_v0
    from gadmm_amd.models import LinearRegression
    X, y, rho = H.make_linear(n, m, d, H.seed_of(n, m, d))
    chains = H.dgadmm_chains(n, K, coh)
    P, C = H.dgadmm_matrices(chains)
    model = LinearRegression(_dev(X), _dev(y))
    a = dynamic_group_admm_v0(model, rho, 0.0, 0.0, K, P, C, coh, faithful_initial_cost=False,
                              engine_opts=dict({"cache": False}, **opts))
    eng = a.extra["engine_obj"]
    assert a.extra["backend"] == "native" and a.extra["engine"] == engine, a.extra
    theta, mu, nxt = a.extra["state"]
    last = nxt - 1
    assert a.iters == K and len(a.obj) == K and not a.converged, (a.iters, len(a.obj))
    if engine == "epochs":
        assert last == K, last
    else:
        assert K <= last <= K + H.PERSISTENT_OVERRUN, last
    X2, y2, rho2, chains2, ref = H.dgadmm_case(n, m, d, coh, last)
    assert chains2 == chains and rho2 == rho and np.array_equal(X2, X)
    th, du = _host(theta), _host(mu)
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(du)) and np.all(np.isfinite(a.obj))
    # the K4 primal residual, on by the algorithm's default: the K sums the solve returns over the case's
    # chains and the per-worker rows behind them (a worker's row is non-zero exactly while it is a tail)
    assert a.primal_res is not None and len(a.primal_res) == K and np.all(np.isfinite(a.primal_res))
    return {"objective": ref.err_obj(a.obj) / ref.b_obj, "theta": ref.err_theta(th, last) / ref.b_theta,
            "dual": ref.err_dual(du) / ref.b_dual, "residual": ref.err_res(a.primal_res) / ref.b_res,
            "residual rows": _residual_rows(eng, ref)}, eng


def _lds_thresholds():
    """``(the last d whose dynamic LDS kernel fits three d x d matrices, the last eligible d)`` from the
    launcher's own formula (chain_persistent.hip: gadmm_chain_persistent_lds_dyn, both inverses and,
    with the exact objective, the Gram in LDS)."""
    from gadmm_amd.ops import native
    lib = native.require()
    fits = lambda d, mode: int(lib.gadmm_chain_persistent_lds_dyn(d, mode, 2)) > 0  # noqa: E731
    exact = max(d for d in range(65, 130) if fits(d, 0))
    ident = max(d for d in range(65, 130) if fits(d, 1))
    assert all(fits(d, 0) for d in range(65, exact + 1)) and all(fits(d, 1) for d in range(65, ident + 1))
    return exact, ident


def _coh(shapes, cohs):
    return [s + (c,) for s in shapes for c in cohs]


# ------------------------------------------------------------------------------------------------
# Per-worker kernel, dynamic mode (GADMM_BLOCKED_DYN=0). pick_variant (chain_persistent.hip), `dyn`
# branch: the register kernel with NV = 2 inverses per worker at d <= DREG = 64 -- QT = 13 at d <= 52,
# QT = 16 at 53..64 -- and above it the LDS kernel NC = 2 with both inverses in LDS.
PER_WORKER_REG = _coh([
    (2, 3, 1),       # QT = 13: two workers, one inverse variant (nvar = 1), every re-chain swaps the roles
    (3, 7, 3),       # QT = 13: one interior worker; a rotation makes it an end
    (5, 40, 32),     # QT = 13
    (4, 40, 33),     # QT = 13
    (5, 60, 52),     # QT = 13: the top
    (5, 70, 53),     # QT = 16: the first
    (4, 40, 64),     # QT = 16: the top; m < d
], (1, 3)) + [(5, 60, 52, 7), (5, 60, 52, K)]   # two re-chains; one, at the cap itself
assert {c[:3] for c in PER_WORKER_REG} == set(H.DGADMM_SMALL + H.DGADMM_REG16)


@pytest.mark.parametrize("n,m,d,coh", PER_WORKER_REG)
def test_per_worker_dynamic_register_kernel(n, m, d, coh, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "0")
    out, eng = solve(n, m, d, coh, "persistent-dynamic")
    assert eng.last_kernel == "per-worker" and eng.nvar == (1 if n == 2 else 2) and eng._obj_mode(True) == 0
    eng.close()
    _report("D-GADMM per-worker REG %s coh %d" % ((n, m, d), coh), out)


# LDS kernel NC = 2: gadmm_chain_persistent_lds_dyn(d, obj_mode, 2) fits both inverses AND the Gram
# (obj_mode 0, the exact objective) up to d = 81; from 82 the engine switches to the identity objective
# (obj_mode 1: _obj_mode(True)), which fits up to d = 99; at 100 the dynamic kernel is not eligible and
# the solve runs epoch by epoch on the phase kernels.
LDS_DYNAMIC = _coh(H.DGADMM_LDS_EXACT + H.DGADMM_LDS_IDENTITY, (1, 3))


@pytest.mark.parametrize("n,m,d,coh", LDS_DYNAMIC)
def test_per_worker_dynamic_lds_kernel(n, m, d, coh, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "0")
    exact, ident = _lds_thresholds()
    assert [s[2] for s in H.DGADMM_LDS_EXACT] == [65, exact], exact
    assert [s[2] for s in H.DGADMM_LDS_IDENTITY] == [exact + 1, ident], (exact, ident)
    out, eng = solve(n, m, d, coh, "persistent-dynamic")
    assert eng.last_kernel == "per-worker" and eng.nvar == 2 and eng.dynamic_eligible()
    assert eng._obj_mode(True) == (0 if d <= exact else 1)
    eng.close()
    _report("D-GADMM per-worker LDS NC=2 %s objective %s coh %d"
            % ("exact" if d <= exact else "identity", (n, m, d), coh), out)


def test_first_ineligible_d_runs_epoch_by_epoch():
    exact, ident = _lds_thresholds()
    n, m, d = H.DGADMM_INELIGIBLE
    assert d == ident + 1
    out, eng = solve(n, m, d, 3, "epochs")
    assert not eng.dynamic_eligible() and eng._lds_need(True, 1) <= 0 and getattr(eng, "last_kernel", None) is None
    eng.close()
    _report("D-GADMM not eligible -> epochs %s coh 3" % ((n, m, d),), out)


# GADMM_PERSIST_LDS (read once per process: static const in pick_variant) sends d <= 64 to the LDS
# kernel NC = 1, here with both inverses and the Gram in LDS. monkeypatch cannot reach it: a child.
ONCE_LDS = (4, 40, 64, 3)


def child_main():
    """Runs in the fresh child process of test_per_worker_dynamic_lds_nc1: one JSON line."""
    from gadmm_amd.ops import native
    assert os.environ.get("GADMM_PERSIST_LDS") and os.environ.get("GADMM_BLOCKED_DYN") == "0"
    native.poison_lds()
    out, eng = solve(*ONCE_LDS, "persistent-dynamic")
    res = {"ratios": out, "kernel": eng.last_kernel, "capacity": eng.resident_capacity(dynamic=True),
           "obj_mode": eng._obj_mode(True)}
    print("RESULT " + json.dumps(res), flush=True)


def test_per_worker_dynamic_lds_nc1():
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    assert os.environ.get("GADMM_PERSIST_LDS") is None
    n, m, d, coh = ONCE_LDS
    env = dict(os.environ, GADMM_PERSIST_LDS="1", GADMM_BLOCKED_DYN="0",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_dgadmm_classes as t; t.child_main()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["kernel"] == "per-worker" and res["obj_mode"] == 0
    # the LDS kernel keeps three 64 x 64 matrices per workgroup in LDS, the register kernel a staging
    # area: fewer of its workgroups fit a CU, which tells the two apart from outside
    X, y, rho = H.make_linear(n, m, d, H.seed_of(n, m, d))
    eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "linear", rho=rho, obj0=0.0, tol=0.0, max_iter=K)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    here = eng.resident_capacity(dynamic=True)
    eng.close()
    assert 0 < res["capacity"] < here, (res["capacity"], here)
    _report("D-GADMM per-worker LDS NC=1 %s coh %d" % ((n, m, d), coh), res["ratios"])


# ------------------------------------------------------------------------------------------------
# Blocked kernel, dynamic mode (GADMM_BLOCKED_DYN=1): gadmm_chain_blocked_plan2 (chain_blocked.hip)
# plans d <= 52 only; chain_blocked_kernel<32> at d <= 32, <52> at 33..52 (gadmm_chain_blocked_pad_dim).
# A workgroup computes 12 chain positions: n > 12 is the first size at which the positions of a chain
# spread over several of them and a re-chain moves a worker, its dual and its halo across workgroups.
BLOCKED = _coh([
    (2, 3, 1),       # DB = 32
    (3, 7, 3),       # DB = 32
    (5, 40, 32),     # DB = 32: the top
    (4, 40, 33),     # DB = 52: the first
    (5, 60, 52),     # DB = 52: the top
    (13, 20, 8),     # DB = 32, n > 12
    (25, 12, 5),     # DB = 32, n > 24: three groups of positions
    (13, 60, 52),    # DB = 52, n > 12
], (1, 3)) + [(13, 20, 8, 7), (13, 20, 8, K)]
assert {c[:3] for c in BLOCKED} == set(H.DGADMM_SMALL + H.DGADMM_MULTI_WG)


def _plan_of(kernel):
    """{"k": .., "L": .., "W": .., "pw": ..} of a ``blocked-dyn(k=2,L=1,W=13,pw=1)`` kernel name."""
    assert kernel.startswith("blocked-dyn(") and kernel.endswith(")"), kernel
    return {k: int(v) for k, v in (kv.split("=") for kv in kernel[len("blocked-dyn("):-1].split(","))}


@pytest.mark.parametrize("n,m,d,coh", BLOCKED)
def test_blocked_dynamic_kernel(n, m, d, coh, monkeypatch):
    from gadmm_amd.ops import native
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "1")
    monkeypatch.delenv("GADMM_BLOCK_K", raising=False)
    out, eng = solve(n, m, d, coh, "persistent-dynamic")
    plan = _plan_of(eng.last_kernel)
    assert plan["pw"] == 1 and plan["W"] * plan["L"] >= n and (plan["W"] > 1 or n <= 12), eng.last_kernel
    assert int(native.require().gadmm_chain_blocked_pad_dim(d)) == (32 if d <= 32 else 52)
    eng.close()
    _report("D-GADMM blocked-dyn DB=%d %s coh %d" % (32 if d <= 32 else 52, (n, m, d), coh), out)


# temporal depth k (iterations per halo hand-off), GADMM_BLOCK_K: the 12-wave planner grants k with
# 12 - 4 k >= 1 owned positions, and falls back to the deepest that fits otherwise
@pytest.mark.parametrize("coh", [1, 3])
@pytest.mark.parametrize("want", [1, 2, 3])
def test_blocked_dynamic_temporal_depths(want, coh, monkeypatch):
    import ctypes
    from gadmm_amd.ops import native
    n, m, d = 13, 20, 8
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "1")
    monkeypatch.setenv("GADMM_BLOCK_K", str(want))
    kk, ll, pp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert native.require().gadmm_chain_blocked_plan2(n, d, want, 0, ctypes.byref(kk), ctypes.byref(ll),
                                                      ctypes.byref(pp)) > 0
    granted = kk.value
    assert 1 <= granted <= want and (granted == want or 12 - 4 * want < 1), (want, granted)
    out, eng = solve(n, m, d, coh, "persistent-dynamic")
    assert _plan_of(eng.last_kernel)["k"] == granted, (eng.last_kernel, granted)
    eng.close()
    _report("D-GADMM blocked-dyn GADMM_BLOCK_K=%d (k=%d) %s coh %d" % (want, granted, (n, m, d), coh), out)


# GADMM_BLOCKED_DYN unset: dynamic_uses_blocked takes the blocked kernel from coherence
# BLOCKED_DYN_MIN_COHERENCE = 3 on, the per-worker kernel below
@pytest.mark.parametrize("coh,family", [(1, "per-worker"), (3, "blocked-dyn(")])
def test_default_dispatch(coh, family, monkeypatch):
    monkeypatch.delenv("GADMM_BLOCKED_DYN", raising=False)
    n, m, d = 5, 60, 52
    out, eng = solve(n, m, d, coh, "persistent-dynamic")
    assert eng.last_kernel.startswith(family) and eng.BLOCKED_DYN_MIN_COHERENCE == 3, eng.last_kernel
    eng.close()
    _report("D-GADMM default dispatch -> %s %s coh %d" % (family, (n, m, d), coh), out)


# ------------------------------------------------------------------------------------------------
# Epoch chunks: engine_opts["epoch_chunk"] = 2 ends the first launch at a hard stop after two epochs;
# every continuation (cont=True, the same tag salt, the previous chunk's last epoch first, whose heads'
# pending duals are flushed with that chain) takes twice as many.
CHUNKED = _coh([(5, 60, 52), (13, 20, 8)], (1, 3))
CHUNKED_PER_WORKER = _coh([(5, 60, 52), (3, 80, 65)], (1, 3))


def _chunked(n, m, d, coh, monkeypatch, family):
    calls = _count_launches(monkeypatch)
    out, eng = solve(n, m, d, coh, "persistent-dynamic", epoch_chunk=2)
    assert eng.last_kernel.startswith(family), eng.last_kernel
    assert len(calls) > 1 and all(h > 0 for h in calls[:-1]) and calls[-1] == 0, calls
    eng.close()
    return out, len(calls)


@pytest.mark.parametrize("n,m,d,coh", CHUNKED)
def test_epoch_chunks_blocked(n, m, d, coh, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "1")
    out, launches = _chunked(n, m, d, coh, monkeypatch, "blocked-dyn(")
    _report("D-GADMM blocked-dyn epoch_chunk=2 (%d launches) %s coh %d" % (launches, (n, m, d), coh), out)


@pytest.mark.parametrize("n,m,d,coh", CHUNKED_PER_WORKER)
def test_epoch_chunks_per_worker(n, m, d, coh, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "0")
    out, launches = _chunked(n, m, d, coh, monkeypatch, "per-worker")
    _report("D-GADMM per-worker epoch_chunk=2 (%d launches) %s coh %d" % (launches, (n, m, d), coh), out)


# ------------------------------------------------------------------------------------------------
# Epoch by epoch (engine_opts["persistent"] = False): the phase kernels up to the iteration before a
# re-chain, flush_duals with the old chain, set_path, on. gadmm_chain_phase (chain_small.hip) takes
# chain_phase_linear<1> at d <= 64, <2> at 65..128, <4> at 129..256 and chain_big.hip above. The state
# is the one after exactly K iterations.
EPOCHS = [(3, 7, 3, 3), (3, 80, 65, 3), (3, 80, 65, 1), (3, 150, 129, 3),
          (3, 280, 257, 3)]   # (the one test that builds the d = 257 reference)
assert {c[:3] for c in EPOCHS} == set(H.DGADMM_GRAPH)


@pytest.mark.parametrize("n,m,d,coh", EPOCHS)
def test_epoch_by_epoch_engine(n, m, d, coh):
    out, eng = solve(n, m, d, coh, "epochs", persistent=False)
    assert getattr(eng, "last_kernel", None) is None and eng.ctl_state()["iter"] == K + 1
    eng.close()
    _report("D-GADMM epoch by epoch %s coh %d" % ((n, m, d), coh), out)


# ------------------------------------------------------------------------------------------------
# Dynamic sweep (engine/dyn_sweep.py): four members with their own data, worker counts and coherences
# in one launch of chain_blocked_dyn_sweep_kernel, one per XCD; d = 33 is the DB = 52 register class.
def test_dynamic_sweep_members():
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.engine.dyn_sweep import DynSweepEngine
    from gadmm_amd.parallel.topology import PathSchedule, Placement
    members, scheds, cases = [], [], []
    for (n, m, d), coh in H.DGADMM_SWEEP:
        X, y, rho = H.make_linear(n, m, d, H.seed_of(n, m, d))
        chains = H.dgadmm_chains(n, K, coh)
        P, C = H.dgadmm_matrices(chains)
        eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "linear", rho=rho, obj0=0.0, tol=0.0, max_iter=K)
        sc = PathSchedule(n, P[0], C[0], coh, kind="matrix", path_matrix=P, cost_matrix=C)
        eng.set_path(sc.path, Placement.contiguous(n, 1), 0)
        members.append(eng)
        scheds.append(sc)
        cases.append((n, m, d, coh, chains))
    assert [c[3] for c in cases] == [1, 3, 7, 3] and [c[0] for c in cases] == [2, 3, 5, 13]
    sw = DynSweepEngine(members)
    runs = sw.run(scheds)
    assert sw.last_kernel.startswith("blocked-dyn-sweep(K=4,"), sw.last_kernel
    assert all(p in (1, 2) for p in sw.last_placed), sw.last_placed
    res = {}
    for (n, m, d, coh, chains), mem, r in zip(cases, members, runs):
        last = int(r.last_launched)
        assert r.iters == K and r.done == 2 and K <= last <= K + H.PERSISTENT_OVERRUN, (r.iters, r.done, last)
        assert mem.last_kernel == sw.last_kernel and [list(p) for p in r.paths] == [p for _, p in chains]
        ref = H.dgadmm_case(n, m, d, coh, last)[4]
        th = _host(mem.local_theta())
        mem.set_path(chains[-1][1], Placement.contiguous(n, 1), 0)  # the chain of iteration `last`
        mem.flush_duals()
        mem.stream.synchronize()
        mu = _host(mem.mu)
        assert np.all(np.isfinite(th)) and np.all(np.isfinite(mu))
        res[(n, m, d, coh)] = {"objective": ref.err_obj(mem.objective_trace(K)) / ref.b_obj,
                               "theta": ref.err_theta(th, last) / ref.b_theta, "dual": ref.err_dual(mu) / ref.b_dual}
    sw.close()
    for (n, m, d, coh), out in res.items():
        _report("D-GADMM sweep member %s coh %d" % ((n, m, d), coh), out)
