"""Concurrent Q-GADMM solves in one launch of the persistent Q body (engine/quant_sweep.py, one solve
per XCD).

Yardstick: the GRAPH-Q engine (``eng.run()``: chain_phase_linear_q, which shares no kernel line with
the persistent body), bit for bit. The single-solve persistent Q kernel shares the sweep's body, so it
is never the only reference.

Run with: pytest -m gpu tests/test_gpu_qsweep.py
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 3.0


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu_qgadmm.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


_PROB = {}


def _problem(N, d):
    """(X (N, 50, d), y (N, 50), obj0) cut from linear_synthetic(N) by column slicing, shared. The data
    set has 50 columns: d > 50 appends seeded N(0, 1) / sqrt(50) columns (tests/test_gpu_qgadmm.py)."""
    if (N, d) not in _PROB:
        from gadmm_amd.data import linear_synthetic
        from gadmm_amd.oracle.reference import opt_linear
        ds = linear_synthetic(N)
        X = ds.X[:, :, :d]
        if d > X.shape[2]:
            extra = np.random.default_rng(64).standard_normal((N, X.shape[1], d - X.shape[2])) / np.sqrt(X.shape[1])
            X = torch.cat([X, torch.from_numpy(extra)], dim=2)
        X = X.contiguous()
        obj0 = opt_linear(X.reshape(-1, d).numpy(), ds.y.reshape(-1).numpy())
        _PROB[(N, d)] = (X, ds.y.contiguous(), float(obj0))
    return _PROB[(N, d)]


def _engine(N, d, bits, seed=1234, rho=RHO, tol=1e-8, max_iter=200, xcd=2):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, obj0 = _problem(N, d)
    eng = NativeChainEngine(X.to(DEV), y.to(DEV), list(range(N)), N, "linear", rho=rho, obj0=obj0, tol=tol,
                            max_iter=max_iter, quant=(bits, seed), xcd=xcd)
    eng.set_path(list(range(N)), Placement.contiguous(N, 1), 0)
    return eng


_GRAPH = {}


def _graph_ref(N, d, bits, seed=1234, rho=RHO, tol=1e-8, max_iter=200, stop_iter=0):
    """(done, iters, trace, th_hat, true theta, mu) of the graph-Q engine, computed once per key."""
    key = (N, d, bits, seed, rho, tol, max_iter, stop_iter)
    if key not in _GRAPH:
        eng = _engine(N, d, bits, seed=seed, rho=rho, tol=tol, max_iter=max_iter)
        eng.reset()
        r = eng.run(stop_iter=stop_iter)
        assert eng.graph_ok()
        tr = eng.objective_trace(r.iters).copy()
        tr.setflags(write=False)
        _GRAPH[key] = (r.done, r.iters, tr, eng.theta.cpu(), eng.theta_true.cpu(), eng.mu.cpu())
        eng.close()
    return _GRAPH[key]


def _check_member(m, r, N, d, bits, seed=1234, rho=RHO, tol=1e-8, max_iter=200):
    """Member ``m`` with its ``EngineRun`` against the graph-Q engine: (done, iters), the objective trace
    (device buffer and pinned read-back copy), and th_hat / true theta / duals after the kernel's last
    iteration (it learns the decision `lag` iterations late) == the graph engine run that far at tol 0
    (tests/test_gpu_qgadmm.py::test_engines_agree). Returns the trace."""
    done, iters, tr, _, _, _ = _graph_ref(N, d, bits, seed, rho, tol, max_iter)
    assert (r.done, r.iters) == (done, iters)
    assert np.array_equal(m.objective_trace(r.iters), tr)
    assert np.array_equal(m.traces(r.iters)[0], tr)
    last = m.ctl_state()["iter"] - 1
    assert iters <= last <= iters + 16
    _, it_g, tr_g, hat_g, true_g, mu_g = _graph_ref(N, d, bits, seed, rho, 0.0, max_iter + 32, stop_iter=last)
    assert it_g == last and np.array_equal(tr_g[:iters], tr)
    assert torch.equal(m.theta.cpu(), hat_g)
    assert torch.equal(m.theta_true.cpu(), true_g)
    assert torch.equal(m.mu.cpu(), mu_g)  # the heads' last dual stays pending, as in the graph engine before its flush
    return tr


def _xcc_ids(xchk):
    """XCC_IDs the blocks of a member's last launch posted (decoded as tests/test_gpu_sweep.py::_xcc_ids)."""
    g = xchk.view(-1, 4).cpu().numpy().astype(np.int64) & 0xffffffff
    tag = int(g[0][0])
    ids = []
    for t, lo, t2, hi in g:
        if not (tag & 0x80000000) or t != tag or t2 != t:
            break
        ids.append(float(np.array([(int(hi) << 32) | int(lo)], dtype=np.uint64).view(np.float64)[0]))
    return ids


def _run_members(shapes):
    """One launch of separately built members ``[(N, d, bits), ...]``; every member checked."""
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    sw = QuantSweepEngine([_engine(N, d, bits) for N, d, bits in shapes])
    runs = sw.run()
    assert sw.last_kernel == "persistent-Q-sweep(K=%d)" % len(shapes)
    assert sw.blocks() == [N + 1 for N, _, _ in shapes]
    for j, ((N, d, bits), m, r) in enumerate(zip(shapes, sw.members, runs)):
        print("slot %d N=%d d=%d b=%d: done=%d iters=%d placed=%d" % (j, N, d, bits, r.done, r.iters, sw.last_placed[j]))
        assert r.done in (1, 2) and r.iters >= 10
        _check_member(m, r, N, d, bits)
        assert sw.last_placed[j] == 2 and m.last_placed == 2
        ids = _xcc_ids(m._xchk)
        assert len(ids) == N + 1 and len(set(ids)) == 1, ids
    sw.close()


def test_mixed_slots_class_13():
    """K = 8, QT = 13: widths 2 / 3 / 8, d from 1 to 52 and all three bit widths side by side. Narrow
    slots sit beside wide ones: the wide slots' grid gives the narrow slots blocks past their own
    n + 1, which must leave before the placement check."""
    _run_members([(2, 1, 4), (3, 7, 8), (8, 50, 16), (8, 50, 4), (3, 52, 8), (2, 50, 16), (8, 7, 4), (3, 1, 16)])


def test_class_16():
    """K = 3, QT = 16 (d = 53..64)."""
    _run_members([(3, 53, 8), (8, 64, 4), (2, 64, 16)])


def test_width_one():
    """K = 1 equals the graph-Q engine and the single run_persistent result."""
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    sw = QuantSweepEngine([_engine(8, 50, 8)])
    (r,) = sw.run()
    m = sw.members[0]
    tr = _check_member(m, r, 8, 50, 8)
    assert (r.done, r.iters) == (1, 93) and sw.last_placed == [2]
    one = _engine(8, 50, 8)
    one.reset()
    r1 = one.run_persistent(fetch_trace=True)
    assert one.last_kernel.startswith("persistent-Q(")
    assert (r1.done, r1.iters) == (r.done, r.iters)
    assert np.array_equal(one.objective_trace(r1.iters), tr)
    assert one.ctl_state()["iter"] == m.ctl_state()["iter"]
    assert torch.equal(one.theta, m.theta) and torch.equal(one.theta_true, m.theta_true) and torch.equal(one.mu, m.mu)
    one.close()
    sw.close()


def _build(configs, N=8, d=50, tols=1e-8, max_iters=200, xcd=2):
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    X, y, obj0 = _problem(N, d)
    return QuantSweepEngine.build(X.to(DEV), y.to(DEV), list(range(N)), N, configs, obj0=obj0, tols=tols,
                                  max_iters=max_iters, xcd=xcd)


def test_width_eight_one_problem():
    """K = 8 on one problem (one Gram, one table of inverses): bits {4, 8} x seeds {1, 2, 3} and two
    members with the identical (8, 7). Every member equals its own graph-Q run, the twins agree, different
    seeds differ (a slot reading another slot's seed is caught), every member is verified on ONE XCD and
    the eight members sit on eight different ones."""
    configs = [(RHO, bits, seed) for bits in (4, 8) for seed in (1, 2, 3)] + [(RHO, 8, 7), (RHO, 8, 7)]
    sw = _build(configs)
    runs = sw.run()
    assert sw.last_kernel == "persistent-Q-sweep(K=8)"
    traces, seen = [], []
    for j, ((rho, bits, seed), m, r) in enumerate(zip(configs, sw.members, runs)):
        traces.append(_check_member(m, r, 8, 50, bits, seed=seed))
        assert sw.last_placed[j] == 2 and m.last_placed == 2
        ids = _xcc_ids(m._xchk)
        assert len(ids) == 9 and len(set(ids)) == 1, ids
        seen.append(ids[0])
    assert len(set(seen)) == 8, seen  # one XCD per member, eight different ones
    assert np.array_equal(traces[6], traces[7])
    assert torch.equal(sw.members[6].theta, sw.members[7].theta)
    for i in range(7):
        for j in range(i + 1, 7):
            n = min(len(traces[i]), len(traces[j]))
            assert not np.array_equal(traces[i][:n], traces[j][:n]), (i, j)
    sw.close()


def test_different_stops_in_one_launch():
    """tol 1e-4 (55 iterations), tol 1e-8 (93) and a cap of 20 iterations at tol 1e-30 side by side: each
    member has the graph engine's (done, iters), and the early finishers do not change the late one's bits."""
    tols, caps = [1e-4, 1e-8, 1e-30], [200, 200, 20]
    sw = _build([(RHO, 8, 1234)] * 3, tols=tols, max_iters=caps)
    runs = sw.run()
    assert [(r.done, r.iters) for r in runs] == [(1, 55), (1, 93), (2, 20)]
    for m, r, tol, cap in zip(sw.members, runs, tols, caps):
        _check_member(m, r, 8, 50, 8, tol=tol, max_iter=cap)
    sw.close()


def test_packed_without_the_placement_check():
    """xcd = 1 at K = 3 (packed, sc1 stores): placed == 1 and the same bits as with xcd = 2."""
    configs = [(RHO, 4, 1234), (RHO, 8, 1234), (RHO, 16, 1234)]
    got = {}
    for xcd in (1, 2):
        sw = _build(configs, xcd=xcd)
        runs = sw.run()
        assert sw.last_placed == [xcd] * 3
        got[xcd] = [_check_member(m, r, 8, 50, bits) for (_, bits, _), m, r in zip(configs, sw.members, runs)]
        sw.close()
    for a, b in zip(got[1], got[2]):
        assert np.array_equal(a, b)


def test_workload_shape():
    """The entries' batch: N = 24, d = 50, bits {4, 8} x rho {3, 5, 7}, seed 1234, to 1e-4, in one launch.
    The iteration counts are the graph engine's."""
    configs = [(rho, bits, 1234) for bits in (4, 8) for rho in (3.0, 5.0, 7.0)]
    sw = _build(configs, N=24, tols=1e-4, max_iters=1000)
    runs = sw.run()
    assert sw.blocks() == [25] * 6
    for j, ((rho, bits, seed), m, r) in enumerate(zip(configs, sw.members, runs)):
        print("slot %d rho=%g b=%d: done=%d iters=%d placed=%d" % (j, rho, bits, r.done, r.iters, sw.last_placed[j]))
        assert r.done == 1
        _check_member(m, r, 24, 50, bits, rho=rho, tol=1e-4, max_iter=1000)
        assert sw.last_placed[j] == 2
    sw.close()


def _model(N, d):
    from gadmm_amd.models.linear import LinearRegression
    X, y, obj0 = _problem(N, d)
    return LinearRegression(X.to(DEV), y.to(DEV)), obj0


def _same_results(got, ref):
    for g, r in zip(got, ref):
        assert g.iters == r.iters and g.converged == r.converged
        assert np.array_equal(g.obj, r.obj) and np.array_equal(g.comm_units, r.comm_units)
        for k in ("payload_bits", "q_granules", "q_wire_bytes", "q_bits", "q_seed"):
            assert g.extra[k] == r.extra[k], k
        assert g.primal_res is None and r.primal_res is None


def test_algorithm_results(monkeypatch):
    """quantized_group_admm_sweep == the loop of chain_admm(quantize=) for five configs; d = 70 and a CU
    budget too small for the group are that loop, with the reason."""
    from gadmm_amd.algorithms import chain_admm, quantized_group_admm_sweep
    model, obj0 = _model(8, 50)
    configs = [(3.0, 8, 1234), (5.0, 4, 1234), (3.0, 16, 7), (7.0, 8, 2), (3.0, 8, 1234)]
    ref = []
    for rho, bits, seed in configs:
        r = chain_admm(model, list(range(8)), 8, rho, obj0, 1e-8, 500, quantize=(bits, seed),
                       engine_opts={"cache": False})
        assert r.extra["kernel"].startswith("persistent-Q(")
        r.extra["engine_obj"].close()
        ref.append(r)
    for rep in range(2):  # the second sweep reuses the cached sweep engine
        got = quantized_group_admm_sweep(model, configs, obj0, 1e-8, 500)
        assert len(model._chain_engines) == 1
        _same_results(got, ref)
        for j, g in enumerate(got):
            assert "sweep_fallback" not in g.extra and "state" not in g.extra
            sx = g.extra["sweep"]
            assert (sx["width"], sx["slot"], sx["placed"]) == (5, j, 2)
            assert sx["kernel"] == g.extra["sweep_kernel"] == "persistent-Q-sweep(K=5)" and g.extra["sweep_slot"] == j
            assert len(g.time_trace) == g.iters and g.wall_s > 0
        # each member's own time: a member that ran fewer iterations of the same problem stopped earlier
        assert got[1].iters != got[0].iters and (got[1].wall_s < got[0].wall_s) == (got[1].iters < got[0].iters)

    monkeypatch.setenv("GADMM_CU_BUDGET", "3")  # 3 CUs hold one solve's 9 one-wave workgroups, not the group's 45
    low = quantized_group_admm_sweep(model, configs, obj0, 1e-8, 500)
    assert all("ResidencyError" in g.extra["sweep_fallback"] for g in low)
    assert all(g.extra["kernel"].startswith("persistent-Q(") and "sweep" not in g.extra for g in low)
    _same_results(low, ref)
    monkeypatch.delenv("GADMM_CU_BUDGET")

    m70, obj70 = _model(4, 70)
    c70 = [(3.0, 8, 1234), (3.0, 4, 1234)]
    wide = quantized_group_admm_sweep(m70, c70, obj70, 1e-6, 60, engine_opts={"cache": False})
    assert [g.extra["sweep_fallback"] for g in wide] == ["d > 64"] * 2
    assert all(g.extra["kernel"] == "graph-Q" for g in wide)
    for g, (rho, bits, seed) in zip(wide, c70):
        r = chain_admm(m70, list(range(4)), 4, rho, obj70, 1e-6, 60, quantize=(bits, seed), engine_opts={"cache": False})
        assert g.iters == r.iters and np.array_equal(g.obj, r.obj)
        r.extra["engine_obj"].close()
        g.extra["engine_obj"].close()


def _entry_summary(tmp_path, name, extra):
    """One entry run in a fresh child process under its own time limit; a failed run fails the test
    before anything else is started."""
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Synthetic", "--quick", "--no-plot",
           "--no-baselines", "--out", out, "--set", "quant_bits=4,8"] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.load(open(os.path.join(out, "summary.json")))["runs"]


def test_entry_concurrent_switch(tmp_path):
    seq = _entry_summary(tmp_path, "seq", [])
    con = _entry_summary(tmp_path, "con", ["sweep=concurrent"])
    keys = ["Q-GADMM_b%d_rho%g" % (bits, rho) for bits in (4, 8) for rho in (3, 5, 7)]
    assert sorted(k for k in seq if k.startswith("Q-GADMM")) == sorted(keys)
    assert sorted(con) == sorted(seq)
    assert [con[k]["iters"] for k in keys] == [seq[k]["iters"] for k in keys]
    assert [con[k]["converged"] for k in keys] == [seq[k]["converged"] for k in keys]
    for j, k in enumerate(keys):
        assert con[k]["algorithm"] == seq[k]["algorithm"]
        assert con[k]["sweep_kernel"] == "persistent-Q-sweep(K=6)" and con[k]["sweep_slot"] == j
        assert "sweep_fallback" not in con[k] and "sweep_kernel" not in seq[k]
