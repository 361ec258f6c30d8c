"""Concurrent solves in one launch of the blocked kernel (engine/chain_sweep.py, one solve per XCD).

Yardsticks: the GRAPH engine (``eng.run()``: chain_small.hip, a kernel family the sweep does not
share a line with), bit for bit, and the NumPy oracle on the first 50 iterations at rtol 1e-11 (both
as in tests/test_gpu.py::test_engine_graph_and_persistent_iterations). The single-solve blocked
kernel shares the sweep's body, so it is never the only reference.

Run with: pytest -m gpu tests/test_gpu_sweep.py
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
IT8 = {3.0: 1373, 5.0: 758, 7.0: 428}  # lin24 to 1e-8 (reference iteration counts)


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _member(X, y, rho, obj0, tol, max_iter):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    n = int(X.shape[0])
    eng = NativeChainEngine(X, y, list(range(n)), n, "linear", rho=rho, obj0=obj0, tol=tol, max_iter=max_iter)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    return eng


_GRAPH = {}


def _graph(key, X, y, rho, obj0, tol, max_iter, stop_iter=0):
    """(done, iters, trace, theta) of the graph engine, computed once per key and shared."""
    if key not in _GRAPH:
        eng = _member(X, y, rho, obj0, tol, max_iter)
        eng.reset()
        r = eng.run(stop_iter=stop_iter)
        assert eng.graph_ok()
        tr = eng.objective_trace(r.iters).copy()
        tr.setflags(write=False)
        _GRAPH[key] = (r.done, r.iters, tr, eng.local_theta().cpu())
        eng.close()
    return _GRAPH[key]


def _lin_graph(lin24, lin_obj0, rho, tol=1e-8, max_iter=3000):
    return _graph(("lin24", rho, tol, max_iter), lin24.X.to(DEV), lin24.y.to(DEV), rho, lin_obj0, tol, max_iter)


def _lin_sweep(lin24, lin_obj0, rhos, tols=1e-8, max_iters=3000):
    from gadmm_amd.engine.chain_sweep import ChainSweepEngine
    return ChainSweepEngine.rho_sweep(lin24.X.to(DEV), lin24.y.to(DEV), list(range(24)), 24, rhos, obj0=lin_obj0,
                                      tols=tols, max_iters=max_iters)


def _xcc_ids(xchk):
    """XCC_IDs the blocks of a member's last launch posted (decoded as tests/test_gpu.py::_xcc_ids)."""
    g = xchk.view(-1, 4).cpu().numpy().astype(np.int64) & 0xffffffff
    tag = int(g[0][0])
    ids = []
    for t, lo, t2, hi in g:
        if not (tag & 0x80000000) or t != tag or t2 != t:
            break
        ids.append(float(np.array([(int(hi) << 32) | int(lo)], dtype=np.uint64).view(np.float64)[0]))
    return ids


def test_rho_sweep_workload_shape(lin24, lin_obj0):
    """rho = 3, 5, 7 to 1e-8 side by side: reference iteration counts, traces == graph engine bit for
    bit and == the oracle on 50 iterations, every member verified on ONE XCD and the three members on
    three different ones; theta after a member's last iteration == the graph engine's after as many."""
    from gadmm_amd.oracle import reference as R
    rhos = (3.0, 5.0, 7.0)
    sw = _lin_sweep(lin24, lin_obj0, rhos)
    runs = sw.run()
    assert sw.last_kernel.startswith("blocked-sweep(K=3,")
    Xn, yn = lin24.numpy()
    seen = []
    for j, (rho, r, m) in enumerate(zip(rhos, runs, sw.members)):
        done, iters, tr, _ = _lin_graph(lin24, lin_obj0, rho)
        print("slot %d rho=%g: done=%d iters=%d placed=%d" % (j, rho, r.done, r.iters, sw.last_placed[j]))
        assert (r.done, r.iters) == (1, IT8[rho]) == (done, iters)
        assert np.array_equal(m.objective_trace(r.iters), tr)
        assert np.array_equal(m.traces(r.iters)[0], tr)  # the pinned read-back copy
        o = R.gadmm_linear(Xn, yn, rho, 50, lin_obj0, 1e-30)
        assert np.allclose(tr[:50], o.obj, rtol=1e-11)
        assert np.allclose(m.objective_trace(50), o.obj, rtol=1e-11)
        tt = m.time_trace(r.iters)
        assert np.all(np.diff(tt) > 0) and 0 < tt[-1] < 1.0  # each curve's own device clock
        # state: the kernel learns the decision `lag` iterations late and stops after iteration
        # ctl.iter - 1; the graph engine run exactly that far (tol 0: no stop rule) holds the same theta
        last = m.ctl_state()["iter"] - 1
        assert r.iters <= last <= r.iters + 16
        _, it_g, tr_g, th_g = _graph(("lin24-to", rho, last), lin24.X.to(DEV), lin24.y.to(DEV), rho, lin_obj0, 0.0,
                                     3000, stop_iter=last)
        assert it_g == last and np.array_equal(tr_g[:r.iters], tr)
        assert torch.equal(m.local_theta().cpu(), th_g)
        assert sw.last_placed[j] == 2 and m.last_placed == 2
        ids = _xcc_ids(m._xchk)
        assert len(ids) == sw.blocks()[j] and len(set(ids)) == 1, ids
        seen.append(ids[0])
    assert len(set(seen)) == 3, seen  # one XCD per member, three different ones
    sw.close()


def test_width_one(lin24, lin_obj0):
    sw = _lin_sweep(lin24, lin_obj0, (3.0,))
    (r,) = sw.run()
    done, iters, tr, _ = _lin_graph(lin24, lin_obj0, 3.0)
    assert (r.done, r.iters) == (done, iters) == (1, 1373)
    assert np.array_equal(sw.members[0].objective_trace(r.iters), tr)
    sw.close()


def test_width_eight(lin24, lin_obj0):
    rhos = tuple(float(r) for r in range(1, 9))
    sw = _lin_sweep(lin24, lin_obj0, rhos, tols=1e-4, max_iters=3000)
    runs = sw.run()
    for rho, r, m in zip(rhos, runs, sw.members):
        done, iters, tr, _ = _lin_graph(lin24, lin_obj0, rho, tol=1e-4)
        print("rho=%g: graph (%d, %d) sweep (%d, %d)" % (rho, done, iters, r.done, r.iters))
        assert (r.done, r.iters) == (done, iters)
        assert np.array_equal(m.objective_trace(r.iters), tr)
    assert sw.last_placed == [2] * 8
    sw.close()


@pytest.mark.parametrize("d,m", [(3, 7), (14, 25), (34, 36), (50, 25)])
def test_smallest_shapes_mixed_block_counts(d, m):
    """Members of 2 (degree-1 workers only), 3, 5 and 9 workers in one launch, both register classes
    (d <= 32, 33..52): slots with different workgroup counts, so a block past its slot's count must
    leave before the placement check. Whatever ends a run (tolerance or the 300-iteration cap), each
    member's (done, iters) and trace equal the graph engine's on the same data."""
    from gadmm_amd.engine.chain_sweep import ChainSweepEngine
    members, refs = [], []
    for n in (2, 3, 5, 9):
        g = torch.Generator().manual_seed(1000 * d + n)
        X = torch.randn(n, m, d, dtype=torch.float64, generator=g)
        th = torch.randn(d, dtype=torch.float64, generator=g)
        y = X @ th + 0.1 * torch.randn(n, m, dtype=torch.float64, generator=g)
        Xf, yf = X.reshape(n * m, d).numpy(), y.reshape(n * m).numpy()
        sol = np.linalg.lstsq(Xf, yf, rcond=None)[0]
        obj0 = 0.5 * float(np.sum((Xf @ sol - yf) ** 2))
        Xd, yd = X.to(DEV), y.to(DEV)
        refs.append(_graph(("gauss", d, m, n), Xd, yd, 1.0, obj0, 1e-6, 300))
        members.append(_member(Xd, yd, 1.0, obj0, 1e-6, 300))
    sw = ChainSweepEngine(members)
    assert len(set(sw.blocks())) > 1, sw.blocks()
    runs = sw.run()
    for n, r, mem, (done, iters, tr, _) in zip((2, 3, 5, 9), runs, members, refs):
        print("d=%d m=%d n=%d: graph (%d, %d) sweep (%d, %d)" % (d, m, n, done, iters, r.done, r.iters))
        assert (r.done, r.iters) == (done, iters)
        assert np.array_equal(mem.objective_trace(r.iters), tr)
    assert sw.last_placed == [2] * 4
    sw.close()


def test_one_member_stops_at_its_cap(lin24, lin_obj0):
    sw = _lin_sweep(lin24, lin_obj0, (3.0, 7.0), max_iters=[200, 3000])
    r0, r1 = sw.run()
    done, iters, tr, _ = _lin_graph(lin24, lin_obj0, 3.0, max_iter=200)
    assert (done, iters) == (2, 200)  # the graph engine's not-converged code at the cap
    assert (r0.done, r0.iters) == (done, iters) and not r0.converged
    assert np.array_equal(sw.members[0].objective_trace(200), tr)
    assert (r1.done, r1.iters) == (1, 428)
    assert np.array_equal(sw.members[1].objective_trace(428), _lin_graph(lin24, lin_obj0, 7.0)[2])
    sw.close()


def test_placement_fast_path_is_speed_only(lin24, lin_obj0, monkeypatch):
    rhos = (3.0, 5.0, 7.0)
    got = {}
    for x in ("1", "2"):
        monkeypatch.setenv("GADMM_XCD", x)
        sw = _lin_sweep(lin24, lin_obj0, rhos)
        runs = sw.run()
        got[x] = ([r.iters for r in runs], [m.objective_trace(r.iters).copy() for m, r in zip(sw.members, runs)],
                  list(sw.last_placed))
        sw.close()
    assert got["1"][2] == [1, 1, 1] and got["2"][2] == [2, 2, 2]
    assert got["1"][0] == got["2"][0] == [IT8[r] for r in rhos]
    for a, b, rho in zip(got["1"][1], got["2"][1], rhos):
        assert np.array_equal(a, b)
        assert np.array_equal(a, _lin_graph(lin24, lin_obj0, rho)[2])


def test_residency_fallback(lin24, lin_obj0, monkeypatch):
    """A CU budget below the three members' workgroups: the launcher refuses before launching
    (ResidencyError, no spin runs into a deadline) and chain_admm_sweep runs the loop instead."""
    from gadmm_amd.algorithms import chain_admm_sweep
    from gadmm_amd.engine.chain_engine import ResidencyError
    from gadmm_amd.models import LinearRegression
    rhos = (3.0, 5.0, 7.0)
    sw = _lin_sweep(lin24, lin_obj0, rhos)
    total = sum(sw.blocks())
    k, L, W, pw = sw.members[0].blocked_plan()
    assert total == 3 * (W + 2 + 1)
    monkeypatch.setenv("GADMM_CU_BUDGET", str(total - 1))
    with pytest.raises(ResidencyError):
        sw.run()
    for m in sw.members:  # nothing ran: the reset state is untouched
        st = m.ctl_state()
        assert st["done"] == 0 and st["iter"] == 1
        assert np.all(np.isnan(m.objective_trace(5)))
    sw.close()
    model = LinearRegression(lin24.X.to(DEV), lin24.y.to(DEV))
    res = chain_admm_sweep(model, list(range(24)), 24, rhos, lin_obj0, 1e-8, 3000, engine_opts={"cache": False})
    assert [r.iters for r in res] == [1373, 758, 428]
    assert all("ResidencyError" in r.extra["sweep_fallback"] for r in res)
    for r, rho in zip(res, rhos):
        assert np.array_equal(r.obj, _lin_graph(lin24, lin_obj0, rho)[2])


def test_refresh_and_repeat(lin24, lin_obj0):
    """Two refresh + run cycles on one engine: fresh tag salts and placement tags, no memset between."""
    rhos = (3.0, 5.0, 7.0)
    X, y = lin24.X.to(DEV), lin24.y.to(DEV)
    sw = _lin_sweep(lin24, lin_obj0, rhos)
    cycles = []
    for _ in range(2):
        sw.refresh(X, y)
        runs = sw.run()
        cycles.append([(r.done, r.iters, m.objective_trace(r.iters).copy()) for m, r in zip(sw.members, runs)])
        assert sw.last_placed == [2, 2, 2]
    for a, b, rho in zip(cycles[0], cycles[1], rhos):
        assert a[:2] == b[:2] == (1, IT8[rho])
        assert np.array_equal(a[2], b[2])
        assert np.array_equal(a[2], _lin_graph(lin24, lin_obj0, rho)[2])
    sw.close()


def test_algorithm_results(lin24, lin_obj0):
    """chain_admm_sweep on the device: one result per rho in the order given, each curve with its own
    clock; the slowest member's wall time is the launch's, the others' are shorter."""
    from gadmm_amd.algorithms import chain_admm_sweep
    from gadmm_amd.models import LinearRegression
    model = LinearRegression(lin24.X.to(DEV), lin24.y.to(DEV))
    rhos = (7.0, 3.0, 5.0)
    for rep in range(2):  # the second sweep reuses the cached sweep engine
        res = chain_admm_sweep(model, list(range(24)), 24, rhos, lin_obj0, 1e-8, 3000,
                               engine_opts={"refresh": rep == 1})
        assert len(model._chain_engines) == 1
        for j, (r, rho) in enumerate(zip(res, rhos)):
            assert "sweep_fallback" not in r.extra
            assert r.iters == IT8[rho] and r.converged
            assert np.array_equal(r.obj, _lin_graph(lin24, lin_obj0, rho)[2])
            sx = r.extra["sweep"]
            assert (sx["width"], sx["slot"], sx["placed"]) == (3, j, 2) and sx["kernel"].startswith("blocked-sweep")
            assert len(r.time_trace) == r.iters and r.primal_res is not None and len(r.primal_res) == r.iters
        assert res[1].wall_s > res[2].wall_s > res[0].wall_s > 0  # 1373 > 758 > 428 iterations
        assert abs(res[1].wall_s - max(r.wall_s for r in res)) == 0.0


def _entry_summary(tmp_path, name, extra):
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Synthetic", "--quick", "--no-plot",
           "--no-baselines", "--out", out] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.load(open(os.path.join(out, "summary.json")))["runs"]


def test_entry_concurrent_switch(tmp_path):
    seq = _entry_summary(tmp_path, "seq", [])
    con = _entry_summary(tmp_path, "con", ["--set", "sweep=concurrent"])
    keys = ["GADMM_rho3", "GADMM_rho5", "GADMM_rho7"]
    assert [con[k]["iters"] for k in keys] == [seq[k]["iters"] for k in keys]
    assert [con[k]["converged"] for k in keys] == [seq[k]["converged"] for k in keys]
    assert con["GADMM_rho7"]["iters"] == 248
    for j, k in enumerate(keys):
        assert "blocked-sweep" in con[k]["sweep_kernel"] and con[k]["sweep_slot"] == j
        assert "sweep_kernel" not in seq[k]
