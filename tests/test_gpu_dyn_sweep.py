"""Concurrent D-GADMM solves, one per XCD, in rounds of epoch-chunk launches of the blocked kernel's
dynamic mode (engine/dyn_sweep.py, algorithms.dynamic_group_admm_sweep).

Yardstick: the sequential ``dynamic_group_admm`` of every member on the single-solve dynamic blocked
kernel (``GADMM_BLOCKED_DYN=1``, a fresh engine per solve), bit for bit (``np.array_equal``); one
member is also held against the NumPy oracle at the tolerance of
tests/test_algorithms.py::test_dgadmm_matches_oracle_with_rechaining, and the small shapes against
the epoch-by-epoch graph engine, which shares no kernel with the sweep.

Run with: pytest -m gpu tests/test_gpu_dyn_sweep.py
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
RHO, TOL, CAP = 1.0, 1e-4, 3000


@pytest.fixture(autouse=True)
def _poison_lds(monkeypatch):
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu_sweep.py); the sequential
    references run on the blocked kernel's dynamic mode at every coherence."""
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "1")
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


@pytest.fixture(scope="module")
def chain24():
    from gadmm_amd.parallel import topology as T
    p0, c0, _ = T.find_path(24, np.random.default_rng(5))
    return p0, c0


@pytest.fixture()
def model24(lin24):
    from gadmm_amd.models import LinearRegression
    return LinearRegression(lin24.X.to(DEV), lin24.y.to(DEV))


_SEQ = {}


def _seq(lin24, lin_obj0, chain24, coh, seed, max_iter=CAP, chunk=None):
    """The sequential solve of one member, computed once per key on a fresh engine and shared:
    (iters, converged, obj, com_cost, comm_units, primal_res), read-only."""
    key = (coh, seed, max_iter)  # (the chunk size changes launches only, never results: not in the key)
    if key not in _SEQ:
        from gadmm_amd.algorithms import dynamic_group_admm
        from gadmm_amd.models import LinearRegression
        m = LinearRegression(lin24.X.to(DEV), lin24.y.to(DEV))
        opts = {"cache": False}
        if chunk is not None:
            opts["epoch_chunk"] = chunk
        r = dynamic_group_admm(m, RHO, lin_obj0, TOL, max_iter, chain24[0], chain24[1], coh, seed=seed,
                               engine_opts=opts)
        r.extra["engine_obj"].close()
        arrs = [np.array(a) for a in (r.obj, r.com_cost, r.comm_units, r.primal_res)]
        for a in arrs:
            a.setflags(write=False)
        _SEQ[key] = (int(r.iters), bool(r.converged), *arrs)
    return _SEQ[key]


def _equal(res, ref):
    iters, conv, obj, com, units, pres = ref
    print("%s: sweep (%d, %s) sequential (%d, %s) sweep=%s" % (res.algorithm, res.iters, res.converged, iters, conv,
                                                              res.extra.get("sweep")))
    assert "sweep_fallback" not in res.extra
    assert (res.iters, res.converged) == (iters, conv)
    assert np.array_equal(res.obj, obj)
    assert np.array_equal(res.com_cost, com)
    assert np.array_equal(res.comm_units, units)
    assert res.primal_res is not None and np.array_equal(res.primal_res, pres)
    assert len(res.time_trace) == iters and "state" not in res.extra


def _sweep(model, lin_obj0, chain24, cohs, seeds, max_iter=CAP, **kw):
    from gadmm_amd.algorithms import dynamic_group_admm_sweep
    kw.setdefault("engine_opts", {"cache": False})
    return dynamic_group_admm_sweep(model, RHO, lin_obj0, TOL, max_iter, chain24[0], chain24[1], cohs, seeds, **kw)


def _close(res):
    for r in res:
        r.extra["engine_obj"].close()


def test_workload_shape(lin24, lin_obj0, chain24, model24):
    """E7's set: coherences 1, 10, 50 side by side; every member == its sequential run, verified on one
    XCD or packed; the coherence-10 member == the NumPy oracle."""
    from gadmm_amd.oracle import reference as R
    from gadmm_amd.parallel import topology as T
    cohs, seeds = (1, 10, 50), (98, 99, 100)
    res = _sweep(model24, lin_obj0, chain24, cohs, seeds)
    for j, (r, c, s) in enumerate(zip(res, cohs, seeds)):
        _equal(r, _seq(lin24, lin_obj0, chain24, c, s))
        sx = r.extra["sweep"]
        assert (sx["width"], sx["slot"]) == (3, j) and sx["placed"] in (1, 2) and sx["launches"] >= 1
        assert sx["kernel"].startswith("blocked-dyn-sweep(K=3,") and r.extra["sweep_kernel"] == sx["kernel"]
        assert r.converged and 0 < r.wall_s < 5.0
    X, y = lin24.numpy()
    sched_rng = np.random.default_rng(99)
    seq = {}

    def rechain(it):
        if it not in seq:
            p, c, _, _, _ = T.find_path2(24, sched_rng)
            seq[it] = (p, c)
        return seq[it]

    o = R.dgadmm_linear(X, y, RHO, CAP, lin_obj0, TOL, chain24[0], chain24[1], 10, rechain)
    assert res[1].iters == o.iters
    assert np.allclose(res[1].obj, o.obj, rtol=1e-10)
    assert np.allclose(res[1].com_cost, o.com_cost, rtol=1e-12)
    _close(res)


@pytest.mark.parametrize("chunk", [4, 16])
def test_continuation_members_leave_in_different_rounds(lin24, lin_obj0, chain24, model24, chunk):
    """Small first chunks: members need different numbers of launches (continuations with the same tag
    salt, possibly in another slot and on another XCD) and leave in different rounds."""
    cohs, seeds = (1, 3, 10), (11, 12, 13)
    res = _sweep(model24, lin_obj0, chain24, cohs, seeds, engine_opts={"cache": False, "epoch_chunk": chunk})
    for r, c, s in zip(res, cohs, seeds):
        _equal(r, _seq(lin24, lin_obj0, chain24, c, s, chunk=chunk))
    launches = [r.extra["sweep"]["launches"] for r in res]
    assert len(set(launches)) > 1 and launches[0] > 1, launches
    assert launches[0] == max(launches)
    # the member of most launches took part in every round: its own time is the longest
    assert res[0].wall_s == max(r.wall_s for r in res)
    _close(res)


def test_width_eight(lin24, lin_obj0, chain24, model24):
    seeds = tuple(range(40, 48))
    res = _sweep(model24, lin_obj0, chain24, (10,) * 8, seeds)
    for j, (r, s) in enumerate(zip(res, seeds)):
        _equal(r, _seq(lin24, lin_obj0, chain24, 10, s))
        assert r.extra["sweep"]["width"] == 8 and r.extra["sweep"]["slot"] == j and r.extra["sweep"]["placed"] in (1, 2)
    for i in range(8):
        for j in range(i + 1, 8):
            assert not (res[i].iters == res[j].iters and np.array_equal(res[i].obj, res[j].obj)), (i, j)
    _close(res)


@pytest.mark.parametrize("d,m", [(3, 7), (14, 25), (34, 36), (50, 25)])
def test_smallest_shapes_mixed_block_counts(d, m):
    """Members of 2, 3, 5 and 24 workers with their own data in one launch, both register classes,
    coherence 3: slots with different workgroup counts (a block past its slot's count leaves before
    any barrier, staging or placement check) and idle decision waves. Each member == the
    epoch-by-epoch graph engine and == the single-solve dynamic blocked kernel on the same data."""
    from gadmm_amd.algorithms import dynamic_group_admm
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.engine.dyn_sweep import DynSweepEngine
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.parallel import topology as T
    from gadmm_amd.parallel.topology import PathSchedule, Placement
    ns = (2, 3, 5, 24)
    members, scheds, refs, blocks = [], [], [], []
    for n in ns:
        g = torch.Generator().manual_seed(1000 * d + n)
        X = torch.randn(n, m, d, dtype=torch.float64, generator=g)
        th = torch.randn(d, dtype=torch.float64, generator=g)
        y = X @ th + 0.1 * torch.randn(n, m, dtype=torch.float64, generator=g)
        Xf, yf = X.reshape(n * m, d).numpy(), y.reshape(n * m).numpy()
        sol = np.linalg.lstsq(Xf, yf, rcond=None)[0]
        obj0 = 0.5 * float(np.sum((Xf @ sol - yf) ** 2))
        model = LinearRegression(X.to(DEV), y.to(DEV))
        p0, c0, _ = T.find_path(n, np.random.default_rng(5))
        ref = []
        for opts in ({"cache": False}, {"cache": False, "persistent": False}):
            r = dynamic_group_admm(model, 1.0, obj0, 1e-6, 300, p0, c0, 3, seed=99, engine_opts=opts)
            ref.append((r.extra["engine"], int(r.iters), bool(r.converged), np.array(r.obj)))
            r.extra["engine_obj"].close()
        assert [x[0] for x in ref] == ["persistent-dynamic", "epochs"]
        refs.append(ref)
        eng = NativeChainEngine(model.X, model.y, list(range(n)), n, "linear", rho=1.0, obj0=obj0, tol=1e-6,
                                max_iter=300, precomputed=(model.A, model.b, model.yy))
        sc = PathSchedule(n, p0, c0, 3, kind="findPath2", seed=99)
        eng.set_path(sc.path, Placement.contiguous(n, 1), 0)
        members.append(eng)
        scheds.append(sc)
        k, L, W, pw = eng.blocked_plan()
        blocks.append(W + (n + 11) // 12 + 1)
    assert len(set(blocks)) > 1, blocks
    sw = DynSweepEngine(members)
    runs = sw.run(scheds)
    assert sw.last_kernel.startswith("blocked-dyn-sweep(K=4,")
    for n, r, mem, ref in zip(ns, runs, members, refs):
        print("d=%d m=%d n=%d: sweep (%d, %d, launches %d) blocked %s graph %s" % (
            d, m, n, r.done, r.iters, r.rounds, ref[0][1:3], ref[1][1:3]))
        for _, iters, conv, obj in ref:
            assert (r.iters, r.converged) == (iters, conv)
            assert np.array_equal(mem.traces(r.iters)[0], obj)
            assert np.array_equal(mem.objective_trace(r.iters), obj)
    assert all(p in (1, 2) for p in sw.last_placed), sw.last_placed
    sw.close()


def test_static_member_runs_as_a_one_epoch_slot(lin24, lin_obj0, model24):
    """A member that never re-chains within max_iter (E5's coherence 1e9) next to one that does: it
    gives what dynamic_group_admm gives for it (there: the static blocked kernel) and what chain_admm
    gives on the same chain, bit for bit, so it needs no launch of its own."""
    from gadmm_amd.algorithms import chain_admm, dynamic_group_admm
    from gadmm_amd.models import LinearRegression
    ident = (list(range(24)), np.arange(23, dtype=np.float64) + 0.5)
    cohs, seeds = (CAP + 1, 10), (5, 6)
    res = _sweep(model24, lin_obj0, ident, cohs, seeds)
    m = LinearRegression(lin24.X.to(DEV), lin24.y.to(DEV))
    a = dynamic_group_admm(m, RHO, lin_obj0, TOL, CAP, ident[0], ident[1], cohs[0], seed=5, engine_opts={"cache": False})
    b = chain_admm(m, list(range(24)), 24, RHO, lin_obj0, TOL, CAP, engine_opts={"cache": False})
    assert a.extra["engine"] == "persistent" and b.extra["engine"] == "persistent"
    r = res[0]
    print("static member: sweep %d, dynamic_group_admm %d, chain_admm %d iterations" % (r.iters, a.iters, b.iters))
    assert r.iters == a.iters == b.iters and r.converged and a.converged
    assert np.array_equal(r.obj, a.obj) and np.array_equal(r.obj, b.obj)
    assert np.array_equal(r.com_cost, a.com_cost) and np.array_equal(r.comm_units, a.comm_units)
    assert np.array_equal(r.primal_res, a.primal_res)
    assert r.extra["sweep"]["launches"] == 1
    _equal(res[1], _seq(lin24, lin_obj0, ident, 10, 6))
    _close(res)
    a.extra["engine_obj"].close()
    b.extra["engine_obj"].close()


def test_one_member_stops_at_its_cap(lin24, lin_obj0, chain24, model24):
    from gadmm_amd.engine.dyn_sweep import DynSweepRun  # noqa: F401  (the engine's record type exists)
    cohs, seeds, caps = (10, 10, 50), (21, 22, 23), (40, CAP, CAP)
    res = _sweep(model24, lin_obj0, chain24, cohs, seeds, max_iters=caps)
    assert res[0].iters == 40 and not res[0].converged
    for r, c, s, mi in zip(res, cohs, seeds, caps):
        _equal(r, _seq(lin24, lin_obj0, chain24, c, s, max_iter=mi))
    assert res[1].converged and res[2].converged
    _close(res)


def test_placement_fast_path_is_speed_only(lin24, lin_obj0, chain24, model24, monkeypatch):
    cohs, seeds = (1, 10, 50), (98, 99, 100)
    got = {}
    for x in ("1", "2"):
        monkeypatch.setenv("GADMM_XCD", x)
        res = _sweep(model24, lin_obj0, chain24, cohs, seeds)
        got[x] = res
        assert [r.extra["sweep"]["placed"] for r in res] == [int(x)] * 3
    for a, b, c, s in zip(got["1"], got["2"], cohs, seeds):
        assert a.iters == b.iters and np.array_equal(a.obj, b.obj) and np.array_equal(a.primal_res, b.primal_res)
        _equal(a, _seq(lin24, lin_obj0, chain24, c, s))
    _close(got["1"] + got["2"])


def test_residency_fallback(lin24, lin_obj0, chain24, model24, monkeypatch):
    """A CU budget below the group's workgroups: the launcher refuses before launching and the function
    returns the sequential loop's results, with the reason recorded."""
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    cohs, seeds = (1, 10, 50), (98, 99, 100)
    refs = [_seq(lin24, lin_obj0, chain24, c, s) for c, s in zip(cohs, seeds)]
    eng = NativeChainEngine(model24.X, model24.y, list(range(24)), 24, "linear", rho=RHO, max_iter=10)
    eng.set_path(list(range(24)), Placement.contiguous(24, 1), 0)
    k, L, W, pw = eng.blocked_plan()
    eng.close()
    monkeypatch.setenv("GADMM_CU_BUDGET", str(3 * (W + 2 + 1) - 1))
    res = _sweep(model24, lin_obj0, chain24, cohs, seeds)
    for r, ref in zip(res, refs):
        print(r.algorithm, r.iters, r.extra["sweep_fallback"])
        assert r.extra["sweep_fallback"] and "sweep" not in r.extra
        assert (r.iters, r.converged) == ref[:2]
        assert np.array_equal(r.obj, ref[2]) and np.array_equal(r.com_cost, ref[3])
    _close(res)


def test_repeat_and_refresh(lin24, lin_obj0, chain24, model24):
    """The cached sweep engine run twice (fresh tag salts and placement tags, the launch-size hint of
    the first run), then once more after a refresh of the shards (one Gram, one table of inverses and
    one padded image for all members, rebuilt in place): the same results every time."""
    cohs, seeds = (1, 10, 50), (98, 99, 100)
    runs = [_sweep(model24, lin_obj0, chain24, cohs, seeds, engine_opts={"refresh": rep == 2}) for rep in range(3)]
    assert len(model24._chain_engines) == 1
    sw = next(iter(model24._chain_engines.values()))
    pads = {m._minv_pad.data_ptr() for m in sw.members}
    assert len(pads) == 1 and len({m.Minv.data_ptr() for m in sw.members}) == 1  # shared, not copied
    for res in runs:
        assert all(r.extra["engine_obj"] is m for r, m in zip(res, sw.members))
        for r, c, s in zip(res, cohs, seeds):
            _equal(r, _seq(lin24, lin_obj0, chain24, c, s))
    sw.close()


def _entry_summary(tmp_path, name, extra):
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_gadmm_vs_admm", "--quick", "--no-plot",
           "--out", out] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.load(open(os.path.join(out, "summary.json")))["runs"]


def test_entry_concurrent_switch(tmp_path, monkeypatch):
    monkeypatch.delenv("GADMM_BLOCKED_DYN")  # the entry's own defaults on both sides
    seq = _entry_summary(tmp_path, "seq", [])
    con = _entry_summary(tmp_path, "con", ["--set", "sweep=concurrent"])
    keys = [k for k in seq if k.startswith("D-GADMM(coh=")]
    assert len(keys) >= 2 and [k for k in con if k.startswith("D-GADMM(coh=")] == keys
    for j, k in enumerate(keys):
        print(k, seq[k]["iters"], con[k]["iters"], seq[k]["final_loss"], con[k]["final_loss"], con[k].get("sweep_kernel"))
        assert con[k]["iters"] == seq[k]["iters"] and con[k]["converged"] == seq[k]["converged"]
        assert con[k]["final_loss"] == seq[k]["final_loss"]
        assert "blocked-dyn-sweep" in con[k]["sweep_kernel"] and con[k]["sweep_slot"] == j
        assert con[k]["sweep_launches"] >= 1
        assert "sweep_kernel" not in seq[k]
    for k in seq:  # the other runs of the entry do not change
        if k not in keys:
            assert con[k]["iters"] == seq[k]["iters"]
