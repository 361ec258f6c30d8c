"""Stop timing of the temporally blocked chain kernel (csrc/kernels/chain_blocked.hip) at small and odd
shapes: the kernel learns the monitor's decision in the head phase and acts on flags that every wave
read one phase before the closing barrier, so what can go wrong is a stop that lands one iteration or
one phase off, or a stale flag. Every case compares with the graph engine (or the epoch-by-epoch
D-GADMM path) bit for bit.

The blocked kernel runs with an effective decision lag of 8 (run_persistent raises lag to 8 for it): a
decision for iteration j ends the kernel after iteration j + 7, so its state is compared with the graph
engine run to exactly that iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RHO = 3.0
LAG = 8  # effective decision lag of the blocked kernel
TARGETS = (1, 2, 3, 7, 8, 9, 20, 21, 33)
TRACE_LEN = max(TARGETS) + LAG
FAR = -1.0  # the objective is a sum of squares: a gap to -1 is never below a tolerance


@pytest.fixture(autouse=True)
def _poison_lds():
    """NaN-filled LDS on every CU before each case (csrc/kernels/debug_poison.hip): a flag or theta
    slot read before its owner wrote it shows up deterministically."""
    from gadmm_amd.ops import native
    native.poison_lds()
    yield


def _shards(n, d, seed=0):
    m = max(d, 4)
    g = torch.Generator().manual_seed(seed * 100003 + 1000 * d + n)
    X = torch.randn(n, m, d, dtype=torch.float64, generator=g)
    th = torch.randn(d, dtype=torch.float64, generator=g)
    y = X @ th + 0.1 * torch.randn(n, m, dtype=torch.float64, generator=g)
    return X.to(DEV), y.to(DEV)


def _engine(X, y, obj0, tol, max_iter=3000, rho=RHO):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    n = int(X.shape[0])
    eng = NativeChainEngine(X, y, list(range(n)), n, "linear", rho=rho, obj0=obj0, tol=tol, max_iter=max_iter)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def _state(eng):
    torch.cuda.synchronize()
    return eng.theta.clone(), eng.mu.clone()


_TRACES = {}


def _graph_trace(n, d, seed=0):
    """The graph engine's objective trace of the first TRACE_LEN iterations, once per shape."""
    key = (n, d, seed)
    if key not in _TRACES:
        X, y = _shards(n, d, seed)
        eng = _engine(X, y, FAR, 1e-30)
        r = eng.run(stop_iter=TRACE_LEN)
        assert r.iters == TRACE_LEN and eng.graph_ok()
        tr = eng.objective_trace(TRACE_LEN).copy()
        tr.setflags(write=False)
        eng.close()
        assert np.all(np.isfinite(tr))
        _TRACES[key] = tr
    return _TRACES[key]


def _target(tr, j):
    """(obj0, tol) that the stop rule first meets at iteration j: obj0 is the trace value there and tol
    half its distance to the nearest earlier value (which must differ: the target is then usable)."""
    obj0 = float(tr[j - 1])
    if j == 1:
        return obj0, 1e-12
    tol = 0.5 * float(np.min(np.abs(tr[:j - 1] - obj0)))
    assert tol > 0.0, "trace value at %d ties with an earlier one: change the seed" % j
    return obj0, tol


def _graph_state_at(eng, it):
    """(theta, mu, next iteration) of the graph engine after exactly `it` iterations."""
    eng.set_targets(FAR, 1e-30)
    eng.reset()
    r = eng.run(stop_iter=it)
    assert r.iters == it
    return _state(eng) + (int(eng.ctl_state()["iter"]),)


def _check_stop(eng, tr, j):
    obj0, tol = _target(tr, j)
    eng.set_targets(obj0, tol)
    eng.reset()
    rg = eng.run()
    cg = eng.ctl_state()
    trg = eng.objective_trace(j).copy()
    eng.reset()
    rp = eng.run_persistent(fetch_trace=True)
    assert eng.last_kernel.startswith("blocked("), eng.last_kernel
    cp = eng.ctl_state()
    trp = eng.objective_trace(j).copy()
    thp, mup = _state(eng)
    print("j=%d graph (done %d, iters %d, conv %d, next %d) blocked (done %d, iters %d, conv %d, next %d)" % (
        j, rg.done, rg.iters, cg["conv_iter"], cg["iter"], rp.done, rp.iters, cp["conv_iter"], cp["iter"]))
    assert (rg.done, rg.iters) == (1, j) and (rp.done, rp.iters) == (1, j)
    assert cg["conv_iter"] == cp["conv_iter"] == j
    assert np.array_equal(trg, tr[:j]) and np.array_equal(trp, tr[:j])
    # the kernel ran exactly the iterations up to j + lag - 1: the graph engine's state there
    assert cp["iter"] == j + LAG and cp["pending"] == 1
    thg, mug, nxt = _graph_state_at(eng, j + LAG - 1)
    assert nxt == cp["iter"]
    assert torch.equal(thp, thg) and torch.equal(mup, mug)


@pytest.mark.parametrize("d", [1, 7, 32, 33, 50, 52])
@pytest.mark.parametrize("n", [2, 3, 5, 13, 24])
def test_stop_lands_where_the_graph_engine_stops(n, d):
    """Targets of both parities, both iterations of a k = 2 block, below, at and above the lag."""
    tr = _graph_trace(n, d)
    X, y = _shards(n, d)
    eng = _engine(X, y, FAR, 1e-30)
    for j in TARGETS:
        _check_stop(eng, tr, j)
    eng.close()


@pytest.mark.parametrize("max_iter", [1, 2, 7, 8, 9, 12])
@pytest.mark.parametrize("n,d", [(5, 7), (24, 50)])
def test_max_iter_exits(n, d, max_iter):
    X, y = _shards(n, d)
    eng = _engine(X, y, FAR, 1e-30, max_iter=max_iter)
    rg = eng.run()
    cg = eng.ctl_state()
    trg = eng.objective_trace(max_iter).copy()
    eng.reset()
    rp = eng.run_persistent(fetch_trace=True)
    assert eng.last_kernel.startswith("blocked("), eng.last_kernel
    cp = eng.ctl_state()
    thp, mup = _state(eng)
    print("max_iter=%d graph (%d, %d) blocked (%d, %d) next %d" % (max_iter, rg.done, rg.iters, rp.done, rp.iters,
                                                                  cp["iter"]))
    assert (rp.done, rp.iters) == (rg.done, rg.iters) == (2, max_iter)
    assert cp["conv_iter"] == cg["conv_iter"]
    assert np.array_equal(eng.objective_trace(max_iter), trg)
    assert cp["iter"] == max_iter + LAG
    eng.close()
    ref = _engine(X, y, FAR, 1e-30)  # the graph engine without the cap, run to the kernel's last iteration
    thg, mug, nxt = _graph_state_at(ref, max_iter + LAG - 1)
    assert nxt == cp["iter"] and torch.equal(thp, thg) and torch.equal(mup, mug)
    ref.close()


@pytest.mark.parametrize("j", [8, 9, 20, 21])
@pytest.mark.parametrize("start", [2, 3])
@pytest.mark.parametrize("n,d", [(5, 7), (13, 33)])
def test_resume_equals_uninterrupted_run(n, d, start, j):
    """The kernel resumed at start_iter with the heads' duals pending == the uninterrupted launch."""
    tr = _graph_trace(n, d)
    X, y = _shards(n, d)
    obj0, tol = _target(tr, j)
    eng = _engine(X, y, obj0, tol)
    r0 = eng.run_persistent(fetch_trace=True)
    c0 = eng.ctl_state()
    th0, mu0 = _state(eng)
    assert (r0.done, r0.iters) == (1, j)
    # the state after start - 1 iterations (graph engine: the heads' duals of the last one still pending)
    eng.set_targets(FAR, 1e-30)
    eng.reset()
    assert eng.run(stop_iter=start - 1).iters == start - 1
    assert eng.ctl_state()["pending"] == 1
    eng.set_targets(obj0, tol)
    eng.reset(start_iter=start, pending=1, zero_state=False)
    r1 = eng.run_persistent(start_iter=start, pending_in=1, fetch_trace=True)
    assert eng.last_kernel.startswith("blocked("), eng.last_kernel
    c1 = eng.ctl_state()
    th1, mu1 = _state(eng)
    assert (r1.done, r1.iters) == (1, j)
    assert (c1["iter"], c1["conv_iter"], c1["pending"]) == (c0["iter"], c0["conv_iter"], c0["pending"])
    assert np.array_equal(eng.objective_trace(j)[start - 1:], tr[start - 1:j])
    assert torch.equal(th1, th0) and torch.equal(mu1, mu0)
    eng.close()


@pytest.mark.parametrize("coh", [1, 3])
@pytest.mark.parametrize("n", [3, 5])
def test_dynamic_chains_stop_around_a_rechain(n, coh, monkeypatch):
    """Blocked dynamic mode: stop targets on a re-chain iteration, the one before and the one after, in
    epoch chunks whose hard stop falls one before, on and one after the target and the iteration the
    kernel leaves at (target + lag - 1) == the epoch-by-epoch path.

    A chunk is a whole number of epochs, so a hard stop is a multiple of the coherence. With coherence 1
    every target gets all three offsets. With coherence 3 a single target gets only the multiples of 3
    among them (two of its six candidates, printed below); the three consecutive targets move each
    multiple of 3 through the offsets -1, 0 and +1, so every offset is still exercised for the shape."""
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.algorithms import dynamic_group_admm
    from gadmm_amd.parallel import topology as T
    monkeypatch.setenv("GADMM_BLOCKED_DYN", "1")
    X, y = _shards(n, 7, seed=3)
    m = LinearRegression(X, y)
    p0, c0, _ = T.find_path(n, np.random.default_rng(5))

    def run(obj0, tol, max_iter, **o):
        return dynamic_group_admm(m, 1.0, obj0, tol, max_iter, p0, c0, coh, seed=99, engine_opts=dict(cache=False, **o))

    tr = np.asarray(run(FAR, 1e-30, 30, persistent=False).obj)
    assert len(tr) == 30
    re = 1 + coh * (9 // coh)  # a re-chain iteration (epochs start at 1, 1 + coh, ...)
    for j in (re - 1, re, re + 1):
        obj0, tol = _target(tr, j)
        b = run(obj0, tol, 3000, persistent=False)
        assert b.extra["engine"] == "epochs" and b.iters == j and b.converged
        stops = sorted({h for c in (j, j + LAG - 1) for h in (c - 1, c, c + 1) if h % coh == 0 and h >= coh})
        assert stops
        for hs in stops:
            a = run(obj0, tol, 3000, epoch_chunk=hs // coh)
            assert a.extra["engine"] == "persistent-dynamic"
            assert a.extra["engine_obj"].last_kernel.startswith("blocked-dyn("), a.extra["engine_obj"].last_kernel
            print("n=%d coh=%d j=%d hard stop %d: iters %d" % (n, coh, j, hs, a.iters))
            assert a.iters == j and a.converged
            assert np.array_equal(np.asarray(a.obj), np.asarray(b.obj))
        a = run(obj0, tol, 3000, epoch_chunk=100000)  # one launch holding every epoch
        assert a.iters == j and a.converged and np.array_equal(np.asarray(a.obj), np.asarray(b.obj))


def test_sweep_members_stop_at_both_parities():
    """Several solves in one launch whose stop iterations differ in parity: each equals its solo run."""
    from gadmm_amd.engine.chain_sweep import ChainSweepEngine
    n, d = 5, 7
    tr = _graph_trace(n, d)
    X, y = _shards(n, d)
    js = (7, 8, 20, 21)
    solo = []
    for j in js:
        eng = _engine(X, y, *_target(tr, j))
        r = eng.run_persistent(fetch_trace=True)
        solo.append((r.done, r.iters, eng.ctl_state(), eng.objective_trace(j).copy()) + _state(eng))
        eng.close()
    members = [_engine(X, y, *_target(tr, j)) for j in js]
    sw = ChainSweepEngine(members)
    runs = sw.run()
    for j, r, mem, (done, iters, ctl, trs, th, mu) in zip(js, runs, members, solo):
        c = mem.ctl_state()
        print("j=%d solo (%d, %d, next %d) sweep (%d, %d, next %d)" % (j, done, iters, ctl["iter"], r.done, r.iters,
                                                                      c["iter"]))
        assert (r.done, r.iters) == (done, iters) == (1, j)
        assert (c["iter"], c["conv_iter"]) == (ctl["iter"], ctl["conv_iter"])
        assert np.array_equal(mem.objective_trace(j), trs)
        ths, mus = _state(mem)
        assert torch.equal(ths, th) and torch.equal(mus, mu)
    sw.close()


def test_xcd_packing_on_and_off(monkeypatch):
    n, d = 13, 33
    tr = _graph_trace(n, d)
    X, y = _shards(n, d)
    out = {}
    for xcd in ("0", "2"):
        monkeypatch.setenv("GADMM_XCD", xcd)
        for j in (8, 21):
            eng = _engine(X, y, *_target(tr, j))
            r = eng.run_persistent(fetch_trace=True)
            assert eng.last_kernel.startswith("blocked("), eng.last_kernel
            c = eng.ctl_state()
            assert (r.done, r.iters, c["conv_iter"], c["iter"]) == (1, j, j, j + LAG)
            out[xcd, j] = (eng.objective_trace(j).copy(),) + _state(eng)
            eng.close()
    for j in (8, 21):
        a, b = out["0", j], out["2", j]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], tr[:j])
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
