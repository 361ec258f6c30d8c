"""GGADMM on the persistent graph kernel (csrc/kernels/graph_persistent.hip) on the MI355X.

The kernel is held to the long-double EDGE-DUAL reference of tests/hp_ggadmm.py (theta, the per-worker
duals, the objective trace and the tails' K4 rows, err / bound <= 1 with ``hp_reference.bound``), to the
torch path on the device (same stop iteration, traces at rtol 1e-11: the tolerance tests/test_gpu_sweep.py
and test_gpu_qgadmm.py use for closed-form solves), and on a chain graph to ``chain_admm`` on the
per-worker persistent chain kernel.

Shapes ``(graph, d)``, the smallest at which each thing can break (hp_ggadmm.CASES):

    one edge, N = 2, d = 1 and 50      the smallest graph (every worker has degree 1)
    ring_graph(4), d = 7               no degree-1 worker
    grid_graph(2, 3), d = 50           degrees 2 and 3 (the deg <= 4 kernel class)
    complete_bipartite_graph(2, 3), 52 the top of the 13-column register class
    complete_bipartite_graph(4, 4), 53 the first d of the 16-column register class
    star_graph(8, 0), d = 64           full lanes, degree 7 (the deg <= 8 class)
    star of 12, hub 5, d = 50          degree 11, past any 8-wide unroll (the deg <= 16 class); the hub
                                       is not worker 0; the heads are chosen explicitly as the leaves
    grid_graph(4, 6), d = 50           the workload's own shape
    star_graph(40, 0), d = 7           degree 39: past the 32 granules one poll group holds, the hub goes
                                       through its neighbours in two groups: the one size at which the
                                       kernel takes another path

No test provokes a timeout, a fault or a hang: the deadline path is read, not exercised.

Run with: pytest -m gpu tests/test_gpu_ggadmm.py -s
"""
import json

import numpy as np
import pytest
import torch

import hp_ggadmm as G
import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
K = H.K_ITERS
PINNED_1E4 = {"chain": 784, "ring": 246, "grid:4x6": 106, "star:0": 91, "kbip": 156}  # N = 24, rho = 3, tol 1e-4
CHAIN_1E8 = {(8, 3.0): 93, (24, 3.0): 1373, (24, 5.0): 758, (24, 7.0): 428}             # the reference's GADMM counts


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
    """Print err / bound of every quantity, then assert all of them <= 1 (as test_gpu_dispatch_classes.py)."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


_MODELS = {}


def _model(name):
    """The case's model on the device, built once and shared (its engines are cached on it)."""
    if name not in _MODELS:
        from gadmm_amd.models import LinearRegression
        g, X, y, rho = G.case_data(name)
        m = LinearRegression(_dev(X), _dev(y))
        _MODELS[name] = (g, m, rho, m.optimum())
    return _MODELS[name]


def _e1(n):
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.oracle.reference import opt_linear
    key = ("e1", n)
    if key not in _MODELS:
        ds = linear_synthetic(n)
        Xf, yf = ds.stacked()
        _MODELS[key] = (LinearRegression(ds.X.to(DEV), ds.y.to(DEV)), opt_linear(Xf.numpy(), yf.numpy()))
    return _MODELS[key]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_native_against_long_double_reference(name):
    """K iterations (the cap's stop decision reaches the workers ``lag`` iterations late: the kernel
    stops after iteration ctl.iter - 1 = last, and theta / mu are compared with the reference run that
    far; the objective trace and the K4 rows cover iterations 1..K)."""
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, X, y, rho = G.case_data(name)
    eng = NativeGraphEngine(_dev(X), _dev(y), g, rho, 0.0, 0.0, K)
    assert eng.eligible(), eng.refusal()
    r = eng.run()
    last = eng.ctl_state()["iter"] - 1
    assert r.done == 2 and r.iters == K and K <= last <= K + G.OVERRUN, (r.iters, r.done, last)
    bound_k = min([k for k in (2, 4, 8, 16, 32) if k >= g.max_degree] or [32 * ((g.max_degree + 31) // 32)])
    assert eng.last_kernel == "persistent-graph(deg<=%d)" % bound_k, eng.last_kernel
    ref = G.case(name, last)[4]
    th, mu = _host(eng.theta), _host(eng.mu)
    tr, _ = eng.traces(K)
    rows = _host(eng.rres[:K])
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(tr))
    tails = ref.tails[:K]
    assert np.all(rows[~tails] == 0.0), "a head's K4 row is not 0"
    assert np.all(np.isfinite(rows[tails])) and np.all(rows[tails] > 0)
    _report("ggadmm native %s (last=%d, %s)" % (name, last, eng.last_kernel), {
        "theta": ref.err_theta(th, last) / ref.b_theta, "dual": ref.err_dual(mu) / ref.b_dual,
        "objective": ref.err_obj(tr) / ref.b_obj, "residual rows": ref.err_res_w(rows) / ref.b_res_w})
    eng.close()


@pytest.mark.parametrize("name", list(G.CASES))
def test_native_against_torch_path_on_device(name):
    """To the 1e-8 stop: the same iteration count, the objective trace at rtol 1e-11, the residual trace
    within what thetas that close allow (derived below)."""
    from gadmm_amd.algorithms import graph_admm
    g, m, rho, obj0 = _model(name)
    a = graph_admm(m, g, rho, obj0, 1e-8, 3000, backend="native")
    b = graph_admm(m, g, rho, obj0, 1e-8, 3000, backend="torch")
    print("%s: native %d iterations (%s, placed %d), torch %d" % (name, a.iters, a.extra["kernel"], a.extra["placed"],
                                                                  b.iters))
    assert a.extra["backend"] == "native" and a.extra["engine"] == "persistent" and "state" not in a.extra
    assert b.extra["backend"] == "torch" and "graph_fallback" not in b.extra
    assert a.converged and b.converged and a.iters == b.iters
    assert np.allclose(a.obj, b.obj, rtol=1e-11, atol=0)
    assert np.array_equal(a.comm_units, b.comm_units) and a.extra["deliveries"] == b.extra["deliveries"] \
        == a.iters * 2 * len(g.edges)
    assert a.extra["graph"] == b.extra["graph"] == g.describe()
    # The residual sums squares of DIFFERENCES of thetas, so a relative tolerance on it means nothing once
    # the workers agree (it falls to 1e-19 here while theta stays O(1)). Two theta tables that agree to
    # eta * S per coordinate (eta = 1e-11, the tolerance of the traces above; S = max |theta|) have
    # differences within 2 eta S of each other, hence residuals r, r' over C = |E| d squared terms with
    # |r - r'| <= 4 eta S sqrt(C r) + 4 eta^2 S^2 C (Cauchy-Schwarz on sum 2 |Delta| |delta| + delta^2).
    S = float(b.extra["state"][0].abs().max())
    C = len(g.edges) * m.d
    slack = 4e-11 * S * np.sqrt(C * b.primal_res) + 4e-22 * S * S * C
    assert np.all(np.abs(a.primal_res - b.primal_res) <= slack)


@pytest.mark.parametrize("n,rho", [(8, 3.0), (8, 5.0), (8, 7.0), (24, 3.0), (24, 5.0), (24, 7.0)])
def test_chain_graph_against_chain_admm(n, rho, monkeypatch):
    """The chain graph on the new kernel against ``chain_admm`` on the per-worker persistent chain kernel."""
    from gadmm_amd.algorithms import chain_admm, graph_admm
    from gadmm_amd.parallel.topology import chain_graph
    monkeypatch.setenv("GADMM_BLOCKED", "0")
    m, obj0 = _e1(n)
    c = chain_admm(m, list(range(n)), n, rho, obj0, 1e-8, 3000)
    a = graph_admm(m, chain_graph(n), rho, obj0, 1e-8, 3000, backend="native")
    assert c.extra["backend"] == "native" and c.extra["engine"] == "persistent", c.extra
    assert a.extra["kernel"] == "persistent-graph(deg<=2)"
    print("chain N=%d rho=%g: %d iterations, trace bit-identical to the chain kernel: %s" % (
        n, rho, a.iters, np.array_equal(a.obj, c.obj)))
    assert a.converged and a.iters == c.iters
    if (n, rho) in CHAIN_1E8:
        assert a.iters == CHAIN_1E8[(n, rho)]
    assert np.allclose(a.obj, c.obj, rtol=1e-11, atol=0)


def test_xcd_packing_on_and_off():
    """``xcd=2`` (verified placement, plain L2-resident stores) against ``xcd=0``: bit for bit."""
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, m, rho, obj0 = _model("grid4x6-d50")
    out = []
    for xcd in (2, 0):
        eng = NativeGraphEngine(m.X, m.y, g, rho, obj0, 1e-8, 3000, precomputed=(m.A, m.b, m.yy), xcd=xcd)
        r = eng.run()
        assert r.done == 1 and eng.last_placed == xcd, (r.done, eng.last_placed)
        out.append((r.iters, eng.traces(r.iters)[0], _host(eng.theta), _host(eng.mu), _host(eng.rres[:r.iters])))
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(x, y)


def test_second_solve_on_cached_engine():
    """A second solve after ``reset()`` equals the first bit for bit: tags are salted per launch, the
    granule tables are never re-zeroed."""
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, m, rho, obj0 = _model("star12hub5-d50")
    eng = NativeGraphEngine(m.X, m.y, g, rho, obj0, 1e-8, 3000, precomputed=(m.A, m.b, m.yy))
    runs = []
    for _ in range(2):
        eng.reset()
        r = eng.run()
        runs.append((r.iters, r.done, eng.traces(r.iters)[0], _host(eng.theta), _host(eng.mu)))
    assert runs[0][:2] == runs[1][:2] and runs[0][1] == 1
    for x, y in zip(runs[0][2:], runs[1][2:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("spec", list(PINNED_1E4))
def test_pinned_iteration_counts(spec):
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.parallel.topology import parse_graph
    m, obj0 = _e1(24)
    r = graph_admm(m, parse_graph(spec, 24), 3.0, obj0, 1e-4, 3000)
    print("%s: %d iterations on %s, placed %d" % (spec, r.iters, r.extra["kernel"], r.extra["placed"]))
    assert r.extra["backend"] == "native" and "graph_fallback" not in r.extra
    assert r.converged and r.iters == PINNED_1E4[spec]


def test_dispatch_d70_takes_the_torch_path():
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.parallel.topology import ring_graph
    X, y, rho = H.make_linear(4, 80, 70, 11)
    m = LinearRegression(_dev(X), _dev(y))
    r = graph_admm(m, ring_graph(4), rho, 0.0, 0.0, 3)
    assert r.extra["backend"] == "torch" and r.extra["graph_fallback"] == "d > 64"
    with pytest.raises(RuntimeError):
        graph_admm(m, ring_graph(4), rho, 0.0, 0.0, 3, backend="native")


def test_dispatch_cu_budget_takes_the_torch_path(monkeypatch):
    """Two CUs hold at most one one-wave workgroup per SIMD, eight in all, not the 25 of the 4 x 6 grid:
    the refusal comes before any launch, the solve runs on the torch path and computes the same trace."""
    from gadmm_amd.algorithms import graph_admm
    g, m, rho, obj0 = _model("grid4x6-d50")
    a = graph_admm(m, g, rho, obj0, 1e-8, 3000, engine_opts={"cache": False})
    monkeypatch.setenv("GADMM_CU_BUDGET", "2")
    b = graph_admm(m, g, rho, obj0, 1e-8, 3000, engine_opts={"cache": False})
    assert a.extra["backend"] == "native"
    assert b.extra["backend"] == "torch" and b.extra["graph_fallback"].startswith("ResidencyError"), b.extra
    assert a.iters == b.iters and np.allclose(a.obj, b.obj, rtol=1e-11, atol=0)
    with pytest.raises(RuntimeError):
        graph_admm(m, g, rho, obj0, 1e-8, 3000, backend="native", engine_opts={"cache": False})


def test_entry_on_the_gpu(tmp_path):
    from gadmm_amd.entry import LinearRegression_Topologies as E
    out = E.main(["--device", "cuda", "--out", str(tmp_path), "--no-plot"])
    runs = out["runs"]
    assert sorted(runs) == sorted("GGADMM_%s_rho3" % s for s in PINNED_1E4)
    for spec, iters in PINNED_1E4.items():
        s = runs["GGADMM_%s_rho3" % spec]
        assert s["iters"] == iters and s["converged"] and s["engine"] == "persistent"
        assert s["kernel"].startswith("persistent-graph") and s["graph_name"] == spec
    with open(out["summary_path"]) as f:
        assert "persistent-graph" in json.dumps(json.load(f))
