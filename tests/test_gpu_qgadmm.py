"""Q-GADMM on the GPU (csrc/kernels/chain_quant.hip): the graph engine's Q phase kernel and the
persistent Q kernel against the NumPy specification (algorithms/quantize.py), against each other bit
for bit, and against the torch path where its flip margins make the comparison meaningful.

Run with: pytest -m gpu tests/test_gpu_qgadmm.py
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
RHO = 3.0


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu_sweep.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


_PROB = {}


def _problem(N, d):
    """(X (N, 50, d), y (N, 50), obj0) cut from linear_synthetic(N) by column slicing, shared. The data
    set has 50 columns: d = 64 appends 14 seeded N(0, 1) / sqrt(50) columns."""
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


def _engine(N, d, bits, seed=1234, tol=1e-8, max_iter=200, xcd=2):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, obj0 = _problem(N, d)
    eng = NativeChainEngine(X.to(DEV), y.to(DEV), list(range(N)), N, "linear", rho=RHO, obj0=obj0, tol=tol,
                            max_iter=max_iter, quant=(bits, seed), xcd=xcd)
    eng.set_path(list(range(N)), Placement.contiguous(N, 1), 0)
    return eng


def _graph_run(eng, stop_iter=0):
    eng.reset()
    r = eng.run(stop_iter=stop_iter)
    assert eng.graph_ok()
    return r


def _model(N, d):
    from gadmm_amd.models.linear import LinearRegression
    X, y, obj0 = _problem(N, d)
    return LinearRegression(X.to(DEV), y.to(DEV)), obj0


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("N,d", [(3, 7), (8, 50), (4, 70), (3, 200)])
def test_quantizer_exactness_one_phase(N, d, bits):
    """One head phase and one tail phase of the graph-Q kernel from a random th_hat table and random
    duals: the codes, R and the new th_hat equal the NumPy specification applied to the kernel's OWN
    theta, bit for bit (the heads' and the tails' messages of iteration 1)."""
    from gadmm_amd.algorithms import quantize as Q
    eng = _engine(N, d, bits, seed=99, max_iter=8)
    rng = np.random.default_rng(1000 * N + d + bits)
    eng.reset()
    with torch.cuda.stream(eng.stream):
        eng.theta.copy_(torch.from_numpy(rng.standard_normal((N, d))))
        eng.mu.copy_(torch.from_numpy(rng.standard_normal((N, d)) * 0.1))
    table0 = eng.theta.cpu().numpy().copy()
    r = eng.run(stop_iter=1, use_graph=False)  # iteration 1: the head phase, then the tail phase
    assert r.iters == 1
    hat1 = eng.theta.cpu().numpy()
    true1 = eng.theta_true.cpu().numpy()
    msg = eng.q_msg.cpu().numpy().view(np.uint64)
    heads, tails = list(range(0, N, 2)), list(range(1, N, 2))
    for ws in (heads, tails):  # a tail quantizes against its own row, which the head phase left alone
        u = Q.u01(99, 1, N, ws, d)
        R, q, new, _ = Q.quantize_rows(true1[ws], table0[ws], bits, u)
        assert np.all(R > 0)
        assert np.array_equal(msg[ws, 0].view(np.float64), R)
        assert np.array_equal(Q.unpack_codes(msg[ws, 1:], bits, d), q)
        assert np.array_equal(msg[ws, 1:], Q.pack_codes(q, bits))
        assert np.array_equal(hat1[ws], new)
        assert not np.array_equal(hat1[ws], true1[ws])
    assert np.isfinite(eng.objective_trace(1)[0])
    eng.close()


_GRAPH = {}


def _graph_ref(N, d, bits, tol=1e-8, max_iter=200, stop_iter=0):
    """(done, iters, trace, th_hat, true theta, mu) of the graph-Q engine, computed once per key."""
    key = (N, d, bits, tol, max_iter, stop_iter)
    if key not in _GRAPH:
        eng = _engine(N, d, bits, tol=tol, max_iter=max_iter)
        r = _graph_run(eng, stop_iter=stop_iter)
        tr = eng.objective_trace(r.iters).copy()
        tr.setflags(write=False)
        _GRAPH[key] = (r.done, r.iters, tr, eng.theta.cpu(), eng.theta_true.cpu(), eng.mu.cpu())
        eng.close()
    return _GRAPH[key]


@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("d", [1, 7, 50, 64])
def test_engines_agree(N, d):
    """persistent-Q == graph-Q bit for bit, b in {4, 8, 16}, XCD packing on (placement verified) and
    off: iterations, objective trace, and th_hat / true theta / duals after the persistent kernel's
    last iteration (it learns the decision `lag` iterations late) == the graph engine run that far."""
    for bits in (4, 8, 16):
        done, iters, tr, _, _, _ = _graph_ref(N, d, bits)
        assert done in (1, 2) and iters >= 10
        for xcd in (2, 0):
            eng = _engine(N, d, bits, xcd=xcd)
            assert eng.persistent_q_eligible()
            eng.reset()
            r = eng.run_persistent(fetch_trace=True)
            print("N=%d d=%d b=%d xcd=%d: done=%d iters=%d placed=%d %s" % (N, d, bits, xcd, r.done, r.iters,
                                                                           eng.last_placed, eng.last_kernel))
            assert eng.last_kernel.startswith("persistent-Q")
            assert eng.last_placed == xcd
            assert (r.done, r.iters) == (done, iters)
            assert np.array_equal(eng.objective_trace(r.iters), tr)
            assert np.array_equal(eng.traces(r.iters)[0], tr)
            last = eng.ctl_state()["iter"] - 1
            assert iters <= last <= iters + 16
            _, it_g, tr_g, hat_g, true_g, mu_g = _graph_ref(N, d, bits, tol=0.0, stop_iter=last)
            assert it_g == last and np.array_equal(tr_g[:iters], tr)
            assert torch.equal(eng.theta.cpu(), hat_g)
            assert torch.equal(eng.theta_true.cpu(), true_g)
            # the kernel leaves the heads' last dual pending, like the graph engine before its flush
            assert torch.equal(eng.mu.cpu(), mu_g)
            eng.close()


@pytest.mark.parametrize("N,d", [(2, 50), (3, 50), (8, 50), (5, 7)])
def test_against_the_spec(N, d):
    """The first 20 iterations at b in {4, 8}, seeds 1234 and 7, against the torch path. First a
    condition on the reference alone: its smallest flip margin is >= 1e-10 (the CPU prototype gives
    >= 1.6e-10 on these cases), far above the engines' rounding differences, so no code flips and the
    traces agree at rtol 1e-11, the tolerance tests/test_gpu_sweep.py uses for the oracle. (b = 16 is
    left out: its margins are about 1e-12; tests/test_gpu_qgadmm_classes.py holds b = 16 to a long-double
    reference under a bound that is checked against the flip margin case by case.)"""
    from gadmm_amd.algorithms import quantized_group_admm
    from gadmm_amd.models.linear import LinearRegression
    X, y, obj0 = _problem(N, d)
    cpu = LinearRegression(X, y)
    gpu, _ = _model(N, d)
    for bits in (4, 8):
        for seed in (1234, 7):
            ref = quantized_group_admm(cpu, RHO, obj0, 1e-30, 20, bits, seed=seed)
            margin = ref.extra["min_flip_margin"]
            print("N=%d d=%d b=%d seed=%d: min flip margin %.3g" % (N, d, bits, seed, margin))
            assert ref.iters == 20 and margin >= 1e-10
            for persistent in (True, False):
                r = quantized_group_admm(gpu, RHO, obj0, 1e-30, 20, bits, seed=seed, backend="native",
                                         engine_opts={"persistent": persistent, "cache": False})
                assert r.extra["kernel"].startswith("persistent-Q" if persistent else "graph-Q")
                assert "quant_fallback" not in r.extra
                rel = np.max(np.abs(r.obj - ref.obj) / np.abs(ref.obj))
                print("   %s: max rel diff %.3g" % (r.extra["kernel"], rel))
                assert r.iters == 20 and np.allclose(r.obj, ref.obj, rtol=1e-11, atol=0.0)
                r.extra["engine_obj"].close()


@pytest.mark.parametrize("bits,tol,iters", [(8, 1e-8, 93), (16, 1e-8, 93), (8, 1e-4, 55)])
def test_counts(bits, tol, iters):
    """N = 8, d = 50, seed 1234: the torch path's counts on both native engines, with the accounting."""
    from gadmm_amd.algorithms import quantized_group_admm
    from gadmm_amd.algorithms.quantize import granules_per_row
    gpu, obj0 = _model(8, 50)
    G = granules_per_row(50, bits)
    assert G == -(-50 * bits // 64) + 1
    for persistent in (True, False):
        r = quantized_group_admm(gpu, RHO, obj0, tol, 500, bits, seed=1234,
                                 engine_opts={"persistent": persistent, "cache": False})
        ex = r.extra
        print("b=%d tol=%g %s: iters %d gap/tol %.4f" % (bits, tol, ex["kernel"], r.iters, r.loss[-1] / tol))
        assert ex["backend"] == "native" and ex["kernel"].startswith("persistent-Q" if persistent else "graph-Q")
        assert r.converged and r.iters == iters and len(r.obj) == iters
        assert ex["q_granules"] == G and ex["q_wire_bytes"] == iters * 8 * G * 16
        assert ex["payload_bits"] == iters * 8 * (bits * 50 + 64) and (ex["q_bits"], ex["q_seed"]) == (bits, 1234)
        assert r.comm_units[-1] == iters * 8 * (bits * 50 + 64) / (64.0 * 50)
        ex["engine_obj"].close()


def test_dispatch(monkeypatch):
    """d = 70 runs graph-Q; ``state=`` takes the torch path and says why; a CU budget below N + 1 sends
    the d <= 64 case to graph-Q with the persistent kernel's trace."""
    from gadmm_amd.algorithms import quantized_group_admm
    gpu70, obj70 = _model(4, 70)
    r = quantized_group_admm(gpu70, RHO, obj70, 1e-6, 60, 8, engine_opts={"cache": False})
    assert r.extra["backend"] == "native" and r.extra["kernel"] == "graph-Q" and r.extra["engine"] == "graph"
    assert r.iters >= 10 and np.all(np.isfinite(r.obj))
    r.extra["engine_obj"].close()

    gpu, obj0 = _model(8, 50)
    st = (torch.zeros((8, 50), dtype=torch.float64, device=DEV), torch.zeros((8, 50), dtype=torch.float64, device=DEV), 1)
    t = quantized_group_admm(gpu, RHO, obj0, 1e-4, 500, 8, state=st)
    assert t.extra["backend"] == "torch" and t.extra["quant_fallback"] == "state= (resume)"
    assert t.iters == 55 and t.extra["min_flip_margin"] > 0

    p = quantized_group_admm(gpu, RHO, obj0, 1e-4, 500, 8, engine_opts={"cache": False})
    assert p.extra["engine"] == "persistent" and p.extra["kernel"].startswith("persistent-Q") and p.iters == 55
    p.extra["engine_obj"].close()
    monkeypatch.setenv("GADMM_CU_BUDGET", "2")  # 2 CUs x (at most 4 one-wave workgroups) < N + 1 = 9
    g = quantized_group_admm(gpu, RHO, obj0, 1e-4, 500, 8, engine_opts={"cache": False})
    assert g.extra["kernel"] == "graph-Q" and g.extra["engine"].startswith("graph")
    assert g.iters == 55 and np.array_equal(g.obj, p.obj)
    g.extra["engine_obj"].close()
