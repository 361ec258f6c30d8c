"""The stop protocol every persistent engine shares (csrc/include/persist_device.h: monitor_loop,
csrc/include/stop_rule.h: stop_code) on every engine that uses it, at both ordinary stops.

Each engine solves a tiny problem (m = 8, d = 6) on a chain of n = 4 (both chain ends, one interior
head, one interior tail) and of n = 66 (the monitor's lane loop ``w = lane; w < n; w += 64`` takes a
second trip, the only shape edge the monitor has; the blocked kernel also runs its smallest chain,
n = 2), once to max_iter = 3 with tol = 0 (code 2) and once to a loose tolerance (code 1), and must
report the iteration count, the stop code and the objective trace of its reference:

  per-worker (register and LDS variant), blocked, Q persistent, logistic one-wave: the graph engine
      (Q: its quantized phase kernel), bit for bit -- the pairs the project states to be bit-identical;
  logistic margins recursion: the graph engine, trace to rtol 1e-12
      (test_gpu.py::test_logistic_persistent_kernel_matches_graph_engine);
  Newton one-wave and pipeline: the torch path, trace to rtol 1e-12
      (test_gpu.py::test_newton_persistent_variants_match_torch);
  star: the long-double reference within its float64 noise bound
      (test_gpu_dispatch_classes.py::test_star_persistent_kernel).

The loose tolerance is built so that no engine's rounding can move the stop: the reference runs K = 10
iterations with no stop rule, obj0 is its objective of iteration STOP_AT = 8 (gap 0 there; an engine
that agrees to 1e-12 has a gap below 1e-12 |obj0|) and tol is half the smallest gap of the earlier
iterations (each at least 2 tol), required to exceed 1e-6 |obj0|. Every engine must stop at 8, code 1.
An engine that is not eligible at these shapes fails; nothing is skipped but for a missing GPU.

Run with: pytest -m gpu tests/test_gpu_stop_rule.py
"""
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
M, D = 8, 6
K, STOP_AT = 10, 8
Q_BITS, Q_SEED = 8, 1234
STOPS = ("max_iter", "tol")


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _targets(trace):
    """(obj0, tol) of the loose-tolerance stop from a reference trace of K iterations (module docstring)."""
    trace = np.asarray(trace, dtype=np.float64)
    assert len(trace) == K and np.all(np.isfinite(trace))
    obj0 = float(trace[STOP_AT - 1])
    tol = 0.5 * float(np.min(np.abs(trace[:STOP_AT - 1] - obj0)))
    assert tol > 1e-6 * abs(obj0), (tol, obj0)
    return obj0, tol


def _settings(stop, trace_fn):
    """(max_iter, obj0, tol, expected done, expected iterations) of a stop condition."""
    if stop == "max_iter":
        return 3, 0.0, 0.0, 2, 3
    obj0, tol = trace_fn()
    return K, obj0, tol, 1, STOP_AT


def _stop_of(trace, obj0, tol, max_iter):
    """The stop rule (stop_rule.h) applied to a reference trace: (code, iteration)."""
    for it, s in enumerate(np.asarray(trace, dtype=np.float64)[:max_iter], 1):
        if not np.isfinite(s):
            return 3, it
        if abs(s - obj0) < tol:
            return 1, it
        if it >= max_iter:
            return 2, it
    raise AssertionError("trace shorter than max_iter")


# ------------------------------------------------------------------------------------------------
# Chain engines (linear, Q, logistic inner GD): graph engine against one persistent launch
_CACHE = {}


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _chain_engine(family, n, max_iter, obj0, tol):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    if family == "logistic":
        X, y, rho, lam, step = _cached(("log-data", n), lambda: H.make_logistic(n, M, D, H.seed_of(n, M, D)))
        kw = dict(lam=lam, step=step, max_inner=H.MAX_INNER, inner_tol=0.0)
    else:
        X, y, rho = _cached(("lin-data", n), lambda: H.make_linear(n, M, D, H.seed_of(n, M, D)))
        kw = dict(quant=(Q_BITS, Q_SEED)) if family == "quant" else {}
    eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "logistic" if family == "logistic" else "linear",
                            rho=rho, obj0=obj0, tol=tol, max_iter=max_iter, **kw)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def _graph_run(family, n, max_iter, obj0, tol):
    """(done, iterations, trace) of the graph engine, once per setting, read-only."""
    def build():
        eng = _chain_engine(family, n, max_iter, obj0, tol)
        r = eng.run()
        assert eng.graph_ok()
        tr = eng.objective_trace(r.iters).copy()
        tr.setflags(write=False)
        eng.close()
        return int(r.done), int(r.iters), tr
    return _cached(("graph", family, n, max_iter, obj0, tol), build)


def _graph_free_trace(family, n):
    done, iters, tr = _graph_run(family, n, K, 0.0, 0.0)
    assert (done, iters) == (2, K)
    return tr


# engine -> (data / graph family, environment, prefix of last_kernel, bit-identical to the graph engine)
CHAIN_ENGINES = {
    "per-worker": ("linear", {"GADMM_BLOCKED": "0"}, "per-worker", True),
    "blocked": ("linear", {}, "blocked(", True),
    "quant": ("quant", {}, "persistent-Q", True),
    "logistic-one-wave": ("logistic", {"GADMM_LOGISTIC_ZREC": "0"}, "per-worker-logistic", True),
    "logistic-zrec": ("logistic", {"GADMM_LOGISTIC_ZREC": "1"}, "per-worker-logistic", False),
}


def check_chain_engine(engine, n, stop):
    """One persistent launch of ``engine`` against the graph engine (the caller has set the environment)."""
    family, _, kernel, identical = CHAIN_ENGINES[engine]
    max_iter, obj0, tol, done, iters = _settings(stop, lambda: _targets(_graph_free_trace(family, n)))
    g_done, g_iters, g_tr = _graph_run(family, n, max_iter, obj0, tol)
    assert (g_done, g_iters) == (done, iters), (g_done, g_iters)
    eng = _chain_engine(family, n, max_iter, obj0, tol)
    if family == "quant":
        assert eng.persistent_q_eligible()
    else:
        assert eng.persistent_eligible()
        if family == "linear":
            assert (eng.blocked_plan() is not None) == (engine == "blocked")
    r = eng.run_persistent()
    assert eng.last_kernel.startswith(kernel), eng.last_kernel
    tr = eng.objective_trace(r.iters)
    print("%s n=%d %s: done %d, iterations %d, max |trace - graph| %.3g" % (
        engine, n, stop, r.done, r.iters, float(np.max(np.abs(tr - g_tr[:len(tr)]))) if len(tr) else -1.0))
    assert (int(r.done), int(r.iters)) == (done, iters), (r.done, r.iters)
    if identical:
        assert np.array_equal(tr, g_tr)
    else:
        np.testing.assert_allclose(tr, g_tr, rtol=1e-12, atol=0)
    eng.close()


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("engine,n", [(e, n) for e in CHAIN_ENGINES for n in ((2, 66) if e == "blocked" else (4, 66))])
def test_chain_engines_stop_like_the_graph_engine(engine, n, stop, monkeypatch):
    for k in ("GADMM_BLOCKED", "GADMM_BLOCK_PW", "GADMM_BLOCK_K", "GADMM_BLOCK_L"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CHAIN_ENGINES[engine][1].items():
        monkeypatch.setenv(k, v)
    check_chain_engine(engine, n, stop)


def child_main():
    """Runs in the fresh child process of test_per_worker_lds_variant_stops_like_the_graph_engine."""
    from gadmm_amd.ops import native
    assert os.environ.get("GADMM_PERSIST_LDS") and os.environ.get("GADMM_BLOCKED") == "0"
    for n in (4, 66):
        for stop in STOPS:
            native.poison_lds()
            check_chain_engine("per-worker", n, stop)
    print("LDS-VARIANT-OK", flush=True)


def test_per_worker_lds_variant_stops_like_the_graph_engine():
    """GADMM_PERSIST_LDS is read once per process (a static in pick_variant, chain_persistent.hip): the
    four-wave LDS variant of the per-worker kernel runs in a fresh child, every case in that one process."""
    env = dict(os.environ, GADMM_PERSIST_LDS="1", GADMM_BLOCKED="0",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_stop_rule as t; t.child_main()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "LDS-VARIANT-OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------
# Newton (exact local solves): both persistent kernels against the torch path
def _newton_run(n, max_iter, obj0, tol, backend, opts=None):
    from gadmm_amd.algorithms.gadmm import group_admm_logistic_exact
    from gadmm_amd.models import LogisticRegression
    X, y, rho, lam, _ = _cached(("log-data", n), lambda: H.make_logistic(n, M, D, H.seed_of(n, M, D)))
    model = LogisticRegression(_dev(X), _dev(y), lam=lam)
    return group_admm_logistic_exact(model, rho, obj0, tol, max_iter, backend=backend, engine_opts=opts)


def _newton_torch(n, max_iter, obj0, tol):
    def build():
        r = _newton_run(n, max_iter, obj0, tol, "torch")
        return (1 if r.converged else 2), int(r.iters), np.asarray(r.obj, dtype=np.float64)
    return _cached(("newton-torch", n, max_iter, obj0, tol), build)


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("n", [4, 66])
@pytest.mark.parametrize("rec,kernel", [("0", "per-worker-newton(one-wave)"), ("1", "per-worker-newton(pipeline)")])
def test_newton_kernels_stop_like_torch(rec, kernel, n, stop, monkeypatch):
    monkeypatch.setenv("GADMM_NEWTON_REC", rec)
    max_iter, obj0, tol, done, iters = _settings(stop, lambda: _targets(_newton_torch(n, K, 0.0, 0.0)[2]))
    t_done, t_iters, t_obj = _newton_torch(n, max_iter, obj0, tol)
    assert (t_done, t_iters) == (done, iters), (t_done, t_iters)
    a = _newton_run(n, max_iter, obj0, tol, "auto", {"cache": False, "persistent": True})
    assert a.extra["engine"] == "persistent", a.extra["engine"]
    assert a.extra["engine_obj"].last_kernel == kernel, a.extra["engine_obj"].last_kernel
    print("newton rec=%s n=%d %s: converged %s, iterations %d" % (rec, n, stop, a.converged, a.iters))
    assert ((1 if a.converged else 2), int(a.iters)) == (done, iters), (a.converged, a.iters)
    np.testing.assert_allclose(a.obj, t_obj[:iters], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------
# Star ADMM against the long-double reference
@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("n", [4, 66])
def test_star_kernel_stops_like_the_reference(n, stop):
    from gadmm_amd.engine.star_engine import StarEngine
    X, y, rho, ref = H.star_case(n, M, D, K)
    ref_obj = np.asarray(ref.obj, dtype=np.float64)
    max_iter, obj0, tol, done, iters = _settings(stop, lambda: _targets(ref_obj))
    assert _stop_of(ref_obj, obj0, tol, max_iter) == (done, iters)
    eng = StarEngine(_dev(X), _dev(y), list(range(n)), n, rho, obj0, tol, max_iter)
    assert eng.eligible() and eng.last_kernel == "star-persistent"
    it, dn, _ = eng.run()
    tr = eng.objective_trace(it)
    ratio = ref.err_obj(tr) / ref.b_obj
    print("star n=%d %s: done %d, iterations %d, objective err/bound %.3f" % (n, stop, dn, it, ratio))
    assert (int(dn), int(it)) == (done, iters), (dn, it)
    assert ratio <= 1.0, ratio
    eng.close()


# ------------------------------------------------------------------------------------------------
# Code 3: a NaN objective stops the solve at iteration 1 with done = 3, returned (ChainCtl::done; the
# engine raises for a hand-off timeout, done = 4, only)
@pytest.mark.parametrize("persistent", [False, True])
def test_nan_objective_is_code_3_at_iteration_1(persistent, monkeypatch):
    monkeypatch.setenv("GADMM_BLOCKED", "0")
    eng = _chain_engine("linear", 4, K, 0.0, 0.0)
    with torch.cuda.stream(eng.stream):
        eng.b[1, 0] = float("nan")
    eng.stream.synchronize()
    if persistent:
        r = eng.run_persistent()
        assert eng.last_kernel == "per-worker", eng.last_kernel
    else:
        r = eng.run()
    assert (int(r.done), int(r.iters)) == (3, 1), (r.done, r.iters)
    assert np.isnan(eng.objective_trace(1)[0])
    eng.close()
