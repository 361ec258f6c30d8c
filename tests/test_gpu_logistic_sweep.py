"""Up to eight inner-GD logistic GADMM solves in one launch (csrc/kernels/chain_logistic_sweep.hip,
engine/logistic_sweep.py, ``logistic_admm_sweep``), one solve per XCD.

Yardsticks: the long-double recurrence of tests/hp_reference.py under its bound rule (as
tests/test_gpu_dispatch_classes.py holds the single kernel), each member's own ``chain_admm`` solve bit for
bit, the graph engine bit for bit on the one-wave layout, and E3's pinned iteration counts.

Run with: pytest -m gpu tests/test_gpu_logistic_sweep.py
"""
import numpy as np
import pytest
import torch

import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
K = H.K_ITERS
HP_SHAPES = [s for s in H.LOGISTIC_SHAPES if max(s[1], s[2]) <= 64]
assert (3, 5, 3) in HP_SHAPES and (3, 40, 52) in HP_SHAPES and (3, 40, 53) in HP_SHAPES and (3, 64, 64) in HP_SHAPES
GD = dict(local_solver="gd", step=2.2)  # E3's inner solver (BASELINE configs[2])


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("n,m,d,inner_tol", [s + (0.0,) for s in HP_SHAPES] + [H.LIVE_STOP[0] + (H.LIVE_STOP[1],)])
def test_member_meets_the_long_double_reference(n, m, d, inner_tol):
    """Three members (rho, rho / 2, 2 rho) in one launch, K iterations of MAX_INNER inner steps: the member
    at the case's rho against ``hp_reference.logistic_case``; the last case has a live inner stop rule."""
    from gadmm_amd.engine.logistic_sweep import LogisticSweepEngine
    X, y, rho, lam, step, _ = H.logistic_case(n, m, d, inner_tol=inner_tol)
    sw = LogisticSweepEngine.build(_dev(X), _dev(y), list(range(n)), n,
                                   [(rho * f, step, H.MAX_INNER, inner_tol) for f in (1.0, 0.5, 2.0)], obj0=0.0,
                                   tols=0.0, max_iters=K, lam=lam)
    runs = sw.run()
    assert sw.last_kernel == "persistent-logistic-sweep(zrec)" and [r.iters for r in runs] == [K] * 3
    eng = sw.members[0]
    last = eng.ctl_state()["iter"] - 1
    assert K <= last <= K + H.PERSISTENT_OVERRUN, last
    ref = H.logistic_case(n, m, d, last, inner_tol=inner_tol)[5]
    th = eng.local_theta().cpu().numpy()
    eng.flush_duals()
    eng.stream.synchronize()
    mu = eng.mu.cpu().numpy()
    ratios = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj,
              "theta": ref.err_theta(th, last) / ref.b_theta, "dual": ref.err_dual(mu) / ref.b_dual}
    sw.close()
    print("logistic sweep %s: err/bound %s" % ((n, m, d, inner_tol), " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


def _hp_model(n, m, d):
    from gadmm_amd.models import LogisticRegression
    X, y, rho, lam, step, _ = H.logistic_case(n, m, d)
    return LogisticRegression(_dev(X), _dev(y), lam=lam), rho, step


def _state(r):
    """(theta, mu, stop code) as the kernel left them."""
    eng = r.extra["engine_obj"]
    return eng.local_theta().cpu().numpy().copy(), eng.mu.cpu().numpy().copy(), eng.ctl_state()["done"]


def _single(model, n, mem, obj0, tol, max_iter, step, **opts):
    """The member's own ``chain_admm`` solve and its (theta, mu) as the kernel left them at the stop."""
    from gadmm_amd.algorithms import chain_admm
    r = chain_admm(model, list(range(n)), n, mem[0], obj0, tol, max_iter, local_solver="gd", step=step,
                   max_inner=mem[1], inner_tol=mem[2], engine_opts=dict({"cache": False, "state": False}, **opts))
    return r, _state(r)


def _same(g, r, g_state, r_state):
    assert g.iters == r.iters and g.converged == r.converged, (g.iters, r.iters)
    assert np.array_equal(g.obj, r.obj)
    assert np.array_equal(g_state[0], r_state[0]) and np.array_equal(g_state[1], r_state[1])
    assert g_state[2] == r_state[2] and g_state[2] == (1 if g.converged else 2), (g_state[2], r_state[2])


@pytest.mark.parametrize("zrec", ["1", "0"])
@pytest.mark.parametrize("n,m,d", [(4, 30, 20), (3, 40, 53)])  # one shape per register class
def test_every_member_equals_its_single_solve(n, m, d, zrec, monkeypatch):
    """Members of different rho / max_inner / inner_tol: iterations, stop, objective trace and theta / mu at
    the stop == each member's own chain_admm, on both layouts; the one-wave layout also == the graph engine."""
    from gadmm_amd.algorithms import logistic_admm_sweep
    monkeypatch.setenv("GADMM_LOGISTIC_ZREC", zrec)
    model, rho, step = _hp_model(n, m, d)
    members = [(rho, H.MAX_INNER, 0.0), (rho * 0.5, 9, 1e-3), (rho * 2.0, 3, 1e-6)]
    got = logistic_admm_sweep(model, list(range(n)), n, members, 0.0, 0.0, 30, step=step, engine_opts={"cache": False})
    states = [_state(g) for g in got]
    for j, (g, mem) in enumerate(zip(got, members)):
        assert "sweep_fallback" not in g.extra and g.extra["sweep"]["slot"] == j and g.extra["sweep"]["width"] == 3
        assert g.extra["sweep_kernel"] == "persistent-logistic-sweep(%s)" % ("zrec" if zrec == "1" else "1w")
        r, r_state = _single(model, n, mem, 0.0, 0.0, 30, step)
        assert r.extra["engine"] == "persistent" and g.iters == 30
        _same(g, r, states[j], r_state)
        if zrec == "0":
            gr, _ = _single(model, n, mem, 0.0, 0.0, 30, step, persistent=False, block=8)
            assert gr.extra["engine"] == "graph" and np.array_equal(g.obj, gr.obj)


@pytest.mark.parametrize("width", [1, 8])
def test_width_one_and_eight(width):
    from gadmm_amd.algorithms import logistic_admm_sweep
    model, rho, step = _hp_model(3, 5, 3)
    members = [(rho * (1.0 + 0.25 * j), H.MAX_INNER, 0.0) for j in range(width)]
    got = logistic_admm_sweep(model, [0, 1, 2], 3, members, 0.0, 0.0, K, step=step, engine_opts={"cache": False})
    states = [_state(g) for g in got]
    assert [g.extra["sweep"]["width"] for g in got] == [width] * width
    for g, st, mem in zip(got, states, members):
        r, r_state = _single(model, 3, mem, 0.0, 0.0, K, step)
        _same(g, r, st, r_state)


@pytest.fixture(scope="module")
def e3(log24):
    from gadmm_amd.models import LogisticRegression
    return LogisticRegression(log24.X.to(DEV), log24.y.to(DEV), lam=1e-5)


@pytest.fixture(scope="module")
def e3_pair(e3, log_obj0):
    """E3's own sweep, rho = 3e-4 and 2e-4 to the 1e-4 gap, run once and shared (read-only)."""
    from gadmm_amd.algorithms import logistic_admm_sweep
    got = logistic_admm_sweep(e3, list(range(24)), 24, [3e-4, 2e-4], log_obj0, 1e-4, 400, engine_opts={"cache": False},
                              **{"step": 2.2})
    for g in got:
        g.obj.setflags(write=False)
    return got, [_state(g) for g in got]


def test_e3_shape_gives_the_pinned_iterations(e3, e3_pair, log_obj0):
    got, states = e3_pair
    assert [g.iters for g in got] == [274, 53] and all(g.converged for g in got)
    assert [g.extra["sweep"]["placed"] for g in got] == [2, 2]
    r, r_state = _single(e3, 24, (2e-4, 100, 1e-4), log_obj0, 1e-4, 400, 2.2)
    _same(got[1], r, states[1], r_state)


def test_mixed_stops_leave_the_other_members_alone(e3, e3_pair, log_obj0):
    """A third member that runs to its iteration cap (tol 1e-13) next to the two that converge."""
    from gadmm_amd.algorithms import logistic_admm_sweep
    pair, pair_states = e3_pair
    got = logistic_admm_sweep(e3, list(range(24)), 24, [3e-4, 2e-4, 2e-4], log_obj0, 1e-4, 400, tols=[1e-4, 1e-4, 1e-13],
                              step=2.2, engine_opts={"cache": False})
    assert [g.iters for g in got] == [274, 53, 400] and [g.converged for g in got] == [True, True, False]
    for g, p, ps in zip(got, pair, pair_states):
        _same(g, p, _state(g), ps)
    assert np.array_equal(got[2].obj[:53], got[1].obj)


def test_placement_is_speed_only(log24, log_obj0):
    from gadmm_amd.engine.logistic_sweep import LogisticSweepEngine
    out = {}
    for xcd in (0, 2):
        sw = LogisticSweepEngine.build(log24.X.to(DEV), log24.y.to(DEV), list(range(24)), 24,
                                       [(2e-4, 2.2, 100, 1e-4), (1e-3, 2.2, 50, 1e-4)], obj0=log_obj0, tols=1e-4,
                                       max_iters=60, lam=1e-5, xcd=xcd)
        runs = sw.run()
        assert sw.last_placed == ([2, 2] if xcd == 2 else [1, 1])
        out[xcd] = [(r.iters, r.done, m.objective_trace(r.iters).copy(), m.local_theta().cpu().numpy())
                    for r, m in zip(runs, sw.members)]
        sw.close()
    for a, b in zip(out[0], out[2]):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert out[2][0][0] == 53


def test_residency_refusal_is_the_loop(e3, e3_pair, log_obj0, monkeypatch):
    """Sixteen CUs hold two 76 KB workgroups each: one 25-workgroup member fits, two do not. Refused before
    any launch, and every member solved alone on the same persistent kernel."""
    from gadmm_amd.algorithms import logistic_admm_sweep
    from gadmm_amd.engine import logistic_sweep
    launched = []
    real = logistic_sweep.LogisticSweepEngine._collect
    monkeypatch.setattr(logistic_sweep.LogisticSweepEngine, "_collect",
                        lambda self, *a, **k: launched.append(1) or real(self, *a, **k))
    monkeypatch.setenv("GADMM_CU_BUDGET", "16")
    got = logistic_admm_sweep(e3, list(range(24)), 24, [3e-4, 2e-4], log_obj0, 1e-4, 400, step=2.2,
                              engine_opts={"cache": False})
    assert not launched
    for g, p in zip(got, e3_pair[0]):
        assert g.extra["sweep_fallback"].startswith("ResidencyError"), g.extra["sweep_fallback"]
        assert g.extra["engine"] == "persistent" and g.iters == p.iters and g.converged == p.converged
        assert np.array_equal(g.obj, p.obj)


def test_entry_switch(tmp_path):
    from gadmm_amd import entry
    runs = {}
    for name, extra in (("seq", []), ("con", ["--set", "sweep=concurrent"])):
        out = entry.get("LogisticRegression_Synthetic").main(
            ["--quick", "--device", "cuda", "--out", str(tmp_path / name), "--no-plot", "--no-baselines"] + extra)
        runs[name] = out["runs"]
    assert sorted(runs["con"]) == sorted(runs["seq"]) and runs["seq"]
    for k, s in runs["seq"].items():
        assert runs["con"][k]["iters"] == s["iters"], k
        if not k.startswith("GADMM_exact"):
            assert runs["con"][k]["sweep_kernel"].startswith("persistent-logistic-sweep"), runs["con"][k]
