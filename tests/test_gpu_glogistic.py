"""Logistic GGADMM on the persistent kernel (csrc/kernels/graph_persistent_logistic.hip) on the MI355X, held
to the long-double EDGE-DUAL reference of tests/hp_glogistic.py (err / bound <= 1 with ``hp_reference.bound``)
and to the torch path on the device (same stop iteration, traces at rtol 1e-11: what tests/test_gpu.py asks of
the one-wave logistic chain kernel against torch). The cases and what each exercises: ``hp_glogistic.CASES``.
No test provokes a timeout, a fault or a hang: the deadline path is read, not exercised.
"""
import numpy as np
import pytest
import torch

import hp_glogistic as GL
import hp_reference as H
from hp_ggadmm import OVERRUN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
K = H.K_ITERS
STAR12 = "star12hub5-m53-d20"


@pytest.fixture(autouse=True)
def _poison_lds():
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _model(name):
    from gadmm_amd.models import LogisticRegression
    g, X, y, rho, lam, step, itol = GL.case_data(name)
    return LogisticRegression(_dev(X), _dev(y), lam)


def _engine(name, max_iter, obj0=0.0, tol=0.0, **kw):
    from gadmm_amd.engine.graph_logistic_engine import NativeGraphLogisticEngine
    g, X, y, rho, lam, step, itol = GL.case_data(name)
    return NativeGraphLogisticEngine(_dev(X), _dev(y), g, rho, obj0, tol, max_iter, lam, step, H.MAX_INNER, itol, **kw)


@pytest.mark.parametrize("name", list(GL.CASES))
def test_native_against_long_double_reference(name):
    """K iterations; the cap's stop decision arrives ``lag`` iterations late, so theta, mu and the step counts are
    compared at ctl.iter - 1 = last, the objective trace and the K4 rows over iterations 1..K."""
    g = GL.case_data(name)[0]
    eng = _engine(name, K)
    assert eng.eligible(), eng.refusal()
    r = eng.run()
    last = eng.ctl_state()["iter"] - 1
    assert r.done == 2 and r.iters == K and K <= last <= K + OVERRUN, (r.iters, r.done, last)
    bound_k = min([k for k in (2, 4, 8) if k >= g.max_degree] or [8 * ((g.max_degree + 7) // 8)])
    assert eng.last_kernel == "persistent-graph-logistic(deg<=%d)" % bound_k, eng.last_kernel
    ref = GL.case(name, last)[-1]
    rows, tails, inner = _host(eng.rres[:K]), ref.tails[:K], ref.extra[0][last - 1]
    assert np.all(rows[~tails] == 0.0) and np.all(np.isfinite(rows[tails])) and np.all(rows[tails] > 0)
    ratios = {"theta": ref.err_theta(_host(eng.theta), last) / ref.b_theta,
              "dual": ref.err_dual(_host(eng.mu)) / ref.b_dual,
              "objective": ref.err_obj(eng.traces(K)[0]) / ref.b_obj, "K4 rows": ref.err_res_w(rows) / ref.b_res_w}
    print("glogistic native %s (last=%d, %s): err/bound %s; inner steps %s" % (
        name, last, eng.last_kernel, " ".join("%s %.3f" % kv for kv in ratios.items()), inner.tolist()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert np.array_equal(_host(eng.inner_iters), inner) and (name != GL.LIVE or inner.max() < H.MAX_INNER)


@pytest.mark.parametrize("name", list(GL.CASES))
def test_native_against_torch_path_on_device(name):
    """To the 1e-4 gap of ``model.optimum()``: the same stop iteration, the objective trace at rtol 1e-11, the
    residual within the slack derived in tests/test_gpu_ggadmm.py (eta = 1e-11, C = |E| d squared terms)."""
    from gadmm_amd.algorithms import graph_admm_logistic
    g, X, y, rho, lam, step, itol = GL.case_data(name)
    m = _model(name)
    a, b = (graph_admm_logistic(m, g, rho, m.optimum(), 1e-4, 3000, step, max_inner=H.MAX_INNER, inner_tol=itol,
                                backend=be) for be in ("native", "torch"))
    print("%s: native %d iterations (%s, placed %d), torch %d" % (name, a.iters, a.extra["kernel"], a.extra["placed"],
                                                                  b.iters))
    assert a.extra["backend"] == "native" and a.extra["engine"] == "persistent" and "state" not in a.extra
    assert b.extra["backend"] == "torch" and "graph_fallback" not in b.extra
    assert a.converged and b.converged and a.iters == b.iters and np.allclose(a.obj, b.obj, rtol=1e-11, atol=0)
    assert np.array_equal(a.comm_units, b.comm_units) and a.extra["deliveries"] == b.extra["deliveries"] \
        == a.iters * 2 * len(g.edges) and a.extra["graph"] == b.extra["graph"] == g.describe()
    S, C = float(b.extra["state"][0].abs().max()), len(g.edges) * m.d
    slack = 4e-11 * S * np.sqrt(C * b.primal_res) + 4e-22 * S * S * C
    assert np.all(np.abs(a.primal_res - b.primal_res) <= slack)


def test_xcd_packing_and_second_solve_bit_for_bit():
    """``xcd=2`` against ``xcd=0``, and a second solve on the same engine after ``reset()``: all bit for bit."""
    obj0, out = _model(STAR12).optimum(), []
    for xcd in (2, 0, 0):
        eng = _engine(STAR12, 600, obj0, 1e-4, xcd=xcd) if len(out) < 2 else eng
        eng.reset()
        r = eng.run()
        assert eng.last_placed == xcd and r.done == 1, (r.done, eng.last_placed)
        out.append((r.iters, eng.traces(r.iters)[0], _host(eng.theta), _host(eng.mu), _host(eng.rres[:r.iters]),
                    _host(eng.inner_iters)))
    for other in out[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(out[0], other))


def test_dispatch_m65_takes_the_torch_path():
    from gadmm_amd.algorithms import graph_admm_logistic
    from gadmm_amd.models import LogisticRegression
    from gadmm_amd.parallel.topology import ring_graph
    X, y, rho, lam, step = H.make_logistic(4, 65, 20, 11)
    m = LogisticRegression(_dev(X), _dev(y), lam)
    r = graph_admm_logistic(m, ring_graph(4), rho, 0.0, 0.0, 3, step, max_inner=H.MAX_INNER)
    assert r.extra["backend"] == "torch" and r.extra["graph_fallback"] == "max(d, m) > 64"
    with pytest.raises(RuntimeError):
        graph_admm_logistic(m, ring_graph(4), rho, 0.0, 0.0, 3, step, backend="native")


def test_entry_on_the_gpu(tmp_path):
    from gadmm_amd.entry import LogisticRegression_Topologies as E
    out = E.main(["--device", "cuda", "--out", str(tmp_path), "--no-plot"])
    assert len(out["runs"]) == 5
    for key, s in out["runs"].items():
        assert s["converged"] and s["engine"] == "persistent" and "graph_fallback" not in s, (key, s)
        assert s["kernel"].startswith("persistent-graph-logistic"), (key, s["kernel"])
    with open(out["summary_path"]) as f:
        assert "persistent-graph-logistic" in f.read()
