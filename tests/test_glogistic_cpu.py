"""Logistic GGADMM (``graph_admm_logistic``) without a GPU: the torch path against the long-double edge-dual
reference of tests/hp_glogistic.py and ``chain_admm``'s torch path, the refusals, and the entry."""
import numpy as np
import pytest
import torch

import hp_glogistic as GL
import hp_reference as H

from gadmm_amd.parallel import topology as T

K = H.K_ITERS


def _model(X, y, lam):
    from gadmm_amd.models import LogisticRegression
    return LogisticRegression(torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(y)), lam)


@pytest.mark.parametrize("name", list(GL.CASES))
def test_torch_path_against_long_double_reference(name):
    from gadmm_amd.algorithms import graph_admm_logistic
    g, X, y, rho, lam, step, tol, ref = GL.case(name)
    r = graph_admm_logistic(_model(X, y, lam), g, rho, 0.0, 0.0, K, step, max_inner=H.MAX_INNER, inner_tol=tol,
                            backend="torch")
    th, mu, nxt = r.extra["state"]
    ratios = {"theta": ref.err_theta(th.numpy(), K) / ref.b_theta, "dual": ref.err_dual(mu.numpy()) / ref.b_dual,
              "objective": ref.err_obj(r.obj) / ref.b_obj}
    print("glogistic torch %s: err/bound %s" % (name, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert nxt == K + 1 and r.iters == K and not r.converged and all(v <= 1.0 for v in ratios.values()), ratios
    assert r.extra["deliveries"] == K * 2 * len(g.edges) and r.extra["graph"] == g.describe() \
        and np.array_equal(r.comm_units, np.arange(1, K + 1) * g.n)
    inner, margin = ref.extra
    assert r.extra["inner_steps_mean"] == pytest.approx(inner.mean())
    # the live case: the stop rule acts and no test sits on its threshold
    assert (margin >= 1e-6 and inner[-1].max() < H.MAX_INNER) if name == GL.LIVE else np.all(inner == H.MAX_INNER)


@pytest.mark.parametrize("n,m,d", [(2, 5, 3), (5, 30, 20)])
def test_chain_graph_is_chain_admm_bit_for_bit(n, m, d):
    from gadmm_amd.algorithms import chain_admm, graph_admm_logistic
    X, y, rho, lam, step = H.make_logistic(n, m, d, H.seed_of(n, m, d))
    model = _model(X, y, lam)
    a = graph_admm_logistic(model, T.chain_graph(n), rho, 0.0, 0.0, K, step, max_inner=H.MAX_INNER, inner_tol=1e-3,
                            backend="torch")
    c = chain_admm(model, list(range(n)), n, rho, 0.0, 0.0, K, local_solver="gd", step=step, max_inner=H.MAX_INNER,
                   inner_tol=1e-3, backend="torch")
    assert np.array_equal(a.obj, c.obj)
    assert all(torch.equal(x, z) for x, z in zip(a.extra["state"][:2], c.extra["state"][:2]))
    assert a.extra["inner_steps_mean"] == c.extra["inner_steps_mean"]


def test_refusals():
    from gadmm_amd.algorithms import generalized_group_admm_logistic_gd, graph_admm, graph_admm_logistic
    from gadmm_amd.models import LinearRegression
    assert generalized_group_admm_logistic_gd is graph_admm_logistic
    g, X, y, rho, lam, step, tol = GL.case_data("ring4-m30-d20")
    m = _model(X, y, lam)
    with pytest.raises(NotImplementedError, match="linear model"):
        graph_admm(m, g, rho, 0.0, 1e-4, 3)
    with pytest.raises(NotImplementedError, match="logistic model"):
        graph_admm_logistic(LinearRegression(m.X, m.y), g, rho, 0.0, 1e-4, 3, step)

    class TwoRanks:
        nranks, rank = 2, 0
    with pytest.raises(NotImplementedError, match="2 ranks"):
        graph_admm_logistic(m, g, rho, 0.0, 1e-4, 3, step, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match="every worker local"):
        graph_admm_logistic(m, T.ring_graph(6), rho, 0.0, 1e-4, 3, step)
    with pytest.raises(RuntimeError, match="cpu tensors"):
        graph_admm_logistic(m, g, rho, 0.0, 1e-4, 3, step, backend="native")
    assert graph_admm_logistic(m, g, rho, 0.0, 1e-4, 3, step).extra["graph_fallback"] == "cpu tensors"
    assert "graph_fallback" not in graph_admm_logistic(m, g, rho, 0.0, 1e-4, 3, step, backend="torch").extra


def test_entry_quick_on_cpu_and_abi(tmp_path):
    from gadmm_amd import entry
    from gadmm_amd.config import get_preset
    from gadmm_amd.ops import native
    cfg = get_preset("LogisticRegression_Topologies")
    assert "LogisticRegression_Topologies" in entry.ENTRIES and cfg.rhos == [2e-4] and cfg.lam == 1e-5
    out = entry.get("LogisticRegression_Topologies").main(["--quick", "--device", "cpu", "--no-plot", "--out",
                                                           str(tmp_path)])
    want = {"chain": 53, "ring": 212, "grid:4x6": 128, "star:0": 134, "kbip": 257}  # the entry's docstring
    assert cfg.graphs == list(want) and list(out["runs"]) == ["GGADMM-logistic_%s_rho0.0002" % s for s in want]
    for spec, iters in want.items():
        s = out["runs"]["GGADMM-logistic_%s_rho0.0002" % spec]
        assert s["iters"] == iters and s["converged"] and s["engine"] == s["kernel"] == "torch"
        assert s["graph_name"] == spec and s["graph_fallback"] == "cpu tensors"
    native.check_graph_logistic_abi(native.require())  # raises on a layout mismatch
