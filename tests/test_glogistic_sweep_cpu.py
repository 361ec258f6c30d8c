"""Logistic GGADMM sweep (``graph_admm_logistic_sweep``, engine/graph_logistic_sweep.py), the parts that need no
device: the sequential fallback and its order, and the member and ``tols`` validation."""
import numpy as np
import pytest
import torch

import hp_glogistic as GL
import hp_reference as H

from gadmm_amd.algorithms import graph_admm_logistic, graph_admm_logistic_sweep
from gadmm_amd.parallel import topology as T

K = H.K_ITERS


@pytest.fixture(scope="module")
def ring4():
    from gadmm_amd.models import LogisticRegression
    g, X, y, rho, lam, step, _ = GL.case_data("ring4-m30-d20")
    return LogisticRegression(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(y)), lam), rho, step


def test_sweep_on_cpu_is_the_loop_of_graph_admm_logistic(ring4):
    m, rho, step = ring4
    members = [(T.ring_graph(4), rho), (T.star_graph(4, 0), 2 * rho), (T.ring_graph(4), rho, step, 3, 1e-3)]
    got = graph_admm_logistic_sweep(m, members, 0.0, 0.0, K, step, max_inner=H.MAX_INNER, inner_tol=0.0)
    assert len(got) == 3
    for g, mem in zip(got, members):
        st, mi, it = mem[2:] if len(mem) == 5 else (step, H.MAX_INNER, 0.0)
        r = graph_admm_logistic(m, mem[0], mem[1], 0.0, 0.0, K, st, max_inner=mi, inner_tol=it)
        assert g.iters == r.iters == K and g.converged == r.converged and np.array_equal(g.obj, r.obj)
        assert np.array_equal(g.comm_units, r.comm_units) and np.array_equal(g.primal_res, r.primal_res)
        assert g.extra["graph"] == mem[0].describe() and g.extra["deliveries"] == r.extra["deliveries"]
        assert g.extra["sweep_fallback"] == "cpu tensors" and "sweep" not in g.extra
    assert not np.array_equal(got[0].obj, got[2].obj)  # (the order is checked on results that differ)
    assert graph_admm_logistic_sweep(m, [], 0.0, 0.0, K, step) == []
    got = graph_admm_logistic_sweep(m, members[:1], 0.0, 0.0, 3, step, backend="torch")
    assert [g.extra["sweep_fallback"] for g in got] == ["torch backend"]


@pytest.mark.parametrize("bad", [(2.0,), ("ring", 2.0), (None, 2.0, 1.0), (None, 2.0, 1.0, 0, 1e-3),
                                 (None, 2.0, 1.0, 2.5, 1e-3), (None, 2.0, 1.0, 5, -1.0)])
def test_member_tuples_and_tols_are_validated(ring4, bad):
    m, rho, step = ring4
    mem = tuple(T.ring_graph(4) if x is None else x for x in bad)
    with pytest.raises(ValueError, match="member"):
        graph_admm_logistic_sweep(m, [(T.ring_graph(4), rho), mem], 0.0, 0.0, 3, step)
    with pytest.raises(ValueError, match="tols"):
        graph_admm_logistic_sweep(m, [(T.ring_graph(4), rho)] * 2, 0.0, 0.0, 3, step, tols=(1e-2,))


def test_a_graph_of_another_size_is_the_loop(ring4):
    """A member graph whose n is not the model's sends the call to the loop (the gate "a member graph's n differs
    from the model's"), where ``graph_admm_logistic`` refuses that member by name, as ``graph_admm_sweep`` does."""
    m, rho, step = ring4
    with pytest.raises(NotImplementedError, match="every worker local"):
        graph_admm_logistic_sweep(m, [(T.ring_graph(4), rho), (T.ring_graph(6), rho)], 0.0, 0.0, 3, step)
