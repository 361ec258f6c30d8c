"""Concurrent rho sweep, the parts that need no device: the sequential fallback of
``chain_admm_sweep``, the sweep launcher's argument validation, and the grouping of long rho lists."""
import ctypes

import numpy as np
import pytest
import torch

from gadmm_amd.algorithms import chain_admm, chain_admm_sweep
from gadmm_amd.algorithms.gadmm import run_in_groups, sweep_groups
from gadmm_amd.data import linear_synthetic
from gadmm_amd.models import LinearRegression
from gadmm_amd.ops import native


def test_sweep_on_cpu_is_the_loop_of_chain_admm():
    ds = linear_synthetic(24)
    m = LinearRegression(ds.X, ds.y)
    obj0 = m.optimum()
    ids = list(range(24))
    rhos = (3.0, 5.0, 7.0)
    got = chain_admm_sweep(m, ids, 24, rhos, obj0, 1e-4, 1000)
    ref = [chain_admm(m, ids, 24, rho, obj0, 1e-4, 1000) for rho in rhos]
    assert [r.iters for r in got] == [784, 434, 248]
    for g, r in zip(got, ref):
        assert g.iters == r.iters and g.converged == r.converged
        assert np.array_equal(g.obj, r.obj)
        assert np.array_equal(g.loss, r.loss)
        assert np.array_equal(g.comm_units, r.comm_units)
        assert g.extra["sweep_fallback"]
        assert "sweep" not in g.extra


def test_sweep_tols_are_per_rho():
    ds = linear_synthetic(24)
    m = LinearRegression(ds.X, ds.y)
    obj0 = m.optimum()
    ids = list(range(24))
    got = chain_admm_sweep(m, ids, 24, (7.0, 7.0), obj0, 1e-4, 1000, tols=(1e-2, 1e-4))
    assert got[1].iters == 248 and got[0].iters < 248
    with pytest.raises(ValueError):
        chain_admm_sweep(m, ids, 24, (7.0, 7.0), obj0, 1e-4, 1000, tols=(1e-2,))


# ---- launcher validation: refused with -1 and a message before any HIP call (no device here)
def _launch(batch, nb):
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    rc = lib.gadmm_chain_blocked_sweep_launch(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def test_sweep_capacity_is_eight():
    assert native.require().gadmm_chain_blocked_sweep_capacity() == 8


@pytest.mark.parametrize("nb", [0, 9])
def test_sweep_launch_refuses_width(nb):
    rc, msg = _launch((native.PersistArgs * 9)(), nb)
    assert rc == -1 and msg


def test_sweep_launch_refuses_dynamic_entry():
    batch = (native.PersistArgs * 2)()
    batch[1].n_epochs = 1
    rc, msg = _launch(batch, 2)
    assert rc == -1 and msg


def test_sweep_launch_refuses_multi_rank_entry():
    batch = (native.PersistArgs * 2)()
    batch[0].nranks = 2
    rc, msg = _launch(batch, 2)
    assert rc == -1 and msg


def test_sweep_launch_refuses_mixed_register_classes():
    batch = (native.PersistArgs * 2)()
    batch[0].d, batch[1].d = 14, 50
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "register class" in msg


def test_sweep_launch_refuses_null_xchk():
    batch = (native.PersistArgs * 1)()
    batch[0].d = 14
    rc, msg = _launch(batch, 1)
    assert rc == -1 and "xchk" in msg


# ---- grouping: more values of rho than one launch takes
def test_eleven_values_run_as_eight_plus_three_in_input_order():
    assert [len(g) for g in sweep_groups(11, 8)] == [8, 3]
    assert sum(sweep_groups(11, 8), []) == list(range(11))
    rhos = [float(11 - i) for i in range(11)]  # not sorted: the order is the caller's
    seen = []

    def run_group(items, idx):
        seen.append((list(items), list(idx)))
        return [("solved", r) for r in reversed(list(reversed(items)))]

    out = run_in_groups(rhos, 8, run_group)
    assert [len(s[0]) for s in seen] == [8, 3]
    assert seen[1][1] == [8, 9, 10]
    assert out == [("solved", r) for r in rhos]


def test_groups_edge_cases():
    assert sweep_groups(0, 8) == []
    assert sweep_groups(8, 8) == [list(range(8))]
    assert [len(g) for g in sweep_groups(9, 8)] == [8, 1]
    with pytest.raises(ValueError):
        sweep_groups(3, 0)
    with pytest.raises(RuntimeError):
        run_in_groups([1.0, 2.0], 8, lambda items, idx: [0])
