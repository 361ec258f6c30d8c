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


# The batches below name buffers by made-up addresses, so none of them may ever reach a launch: the LAST
# entry of every batch keeps an iteration-tag range that the launcher refuses (start_iter + max_iter +
# lag >= 2^20), and each case adds ONE defect to an earlier entry, so the message tells which check fired.
_WRITTEN = ("ctl", "trace", "theta", "mu", "blk_tab", "objg", "decg", "xchk", "tstamp", "rres")
_READ_ONLY = ("A", "b", "yy", "Minv", "slots")


def _valid(nb):
    """Entries that pass every per-entry check but the last one's tag range: addresses that are never
    dereferenced, distinct per entry and per field."""
    batch = (native.PersistArgs * max(nb, 1))()
    for j in range(nb):
        a = batch[j]
        a.d, a.n, a.n_local, a.start_iter, a.max_iter, a.lag, a.ring, a.nvar = 14, 24, 24, 1, 100, 8, 12, 2
        a.has_monitor, a.nranks, a.blk_pw, a.blk_k, a.blk_len = 1, 1, 1, 2, 4
        for i, f in enumerate(_READ_ONLY + _WRITTEN + ("dec_push",)):
            setattr(a, f, 0x10000000 + 0x100000 * j + 0x1000 * (i + 1))
    batch[max(nb, 1) - 1].max_iter = 1 << 20  # never launched, whatever else the case changes
    return batch


def test_sweep_launch_base_batch_is_refused_by_its_tag_range_only():
    for nb in (1, 3, 8):
        rc, msg = _launch(_valid(nb), nb)
        assert rc == -1 and "blocked sweep: solve %d: ring/lag/tag range" % (nb - 1) in msg, msg


def test_sweep_launch_refuses_null_batch_or_staging():
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    batch = _valid(1)
    for args in ((None, 1, ctypes.addressof(stage), ctypes.addressof(stage)),
                 (batch, 1, None, ctypes.addressof(stage)), (batch, 1, ctypes.addressof(stage), None)):
        assert lib.gadmm_chain_blocked_sweep_launch(*args, None) == -1
        assert "blocked sweep: null batch or staging buffer" in lib.gadmm_last_error().decode()


def test_sweep_launch_refuses_more_workgroups_than_the_placement_check_holds():
    batch = _valid(2)
    batch[0].n = batch[0].n_local = 768  # 768 / 4 worker + 768 / 12 objective workgroups + the monitor
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 0 has 257 workgroups, the placement check holds 256" in msg, msg


@pytest.mark.parametrize("field,value", [("ring", 9), ("lag", 0), ("max_iter", 1 << 20)])
def test_sweep_launch_refuses_ring_lag_tag_range(field, value):
    batch = _valid(3)
    setattr(batch[1], field, value)  # lag = 8: ring 9 = lag + 1
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "blocked sweep: solve 1: ring/lag/tag range" in msg, msg


@pytest.mark.parametrize("name", _WRITTEN)
def test_sweep_launch_refuses_a_shared_written_buffer(name):
    batch = _valid(3)
    setattr(batch[0], name, 0x7fff0000)
    setattr(batch[1], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "blocked sweep: solves 0 and 1 share a buffer that both write" in msg, msg


@pytest.mark.parametrize("name", _READ_ONLY)
def test_sweep_launch_lets_read_only_inputs_be_shared(name):
    batch = _valid(3)
    for j in range(3):
        setattr(batch[j], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "solve 2: ring/lag/tag range" in msg, msg  # no earlier check objected


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
