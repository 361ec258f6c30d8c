"""Concurrent D-GADMM coherence sweep, the parts that need no device: the sequential fallback of
``dynamic_group_admm_sweep``, its argument checks, the grouping of long coherence lists, and the
dynamic sweep launcher's validation (refused with -1 and a message before any HIP call)."""
import ctypes

import numpy as np
import pytest

from gadmm_amd.algorithms import dynamic_group_admm, dynamic_group_admm_sweep
from gadmm_amd.algorithms import gadmm as G
from gadmm_amd.data import linear_synthetic
from gadmm_amd.models import LinearRegression
from gadmm_amd.ops import native
from gadmm_amd.parallel import topology as T


@pytest.fixture(scope="module")
def prob():
    ds = linear_synthetic(24)
    m = LinearRegression(ds.X, ds.y)
    p0, c0, _ = T.find_path(24, np.random.default_rng(5))
    return m, m.optimum(), p0, c0


def _same(g, r):
    assert g.iters == r.iters and g.converged == r.converged
    assert np.array_equal(g.obj, r.obj)
    assert np.array_equal(g.com_cost, r.com_cost)
    assert np.array_equal(g.comm_units, r.comm_units)


def test_sweep_on_cpu_is_the_loop_of_dynamic_group_admm(prob):
    m, obj0, p0, c0 = prob
    cohs, seeds = (1, 10, 401), (7, 8, 9)  # the last one never re-chains within 400 iterations
    got = dynamic_group_admm_sweep(m, 1.0, obj0, 1e-4, 400, p0, c0, cohs, seeds)
    ref = [dynamic_group_admm(m, 1.0, obj0, 1e-4, 400, p0, c0, c, seed=s) for c, s in zip(cohs, seeds)]
    assert len(got) == 3
    for g, r, c in zip(got, ref, cohs):
        _same(g, r)
        assert g.algorithm == "D-GADMM(coh=%s)" % c
        assert g.extra["sweep_fallback"] == "cpu tensors"
        assert "sweep" not in g.extra
    assert not np.array_equal(got[0].obj[:50], got[1].obj[:50])  # the members do follow different chains


def test_seeds_and_coherences_of_different_lengths_raise(prob):
    m, obj0, p0, c0 = prob
    with pytest.raises(ValueError, match="seeds"):
        dynamic_group_admm_sweep(m, 1.0, obj0, 1e-4, 50, p0, c0, (1, 10, 50), (1, 2))
    with pytest.raises(ValueError, match="max_iters"):
        dynamic_group_admm_sweep(m, 1.0, obj0, 1e-4, 50, p0, c0, (1, 10), (1, 2), max_iters=(50,))
    assert dynamic_group_admm_sweep(m, 1.0, obj0, 1e-4, 50, p0, c0, (), ()) == []


def test_eleven_members_run_as_eight_plus_three_in_input_order(prob, monkeypatch):
    """The grouping the device path uses (run_in_groups over sweep_capacity), and on CPU tensors eleven
    members come back in input order."""
    assert native.require().gadmm_chain_blocked_sweep_capacity() == 8
    cohs = [11 - i for i in range(11)]  # not sorted: the order is the caller's
    seen = []

    def run_group(items, idx):
        seen.append((list(items), list(idx)))
        return [("solved", c) for c in items]

    out = G.run_in_groups(cohs, 8, run_group)
    assert [len(s[0]) for s in seen] == [8, 3] and seen[1][1] == [8, 9, 10]
    assert out == [("solved", c) for c in cohs]
    m, obj0, p0, c0 = prob
    got = dynamic_group_admm_sweep(m, 1.0, obj0, 1e-4, 30, p0, c0, cohs, list(range(11)))
    assert [g.algorithm for g in got] == ["D-GADMM(coh=%s)" % c for c in cohs]
    for g, c, s in zip(got[8:], cohs[8:], range(8, 11)):
        _same(g, dynamic_group_admm(m, 1.0, obj0, 1e-4, 30, p0, c0, c, seed=s))


# ---- launcher validation: refused with -1 and a message before any HIP call (no device here)
def _launch(batch, nb):
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    rc = lib.gadmm_chain_blocked_dyn_sweep_launch(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def _valid(n_entries):
    """Entries that pass every per-entry check: addresses that are never dereferenced (the launcher
    refuses, or the test stops, before any HIP call), distinct per entry and per field."""
    batch = (native.PersistArgs * n_entries)()
    for j in range(n_entries):
        a = batch[j]
        a.d, a.n, a.n_local, a.start_iter, a.max_iter, a.lag, a.ring, a.nvar = 14, 24, 24, 1, 100, 8, 12, 2
        a.has_monitor, a.nranks, a.blk_pw, a.blk_k, a.blk_len, a.n_epochs = 1, 1, 1, 2, 4, 3
        base = 0x10000 * (j + 1)
        for i, f in enumerate(("slots", "Minv", "A", "b", "yy", "theta", "mu", "objg", "decg", "dec_push", "trace",
                               "ctl", "blk_tab", "epoch_start", "ep_slots", "ep_pos", "ep_flush", "minv_pad", "xchk",
                               "tstamp")):
            setattr(a, f, base + 0x100 * (i + 1))
    return batch


@pytest.mark.parametrize("nb", [0, 9])
def test_dyn_sweep_launch_refuses_width(nb):
    rc, msg = _launch(_valid(9), nb)
    assert rc == -1 and "1..8" in msg


def test_dyn_sweep_launch_refuses_static_entry():
    batch = _valid(2)
    batch[1].n_epochs = 0
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "static" in msg


def test_dyn_sweep_launch_refuses_multi_rank_entry():
    batch = _valid(2)
    batch[0].nranks = 2
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "multi-rank" in msg


def test_dyn_sweep_launch_refuses_mixed_register_classes():
    batch = _valid(2)
    batch[1].d = 50
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "register class" in msg


def test_dyn_sweep_launch_refuses_too_many_epochs():
    batch = _valid(1)
    epl = native.require().gadmm_chain_blocked_max_epochs()
    batch[0].n_epochs = epl + 1
    rc, msg = _launch(batch, 1)
    assert rc == -1 and "epochs" in msg


@pytest.mark.parametrize("field", ["epoch_start", "ep_slots", "ep_pos", "ep_flush", "minv_pad"])
def test_dyn_sweep_launch_refuses_missing_epoch_tables(field):
    batch = _valid(2)
    setattr(batch[1], field, None)
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "epoch tables" in msg


def test_dyn_sweep_launch_refuses_hard_stop_before_start():
    batch = _valid(1)
    batch[0].start_iter, batch[0].hard_stop = 10, 5
    rc, msg = _launch(batch, 1)
    assert rc == -1 and "hard stop" in msg


def test_dyn_sweep_launch_refuses_null_xchk():
    batch = _valid(1)
    batch[0].xchk = None
    rc, msg = _launch(batch, 1)
    assert rc == -1 and "xchk" in msg


def test_dyn_sweep_launch_refuses_two_entries_sharing_blk_tab():
    batch = _valid(2)
    batch[1].blk_tab = batch[0].blk_tab
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "share a buffer" in msg


# The cases below pass every check the ones above stop at, so none of their batches may ever reach a
# launch: the LAST entry keeps an iteration-tag range that the launcher refuses (start_iter + max_iter +
# lag >= 2^20), and each case adds ONE defect to an earlier entry, so the message tells which check fired.
_WRITTEN = ("ctl", "trace", "theta", "mu", "blk_tab", "objg", "decg", "xchk", "tstamp", "rres")
_READ_ONLY = ("A", "b", "yy", "Minv", "slots")


def _guarded(nb):
    batch = _valid(nb)
    for j in range(nb):
        batch[j].rres = 0x10000 * (j + 1) + 0x100 * 0x40
    batch[nb - 1].max_iter = 1 << 20  # never launched, whatever else the case changes
    return batch


def test_dyn_sweep_launch_base_batch_is_refused_by_its_tag_range_only():
    for nb in (1, 3, 8):
        rc, msg = _launch(_guarded(nb), nb)
        assert rc == -1 and "blocked dynamic sweep: solve %d: ring/lag/tag range" % (nb - 1) in msg, msg


def test_dyn_sweep_launch_refuses_null_batch_or_staging():
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    batch = _guarded(1)
    for args in ((None, 1, ctypes.addressof(stage), ctypes.addressof(stage)),
                 (batch, 1, None, ctypes.addressof(stage)), (batch, 1, ctypes.addressof(stage), None)):
        assert lib.gadmm_chain_blocked_dyn_sweep_launch(*args, None) == -1
        assert "blocked dynamic sweep: null batch or staging buffer" in lib.gadmm_last_error().decode()


def test_dyn_sweep_launch_refuses_more_workgroups_than_the_placement_check_holds():
    batch = _guarded(2)
    batch[0].n = batch[0].n_local = 768  # 768 / 4 worker + 768 / 12 objective workgroups + the monitor
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 0 has 257 workgroups, the placement check holds 256" in msg, msg


@pytest.mark.parametrize("field,value", [("ring", 9), ("lag", 0), ("max_iter", 1 << 20)])
def test_dyn_sweep_launch_refuses_ring_lag_tag_range(field, value):
    batch = _guarded(3)
    setattr(batch[1], field, value)  # lag = 8: ring 9 = lag + 1
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "blocked dynamic sweep: solve 1: ring/lag/tag range" in msg, msg


@pytest.mark.parametrize("name", _WRITTEN)
def test_dyn_sweep_launch_refuses_a_shared_written_buffer(name):
    batch = _guarded(3)
    setattr(batch[0], name, 0x7fff0000)
    setattr(batch[1], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "blocked dynamic sweep: solves 0 and 1 share a buffer that both write" in msg, msg


@pytest.mark.parametrize("name", _READ_ONLY)
def test_dyn_sweep_launch_lets_read_only_inputs_be_shared(name):
    batch = _guarded(3)
    for j in range(3):
        setattr(batch[j], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "solve 2: ring/lag/tag range" in msg, msg  # no earlier check objected


def test_static_sweep_launcher_still_refuses_what_the_dynamic_one_takes():
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    rc = lib.gadmm_chain_blocked_sweep_launch(_valid(1), 1, ctypes.addressof(stage), ctypes.addressof(stage), None)
    assert rc == -1 and "dynamic" in lib.gadmm_last_error().decode()
