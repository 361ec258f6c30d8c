"""Logistic sweep (``logistic_admm_sweep``, engine/logistic_sweep.py), the parts that need no device: the
sequential fallback and its order, the member and ``tols`` validation, the ABI check, and the sweep
launcher's argument checks (every refusal comes back as -1 before any HIP call)."""
import ctypes

import numpy as np
import pytest

from gadmm_amd.algorithms import chain_admm, logistic_admm_sweep
from gadmm_amd.data import logistic_synthetic
from gadmm_amd.models import LogisticRegression
from gadmm_amd.ops import native


@pytest.fixture(scope="module")
def log6():
    ds = logistic_synthetic(6)
    return LogisticRegression(ds.X, ds.y, lam=1e-5)


def test_sweep_on_cpu_is_the_loop_of_chain_admm(log6):
    members = [3e-4, (2e-4, 20, 1e-3), (2e-4, 100, 1e-4)]
    got = logistic_admm_sweep(log6, list(range(6)), 6, members, 0.0, 1e-4, 12, step=2.2)
    assert len(got) == 3
    for g, mem in zip(got, [(3e-4, 100, 1e-4)] + members[1:]):
        r = chain_admm(log6, list(range(6)), 6, mem[0], 0.0, 1e-4, 12, local_solver="gd", step=2.2, max_inner=mem[1],
                       inner_tol=mem[2])
        assert g.iters == r.iters and g.converged == r.converged and np.array_equal(g.obj, r.obj)
        assert g.extra["sweep_fallback"] == "cpu tensors" and "sweep" not in g.extra
    assert not np.array_equal(got[1].obj, got[2].obj)  # (the order is checked on results that differ)
    assert logistic_admm_sweep(log6, list(range(6)), 6, [], 0.0, 1e-4, 12) == []


@pytest.mark.parametrize("bad", [(2e-4, 100), (2e-4, 0, 1e-4), (2e-4, 2.5, 1e-4), (2e-4, 10, -1.0), (2e-4, 10, 1e-4, 1)])
def test_member_tuples_and_tols_are_validated(log6, bad):
    with pytest.raises(ValueError, match="logistic sweep member"):
        logistic_admm_sweep(log6, list(range(6)), 6, [2e-4, bad], 0.0, 1e-4, 12)
    with pytest.raises(ValueError, match="tols"):
        logistic_admm_sweep(log6, list(range(6)), 6, [2e-4, 3e-4], 0.0, 1e-4, 12, tols=[1e-4])


def test_capacity_is_eight_and_the_abi_check_catches_a_moved_layout():
    lib = native.require()
    assert lib.gadmm_chain_persistent_logistic_sweep_capacity() == 8
    native.check_logi_sweep_abi(lib)

    class Stub:  # a library built from a header in which LogiArgs grew by a field
        @staticmethod
        def gadmm_logi_sweep_abi_layout(buf, n):
            vals = native.logi_sweep_abi_expected()
            vals[0] += 8
            vals[4] += 8
            buf[:len(vals)] = vals
            return len(vals)
    with pytest.raises(RuntimeError, match="LogiSweepArgs layout mismatch"):
        native.check_logi_sweep_abi(Stub)


# ---- launcher validation: the batches name buffers by made-up addresses, so none may ever reach a launch:
# the LAST entry of every batch keeps an iteration-tag range that its own last check refuses, and each case
# adds ONE defect that an earlier check must name.
_P_BUFS = ("slots", "pos", "theta", "mu", "thg", "objg", "decg", "dec_push", "trace", "tstamp", "rres", "ctl", "xchk")
_WRITTEN = tuple(b for b in _P_BUFS if b not in ("slots", "pos"))


def _batch(nb, d=50, m=50, n=6):
    batch = (native.LogiSweepArgs * max(nb, 1))()
    for j in range(nb):
        p, g = batch[j].p, batch[j].g
        p.d, p.n, p.n_local, p.nranks, p.has_monitor = d, n, n, 1, 1
        p.start_iter, p.max_iter, p.lag, p.ring = 1, 200, 4, 8
        p.rho, p.tol, p.timeout_ticks = 2e-4, 1e-4, 10 ** 8
        for k, name in enumerate(_P_BUFS):
            setattr(p, name, 0x10000000 + 0x100000 * j + 0x1000 * (k + 1))
        g.X, g.Y, g.m, g.max_inner = 0x40000000, 0x50000000, m, 100  # (the shards are shared)
        g.lam, g.step, g.inner_tol = 1e-5, 2.2, 1e-4
        g.inner_iters = 0x60000000 + 0x1000 * j
    batch[max(nb, 1) - 1].p.max_iter = 1 << 20  # never launched, whatever else the case changes
    return batch


def _launch(batch, nb):
    lib = native.require()
    stage = (native.LogiSweepArgs * 8)()
    rc = lib.gadmm_chain_persistent_logistic_sweep_launch(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def test_launch_base_batch_is_refused_by_its_tag_range_only():
    for nb in (1, 3, 8):
        rc, msg = _launch(_batch(nb), nb)
        assert rc == -1 and "solve %d: ring/lag/tag range" % (nb - 1) in msg, msg
    for nb in (0, 9):
        rc, msg = _launch((native.LogiSweepArgs * 9)(), nb)
        assert rc == -1 and "one launch takes 1..8" in msg


@pytest.mark.parametrize("where,field,value,j,expect", [
    ("p", "sys_scope", 1, 0, "solve 0: one GPU, every worker local"),
    ("p", "n_epochs", 2, 1, "solve 1: one GPU, every worker local"),
    ("p", "nranks", 2, 0, "solve 0: one GPU, every worker local"),
    ("p", "has_monitor", 0, 1, "solve 1: one GPU, every worker local"),
    ("p", "d", 65, 0, "solve 0: d=65, m=50 not eligible"),
    ("g", "m", 65, 1, "solve 1: d=50, m=65 not eligible"),
    ("g", "max_inner", 0, 1, "solve 1: max_inner must be >= 1"),
    ("g", "X", None, 0, "solve 0: a required buffer is null"),
    ("p", "xchk", None, 1, "solve 1 has no placement-check buffer (xchk)"),
    ("p", "ring", 5, 0, "solve 0: ring/lag/tag range"),
])
def test_launch_refuses_entry(where, field, value, j, expect):
    batch = _batch(3)
    setattr(getattr(batch[j], where), field, value)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and expect in msg, msg


def test_launch_refuses_too_many_workgroups_and_mixed_register_classes():
    batch = _batch(2, n=256)
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 0 has 257 workgroups, the placement check holds 256" in msg, msg
    batch = _batch(2)
    batch[0].g.m, batch[1].p.d = 52, 53
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "register class" in msg, msg
    batch = _batch(2)
    batch[0].p.d, batch[1].g.m = 53, 64  # one class: on to the last check
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 1: ring/lag/tag range" in msg, msg


@pytest.mark.parametrize("name", _WRITTEN + ("inner_iters",))
def test_launch_refuses_a_shared_written_buffer(name):
    batch = _batch(3)
    for j in (0, 1):
        setattr(batch[j].g if name == "inner_iters" else batch[j].p, name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "solves 0 and 1 share a buffer that both write" in msg, msg
