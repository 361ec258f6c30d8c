"""Concurrent Q-GADMM sweep, the parts that need no device: the sequential fallback of
``quantized_group_admm_sweep``, the grouping of long config lists, the sweep launcher's argument
validation (every refusal comes back as -1 before any HIP call) and the entry switch on the CPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gadmm_amd.algorithms import chain_admm, quantized_group_admm_sweep
from gadmm_amd.algorithms.gadmm import run_in_groups, sweep_groups
from gadmm_amd.data import linear_synthetic
from gadmm_amd.models import LinearRegression
from gadmm_amd.ops import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lin8():
    ds = linear_synthetic(8)
    m = LinearRegression(ds.X, ds.y)
    return m, m.optimum()


def test_sweep_on_cpu_is_the_loop_of_chain_admm(lin8):
    m, obj0 = lin8
    configs = [(3.0, 8, 1234), (5.0, 4, 7), (3.0, 16, 1234)]
    got = quantized_group_admm_sweep(m, configs, obj0, 1e-4, 500)
    ref = [chain_admm(m, list(range(8)), 8, rho, obj0, 1e-4, 500, quantize=(bits, seed))
           for rho, bits, seed in configs]
    assert got[0].iters == 55  # N = 8, rho = 3, b = 8, seed 1234 to 1e-4 (tests/test_gpu_qgadmm.py::test_counts)
    for g, r, (rho, bits, seed) in zip(got, ref, configs):
        assert g.iters == r.iters and g.converged == r.converged
        assert np.array_equal(g.obj, r.obj)
        assert np.array_equal(g.comm_units, r.comm_units)
        assert (g.extra["q_bits"], g.extra["q_seed"]) == (bits, seed)
        assert g.extra["sweep_fallback"] == "cpu tensors"
        assert "sweep" not in g.extra


def test_sweep_tols_are_per_config(lin8):
    m, obj0 = lin8
    cfg = (3.0, 8, 1234)
    got = quantized_group_admm_sweep(m, [cfg, cfg], obj0, 1e-4, 500, tols=(1e-2, 1e-4))
    assert got[1].iters == 55 and got[0].iters < 55
    assert np.array_equal(got[0].obj, got[1].obj[:got[0].iters])
    with pytest.raises(ValueError):
        quantized_group_admm_sweep(m, [cfg, cfg], obj0, 1e-4, 500, tols=(1e-2,))
    assert quantized_group_admm_sweep(m, [], obj0, 1e-4, 500) == []


def test_sweep_capacity_is_eight():
    assert native.require().gadmm_chain_persistent_q_sweep_capacity() == 8


def test_eleven_configs_run_as_eight_plus_three_in_input_order():
    configs = [(float(11 - i), (4, 8, 16)[i % 3], i) for i in range(11)]  # not sorted: the order is the caller's
    width = native.require().gadmm_chain_persistent_q_sweep_capacity()
    assert [len(g) for g in sweep_groups(len(configs), width)] == [8, 3]
    seen = []

    def run_group(items, idx):
        seen.append((list(items), list(idx)))
        return [("solved", c) for c in items]

    out = run_in_groups(configs, width, run_group)
    assert [s[1] for s in seen] == [list(range(8)), [8, 9, 10]]
    assert seen[0][0] == configs[:8] and seen[1][0] == configs[8:]
    assert out == [("solved", c) for c in configs]


# ---- launcher validation: refused with -1 and a message before any HIP call (no device here).
# The batches below name buffers by made-up addresses, so none of them may ever reach a launch: the
# LAST entry of every batch keeps an iteration-tag range that the launcher refuses as its last check
# (start_iter + max_iter + lag >= 2^20), and each case adds ONE defect that an earlier check must
# name, so the message tells which check fired.
_BUFS = ("qg", "slots", "pos", "objg", "decg", "dec_push", "theta", "mu", "Minv", "A", "b", "yy", "ctl", "trace",
         "xchk", "q_true", "tstamp")


def _entry(a, j, d=50, n=8):
    a.d, a.n, a.n_local, a.nranks, a.has_monitor = d, n, n, 1, 1
    a.start_iter, a.max_iter, a.lag, a.ring = 1, 200, 4, 8
    a.q_bits, a.q_seed = 8, 1234
    a.rho, a.tol, a.timeout_ticks = 3.0, 1e-8, 10 ** 8
    for k, name in enumerate(_BUFS):
        setattr(a, name, 0x10000000 + 0x100000 * j + 0x1000 * (k + 1))


def _batch(nb, **kw):
    batch = (native.PersistArgs * max(nb, 1))()
    for j in range(nb):
        _entry(batch[j], j, **kw)
    batch[max(nb, 1) - 1].max_iter = 1 << 20  # never launched, whatever else the case changes
    return batch


def _launch(batch, nb):
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    rc = lib.gadmm_chain_persistent_q_sweep_launch(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def test_launch_base_batch_is_refused_by_its_tag_range_only():
    for nb in (1, 3, 8):
        rc, msg = _launch(_batch(nb), nb)
        assert rc == -1 and "solve %d: ring/lag/tag range" % (nb - 1) in msg, msg


@pytest.mark.parametrize("nb", [0, 9])
def test_launch_refuses_width(nb):
    rc, msg = _launch((native.PersistArgs * 9)(), nb)
    assert rc == -1 and "one launch takes 1..8" in msg


def test_launch_refuses_null_batch_or_staging():
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    batch = _batch(1)
    for args in ((None, 1, ctypes.addressof(stage), ctypes.addressof(stage)),
                 (batch, 1, None, ctypes.addressof(stage)), (batch, 1, ctypes.addressof(stage), None)):
        assert lib.gadmm_chain_persistent_q_sweep_launch(*args, None) == -1
        assert "null batch or staging" in lib.gadmm_last_error().decode()


def _set(name, value, j=0):
    def f(batch):
        setattr(batch[j], name, value)
    return f


def _n_not_local(batch):
    batch[1].n_local = 7


_ENTRY_CASES = {
    "null qg": (_set("qg", None), "solve 0: a required buffer is null"),
    "null theta": (_set("theta", None, 1), "solve 1: a required buffer is null"),
    "null ctl": (_set("ctl", None), "solve 0: a required buffer is null"),
    "null trace": (_set("trace", None, 1), "solve 1: a required buffer is null"),
    "null dec_push": (_set("dec_push", None), "solve 0: a required buffer is null"),
    "q_bits 5": (_set("q_bits", 5, 1), "solve 1: q_bits must be 4, 8 or 16, got 5"),
    "q_bits 0": (_set("q_bits", 0), "solve 0: q_bits must be 4, 8 or 16, got 0"),
    "d 65": (_set("d", 65), "different register classes"),
    "d 0": (_set("d", 0, 1), "solve 1: d=0"),
    "n_epochs": (_set("n_epochs", 1, 1), "solve 1: one GPU, every worker local, a static chain"),
    "nranks 2": (_set("nranks", 2), "solve 0: one GPU, every worker local, a static chain"),
    "sys_scope": (_set("sys_scope", 1), "solve 0: one GPU"),
    "push": (_set("push", 0x7000), "solve 0: one GPU"),
    "n_local != n": (_n_not_local, "solve 1: one GPU, every worker local"),
    "no monitor": (_set("has_monitor", 0, 1), "solve 1: one GPU"),
    "hard_stop": (_set("hard_stop", 50), "solve 0: one GPU"),
    "cont": (_set("cont", 1, 1), "solve 1: one GPU"),
    "ring <= lag + 1": (_set("ring", 5), "solve 0: ring/lag/tag range"),
    "lag 0": (_set("lag", 0), "solve 0: ring/lag/tag range"),
    "tag range": (_set("max_iter", 1 << 20), "solve 0: ring/lag/tag range"),
    "null xchk": (_set("xchk", None, 1), "solve 1 has no placement-check buffer (xchk)"),
}


@pytest.mark.parametrize("case", sorted(_ENTRY_CASES))
def test_launch_refuses_entry(case):
    mutate, expect = _ENTRY_CASES[case]
    batch = _batch(3)
    mutate(batch)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and expect in msg, msg


def test_launch_refuses_d_65_alone():
    batch = _batch(1, d=65)
    rc, msg = _launch(batch, 1)
    assert rc == -1 and "d=65" in msg and "not eligible" in msg


def test_launch_refuses_more_workgroups_than_the_placement_check_holds():
    batch = _batch(2, n=256)  # 257 workgroups, xchk holds 256 granules
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 0 has 257 workgroups, the placement check holds 256" in msg, msg


def test_launch_refuses_mixed_register_classes():
    batch = _batch(2)
    batch[0].d, batch[1].d = 52, 53
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "register class" in msg and "52" in msg and "53" in msg
    batch = _batch(2)
    batch[0].d, batch[1].d = 53, 64  # one class: on to the last check
    rc, msg = _launch(batch, 2)
    assert rc == -1 and "solve 1: ring/lag/tag range" in msg


@pytest.mark.parametrize("name", ["ctl", "trace", "theta", "mu", "qg", "q_true", "objg", "decg", "dec_push", "xchk",
                                  "tstamp", "rres"])
def test_launch_refuses_a_shared_written_buffer(name):
    batch = _batch(3)
    setattr(batch[0], name, 0x7fff0000)
    setattr(batch[2], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "solves 0 and 2 share a buffer that both write" in msg, msg


@pytest.mark.parametrize("name", ["A", "b", "yy", "Minv", "slots", "pos"])
def test_launch_lets_read_only_inputs_be_shared(name):
    batch = _batch(3)
    for j in range(3):
        setattr(batch[j], name, 0x7fff0000)
    rc, msg = _launch(batch, 3)
    assert rc == -1 and "solve 2: ring/lag/tag range" in msg, msg  # nothing before the last check objected


# ---- the entry switch on the CPU: the same runs, through the sweep call's sequential fallback
def _entry_summary(tmp_path, name, extra):
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Synthetic", "--quick", "--device", "cpu", "--no-plot",
           "--no-baselines", "--out", out, "--set"] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.load(open(os.path.join(out, "summary.json")))["runs"]


def test_entry_concurrent_switch_on_cpu(tmp_path):
    seq = _entry_summary(tmp_path, "seq", ["quant_bits=8"])
    con = _entry_summary(tmp_path, "con", ["sweep=concurrent", "quant_bits=8"])
    assert sorted(con) == sorted(seq)
    qkeys = [k for k in seq if k.startswith("Q-GADMM_b8_rho")]
    assert len(qkeys) == 3
    for k in seq:
        assert con[k]["iters"] == seq[k]["iters"] and con[k]["converged"] == seq[k]["converged"]
    for k in qkeys:
        assert con[k]["algorithm"] == seq[k]["algorithm"]
        assert con[k]["sweep_fallback"] == "cpu tensors"
        assert "sweep_fallback" not in seq[k]
