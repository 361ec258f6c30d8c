"""CQ-GADMM (censored Q-GADMM) on the CPU: the censoring specification (algorithms/quantize.py) against
known answers, the torch path of ``chain_admm(..., quantize=, censor=)``, its accounting, the dispatch
and the ABI of the censor fields.

The known answers of the specification are worked out by hand (the docstrings say how) or come from an
independent NumPy prototype (tools/cqgadmm_prototype.py: plain Python floats, its own butterfly sum, its
own threshold products; its outputs are tests/golden/cqgadmm_prototype.json); they are not re-pinned
from this code.

How far a censored run is determined by the specification. A stochastic quantizer amplifies the
rounding of the local solve once a flip margin is down at that level, and under censoring one flipped
code moves ``s`` by about 1 / 2^bits of itself, more than the censor margins of these runs (about
2e-3): from there on two correct implementations take different decisions and the runs part for
good. On the shipped data (b = 8, seed 1234, rho = 3) the prototype's flip margin falls below 1e-11
around iteration 96 at N = 8, and its two variants -- local solves by ``numpy.linalg.solve`` and by a
product with the explicit inverse -- agree on every decision of the first 80 iterations and then
stop in

    N = 8,  (1, 0.9),  1e-8:  166 iterations / 544 transmissions  and  171 / 559
    N = 24, (1, 0.98), 1e-4:  760 / 6711  and  759 / 6694

where an earlier prototype had 140 / 461 and 760 / 6713 and the torch path (batched Cholesky
solves) has 150 / 493 and 756 / 6657. So the counts to the stop are a property of one implementation's
rounding, not of the specification: what is pinned from the prototype here are the transmissions of the
first 80 iterations, on which every variant agrees, and the torch path's own counts to the stop are
pinned as a regression check of that one code path.
"""
import ctypes

import numpy as np
import pytest
import torch

from gadmm_amd.algorithms import quantize as Q
from gadmm_amd.algorithms import (chain_admm, censored_quantized_group_admm, quantized_group_admm,
                                  quantized_group_admm_sweep)
from gadmm_amd.ops import native

THETA = np.array([0.5, -0.25, 0.125, 1.0])
HAT = np.array([0.0, 0.25, 0.125, 0.0])
# the b = 8 public model of tests/test_qgadmm_cpu.py (KNOWN[8]): quantize_row(THETA, HAT, 8, u(1234, 1, 8, 0))
CAND8 = np.array([float.fromhex(h) for h in
                  ["0x1.fdfdfdfdfdfe0p-2", "-0x1.fbfbfbfbfbfc0p-3", "0x1.0808080808080p-3", "0x1p+0"]])


def test_sum64_order_known_answers():
    """v = [1, 2^-53, 0, 2^-53, 0, ...]: the butterfly meets lanes 1 and 3 first (off = 2: 2^-53 + 2^-53
    = 2^-52) and then adds that to 1: 1 + 2^-52; left to right every 2^-53 is a tie that rounds back to
    1. A second chunk (d = 70, 2^-53 at index 64) is added to the first chunk's result afterwards:
    (1 + 2^-52) + 2^-53 is a tie whose even neighbour is 1 + 2^-51."""
    e = 2.0 ** -53
    v = np.zeros(50)
    v[0], v[1], v[3] = 1.0, e, e
    left_to_right = 0.0
    for x in v:
        left_to_right += x
    assert left_to_right == 1.0
    assert float(Q.sum64(v)) == float.fromhex("0x1.0000000000001p+0")
    v2 = np.zeros(70)
    v2[:50] = v
    v2[64] = e
    assert float(Q.sum64(v2)) == float.fromhex("0x1.0000000000002p+0")
    assert float(Q.sum64(np.zeros(7))) == 0.0 and float(Q.sum64(np.array([3.5]))) == 3.5
    both = Q.sum64(np.stack([v, np.zeros(50)]))  # rows
    assert both.shape == (2,) and both[0] == float.fromhex("0x1.0000000000001p+0") and both[1] == 0.0
    # 256 ones and a tie in the last chunk: four chunks in order
    w = np.ones(256)
    assert float(Q.sum64(w)) == 256.0


def test_censor_thresholds_known_answers():
    t, thr = 1.0, []
    for _ in range(6):
        thr.append(t)
        t = t * 0.98
    got = Q.censor_thresholds(1.0, 0.98, 5)
    assert got.shape == (6,) and got.tolist() == [x * x for x in thr]
    assert got[0] == 1.0 and got[1] == 0.98 * 0.98
    # the table is the repeated product, which is not the power
    long = Q.censor_thresholds(1.0, 0.98, 400)
    assert long[400] != (0.98 ** 400) ** 2 and abs(long[400] / (0.98 ** 400) ** 2 - 1.0) < 1e-12
    assert np.all(Q.censor_thresholds(0.0, 0.5, 9) == 0.0)
    for bad in ((-1.0, 0.5), (1.0, 0.0), (1.0, 1.0), (1.0, 1.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError):
            Q.censor_thresholds(bad[0], bad[1], 3)


def test_censor_rows_known_answers():
    """Row 0: the b = 8 candidate of the Q test against HAT. d = 4, so the butterfly is
    (sq0 + sq2) + (sq1 + sq3) with sq_i = (cand_i - hat_i)^2, in plain Python floats below; it is about
    1.496 >= 1: sent. Row 1: the candidate moves one coordinate by 2^-10: s = 2^-20 < 1, censored."""
    st = [float(c) - float(h) for c, h in zip(CAND8, HAT)]
    sq = [x * x for x in st]
    s0 = (sq[0] + sq[2]) + (sq[1] + sq[3])
    assert s0 == float.fromhex("0x1.7f00820385068p+0")  # the prototype's bits
    assert ((sq[0] + sq[1]) + sq[2]) + sq[3] == float.fromhex("0x1.7f00820385069p+0")  # left to right: one ulp off
    cand = np.stack([CAND8, HAT + np.array([0.0, 0.0, 2.0 ** -10, 0.0])])
    hat = np.stack([HAT, HAT])
    send, s, margin = Q.censor_rows(cand, hat, 1.0)
    assert send.tolist() == [True, False]
    assert s.tolist() == [s0, 2.0 ** -20]
    assert margin == min(abs(s0 - 1.0), abs(2.0 ** -20 - 1.0))
    # one threshold per row; thr2 = 0 always sends (also at R = 0, s = 0) and has no margin
    send, s, margin = Q.censor_rows(cand, hat, np.array([2.0, 2.0 ** -20]))
    assert send.tolist() == [False, True] and margin == 0.0
    send, s, margin = Q.censor_rows(hat, hat, 0.0)
    assert send.tolist() == [True, True] and s.tolist() == [0.0, 0.0] and margin == float("inf")
    send, _, _ = Q.censor_rows(hat, hat, 1e-300)  # R == 0: censored whenever thr2 > 0
    assert send.tolist() == [False, False]


@pytest.fixture(scope="module")
def lin8():
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models.linear import LinearRegression
    from gadmm_amd.oracle.reference import opt_linear
    ds = linear_synthetic(8)
    Xf, yf = ds.stacked()
    return LinearRegression(ds.X, ds.y), opt_linear(Xf.numpy(), yf.numpy())


@pytest.fixture(scope="module")
def lin24m(lin24, lin_obj0):
    from gadmm_amd.models.linear import LinearRegression
    return LinearRegression(lin24.X, lin24.y), lin_obj0


def test_tau0_zero_is_q_gadmm(lin8):
    m, obj0 = lin8
    q = chain_admm(m, list(range(8)), 8, 3.0, obj0, 1e-8, 500, quantize=(8, 1234))
    c = chain_admm(m, list(range(8)), 8, 3.0, obj0, 1e-8, 500, quantize=(8, 1234), censor=(0.0, 0.9))
    assert q.iters == c.iters == 93
    assert np.array_equal(q.obj, c.obj)
    assert torch.equal(q.extra["state"][0], c.extra["state"][0]) and torch.equal(q.extra["state"][1], c.extra["state"][1])
    assert torch.equal(q.extra["theta_true"], c.extra["theta_true"])
    assert c.extra["transmissions"] == 93 * 8 and c.extra["censored"] == 0 and c.extra["sent_trace"].all()
    assert np.array_equal(q.comm_units, c.comm_units) and q.extra["payload_bits"] == c.extra["payload_bits"]
    assert c.extra["min_censor_margin"] == float("inf")
    assert "transmissions" not in q.extra and "sent_trace" not in q.extra


def _check_accounting(r, N, d, bits):
    ex = r.extra
    pb = bits * d + 64
    assert ex["transmissions"] + ex["censored"] == r.iters * N
    assert ex["sent_trace"].shape == (r.iters, N) and ex["sent_trace"].dtype == bool
    assert int(ex["sent_trace"].sum()) == ex["transmissions"]
    assert ex["payload_bits"] == ex["transmissions"] * pb
    assert r.comm_units.shape == (r.iters,)
    assert r.comm_units[-1] == ex["transmissions"] * pb / (64.0 * d)
    assert np.array_equal(r.comm_units, np.cumsum(ex["sent_trace"].sum(axis=1)) * pb / (64.0 * d))


@pytest.mark.parametrize("N,censor,cum", [(8, (1.0, 0.9), (76, 134, 195, 261)), (24, (1.0, 0.98), (191, 368, 547, 718))])
def test_first_80_iterations_match_the_prototype(lin8, lin24m, N, censor, cum):
    """b = 8, seed 1234, rho = 3 on the shipped data: cumulative transmissions after 20 / 40 / 60 / 80
    iterations, equal in both variants of the prototype (module docstring); its flip margins there are
    >= 3e-11 and its censor margins >= 1.5e-3, far above any solve's rounding."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cqgadmm_prototype.json")) as f:
        gold = {c["N"]: c for c in json.load(f)["cases"]}[N]
    assert tuple(gold["censor"]) == censor and tuple(gold["cumulative_transmissions_20_40_60_80"]) == cum
    m, obj0 = lin8 if N == 8 else lin24m
    r = chain_admm(m, list(range(N)), N, 3.0, obj0, 0.0, 80, quantize=(8, 1234), censor=censor)
    tr = r.extra["sent_trace"]
    print("N=%d: flip margin %.3g censor margin %.3g" % (N, r.extra["min_flip_margin"], r.extra["min_censor_margin"]))
    assert r.iters == 80 and not r.converged
    assert tuple(int(tr[:k].sum()) for k in (20, 40, 60, 80)) == cum
    assert r.extra["min_censor_margin"] >= 1e-3 and r.extra["min_flip_margin"] >= 1e-11
    _check_accounting(r, N, m.d, 8)
    if N == 8:  # the trace holds an iteration in which everybody sends and one in which nobody does
        assert tr.all(axis=1).sum() == 2 == gold["iterations_everybody_sends"]
        assert (~tr.any(axis=1)).sum() == 1 == gold["iterations_nobody_sends"]


@pytest.mark.parametrize("N,censor,tol,iters,tx", [(8, (1.0, 0.9), 1e-8, 150, 493), (24, (1.0, 0.98), 1e-4, 756, 6657)])
def test_torch_path_counts(lin8, lin24m, N, censor, tol, iters, tx):
    """The torch path's own counts to the stop (an earlier prototype: 140 / 461 and 760 / 6713; why they
    differ, and by how much other roundings of the same specification differ, is in the module
    docstring). Fewer than half of the workers x iterations transmit."""
    m, obj0 = lin8 if N == 8 else lin24m
    r = censored_quantized_group_admm(m, 3.0, obj0, tol, 3000, 8, censor[0], censor[1], seed=1234)
    ex = r.extra
    print("N=%d tol=%g: iters %d transmissions %d censored %d censor margin %.3g flip margin %.3g" % (
        N, tol, r.iters, ex["transmissions"], ex["censored"], ex["min_censor_margin"], ex["min_flip_margin"]))
    assert r.converged and r.loss[-1] < tol <= r.loss[-2]
    assert (r.iters, ex["transmissions"]) == (iters, tx)
    assert ex["transmissions"] < 0.5 * r.iters * N
    assert r.algorithm == "CQ-GADMM(b=8)" and ex["censor"] == censor
    assert ex["quant_fallback"] == "cpu tensors" and ex["backend"] == "torch"
    assert 0.0 < ex["min_censor_margin"] < 1.0
    _check_accounting(r, N, m.d, 8)
    q = quantized_group_admm(m, 3.0, obj0, tol, 3000, 8, seed=1234)
    assert r.comm_units[-1] < q.comm_units[-1]  # fewer transmissions outweigh the extra iterations


def test_validation(lin8):
    m, obj0 = lin8
    ids = list(range(8))
    with pytest.raises(ValueError, match="needs quantize"):
        chain_admm(m, ids, 8, 3.0, obj0, 1e-4, 10, censor=(1.0, 0.9))
    for bad in ((1.0, 0.0), (1.0, 1.0), (1.0, -0.5), (1.0, 1.5), (-1.0, 0.9), (1.0,), (1.0, 0.9, 0.5)):
        with pytest.raises(ValueError):
            chain_admm(m, ids, 8, 3.0, obj0, 1e-4, 10, quantize=(8, 1234), censor=bad)
    with pytest.raises(ValueError):
        quantized_group_admm_sweep(m, [(3.0, 8, 1234, 1.0)], obj0, 1e-4, 10)
    with pytest.raises(ValueError):
        quantized_group_admm_sweep(m, [(3.0, 8, 1234, 1.0, 1.0)], obj0, 1e-4, 10)
    with pytest.raises(RuntimeError, match="cpu tensors"):  # no quiet fall-back when the native backend is asked for
        chain_admm(m, ids, 8, 3.0, obj0, 1e-4, 10, quantize=(8, 1234), censor=(1.0, 0.9), backend="native")


def test_sweep_on_cpu_is_the_loop_of_chain_admm(lin8):
    """Five-element members next to three-element ones; each equals its own solve, and the uncensored
    ones are what they were."""
    m, obj0 = lin8
    configs = [(3.0, 8, 1234), (3.0, 8, 1234, 1.0, 0.9), (5.0, 4, 7, 0.5, 0.95), (3.0, 16, 1234)]
    got = quantized_group_admm_sweep(m, configs, obj0, 1e-4, 500)
    assert got[0].iters == 55
    for g, c in zip(got, configs):
        cen = tuple(c[3:]) if len(c) == 5 else None
        r = chain_admm(m, list(range(8)), 8, c[0], obj0, 1e-4, 500, quantize=(c[1], c[2]), censor=cen)
        assert g.iters == r.iters and g.converged == r.converged
        assert np.array_equal(g.obj, r.obj) and np.array_equal(g.comm_units, r.comm_units)
        assert g.extra["sweep_fallback"] == "cpu tensors"
        assert ("sent_trace" in g.extra) == (cen is not None)
        if cen is not None:
            assert np.array_equal(g.extra["sent_trace"], r.extra["sent_trace"]) and g.extra["censor"] == cen
            _check_accounting(g, 8, m.d, c[1])


# ---- dispatch on a (pretended) device: which engine, which kernel, which groups
class _FakeMember:
    def __init__(self, censor):
        self.censor = censor
        self.asked = None
        self.last_kernel = None
        self._ctl_host = torch.zeros(8, dtype=torch.int32)

    def reset(self):
        pass

    def prepare_persistent_q(self, lag=4, timeout_s=20.0, censored=None):
        self.asked = censored
        return native.PersistArgs()

    def _queue_readback(self, fetch):
        return fetch

    def finish_persistent_q(self, wall_ms, fetch, what):
        return what


class _FakeLib:
    def __init__(self):
        self.calls = []

    def gadmm_chain_persistent_q_sweep_launch(self, batch, K, *a):
        self.calls.append(("q", K))
        return 0

    def gadmm_chain_persistent_cq_sweep_launch(self, batch, K, *a):
        self.calls.append(("cq", K))
        return 0


class _FakeStream:
    cuda_stream = 0

    def synchronize(self):
        pass


def _fake_sweep(censors):
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    sw = object.__new__(QuantSweepEngine)
    sw.members = [_FakeMember(c) for c in censors]
    sw.lib = _FakeLib()
    sw.stream = _FakeStream()
    sw._stage_host = sw._stage_dev = torch.zeros(1)
    return sw


def test_mixed_batch_runs_on_the_censored_kernel():
    """One censored member sends the whole batch to the censored sweep kernel, and every member is then
    prepared for it (an uncensored one brings an all-zero table); a batch of three-element members keeps
    today's kernel and its name."""
    sw = _fake_sweep([None, (1.0, 0.9), None])
    out = sw.run()
    assert sw.lib.calls == [("cq", 3)] and sw.last_kernel == "persistent-CQ-sweep(K=3)"
    assert [m.asked for m in sw.members] == [True, True, True]
    assert all(m.last_kernel == sw.last_kernel for m in sw.members) and len(out) == 3
    sw = _fake_sweep([None, None])
    sw.run()
    assert sw.lib.calls == [("q", 2)] and sw.last_kernel == "persistent-Q-sweep(K=2)"
    assert [m.asked for m in sw.members] == [False, False]


def test_eleven_members_run_as_eight_plus_three(lin8):
    """A mixed list longer than a launch is split into groups of eight in input order (``sweep_groups`` /
    ``run_in_groups``, as for three-element members), each member parsed to its (config, censor) pair."""
    from gadmm_amd.algorithms import gadmm as G
    m, obj0 = lin8
    configs = [(3.0 + i, 8, i) if i % 3 else (3.0 + i, 8, i, 1.0, 0.9) for i in range(11)]
    parsed = [G._sweep_member(c) for c in configs]
    assert [p[0] for p in parsed] == [(3.0 + i, 8, i) for i in range(11)]
    assert [p[1] for p in parsed] == [None if i % 3 else (1.0, 0.9) for i in range(11)]
    width = native.require().gadmm_chain_persistent_q_sweep_capacity()
    assert [list(g) for g in G.sweep_groups(len(configs), width)] == [list(range(8)), [8, 9, 10]]
    got = quantized_group_admm_sweep(m, configs, obj0, 1e-4, 5)  # here the loop; the results in input order
    assert [g.extra.get("censor") for g in got] == [p[1] for p in parsed]
    assert [g.extra["q_seed"] for g in got] == list(range(11))


# ---- launcher validation of the censored entry points: refused before any HIP call (no device here)
_BUFS = ("qg", "slots", "pos", "objg", "decg", "dec_push", "theta", "mu", "Minv", "A", "b", "yy", "ctl", "trace",
         "xchk", "q_true", "tstamp", "c_thr2", "c_sent")


def _entry(a, j, d=50, n=8):
    a.d, a.n, a.n_local, a.nranks, a.has_monitor = d, n, n, 1, 1
    a.start_iter, a.max_iter, a.lag, a.ring = 1, 200, 4, 8
    a.q_bits, a.q_seed = 8, 1234
    a.rho, a.tol, a.timeout_ticks = 3.0, 1e-8, 10 ** 8
    for k, name in enumerate(_BUFS):
        setattr(a, name, 0x10000000 + 0x100000 * j + 0x1000 * (k + 1))


def _batch(nb):
    batch = (native.PersistArgs * nb)()
    for j in range(nb):
        _entry(batch[j], j)
    batch[nb - 1].max_iter = 1 << 20  # never launched: the tag range is the launcher's last check
    return batch


def _launch(name, batch, nb):
    lib = native.require()
    stage = (native.PersistArgs * 8)()
    rc = getattr(lib, name)(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def test_censored_sweep_launcher_refusals():
    rc, msg = _launch("gadmm_chain_persistent_cq_sweep_launch", _batch(3), 3)
    assert rc == -1 and "persistent CQ sweep: solve 2: ring/lag/tag range" in msg, msg
    for name in ("c_thr2", "c_sent"):
        b = _batch(3)
        setattr(b[1], name, None)
        rc, msg = _launch("gadmm_chain_persistent_cq_sweep_launch", b, 3)
        assert rc == -1 and "solve 1: the censored kernel needs a threshold table (c_thr2) and a c_sent buffer" in msg, msg
        rc, msg = _launch("gadmm_chain_persistent_q_sweep_launch", b, 3)  # the Q launcher never looks at them
        assert rc == -1 and "persistent Q sweep: solve 2: ring/lag/tag range" in msg, msg
    b = _batch(3)
    b[0].c_sent = b[2].c_sent = 0x7fff0000
    rc, msg = _launch("gadmm_chain_persistent_cq_sweep_launch", b, 3)
    assert rc == -1 and "solves 0 and 2 share a buffer that both write" in msg, msg
    b = _batch(3)
    b[0].c_thr2 = b[1].c_thr2 = b[2].c_thr2 = 0x7fff0000  # a read-only table may be shared
    rc, msg = _launch("gadmm_chain_persistent_cq_sweep_launch", b, 3)
    assert rc == -1 and "solve 2: ring/lag/tag range" in msg, msg
    rc, msg = _launch("gadmm_chain_persistent_cq_sweep_launch", (native.PersistArgs * 9)(), 9)
    assert rc == -1 and "one launch takes 1..8" in msg
    # the single launch: the same entry check
    lib = native.require()
    a = native.PersistArgs()
    _entry(a, 0)
    a.c_thr2 = None
    assert lib.gadmm_chain_persistent_cq_launch(ctypes.byref(a), None) == -1
    assert "persistent CQ kernel: the censored kernel needs a threshold table" in lib.gadmm_last_error().decode()
    a.d = 65
    assert lib.gadmm_chain_persistent_cq_launch(ctypes.byref(a), None) == -1
    assert "d=65" in lib.gadmm_last_error().decode()
    assert lib.gadmm_chain_persistent_cq_capacity(ctypes.byref(a)) == 0


def test_censor_abi_layout_matches_ctypes():
    """The censor fields of PhaseArgs / PersistArgs sit where the native library has them: directly in
    front of the Q-GADMM fields, which stay the last four of both structs."""
    lib = native.require()
    buf = (ctypes.c_longlong * 8)()
    k = lib.gadmm_censor_abi_layout(buf, 8)
    PA, PS = native.PhaseArgs, native.PersistArgs
    assert list(buf[:k]) == [PA.c_thr2.offset, PA.c_sent.offset, ctypes.sizeof(PA),
                             PS.c_thr2.offset, PS.c_sent.offset, ctypes.sizeof(PS)]
    assert [n for n, _ in PA._fields_][-6:-4] == ["c_thr2", "c_sent"]
    assert [n for n, _ in PS._fields_][-6:-4] == ["c_thr2", "c_sent"]
    assert PA.rres.offset < PA.c_thr2.offset < PA.q_true.offset
    assert PS.ep_flush.offset < PS.c_thr2.offset < PS.qg.offset
    z = native.PersistArgs()  # zeroed: off
    assert z.c_thr2 is None and z.c_sent is None


def test_entry_adds_cq_runs(tmp_path):
    """``--set quant_bits=8 censor=1,0.98``: a CQ-GADMM run next to every Q run, sequential and through
    the batch call, with fewer comm units at the stop; the default adds none."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for tag, extra in (("seq", []), ("con", ["sweep=concurrent"])):
        out = str(tmp_path / tag)
        cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Synthetic", "--quick", "--device", "cpu",
               "--no-plot", "--no-baselines", "--out", out, "--set", "rhos=7", "quant_bits=8", "censor=1,0.98"] + extra
        p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        runs[tag] = json.load(open(os.path.join(out, "summary.json")))["runs"]
    for tag in ("seq", "con"):
        r = runs[tag]
        assert sorted(r) == ["CQ-GADMM_b8_rho7", "GADMM_rho7", "Q-GADMM_b8_rho7"]
        cq, q = r["CQ-GADMM_b8_rho7"], r["Q-GADMM_b8_rho7"]
        assert cq["algorithm"] == "CQ-GADMM(b=8,rho=7)" and cq["converged"] and q["converged"]
        assert cq["comm_units"] < q["comm_units"]
        assert cq["transmissions"] + cq["censored"] == cq["iters"] * 24
    for k in runs["seq"]:
        assert runs["con"][k]["iters"] == runs["seq"][k]["iters"]
    assert runs["con"]["CQ-GADMM_b8_rho7"]["sweep_fallback"] == "cpu tensors"
