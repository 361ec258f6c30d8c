"""CQ-GADMM (censored Q-GADMM) on the GPU (csrc/kernels/chain_quant.hip, CENS = true; compiled in
chain_cquant.hip): the censored graph-engine phase kernel against the NumPy specification
(algorithms/quantize.py) bit for bit, the persistent censored kernel against the graph engine bit for
bit, both against the Q kernels under an all-zero threshold table, against the torch path where its
margins make the comparison meaningful, and the mixed sweep.

How far the counts of a censored run are determined by the specification is in the docstring of
tests/test_cqgadmm_cpu.py: the decisions of the first 80 iterations on the shipped data are (every
rounding of the local solve agrees on them), the iteration of the stop is not.

Run with: pytest -m gpu tests/test_gpu_cqgadmm.py
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
RHO = 3.0
CENSOR = (1.0, 0.9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu_sweep.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


_PROB = {}


def _problem(N, d):
    """(X (N, 50, d), y (N, 50), obj0) cut from linear_synthetic(N) by column slicing, shared. The data
    set has 50 columns: d > 50 appends seeded N(0, 1) / sqrt(50) columns."""
    if (N, d) not in _PROB:
        from gadmm_amd.data import linear_synthetic
        from gadmm_amd.oracle.reference import opt_linear
        ds = linear_synthetic(N)
        X = ds.X[:, :, :d]
        if d > X.shape[2]:
            extra = np.random.default_rng(64).standard_normal((N, X.shape[1], d - X.shape[2])) / np.sqrt(X.shape[1])
            X = torch.cat([X, torch.from_numpy(extra)], dim=2)
        X = X.contiguous()
        obj0 = opt_linear(X.reshape(-1, d).numpy(), ds.y.reshape(-1).numpy())
        _PROB[(N, d)] = (X, ds.y.contiguous(), float(obj0))
    return _PROB[(N, d)]


def _engine(N, d, bits, seed=1234, tol=1e-8, max_iter=120, xcd=2, censor=CENSOR):
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, obj0 = _problem(N, d)
    eng = NativeChainEngine(X.to(DEV), y.to(DEV), list(range(N)), N, "linear", rho=RHO, obj0=obj0, tol=tol,
                            max_iter=max_iter, quant=(bits, seed), xcd=xcd, censor=censor)
    eng.set_path(list(range(N)), Placement.contiguous(N, 1), 0)
    return eng


def _model(N, d):
    from gadmm_amd.models.linear import LinearRegression
    X, y, obj0 = _problem(N, d)
    return LinearRegression(X.to(DEV), y.to(DEV)), obj0


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("N,d", [(3, 7), (8, 50), (4, 70), (3, 200)])
def test_censoring_exactness_one_phase(N, d, bits):
    """Iteration 1 (a head launch, then a tail launch) of the censored phase kernel from a random th_hat
    table and random duals, under a threshold taken from the specification's own ``s``: the midpoint of
    the two smallest ``s`` among the heads, so the head launch holds a censored and a sent worker (the
    tails solve after the heads; theirs follow from the kernel's own theta). The public rows, the header
    word of every message, the codes of the sent ones and ``c_sent`` equal the specification applied
    to the kernel's own theta, bit for bit."""
    from gadmm_amd.algorithms import quantize as Q
    eng = _engine(N, d, bits, seed=99, max_iter=8)
    rng = np.random.default_rng(1000 * N + d + bits)
    th0 = torch.from_numpy(rng.standard_normal((N, d)))
    mu0 = torch.from_numpy(rng.standard_normal((N, d)) * 0.1)
    heads, tails = list(range(0, N, 2)), list(range(1, N, 2))

    def one_iteration(thr2):
        eng.reset()
        with torch.cuda.stream(eng.stream):
            eng.theta.copy_(th0)
            eng.mu.copy_(mu0)
            eng.q_msg.zero_()
            eng.c_thr2.fill_(thr2)
        r = eng.run(stop_iter=1, use_graph=False)
        assert r.iters == 1
        return (eng.theta.cpu().numpy(), eng.theta_true.cpu().numpy(), eng.q_msg.cpu().numpy().view(np.uint64),
                eng.sent_trace(1)[0])

    table0 = th0.numpy()
    _, true_a, _, sent_a = one_iteration(0.0)  # a zero threshold: everybody sends
    assert sent_a.all()
    cand = Q.quantize_rows(true_a[heads], table0[heads], bits, Q.u01(99, 1, N, heads, d))[2]
    s_heads = np.sort(Q.censor_rows(cand, table0[heads], 0.0)[1])
    assert s_heads[0] < s_heads[1]
    thr2 = 0.5 * (s_heads[0] + s_heads[1])
    hat1, true1, msg, sent = one_iteration(thr2)
    assert np.array_equal(true1[heads], true_a[heads])  # the heads solve before anything is censored
    n_sent = n_cens = 0
    for ws in (heads, tails):  # a tail decides against its own row, which the head launch left alone
        R, q, new, _ = Q.quantize_rows(true1[ws], table0[ws], bits, Q.u01(99, 1, N, ws, d))
        send, s, margin = Q.censor_rows(new, table0[ws], thr2)
        print("N=%d d=%d b=%d %s: s/thr2 %s" % (N, d, bits, "heads" if ws is heads else "tails", (s / thr2).round(3)))
        assert margin > 1e-9  # the reference's own decisions are not at a rounding's mercy
        assert np.array_equal(sent[ws], send)
        assert np.array_equal(hat1[ws], np.where(send[:, None], new, table0[ws]))
        for k, w in enumerate(ws):
            if send[k]:
                assert msg[w, 0] == R[k:k + 1].view(np.uint64)[0]
                assert np.array_equal(msg[w, 1:], Q.pack_codes(q[k], bits))
            else:  # the censored notice alone: no code word written
                assert int(msg[w, 0]) == Q.CENSORED_HEADER and not msg[w, 1:].any()
        n_sent += int(send.sum())
        n_cens += int((~send).sum())
        if ws is heads:
            assert send.any() and not send.all()
    assert n_sent >= 1 and n_cens >= 1
    assert np.isfinite(eng.objective_trace(1)[0])
    eng.close()


@pytest.mark.parametrize("N,d", [(3, 7), (8, 50), (3, 64), (4, 70), (3, 200)])
def test_censoring_sum_bit_for_bit(N, d):
    """The kernels' ``s`` is the specification's ``sum64`` to the last bit (the order of the butterfly
    and of the chunks): with the threshold of iteration 1 at exactly the specification's ``s`` of one head
    that head sends, and at the next float above it is censored. Phase kernel at every d; persistent
    kernel (one wave per worker) at d <= 64, from the same random table."""
    from gadmm_amd.algorithms import quantize as Q
    bits = 8
    eng = _engine(N, d, bits, seed=99, max_iter=8)
    rng = np.random.default_rng(77 * N + d)
    th0 = torch.from_numpy(rng.standard_normal((N, d)))
    mu0 = torch.from_numpy(rng.standard_normal((N, d)) * 0.1)
    heads = list(range(0, N, 2))

    def first_iteration(thr2, persistent):
        eng.reset()
        with torch.cuda.stream(eng.stream):
            eng.theta.copy_(th0)
            eng.mu.copy_(mu0)
            eng.c_thr2.zero_()
            eng.c_thr2[1] = thr2
        if persistent:
            r = eng.run_persistent(fetch_trace=True)
            assert r.done != 4
        else:
            eng.run(stop_iter=1, use_graph=False)
        return eng.theta_true.cpu().numpy(), eng.sent_trace(1)[0]

    true1, sent = first_iteration(0.0, False)
    assert sent.all()
    cand = Q.quantize_rows(true1[heads], th0.numpy()[heads], bits, Q.u01(99, 1, N, heads, d))[2]
    s = Q.censor_rows(cand, th0.numpy()[heads], 0.0)[1]
    k = int(np.argmax(s))  # the head with the largest s: at its threshold the other heads are censored
    w, s_w = heads[k], float(s[k])
    assert s_w > 0.0
    for persistent in ((False, True) if d <= 64 else (False,)):
        _, at = first_iteration(s_w, persistent)
        _, above = first_iteration(float(np.nextafter(s_w, np.inf)), persistent)
        print("N=%d d=%d %s: s=%s sent at s %s, above s %s" % (N, d, "persistent" if persistent else "phase", s_w.hex(),
                                                                 at[heads], above[heads]))
        assert at[w] and not above[w]
        assert not at[[h for h in heads if h != w]].any()
    eng.close()


_GRAPH = {}


def _graph_ref(N, d, bits, tol=1e-8, max_iter=120, stop_iter=0, censor=CENSOR):
    """(done, iters, trace, th_hat, true theta, mu, sent trace) of the graph engine, once per key."""
    key = (N, d, bits, tol, max_iter, stop_iter, censor)
    if key not in _GRAPH:
        eng = _engine(N, d, bits, tol=tol, max_iter=max_iter, censor=censor)
        eng.reset()
        r = eng.run(stop_iter=stop_iter)
        assert eng.graph_ok()
        tr = eng.objective_trace(r.iters).copy()
        tr.setflags(write=False)
        sent = eng.sent_trace(r.iters) if censor is not None else None
        _GRAPH[key] = (r.done, r.iters, tr, eng.theta.cpu(), eng.theta_true.cpu(), eng.mu.cpu(), sent)
        eng.close()
    return _GRAPH[key]


@pytest.mark.parametrize("N", [2, 3, 8])
@pytest.mark.parametrize("d", [1, 7, 50, 64])
def test_engines_agree(N, d):
    """persistent-CQ == graph-CQ bit for bit at (tau0, xi) = (1, 0.9), max_iter = 120, XCD packing on
    (placement verified) and off: iterations, objective trace, the sent trace, and th_hat / true theta /
    duals after the persistent kernel's last iteration (it learns the decision `lag` iterations late; the
    graph engine is run that far on a longer buffer). d = 1: a single code granule; d = 64: the 53..64
    register class; N = 2: a chain with no interior worker. done != 4: the hand-off never timed out."""
    for bits in ((4, 8, 16) if (N, d) == (3, 50) else (8,)):
        done, iters, tr, _, _, _, sent = _graph_ref(N, d, bits)
        assert done in (1, 2) and iters >= 10
        assert sent.shape == (iters, N)
        assert sent.any() and not sent.all()  # censoring is at work in every case
        if (N, d) == (8, 50):  # an iteration in which everybody sends, and one in which nobody does
            assert sent.all(axis=1).any() and (~sent.any(axis=1)).any()
        if (N, d) == (2, 50):
            assert (~sent.any(axis=1)).sum() >= 10
        for xcd in (2, 0):
            eng = _engine(N, d, bits, xcd=xcd)
            assert eng.persistent_q_eligible()
            eng.reset()
            r = eng.run_persistent(fetch_trace=True)
            print("N=%d d=%d b=%d xcd=%d: done=%d iters=%d placed=%d %s sent %d of %d" % (
                N, d, bits, xcd, r.done, r.iters, eng.last_placed, eng.last_kernel, sent.sum(), sent.size))
            assert r.done != 4
            assert eng.last_kernel == "persistent-CQ(b=%d,G=%d)" % (bits, -(-d * bits // 64) + 1)
            assert eng.last_placed == xcd
            assert (r.done, r.iters) == (done, iters)
            assert np.array_equal(eng.objective_trace(r.iters), tr)
            assert np.array_equal(eng.sent_trace(r.iters), sent)
            last = eng.ctl_state()["iter"] - 1
            assert iters <= last <= iters + 16
            _, it_g, tr_g, hat_g, true_g, mu_g, sent_g = _graph_ref(N, d, bits, tol=0.0, max_iter=136, stop_iter=last)
            assert it_g == last and np.array_equal(tr_g[:iters], tr)
            k = min(last, 120)  # (the kernel records the rows below max_iter)
            assert np.array_equal(eng.sent_trace(k), sent_g[:k])
            assert torch.equal(eng.theta.cpu(), hat_g)
            assert torch.equal(eng.theta_true.cpu(), true_g)
            # the kernel leaves the heads' last dual pending, like the graph engine before its flush
            assert torch.equal(eng.mu.cpu(), mu_g)
            eng.close()


def test_zero_threshold_is_q_gadmm():
    """tau0 = 0 on the censored kernels == the Q kernels bit for bit, graph and persistent (N = 8, d = 50)."""
    N, d, bits = 8, 50, 8
    ref = _graph_ref(N, d, bits, max_iter=200, censor=None)
    got = _graph_ref(N, d, bits, max_iter=200, censor=(0.0, 0.9))
    assert ref[1] == got[1] == 93 and ref[0] == got[0] == 1
    assert np.array_equal(ref[2], got[2])
    for a, b in zip(ref[3:6], got[3:6]):
        assert torch.equal(a, b)
    assert got[6].all()
    for censor in (None, (0.0, 0.9)):  # each persistent kernel == the graph-Q engine run as far as it ran
        eng = _engine(N, d, bits, max_iter=200, censor=censor)
        eng.reset()
        r = eng.run_persistent(fetch_trace=True)
        assert r.done == 1 and r.iters == 93
        assert eng.last_kernel.startswith("persistent-CQ(" if censor else "persistent-Q(")
        assert np.array_equal(eng.objective_trace(93), ref[2])
        last = eng.ctl_state()["iter"] - 1
        q_ref = _graph_ref(N, d, bits, tol=0.0, max_iter=200, stop_iter=last, censor=None)
        assert q_ref[1] == last
        assert torch.equal(eng.theta.cpu(), q_ref[3]) and torch.equal(eng.theta_true.cpu(), q_ref[4])
        assert torch.equal(eng.mu.cpu(), q_ref[5])
        if censor:
            assert eng.sent_trace(last).all()
        eng.close()


@pytest.mark.parametrize("N", [2, 3, 8])
def test_against_the_torch_path(N):
    """The first 40 iterations at d = 50, b = 8, (1, 0.9), seeds 1234 and 2, against the torch path. First
    conditions on the reference alone: its smallest flip margin is >= 1e-10 and its smallest censor
    margin >= 1e-9 (on the CPU they are >= 5e-10 and >= 1.9e-3 on these cases; the seeds were chosen for
    that), far above the engines' rounding differences: no code flips, no decision flips, the sent traces
    are equal and the objective traces agree at rtol 1e-11."""
    from gadmm_amd.algorithms import censored_quantized_group_admm
    from gadmm_amd.models.linear import LinearRegression
    X, y, obj0 = _problem(N, 50)
    cpu = LinearRegression(X, y)
    gpu, _ = _model(N, 50)
    for seed in (1234, 2):
        ref = censored_quantized_group_admm(cpu, RHO, obj0, 1e-30, 40, 8, CENSOR[0], CENSOR[1], seed=seed)
        fm, cm = ref.extra["min_flip_margin"], ref.extra["min_censor_margin"]
        print("N=%d seed=%d: min flip margin %.3g min censor margin %.3g" % (N, seed, fm, cm))
        assert ref.iters == 40 and fm >= 1e-10 and cm >= 1e-9
        for persistent in (True, False):
            r = censored_quantized_group_admm(gpu, RHO, obj0, 1e-30, 40, 8, CENSOR[0], CENSOR[1], seed=seed,
                                              backend="native", engine_opts={"persistent": persistent, "cache": False})
            ex = r.extra
            assert "quant_fallback" not in ex
            if persistent:
                assert ex["engine"] == "persistent" and ex["kernel"].startswith("persistent-CQ")
                assert ex["engine_obj"].ctl_state()["done"] != 4
            else:
                assert ex["kernel"] == "graph-CQ" and ex["engine"] == "graph"
            rel = np.max(np.abs(r.obj - ref.obj) / np.abs(ref.obj))
            print("   %s: max rel diff %.3g, %d transmissions" % (ex["kernel"], rel, ex["transmissions"]))
            assert r.iters == 40 and np.array_equal(ex["sent_trace"], ref.extra["sent_trace"])
            assert np.allclose(r.obj, ref.obj, rtol=1e-11, atol=0.0)
            assert ex["transmissions"] == ref.extra["transmissions"] and np.array_equal(r.comm_units, ref.comm_units)
            ex["engine_obj"].close()


@pytest.mark.parametrize("N,censor,cum,own", [(8, (1.0, 0.9), (76, 134, 195, 261), (117, 385)),
                                              (24, (1.0, 0.98), (191, 368, 547, 718), (1339, 15845))])
def test_counts(N, censor, cum, own):
    """d = 50, b = 8, seed 1234 to 1e-8 on both native engines. Pinned from the independent prototype:
    the cumulative transmissions after 20 / 40 / 60 / 80 iterations, on which every rounding of the local
    solve agrees (tests/test_cqgadmm_cpu.py). The counts at the stop (``own``) are those of the kernels'
    arithmetic, the same on both engines bit for bit and in every run; other roundings of the same
    specification stop elsewhere (N = 8: the kernels 117 / 385, an earlier prototype 140 / 461, the torch
    path 150 / 493, NumPy solves 166 / 544 and 171 / 559; N = 24 to 1e-8: an earlier prototype
    1344 / 16220, the torch path 1340 / 15955, the kernels 1339 / 15845). Well under 60 % of the workers x iterations transmit."""
    from gadmm_amd.algorithms import censored_quantized_group_admm
    from gadmm_amd.algorithms.quantize import granules_per_row
    gpu, obj0 = _model(N, 50)
    G = granules_per_row(50, 8)
    res = []
    for persistent in (True, False):
        r = censored_quantized_group_admm(gpu, RHO, obj0, 1e-8, 3000, 8, censor[0], censor[1], seed=1234,
                                          engine_opts={"persistent": persistent, "cache": False})
        ex = r.extra
        tx, tr = ex["transmissions"], ex["sent_trace"]
        print("N=%d %s: iters %d transmissions %d (%.1f %%) gap/tol %.4f" % (
            N, ex["kernel"], r.iters, tx, 100.0 * tx / (r.iters * N), r.loss[-1] / 1e-8))
        assert ex["backend"] == "native" and ex["kernel"].startswith("persistent-CQ" if persistent else "graph-CQ")
        if persistent:
            assert ex["engine"] == "persistent" and ex["engine_obj"].ctl_state()["done"] != 4
        assert r.converged and len(r.obj) == r.iters and tr.shape == (r.iters, N)
        assert tuple(int(tr[:k].sum()) for k in (20, 40, 60, 80)) == cum
        assert tx + ex["censored"] == r.iters * N and int(tr.sum()) == tx
        assert tx < 0.6 * r.iters * N
        assert ex["payload_bits"] == tx * (8 * 50 + 64) and r.comm_units[-1] == tx * (8 * 50 + 64) / (64.0 * 50)
        assert ex["q_granules"] == G and ex["q_wire_bytes"] == tx * G * 16 + ex["censored"] * 16
        res.append((r.iters, tx, r.obj.copy(), tr.copy()))
        ex["engine_obj"].close()
    assert res[0][:2] == res[1][:2] and np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])
    assert res[0][:2] == own


def test_dispatch(monkeypatch):
    """Through the public call: d = 70 runs graph-CQ; ``state=`` takes the torch path, says why and still
    censors; a CU budget below N + 1 sends the d <= 64 case to graph-CQ with the persistent kernel's
    trace and sent trace; ``backend='native'`` refuses what the native path does not cover."""
    from gadmm_amd.algorithms import censored_quantized_group_admm as cq
    gpu70, obj70 = _model(4, 70)
    r = cq(gpu70, RHO, obj70, 1e-6, 60, 8, 1.0, 0.9, engine_opts={"cache": False})
    assert r.extra["backend"] == "native" and r.extra["kernel"] == "graph-CQ" and r.extra["engine"] == "graph"
    assert r.iters >= 10 and np.all(np.isfinite(r.obj))
    assert r.extra["sent_trace"].any() and not r.extra["sent_trace"].all()
    r.extra["engine_obj"].close()

    gpu, obj0 = _model(8, 50)
    st = (torch.zeros((8, 50), dtype=torch.float64, device=DEV), torch.zeros((8, 50), dtype=torch.float64, device=DEV), 1)
    t = cq(gpu, RHO, obj0, 1e-30, 40, 8, 1.0, 0.9, state=st)
    assert t.extra["backend"] == "torch" and t.extra["quant_fallback"] == "state= (resume)"
    assert tuple(int(t.extra["sent_trace"][:k].sum()) for k in (20, 40)) == (76, 134) and t.extra["min_censor_margin"] > 0
    with pytest.raises(RuntimeError, match="does not cover this case"):
        cq(gpu, RHO, obj0, 1e-30, 40, 8, 1.0, 0.9, state=st, backend="native")

    p = cq(gpu, RHO, obj0, 1e-8, 500, 8, 1.0, 0.9, engine_opts={"cache": False})
    assert p.extra["engine"] == "persistent" and p.extra["kernel"].startswith("persistent-CQ") and p.iters == 117
    p.extra["engine_obj"].close()
    monkeypatch.setenv("GADMM_CU_BUDGET", "2")  # 2 CUs x (at most 4 one-wave workgroups) < N + 1 = 9
    g = cq(gpu, RHO, obj0, 1e-8, 500, 8, 1.0, 0.9, engine_opts={"cache": False})
    assert g.extra["kernel"] == "graph-CQ" and g.extra["engine"].startswith("graph")
    assert g.iters == 117 and np.array_equal(g.obj, p.obj)
    assert np.array_equal(g.extra["sent_trace"], p.extra["sent_trace"]) and g.extra["transmissions"] == 385
    g.extra["engine_obj"].close()


@pytest.mark.parametrize("N,d", [(3, 7), (8, 50), (3, 50), (8, 7)])
def test_sweep_mixed_members(N, d):
    """Eight members, (rho, bits, seed) next to (rho, bits, seed, tau0, xi), in one launch of the censored
    sweep kernel: every member equals its own single solve bit for bit, sent trace included, and the
    uncensored ones equal ``quantized_group_admm``."""
    from gadmm_amd.algorithms import chain_admm, quantized_group_admm, quantized_group_admm_sweep
    gpu, obj0 = _model(N, d)
    configs = [(3.0, 8, 1234), (3.0, 8, 1234, 1.0, 0.9), (5.0, 4, 7, 0.5, 0.95), (3.0, 16, 1234), (7.0, 8, 3, 1.0, 0.98),
               (5.0, 8, 7), (3.0, 4, 5, 2.0, 0.9), (3.0, 16, 9, 1.0, 0.9)]
    got = quantized_group_admm_sweep(gpu, configs, obj0, 1e-6, 150, engine_opts={"cache": False})
    for j, (g, c) in enumerate(zip(got, configs)):
        cen = tuple(c[3:]) if len(c) == 5 else None
        assert "sweep_fallback" not in g.extra
        assert g.extra["sweep"]["kernel"] == "persistent-CQ-sweep(K=8)" and g.extra["sweep"]["slot"] == j
        s = chain_admm(gpu, list(range(N)), N, c[0], obj0, 1e-6, 150, quantize=(c[1], c[2]), censor=cen,
                       engine_opts={"cache": False})
        assert s.extra["kernel"].startswith("persistent-CQ(" if cen else "persistent-Q(")
        print("N=%d d=%d member %d %s: iters %d / %d" % (N, d, j, c, g.iters, s.iters))
        assert (g.iters, g.converged) == (s.iters, s.converged) and np.array_equal(g.obj, s.obj)
        assert np.array_equal(g.comm_units, s.comm_units)
        if cen is not None:
            assert np.array_equal(g.extra["sent_trace"], s.extra["sent_trace"])
            for k in ("transmissions", "censored", "payload_bits", "q_wire_bytes"):
                assert g.extra[k] == s.extra[k]
        else:
            assert "sent_trace" not in g.extra
            q = quantized_group_admm(gpu, c[0], obj0, 1e-6, 150, c[1], seed=c[2], engine_opts={"cache": False})
            assert q.iters == g.iters and np.array_equal(q.obj, g.obj) and np.array_equal(q.comm_units, g.comm_units)
            q.extra["engine_obj"].close()
        s.extra["engine_obj"].close()
    for g in got:
        g.extra["engine_obj"].close()


def test_sweep_of_three_element_members_keeps_the_q_kernel():
    from gadmm_amd.algorithms import quantized_group_admm_sweep
    gpu, obj0 = _model(8, 50)
    got = quantized_group_admm_sweep(gpu, [(3.0, 8, 1234), (5.0, 4, 7)], obj0, 1e-4, 200, engine_opts={"cache": False})
    assert got[0].iters == 55
    for g in got:
        assert g.extra["sweep"]["kernel"] == "persistent-Q-sweep(K=2)" and "sent_trace" not in g.extra
        g.extra["engine_obj"].close()


def test_entry_writes_cq_runs(tmp_path):
    """E1 ``--quick --set quant_bits=8 censor=1,0.98`` on the GPU: the CQ-GADMM runs next to the Q runs,
    on the native kernels, with fewer comm units than their Q runs at the stop."""
    out = str(tmp_path / "e1")
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Synthetic", "--quick", "--no-plot", "--no-baselines",
           "--out", out, "--set", "quant_bits=8", "censor=1,0.98"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    runs = json.load(open(os.path.join(out, "summary.json")))["runs"]
    for rho in (3, 5, 7):
        cq, q = runs["CQ-GADMM_b8_rho%d" % rho], runs["Q-GADMM_b8_rho%d" % rho]
        print("rho=%d: Q %d iters %.1f units; CQ %d iters %.1f units, %d transmissions" % (
            rho, q["iters"], q["comm_units"], cq["iters"], cq["comm_units"], cq["transmissions"]))
        assert cq["algorithm"] == "CQ-GADMM(b=8,rho=%d)" % rho and cq["backend"] == "native"
        assert cq["kernel"].startswith("persistent-CQ") and "quant_fallback" not in cq
        assert cq["transmissions"] + cq["censored"] == cq["iters"] * 24
        assert cq["comm_units"] < q["comm_units"]
