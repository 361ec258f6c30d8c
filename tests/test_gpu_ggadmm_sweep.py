"""Concurrent GGADMM / Q-GGADMM solves in one launch of the persistent graph kernels' bodies
(engine/graph_sweep.py: up to eight solves, one per XCD) on the MI355X.

Yardstick: a separately built single ``NativeGraphEngine`` run of the same member, bit for bit, over
``(done, iters)``, the objective trace, ``theta``, ``mu``, ``rres``, ``ctl_state()["iter"]`` and, for
Q-GGADMM, ``theta_true`` and ``q_msg``. The single kernel shares the sweep's body, so it is not the only
reference: the mixed launch is also held to the long-double reference of tests/hp_ggadmm.py with the
comparison of tests/test_gpu_ggadmm.py::test_native_against_long_double_reference, the workload launch to
the pinned iteration counts, and a chain-graph Q member to the chain Q sweep (engine/quant_sweep.py).

Shapes are hp_ggadmm.CASES, the smallest at which each thing can break. Every run has ``timeout_s=5``. No
test provokes a timeout, a fault or a hang.

Run with: pytest -m gpu tests/test_gpu_ggadmm_sweep.py -s
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hp_ggadmm as G
import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = H.K_ITERS
TIMEOUT = 5.0
PINNED_1E4 = {"chain": 784, "ring": 246, "grid:4x6": 106, "star:0": 91, "kbip": 156}  # N = 24, rho = 3, tol 1e-4


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu_ggadmm.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


_DATA = {}


def _data(name):
    """``(graph, X, y, rho, obj0)`` of a case, on the device, shared. Names outside hp_ggadmm.CASES:
    ``star20-d7`` (degree 19: the 32-wide class of the unquantized kernel) and ``edge-d64``."""
    if name not in _DATA:
        from gadmm_amd.models import LinearRegression
        from gadmm_amd.parallel.topology import chain_graph, star_graph
        if name == "star20-d7":
            g = star_graph(20, 0)
            X, y, rho = H.make_linear(20, 12, 7, H.seed_of(20, 12, 7) + 7919 * len(g.edges))
        elif name == "edge-d64":
            g = chain_graph(2)
            X, y, rho = H.make_linear(2, 70, 64, H.seed_of(2, 70, 64) + 7919)
        else:
            g, X, y, rho = G.case_data(name)
        X, y = _dev(X), _dev(y)
        _DATA[name] = (g, X, y, float(rho), float(LinearRegression(X, y).optimum()))
    return _DATA[name]


def _engine(name, rho=None, tol=0.0, max_iter=K, obj0=None, quant=None, xcd=2):
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, X, y, rho0, opt = _data(name)
    return NativeGraphEngine(X, y, g, rho0 if rho is None else rho, opt if obj0 is None else obj0, tol, max_iter,
                             quant=quant, xcd=xcd)


def _snap(eng, r):
    """What a member is compared on, as host arrays."""
    out = {"done_iters": (int(r.done), int(r.iters)), "trace": eng.traces(r.iters)[0].copy(),
           "theta": _host(eng.theta), "mu": _host(eng.mu), "rres": _host(eng.rres), "ctl_iter": eng.ctl_state()["iter"]}
    if eng.quant is not None:
        out["theta_true"] = _host(eng.theta_true)
        out["q_msg"] = _host(eng.q_msg)
    return out


def _assert_same(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        same = a[k] == b[k] if isinstance(a[k], (tuple, int)) else np.array_equal(a[k], b[k])
        assert same, "%s: %s differs from the single solve" % (what, k)


_SINGLE = {}


def _single(name, **kw):
    """The single solve of a member (its own engine, its own launch), computed once per configuration."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _SINGLE:
        eng = _engine(name, **kw)
        assert eng.eligible(), eng.refusal()
        r = eng.run(timeout_s=TIMEOUT)
        s = _snap(eng, r)
        s["kernel"] = eng.last_kernel
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SINGLE[key] = s
        eng.close()
    return {k: v for k, v in _SINGLE[key].items() if k != "kernel"}


def _xcc_ids(xchk):
    """XCC_IDs the blocks of a member's last launch posted (decoded as tests/test_gpu_qsweep.py::_xcc_ids)."""
    g = xchk.view(-1, 4).cpu().numpy().astype(np.int64) & 0xffffffff
    tag = int(g[0][0])
    ids = []
    for t, lo, t2, hi in g:
        if not (tag & 0x80000000) or t != tag or t2 != t:
            break
        ids.append(float(np.array([(int(hi) << 32) | int(lo)], dtype=np.uint64).view(np.float64)[0]))
    return ids


def _sweep_of(members):
    """``members``: ``[(name, kwargs of _engine), ...]``, separately built."""
    from gadmm_amd.engine.graph_sweep import GraphSweepEngine
    return GraphSweepEngine([_engine(name, **kw) for name, kw in members])


def _run_and_compare(members, quantized=False):
    sw = _sweep_of(members)
    runs = sw.run(timeout_s=TIMEOUT)
    assert sw.last_kernel == "persistent-graph-%ssweep(K=%d)" % ("Q-" if quantized else "", len(members))
    assert sw.blocks() == [_data(name)[0].n + 1 for name, _ in members]
    snaps = []
    for j, ((name, kw), m, r) in enumerate(zip(members, sw.members, runs)):
        print("slot %d %s %s: done=%d iters=%d placed=%d" % (j, name, kw, r.done, r.iters, sw.last_placed[j]))
        s = _snap(m, r)
        _assert_same(s, _single(name, **kw), "slot %d (%s)" % (j, name))
        assert sw.last_placed[j] == 2 and m.last_placed == 2
        ids = _xcc_ids(m._xchk)
        assert len(ids) == m.n + 1 and len(set(ids)) == 1, (j, ids)
        snaps.append(s)
    return sw, runs, snaps


# ------------------------------------------------------------------------------------------------
MIXED = ["edge-d1", "edge-d50", "ring4-d7", "grid2x3-d50", "k23-d52", "star12hub5-d50", "grid4x6-d50"]


def test_mixed_slots_class_13():
    """K = 8, QT = 13: widths 3 to 25 blocks side by side (the narrow slots' surplus blocks must leave
    before the placement check), degree classes 2, 4 and 16 in one launch, d from 1 to 52. Every member
    equals its single solve and lies within the bounds of its long-double reference (theta, dual, objective,
    K4 rows; the eighth member, ring4-d7 at another rho, has no such reference and is held to its single
    solve and to differing from the third)."""
    rho2 = 1.5 * _data("ring4-d7")[3]
    members = [(name, {}) for name in MIXED] + [("ring4-d7", {"rho": rho2})]
    sw, runs, snaps = _run_and_compare(members)
    assert [_single(n)["ctl_iter"] for n in MIXED] == [s["ctl_iter"] for s in snaps[:7]]
    assert {_SINGLE[(n,)]["kernel"] for n in MIXED} == {"persistent-graph(deg<=2)", "persistent-graph(deg<=4)",
                                                        "persistent-graph(deg<=16)"}
    for name, m, r, s in zip(MIXED, sw.members, runs, snaps):
        last = s["ctl_iter"] - 1
        assert r.done == 2 and r.iters == K and K <= last <= K + G.OVERRUN, (name, r.iters, r.done, last)
        ref = G.case(name, last)[4]
        rows = s["rres"][:K]
        tails = ref.tails[:K]
        assert np.all(rows[~tails] == 0.0), "a head's K4 row is not 0"
        assert np.all(np.isfinite(rows[tails])) and np.all(rows[tails] > 0)
        ratios = {"theta": ref.err_theta(s["theta"], last) / ref.b_theta, "dual": ref.err_dual(s["mu"]) / ref.b_dual,
                  "objective": ref.err_obj(s["trace"]) / ref.b_obj,
                  "residual rows": ref.err_res_w(rows) / ref.b_res_w}
        print("ggadmm sweep %s (last=%d): err/bound %s" % (name, last, " ".join("%s %.3f" % kv for kv in ratios.items())))
        bad = {k: v for k, v in ratios.items() if not v <= 1.0}
        assert not bad, (name, bad)
    assert not np.array_equal(snaps[2]["trace"], snaps[7]["trace"])
    sw.close()


def test_class_32_next_to_class_2():
    """A star of 20 (degree 19: the 32-wide poll group) beside a ring and an edge (classes 2): every slot
    runs the body of its own class."""
    members = [("star20-d7", {}), ("ring4-d7", {}), ("edge-d1", {})]
    sw, _, _ = _run_and_compare(members)
    assert [_SINGLE[(n,)]["kernel"] for n, _ in members] == ["persistent-graph(deg<=32)", "persistent-graph(deg<=2)",
                                                             "persistent-graph(deg<=2)"]
    sw.close()


def test_class_16_registers():
    """QT = 16 (d = 53..64): K(4, 4) at 53, a star of 8 at 64, one edge at 64. A d = 50 member next to a
    d = 53 member is refused before any launch."""
    sw, _, _ = _run_and_compare([("k44-d53", {}), ("star8-d64", {}), ("edge-d64", {})])
    sw.close()
    with pytest.raises(ValueError, match="register classes"):
        _sweep_of([("grid2x3-d50", {}), ("k44-d53", {})])


def test_width_one():
    sw, _, _ = _run_and_compare([("grid2x3-d50", {"tol": 1e-8, "max_iter": 3000})])
    assert sw.last_placed == [2]
    sw.close()


def _build(name, members, tols=1e-8, max_iters=3000, xcd=2):
    from gadmm_amd.engine.graph_sweep import GraphSweepEngine
    g, X, y, rho, obj0 = _data(name)
    return GraphSweepEngine.build(X, y, [(g,) + tuple(m) for m in members], obj0=obj0, tols=tols, max_iters=max_iters,
                                  xcd=xcd)


def test_width_eight_one_problem():
    """K = 8 on one problem through ``build`` (one Gram, one inverse launch): eight rho of which two are
    identical. Every member equals its single solve, the twins agree, different rho differ (a slot reading
    another slot's arguments is caught), every member sits on ONE XCD and the eight on eight different ones."""
    rho = _data("grid2x3-d50")[3]
    rhos = [rho * f for f in (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 1.0, 3.0)]
    sw = _build("grid2x3-d50", [(r,) for r in rhos])
    runs = sw.run(timeout_s=TIMEOUT)
    assert sw.last_kernel == "persistent-graph-sweep(K=8)"
    snaps, seen = [], []
    for j, (r, m, run) in enumerate(zip(rhos, sw.members, runs)):
        assert run.done == 1
        s = _snap(m, run)
        _assert_same(s, _single("grid2x3-d50", rho=r, tol=1e-8, max_iter=3000), "slot %d" % j)
        assert sw.last_placed[j] == 2
        ids = _xcc_ids(m._xchk)
        assert len(ids) == 7 and len(set(ids)) == 1, ids
        seen.append(ids[0])
        snaps.append(s)
    assert len(set(seen)) == 8, seen
    _assert_same(snaps[2], snaps[6], "the twins")
    for i in range(8):
        for j in range(i + 1, 8):
            if (i, j) != (2, 6):
                n = min(len(snaps[i]["trace"]), len(snaps[j]["trace"]))
                assert not np.array_equal(snaps[i]["trace"][:n], snaps[j]["trace"][:n]), (i, j)
    sw.close()


def test_different_stops_in_one_launch():
    """tol 1e-4, tol 1e-8 and a cap of 20 iterations at tol 1e-30 side by side: each member has its single
    solve's (done, iters) and bits, so the early finishers do not disturb the late one."""
    rho = _data("grid2x3-d50")[3]
    tols, caps = [1e-4, 1e-8, 1e-30], [3000, 3000, 20]
    sw = _build("grid2x3-d50", [(rho,)] * 3, tols=tols, max_iters=caps)
    runs = sw.run(timeout_s=TIMEOUT)
    assert [r.done for r in runs] == [1, 1, 2] and runs[2].iters == 20 and runs[0].iters < runs[1].iters
    for j, (m, r, tol, cap) in enumerate(zip(sw.members, runs, tols, caps)):
        _assert_same(_snap(m, r), _single("grid2x3-d50", rho=rho, tol=tol, max_iter=cap), "slot %d" % j)
    sw.close()


def test_packed_without_the_placement_check():
    """xcd = 1 at K = 3 (packed, sc1 stores): placed == 1 and the same bits as with xcd = 2."""
    rho = _data("grid2x3-d50")[3]
    got = {}
    for xcd in (1, 2):
        sw = _build("grid2x3-d50", [(rho,), (2 * rho,), (3 * rho,)], xcd=xcd)
        runs = sw.run(timeout_s=TIMEOUT)
        assert sw.last_placed == [xcd] * 3
        got[xcd] = [_snap(m, r) for m, r in zip(sw.members, runs)]
        sw.close()
    for a, b in zip(got[1], got[2]):
        _assert_same(a, b, "xcd 1 against 2")


def test_second_run_on_a_cached_sweep_engine():
    """``reset`` + ``run`` twice: equal results (a fresh tag salt per launch: the un-zeroed tables never match)."""
    rho = _data("star12hub5-d50")[3]
    sw = _build("star12hub5-d50", [(rho,), (2 * rho,)])
    out = []
    for _ in range(2):
        sw.reset()
        runs = sw.run(timeout_s=TIMEOUT)
        out.append([_snap(m, r) for m, r in zip(sw.members, runs)])
    for a, b in zip(out[0], out[1]):
        assert a["done_iters"][0] == 1
        _assert_same(a, b, "second run")
    _assert_same(out[1][0], _single("star12hub5-d50", rho=rho, tol=1e-8, max_iter=3000), "second run, slot 0")
    sw.close()


def test_refusals_before_any_launch(monkeypatch):
    """A star of 40 (41 workgroups in one slot, an XCD has 32 CUs) is refused with ``ResidencyError`` and
    ``graph_admm_sweep`` is then the loop; two members that share a written buffer are refused; a CU budget
    too small for the group makes the algorithm the loop."""
    from gadmm_amd.algorithms import graph_admm_sweep
    from gadmm_amd.engine.chain_engine import ResidencyError
    from gadmm_amd.models import LinearRegression
    sw = _sweep_of([("star40-d7", {}), ("ring4-d7", {})])
    with pytest.raises(ResidencyError, match="41 workgroups"):
        sw.run(timeout_s=TIMEOUT)
    sw.close()
    g, X, y, rho, obj0 = _data("star40-d7")
    m40 = LinearRegression(X, y)
    got = graph_admm_sweep(m40, [(g, rho), (g, 2 * rho)], obj0, 1e-6, 500, engine_opts={"timeout_s": TIMEOUT})
    assert all(r.extra["sweep_fallback"].startswith("ResidencyError") for r in got)
    assert all(r.extra["backend"] == "native" and r.extra["kernel"] == "persistent-graph(deg<=64)" for r in got)

    sw = _sweep_of([("ring4-d7", {}), ("ring4-d7", {})])
    sw.members[1].mu = sw.members[0].mu
    with pytest.raises(ValueError, match="solves 0 and 1 share a buffer that both write"):
        sw.run(timeout_s=TIMEOUT)
    sw.close()

    g, X, y, rho, obj0 = _data("ring4-d7")
    m4 = LinearRegression(X, y)
    monkeypatch.setenv("GADMM_CU_BUDGET", "2")  # 2 CUs hold one solve's 5 one-wave workgroups, not the group's 10
    low = graph_admm_sweep(m4, [(g, rho), (g, 2 * rho)], obj0, 1e-8, 500,
                           engine_opts={"cache": False, "timeout_s": TIMEOUT})
    assert all(r.extra["sweep_fallback"].startswith("ResidencyError") and "sweep" not in r.extra for r in low)
    assert all(r.extra["kernel"] == "persistent-graph(deg<=2)" for r in low)


def test_workload_shape():
    """E1 data, N = 24, d = 50, rho = 3, to 1e-4: the five graphs of the topology entry in one launch, 25
    workgroups each, the pinned iteration counts, each equal to its single solve."""
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    from gadmm_amd.engine.graph_sweep import GraphSweepEngine
    from gadmm_amd.oracle.reference import opt_linear
    from gadmm_amd.parallel.topology import parse_graph
    ds = linear_synthetic(24)
    Xf, yf = ds.stacked()
    obj0 = float(opt_linear(Xf.numpy(), yf.numpy()))
    X, y = ds.X.to(DEV), ds.y.to(DEV)
    graphs = [parse_graph(spec, 24) for spec in PINNED_1E4]
    sw = GraphSweepEngine.build(X, y, [(g, 3.0) for g in graphs], obj0=obj0, tols=1e-4, max_iters=3000)
    runs = sw.run(timeout_s=TIMEOUT)
    assert sw.blocks() == [25] * 5 and sw.last_placed == [2] * 5
    assert [(r.done, r.iters) for r in runs] == [(1, it) for it in PINNED_1E4.values()]
    for spec, g, m, r in zip(PINNED_1E4, graphs, sw.members, runs):
        one = NativeGraphEngine(X, y, g, 3.0, obj0, 1e-4, 3000)
        _assert_same(_snap(m, r), _snap(one, one.run(timeout_s=TIMEOUT)), spec)
        one.close()
    sw.close()


# ---- Q-GGADMM ------------------------------------------------------------------------------------
def test_q_width_eight_one_problem():
    """bits {4, 8, 16} x seeds {1, 2} and twins of (8, 7) on one problem: each member equals its single Q
    run including the last message words and the true iterates, the twins agree, different seeds differ."""
    rho = _data("grid2x3-d50")[3]
    cfgs = [(bits, seed) for bits in (4, 8, 16) for seed in (1, 2)] + [(8, 7), (8, 7)]
    sw = _build("grid2x3-d50", [(rho, b, s) for b, s in cfgs], tols=1e-6, max_iters=1000)
    runs = sw.run(timeout_s=TIMEOUT)
    assert sw.last_kernel == "persistent-graph-Q-sweep(K=8)" and sw.last_placed == [2] * 8
    snaps = []
    for j, (q, m, r) in enumerate(zip(cfgs, sw.members, runs)):
        print("slot %d b=%d seed=%d: done=%d iters=%d" % (j, q[0], q[1], r.done, r.iters))
        s = _snap(m, r)
        _assert_same(s, _single("grid2x3-d50", rho=rho, tol=1e-6, max_iter=1000, quant=q), "slot %d" % j)
        snaps.append(s)
    _assert_same(snaps[6], snaps[7], "the twins")
    for i in range(7):
        for j in range(i + 1, 7):
            assert not np.array_equal(snaps[i]["trace"][:20], snaps[j]["trace"][:20]), (i, j)
    sw.close()


def test_q_mixed_graphs():
    """Degree classes 2 / 4 / 16 of the Q kernel in one launch at b = 8."""
    kw = {"tol": 1e-6, "max_iter": 1000, "quant": (8, 1234)}
    sw, runs, _ = _run_and_compare([("ring4-d7", kw), ("k23-d52", kw), ("star12hub5-d50", kw)], quantized=True)
    assert [_SINGLE[("ring4-d7",) + tuple(sorted(kw.items()))]["kernel"],
            _SINGLE[("k23-d52",) + tuple(sorted(kw.items()))]["kernel"],
            _SINGLE[("star12hub5-d50",) + tuple(sorted(kw.items()))]["kernel"]] == [
        "persistent-graph-Q(deg<=2,b=8)", "persistent-graph-Q(deg<=4,b=8)", "persistent-graph-Q(deg<=16,b=8)"]
    sw.close()


def test_q_chain_graph_member_equals_the_chain_q_sweep():
    """E1 data, N = 8, rho = 3, (8, 1234) and (4, 7): a chain-graph member of the graph Q sweep against the same
    config's member of ``QuantSweepEngine`` -- iterations, objective trace, public models and true iterates
    bit for bit (the chain kernels keep a head's last dual pending, so the duals are not compared)."""
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.engine.graph_sweep import GraphSweepEngine
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    from gadmm_amd.oracle.reference import opt_linear
    from gadmm_amd.parallel.topology import chain_graph
    ds = linear_synthetic(8)
    Xf, yf = ds.stacked()
    obj0 = float(opt_linear(Xf.numpy(), yf.numpy()))
    X, y = ds.X.to(DEV), ds.y.to(DEV)
    cfgs = [(3.0, 8, 1234), (3.0, 4, 7)]
    gs = GraphSweepEngine.build(X, y, [(chain_graph(8),) + c for c in cfgs], obj0=obj0, tols=1e-8, max_iters=200)
    cs = QuantSweepEngine.build(X, y, list(range(8)), 8, cfgs, obj0=obj0, tols=1e-8, max_iters=200)
    gr, cr = gs.run(timeout_s=TIMEOUT), cs.run(timeout_s=TIMEOUT)
    for a, b, ra, rb in zip(gs.members, cs.members, gr, cr):
        assert (ra.done, ra.iters) == (rb.done, rb.iters)
        assert np.array_equal(a.traces(ra.iters)[0], b.traces(rb.iters)[0])
        assert torch.equal(a.theta.cpu(), b.theta.cpu()) and torch.equal(a.theta_true.cpu(), b.theta_true.cpu())
    assert (gr[0].done, gr[0].iters) == (1, 93)  # the chain Q kernels' count (tests/test_gpu_qsweep.py)
    gs.close()
    cs.close()


# ---- algorithm and entry -------------------------------------------------------------------------
def _same_results(got, ref):
    for g, r in zip(got, ref):
        assert g.iters == r.iters and g.converged == r.converged
        assert np.array_equal(g.obj, r.obj) and np.array_equal(g.comm_units, r.comm_units)
        assert np.array_equal(g.primal_res, r.primal_res)
        assert g.extra["graph"] == r.extra["graph"] and g.extra["deliveries"] == r.extra["deliveries"]
        assert ("q_bits" in g.extra) == ("q_bits" in r.extra)
        if "q_bits" in r.extra:
            for k in ("payload_bits", "q_granules", "q_wire_bytes", "q_bits", "q_seed", "transmissions"):
                assert g.extra[k] == r.extra[k], k
            assert torch.equal(g.extra["theta_true"].cpu(), r.extra["theta_true"].cpu())


def test_algorithm_results():
    """``graph_admm_sweep`` == the loop of ``graph_admm`` on the device; ten members run as 8 + 2; a mixed
    plain / quantized list keeps its order."""
    from gadmm_amd.algorithms import graph_admm, graph_admm_sweep
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.parallel.topology import complete_bipartite_graph, grid_graph, ring_graph
    g, X, y, rho, obj0 = _data("grid2x3-d50")
    model = LinearRegression(X, y)
    ring, kb = ring_graph(6), complete_bipartite_graph(3, 3)
    opts = {"timeout_s": TIMEOUT}

    def loop(members):
        out = []
        for mem in members:
            r = graph_admm(model, mem[0], mem[1], obj0, 1e-6, 1000, backend="native", engine_opts=opts,
                           quantize=None if len(mem) == 2 else (mem[2], mem[3]))
            assert r.extra["kernel"].startswith("persistent-graph")
            out.append(r)
        return out

    plain = [(gr, rho * f) for gr in (g, ring, kb) for f in (1.0, 2.0, 0.5)] + [(g, 3 * rho)]
    assert len(plain) == 10
    got = graph_admm_sweep(model, plain, obj0, 1e-6, 1000, engine_opts=opts)
    _same_results(got, loop(plain))
    for j, r in enumerate(got):
        sx = r.extra["sweep"]
        width, slot = (8, j) if j < 8 else (2, j - 8)
        assert "sweep_fallback" not in r.extra and "state" not in r.extra
        assert (sx["width"], sx["slot"], sx["placed"]) == (width, slot, 2)
        assert sx["kernel"] == r.extra["kernel"] == r.extra["sweep_kernel"] == "persistent-graph-sweep(K=%d)" % width
        assert r.extra["sweep_slot"] == slot and len(r.time_trace) == r.iters and r.wall_s > 0

    mixed = [(ring, rho, 8, 7), (g, rho), (g, rho, 4, 1), (kb, 2 * rho), (ring, rho, 8, 8)]
    got = graph_admm_sweep(model, mixed, obj0, 1e-6, 1000, engine_opts=opts)
    _same_results(got, loop(mixed))
    assert [r.extra["kernel"] for r in got] == ["persistent-graph-Q-sweep(K=3)", "persistent-graph-sweep(K=2)",
                                                "persistent-graph-Q-sweep(K=3)", "persistent-graph-sweep(K=2)",
                                                "persistent-graph-Q-sweep(K=3)"]
    assert [r.extra["sweep"]["slot"] for r in got] == [0, 0, 1, 1, 2]


def _entry_summary(tmp_path, name, extra):
    """One entry run in a fresh child process under its own time limit; a failed run fails the test before
    anything else is started."""
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "gadmm_amd", "LinearRegression_Topologies", "--quick", "--no-plot", "--out", out,
           "--set", "quant_bits=8"] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.load(open(os.path.join(out, "summary.json")))["runs"]


def test_entry_concurrent_switch(tmp_path):
    seq = _entry_summary(tmp_path, "seq", [])
    con = _entry_summary(tmp_path, "con", ["sweep=concurrent"])
    assert sorted(con) == sorted(seq)
    plain = [k for k in seq if k.startswith("GGADMM_")]
    quant = [k for k in seq if k.startswith("Q-GGADMM_b8_")]
    assert len(plain) >= 2 and len(quant) == len(plain) and len(seq) == 2 * len(plain)
    for keys, kernel in ((plain, "persistent-graph-sweep(K=%d)"), (quant, "persistent-graph-Q-sweep(K=%d)")):
        for j, k in enumerate(keys):  # (a summary keeps the order the runs were made in)
            assert con[k]["iters"] == seq[k]["iters"] and con[k]["converged"] == seq[k]["converged"]
            assert con[k]["algorithm"] == seq[k]["algorithm"]
            width = min(8, len(keys) - 8 * (j // 8))  # (more than eight runs go in groups)
            assert con[k]["sweep_kernel"] == kernel % width and con[k]["sweep_slot"] == j % 8
            assert "sweep_fallback" not in con[k] and "sweep_kernel" not in seq[k]
