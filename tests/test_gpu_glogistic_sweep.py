"""Logistic GGADMM sweep (csrc/kernels/graph_persistent_logistic.hip: graph_logistic_sweep_kernel) on the MI355X:
every slot of a launch held to the long-double reference of tests/hp_glogistic.py (what tests/test_gpu_glogistic.py
asks of the single solve, bounds ``hp_reference.bound`` unchanged), the public function bit for bit against the
single solves, the fallback and the launcher's refusal, and the entry. No test provokes a timeout, a fault or a hang.
"""
import ctypes

import numpy as np
import pytest
import torch

import hp_glogistic as GL
import hp_reference as H
from hp_ggadmm import OVERRUN, _star_leaf_heads
from test_gpu_glogistic import STAR12, _dev, _engine, _host, _model, _poison_lds  # noqa: F401 (the autouse fixture)

from gadmm_amd.parallel import topology as T

pytestmark = pytest.mark.gpu
K = H.K_ITERS
SLOTS = {13: [n for n, c in GL.CASES.items() if max(c[1], c[2]) <= 52],   # six of the eight slots, idle ones behind
         16: [n for n, c in GL.CASES.items() if max(c[1], c[2]) > 52]}   # three


@pytest.mark.parametrize("qt", list(SLOTS))
def test_every_slot_against_long_double_reference(qt):
    """One launch per register class over already-built members: n = 2 .. 20, degree classes 2, 4 and 8, second and
    third poll groups, the live inner stop and idle slots side by side."""
    from gadmm_amd.engine.graph_logistic_sweep import GraphLogisticSweepEngine
    names = SLOTS[qt]
    assert len(names) == {13: 6, 16: 3}[qt]
    sw = GraphLogisticSweepEngine([_engine(name, K) for name in names])
    runs = sw.run()
    assert sw.last_kernel == "persistent-graph-logistic-sweep(K=%d)" % len(names)
    for name, eng, r in zip(names, sw.members, runs):
        last = eng.ctl_state()["iter"] - 1
        assert r.done == 2 and r.iters == K and K <= last <= K + OVERRUN, (name, r.iters, r.done, last)
        ref = GL.case(name, last)[-1]
        rows, inner = _host(eng.rres[:K]), ref.extra[0][last - 1]
        ratios = {"theta": ref.err_theta(_host(eng.theta), last) / ref.b_theta,
                  "dual": ref.err_dual(_host(eng.mu)) / ref.b_dual,
                  "objective": ref.err_obj(eng.traces(K)[0]) / ref.b_obj, "K4 rows": ref.err_res_w(rows) / ref.b_res_w}
        print("glogistic sweep QT=%d %s (last=%d, class %d, placed %d): err/bound %s; inner steps %s" % (
            qt, name, last, eng.kernel_class(), eng.last_placed, " ".join("%s %.3f" % kv for kv in ratios.items()),
            inner.tolist()))
        assert all(v <= 1.0 for v in ratios.values()), (name, ratios)
        assert np.array_equal(_host(eng.inner_iters), inner) and (name != GL.LIVE or inner.max() < H.MAX_INNER)


def test_public_function_is_the_single_solves_bit_for_bit():
    """Ten members over the shards of star12hub5-m53-d20 (8 + 2), each to its own tolerance stop. Every member stops by
    its tolerance inside 1000 iterations on the torch path (chain 659, ring 192, grid 168, star 493, hub 469, complete
    bipartite 64, the ring at half its rho 374, the short inner solve 397, the 1e-3 repeats 521 and 155)."""
    from gadmm_amd.algorithms import graph_admm_logistic, graph_admm_logistic_sweep
    step = GL.case_data(STAR12)[5]
    model = _model(STAR12)
    obj0 = model.optimum()
    gs = [T.chain_graph(12), T.ring_graph(12), T.grid_graph(3, 4), T.star_graph(12, 0), _star_leaf_heads(12, 5),
          T.complete_bipartite_graph(6, 6)]
    rule = [0.2 / (step * g.max_degree) for g in gs]
    members = [(g, rho) for g, rho in zip(gs, rule)] + [(gs[1], 0.5 * rule[1]), (gs[0], rule[0], step, 7, 1e-3),
                                                      (gs[0], rule[0]), (gs[1], rule[1])]
    tols = [1e-4] * 8 + [1e-3] * 2
    got = graph_admm_logistic_sweep(model, members, obj0, 1e-4, 1000, step, max_inner=H.MAX_INNER, inner_tol=0.0,
                                    tols=tols)
    assert len(got) == 10
    for j, (g, mem, tol) in enumerate(zip(got, members, tols)):
        st, mi, it = mem[2:] if len(mem) == 5 else (step, H.MAX_INNER, 0.0)
        r = graph_admm_logistic(model, mem[0], mem[1], obj0, tol, 1000, st, max_inner=mi, inner_tol=it, backend="native")
        a, b = g.extra["engine_obj"], r.extra["engine_obj"]
        print("member %d: %d iterations, %s slot %d placed %d" % (j, g.iters, g.extra["kernel"], g.extra["sweep"]["slot"],
                                                                  g.extra["sweep"]["placed"]))
        assert g.converged and r.converged and g.iters == r.iters and np.array_equal(g.obj, r.obj), (j, g.iters, r.iters)
        assert np.array_equal(g.primal_res, r.primal_res) and np.array_equal(g.comm_units, r.comm_units)
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("theta", "mu", "inner_iters")), j
        assert g.extra["graph"] == r.extra["graph"] and g.extra["deliveries"] == r.extra["deliveries"]
        sw = g.extra["sweep"]
        assert (sw["width"], sw["slot"]) == ((8, j) if j < 8 else (2, j - 8)) and sw["placed"] in (1, 2)
        assert sw["kernel"] == g.extra["kernel"] == "persistent-graph-logistic-sweep(K=%d)" % sw["width"]
        assert "sweep_fallback" not in g.extra


def test_fallback_and_refusal():
    """m = 65 is the loop; two members that name one ``inner_iters`` buffer are refused with -1 before any launch."""
    from gadmm_amd.algorithms import graph_admm_logistic_sweep
    from gadmm_amd.models import LogisticRegression
    from gadmm_amd.ops import native
    X, y, rho, lam, step = H.make_logistic(4, 65, 20, 11)
    got = graph_admm_logistic_sweep(LogisticRegression(_dev(X), _dev(y), lam), [(T.ring_graph(4), rho)], 0.0, 0.0, 3,
                                    step, max_inner=H.MAX_INNER)
    assert got[0].extra["sweep_fallback"] == "max(d, m) > 64" and got[0].extra["backend"] == "torch"
    engs = [_engine("edge-m5-d3", K) for _ in range(2)]
    batch = (native.GraphLogiArgs * 2)(*[e.prepare() for e in engs])
    batch[1].l.inner_iters = batch[0].l.inner_iters
    stage = (native.GraphLogiArgs * 8)()
    lib = native.require()
    rc = lib.gadmm_graph_logistic_sweep_launch(batch, 2, ctypes.addressof(stage), ctypes.addressof(stage), None)
    assert rc == -1 and "solves 0 and 1 share a buffer that both write" in lib.gadmm_last_error().decode()
    assert all(e.ctl_state()["done"] == 0 and e.ctl_state()["placed"] == 0 for e in engs)  # nothing ran


def test_entry_with_the_switch(tmp_path):
    from gadmm_amd.entry import LogisticRegression_Topologies as E
    runs = {k: E.main(["--device", "cuda", "--out", str(tmp_path / k), "--no-plot"] + extra)["runs"]
            for k, extra in (("seq", []), ("con", ["--set", "sweep=concurrent"]))}
    assert list(runs["con"]) == list(runs["seq"]) and len(runs["con"]) == 5
    for key, s in runs["con"].items():
        assert s["converged"] and s["iters"] == runs["seq"][key]["iters"] and "sweep_fallback" not in s, (key, s)
        assert s["kernel"].startswith("persistent-graph-logistic-sweep"), (key, s["kernel"])
