"""GGADMM without a GPU: the bipartite-graph topology, the torch path of ``graph_admm`` (bit for bit the
chain's torch path on a chain graph, the pinned iteration counts of every graph, the accounting), the
long-double edge-dual reference of tests/hp_ggadmm.py and its mutants, the entry, every refusal and the
ABI of ``GraphArgs``."""
import json

import numpy as np
import pytest
import torch

import hp_ggadmm as G
import hp_reference as H
from gadmm_amd.parallel import topology as T

K = H.K_ITERS

# iterations to |objective - obj0| < 1e-4 on the E1 data: {graph: {N: (rho = 3, rho = 1)}}. The chain
# column is the reference's GADMM; the others come from a NumPy float64 prototype of the recurrence
# whose crossings sit >= 0.3 % inside the tolerance, far above float64 noise.
PINNED = {
    "chain": {24: (784, 2425), 8: (55, 196)},
    "ring": {24: (246, 847), 8: (22, 55)},
    "grid": {24: (106, 258), 8: (33, 49)},
    "star:0": {24: (91, 348), 8: (35, 68)},
    "kbip": {24: (156, 98), 8: (47, 19)},
}
EDGES = {"chain": {24: 23, 8: 7}, "ring": {24: 24, 8: 8}, "grid": {24: 38, 8: 10}, "star:0": {24: 23, 8: 7},
         "kbip": {24: 144, 8: 16}}


# ------------------------------------------------------------------------------------------------ topology
def test_rejects_odd_cycles_and_names_them():
    with pytest.raises(ValueError, match=r"odd cycle through workers \[1, 0, 2\]"):
        T.BipartiteGraph(3, [(0, 1), (1, 2), (2, 0)])
    with pytest.raises(ValueError) as e:
        T.BipartiteGraph(5, [(k, (k + 1) % 5) for k in range(5)])
    named = [int(v) for v in str(e.value).split("[")[1].split("]")[0].split(",")]
    assert sorted(named) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="odd cycle"):  # a triangle hanging off a path
        T.BipartiteGraph(5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 2)])
    with pytest.raises(ValueError):
        T.ring_graph(5)


def test_rejects_malformed_graphs():
    with pytest.raises(ValueError, match="not connected"):
        T.BipartiteGraph(4, [(0, 1), (2, 3)])
    with pytest.raises(ValueError, match="duplicate edge"):
        T.BipartiteGraph(3, [(0, 1), (1, 0), (1, 2)])
    with pytest.raises(ValueError, match="self-loop"):
        T.BipartiteGraph(3, [(0, 1), (1, 1), (1, 2)])
    with pytest.raises(ValueError, match="worker ids"):
        T.BipartiteGraph(3, [(0, 1), (1, 3)])
    with pytest.raises(ValueError, match="not a colour class"):
        T.BipartiteGraph(4, [(0, 1), (1, 2), (2, 3)], heads=[0, 1])
    with pytest.raises(ValueError, match="not a colour class"):
        T.BipartiteGraph(4, [(0, 1), (1, 2), (2, 3)], heads=[0])
    with pytest.raises(ValueError):
        T.parse_graph("grid:4x5", 24)
    with pytest.raises(ValueError):
        T.parse_graph("torus", 24)


def test_heads_default_and_explicit():
    g = T.BipartiteGraph(4, [(3, 2), (1, 2), (0, 1)])
    assert g.heads == [0, 2] and g.tails == [1, 3] and g.edges == [(0, 1), (2, 1), (2, 3)]
    h = T.BipartiteGraph(4, [(3, 2), (1, 2), (0, 1)], heads=[3, 1])
    assert h.heads == [1, 3] and h.tails == [0, 2] and h.edges == [(1, 0), (1, 2), (3, 2)]
    assert g.neighbours(2) == [1, 3] and g.degree == [1, 2, 2, 1] and g.max_degree == 2


def test_builders_degrees_and_csr_order():
    c = T.chain_graph(5)
    assert c.heads == [0, 2, 4] and c.degree == [1, 2, 2, 2, 1]
    p = T.chain_graph(4, path=[2, 0, 3, 1])
    assert p.heads == [2, 3] and p.edges == [(2, 0), (3, 0), (3, 1)]  # heads at even POSITIONS, as GADMM
    r = T.ring_graph(6)
    assert r.degree == [2] * 6 and len(r.edges) == 6 and r.neighbours(0) == [1, 5]
    g = T.grid_graph(4, 6)
    assert sorted(g.degree) == [2] * 4 + [3] * 12 + [4] * 8 and len(g.edges) == 38 and g.max_degree == 4
    s = T.star_graph(12, 5)
    assert s.degree[5] == 11 and s.tails == [5] and s.max_degree == 11 and len(s.edges) == 11
    k = T.complete_bipartite_graph(2, 3)
    assert k.heads == [0, 2] and k.tails == [1, 3, 4] and len(k.edges) == 6 and k.degree == [3, 2, 3, 2, 2]
    kb = T.parse_graph("kbip", 8)
    assert kb.heads == [0, 2, 4, 6] and len(kb.edges) == 16
    assert T.graph_from_edges(3, [(0, 1), (1, 2)]).key() == T.chain_graph(3).key()
    for name in EDGES:
        for n in (24, 8):
            spec = ("grid:4x%d" % (n // 4)) if name == "grid" else name
            assert len(T.parse_graph(spec, n).edges) == EDGES[name][n]
    # CSR in launch order: the heads in ascending id, then the tails; neighbours ascending inside a row
    g = T.grid_graph(2, 3)
    ptr, idx = g.csr()
    assert g.order == [0, 2, 4, 1, 3, 5] and ptr.dtype == idx.dtype == np.int32
    assert ptr.tolist() == [0, 2, 4, 7, 10, 12, 14]
    assert idx.tolist() == [1, 3, 1, 5, 1, 3, 5, 0, 2, 4, 0, 4, 2, 4]
    assert np.array_equal(g.nb_ptr, ptr) and np.array_equal(g.nb_idx, idx)
    for k_, w in enumerate(g.order):
        assert idx[ptr[k_]:ptr[k_ + 1]].tolist() == g.neighbours(w) == sorted(g.neighbours(w))


# ------------------------------------------------------------------------------------------------ torch path
_E1 = {}


def _e1(n):
    if n not in _E1:
        from gadmm_amd.data import linear_synthetic
        from gadmm_amd.models import LinearRegression
        from gadmm_amd.oracle.reference import opt_linear
        ds = linear_synthetic(n)
        Xf, yf = ds.stacked()
        _E1[n] = (LinearRegression(ds.X, ds.y), opt_linear(Xf.numpy(), yf.numpy()))
    return _E1[n]


@pytest.mark.parametrize("n,iters", [(8, 55), (24, 784)])
def test_chain_graph_is_chain_admm_bit_for_bit(n, iters):
    from gadmm_amd.algorithms import chain_admm, graph_admm, generalized_group_admm
    assert generalized_group_admm is graph_admm
    m, obj0 = _e1(n)
    c = chain_admm(m, list(range(n)), n, 3.0, obj0, 1e-4, 3000, backend="torch")
    g = graph_admm(m, T.chain_graph(n), 3.0, obj0, 1e-4, 3000, backend="torch")
    assert c.iters == g.iters == iters and g.converged
    assert np.array_equal(c.obj, g.obj)
    assert torch.equal(c.extra["state"][0], g.extra["state"][0])  # theta
    assert torch.equal(c.extra["state"][1], g.extra["state"][1])  # mu
    assert c.extra["state"][2] == g.extra["state"][2] == iters + 1
    assert np.array_equal(c.comm_units, g.comm_units)
    assert np.allclose(c.primal_res, g.primal_res, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [8, 24])
@pytest.mark.parametrize("name", [k for k in PINNED if k != "chain"])
def test_pinned_iteration_counts(name, n):
    """(The chain's counts at rho = 3 are held by test_chain_graph_is_chain_admm_bit_for_bit, at rho = 1
    by test_pinned_chain_rho1.)"""
    from gadmm_amd.algorithms import graph_admm
    m, obj0 = _e1(n)
    g = T.parse_graph(("grid:4x%d" % (n // 4)) if name == "grid" else name, n)
    got = tuple(graph_admm(m, g, rho, obj0, 1e-4, 3000, backend="torch").iters for rho in (3.0, 1.0))
    assert got == PINNED[name][n], (name, n, got)


@pytest.mark.parametrize("n", [8, 24])
def test_pinned_chain_rho1(n):
    from gadmm_amd.algorithms import graph_admm
    m, obj0 = _e1(n)
    r = graph_admm(m, T.chain_graph(n), 1.0, obj0, 1e-4, 3000, backend="torch")
    assert r.converged and r.iters == PINNED["chain"][n][1]


def test_accounting_and_primal_residual():
    from gadmm_amd.algorithms import graph_admm
    m, obj0 = _e1(8)
    g = T.grid_graph(4, 2)
    r = graph_admm(m, g, 3.0, obj0, 1e-4, 3000, backend="torch", record_theta=True)
    assert r.iters == 33 and len(r.obj) == 33
    assert np.array_equal(r.comm_units, (np.arange(33) + 1.0) * 8)
    assert r.extra["deliveries"] == 33 * 2 * 10
    assert r.extra["graph"] == {"n": 8, "edges": [list(e) for e in g.edges], "max_degree": 3, "heads": g.heads}
    theta, mu, nxt = r.extra["state"]
    assert nxt == 34 and np.array_equal(r.theta, theta.numpy())
    direct = sum(float(((theta[h] - theta[t]) ** 2).sum()) for h, t in g.edges)  # each edge once
    assert np.isclose(r.primal_res[-1], direct, rtol=1e-12, atol=0)
    assert abs(float(mu.sum())) < 1e-9 * float(mu.abs().max())  # the per-worker duals sum to zero
    # an unconverged run reports the iterations it ran
    s = graph_admm(m, g, 3.0, obj0, 1e-4, 5, backend="torch")
    assert not s.converged and s.iters == 5 and s.extra["deliveries"] == 5 * 20 and s.extra["state"][2] == 6


@pytest.mark.parametrize("name", list(G.CASES))
def test_torch_path_against_long_double_reference(name):
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.models import LinearRegression
    g, X, y, rho, ref = G.case(name)
    m = LinearRegression(torch.from_numpy(X.copy()), torch.from_numpy(y.copy()))
    r = graph_admm(m, g, rho, 0.0, 0.0, K, backend="torch")
    theta, mu, _ = r.extra["state"]
    ratios = {"theta": ref.err_theta(theta.numpy(), K) / ref.b_theta, "dual": ref.err_dual(mu.numpy()) / ref.b_dual,
              "objective": ref.err_obj(r.obj) / ref.b_obj}
    res = ref.res_w.sum(axis=1)
    res64 = G.graph_residual(np.asarray(G._history(name, K, np.float64)[0][:K]), g.edges, g.heads, np.float64).sum(axis=1)
    e_res = H.noise_level(res, res64, np.abs(res))
    ratios["residual"] = H.noise_level(res, r.primal_res, np.abs(res)) / H.bound(e_res, G.CASES[name][2])
    print("ggadmm torch %s: err/bound %s" % (name, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("name", [n for n in G.CASES if G.case_graph(n).max_degree >= 3])
def test_mutants_of_the_reference_land_above_the_bound(name):
    """One dropped edge, one neighbour read one iteration stale, deg - 1 in one inverse: each at a worker
    of degree >= 3, each far above the bound the implementations are held to."""
    f = G.mutant_factors(name)
    print("ggadmm mutants %s: err/bound %s" % (name, " ".join("%s %.3g" % kv for kv in f.items())))
    assert set(f) == set(G.MUTANTS) and all(v > 1.0 for v in f.values()), f


def test_edge_dual_reference_is_gadmm_on_a_chain():
    """On the identity chain the edge-dual recurrence is hp_reference.gadmm_linear (same operations up to
    the order of the dual sums): float64 runs agree to rounding."""
    X, y, rho = H.make_linear(5, 40, 33, 3)
    g = T.chain_graph(5)
    th, mu, obj = G.ggadmm_linear(X, y, rho, K, g.edges, g.heads, np.float64)
    th0, mu0, obj0 = H.gadmm_linear(X, y, rho, K, np.float64)
    assert np.allclose(th, th0, rtol=0, atol=1e-13 * np.abs(th0).max())
    assert np.allclose(mu, mu0, rtol=0, atol=1e-13 * rho * np.abs(th0).max())
    assert np.allclose(obj, obj0, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.data import logistic_synthetic
    from gadmm_amd.models import make_model
    m, obj0 = _e1(8)
    g = T.ring_graph(8)
    with pytest.raises(RuntimeError, match="cpu tensors"):
        graph_admm(m, g, 3.0, obj0, 1e-4, 10, backend="native")
    ds = logistic_synthetic(8)
    with pytest.raises(NotImplementedError, match="linear model"):
        graph_admm(make_model("logistic", ds.X, ds.y, lam=1e-5), g, 3.0, 0.0, 1e-4, 10)

    class TwoRanks:
        nranks, rank = 2, 0
    with pytest.raises(NotImplementedError, match="2 ranks"):
        graph_admm(m, g, 3.0, obj0, 1e-4, 10, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match="every worker local"):
        graph_admm(m, T.ring_graph(6), 3.0, obj0, 1e-4, 10)
    with pytest.raises(TypeError):
        graph_admm(m, [(0, 1)], 3.0, obj0, 1e-4, 10)
    with pytest.raises(ValueError):
        graph_admm(m, g, 3.0, obj0, 1e-4, 10, backend="hip")
    r = graph_admm(m, g, 3.0, obj0, 1e-4, 10)  # auto on CPU tensors: the torch path, with the reason
    assert r.extra["backend"] == "torch" and r.extra["graph_fallback"] == "cpu tensors"
    assert "graph_fallback" not in graph_admm(m, g, 3.0, obj0, 1e-4, 10, backend="torch").extra


# ------------------------------------------------------------------------------------------------ entry, ABI
def test_entry_quick_on_cpu(tmp_path):
    from gadmm_amd import entry
    from gadmm_amd.config import get_preset
    assert "LinearRegression_Topologies" in entry.ENTRIES
    cfg = get_preset("LinearRegression_Topologies")
    assert cfg.graphs == ["chain", "ring", "grid:4x6", "star:0", "kbip"] and cfg.rhos == [3.0] and cfg.acc == 1e-4
    out = entry.get("LinearRegression_Topologies").main(["--quick", "--device", "cpu", "--out", str(tmp_path)])
    runs = out["runs"]
    assert list(runs) == ["GGADMM_%s_rho3" % s for s in cfg.graphs]
    want = {"chain": 400, "ring": 246, "grid:4x6": 106, "star:0": 91, "kbip": 156}  # --quick caps the chain at 400
    for spec, iters in want.items():
        s = runs["GGADMM_%s_rho3" % spec]
        assert s["iters"] == iters and s["converged"] == (spec != "chain")
        assert s["engine"] == "torch" and s["kernel"] == "torch" and s["graph_name"] == spec
        assert s["comm_units"] == iters * 24
    with open(out["summary_path"]) as f:
        summ = json.load(f)
    assert summ["entry"] == "LinearRegression_Topologies" and len(summ["runs"]) == 5
    files = {p.name for p in tmp_path.iterdir()}
    assert "GGADMM_ring_rho3.jsonl" in files and any(n.endswith(".png") for n in files)


def test_entry_graph_override():
    from gadmm_amd.config import get_preset, parse_overrides
    cfg = parse_overrides(get_preset("LinearRegression_Topologies"), ["graphs=ring,grid:3x8", "rhos=1,3"])
    assert cfg.graphs == ["ring", "grid:3x8"] and cfg.rhos == [1.0, 3.0]


def test_graph_abi_layout_matches_ctypes():
    import ctypes
    from gadmm_amd.ops import native
    lib = native.require()
    buf = (ctypes.c_longlong * 16)()
    k = lib.gadmm_graph_abi_layout(buf, 16)
    G_ = native.GraphArgs
    exp = [ctypes.sizeof(G_), G_.epoch.offset, G_.rho.offset, G_.timeout_ticks.offset, G_.nb_ptr.offset,
           G_.Minv.offset, G_.thg.offset, G_.dec_push.offset, G_.rres.offset, G_.ctl.offset, G_.xchk.offset,
           G_.xtag.offset]
    assert k == 12 and list(buf[:k]) == exp
    native.check_graph_abi(lib)
    # the launcher's shape rules, asked without a device: the degree class and the LDS it sizes
    a = native.GraphArgs()
    for d, n, deg, cls in ((50, 24, 2, 2), (50, 24, 4, 4), (64, 8, 7, 8), (50, 12, 11, 16), (50, 24, 23, 32),
                            (50, 64, 40, 32), (65, 4, 2, 0), (50, 1, 1, 0)):
        a.d, a.n, a.max_degree = d, n, deg
        assert lib.gadmm_graph_persistent_class(ctypes.byref(a)) == cls, (d, n, deg)
    assert lib.gadmm_graph_persistent_lds(24, 4) == (2 + 344 + 4 * 64 + 2) * 8
    # 64 KB hold the staging of degree 121: (2 + 344 + 64 deg + ceil(deg / 2)) * 8 <= 65536
    assert lib.gadmm_graph_persistent_lds(200, 122) > 65536 >= lib.gadmm_graph_persistent_lds(200, 121)
