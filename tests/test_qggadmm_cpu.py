"""Q-GGADMM (``graph_admm(quantize=)``, gadmm_amd/algorithms/ggadmm.py) without a GPU: the torch path
against ``chain_admm(quantize=)`` on a chain graph (bit for bit), against the long-double quantized graph
recurrence of tests/hp_qggadmm.py (under ``hp_reference.bound``, the last messages' codes exact), the seed
table of that helper, the accounting, the refusals, and how far wrong variants of the recurrence land.

Measured mutant factors (max err / bound over theta, hat, dual and objective, 24 iterations; the smallest
over the cases with a worker of degree >= 3 and their bit widths): profiles/qggadmm/README.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import hp_qggadmm as Q
import hp_reference as H

PINNED_1E4 = {"ring": 246, "grid:4x6": 106, "star:0": 91}   # E1, N = 24, rho = 3 (tests/test_gpu_ggadmm.py)


def _model(X, y):
    from gadmm_amd.models import LinearRegression
    return LinearRegression(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(y)))


_E1 = {}


def _e1(n):
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models import LinearRegression
    if n not in _E1:
        ds = linear_synthetic(n)
        m = LinearRegression(ds.X, ds.y)
        _E1[n] = (m, m.optimum())
    return _E1[n]


@pytest.mark.parametrize("n", [8, 24])
@pytest.mark.parametrize("bits", [4, 8, 16])
def test_chain_graph_equals_chain_admm_bit_for_bit(n, bits):
    """60 iterations (N = 8 stops at 55 under the 1e-4 rule, N = 24 runs to the cap): objective, iteration
    count, public models, true iterates, duals and accounting of the two torch paths are identical."""
    from gadmm_amd.algorithms import chain_admm, graph_admm
    from gadmm_amd.parallel.topology import chain_graph
    m, obj0 = _e1(n)
    c = chain_admm(m, list(range(n)), n, 3.0, obj0, 1e-4, 60, quantize=(bits, 1234), backend="torch")
    a = graph_admm(m, chain_graph(n), 3.0, obj0, 1e-4, 60, quantize=(bits, 1234), backend="torch")
    assert a.iters == c.iters and a.converged == c.converged
    assert np.array_equal(a.obj, c.obj)
    for i in (0, 1):
        assert torch.equal(a.extra["state"][i], c.extra["state"][i])
    assert a.extra["state"][2] == c.extra["state"][2]
    assert torch.equal(a.extra["theta_true"], c.extra["theta_true"])
    assert np.array_equal(a.comm_units, c.comm_units)
    for k in ("q_bits", "q_seed", "payload_bits", "min_flip_margin"):
        assert a.extra[k] == c.extra[k], k


@pytest.mark.parametrize("name,bits", Q.cases())
def test_torch_path_against_long_double_reference(name, bits):
    from gadmm_amd.algorithms import graph_admm
    g, X, y, rho, ref = Q.case(name, bits, Q.RUN)
    r = graph_admm(_model(X, y), g, rho, 0.0, 0.0, Q.RUN, backend="torch", quantize=(bits, ref.seed))
    assert r.iters == Q.RUN and not r.converged
    hat, mu = r.extra["state"][0].numpy(), r.extra["state"][1].numpy()
    R, codes = r.extra["q_msg"]
    assert np.array_equal(codes, ref.codes[-1]), "codes of the last messages"
    ratios = {"theta": ref.err_theta(r.extra["theta_true"].numpy()) / ref.b_theta, "hat": ref.err_hat(hat) / ref.b_hat,
              "dual": ref.err_dual(mu) / ref.b_dual, "objective": ref.err_obj(r.obj) / ref.b_obj,
              "R": ref.err_R(R) / ref.b_R}
    print("%s b=%d: err/bound %s" % (name, bits, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the residual trace is the sum of the K4 rows (public models): every row within b_res_w of its own
    # value, all of them >= 0, so the sum within b_res_w of itself
    total = ref.res_w.sum(axis=1)
    assert np.all(np.abs(np.asarray(r.primal_res, dtype=H.LD) - total) <= ref.b_res_w * total)


def test_seed_table():
    """Every case qualifies at its seed over the longest run a test asks for; a listed case fails at 1234;
    nothing is dropped, and every shape of the issue is there."""
    assert Q.DROPPED == ()
    assert len(Q.cases()) == 29 and {b for _, b in Q.cases()} == {4, 8, 16}
    for name, bits in Q.cases():
        agree, ratio = Q.condition(name, bits)
        assert agree and ratio >= H.QGADMM_MARGIN, (name, bits, agree, ratio)
    for (name, bits), seed in Q.SEEDS.items():
        agree, ratio = Q.condition(name, bits, seed=H.QGADMM_FIRST_SEED)
        assert seed > H.QGADMM_FIRST_SEED and not (agree and ratio >= H.QGADMM_MARGIN), (name, bits)
    d = {n: Q.case_data(n)[1].shape[2] for n in Q.CASES}
    assert [d[n] for n in ("edge-d16", "edge-d17", "edge-d8", "edge-d9", "edge-d4", "edge-d5")] == [16, 17, 8, 9, 4, 5]
    assert Q.case_graph("star20-d7").max_degree == Q.case_graph("star20tail-d7").max_degree == 19
    assert Q.case_graph("star20-d7").is_head[0] and not Q.case_graph("star20tail-d7").is_head[0]


def test_accounting():
    from gadmm_amd.algorithms import graph_admm, quantized_graph_admm
    g, X, y, rho = Q.case_data("grid2x3-d50")
    m = _model(X, y)
    r = quantized_graph_admm(m, g, rho, 0.0, 0.0, 5, 8, backend="torch")
    n, d = g.n, 50
    assert r.algorithm == "Q-GGADMM" and r.iters == 5
    assert r.extra["transmissions"] == 5 * n and r.extra["payload_bits"] == 5 * n * (8 * d + 64)
    assert r.extra["deliveries"] == 5 * 2 * len(g.edges)
    assert r.extra["q_bits"] == 8 and r.extra["q_seed"] == 1234 and r.extra["min_flip_margin"] > 0
    assert np.allclose(r.comm_units, np.arange(1, 6) * n * (8 * d + 64) / (64.0 * d), rtol=1e-15)
    u = graph_admm(m, g, rho, 0.0, 0.0, 5, backend="torch")
    assert np.array_equal(u.comm_units, np.arange(1, 6) * float(n))
    same = graph_admm(m, g, rho, 0.0, 0.0, 5, backend="torch", quantize=(8, 1234))
    assert np.array_equal(same.obj, r.obj) and torch.equal(same.extra["state"][0], r.extra["state"][0])
    other = graph_admm(m, g, rho, 0.0, 0.0, 5, backend="torch", quantize=(8, 1235))
    assert not torch.equal(other.extra["state"][0], r.extra["state"][0])
    # on the CPU backend='auto' is the torch path, with the reason recorded
    auto = graph_admm(m, g, rho, 0.0, 0.0, 5, quantize=(8, 1234))
    assert auto.extra["graph_fallback"] == "cpu tensors" and np.array_equal(auto.obj, r.obj)


def test_refusals():
    from gadmm_amd.algorithms import graph_admm
    g, X, y, rho = Q.case_data("ring4-d7")
    m = _model(X, y)
    with pytest.raises(NotImplementedError, match="censoring on graphs is not offered"):
        graph_admm(m, g, rho, 0.0, 0.0, 3, backend="torch", quantize=(8, 1234), censor=(0.1, 0.9))
    with pytest.raises(NotImplementedError, match="censoring on graphs is not offered"):
        graph_admm(m, g, rho, 0.0, 0.0, 3, backend="torch", censor=(0.1, 0.9))
    with pytest.raises(ValueError):
        graph_admm(m, g, rho, 0.0, 0.0, 3, backend="torch", quantize=(2, 1234))
    with pytest.raises(ValueError):
        graph_admm(m, g, rho, 0.0, 0.0, 3, backend="torch", quantize=(8,))


@pytest.mark.parametrize("spec", list(PINNED_1E4))
def test_quantize_none_changes_nothing(spec):
    """Without ``quantize`` the solve is the one before the argument existed: the pinned iteration counts,
    the same bits with the argument spelled out, no quantizer key in ``extra``."""
    from gadmm_amd.algorithms import graph_admm
    from gadmm_amd.algorithms.ggadmm import _graph_admm_torch
    from gadmm_amd.parallel.topology import parse_graph
    m, obj0 = _e1(24)
    g = parse_graph(spec, 24)
    a = graph_admm(m, g, 3.0, obj0, 1e-4, 3000, backend="torch")
    b = graph_admm(m, g, 3.0, obj0, 1e-4, 3000, backend="torch", quantize=None, censor=None)
    c = _graph_admm_torch(m, g, 3.0, obj0, 1e-4, 3000, "GGADMM", False)
    assert a.iters == b.iters == c.iters == PINNED_1E4[spec] and a.converged
    for r in (b, c):
        assert np.array_equal(a.obj, r.obj) and np.array_equal(a.primal_res, r.primal_res)
        assert torch.equal(a.extra["state"][0], r.extra["state"][0]) and torch.equal(a.extra["state"][1], r.extra["state"][1])
    assert not {"q_bits", "transmissions", "theta_true", "q_msg", "payload_bits"} & set(a.extra)
    assert np.array_equal(a.comm_units, np.arange(1, a.iters + 1) * 24.0)


MUTANT_CASES = [(n, b) for n, b in Q.cases() if Q.case_graph(n).max_degree >= 3]


@pytest.mark.parametrize("name,bits", MUTANT_CASES)
def test_mutants_land_outside_the_bound(name, bits):
    """Each wrong variant of the float64 recurrence lands more than one bound away. ``"u-slot"`` (the
    uniforms indexed by launch slot) IS the recurrence where the launch order -- heads in ascending id,
    then tails -- is the identity (star_graph(n, 0) with the hub a head): there the factor is None,
    and the variant is asserted to reproduce the float64 run bit for bit instead."""
    f = Q.mutant_factors(name, bits)
    print("%s b=%d: %s" % (name, bits, " ".join("%s %s" % (k, "same" if v is None else "%.3g" % v) for k, v in f.items())))
    g = Q.case_graph(name)
    for mut, v in f.items():
        if v is None:
            assert mut == "u-slot" and list(g.order) == list(range(g.n))
            ref = Q.case(name, bits)[4]
            a = Q._history(name, bits, ref.seed, Q.RUN, np.float64, "u-slot")
            b = Q._history(name, bits, ref.seed, Q.RUN, np.float64)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        else:
            assert v > 1.0, (name, bits, mut, v)


def test_graph_q_abi_and_launcher_rules():
    """The ctypes mirror of GraphQArgs, and the launcher's shape rules asked without a device."""
    from gadmm_amd.ops import native
    lib = native.require()
    buf = (ctypes.c_longlong * 16)()
    k = lib.gadmm_graph_q_abi_layout(buf, 16)
    Qa = native.GraphQArgs
    assert k == 7 and list(buf[:k]) == [ctypes.sizeof(Qa), 0, Qa.qg.offset, Qa.q_bits.offset, Qa.q_seed.offset,
                                        Qa.q_true.offset, ctypes.sizeof(native.GraphArgs)]
    native.check_graph_q_abi(lib)
    native.check_graph_abi(lib)   # GraphArgs did not move
    a = native.GraphQArgs()
    for d, n, deg, bits, cls in ((50, 24, 2, 8, 2), (50, 24, 4, 4, 4), (64, 8, 7, 16, 8), (50, 12, 11, 8, 16),
                                 (7, 20, 19, 8, 16), (50, 24, 23, 8, 16), (65, 4, 2, 8, 0), (50, 1, 1, 8, 0),
                                 (50, 24, 2, 2, 0), (50, 24, 2, 0, 0), (50, 24, 2, 32, 0)):
        a.g.d, a.g.n, a.g.max_degree, a.q_bits = d, n, deg, bits
        assert lib.gadmm_graph_persistent_q_class(ctypes.byref(a)) == cls, (d, n, deg, bits)
    assert lib.gadmm_graph_persistent_q_lds(24, 4) == lib.gadmm_graph_persistent_lds(24, 4)
    assert lib.gadmm_graph_persistent_q_lds(200, 122) > 65536 >= lib.gadmm_graph_persistent_q_lds(200, 121)
    # malformed arguments are refused with -1 before any HIP call
    a.g.d, a.g.n, a.g.max_degree, a.q_bits = 50, 24, 4, 2
    assert lib.gadmm_graph_persistent_q_launch(ctypes.byref(a), None) == -1
    assert b"q_bits must be 4, 8 or 16" in lib.gadmm_last_error()
    a.q_bits = 8
    assert lib.gadmm_graph_persistent_q_launch(ctypes.byref(a), None) == -1
    assert b"a required buffer is null" in lib.gadmm_last_error()


def test_entry_quant_bits(tmp_path):
    from gadmm_amd.entry import LinearRegression_Topologies as E
    out = E.main(["--device", "cpu", "--quick", "--out", str(tmp_path), "--no-plot", "--set", "quant_bits=8,4",
                  "graphs=ring,star:0"])
    runs = out["runs"]
    assert sorted(runs) == sorted(["GGADMM_ring_rho3", "GGADMM_star:0_rho3"] +
                                  ["Q-GGADMM_b%d_%s_rho3" % (b, s) for b in (8, 4) for s in ("ring", "star:0")])
    for k, s in runs.items():
        if k.startswith("Q-"):
            assert s["q_bits"] in (4, 8) and s["transmissions"] == s["iters"] * 24 and s["converged"]
