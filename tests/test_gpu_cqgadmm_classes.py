"""The CQ-GADMM kernels (the CENS = true bodies of csrc/kernels/chain_quant.hip, compiled in
chain_cquant.hip) against a long-double reference of the censored quantized recurrence, class by class.

tests/test_gpu_cqgadmm.py holds the censored kernels against the specification applied to the kernel's
OWN theta, for one iteration, and the two engines against each other: a mistake both engines share --
a dual that reads a censored worker's candidate row, a neighbour copy that moves on a censored header,
a stale code granule applied, a threshold read one slot off -- passes there. Here the graph engine's
censored phase kernel (chain_phase_linear_cq<1>, <2>, <4>), the persistent censored kernel
(chain_persistent_cq_kernel<13>, <16>) and the censored sweep kernel run a tiny problem with no stop
rule (tol = 0, obj0 = 0, max_iter = K, the exact objective), and the sent trace (exactly), the true
theta, the public models th_hat, the duals, every objective value, the K4 residual, and from the graph
engine's message table the codes, R, the packed words and the censored headers, are compared with the
censored hp_reference.qgadmm_linear in long double under the bound of tests/test_gpu_dispatch_classes.py,

    err_kernel <= 8 * max(e64, max(d, 16) * 2^-53),

e64 being the distance of the float64 run of the same recurrence from its long-double run. A censored
run is comparable only while neither a code nor a censoring decision can flip, and it tests censoring
only if workers are censored: per case (seed, tau0, xi) is the first combination of a fixed search order
(hp_reference.cq_search_order) for which both runs take identical codes and decisions, the flip margin
is >= 4 b_theta, the censor margin >= 4 b_s, and within the first 8 and the first 20 iterations a head
and a tail are censored, a head and a tail send, somebody solves between a censored and a sent
neighbour and somebody sends, is censored and sends again (hp_reference.CQGADMM_CASES, found on the CPU;
tests/test_hp_reference_cpu.py asserts the conditions and that six wrong variants of the censored part
fail the comparison made here).
A persistent kernel stops ``last - K <= 16`` iterations after the cap: the reference runs to ``last``.
Each test prints err / bound; profiles/cqgadmm_classes/README.md records the measured table.

Each parameter list names the dispatch condition that puts its shape in its class: if a threshold
moves, the list next to it is the one to revisit.

Run with: pytest -m gpu tests/test_gpu_cqgadmm_classes.py -s
"""
import numpy as np
import pytest
import torch

import hp_reference as H
from test_gpu_dispatch_classes import _dev, _host, _report

pytestmark = pytest.mark.gpu

K = H.K_ITERS
BLOCK = 4  # iterations per graph replay: divides K
PK = H.QGADMM_PERSISTENT_K
assert K % BLOCK == 0 and PK % BLOCK == 0
BITS = H.QGADMM_BITS


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _engine(n, m, d, bits, cap, path=None, seed=None, censor=None, **kw):
    """A CQ engine on the case's data with the case's (seed, tau0, xi) -- or the ones given -- ``cap``
    iterations, nothing stops early. ``censor=False``: a Q engine (an uncensored member of a sweep)."""
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    X, y, rho = H.make_linear(n, m, d, H.seed_of(n, m, d))
    if censor is False:
        seed, censor = H.qgadmm_seed(n, m, d, bits, path)[0], None
    elif censor is None:
        seed, tau0, xi = H.cqgadmm_censor(n, m, d, bits, path)
        censor = (tau0, xi)
    eng = NativeChainEngine(_dev(X), _dev(y), list(range(n)), n, "linear", rho=rho, obj0=0.0, tol=0.0, max_iter=cap,
                            obj_mode="exact", block=BLOCK, quant=(bits, seed), censor=censor, **kw)
    eng.set_path(list(range(n)) if path is None else list(path), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def _table_is_the_references(eng, ref):
    """The engine's threshold table (longer: the persistent kernel overruns) starts with the reference's,
    bit for bit."""
    thr2 = _host(eng.c_thr2)
    assert thr2.dtype == np.float64 and len(thr2) >= len(ref.thr2)
    assert np.array_equal(thr2[:len(ref.thr2)].view(np.uint64), ref.thr2.view(np.uint64))


def _state_ratios(eng, ref, last):
    """The true theta and th_hat after iteration ``last`` and, once the heads' lazy last dual update
    is applied (flush_duals), mu after it."""
    true, hat = _host(eng.theta_true), _host(eng.theta)
    eng.flush_duals()
    eng.stream.synchronize()
    mu = _host(eng.mu)
    assert np.all(np.isfinite(true)) and np.all(np.isfinite(hat)) and np.all(np.isfinite(mu))
    return {"theta_true": ref.err_theta(true, last) / ref.b_theta, "th_hat": ref.err_hat(hat) / ref.b_hat,
            "dual": ref.err_dual(mu) / ref.b_dual}


def _message_ratios(eng, ref, d, bits):
    """``q_msg`` after the reference's last iteration. A worker that sent in it: its codes exactly, the
    words ``pack_codes`` of them, R within its bound. A censored one: the censored header, and the code
    words of its last sent message (the kernel writes none), all zero if it never sent."""
    from gadmm_amd.algorithms import quantize as Q
    msg = _host(eng.q_msg).view(np.uint64)
    n = ref.codes.shape[1]
    assert msg.shape == (n, 1 + Q.words_per_row(d, bits))
    now = ref.sent[-1]
    for w in range(n):
        if now[w]:
            codes = Q.unpack_codes(msg[w, 1:], bits, d)
            flips = int(np.sum(codes != ref.codes[-1, w]))
            assert flips == 0, "worker %d: %d codes differ from the reference's" % (w, flips)
            assert np.array_equal(msg[w, 1:], Q.pack_codes(ref.codes[-1, w], bits))
        else:
            assert int(msg[w, 0]) == Q.CENSORED_HEADER, (w, hex(int(msg[w, 0])))
            it = int(ref.last_sent[w])
            want = Q.pack_codes(ref.codes[it - 1, w], bits) if it else np.zeros_like(msg[w, 1:])
            assert np.array_equal(msg[w, 1:], want), (w, it)
    if not now.any():
        return {}
    R = msg[now, 0].copy().view(np.float64)
    return {"R": H.noise_level(ref.R[-1][now], R, ref.scale_theta) / ref.b_R}


def run_graph(n, m, d, bits, use_graph=True, path=None, residual=False):
    ref = H.cqgadmm_case(n, m, d, bits, K, path)[3]
    eng = _engine(n, m, d, bits, K, path, residual=residual)
    _table_is_the_references(eng, ref)
    r = eng.run(stop_iter=K, use_graph=use_graph)
    assert r.iters == K and eng.ctl_state()["iter"] == K + 1, (r.iters, r.done, eng.ctl_state())
    assert r.replays == K // BLOCK and (eng.graph_ok() or not use_graph) and eng.obj_mode_name == "exact"
    sent = eng.sent_trace(K)
    assert np.array_equal(sent, ref.sent), np.argwhere(sent != ref.sent)
    out = {"objective": ref.err_obj(eng.objective_trace(K)) / ref.b_obj}
    if residual:
        out["residual"] = ref.err_res(eng.primal_residual(K)) / ref.b_res
    out.update(_message_ratios(eng, ref, d, bits))
    out.update(_state_ratios(eng, ref, K))
    eng.close()
    return out


def _persistent_ratios(eng, n, m, d, bits, path, residual, case=None):
    """After a persistent launch capped at PK: it stops after iteration ``last = ctl.iter - 1``; the sent
    trace and the objective over 1..PK, the state against the reference run to ``last``."""
    st = eng.ctl_state()
    last = st["iter"] - 1
    assert st["done"] == 2 and PK <= last <= PK + H.PERSISTENT_OVERRUN, (st, last)
    ref = (H.cqgadmm_case(n, m, d, bits, last, path) if case is None else case(last))[3]
    if eng.censor is not None:
        _table_is_the_references(eng, ref)
        sent = eng.sent_trace(PK)
        assert np.array_equal(sent, ref.sent[:PK]), np.argwhere(sent != ref.sent[:PK])
    out = {"objective": ref.err_obj(eng.objective_trace(PK)) / ref.b_obj}
    if residual:
        out["residual"] = ref.err_res(eng.primal_residual(PK)) / ref.b_res
    out.update(_state_ratios(eng, ref, last))
    return out


def run_persistent(n, m, d, bits, xcd=2, path=None, residual=False):
    """One launch of the persistent CQ kernel with the cap at PK."""
    eng = _engine(n, m, d, bits, PK, path, residual=residual, xcd=xcd)
    assert eng.persistent_q_eligible()
    r = eng.run_persistent(fetch_trace=True)
    assert eng.last_kernel.startswith("persistent-CQ"), eng.last_kernel
    assert eng.last_placed == xcd, (eng.last_placed, xcd)
    assert r.iters == PK and r.done == 2, (r.iters, r.done)
    out = _persistent_ratios(eng, n, m, d, bits, path, residual)
    eng.close()
    return out


# ------------------------------------------------------------------------------------------------
# Graph-CQ: gadmm_chain_phase_cquant switches on nc = (d + 63) / 64 between chain_phase_linear_cq<1>
# (d <= 64), <2> (65..128) and <4> (129..256); block_sum_f64 adds the censoring sum's nc chunks. The
# message has q_words = ceil(d / (64 / b)) code words: 16 / 8 / 4 codes per word at b = 4 / 8 / 16, so
# the last word is full at d = 16 / 8 / 4 and a new, partly filled one starts at d = 17 / 9 / 5; a
# censored worker writes the header alone.
GRAPH_CQ = [
    (2, 3, 1),       # <1>: one coordinate, always extremal (its code is 0 or L); no interior worker
    (3, 7, 3),       # <1>: one partly filled word at every b
    (3, 20, 4),      # <1>: b = 16: one full word
    (3, 20, 5),      # <1>: b = 16: q_words 1 -> 2, one code in the last
    (3, 20, 8),      # <1>: b = 8: one full word; b = 16: two full words
    (3, 20, 9),      # <1>: b = 8: q_words 1 -> 2
    (4, 30, 16),     # <1>: b = 4: one full word
    (3, 30, 17),     # <1>: b = 4: q_words 1 -> 2
    (4, 40, 64),     # <1>: the top of nc = 1 (q_words 4 / 8 / 16): one full chunk of the sum; m < d
    (3, 80, 65),     # <2>: the first nc = 2 shape (q_words 5 / 9 / 17): a second chunk with one term
    (4, 150, 128),   # <2>: the top of nc = 2
    (3, 150, 129),   # <4>: the first: a third chunk with one term, a fourth of zeros
    (3, 280, 256),   # <4>: the top, and the top of the CQ kernels: every thread holds a term
]
assert GRAPH_CQ == H.QGADMM_GRAPH_SHAPES
GRAPH_CASES = [s + (b,) for s in GRAPH_CQ for b in BITS if (s, b) not in H.CQGADMM_DROPPED]
assert not H.CQGADMM_DROPPED   # every (shape, bits) pair runs


@pytest.mark.parametrize("n,m,d,bits", GRAPH_CASES)
def test_graph_cq(n, m, d, bits):
    _report("CQ-GADMM graph-CQ %s b=%d" % ((n, m, d), bits), run_graph(n, m, d, bits))


@pytest.mark.parametrize("n,m,d,bits", GRAPH_CASES)
def test_graph_cq_eager(n, m, d, bits):
    _report("CQ-GADMM graph-CQ eager %s b=%d" % ((n, m, d), bits), run_graph(n, m, d, bits, use_graph=False))


# ------------------------------------------------------------------------------------------------
# Persistent-CQ: pick_q_variant takes chain_persistent_cq_kernel<13> at d <= 52 and <16> at 53..64. Lane i
# reads the granule my_g = 1 + (i >> log2(64 / b)) that holds its code: a second granule starts at
# d = 17 / 9 / 5 for b = 4 / 8 / 16 -- behind a censored header it still holds an older tag and older
# codes, and must be neither waited for nor applied. The cap is PK = 8, so the longest reference has 24
# iterations.
PERSISTENT_CQ = [
    (2, 3, 1),       # QT = 13: one lane in use
    (3, 20, 4),      # QT = 13: b = 16: one full word
    (3, 20, 5),      # QT = 13: b = 16: a second granule, one lane in it
    (3, 20, 8),      # QT = 13: b = 8: one full word
    (3, 20, 9),      # QT = 13: b = 8: a second granule
    (4, 30, 16),     # QT = 13: b = 4: one full word
    (3, 30, 17),     # QT = 13: b = 4: a second granule
    (5, 40, 32),     # QT = 13
    (4, 40, 33),     # QT = 13
    (5, 60, 52),     # QT = 13: the top
    (5, 70, 53),     # QT = 16: the first
    (4, 40, 64),     # QT = 16: the top; every lane in use; m < d
]
assert PERSISTENT_CQ == H.QGADMM_PERSISTENT_SHAPES
PERSISTENT_XCD0 = [(3, 20, 9), (5, 70, 53)]   # also with XCD packing off
PERSISTENT_CASES = [s + (b, x) for s in PERSISTENT_CQ for b in BITS if (s, b) not in H.CQGADMM_DROPPED
                    for x in ((2, 0) if s in PERSISTENT_XCD0 else (2,))]


@pytest.mark.parametrize("n,m,d,bits,xcd", PERSISTENT_CASES)
def test_persistent_cq(n, m, d, bits, xcd):
    _report("CQ-GADMM persistent-CQ %s b=%d xcd=%d" % ((n, m, d), bits, xcd), run_persistent(n, m, d, bits, xcd))


# ------------------------------------------------------------------------------------------------
# A static chain that is not the identity: q_u01, c_sent and the message rows are indexed by worker id;
# slots, pos, heads / tails and left / right by chain position. Reversed at n = 4 (every head becomes a
# tail), a fixed permutation at n = 5.
PERMUTED = [((5, 40, 33), (2, 0, 4, 1, 3)), ((4, 30, 16), (3, 2, 1, 0))]
assert dict(PERMUTED) == H.QGADMM_PATHS


@pytest.mark.parametrize("shape,path", PERMUTED)
@pytest.mark.parametrize("engine", ["graph", "persistent"])
def test_permuted_static_chain(shape, path, engine):
    out = run_graph(*shape, 8, path=path) if engine == "graph" else run_persistent(*shape, 8, path=path)
    _report("CQ-GADMM %s-CQ chain %s %s b=8" % (engine, list(path), shape), out)


# ------------------------------------------------------------------------------------------------
# K4 primal residual (residual=True): the tails' edges, on public models -- the KEPT row of a censored
# worker.
@pytest.mark.parametrize("engine,n,m,d", [("graph", 4, 30, 16), ("graph", 3, 80, 65), ("persistent", 4, 30, 16),
                                          ("persistent", 5, 70, 53)])
def test_k4_residual(engine, n, m, d):
    out = run_graph(n, m, d, 8, residual=True) if engine == "graph" else run_persistent(n, m, d, 8, residual=True)
    assert "residual" in out
    _report("CQ-GADMM %s-CQ K4 residual %s b=8" % (engine, (n, m, d)), out)


# ------------------------------------------------------------------------------------------------
# Nobody ever sends: tau0 so large that the last threshold of the run is 1e6 times the largest s of the
# uncensored run (hp_reference.cqgadmm_silent_case). No public row, no dual and no neighbour copy may
# move; every solve returns the same theta; the graph engine writes headers only, the persistent kernel
# no code granule at all.
@pytest.mark.parametrize("bits", [4, 16])
@pytest.mark.parametrize("n,m,d", [(3, 20, 9), (4, 40, 64)])
@pytest.mark.parametrize("engine", ["graph", "persistent"])
def test_nobody_ever_sends(engine, n, m, d, bits):
    from gadmm_amd.algorithms import quantize as Q
    ref = H.cqgadmm_silent_case(n, m, d, bits, PK)[3]
    assert not ref.sent.any() and ref.censor[0] > 0
    eng = _engine(n, m, d, bits, PK, seed=ref.seed, censor=ref.censor)
    if engine == "graph":
        r = eng.run(stop_iter=PK)
        assert r.iters == PK and eng.graph_ok()
        last = PK
        msg = _host(eng.q_msg).view(np.uint64)
        assert (msg[:, 0] == np.uint64(Q.CENSORED_HEADER)).all() and not msg[:, 1:].any()
    else:
        r = eng.run_persistent(fetch_trace=True)
        assert eng.last_kernel.startswith("persistent-CQ") and r.iters == PK and r.done == 2
        last = eng.ctl_state()["iter"] - 1
        assert PK <= last <= PK + H.PERSISTENT_OVERRUN
        g = _host(eng._qg).view(np.uint32).reshape(n, -1, 4).astype(np.uint64)   # granules (tag, low, tag, high)
        assert g.shape[1] == Q.granules_per_row(d, bits)
        assert not g[:, 1:].any()   # the code granules still carry their reset tag (the table is zeroed once): none written
        assert (((g[:, 0, 3] << np.uint64(32)) | g[:, 0, 1]) == np.uint64(Q.CENSORED_HEADER)).all()   # every header: censored
        assert (g[:, 0, 0] == g[:, 0, 2]).all() and g[:, 0, 0].all()            # ... under a tag of this run
        ref = H.cqgadmm_silent_case(n, m, d, bits, last)[3]
    _table_is_the_references(eng, ref)
    assert not eng.sent_trace(PK).any()
    true, hat = _host(eng.theta_true), _host(eng.theta)
    eng.flush_duals()
    eng.stream.synchronize()
    mu = _host(eng.mu)
    for name, v in (("th_hat", hat), ("dual", mu)):
        assert not np.isnan(v).any() and np.array_equal(v, np.zeros_like(v)), (name, v)
    assert np.all(np.isfinite(true)) and not ref.hat.any() and not ref.dual.any()
    _report("CQ-GADMM %s-CQ nobody sends %s b=%d" % (engine, (n, m, d), bits),
            {"objective": ref.err_obj(eng.objective_trace(PK)) / ref.b_obj, "theta_true": ref.err_theta(true, last) / ref.b_theta})
    eng.close()


# ------------------------------------------------------------------------------------------------
# Sweep: chain_persistent_cq_sweep_kernel<13> / <16>, one batch per register class. Two censored members
# of different d within the class beside one uncensored member, which brings an all-zero table and is
# held to its Q reference (hp_reference.qgadmm_case).
SWEEP_BATCHES = [
    [(3, 20, 9, 8, True), (5, 60, 52, 4, True), (4, 30, 16, 16, False)],    # QT = 13: d <= 52
    [(5, 70, 53, 16, True), (4, 40, 64, 8, True), (4, 40, 64, 4, False)],   # QT = 16: d = 53..64
]


@pytest.mark.parametrize("batch", SWEEP_BATCHES, ids=["QT13", "QT16"])
def test_sweep_mixed_members(batch):
    from gadmm_amd.engine.quant_sweep import QuantSweepEngine
    sw = QuantSweepEngine([_engine(n, m, d, bits, PK, censor=None if cens else False) for n, m, d, bits, cens in batch])
    runs = sw.run()
    assert sw.last_kernel == "persistent-CQ-sweep(K=%d)" % len(batch), sw.last_kernel
    for (n, m, d, bits, cens), mem, r in zip(batch, sw.members, runs):
        assert r.iters == PK and r.done == 2, (r.iters, r.done)
        case = None if cens else (lambda last, a=(n, m, d, bits): H.qgadmm_case(*a, last))
        out = _persistent_ratios(mem, n, m, d, bits, None, False, case)
        if not cens:
            assert mem.sent_trace(PK).all()   # a zero table: everybody always sends
        _report("CQ-GADMM CQ-sweep member %s b=%d %s" % ((n, m, d), bits, "censored" if cens else "uncensored"), out)
    sw.close()
