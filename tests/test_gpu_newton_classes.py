"""The exact-logistic (Newton) kernels against a long-double reference, at every edge of their layouts.

Three kernels solve a worker's prox exactly: the graph engine's phase kernel (chain_newton.hip: 512
threads per worker, MFMA Hessian, 4 x 4-block in-place Gauss-Jordan inverse; d, m <= 64) and the two
persistent kernels of chain_persistent_newton.hip (d, m <= 52, quad layout QT = 13): the one-wave
solver with a 4-wave crew (GADMM_NEWTON_REC=0) and the default four-wave chord-step pipeline. The rest
of the suite runs the persistent ones at (24, 50, 50) only and compares objective traces with the torch
path at rtol 1e-12; here every kernel runs K = 20 iterations (tol = 0, obj0 = 0, max_iter = K: no outer
stop rule) at the shapes where padding, tile tails and pivot blocks change, and theta, the duals and
the K objectives are compared with tests/hp_reference.py:gadmm_logistic_newton, the converged prox in
long double. Per quantity (theta / max|theta|, dual / (rho max|theta|), each objective relative)

    err <= 8 * max(e, max(d, m, 16) * 2^-53, tau(c) / max|theta|)

e: the distance of the float64 NumPy run of the same recurrence (stop tolerance 1e-13, chord threshold
c) from the long-double one; tau(c) = c / (1 - c) * 1e-13 * max(1, max|x|): what the stop rule admits
after a chord-accepted last step (0 at c = 0, where Newton converges quadratically). The persistent
kernels follow another refresh schedule under the same two rules (their inverse is built at the
previous iterate, refreshes are lagged or urgent), hence the same bound. Every test also asserts which
kernel ran, ctl inner_fail == 0, 1 <= inner_iters < 50 and, at c = 0, each worker's step count of its
last solve within +-1 of the float64 reference's (a stop test can tie).
Each test prints err / bound; profiles/newton_classes/README.md records the measured table.
The "K4 primal residual" section runs every kernel once more with ``residual=True`` at chord 0 and holds
the residual sums and per-worker rows to hp_reference.chain_residual (profiles/residual_classes/README.md).

Run with: pytest -m gpu tests/test_gpu_newton_classes.py -s
"""
import numpy as np
import pytest
import torch

import hp_reference as H
from test_gpu_dispatch_classes import _residual_ratios

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
K = H.K_ITERS
BLOCK = 4  # iterations per graph replay: divides K, so the graph engine replays every iteration
assert K % BLOCK == 0
CHORD_GRAPH, CHORD_PERSISTENT = 0.02, 0.3  # the engine's defaults (chord=None)
assert (0.0, CHORD_GRAPH, CHORD_PERSISTENT) == H.NEWTON_CHORDS
# chain_persistent_newton.hip: a solve of more chord steps than this asks for a background refresh
# (bg_steps of either kernel at the engine's default max_inner; GADMM_NEWTON_BG moves the pipeline's)
BG_STEPS = {"one-wave": 1, "pipeline": 4}


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached case's arrays are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _report(tag, ratios):
    """Print err / bound of every quantity, then assert all of them <= 1."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _newton_engine(n, m, d, chord, residual=False):
    """As test_gpu_dispatch_classes._logistic_engine, with exact local solves. ``chord`` None: the
    engine's defaults, 0.02 for the phase kernel and 0.3 for the persistent ones."""
    from gadmm_amd.engine.chain_engine import NativeChainEngine
    from gadmm_amd.parallel.topology import Placement
    ref = H.newton_case(n, m, d)
    eng = NativeChainEngine(_dev(ref.X), _dev(ref.y), list(range(n)), n, "logistic", rho=ref.rho, obj0=0.0, tol=0.0,
                            max_iter=K, lam=ref.lam, local_solver="newton", chord=chord, block=BLOCK,
                            residual=residual)
    eng.set_path(list(range(n)), Placement.contiguous(n, 1), 0)
    eng.reset()
    return eng


def _state(eng):
    """(theta, mu once the heads' lazy last dual update is applied, the K objectives), on the host."""
    th = _host(eng.local_theta())
    eng.flush_duals()
    eng.stream.synchronize()
    mu = _host(eng.mu)
    tr = np.array(eng.objective_trace(K))
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(tr))
    return th, mu, tr


def _ratios(state, ref, last):
    th, mu, tr = state
    return {"objective": ref.err_obj(tr) / ref.b_obj, "theta": ref.err_theta(th, last) / ref.b_theta,
            "dual": ref.err_dual(mu) / ref.b_dual}


def _check_inner(eng, ref, last, tag, bg=None):
    """No local solve of the whole run reached the step cap unconverged; the last solve of every
    worker took 1 .. 49 steps and, without a chord rule, the float64 reference's count +-1. ``bg``
    (persistent kernels): also print how many of those last solves asked for a background refresh."""
    n = ref.theta.shape[1]
    assert eng.ctl_state()["inner_fail"] == 0, eng.ctl_state()
    inner = _host(eng.inner_iters)[:n]
    want = ref.steps64[last - 1]
    asked = "" if bg is None else "; %d of %d took more than %d (background refresh)" % (int(np.sum(inner > bg)), n, bg)
    print("%s: Newton steps of the last solves %s (float64 reference %s)%s"
          % (tag, inner.tolist(), want.tolist(), asked))
    assert inner.min() >= 1 and inner.max() < H.NEWTON_MAX, inner
    if ref.chord == 0.0:
        assert np.all(np.abs(inner - want) <= 1), (inner, want)
    return inner


def run_graph(n, m, d, chord, use_graph=True, eng=None, residual=False):
    """The phase kernel, replayed as a graph or launched eagerly: K iterations. ``residual``: the engine
    also emits the K4 primal residual, and its ratios join the returned ones."""
    c = CHORD_GRAPH if chord is None else chord
    ref = H.newton_case(n, m, d, K, c)
    own = eng is None
    if own:
        eng = _newton_engine(n, m, d, chord, residual=residual)
    assert eng.chord == c
    r = eng.run(stop_iter=K, use_graph=use_graph)
    assert r.iters == K and eng.ctl_state()["iter"] == K + 1, (r.iters, r.done, eng.ctl_state())
    assert r.replays == K // BLOCK and (eng.graph_ok() or not use_graph)
    _check_inner(eng, ref, K, "newton graph c=%g %s" % (c, (n, m, d)))
    st = _state(eng)
    out = _ratios(st, ref, K)
    if residual:
        out.update(_residual_ratios(eng, ref))  # sums and per-worker rows; heads exactly 0
    if own:
        eng.close()
    return out, st


def run_persistent(n, m, d, chord, kernel, eng=None, bg=None, residual=False):
    """One persistent launch; ``kernel``: "one-wave" or "pipeline", chosen by the environment the caller
    set. The kernel learns the cap's stop decision ``lag`` iterations late and stops after iteration
    ctl.iter - 1: theta and mu are compared with the reference run that far."""
    c = CHORD_PERSISTENT if chord is None else chord
    own = eng is None
    if own:
        eng = _newton_engine(n, m, d, chord, residual=residual)
    assert eng.chord_persistent == c and eng.persistent_eligible()
    r = eng.run_persistent()
    assert eng.last_kernel == "per-worker-newton(%s)" % kernel, eng.last_kernel
    last = eng.ctl_state()["iter"] - 1
    assert r.iters == K and K <= last <= K + H.PERSISTENT_OVERRUN, (r.iters, r.done, last)
    ref = H.newton_case(n, m, d, last, c)
    _check_inner(eng, ref, last, "newton %s c=%g %s" % (kernel, c, (n, m, d)), BG_STEPS[kernel] if bg is None else bg)
    st = _state(eng)
    out = _ratios(st, ref, last)
    if residual:
        out.update(_residual_ratios(eng, ref))  # sums and per-worker rows; heads exactly 0
    if own:
        eng.close()
    return out, st, last


# ------------------------------------------------------------------------------------------------
# Graph engine: chain_phase_logistic_newton (chain_newton.hip), d, m <= 64. X rows are padded to
# DP = (d + 3) & ~3, the Hessian is a 4 x 4 grid of 16 x 16 MFMA tiles over samples in chunks of 4, the
# inverse walks (d + 3) / 4 pivot blocks of 4 with identity padding up to 64.
NEWTON_GRAPH = [
    (2, 1, 1),       # the smallest: every degree is 1; one pivot block, three of its four pivots padding
    (3, 5, 3),       # odd n, the last worker is a head
    (3, 7, 5),       # a second pivot block with one live column; m no multiple of the MFMA K = 4
    (4, 17, 16),     # the 16-wide MFMA tile boundary from below in d, one past it in m
    (3, 15, 17),     # ... and from above in d
    (5, 36, 34),     # real-shaped (Derm 36 x 34)
    (3, 52, 52),     # the top of the persistent kernels' range
    (3, 40, 53),     # graph only: persistent_eligible() is False through d
    (3, 53, 40),     # graph only: ... and through m
    (4, 7, 61),      # m < d: the Hessian is SPD only through the shift; row stride padded 61 -> 64
    (2, 3, 64),      # m < d at the top of the d range
    (3, 63, 63),     # one short of the full 64 x 64 register rows
    (3, 64, 64),     # full register rows
]
assert NEWTON_GRAPH == H.NEWTON_GRAPH_SHAPES


@pytest.mark.parametrize("chord", [0.0, None])
@pytest.mark.parametrize("n,m,d", NEWTON_GRAPH)
def test_newton_graph_engine(n, m, d, chord):
    _report("newton graph chord=%s %s" % (chord, (n, m, d)), run_graph(n, m, d, chord)[0])


@pytest.mark.parametrize("chord", [0.0, None])
def test_newton_eager_phases(chord):
    _report("newton eager chord=%s (3, 5, 3)" % (chord,), run_graph(3, 5, 3, chord, use_graph=False)[0])


@pytest.mark.parametrize("n,m,d", [(3, 40, 53), (3, 53, 40)])
def test_newton_persistent_stops_at_52(n, m, d, monkeypatch):
    """newton_variant (chain_persistent_newton.hip) takes d, m <= 4 QT = 52 only, for either kernel;
    run_graph above shows that these shapes still solve natively."""
    for rec in ("0", "1"):
        monkeypatch.setenv("GADMM_NEWTON_REC", rec)
        eng = _newton_engine(n, m, d, None)
        assert not eng.persistent_eligible()
        eng.close()


# ------------------------------------------------------------------------------------------------
# Persistent kernels (chain_persistent_newton.hip): quad layout QT = 13, lane (i, q) holds columns
# j = q (mod 4) of row i, so a row of 52 is full, 49 leaves three lanes of the last quad column padded,
# 1 / 3 / 5 nearly all of them; the crew's Gauss-Jordan and MFMA Hessian pad to 64 as the graph kernel's.
NEWTON_PERSISTENT = [
    (2, 1, 1),       # a two-worker chain: one head, one tail, no interior worker
    (3, 5, 3), (3, 7, 5), (4, 17, 16), (3, 15, 17), (5, 36, 34),
    (4, 12, 49),     # m < d, d one past a multiple of 4 and of 16
    (3, 40, 52),     # the top through d
    (3, 52, 20),     # the top through m
    (3, 52, 52),     # full quad rows
]
assert NEWTON_PERSISTENT == H.NEWTON_PERSISTENT_SHAPES
KERNEL_OF_REC = {"0": "one-wave", "1": "pipeline"}


@pytest.mark.parametrize("chord", [0.0, None])
@pytest.mark.parametrize("rec", ["0", "1"])
@pytest.mark.parametrize("n,m,d", NEWTON_PERSISTENT)
def test_newton_persistent_kernel(n, m, d, rec, chord, monkeypatch):
    monkeypatch.setenv("GADMM_NEWTON_REC", rec)
    out, _, last = run_persistent(n, m, d, chord, KERNEL_OF_REC[rec])
    _report("newton %s chord=%s %s (stopped after %d)" % (KERNEL_OF_REC[rec], chord, (n, m, d), last), out)


# ------------------------------------------------------------------------------------------------
# K4 primal residual (residual=True, what every solve a user runs has on): the tails' branch of the phase
# kernel and of both persistent kernels, the K sums and the per-worker rows against
# hp_reference.chain_residual of the long-double theta history (tests/test_gpu_dispatch_classes.py, "K4
# primal residual"). At chord = 0 only: the bound of a DIFFERENCE of thetas under the chord rule's
# admitted truncation is not derived, and the residual branch does not depend on the chord.
@pytest.mark.parametrize("n,m,d", NEWTON_GRAPH)
def test_residual_newton_graph_engine(n, m, d):
    _report("K4 newton graph %s" % ((n, m, d),), run_graph(n, m, d, 0.0, residual=True)[0])


@pytest.mark.parametrize("rec", ["0", "1"])
@pytest.mark.parametrize("n,m,d", NEWTON_PERSISTENT)
def test_residual_newton_persistent_kernel(n, m, d, rec, monkeypatch):
    monkeypatch.setenv("GADMM_NEWTON_REC", rec)
    out, _, last = run_persistent(n, m, d, 0.0, KERNEL_OF_REC[rec], residual=True)
    _report("K4 newton %s %s (stopped after %d)" % (KERNEL_OF_REC[rec], (n, m, d), last), out)


# The pipeline kernel's schedule and arithmetic switches (read per launch), one per test, at the default
# chord 0.3: they change which inverse a chord step uses or how sigma is evaluated, never the fixed
# point. Whether a 20-iteration run at these shapes takes an urgent or a background refresh at all is
# not observable from here (the printed step counts say only when the LAST solve asked for one).
KNOBS = [
    {"GADMM_NEWTON_RLAG": "1", "GADMM_NEWTON_BG": "1"},  # ask after any solve of > 1 step, adopt at the next iteration
    {"GADMM_NEWTON_URGENT_NS": "1"},                     # urgent refreshes by one Newton-Schulz step
    {"GADMM_NEWTON_FASTSIGM": "0"},                      # exp-based sigmoid in the chord steps
    {"GADMM_NEWTON_POSTFENCE": "1"},                     # fenced LDS posts between the pipeline's waves
]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "+".join(sorted(k)))
@pytest.mark.parametrize("n,m,d", [(3, 5, 3), (5, 36, 34), (3, 52, 52)])
def test_newton_pipeline_knobs(n, m, d, knobs, monkeypatch):
    monkeypatch.setenv("GADMM_NEWTON_REC", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    out, _, last = run_persistent(n, m, d, None, "pipeline", bg=int(knobs.get("GADMM_NEWTON_BG", BG_STEPS["pipeline"])))
    _report("newton pipeline %s %s (stopped after %d)" % (" ".join("%s=%s" % kv for kv in knobs.items()), (n, m, d),
                                                          last), out)


# ------------------------------------------------------------------------------------------------
# Stale state: a second solve on the same engine, after reset(), must not see the first one's cached
# inverses (graph: the per-worker store keyed by a valid flag; pipeline: the refresh images in
# LogiArgs::scratch) nor anything else of it. Both runs are deterministic, so: bit for bit.
def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


def test_newton_graph_second_solve_is_identical():
    n, m, d = 5, 36, 34
    eng = _newton_engine(n, m, d, CHORD_GRAPH)
    out1, st1 = run_graph(n, m, d, CHORD_GRAPH, eng=eng)
    eng.reset()
    out2, st2 = run_graph(n, m, d, CHORD_GRAPH, eng=eng)
    eng.close()
    _report("newton graph, first solve %s" % ((n, m, d),), out1)
    _report("newton graph, second solve %s" % ((n, m, d),), out2)
    assert _same_bits(st1, st2)


def test_newton_pipeline_second_solve_is_identical(monkeypatch):
    monkeypatch.setenv("GADMM_NEWTON_REC", "1")
    n, m, d = 5, 36, 34
    eng = _newton_engine(n, m, d, CHORD_PERSISTENT)
    out1, st1, last1 = run_persistent(n, m, d, CHORD_PERSISTENT, "pipeline", eng=eng)
    eng.reset()
    out2, st2, last2 = run_persistent(n, m, d, CHORD_PERSISTENT, "pipeline", eng=eng)
    eng.close()
    _report("newton pipeline, first solve %s" % ((n, m, d),), out1)
    _report("newton pipeline, second solve %s" % ((n, m, d),), out2)
    assert last1 == last2 and _same_bits(st1, st2)
