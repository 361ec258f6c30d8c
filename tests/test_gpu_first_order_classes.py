"""Every dispatch class of the first-order baseline engines against a long-double reference.

The comparators every E-series figure plots GADMM against -- GD, DGD, LAG-PS, LAG-WK, cyclic and
randomized IAG, dual averaging in Gauss-Seidel and Jacobi order -- run on two engines:

* the persistent engine (csrc/kernels/first_order.hip, d <= 128), six single-GPU instantiations
  ``fo_persistent_kernel<NC, MC, false>``: NC = 1 at d <= 64, 2 at d <= 128; MC = 0 for the linear model
  and for logistic shards with m > 128 (one wave per row), 1 at logistic m <= 64, 2 at m <= 128. The rest
  of the suite launches <1,0> (linear) and <1,1> at n = 24, d = m = 50 and nothing else;
* the stream-ordered large-d engine (csrc/kernels/first_order_big.hip), which works in 128-element
  blocks and whose one recorded bug was a block-boundary bug.

Each case runs K = 80 iterations (more than the 67 IAG table slots and the 64 objective-ring slots;
LAG takes no decision before iteration 11) with no stop rule and is compared with
tests/hp_reference.py:first_order, plain NumPy in long double following the torch path line for line.
The scalar inputs (step, Hmax_n^2, LAG's threshold factor, IAG's schedule) are computed once in float64
NumPy and handed to reference and engine alike. Asserted per case:

* ``iters == K``, not converged (a timeout raises);
* objective trace and final theta: ``err <= 8 * max(e64, max(d, m_logistic, n, 16) * 2^-53)``, e64 the
  distance of the same recurrence in float64 NumPy from its long-double run (``hp_reference.bound``);
* server algorithms: every worker's row of theta bit-identical (the kernel header promises it);
* LAG: the per-iteration upload counts and their total equal the reference's exactly --
  tests/test_hp_reference_cpu.py holds every LAG case to a trigger margin >= 1e-9 and to identical
  decisions in both precisions, and to runs that mix no / partial / full uploads;
* the kernel instantiation that ran (``gadmm_fo_kernel_class``, the launcher's own two expressions).

Each parameter list names the threshold that puts its shape in its class. Each test prints
err / bound; profiles/first_order_classes/README.md records the measured table.

Run with: pytest -m gpu tests/test_gpu_first_order_classes.py -s
"""
import numpy as np
import pytest
import torch

import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
K = H.FO_K
SERVER = ("GD", "LAG-PS", "LAG-WK", "cIAG", "R-IAG")
TIMEOUT_S = 10.0  # the persistent kernel's own deadline: a missed granule ends the launch, not the suite
_ENGINES = {}


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cases' arrays are frozen


def _report(tag, ratios):
    """Print err / bound of every quantity, then assert all of them <= 1."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _engine(case, big):
    """The engine of a shape's model on the device, shared by the shape's algorithms (an engine is made
    to be re-used across runs: its tags are epoch-salted)."""
    key = (case.kind, case.n, case.m, case.d, big)
    if key not in _ENGINES:
        from gadmm_amd.models import LinearRegression, LogisticRegression
        if case.kind == "linear":
            model = LinearRegression(_dev(case.X), _dev(case.y))
        else:
            model = LogisticRegression(_dev(case.X), _dev(case.y), lam=case.lam)
        if big:
            from gadmm_amd.engine.first_order_big import FirstOrderBigEngine
            _ENGINES[key] = FirstOrderBigEngine(model, n_total=case.n)
        else:
            from gadmm_amd.engine.first_order import FirstOrderEngine
            alg = "DGD" if case.n > 256 else "GD"
            assert FirstOrderEngine.eligible(model, None, case.n, alg=alg)
            _ENGINES[key] = FirstOrderEngine(model)
    return _ENGINES[key]


def _run(case, big=False, obj0=0.0, tol=None, **kw):
    a = dict(case.args)
    if "hsq" in a:
        a["hsq"] = _dev(a["hsq"])
    step = a.pop("step")
    if not big:
        kw["timeout_s"] = TIMEOUT_S
    return _engine(case, big).run(case.alg, K, step, obj0, tol, case.faithful, **a, **kw)


def _check(tag, case, out, kernel=None, big=False):
    assert out["iters"] == K and not out["converged"] and len(out["obj"]) == K, (out["iters"], out["converged"])
    th = out["theta"].cpu().numpy()
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(out["obj"]))
    if case.variant in SERVER:
        assert th.shape == ((1, case.d) if big else (case.n, case.d))
        assert np.array_equal(th, np.broadcast_to(th[0], th.shape)), "replicated theta differs between workers"
    else:
        assert th.shape == (case.n, case.d)
    if case.cnt is not None:
        assert np.array_equal(out["cnt"], case.cnt), (np.nonzero(out["cnt"] != case.cnt)[0][:5], case.margin)
        assert out["uploads"] == case.uploads
    else:
        assert not np.any(out["cnt"])
    if big:
        assert out["engine"] == "native-big"
    else:
        assert out["kernel"] == kernel, (out["kernel"], kernel)
    _report(tag, {"objective": case.err_obj(out["obj"]) / case.b_obj, "theta": case.err_theta(th) / case.b_theta})


def _cases(shapes):
    """(shape..., class, algorithm) for every algorithm run at the shape's worker count."""
    return [s + (a,) for s in shapes for a in H.fo_algs(s[0])]


# ------------------------------------------------------------------------------------------------
# Persistent engine, linear: MC = 0 always; gadmm_fo_launch takes NC = 1 at d <= 64, NC = 2 at d <= 128.
# The worker count moves the server step: wave wv owns the table rows wv, wv + 4, ..., fetches the
# changed ones in batches of RB = 8 and keeps a 64-bit changed-row mask (so n <= 256); the monitor's
# lanes take 64 workers per pass.
LINEAR_PERSISTENT = [
    (2, 3, 1, "fo<1,0>"),      # d = 1
    (3, 7, 3, "fo<1,0>"),
    (5, 70, 64, "fo<1,0>"),    # d <= 64: the top of NC = 1
    (4, 80, 65, "fo<2,0>"),    # the first NC = 2 shape
    (3, 150, 128, "fo<2,0>"),  # d <= 128: the top of NC = 2 and of the engine
    (1, 5, 3, "fo<1,0>"),      # n = 1: DGD's n == 1 branch, dual averaging with no neighbour (no LAG-WK)
    (33, 8, 4, "fo<1,0>"),     # wave 0 owns 9 rows > RB: fetch_rows runs in two batches
    (65, 6, 3, "fo<1,0>"),     # n > 64: the second pass of the monitor's lane loop (R-IAG, not cyclic)
    (253, 4, 2, "fo<1,0>"),    # waves own 64 / 63 / 63 / 63 rows: ~0ull next to (1ull << 63) - 1
    (256, 4, 2, "fo<1,0>"),    # the largest server run: every wave's mask is full
]
assert [s[:3] for s in LINEAR_PERSISTENT] == H.FO_LINEAR_SHAPES


@pytest.mark.parametrize("n,m,d,kernel,alg", _cases(LINEAR_PERSISTENT))
def test_persistent_linear(n, m, d, kernel, alg):
    case = H.first_order_case("linear", alg, n, m, d)
    _check("persistent linear %s %s %s" % ((n, m, d), kernel, alg), case, _run(case), kernel)


# DGD and dual averaging read only their chain neighbours: no changed-row mask, no 256 limit.
@pytest.mark.parametrize("alg", ["DGD", "DualAvg", "DualAvg-J"])
def test_persistent_linear_past_the_server_limit(alg):
    n, m, d = H.FO_LINEAR_WIDE
    case = H.first_order_case("linear", alg, n, m, d)
    _check("persistent linear %s fo<1,0> %s" % ((n, m, d), alg), case, _run(case), "fo<1,0>")


def test_server_algorithms_leave_the_engine_above_256_workers():
    """n = 257: the server algorithms are not eligible (the 64-bit changed-row mask of four waves) and
    ``backend="auto"`` takes the torch path, which the reference reproduces."""
    from gadmm_amd.algorithms import gradient_descent
    from gadmm_amd.engine.first_order import FirstOrderEngine
    n, m, d = H.FO_LINEAR_WIDE
    case = H.first_order_case("linear", "GD", n, m, d)
    model = _engine(H.first_order_case("linear", "DGD", n, m, d), False).model
    assert not FirstOrderEngine.eligible(model, None, n, alg="GD")
    assert not FirstOrderEngine.eligible(model, None, n, alg="LAG-WK")
    assert FirstOrderEngine.eligible(model, None, n, alg="DGD")
    r = gradient_descent(model, list(range(n)), n, K, 0.0, case.step0, backend="auto")
    assert "engine" not in r.extra and len(r.obj) == K
    _report("torch path linear %s GD" % ((n, m, d),), {"objective": case.err_obj(r.obj) / case.b_obj})


# ------------------------------------------------------------------------------------------------
# Persistent engine, logistic: fo_mc picks MC = 1 at m <= 64 and MC = 2 at m <= 128 (z = X theta from the
# transposed shard, lanes own samples), MC = 0 at m > 128 (one wave per row). <1,2> is the class whose
# z needs 4 * MC * 64 doubles of reduction scratch where the d class alone would give 4 * NC * 64.
LOGISTIC_PERSISTENT = [
    (3, 5, 3, "fo<1,1>"),
    (3, 64, 20, "fo<1,1>"),     # m <= 64: the top of MC = 1
    (3, 65, 20, "fo<1,2>"),     # the first MC = 2 shape, d <= 64
    (3, 128, 64, "fo<1,2>"),    # m <= 128 and d <= 64: the top of both
    (4, 70, 60, "fo<1,2>"),     # the same class with a server table of 240 doubles
    (3, 129, 20, "fo<1,0>"),    # m > 128: one wave per row
    (2, 60, 65, "fo<2,1>"),
    (2, 66, 128, "fo<2,2>"),    # 144 KB of LDS: must not fall back
    (2, 130, 70, "fo<2,0>"),
    (33, 6, 3, "fo<1,1>"),      # more table rows per wave than RB, logistic
]
assert [s[:3] for s in LOGISTIC_PERSISTENT] == H.FO_LOGISTIC_SHAPES


@pytest.mark.parametrize("n,m,d,kernel,alg", _cases(LOGISTIC_PERSISTENT))
def test_persistent_logistic(n, m, d, kernel, alg):
    case = H.first_order_case("logistic", alg, n, m, d)
    if (n, m, d) == (2, 66, 128):
        from gadmm_amd.engine.first_order import ALG_IDS
        from gadmm_amd.ops import native
        lds = native.require().gadmm_fo_lds(1, ALG_IDS[case.alg], n, d, m)
        assert 128 * 1024 < lds <= 159 * 1024, lds  # eligible()'s limit: the case cannot fall back
    _check("persistent logistic %s %s %s" % ((n, m, d), kernel, alg), case, _run(case), kernel)


def test_kernel_class_query_follows_the_thresholds():
    from gadmm_amd.ops import native
    q = native.require().gadmm_fo_kernel_class
    for d, nci in ((1, 0), (64, 0), (65, 1), (128, 1)):
        assert q(0, d, 5) == q(0, d, 500) == 3 * nci           # linear: MC = 0 whatever m
        for m, mc in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 0)):
            assert q(1, d, m) == 3 * nci + mc, (d, m)


# ------------------------------------------------------------------------------------------------
# faithful=False: GD and DGD start from the real gradients, LAG-PS drops the forced refresh of worker 0
@pytest.mark.parametrize("alg", H.FO_ALGS)
@pytest.mark.parametrize("kind,n,m,d,kernel", [("linear", 3, 7, 3, "fo<1,0>"), ("logistic", 3, 5, 3, "fo<1,1>")])
def test_persistent_not_faithful(kind, n, m, d, kernel, alg):
    case = H.first_order_case(kind, alg, n, m, d, faithful=False)
    _check("persistent %s %s faithful=0 %s" % (kind, (n, m, d), alg), case, _run(case), kernel)


# ------------------------------------------------------------------------------------------------
# A live stop rule. obj0 = the long-double objective after iteration 80, tol = the midpoint of the gaps
# of iterations 39 and 40 (tests/test_hp_reference_cpu.py: the gaps decrease strictly and the tolerance
# is further from both than the bound reaches). theta is not compared: workers may run one iteration
# past the stop, by design.
@pytest.mark.parametrize("alg,n,m,d,faithful", H.FO_LIVE_STOP)
def test_live_stop_rule(alg, n, m, d, faithful):
    case = H.first_order_case("linear", alg, n, m, d, faithful=faithful)
    obj0, tol, gaps = H.fo_live_stop(case)
    k = H.FO_LIVE_STOP_AT
    assert np.all(np.diff(gaps[:k]) < 0) and (gaps[k - 2] - gaps[k - 1]) / gaps[k - 2] > 1e-6
    big = d > 128
    out = _run(case, big=big, obj0=obj0, tol=tol, **({"block": 16} if big else {}))
    assert out["converged"] and out["iters"] == k and len(out["obj"]) == k, (out["converged"], out["iters"])
    _report("live stop %s %s" % ((n, m, d), alg), {"objective": case.err_obj(out["obj"]) / case.b_obj})


# ------------------------------------------------------------------------------------------------
# Large-d engine (linear only; dispatched at d > 128): vectors and objective partials in 128-element
# blocks, the Grams block-packed. block = 16 iterations per host look divides K.
BIG = [
    (1, 140, 129),   # one element in the second block; n = 1 (no LAG-WK)
    (3, 140, 129),
    (3, 270, 256),   # two full blocks
    (3, 270, 257),   # one element in the third
    (3, 60, 50),     # run directly below the dispatch threshold, as the goldens do: one partial block
]
assert BIG == H.FO_BIG_SHAPES


@pytest.mark.parametrize("n,m,d,alg", _cases(BIG))
def test_big_linear(n, m, d, alg):
    case = H.first_order_case("linear", alg, n, m, d)
    _check("big linear %s %s" % ((n, m, d), alg), case, _run(case, big=True, block=16), big=True)


@pytest.mark.parametrize("alg", ["GD", "LAG-PS"])
def test_big_linear_block_not_dividing_the_run(alg):
    """block = 7 does not divide K = 80: the last host block is shorter than the others."""
    case = H.first_order_case("linear", alg, 3, 140, 129)
    _check("big linear (3, 140, 129) block=7 %s" % alg, case, _run(case, big=True, block=7), big=True)
