"""Q-GGADMM on the persistent graph kernel with a quantized exchange (csrc/kernels/graph_quant.hip) on the
MI355X.

The kernel is held to the long-double quantized graph recurrence of tests/hp_qggadmm.py: the true theta,
the public models, the per-worker duals, the objective trace, the tails' K4 rows and R of the last
messages under ``hp_reference.bound`` (err / bound <= 1), the codes of the last messages and their packed
words EXACTLY. On a chain graph it is held bit for bit to ``chain_admm(quantize=)`` on the per-worker
persistent Q kernel (the same arithmetic in the same order).

Shapes of the class test (hp_qggadmm.CASES; bits 4, 8 and 16 unless noted), no stop rule, a cap of 8:

    one edge, d = 1                       one coordinate, always extremal
    one edge, d = 16 / 17 (b = 4),        the last code word full, then one code in a new word
      8 / 9 (b = 8), 4 / 5 (b = 16)
    ring_graph(4), d = 7                  DK = 2, several heads
    grid_graph(2, 3), d = 50              DK = 4, the workload's d
    K(2, 3), d = 52                       the top of the 13-column register class
    K(4, 4), d = 53                       the bottom of the 16-column register class
    star_graph(8, 0), d = 64              DK = 8; G = 9 granules at b = 8, 17 at b = 16
    star of 12, hub 5, d = 50 (b = 8)     the hub a tail, its id in mid-order, heads = the leaves
    star of 20, d = 7, the hub a head;    degree 19: two poll groups, on both exit paths (the head's exit
      and the hub a tail (b = 8)          poll, the tail's abandoned wait)

Every run has ``timeout_s=5``. No test provokes a timeout, a fault or a hang.

Run with: pytest -m gpu tests/test_gpu_qggadmm.py -s
"""
import numpy as np
import pytest
import torch

import hp_qggadmm as Q
import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
CAP = Q.CAP
OPTS = {"timeout_s": 5.0}


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


def _report(tag, ratios):
    """Print err / bound of every quantity, then assert all of them <= 1."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _class_bound(deg):
    return min([k for k in (2, 4, 8, 16) if k >= deg] or [16 * ((deg + 15) // 16)])


_MODELS = {}


def _model(name):
    """A case's model on the device, built once and shared (its engines are cached on it)."""
    if name not in _MODELS:
        from gadmm_amd.models import LinearRegression
        g, X, y, rho = Q.case_data(name)
        m = LinearRegression(_dev(X), _dev(y))
        _MODELS[name] = (g, m, rho, m.optimum())
    return _MODELS[name]


def _e1(n):
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.oracle.reference import opt_linear
    key = ("e1", n)
    if key not in _MODELS:
        ds = linear_synthetic(n)
        Xf, yf = ds.stacked()
        _MODELS[key] = (LinearRegression(ds.X.to(DEV), ds.y.to(DEV)), opt_linear(Xf.numpy(), yf.numpy()))
    return _MODELS[key]


def _messages(eng):
    """``(R (n,) float64, code words (n, G - 1) uint64)`` of the last messages in the engine's table."""
    msg = np.ascontiguousarray(_host(eng.q_msg)).view(np.uint64)
    return np.ascontiguousarray(msg[:, 0]).view(np.float64), msg[:, 1:]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits", Q.cases())
def test_native_against_long_double_reference(name, bits):
    """No stop rule (tol = 0), a cap of 8: the cap's decision reaches the workers ``lag`` iterations late,
    the kernel stops after iteration ctl.iter - 1 = last and the state is compared with the reference run
    that far; the objective trace and the K4 rows cover iterations 1..8."""
    from gadmm_amd.algorithms import quantize as Z
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, X, y, rho = Q.case_data(name)
    d = X.shape[2]
    seed = Q.seed_for(name, bits)
    eng = NativeGraphEngine(_dev(X), _dev(y), g, rho, 0.0, 0.0, CAP, quant=(bits, seed))
    assert eng.eligible(), eng.refusal()
    r = eng.run(timeout_s=5.0)
    last = eng.ctl_state()["iter"] - 1
    assert r.done == 2 and r.iters == CAP and CAP <= last <= CAP + Q.OVERRUN, (r.iters, r.done, last)
    assert eng.last_placed == 2, eng.last_placed
    assert eng.last_kernel == "persistent-graph-Q(deg<=%d,b=%d)" % (_class_bound(g.max_degree), bits), eng.last_kernel
    ref = Q.case(name, bits, last)[4]
    th, hat, mu = _host(eng.theta_true), _host(eng.theta), _host(eng.mu)
    tr, _ = eng.traces(CAP)
    rows = _host(eng.rres[:CAP])
    R, words = _messages(eng)
    for a in (th, hat, mu, tr, rows, R):
        assert np.all(np.isfinite(a))
    tails = ref.tails[:CAP]
    assert np.all(rows[~tails] == 0.0), "a head's K4 row is not 0"
    assert words.shape == (g.n, Z.words_per_row(d, bits))
    codes = ref.codes[last - 1]
    assert np.array_equal(Z.unpack_codes(words, bits, d), codes), "codes of the last messages"
    assert np.array_equal(words, Z.pack_codes(codes, bits)), "packed words of the last messages"
    _report("qggadmm native %s b=%d (last=%d, %s)" % (name, bits, last, eng.last_kernel), {
        "theta": ref.err_theta(th, last) / ref.b_theta, "hat": ref.err_hat(hat) / ref.b_hat,
        "dual": ref.err_dual(mu) / ref.b_dual, "objective": ref.err_obj(tr) / ref.b_obj,
        "residual rows": ref.err_res_w(rows) / ref.b_res_w, "R": ref.err_R(R) / ref.b_R})
    eng.close()


@pytest.mark.parametrize("n", [8, 24])
def test_chain_graph_bitwise_against_chain_q_kernel(n, monkeypatch):
    """E1 data, rho = 3, b = 8, to 1e-4: the chain graph on the graph Q kernel against ``chain_admm(quantize=)``
    on the per-worker persistent Q kernel: the same iteration count, a bit-identical objective trace and
    bit-identical public models."""
    from gadmm_amd.algorithms import chain_admm, graph_admm
    from gadmm_amd.parallel.topology import chain_graph
    monkeypatch.setenv("GADMM_BLOCKED", "0")
    m, obj0 = _e1(n)
    c = chain_admm(m, list(range(n)), n, 3.0, obj0, 1e-4, 3000, quantize=(8, 1234))
    a = graph_admm(m, chain_graph(n), 3.0, obj0, 1e-4, 3000, backend="native", quantize=(8, 1234), engine_opts=OPTS)
    assert c.extra["backend"] == "native" and c.extra["engine"] == "persistent", c.extra
    assert a.extra["kernel"] == "persistent-graph-Q(deg<=2,b=8)", a.extra["kernel"]
    ce, ae = c.extra["engine_obj"], a.extra["engine_obj"]
    same_hat = torch.equal(ce.theta.cpu(), ae.theta.cpu())
    print("chain N=%d: chain kernel %d iterations, graph kernel %d; trace bit-identical %s, public models %s" % (
        n, c.iters, a.iters, np.array_equal(a.obj, c.obj), same_hat))
    assert a.converged and c.converged and a.iters == c.iters
    assert np.array_equal(a.obj, c.obj)
    assert same_hat
    assert torch.equal(ce.theta_true.cpu(), ae.theta_true.cpu())


@pytest.mark.parametrize("name", list(Q.STOP_CASES))
def test_stop_rule_and_exit_path(name):
    """To the 1e-4 stop, b = 8: the stop decision reaches the workers in mid-wait (two poll groups on the
    star of 20). done == 1, the final gap is below tol, the duals sum to zero over the workers to rounding
    (every edge adds to its head what it takes from its tail: at most n b_dual rho max|theta| once every
    dual is within its bound), and the duals, public models and true iterates equal the reference run to
    the same ``last`` under the bound -- a head's last dual step from copies that absorbed its tails' last
    message twice, or not at all, breaks exactly this."""
    from gadmm_amd.algorithms import graph_admm
    g, m, rho, obj0 = _model(name)
    seed = Q.STOP_SEEDS[name]
    r = graph_admm(m, g, rho, obj0, Q.STOP_TOL, Q.STOP_MAX_ITER, backend="native", quantize=(8, seed),
                   engine_opts=OPTS)
    eng = r.extra["engine_obj"]
    st = eng.ctl_state()
    last = st["iter"] - 1
    print("%s: %d iterations on %s, placed %d, last %d" % (name, r.iters, r.extra["kernel"], r.extra["placed"], last))
    assert st["done"] == 1 and r.converged and abs(r.obj[-1] - obj0) < Q.STOP_TOL
    assert r.iters <= last <= r.iters + Q.OVERRUN and last <= Q.STOP_RUN[name], (r.iters, last)
    ref = Q.reference(name, 8, last, seed, Q.STOP_RUN[name])[4]
    mu = _host(eng.mu)
    drift = float(np.max(np.abs(mu.sum(axis=0)))) / (g.n * ref.b_dual * ref.rho * ref.scale_theta)
    _report("qggadmm stop %s (last=%d)" % (name, last), {
        "theta": ref.err_theta(_host(eng.theta_true), last) / ref.b_theta,
        "hat": ref.err_hat(_host(eng.theta)) / ref.b_hat, "dual": ref.err_dual(mu) / ref.b_dual,
        "objective": ref.err_obj(r.obj) / ref.b_obj, "sum of duals": drift})


def test_second_solve_on_cached_engine():
    """Two back-to-back solves through one cached engine are identical: tags are salted per launch and the
    message table is never re-zeroed."""
    from gadmm_amd.algorithms import graph_admm
    g, m, rho, obj0 = _model("star12hub5-d50")
    runs = []
    for _ in range(2):
        r = graph_admm(m, g, rho, obj0, 1e-6, 3000, backend="native", quantize=(8, 1234), engine_opts=OPTS)
        eng = r.extra["engine_obj"]
        runs.append((r.iters, r.converged, r.obj.copy(), _host(eng.theta), _host(eng.theta_true), _host(eng.mu),
                     _host(eng.q_msg), id(eng)))
    assert runs[0][7] == runs[1][7], "the engine was not cached"
    assert runs[0][:2] == runs[1][:2] and runs[0][1]
    for x, y in zip(runs[0][2:7], runs[1][2:7]):
        assert np.array_equal(x, y)


def test_xcd_packing_on_and_off():
    """``xcd`` 0 / 1 / 2 (default grid, packed onto one XCD, plain L2-resident stores): bit for bit."""
    from gadmm_amd.engine.graph_engine import NativeGraphEngine
    g, m, rho, obj0 = _model("grid2x3-d50")
    out = []
    for xcd in (2, 1, 0):
        eng = NativeGraphEngine(m.X, m.y, g, rho, obj0, 1e-6, 3000, precomputed=(m.A, m.b, m.yy), xcd=xcd,
                                quant=(8, 1234))
        r = eng.run(timeout_s=5.0)
        assert r.done == 1 and eng.last_placed == xcd, (r.done, eng.last_placed)
        out.append((r.iters, eng.traces(r.iters)[0], _host(eng.theta), _host(eng.theta_true), _host(eng.mu),
                    _host(eng.rres[:r.iters]), _host(eng.q_msg)))
    for other in out[1:]:
        assert out[0][0] == other[0]
        for x, y in zip(out[0][1:], other[1:]):
            assert np.array_equal(x, y)


def test_dispatch_cu_budget_takes_the_torch_path(monkeypatch):
    """Two CUs hold eight one-wave workgroups, not the 9 of the star of 8: the refusal comes before any
    launch, ``backend='auto'`` runs the torch path with the reason recorded, ``backend='native'`` raises."""
    from gadmm_amd.algorithms import graph_admm
    g, m, rho, obj0 = _model("star8-d64")
    opts = dict(OPTS, cache=False)
    a = graph_admm(m, g, rho, obj0, 1e-6, 3000, quantize=(8, 1234), engine_opts=opts)
    monkeypatch.setenv("GADMM_CU_BUDGET", "2")
    b = graph_admm(m, g, rho, obj0, 1e-6, 3000, quantize=(8, 1234), engine_opts=opts)
    assert a.extra["backend"] == "native" and a.extra["kernel"] == "persistent-graph-Q(deg<=8,b=8)"
    assert b.extra["backend"] == "torch" and b.extra["graph_fallback"].startswith("ResidencyError"), b.extra
    assert a.extra["transmissions"] == a.iters * g.n and a.extra["q_wire_bytes"] == a.iters * g.n * 9 * 16
    assert a.extra["payload_bits"] == a.iters * g.n * (8 * 64 + 64) and a.extra["deliveries"] == a.iters * 2 * 7
    with pytest.raises(RuntimeError):
        graph_admm(m, g, rho, obj0, 1e-6, 3000, backend="native", quantize=(8, 1234), engine_opts=opts)


def test_entry_writes_the_quantized_runs(tmp_path):
    from gadmm_amd.entry import LinearRegression_Topologies as E
    out = E.main(["--device", "cuda", "--out", str(tmp_path), "--no-plot", "--set", "quant_bits=8"])
    runs = out["runs"]
    q = [k for k in runs if k.startswith("Q-GGADMM_b8_")]
    assert len(q) == len([k for k in runs if k.startswith("GGADMM_")]) == 5, sorted(runs)
    for k in q:
        assert runs[k]["kernel"].startswith("persistent-graph-Q(") and runs[k]["converged"], runs[k]
