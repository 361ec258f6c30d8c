"""CQ-GADMM dispatch and accounting, the parts that need no device: every case the native path does not
cover reaches the torch path with its reason and with the censoring still applied (and is refused under
``backend='native'``), what the native path is handed, the mixed sweep's groups of eight through a faked
native layer, and the accounting across ranks (gloo), after ``failures=`` and on a resumed run.

The dispatcher decides on ``model.device``, ``comm.nranks`` and friends before anything touches a
tensor, so a model that CLAIMS to live on a HIP device takes it through every branch on the CPU; the
torch path below then runs on the real model (one rank)."""
import numpy as np
import pytest
import torch

from gadmm_amd.algorithms import chain_admm, quantized_group_admm_sweep
from gadmm_amd.algorithms import gadmm as G
from gadmm_amd.parallel.launch import spawn

CENSOR = (1.0, 0.9)
QUANT = (8, 1234)


class _CudaDev:
    type = "cuda"


class _OnDevice:
    """``model`` as the dispatcher sees it if it lived on a HIP device (optionally with another ``d``)."""

    def __init__(self, model, d=None):
        self._m = model
        self._d = d

    def __getattr__(self, k):
        if k == "device":
            return _CudaDev()
        if k == "d" and self._d is not None:
            return self._d
        return getattr(self._m, k)


class _TwoRanks:
    rank, nranks = 0, 2


@pytest.fixture(scope="module")
def lin8():
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models.linear import LinearRegression
    ds = linear_synthetic(8)
    m = LinearRegression(ds.X, ds.y)
    return m, m.optimum()


@pytest.fixture
def torch_path_on_the_real_model(monkeypatch):
    """The torch path is handed the pretended model (and communicator): run it on the real ones."""
    real = G._chain_admm_torch
    seen = {}

    def run(model, local_ids, n_total, rho, obj0, tol, max_iter, comm, *a, **kw):
        from gadmm_amd.parallel.comm import LocalComm
        seen["censor"] = kw.get("censor")
        if isinstance(model, _OnDevice):
            model = model._m
        if isinstance(comm, _TwoRanks):
            comm = LocalComm()
        return real(model, local_ids, n_total, rho, obj0, tol, max_iter, comm, *a, **kw)

    monkeypatch.setattr(G, "_chain_admm_torch", run)
    return seen


def _schedule_dynamic():
    from gadmm_amd.parallel.topology import PathSchedule
    return PathSchedule(8, list(range(8)), np.zeros(7), coherence=5, seed=3)


def _one_rank_placement():  # (the pretended second rank owns nobody: the torch path runs on one)
    from gadmm_amd.parallel.topology import Placement
    return Placement.contiguous(8, 1)


def _state():
    return (torch.zeros((8, 50), dtype=torch.float64), torch.zeros((8, 50), dtype=torch.float64), 1)


_CASES = {
    "state= (resume)": lambda: dict(state=_state()),
    "failures= (elastic recovery)": lambda: dict(failures={10: [3]}),
    "exchange checker": lambda: dict(check_exchange=True),
    "several ranks": lambda: dict(comm=_TwoRanks(), placement=_one_rank_placement()),
    "dynamic schedule": lambda: dict(schedule=_schedule_dynamic()),
    "d > 256": lambda: dict(),
    "xgmi fabric": lambda: dict(engine_opts={"fabric": object()}),
}


@pytest.mark.parametrize("why", sorted(_CASES))
def test_uncovered_cases_run_the_torch_path_censored(lin8, torch_path_on_the_real_model, why):
    m, obj0 = lin8
    model = _OnDevice(m, d=300 if why == "d > 256" else None)
    kw = _CASES[why]()
    r = chain_admm(model, list(range(8)), 8, 3.0, obj0, 1e-30, 40, quantize=QUANT, censor=CENSOR, **kw)
    ex = r.extra
    assert ex["backend"] == "torch" and ex["quant_fallback"] == why
    assert torch_path_on_the_real_model["censor"] == CENSOR and ex["censor"] == CENSOR
    tr = ex["sent_trace"]
    assert tr.shape == (40, 8) and tr.any() and not tr.all()  # the censoring is applied
    assert ex["transmissions"] == int(tr.sum()) and 0.0 < ex["min_censor_margin"] < 1.0
    if why not in ("failures= (elastic recovery)", "dynamic schedule"):  # the chain of the plain run
        assert tuple(int(tr[:k].sum()) for k in (20, 40)) == (76, 134)  # tests/test_cqgadmm_cpu.py
    with pytest.raises(RuntimeError, match="does not cover this case"):
        chain_admm(model, list(range(8)), 8, 3.0, obj0, 1e-30, 40, quantize=QUANT, censor=CENSOR, backend="native",
                   **_CASES[why]())


def test_logistic_model_runs_the_torch_path_censored(torch_path_on_the_real_model):
    from gadmm_amd.data import logistic_synthetic
    from gadmm_amd.models import LogisticRegression
    ds = logistic_synthetic(4)
    m = LogisticRegression(ds.X, ds.y, 1e-5)
    r = chain_admm(_OnDevice(m), list(range(4)), 4, 3e-4, 0.0, 1e-30, 30, quantize=QUANT, censor=(30.0, 0.9), step=2.2)
    assert r.extra["quant_fallback"] == "not the linear closed-form model" and r.extra["backend"] == "torch"
    tr = r.extra["sent_trace"]
    assert tr.shape == (30, 4) and tr.any() and not tr.all()
    with pytest.raises(RuntimeError, match="does not cover this case"):
        chain_admm(_OnDevice(m), list(range(4)), 4, 3e-4, 0.0, 1e-30, 30, quantize=QUANT, censor=(30.0, 0.9), step=2.2,
                   backend="native")


def test_native_path_is_handed_the_censor(lin8, monkeypatch, torch_path_on_the_real_model):
    """A covered case goes to the native solve with the validated (tau0, xi); without a native library
    it is the torch path with that reason, or an error under ``backend='native'``."""
    from gadmm_amd.ops import native
    m, obj0 = lin8
    got = {}

    def native_quant(model, local_ids, n_total, rho, obj0_, tol, max_iter, placement, schedule, cost_quirk, name,
                     opts, bits, seed, censor=None):
        got.update(bits=bits, seed=seed, censor=censor, opts=opts)
        return "native result"

    monkeypatch.setattr(G, "_chain_admm_native_quant", native_quant)
    monkeypatch.setattr(native, "available", lambda: True)
    r = chain_admm(_OnDevice(m), list(range(8)), 8, 3.0, obj0, 1e-4, 40, quantize=QUANT, censor=(1, 0.9),
                   engine_opts={"persistent": False})
    assert r == "native result"
    assert got == {"bits": 8, "seed": 1234, "censor": (1.0, 0.9), "opts": {"persistent": False}}
    got.clear()
    chain_admm(_OnDevice(m), list(range(8)), 8, 3.0, obj0, 1e-4, 40, quantize=QUANT)
    assert got["censor"] is None
    monkeypatch.setattr(native, "available", lambda: False)
    r = chain_admm(_OnDevice(m), list(range(8)), 8, 3.0, obj0, 1e-30, 20, quantize=QUANT, censor=CENSOR)
    assert r.extra["quant_fallback"] == "native library unavailable" and not r.extra["sent_trace"].all()
    with pytest.raises(RuntimeError, match="unavailable"):
        chain_admm(_OnDevice(m), list(range(8)), 8, 3.0, obj0, 1e-30, 20, quantize=QUANT, censor=CENSOR, backend="native")


# ---- the mixed sweep through a faked native layer: groups of eight, the kernel of each group
class _FakeRun:
    def __init__(self, iters):
        self.iters, self.done = iters, 1


class _FakeMember:
    obj_mode_name = "exact"

    def __init__(self, cfg, censor, n):
        self.cfg, self.censor, self.n = cfg, censor, n
        self.iters = 3 + int(cfg[2])

    def traces(self, iters):
        return np.full(iters, float(self.cfg[2])), np.arange(iters, dtype=np.float64)

    def sent_trace(self, upto):
        assert self.censor is not None  # only censored members are asked
        tr = np.zeros((upto, self.n), dtype=bool)
        tr[:, 0] = True
        return tr


class _FakeSweep:
    built = []

    def __init__(self, cfgs, censors, n):
        self.members = [_FakeMember(c, cen, n) for c, cen in zip(cfgs, censors)]
        cens = any(c is not None for c in censors)
        self.last_kernel = "persistent-%s-sweep(K=%d)" % ("CQ" if cens else "Q", len(cfgs))
        self.last_placed = [2] * len(cfgs)
        self.last_wall_ms = 1.0

    @classmethod
    def build(cls, X, y, local_ids, n_total, configs, censors=None, **kw):
        cls.built.append((list(configs), list(censors), list(kw["tols"])))
        return cls(configs, censors, n_total)

    def run(self):
        return [_FakeRun(m.iters) for m in self.members]

    def stop_ticks(self, runs):
        return [0] * len(runs)


def test_nineteen_mixed_members_through_the_sweep_engine(lin8, monkeypatch):
    """19 members = 8 + 8 + 3, censored ones in the first and the last group, none in the middle one: each group is built
    with its own configs, censor list and tolerances, in input order; every result carries its own
    member's trace, accounting and its group's kernel."""
    import gadmm_amd.engine.quant_sweep as QS
    from gadmm_amd.ops import native
    m, obj0 = lin8
    _FakeSweep.built = []
    monkeypatch.setattr(QS, "QuantSweepEngine", _FakeSweep)
    monkeypatch.setattr(QS, "quant_sweep_capacity", lambda: 8)
    monkeypatch.setattr(native, "available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    configs = [(3.0 + i, 8, i, 1.0, 0.9) if i in (1, 6, 17) else (3.0 + i, 8, i) for i in range(19)]
    tols = [10.0 ** -(i % 5 + 2) for i in range(len(configs))]
    got = quantized_group_admm_sweep(_OnDevice(m), configs, obj0, 1e-4, 50, tols=tols, engine_opts={"cache": False})
    cens = [(1.0, 0.9) if len(c) == 5 else None for c in configs]
    assert [len(b[0]) for b in _FakeSweep.built] == [8, 8, 3]
    lo = 0
    for cfgs, censors, g_tols in _FakeSweep.built:
        hi = lo + len(cfgs)
        assert cfgs == [(float(c[0]), c[1], c[2]) for c in configs[lo:hi]]
        assert censors == cens[lo:hi] and g_tols == tols[lo:hi]
        lo = hi
    assert len(got) == len(configs)
    for i, (r, c) in enumerate(zip(got, configs)):
        group = i // 8
        assert r.iters == 3 + c[2] and np.all(r.obj == float(c[2]))  # its own member's result, in input order
        assert r.extra["sweep"]["slot"] == i % 8
        assert r.extra["sweep"]["kernel"] == ("persistent-CQ-sweep(K=8)", "persistent-Q-sweep(K=8)",
                                              "persistent-CQ-sweep(K=3)")[group]
        G_ = -(-50 * c[1] // 64) + 1
        if cens[i] is not None:
            assert r.extra["censor"] == cens[i] and r.extra["transmissions"] == r.iters
            assert r.extra["censored"] == r.iters * 7
            assert r.extra["q_wire_bytes"] == r.iters * G_ * 16 + r.iters * 7 * 16
            assert r.comm_units[-1] == r.iters * (c[1] * 50 + 64) / (64.0 * 50)
        else:
            assert "sent_trace" not in r.extra and "transmissions" not in r.extra
            assert r.extra["q_wire_bytes"] == r.iters * 8 * G_ * 16
            assert r.comm_units[-1] == r.iters * 8 * (c[1] * 50 + 64) / (64.0 * 50)


# ---- accounting: across ranks, after failures, on a resumed run
def _rank_fn(rank, world, params):
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models import LinearRegression
    from gadmm_amd.parallel.comm import TorchDistComm
    from gadmm_amd.parallel.topology import Placement
    n = params["n"]
    comm = TorchDistComm()
    pl = Placement.contiguous(n, world)
    local = pl.local_workers(rank)
    ds = linear_synthetic(n)
    m = LinearRegression(ds.X[local], ds.y[local])
    r = chain_admm(m, local, n, 3.0, params["obj0"], params["tol"], params["max_iter"], comm=comm, placement=pl,
                   quantize=QUANT, censor=CENSOR)
    ex = r.extra
    return {"iters": r.iters, "obj": r.obj, "comm_units": r.comm_units, "sent_trace": ex["sent_trace"],
            "transmissions": ex["transmissions"], "censored": ex["censored"], "payload_bits": ex["payload_bits"],
            "margin": ex["min_censor_margin"], "why": ex["quant_fallback"]}


@pytest.mark.parametrize("world", [2, 3])
def test_accounting_across_ranks_equals_one_rank(lin8, world):
    """Every rank decides for its own workers only; the reported trace, transmissions, censored count
    and comm units are global, the same on every rank and equal to the one-process run's."""
    m, obj0 = lin8
    params = {"n": 8, "obj0": obj0, "tol": 1e-30, "max_iter": 60}
    single = chain_admm(m, list(range(8)), 8, 3.0, obj0, 1e-30, 60, quantize=QUANT, censor=CENSOR)
    res = spawn(_rank_fn, world, params)
    for r in res:
        assert r["iters"] == single.iters == 60
        assert np.allclose(r["obj"], single.obj, rtol=1e-12)
        assert np.array_equal(r["sent_trace"], single.extra["sent_trace"])
        assert r["transmissions"] == single.extra["transmissions"] == 195
        assert r["censored"] == single.extra["censored"] == 60 * 8 - 195
        assert r["payload_bits"] == single.extra["payload_bits"]
        assert np.array_equal(r["comm_units"], single.comm_units)
        assert r["margin"] == single.extra["min_censor_margin"]
        assert r["why"] == "cpu tensors"


def test_dropped_workers_are_not_counted_as_censored(lin8):
    m, obj0 = lin8
    r = chain_admm(m, list(range(8)), 8, 3.0, obj0, 1e-30, 40, quantize=QUANT, censor=CENSOR, failures={11: [3, 6]})
    tr = r.extra["sent_trace"]
    assert not tr[10:, [3, 6]].any()  # gone from iteration 11 on
    assert r.extra["transmissions"] == int(tr.sum())
    assert r.extra["transmissions"] + r.extra["censored"] == 10 * 8 + 30 * 6


def test_resumed_run_counts_its_own_transmissions(lin8):
    """``state=``: the comm units of a censored run start at the resumed iteration (what was sent before the
    checkpoint is not known to it), and the run continues the plain one's decisions."""
    m, obj0 = lin8
    ids = list(range(8))
    full = chain_admm(m, ids, 8, 3.0, obj0, 1e-30, 40, quantize=QUANT, censor=CENSOR)
    a = chain_admm(m, ids, 8, 3.0, obj0, 1e-30, 15, quantize=QUANT, censor=CENSOR)
    th, mu, nxt = a.extra["state"]
    assert nxt == 16
    b = chain_admm(m, ids, 8, 3.0, obj0, 1e-30, 40, quantize=QUANT, censor=CENSOR, state=(th, mu, nxt))
    tr = b.extra["sent_trace"]
    assert tr.shape == (25, 8) and len(b.obj) == 25
    assert b.extra["transmissions"] + b.extra["censored"] == 25 * 8
    assert b.comm_units[0] == tr[0].sum() * (8 * 50 + 64) / (64.0 * 50)
    # the heads' pending state travels in (theta, mu) only for the public models: the true iterates restart
    # from them, so the resumed decisions are compared where they are determined -- the thresholds' index
    assert np.array_equal(a.extra["sent_trace"], full.extra["sent_trace"][:15])
