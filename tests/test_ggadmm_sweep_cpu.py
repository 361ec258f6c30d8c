"""GGADMM / Q-GGADMM sweep (``graph_admm_sweep``, engine/graph_sweep.py), the parts that need no device:
the sequential fallback and its order, the member and ``tols`` validation, and the two sweep launchers'
argument checks (every refusal comes back as -1 before any HIP call)."""
import ctypes

import numpy as np
import pytest

from gadmm_amd.algorithms import graph_admm, graph_admm_sweep
from gadmm_amd.data import linear_synthetic
from gadmm_amd.models import LinearRegression
from gadmm_amd.ops import native
from gadmm_amd.parallel.topology import grid_graph, ring_graph, star_graph


@pytest.fixture(scope="module")
def lin():
    """E1 data cut to 8 and to 6 workers: ``{n: (model, obj0)}``."""
    out = {}
    for n in (8, 6):
        ds = linear_synthetic(n)
        m = LinearRegression(ds.X, ds.y)
        out[n] = (m, m.optimum())
    return out


def _single(m, obj0, mem, tol=1e-4, max_iter=600, **kw):
    quant = None if len(mem) == 2 else (mem[2], mem[3])
    return graph_admm(m, mem[0], mem[1], obj0, tol, max_iter, quantize=quant, **kw)


def _same(g, r):
    assert g.iters == r.iters and g.converged == r.converged
    assert np.array_equal(g.obj, r.obj) and np.array_equal(g.comm_units, r.comm_units)
    assert np.array_equal(g.primal_res, r.primal_res)


def test_sweep_on_cpu_is_the_loop_of_graph_admm(lin):
    m, obj0 = lin[8]
    members = [(ring_graph(8), 3.0), (star_graph(8, 0), 5.0), (ring_graph(8), 7.0)]
    got = graph_admm_sweep(m, members, obj0, 1e-4, 600)
    assert len(got) == 3
    for g, mem in zip(got, members):
        _same(g, _single(m, obj0, mem))
        assert g.extra["sweep_fallback"] == "cpu tensors" and "sweep" not in g.extra
    assert got[0].iters != got[2].iters  # (two rho on one graph: the order is checked on results that differ)
    m6, obj6 = lin[6]
    members = [(ring_graph(6), 3.0), (grid_graph(2, 3), 3.0)]
    got = graph_admm_sweep(m6, members, obj6, 1e-4, 600)
    for g, mem in zip(got, members):
        _same(g, _single(m6, obj6, mem))
        assert g.extra["sweep_fallback"] == "cpu tensors"
        assert g.extra["graph"] == mem[0].describe()


def test_mixed_plain_and_quantized_list_keeps_its_order(lin):
    m, obj0 = lin[6]
    ring, grid = ring_graph(6), grid_graph(2, 3)
    members = [(ring, 3.0, 8, 7), (grid, 3.0), (grid, 3.0, 4, 1), (ring, 3.0), (ring, 3.0, 8, 8)]
    got = graph_admm_sweep(m, members, obj0, 1e-4, 600)
    for g, mem in zip(got, members):
        r = _single(m, obj0, mem)
        _same(g, r)
        assert g.extra["sweep_fallback"] == "cpu tensors"
        if len(mem) == 4:
            assert (g.extra["q_bits"], g.extra["q_seed"]) == (mem[2], mem[3])
            assert g.extra["payload_bits"] == r.extra["payload_bits"]
            assert np.array_equal(g.extra["theta_true"], r.extra["theta_true"])
        else:
            assert "q_bits" not in g.extra
    assert not np.array_equal(got[0].obj[:20], got[4].obj[:20])  # the two seeds are two runs


def test_torch_backend_is_the_loop(lin):
    m, obj0 = lin[6]
    got = graph_admm_sweep(m, [(ring_graph(6), 3.0)], obj0, 1e-4, 600, backend="torch")
    assert [g.extra["sweep_fallback"] for g in got] == ["torch backend"]
    assert graph_admm_sweep(m, [], obj0, 1e-4, 600) == []


def test_tols_are_per_member(lin):
    m, obj0 = lin[6]
    mem = (ring_graph(6), 3.0)
    got = graph_admm_sweep(m, [mem, mem], obj0, 1e-4, 600, tols=(1e-2, 1e-4))
    assert got[0].iters < got[1].iters and np.array_equal(got[0].obj, got[1].obj[:got[0].iters])
    with pytest.raises(ValueError, match="tols"):
        graph_admm_sweep(m, [mem, mem], obj0, 1e-4, 600, tols=(1e-2,))


@pytest.mark.parametrize("bad", [(3.0,), ("ring", 3.0), (None, 3.0, 8), (None, 3.0, 8, 1, 2), (None, 3.0, 5, 1)])
def test_member_tuples_are_validated(lin, bad):
    m, obj0 = lin[6]
    mem = tuple(ring_graph(6) if x is None else x for x in bad)
    with pytest.raises(ValueError):
        graph_admm_sweep(m, [(ring_graph(6), 3.0), mem], obj0, 1e-4, 600)


def test_a_graph_of_another_size_is_the_loop(lin):
    """A member graph whose n is not the model's goes to the loop, where graph_admm refuses it by name."""
    m, obj0 = lin[6]
    with pytest.raises(NotImplementedError, match="every worker local"):
        graph_admm_sweep(m, [(ring_graph(6), 3.0), (ring_graph(8), 3.0)], obj0, 1e-4, 600)


# ---- launcher validation: refused with -1 and a message before any HIP call (no device here). The
# batches name buffers by made-up addresses, so none of them may ever reach a launch: the LAST entry of
# every batch keeps an iteration-tag range that its own checks refuse, and each case adds ONE defect that
# an earlier entry's check, or an earlier check of that entry, must name.
_BUFS = ("nb_ptr", "nb_idx", "wid", "is_head", "Minv", "A", "b", "yy", "theta", "mu", "thg", "objg", "decg",
         "dec_push", "trace", "tstamp", "rres", "ctl", "xchk")
_SHARED_OK = ("nb_ptr", "nb_idx", "wid", "is_head", "Minv", "A", "b", "yy")
_WRITTEN = tuple(b for b in _BUFS if b not in _SHARED_OK)
KINDS = ("plain", "quant")


def _fill(g, j, d=50, n=6, deg=3):
    g.d, g.n, g.n_local, g.nranks, g.max_degree = d, n, n, 1, deg
    g.start_iter, g.max_iter, g.lag, g.ring = 1, 200, 4, 8
    g.rho, g.tol, g.timeout_ticks = 3.0, 1e-8, 10 ** 8
    for k, name in enumerate(_BUFS):
        setattr(g, name, 0x10000000 + 0x100000 * j + 0x1000 * (k + 1))


def _batch(kind, nb, **kw):
    T = native.GraphQArgs if kind == "quant" else native.GraphArgs
    batch = (T * max(nb, 1))()
    for j in range(nb):
        _fill(_g(kind, batch[j]), j, **kw)
        if kind == "quant":
            batch[j].qg, batch[j].q_true = 0x20000000 + 0x100000 * j, 0x30000000 + 0x100000 * j
            batch[j].q_bits, batch[j].q_seed = 8, 1234
    _g(kind, batch[max(nb, 1) - 1]).max_iter = 1 << 20  # never launched, whatever else the case changes
    return batch


def _g(kind, entry):
    return entry.g if kind == "quant" else entry


def _launch(kind, batch, nb):
    lib = native.require()
    T = native.GraphQArgs if kind == "quant" else native.GraphArgs
    stage = (T * 8)()
    fn = lib.gadmm_graph_persistent_q_sweep_launch if kind == "quant" else lib.gadmm_graph_persistent_sweep_launch
    rc = fn(batch, nb, ctypes.addressof(stage), ctypes.addressof(stage), None)
    return rc, lib.gadmm_last_error().decode()


def test_capacity_is_eight_and_the_layouts_did_not_move():
    lib = native.require()
    assert lib.gadmm_graph_persistent_sweep_capacity() == 8 and lib.gadmm_graph_persistent_q_sweep_capacity() == 8
    native.check_graph_abi(lib)
    native.check_graph_q_abi(lib)


@pytest.mark.parametrize("kind", KINDS)
def test_launch_base_batch_is_refused_by_its_tag_range_only(kind):
    for nb in (1, 3, 8):
        rc, msg = _launch(kind, _batch(kind, nb), nb)
        assert rc == -1 and "solve %d: ring must exceed lag + 1, iteration tags" % (nb - 1) in msg, msg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb", [0, 9])
def test_launch_refuses_width(kind, nb):
    T = native.GraphQArgs if kind == "quant" else native.GraphArgs
    rc, msg = _launch(kind, (T * 9)(), nb)
    assert rc == -1 and "one launch takes 1..8" in msg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field,value,j,expect", [
    ("theta", None, 1, "solve 1: a required buffer is null"),
    ("ctl", None, 0, "solve 0: a required buffer is null"),
    ("nb_idx", None, 1, "solve 1: a required buffer is null"),
    ("n_local", 5, 1, "solve 1: one GPU, every worker local"),
    ("nranks", 2, 0, "solve 0: one GPU, every worker local"),
    ("ring", 5, 0, "solve 0: ring must exceed lag + 1"),
    ("lag", 0, 0, "solve 0: ring must exceed lag + 1"),
    ("d", 65, 0, "solve 0: d=65"),
    ("max_degree", 6, 1, "solve 1: d=50, n=6, max_degree=6 not eligible"),
    ("xchk", None, 1, "solve 1 has no placement-check buffer (xchk)"),
])
def test_launch_refuses_entry(kind, field, value, j, expect):
    batch = _batch(kind, 3)
    setattr(_g(kind, batch[j]), field, value)
    rc, msg = _launch(kind, batch, 3)
    assert rc == -1 and expect in msg, msg


def test_q_launch_refuses_bits_and_a_null_message_table():
    batch = _batch("quant", 3)
    batch[1].q_bits = 5
    rc, msg = _launch("quant", batch, 3)
    assert rc == -1 and "solve 1: q_bits must be 4, 8 or 16, got 5" in msg
    batch = _batch("quant", 3)
    batch[0].qg = None
    rc, msg = _launch("quant", batch, 3)
    assert rc == -1 and "solve 0: a required buffer is null" in msg


@pytest.mark.parametrize("kind", KINDS)
def test_launch_refuses_mixed_register_classes(kind):
    batch = _batch(kind, 2)
    _g(kind, batch[0]).d, _g(kind, batch[1]).d = 52, 53
    rc, msg = _launch(kind, batch, 2)
    assert rc == -1 and "register class" in msg and "52" in msg and "53" in msg
    batch = _batch(kind, 2)
    _g(kind, batch[0]).d, _g(kind, batch[1]).d = 53, 64  # one class: on to the last check
    rc, msg = _launch(kind, batch, 2)
    assert rc == -1 and "solve 1: ring must exceed" in msg


@pytest.mark.parametrize("kind", KINDS)
def test_launch_takes_mixed_degree_classes_and_sizes(kind):
    """Degree classes 2 / 16 (32 for the unquantized kernel's star) and n = 2 .. 20 in one batch: nothing
    before the last check objects."""
    batch = _batch(kind, 3)
    for j, (n, deg) in enumerate(((2, 1), (20, 19), (12, 11))):
        g = _g(kind, batch[j])
        g.n, g.n_local, g.max_degree = n, n, deg
    rc, msg = _launch(kind, batch, 3)
    assert rc == -1 and "solve 2: ring must exceed" in msg, msg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", _WRITTEN)
def test_launch_refuses_a_shared_written_buffer(kind, name):
    batch = _batch(kind, 3)
    setattr(_g(kind, batch[0]), name, 0x7fff0000)
    setattr(_g(kind, batch[1]), name, 0x7fff0000)
    rc, msg = _launch(kind, batch, 3)
    assert rc == -1 and "solves 0 and 1 share a buffer that both write" in msg, msg


@pytest.mark.parametrize("name", ["qg", "q_true"])
def test_q_launch_refuses_a_shared_message_table_or_true_iterates(name):
    batch = _batch("quant", 3)
    setattr(batch[0], name, 0x7fff0000)
    setattr(batch[1], name, 0x7fff0000)
    rc, msg = _launch("quant", batch, 3)
    assert rc == -1 and "solves 0 and 1 share a buffer that both write" in msg, msg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", _SHARED_OK)
def test_launch_lets_read_only_inputs_be_shared(kind, name):
    batch = _batch(kind, 3)
    for j in range(3):
        setattr(_g(kind, batch[j]), name, 0x7fff0000)
    rc, msg = _launch(kind, batch, 3)
    assert rc == -1 and "solve 2: ring must exceed" in msg, msg  # nothing before the last check objected


def test_entry_switch_on_cpu_changes_nothing(tmp_path):
    """On the CPU the switch is not taken: the same runs, no sweep fields."""
    from gadmm_amd.entry import LinearRegression_Topologies as E
    runs = {}
    for name, extra in (("seq", []), ("con", ["sweep=concurrent"])):
        out = E.main(["--device", "cpu", "--quick", "--out", str(tmp_path / name), "--no-plot", "--set",
                      "graphs=ring,star:0", "quant_bits=8"] + extra)
        runs[name] = out["runs"]
    assert sorted(runs["con"]) == sorted(runs["seq"]) and len(runs["seq"]) == 4
    for k, s in runs["seq"].items():
        assert runs["con"][k]["iters"] == s["iters"] and "sweep_kernel" not in runs["con"][k]
