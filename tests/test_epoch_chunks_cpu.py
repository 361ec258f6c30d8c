"""The epoch-chunk cursor of D-GADMM (engine/epoch_chunks.py) without a device: its launch windows
against the hand-derived sequence, its chain table against one-at-a-time ``PathSchedule.step`` draws, its
cumulative cost against the torch path's running sum (which shares no code with it), the hint, the early
draw and the epoch limit. The cursor is driven by a fake outcome feed: "hard stop reached" until the
launch that covers the chosen stop iteration, then "converged at iteration k"."""
import copy

import numpy as np
import pytest

from gadmm_amd.algorithms import chain_admm, dynamic_group_admm, dynamic_group_admm_v0
from gadmm_amd.data import linear_synthetic
from gadmm_amd.engine.epoch_chunks import EpochCursor
from gadmm_amd.models import LinearRegression
from gadmm_amd.parallel import topology as T

N, MAX_ITER = 6, 40


def _schedule(coh, kind="findPath2", seed=11, n=N):
    p0, c0, _ = T.find_path(n, np.random.default_rng(5))
    return T.PathSchedule(n, p0, c0, coh, kind=kind, seed=seed)


def _drive(cur, stop_at, each=None):
    """Feed ``cur`` until the launch that covers iteration ``stop_at``; the windows it gave."""
    seen = []
    while True:
        w = cur.window()
        seen.append((cur.e0, cur.e1) + tuple(w[2:]))
        if each is not None:
            each(w)
        hard_stop = w[4]
        if hard_stop == 0 or stop_at <= hard_stop:
            assert not cur.advance(1, stop_at, stop_at + 4)
            cur.finish()
            return seen
        assert cur.advance(5, 0, 0)


# (e0, e1, start_iter, pending_in, hard_stop, cont) of every launch of a solve that runs to the cap, by hand:
# coherence 3 re-chains at 3, 6, .., 39 (14 epochs, epoch e >= 1 starting at 3 e); coherence 1 at 2, 3, .., 40
# (40 epochs, epoch e >= 1 starting at e + 1). Chunks of 2, 4, 8, .. epochs, each starting at the last epoch
# of the one before; the hard stop is the iteration before epoch e1 starts.
WINDOWS = {
    3: [(0, 2, 1, 0, 5, False), (1, 5, 6, 1, 14, True), (4, 12, 15, 1, 35, True), (11, 14, 36, 1, 0, True)],
    1: [(0, 2, 1, 0, 2, False), (1, 5, 3, 1, 5, True), (4, 12, 6, 1, 12, True), (11, 27, 13, 1, 27, True),
        (26, 40, 28, 1, 0, True)],
}


@pytest.mark.parametrize("coh", [1, 3])
def test_windows_are_the_hand_derived_sequence(coh):
    cur = EpochCursor(_schedule(coh), MAX_ITER, N, {}, epoch_chunk=2, cap=1000)
    rech = T.rechain_iterations(MAX_ITER, coh)
    starts_of = np.concatenate([[1], rech])
    drawn = []

    def each(w):
        starts, chains, start_iter, pending_in, hard_stop, cont = w
        e0, e1 = cur.e0, cur.e1
        look = e1 if e1 < len(starts_of) else e1 - 1
        assert np.array_equal(starts, starts_of[e0:look + 1]) and chains.shape == (look + 1 - e0, N)
        assert hard_stop == (rech[e1 - 1] - 1 if e1 < len(starts_of) else 0)  # epoch e1 starts at rech[e1 - 1]
        assert cur.n_drawn == look + 1  # only the chains this launch needs
        drawn.append(look)

    seen = _drive(cur, MAX_ITER, each)
    assert seen == WINDOWS[coh]
    assert [b - a for a, b, *_ in seen[:-1]] == [2, 4, 8, 16][:len(seen) - 1]
    assert all(nxt[0] == prev[1] - 1 and nxt[2:4] + nxt[5:] == (prev[4] + 1, 1, True) for prev, nxt in zip(seen, seen[1:]))
    assert seen[0][2:4] == (1, 0) and seen[0][5] is False
    assert seen[-1][4] == 0 and drawn[-1] == seen[-1][1] - 1 == len(rech)  # no look-ahead epoch past the last


@pytest.mark.parametrize("coh", [1, 3])
def test_cap_bounds_every_chunk(coh):
    cur = EpochCursor(_schedule(coh), MAX_ITER, N, {}, epoch_chunk=2, cap=3)
    seen = _drive(cur, MAX_ITER)
    assert [b - a for a, b, *_ in seen[:3]] == [2, 3, 3] and all(b - a <= 3 for a, b, *_ in seen)
    assert seen[-1][1] == 1 + len(T.rechain_iterations(MAX_ITER, coh)) and seen[-1][4] == 0


@pytest.mark.parametrize("kind", ["findPath2", "findPath"])
@pytest.mark.parametrize("coh", [1, 3])
def test_chains_equal_one_at_a_time_draws(kind, coh):
    cur = EpochCursor(_schedule(coh, kind), MAX_ITER, N, {}, epoch_chunk=2, cap=1000)
    one = _schedule(coh, kind)
    chains = [list(one.path)]
    costs = []
    for it in range(2, MAX_ITER + 1):
        if one.step(it):
            chains.append(list(one.path))
            costs.append(np.array(one.cost))
    _drive(cur, MAX_ITER)
    assert cur.n_drawn == len(chains) and [list(p) for p in cur.paths] == chains
    assert np.array_equal(np.concatenate(cur.costs), np.asarray(costs))
    assert np.array_equal(cur.starts, np.concatenate([[1], T.rechain_iterations(MAX_ITER, coh)]))


def test_a_solve_that_stops_early_draws_only_what_its_launches_need():
    cur = EpochCursor(_schedule(3), MAX_ITER, N, {}, epoch_chunk=2, cap=1000)
    seen = _drive(cur, 10)  # decided in the second launch: epochs 1 .. 4, hard stop 14
    assert len(seen) == 2 and cur.n_drawn == 6 and cur.iters == 10 and cur.done == 1 and cur.last_launched == 14
    assert cur.span == 17 and cur.reached == 5  # epoch 4 (iterations 12 .. 14) holds iteration 14


# ---- cost: the torch path's running sum on a small problem
@pytest.fixture(scope="module")
def prob():
    ds = linear_synthetic(24)
    m = LinearRegression(ds.X, ds.y)
    p0, c0, _ = T.find_path(24, np.random.default_rng(5))
    return m, m.optimum(), p0, c0


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("coh", [1, 10])
def test_com_cost_is_the_torch_paths_running_sum(prob, coh, quirk):
    m, obj0, p0, c0 = prob
    ref = dynamic_group_admm(m, 1.0, obj0, 1e-4, 120, p0, c0, coh, seed=7, backend="torch", cost_quirk=quirk)
    cur = EpochCursor(T.PathSchedule(24, p0, c0, coh, seed=7), 120, 24, {}, epoch_chunk=4, cap=1000)
    _drive(cur, ref.iters)
    got = cur.com_cost(12 if quirk else 1)
    assert len(got) == cur.span >= ref.iters and np.array_equal(got[:ref.iters], ref.com_cost)
    assert cur.com_cost(12 if quirk else 1) is got  # summed once per number of drawn epochs


def test_com_cost_with_the_v0_initial_cost_and_ragged_rows(prob):
    m, obj0, _, _ = prob
    rng = np.random.default_rng(2)
    paths, costs = [], []
    for _ in range(5):
        p, c, _ = T.find_path(24, rng)
        paths.append(p)
        costs.append(c)
    cm = np.asarray(costs)
    # the reference's column slice as the initial cost: 5 entries beside rows of 23
    ref = dynamic_group_admm_v0(m, 3.0, obj0, 1e-4, 30, paths, cm, 10, backend="torch")
    sc = T.PathSchedule(24, paths[0], cm[:, 0], 10, kind="matrix", path_matrix=paths, cost_matrix=cm)
    cur = EpochCursor(sc, 30, 24, {}, cap=1000)
    _drive(cur, ref.iters)
    assert np.array_equal(cur.com_cost(12)[:ref.iters], ref.com_cost)
    # rows of different lengths: the schedule hands them over as an object array
    ragged = [c[:23 - k] for k, c in enumerate(costs)]
    mk = lambda: T.PathSchedule(24, paths[0], ragged[0], 10, kind="matrix", path_matrix=paths, cost_matrix=ragged)  # noqa: E731
    ref = chain_admm(m, list(range(24)), 24, 3.0, obj0, 1e-4, 30, schedule=mk(), backend="torch")
    cur = EpochCursor(mk(), 30, 24, {}, cap=1000)
    _drive(cur, ref.iters)
    assert cur.costs[0].dtype == object and np.array_equal(cur.com_cost(12)[:ref.iters], ref.com_cost)


# ---- hint
def test_hint_sizes_the_next_first_launch():
    hints = {}
    cur = EpochCursor(_schedule(1), 400, N, hints, cap=1000)
    assert cur.chunk == 128
    _drive(cur, 100)
    assert cur.reached == 104 and hints == {(1.0, "findPath2", 400, N): 104}  # launched to 104: epoch 103
    assert EpochCursor(_schedule(1), 400, N, hints, cap=1000).chunk == 112  # max(16, reached + 8)
    assert EpochCursor(_schedule(1), 400, N, hints, cap=50).chunk == 50
    assert EpochCursor(_schedule(1), 400, N, hints, epoch_chunk=2, cap=1000).chunk == 2
    assert EpochCursor(_schedule(1), 400, N, {(1.0, "findPath2", 400, N): 3}, cap=1000).chunk == 16
    assert EpochCursor(_schedule(3), 400, N, hints, cap=1000).chunk == 128  # another shape: no hint


# ---- early draw
def _early(schedule, counts):
    """A stand-in for ``schedule.prefetch_async``: the RNG position moves at once, ``join`` gives the chains."""
    def start(count):
        counts.append(count)
        clone = copy.deepcopy(schedule)
        schedule._consume(2 * schedule.n * count)
        return lambda: clone.prefetch_arrays(count)
    return start


def _position(schedule):
    rs, path, cost, k = schedule.save()
    return rs, path, cost.tolist(), k


@pytest.mark.parametrize("coh,chunk,cap", [(1, 2, 1000), (3, 2, 1000), (1, 2, 3), (3, None, 1000), (1, None, 16)])
def test_early_draw_is_the_first_window(coh, chunk, cap):
    a, b, counts = _schedule(coh), _schedule(coh), []
    early = EpochCursor(a, MAX_ITER, N, {}, chunk, cap, early=_early(a, counts))
    plain = EpochCursor(b, MAX_ITER, N, {}, chunk, cap)
    assert counts == [plain.look_ahead()] == [early.look_ahead()]
    w_e, w_p = early.window(), plain.window()
    assert early.n_drawn == plain.n_drawn == counts[0] + 1
    assert np.array_equal(w_e[1], w_p[1]) and w_e[2:] == w_p[2:]
    for cur in (early, plain):
        _drive(cur, 20)
        cur.skip_schedule()
    assert np.array_equal(early.paths, plain.paths) and _position(a) == _position(b)
    assert np.array_equal(np.concatenate(early.costs), np.concatenate(plain.costs))


def test_an_abandoned_early_draw_rewinds_the_schedule():
    a, counts = _schedule(3), []
    saved = _position(a)
    cur = EpochCursor(a, MAX_ITER, N, {}, early=_early(a, counts))
    assert counts == [13] and _position(a) != saved
    cur.abandon()
    assert _position(a) == saved
    again = EpochCursor(a, MAX_ITER, N, {})
    again.window()
    assert [list(p) for p in again.paths] == [list(p) for p in EpochCursor(_schedule(3), MAX_ITER, N, {}).window()[1]]


def test_too_many_epochs_raise():
    with pytest.raises(ValueError, match="too many epochs"):
        EpochCursor(_schedule(1), (1 << 20) + 1, N, {})
    EpochCursor(_schedule(2), 1 << 20, N, {})  # 2^19 epochs: taken


def test_outcome_less_launch_raises():
    cur = EpochCursor(_schedule(3), MAX_ITER, N, {}, epoch_chunk=2)
    cur.window()
    with pytest.raises(RuntimeError, match=r"D-GADMM chunk of member 2 ended without an outcome \(hard stop 5\)"):
        cur.advance(0, 0, 0, " of member 2")
