"""The epoch-chunk cursor of a D-GADMM solve: everything the solve carries from one persistent launch to
the next, and nothing about how a launch is made.

D-GADMM runs in persistent launches of a CHUNK of epochs each: the seeded chain sequence is drawn a
chunk ahead (batched, the identical RNG stream), every worker switches neighbours / role at each epoch on
the device. A chunk ends at a hard stop just before its last + 1 epoch (whose neighbours already receive
theta); unless the monitor decided a stop, the next launch continues with the same tag salt from there,
its epoch 0 being this chunk's last (the flush of the heads' pending duals). Only the chains a solve
reaches are drawn. The single solve (algorithms/gadmm.py: ``_solve_dynamic``) and every member of a
sweep (engine/dyn_sweep.py) walk their solve with one ``EpochCursor``: ``window`` -> launch -> ``advance``
until it returns False, then ``finish``.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from ..parallel.topology import rechain_iterations

MAX_EPOCHS = 1 << 20  # the epochs of one solve share one tag range
_RECHAINS: dict = {}


def rechains(max_iter: int, coherence) -> np.ndarray:
    """``rechain_iterations`` memoised per (max_iter, coherence) (read-only array)."""
    key = (int(max_iter), float(coherence))
    r = _RECHAINS.get(key)
    if r is None:
        r = rechain_iterations(max_iter, coherence)
        r.setflags(write=False)
        if len(_RECHAINS) < 64:
            _RECHAINS[key] = r
    return r


class EpochCursor:
    """``schedule``: the ``PathSchedule`` at its initial chain (epoch 0). ``hints``: the dict, kept by the
    caller per engine, of the epochs earlier solves of a shape (coherence, kind, max_iter, N) reached.
    ``cap``: the most epochs one launch may execute. ``early``: ``count -> join or None``
    (``PathSchedule.prefetch_async``): the first launch's chains start drawing at construction and are
    joined by the first ``window``; a cursor that never gets there is given up with ``abandon``."""

    def __init__(self, schedule, max_iter: int, n_total: int, hints: dict, epoch_chunk: Optional[int] = None,
                 cap: int = 1 << 30, early: Optional[Callable] = None):
        starts = rechains(max_iter, schedule.coherence)
        if len(starts) >= MAX_EPOCHS:
            raise ValueError("too many epochs for one tag range")
        self.schedule, self.max_iter, self.n_total = schedule, int(max_iter), int(n_total)
        self.hints, self.cap = hints, int(cap)
        # first launch: `epoch_chunk` epochs, each continuation twice the previous. Drawing a chain
        # costs ~0.75 us on the host, a launch + read-back ~0.25 ms: 128 keeps coherence-10 solves
        # (~51 epochs) to one launch with few spare chains, coherence-1 solves (~250) to two.
        # Without an explicit chunk, a repeat of a schedule of the same shape sizes its first launch from
        # the epochs the previous solve reached (+ margin): chains beyond them would be drawn for nothing.
        # Only the launch size follows the hint; the chains and iterates do not (a shortfall costs a
        # continuation launch).
        self.hint_key = (float(schedule.coherence), schedule.kind, int(max_iter), int(n_total))
        if epoch_chunk is not None:
            chunk = max(1, int(epoch_chunk))
        elif self.hint_key in hints:
            chunk = max(16, int(hints[self.hint_key]) + 8)
        else:
            chunk = 128
        self.chunk = min(chunk, self.cap)
        self.saved = schedule.save()
        self.E_total = 1 + len(starts)
        # the tables wait for the first window: a cursor made for its early draw stands between the caller
        # and the GPU work the draw is to overlap
        self.Pall = self.ep_start = None
        self.n_drawn = 1
        self.costs: list = []  # hop costs of the drawn epochs 1.., one array per draw
        self.e0 = self.e1 = 0
        self.start_iter, self.pending_in, self.cont, self.hard_stop = 1, 0, False, 0
        self.done = self.iters = self.last_launched = 0
        self._memo: dict = {}
        self._early = None
        look = self.look_ahead()
        if early is not None and look > 0:
            join = early(look)  # exactly what the first window's ensure needs
            if join is not None:
                self._early = (look, join)

    def look_ahead(self) -> int:
        """The last epoch whose chain the next launch needs: its chunk's epochs and the one after them
        (the push targets of theta^hard_stop), if there is one. Draws nothing."""
        e1 = min(self.e0 + self.chunk, self.E_total)
        return e1 if e1 < self.E_total else e1 - 1

    def _ensure(self, upto: int) -> None:  # epochs 0..upto drawn
        if self.Pall is None:
            # epoch e's chain is row e of one (E_total, N) table, filled as chains are drawn (epoch 0: the
            # initial chain); epoch e starts at iteration ep_start[e]
            self.Pall = np.empty((self.E_total, self.n_total), dtype=np.int64)
            self.Pall[0] = self.saved[1]
            self.ep_start = np.concatenate([np.ones(1, dtype=np.int64),
                                            rechains(self.max_iter, self.schedule.coherence)])
        need = upto + 1 - self.n_drawn
        if need <= 0:
            return
        if self._early is not None:  # the early draw covers the first window, the only caller before it is joined
            Pn, Cn = self._early[1]()
            self._early = None
        else:
            Pn, Cn = self.schedule.prefetch_arrays(need)
        self.Pall[self.n_drawn:self.n_drawn + need] = Pn
        self.n_drawn += need
        self.costs.append(Cn)

    def abandon(self) -> None:
        """Give the solve up before its first window: the early draw moved the schedule's RNG ahead of its
        chains, so join the worker and rewind, and a re-run of this schedule draws the same chain sequence
        (seeded D-GADMM reproducibility)."""
        if self._early is not None:
            self._early[1]()
            self._early = None
            self.schedule.restore(self.saved)

    def window(self):
        """The next launch, its missing chains drawn: ``(starts, chains, start_iter, pending_in,
        hard_stop, cont)``. The launch executes epochs e0 .. e1 - 1 from ``start_iter`` to ``hard_stop``
        (0: none, the last epoch is among them); ``starts`` / ``chains`` are views of rows e0 .. look-ahead."""
        self.e1 = e1 = min(self.e0 + self.chunk, self.E_total)
        look = self.look_ahead()
        self._ensure(look)
        self.hard_stop = int(self.ep_start[e1] - 1) if e1 < self.E_total else 0
        return (self.ep_start[self.e0:look + 1], self.Pall[self.e0:look + 1], self.start_iter, self.pending_in,
                self.hard_stop, self.cont)

    def advance(self, done: int, iters: int, last_launched: int, who: str = "") -> bool:
        """Take the outcome of the launch of the last ``window``: whether another launch follows. ``done``
        5: it ran to its hard stop; 1 / 2 / 3: a stop decision at iteration ``iters``, the kernels having
        launched iterations up to ``last_launched``."""
        self.done = int(done)
        if self.done == 5:
            self.last_launched = self.hard_stop
            self.start_iter, self.pending_in, self.cont = self.hard_stop + 1, 1, True
            self.e0 = self.e1 - 1  # epoch 0 of the next launch: this chunk's last (the flush of pending duals)
            self.chunk = min(2 * self.chunk, self.cap)
            return True
        if self.done not in (1, 2, 3):
            raise RuntimeError("D-GADMM chunk%s ended without an outcome (hard stop %d)" % (who, self.hard_stop))
        self.iters, self.last_launched = int(iters), int(last_launched)
        return False

    # ---- what the drawn epochs are (from the first ``window`` on; ``reached`` after the last ``advance``)
    @property
    def starts(self) -> np.ndarray:
        return self.ep_start[:self.n_drawn]

    @property
    def paths(self) -> np.ndarray:
        return self.Pall[:self.n_drawn]

    @property
    def cost0(self) -> np.ndarray:
        return np.asarray(self.saved[2])

    @property
    def span(self) -> int:
        """The iterations the drawn epochs cover."""
        return int(self.ep_start[self.n_drawn] - 1) if self.n_drawn < self.E_total else self.max_iter

    @property
    def reached(self) -> int:
        """The epochs the launches reached; ``reached - 1`` is the epoch of iteration ``last_launched``,
        whose chain an epoch-by-epoch run would have left installed on the engine."""
        return int(np.searchsorted(self.starts, max(self.last_launched, 1), side="right"))

    def _stacked_costs(self):
        if self._memo.get("stacked") != self.n_drawn:
            if self.costs and any(c.dtype == object for c in self.costs):
                Cn = np.empty(sum(len(c) for c in self.costs), dtype=object)
                Cn[:] = [c for cc in self.costs for c in cc]
            else:
                Cn = np.concatenate(self.costs) if self.costs else np.zeros((0, max(self.n_total - 1, 0)))
            self._memo.update(stacked=self.n_drawn, Cn=Cn)
        return self._memo["Cn"]

    def com_cost(self, scale) -> np.ndarray:
        """Cumulative ``com_cost`` of every iteration the drawn epochs cover: per-epoch hop-cost sums times
        ``scale``, one cumsum. Needs no outcome, so it can run while a launch executes (run_persistent's
        on_enqueued) instead of after it; computed once per number of drawn epochs."""
        if self._memo.get("com") != (self.n_drawn, scale):
            Cn = self._stacked_costs()
            # per-epoch cost; the initial cost vector may be ragged (the v0 column-slice quirk)
            csum = Cn.sum(axis=1) if (len(Cn) and Cn.dtype != object) else np.asarray([float(np.sum(c)) for c in Cn])
            per_it = np.concatenate([[float(np.sum(self.saved[2]))], csum]) * scale
            which = np.searchsorted(self.starts, np.arange(1, self.span + 1), side="right") - 1
            self._memo.update(com=(self.n_drawn, scale), cum=np.cumsum(per_it[which]))
        return self._memo["cum"]

    def finish(self) -> None:
        """After the last ``advance``: a repeat of this shape sizes its first launch from here."""
        self.hints[self.hint_key] = self.reached

    def skip_schedule(self) -> None:
        """Leave the schedule where an epoch-by-epoch run to ``iters`` would have left it."""
        count = int(np.searchsorted(self.ep_start[1:], self.iters, side="right"))  # re-chains ascend
        self.schedule.skip(self.saved, self.Pall[1:self.n_drawn], self._stacked_costs(), count)
