"""Up to eight independent D-GADMM solves side by side, one per XCD, in launches of the temporally
blocked kernel's dynamic mode (csrc/kernels/chain_blocked.hip: chain_blocked_dyn_sweep_kernel).

A D-GADMM solve is not one launch: it runs in epoch chunks (a chunk ends at a hard stop just before
its last + 1 epoch; the next launch continues with the same tag salt), and an LDS-staged launch takes
at most ``gadmm_chain_blocked_max_epochs`` epochs. The members of a sweep therefore finish in different
launches. ``DynSweepEngine.run`` works in ROUNDS: each round draws and stages the next chunk of every
unfinished member (the member's own ``EpochCursor``, epoch_chunks.py: first ``epoch_chunk`` epochs,
default 128, then doubling, capped at the LDS rows, plus the look-ahead epoch), launches them
all in one call, reads every control block back and decodes it. A member that ran to its hard stop
(done == 5) continues in the next round; one that reached a stop decision drops out. Slot ``j`` of a
round's launch is the j-th member still running, so a member may change slot, and XCD, between its
chunks: nothing it carries across depends on either (see the kernel's comment).

Members are ``NativeChainEngine``s on one stream. ``coherence_sweep`` builds K members over the same
shards at one rho: one Gram, one table of inverses (as ``ChainSweepEngine.rho_sweep`` passes
``inverses=``) and one padded inverse image shared by all, built once and rebuilt once per
``refresh``. ``DynSweepEngine(members)`` takes engines with their own data (different N and d within
one register class). Every member runs the blocked dynamic mode, whatever its coherence.

What a sweep engine is apart from its kernel and its members' preparation: sweep_base.py.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

from ..ops import native
from ..utils import timing as _timing
from .chain_engine import NativeChainEngine
from .chain_sweep import sweep_capacity
from .epoch_chunks import EpochCursor
from .sweep_base import SweepEngineBase, per_member


@dataclass
class DynSweepRun:
    """Outcome of one member. ``rounds``: launches it took part in (rounds 0 .. rounds - 1);
    ``tail_ticks``: device time (s_memrealtime, 100 MHz) between its stop decision and the end of its
    last round; ``starts`` / ``paths`` / ``costs``: first iterations, chains and hop costs of the
    epochs drawn (epoch 0 = the initial chain, whose cost is ``cost0``); ``span``: the iterations they cover;
    ``cursor``: the member's ``EpochCursor`` (its ``com_cost``)."""
    iters: int
    done: int
    rounds: int
    slot: int
    placed: int
    last_launched: int
    tail_ticks: int
    starts: np.ndarray
    paths: np.ndarray
    costs: list
    cost0: np.ndarray
    span: int
    cursor: EpochCursor

    @property
    def converged(self) -> bool:
        return self.done == 1


@dataclass
class _Member:
    """A member between rounds: its engine, its chunk cursor, and where its last round put it."""
    eng: NativeChainEngine
    cur: EpochCursor
    rounds: int = 0
    placed: int = 0
    slot: int = -1
    stop_tick: int = 0
    fetch: bool = False


class DynSweepEngine(SweepEngineBase):
    _WHAT = "blocked dynamic sweep kernel"
    capacity = staticmethod(sweep_capacity)

    def __init__(self, members: Sequence[NativeChainEngine], stream=None):
        super().__init__(members, stream)
        self.last_round_ms: List[float] = []

    @classmethod
    def coherence_sweep(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int, rho: float,
                        width: int, obj0: float = 0.0, tol: float = 1e-4, max_iters=1000, precomputed=None,
                        residual: bool = False, xcd: int = 2) -> "DynSweepEngine":
        """``width`` members over the same shards at ``rho``. ``max_iters``: one value or one per
        member. ``precomputed``: an ``(A, b, yy)`` Gram to share (else computed here, once)."""
        K, n_total = int(width), int(n_total)
        X, y, stream, shared = cls._shared_tables(X, y, local_ids, n_total, [rho], K, "members", precomputed)
        max_iters = per_member(max_iters, K, int, "max_iters: one value, or one per member")
        A, b, yy, _, Minv, _, V = shared
        members = [NativeChainEngine(X, y, local_ids, n_total, "linear", rho=float(rho), obj0=obj0, tol=tol,
                                     max_iter=max_iters[j], stream=stream, precomputed=(A, b, yy), residual=residual,
                                     xcd=xcd, inverses=(Minv, V, (0, 0, V - 1))) for j in range(K)]
        self = cls(members, stream=stream)
        self._shared = shared
        self._refreshed()
        return self

    def _refreshed(self):
        """One padded inverse image for all members of a shared table: member 0 builds it (in place
        after the first time) on the sweep's stream, the others name the same buffer."""
        m0 = self.members[0]
        m0._minv_pad_version = None
        m0._attach_minv_pad(native.PersistArgs())
        for m in self.members[1:]:
            m._minv_pad, m._minv_pad_version = m0._minv_pad, m._minv_version

    def run(self, schedules: Sequence, epoch_chunk=None, lag: int = 4, timeout_s: float = 20.0) -> List[DynSweepRun]:
        """Reset every member and run member j over ``schedules[j]`` (a ``PathSchedule`` at its initial
        chain, already installed with ``set_path``) to its own stop; one ``DynSweepRun`` per member.
        Each member then answers ``traces`` / ``primal_residual`` as after its own ``run_persistent``.
        ``epoch_chunk``: epochs of every member's first launch (None: 128, or the member's hint).
        ``ResidencyError``: the launcher refused a round before launching; ``ValueError``: a member is
        not eligible; ``HandoffTimeout`` names the slot, after every control block has been read, and
        nothing more is started on the GPU in this call."""
        if len(schedules) != len(self.members):
            raise ValueError("one schedule per member")
        for m in self.members:
            m.reset()
        cap = int(self.lib.gadmm_chain_blocked_max_epochs()) - 1  # a launch's epoch tables are staged in LDS
        state = [_Member(m, EpochCursor(s, m.max_iter, m.n_total, m.__dict__.setdefault("_dyn_epoch_hint", {}),
                                        epoch_chunk, cap)) for m, s in zip(self.members, schedules)]
        live = list(range(len(state)))
        self.last_round_ms = []
        round_end = []
        kname = None
        while live:
            t0 = time.perf_counter()
            _timing.host_stamp("dsw:round")
            K = len(live)
            batch = (native.PersistArgs * K)()
            plans = []
            for slot, i in enumerate(live):
                s = state[i]
                # drawn member after member on this thread: the draws are most of the host time ahead of a
                # launch (~2 us per chain at N = 50), but handing them to host threads did not shorten it
                # (the schedule's batched draw holds the interpreter lock: profiles/dyn_sweep)
                starts, chains, start_iter, pending_in, hard_stop, cont = s.cur.window()
                _timing.host_stamp("dsw:drawn")
                try:
                    pa, plan = s.eng.prepare_blocked_dyn(
                        np.ascontiguousarray(starts), np.ascontiguousarray(chains), lag=lag, timeout_s=timeout_s,
                        start_iter=start_iter, pending_in=pending_in, hard_stop=hard_stop, cont=cont)
                except ValueError as e:
                    raise ValueError("sweep member %d: %s" % (i, e))
                batch[slot] = pa
                plans.append(plan)
                s.slot = slot
            _timing.host_stamp("dsw:staged")
            if kname is None:
                kname = "blocked-dyn-sweep(K=%d,k=%s,L=%s)" % (
                    K, "/".join(sorted({str(p[0]) for p in plans})), "/".join(sorted({str(p[1]) for p in plans})))
                self.last_kernel = kname
                for m in self.members:
                    m.last_kernel = kname
            self._launch(self.lib.gadmm_chain_blocked_dyn_sweep_launch, batch, K, "chain_blocked_dyn_sweep_launch")
            _timing.host_stamp("dsw:launched")
            fetch, codes = self._collect([state[i].eng for i in live], True, t0, "dsw:synced",
                                         lambda slot: "slot %d (member %d)" % (slot, live[slot]))
            for i, f in zip(live, fetch):
                s = state[i]
                s.fetch = s.eng._tr_valid = f
                s.placed = s.eng.last_placed
                s.eng.last_timeline = s.eng.last_timeline_slots = None
            nxt_live = []
            ticks = []
            for i, c in zip(live, codes):
                s = state[i]
                done, conv, nxt = c[1], c[2], c[0]
                s.rounds += 1
                last_it = conv if done in (1, 2, 3) else s.cur.hard_stop  # the last iteration decided in this round
                if not 1 <= last_it <= s.eng.trace.numel():
                    s.stop_tick = 0
                elif s.fetch:
                    s.stop_tick = self._stop_tick(s.eng, last_it)
                else:  # a trace too long for the one-copy read-back: this stamp alone (a blocking 8-byte copy)
                    s.stop_tick = int(s.eng.tstamp[last_it - 1:last_it].cpu().item())
                ticks.append(s.stop_tick)
                if s.cur.advance(done, conv, nxt - 1, " of member %d" % i):
                    nxt_live.append(i)  # ran to its hard stop: the next round continues it with the same tag salt
            round_end.append(max(ticks))
            self.last_round_ms.append((time.perf_counter() - t0) * 1e3)
            live = nxt_live
        self.last_wall_ms = float(sum(self.last_round_ms))
        out = []
        for s in state:
            c = s.cur
            c.finish()
            end = round_end[s.rounds - 1]
            out.append(DynSweepRun(iters=c.iters, done=c.done, rounds=s.rounds, slot=s.slot, placed=s.placed,
                                   last_launched=c.last_launched,
                                   tail_ticks=max(end - s.stop_tick, 0) if s.stop_tick > 0 else 0,
                                   starts=c.starts, paths=c.paths, costs=c.costs, cost0=c.cost0, span=c.span, cursor=c))
        return out
