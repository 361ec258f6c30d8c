"""Up to eight independent D-GADMM solves side by side, one per XCD, in launches of the temporally
blocked kernel's dynamic mode (csrc/kernels/chain_blocked.hip: chain_blocked_dyn_sweep_kernel).

A D-GADMM solve is not one launch: it runs in epoch chunks (a chunk ends at a hard stop just before
its last + 1 epoch; the next launch continues with the same tag salt), and an LDS-staged launch takes
at most ``gadmm_chain_blocked_max_epochs`` epochs. The members of a sweep therefore finish in different
launches. ``DynSweepEngine.run`` works in ROUNDS: each round draws and stages the next chunk of every
unfinished member (the member's own chunk rule, as ``_chain_admm_native``: first ``epoch_chunk``
epochs, default 128, then doubling, capped at the LDS rows, plus the look-ahead epoch), launches them
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
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np
import torch

from ..ops import native
from ..parallel.topology import rechain_iterations
from ..utils import timing as _timing
from .chain_engine import NativeChainEngine
from .chain_sweep import sweep_capacity
from .sweep_base import SweepEngineBase, per_member


@dataclass
class DynSweepRun:
    """Outcome of one member. ``rounds``: launches it took part in (rounds 0 .. rounds - 1);
    ``tail_ticks``: device time (s_memrealtime, 100 MHz) between its stop decision and the end of its
    last round; ``starts`` / ``paths`` / ``costs``: first iterations, chains and hop costs of the
    epochs drawn (epoch 0 = the initial chain, whose cost is ``cost0``); ``span``: the iterations they cover."""
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

    @property
    def converged(self) -> bool:
        return self.done == 1


@dataclass
class _Member:
    """A member's chunk cursor between rounds."""
    eng: NativeChainEngine
    schedule: object
    saved: tuple
    ep_start: np.ndarray
    Pall: np.ndarray
    E_total: int
    chunk: int
    cap: int
    hint_key: tuple
    n_drawn: int = 1
    costs: list = field(default_factory=list)
    e0: int = 0
    e1: int = 0
    start_iter: int = 1
    pending_in: int = 0
    cont: bool = False
    hard_stop: int = 0
    rounds: int = 0
    done: int = 0
    iters: int = 0
    placed: int = 0
    slot: int = -1
    last_launched: int = 0
    stop_tick: int = 0
    fetch: bool = False

    def ensure(self, upto: int):  # epochs 0..upto drawn (only the chains a member reaches)
        need = upto + 1 - self.n_drawn
        if need > 0:
            Pn, Cn = self.schedule.prefetch_arrays(need)
            self.Pall[self.n_drawn:self.n_drawn + need] = Pn
            self.n_drawn += need
            self.costs.append(Cn)


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

    # ---------------------------------------------------------------------------------------------
    def _begin(self, m: NativeChainEngine, schedule, epoch_chunk) -> _Member:
        max_iter = m.max_iter
        rechains = rechain_iterations(max_iter, schedule.coherence)
        if len(rechains) >= (1 << 20):
            raise ValueError("too many epochs for one tag range")
        cap = int(self.lib.gadmm_chain_blocked_max_epochs()) - 1
        hint_key = (float(schedule.coherence), schedule.kind, int(max_iter), int(m.n_total))
        hints = m.__dict__.setdefault("_dyn_epoch_hint", {})
        if epoch_chunk is not None:
            chunk = max(1, int(epoch_chunk))
        elif hint_key in hints:  # a repeat sizes its first launch from the epochs the last solve reached
            chunk = max(16, int(hints[hint_key]) + 8)
        else:
            chunk = 128
        saved = schedule.save()
        E_total = 1 + len(rechains)
        Pall = np.empty((E_total, m.n_total), dtype=np.int64)
        Pall[0] = saved[1]
        ep_start = np.concatenate([np.ones(1, dtype=np.int64), np.asarray(rechains, dtype=np.int64)])
        return _Member(eng=m, schedule=schedule, saved=saved, ep_start=ep_start, Pall=Pall, E_total=E_total,
                       chunk=min(chunk, cap), cap=cap, hint_key=hint_key)

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
        state = [self._begin(m, s, epoch_chunk) for m, s in zip(self.members, schedules)]
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
                s.e1 = min(s.e0 + s.chunk, s.E_total)  # this launch executes epochs e0 .. e1 - 1
                look = s.e1 if s.e1 < s.E_total else s.e1 - 1  # + the next epoch's chain
                # drawn member after member on this thread: the draws are most of the host time ahead of a
                # launch (~2 us per chain at N = 50), but handing them to host threads did not shorten it
                # (the schedule's batched draw holds the interpreter lock: profiles/dyn_sweep)
                s.ensure(look)
                _timing.host_stamp("dsw:drawn")
                s.hard_stop = int(s.ep_start[s.e1] - 1) if s.e1 < s.E_total else 0
                try:
                    pa, plan = s.eng.prepare_blocked_dyn(
                        np.ascontiguousarray(s.ep_start[s.e0:look + 1]), np.ascontiguousarray(s.Pall[s.e0:look + 1]),
                        lag=lag, timeout_s=timeout_s, start_iter=s.start_iter, pending_in=s.pending_in,
                        hard_stop=s.hard_stop, cont=s.cont)
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
                s.done = done
                last_it = conv if done in (1, 2, 3) else s.hard_stop  # the last iteration decided in this round
                if not 1 <= last_it <= s.eng.trace.numel():
                    s.stop_tick = 0
                elif s.fetch:
                    s.stop_tick = self._stop_tick(s.eng, last_it)
                else:  # a trace too long for the one-copy read-back: this stamp alone (a blocking 8-byte copy)
                    s.stop_tick = int(s.eng.tstamp[last_it - 1:last_it].cpu().item())
                ticks.append(s.stop_tick)
                if done == 5:  # ran to its hard stop: the next round continues it with the same tag salt
                    s.last_launched = s.hard_stop
                    s.start_iter, s.pending_in, s.cont = s.hard_stop + 1, 1, True
                    s.e0 = s.e1 - 1  # epoch 0 of the next launch: this chunk's last (the pending duals' flush)
                    s.chunk = min(2 * s.chunk, s.cap)
                    nxt_live.append(i)
                elif done in (1, 2, 3):
                    s.iters = conv
                    s.last_launched = nxt - 1
                else:
                    raise RuntimeError("D-GADMM chunk of member %d ended without an outcome (hard stop %d)"
                                       % (i, s.hard_stop))
            round_end.append(max(ticks))
            self.last_round_ms.append((time.perf_counter() - t0) * 1e3)
            live = nxt_live
        self.last_wall_ms = float(sum(self.last_round_ms))
        out = []
        for s in state:
            hints = s.eng.__dict__.setdefault("_dyn_epoch_hint", {})
            starts = s.ep_start[:s.n_drawn]
            hints[s.hint_key] = int(np.searchsorted(starts, max(s.last_launched, 1), side="right"))
            end = round_end[s.rounds - 1]
            out.append(DynSweepRun(iters=s.iters, done=s.done, rounds=s.rounds, slot=s.slot, placed=s.placed,
                                   last_launched=s.last_launched,
                                   tail_ticks=max(end - s.stop_tick, 0) if s.stop_tick > 0 else 0,
                                   starts=starts, paths=s.Pall[:s.n_drawn], costs=s.costs,
                                   cost0=np.asarray(s.saved[2]), span=int(s.ep_start[s.n_drawn] - 1) if s.n_drawn < s.E_total else int(s.eng.max_iter)))
        return out
