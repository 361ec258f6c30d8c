"""What the sweep engines share: up to eight ``NativeChainEngine`` members on one stream, run side
by side in one kernel launch, one solve per XCD (chain_sweep.py: static chains at several rho;
quant_sweep.py: Q/CQ-GADMM configs; dyn_sweep.py: D-GADMM coherences, in rounds of launches;
graph_sweep.py: GGADMM / Q-GGADMM over graphs, whose members are ``NativeGraphEngine``, which offers the
same surface: ``model``, ``nranks``, ``n_local`` / ``n_total``, ``adopt_stream``, ``_queue_readback``).

``SweepEngineBase`` owns the member validation, the stream, the launcher's staging pair, the shared
Gram and table of inverses of a sweep over the same shards (``_shared``, ``refresh``), the launch call
with its return codes, and the read-back of every member's control block after the one synchronize.
An engine adds its kernel's register classes, what it asks of a member, its builder and its ``run``.
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Optional, Sequence

import torch

from ..ops import native
from ..ops.linalg import gram, spd_inverse
from ..utils import timing as _timing
from .chain_engine import EngineRun, HandoffTimeout, NativeChainEngine, ResidencyError


def per_member(value, K: int, cast, what: str) -> list:
    """``value`` (one for all, or one per member) as a list of K."""
    out = [cast(value)] * K if not isinstance(value, (list, tuple)) else [cast(v) for v in value]
    if len(out) != K:
        raise ValueError(what)
    return out


class SweepEngineBase:
    _SPLIT = 32  # members with d <= _SPLIT and d > _SPLIT run on different instantiations of the kernel
    _CLASSES = "d <= 32 and 33..52"
    _SOLVES = "closed-form solves"  # what a member is, in the refusal of one that is not
    _WHAT = "blocked sweep kernel"  # prefix of a hand-off timeout's text

    @staticmethod
    def capacity() -> int:
        """Solves one launch takes."""
        raise NotImplementedError

    def _member_defect(self, m: NativeChainEngine) -> Optional[str]:
        """What else keeps ``m`` out of this sweep (the text after ``member j``), or None."""
        return None

    def __init__(self, members: Sequence[NativeChainEngine], stream: Optional[torch.cuda.Stream] = None):
        members = list(members)
        if not members:
            raise ValueError("a sweep needs at least one member")
        cap = self.capacity()
        if len(members) > cap:
            raise ValueError("%d members: one sweep launch takes at most %d" % (len(members), cap))
        if len({id(m) for m in members}) != len(members):
            raise ValueError("a member appears twice (every slot needs its own state)")
        dev = members[0].device
        if any(m.device != dev for m in members):
            raise ValueError("the members of a sweep live on one device")
        for j, m in enumerate(members):
            defect = self._member_defect(m)
            if defect is None and (m.model != "linear" or m.nranks != 1 or m.n_local != m.n_total):
                defect = ": one-GPU linear %s only" % self._SOLVES
            if defect is not None:
                raise ValueError("member %d%s" % (j, defect))
        if len({m.d <= self._SPLIT for m in members}) != 1:
            raise ValueError("members of different register classes (%s) cannot share a launch" % self._CLASSES)
        self.lib = native.require()
        self.device = dev
        self.members = members
        self.stream = stream if stream is not None else members[0].stream
        for m in members:  # one stream: every member's resets, table copies and zero-fills precede the launch
            if m.stream is not self.stream:
                m.adopt_stream(self.stream)
        nbytes = cap * ctypes.sizeof(native.PersistArgs)
        # the launcher's staging pair: the slots' PersistArgs go up in one async copy ahead of the kernel
        self._stage_host = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        self._stage_dev = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self._shared = None
        self.last_kernel = None
        self.last_placed: List[int] = []
        self.last_wall_ms = 0.0

    # ---- a sweep over the same shards: one Gram, one table of inverses ------------------------------
    @classmethod
    def _shared_tables(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int,
                       rhos: Sequence[float], K: int, noun: str, precomputed=None):
        """For a builder of K members over the shards ``X, y``: the checks, the members' stream, the shared
        Gram and ONE ``spd_inverse`` launch for the degree-1 and degree-2 shifts of every rho of ``rhos``,
        as ``NativeChainEngine._build_inverses`` picks them: ``rhos[i]`` is variants ``i V .. i V + V - 1``
        of the table. Returns ``(X, y, stream, shared)``, ``shared = (A, b, yy, shifts, Minv,
        status, V)``."""
        if not X.is_cuda:
            raise ValueError("%s runs on a HIP device" % cls.__name__)
        if K < 1 or K > cls.capacity():
            raise ValueError("%d %s: one sweep launch takes 1..%d" % (K, noun, cls.capacity()))
        X = X.to(torch.float64).contiguous()
        y = y.to(torch.float64).contiguous()
        if len(local_ids) != n_total:
            raise ValueError("a sweep member holds every worker of its chain (one GPU)")
        if n_total < 2:
            raise ValueError("a chain needs at least two workers")
        dev = X.device
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        per = [[r] if n_total == 2 else [r, 2.0 * r] for r in (float(r) for r in rhos)]
        V = len(per[0])
        with torch.cuda.stream(stream):
            A, b, yy = precomputed if precomputed is not None else gram(X, y)
            shifts = torch.tensor([s for p in per for s in p], dtype=torch.float64, device=dev).unsqueeze(0).expand(
                A.shape[0], -1).contiguous()
            Minv = spd_inverse(A, shifts)  # ONE launch for all the shifts (checks positive definiteness)
        return X, y, stream, (A, b, yy, shifts, Minv, torch.zeros((1,), dtype=torch.int32, device=dev), V)

    def _refreshed(self) -> None:
        """After ``refresh`` has rewritten the shared tables (an engine with more shared state rebuilds it)."""

    def refresh(self, X: torch.Tensor, y: torch.Tensor):
        """Recompute the shared Gram and the shared table of inverses from the raw shards, in place, on
        the sweep's stream: one Gram and one inverse launch for the whole sweep (engines of a builder)."""
        if self._shared is None:
            raise RuntimeError("refresh: members built elsewhere refresh themselves")
        A, b, yy, shifts, Minv, status, _ = self._shared
        with torch.cuda.stream(self.stream):
            gram(X, y, out=(A, b, yy))
            spd_inverse(A, shifts, out=Minv, check_status=False, status=status)
        for m in self.members:
            m._minv_version += 1
        self._refreshed()

    def set_targets(self, obj0: float, tols) -> None:
        for m, t in zip(self.members, per_member(tols, len(self.members), float, "tols: one value, or one per member")):
            m.set_targets(obj0, t)

    # ---- one launch ------------------------------------------------------------------------------
    def _launch(self, fn, batch, K: int, what: str) -> None:
        """``fn``: a sweep launcher of the library. ``ResidencyError``: it refused before launching (the
        workgroups cannot all be resident); ``ValueError``: an entry is not eligible."""
        rc = int(fn(batch, K, self._stage_host.data_ptr(), self._stage_dev.data_ptr(), self.stream.cuda_stream))
        if rc == -2:
            raise ResidencyError(self.lib.gadmm_last_error().decode())
        if rc == -1:
            raise ValueError(self.lib.gadmm_last_error().decode())
        native.check(rc, what)

    def _collect(self, members: Sequence[NativeChainEngine], fetch_trace: bool, t0: float, stamp: Optional[str] = None,
                 slot_name=lambda slot: "slot %d" % slot):
        """After the launch of ``members`` (slot j = members[j]): queue every read-back, one synchronize
        (``last_wall_ms`` = the time since ``t0``), then every control block (host memory only) and only
        then the verdicts: after a timeout nothing more is started on the GPU in this call.
        ``HandoffTimeout`` names the first slot that timed out. Returns ``(fetch, codes)`` per member."""
        fetch = [m._queue_readback(fetch_trace) for m in members]
        self.stream.synchronize()
        self.last_wall_ms = (time.perf_counter() - t0) * 1e3
        if stamp is not None:
            _timing.host_stamp(stamp)
        codes = [m._ctl_host.tolist() for m in members]
        for m, c in zip(members, codes):
            m.last_placed = c[6]
        self.last_placed = [m.last_placed for m in self.members]  # (a member not in this launch keeps its last)
        bad = [j for j, c in enumerate(codes) if c[1] == 4]
        if bad:
            raise HandoffTimeout("%s: %s timed out (hand-off never completed)" % (self._WHAT, slot_name(bad[0])))
        return fetch, codes

    @staticmethod
    def _stop_tick(m: NativeChainEngine, it: int) -> int:
        """Device clock (s_memrealtime, 100 MHz) stamped with iteration ``it``'s decision, from ``m``'s
        pinned read-back block of a run that fetched the trace."""
        nt = m.trace.numel()
        return int(m._rb_host_np[8 + nt + it - 1:8 + nt + it].view("int64")[0])

    def stop_ticks(self, runs: Sequence[EngineRun]) -> List[int]:
        """Device clock of each member's stop decision in the last run, read from the pinned read-back
        block (``run(fetch_trace=True)``); 0 where no decision was stamped."""
        return [self._stop_tick(m, r.iters)
                if getattr(m, "_tr_valid", False) and 1 <= r.iters <= m.trace.numel() else 0
                for m, r in zip(self.members, runs)]

    def close(self):
        for m in self.members:
            m.close()
