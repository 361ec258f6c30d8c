"""Up to eight independent inner-GD logistic GADMM solves in ONE launch, one solve per XCD
(csrc/kernels/chain_logistic_sweep.hip: chain_persistent_logistic_sweep_kernel).

The logistic solve is the most latency-bound one here (every inner step is one dependent register GEMV),
and what a user does with it is run it several times: at several rho, ``max_inner`` or ``inner_tol``. The
single solve (one workgroup per worker plus the monitor) is packed onto one of the MI355X's eight XCDs
by an 8x wider grid whose blocks ``b % 8 != 0`` exit at once; here slot ``j`` of a launch runs member
``j`` on the blocks ``b % 8 == j``. A member is a ``NativeChainEngine(model="logistic",
local_solver="gd")`` with its own iterates, duals, granule tables, control block, trace, rings and
placement-check buffer; the members share one stream and, read-only, the shards ``X``, ``Y``.

``GADMM_LOGISTIC_ZREC`` picks the worker layout of the whole launch, as for the single solve: the
two-wave margins recursion (default, ``persistent-logistic-sweep(zrec)``) or the one-wave worker
(``=0``, ``persistent-logistic-sweep(1w)``, bit-identical to the graph engine).

What a sweep engine is apart from its kernel and its members' preparation: sweep_base.py.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import torch

from ..ops import native
from ..parallel.topology import Placement
from ..utils.env import getenv
from .chain_engine import EngineRun, NativeChainEngine
from .sweep_base import SweepEngineBase, per_member


def logistic_sweep_capacity() -> int:
    """Solves one logistic sweep launch takes (gadmm_chain_persistent_logistic_sweep_capacity)."""
    return int(native.require().gadmm_chain_persistent_logistic_sweep_capacity())


class LogisticSweepEngine(SweepEngineBase):
    _SPLIT = 52
    _CLASSES = "max(d, m) <= 52 and 53..64"
    _SOLVES = "inner-GD solves with max(d, m) <= 64"
    _WHAT = "persistent logistic sweep kernel"
    _MODEL = "logistic"
    _ARGS = native.LogiSweepArgs

    capacity = staticmethod(logistic_sweep_capacity)

    @staticmethod
    def _size(m) -> int:
        return max(m.d, m.m)

    def _member_defect(self, m):
        if m.model != "logistic" or m.local_solver != "gd" or max(m.d, m.m) > 64:
            return ": one-GPU logistic %s only" % self._SOLVES
        return " has no chain installed (set_path)" if m.plan is None else None

    def __init__(self, members: Sequence[NativeChainEngine], stream: Optional[torch.cuda.Stream] = None):
        super().__init__(members, stream)
        native.check_logi_sweep_abi(self.lib)

    @classmethod
    def build(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int, members: Sequence,
              obj0: float = 0.0, tols=1e-4, max_iters=1000, lam: float = 0.0,
              placement: Optional[Placement] = None, xcd: int = 2, residual: bool = True) -> "LogisticSweepEngine":
        """Members = the same shards under every ``(rho, step, max_inner, inner_tol)`` of ``members``.
        ``tols`` / ``max_iters``: one value or one per member."""
        if not X.is_cuda:
            raise ValueError("%s runs on a HIP device" % cls.__name__)
        cfgs = [(float(r), float(s), int(mi), float(it)) for r, s, mi, it in members]
        K, n_total = len(cfgs), int(n_total)
        if K < 1 or K > cls.capacity():
            raise ValueError("%d members: one sweep launch takes 1..%d" % (K, cls.capacity()))
        if len(local_ids) != n_total:
            raise ValueError("a sweep member holds every worker of its chain (one GPU)")
        if max(int(X.shape[1]), int(X.shape[2])) > 64:
            raise ValueError("the persistent logistic kernel takes max(d, m) <= 64 (d = %d, m = %d)"
                             % (int(X.shape[2]), int(X.shape[1])))
        tols = per_member(tols, K, float, "tols / max_iters: one value, or one per member")
        max_iters = per_member(max_iters, K, int, "tols / max_iters: one value, or one per member")
        X = X.to(torch.float64).contiguous()  # every member reads these two tensors
        y = y.to(torch.float64).contiguous()
        stream = torch.cuda.Stream(X.device)
        stream.wait_stream(torch.cuda.current_stream(X.device))
        pl = placement if placement is not None else Placement.contiguous(n_total, 1)
        engines = []
        for j, (rho, step, max_inner, inner_tol) in enumerate(cfgs):
            m = NativeChainEngine(X, y, local_ids, n_total, "logistic", rho=rho, obj0=obj0, tol=tols[j],
                                  max_iter=max_iters[j], lam=lam, step=step, max_inner=max_inner, inner_tol=inner_tol,
                                  stream=stream, local_solver="gd", residual=residual, xcd=xcd)
            m.set_path(list(range(n_total)), pl, 0)
            engines.append(m)
        return cls(engines, stream=stream)

    def blocks(self) -> List[int]:
        """Workgroups of every member (one per worker + the monitor)."""
        return [m.n_total + 1 for m in self.members]

    def run(self, lag: int = 4, timeout_s: float = 20.0, fetch_trace: bool = True) -> List[EngineRun]:
        """Reset every member and run all of them in one launch; one ``EngineRun`` per member. Each member
        then answers ``traces`` / ``objective_trace`` / ``local_theta`` / ``ctl_state`` as after its own
        ``run_persistent``; ``last_placed`` holds each member's placement verdict. ``ResidencyError``: the
        launcher refused before launching (the workgroups cannot all be resident); ``ValueError``: a member
        is not eligible; ``HandoffTimeout`` names the slot."""
        K = len(self.members)
        for m in self.members:
            m.reset()
        batch = (native.LogiSweepArgs * K)()
        for j, m in enumerate(self.members):
            batch[j].p = m._persist_args(lag, lag + 4, timeout_s, 1, 0, None, False, 0, False)[0]
            batch[j].g = m._logi_args()
        self.last_kernel = "persistent-logistic-sweep(%s)" % ("1w" if getenv("GADMM_LOGISTIC_ZREC", "1").startswith("0") else "zrec")
        for m in self.members:
            m.last_kernel = self.last_kernel
        t0 = time.perf_counter()
        self._launch(self.lib.gadmm_chain_persistent_logistic_sweep_launch, batch, K,
                     "chain_persistent_logistic_sweep_launch")
        fetch, _ = self._collect(self.members, fetch_trace, t0)
        out = []
        for j, (m, f) in enumerate(zip(self.members, fetch)):
            m._tr_valid = f
            m.last_timeline = m.last_timeline_slots = None
            done, conv, nxt = m._decode_ctl("persistent logistic sweep kernel: slot %d" % j)
            out.append(EngineRun(conv, done, nxt - 1, 1, self.last_wall_ms, 0, 0, 0, 0))
        return out
