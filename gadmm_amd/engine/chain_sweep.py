"""Up to eight independent static-chain GADMM solves in ONE launch of the temporally blocked kernel,
one solve per XCD (csrc/kernels/chain_blocked.hip: chain_blocked_sweep_kernel).

The single solve is packed onto one of the MI355X's eight XCDs by an 8x wider grid whose blocks
``b % 8 != 0`` exit at once; here slot ``j`` of a launch runs member ``j`` on the blocks ``b % 8 == j``.
A member is a ``NativeChainEngine`` (its own state, control block, trace, granule tables and
placement-check buffer); the members share one stream, so every reset, zero-fill and table
allocation of every member is ordered ahead of the one launch, and only read-only inputs (the Gram
and, in a rho sweep, one table of inverses) are shared between slots.

Two ways to build one:

* ``ChainSweepEngine.rho_sweep(X, y, local_ids, n_total, rhos, ...)``: the same shards at K values of
  rho -- one Gram, ONE ``spd_inverse`` launch for all K x V shifts (member j reads variants
  ``j V .. j V + V - 1`` of the shared ``(N, K V, d, d)`` table); ``refresh(X, y)`` recomputes both
  in place;
* ``ChainSweepEngine(members)``: already-built engines (different data, N and d within one register
  class of the kernel: d <= 32 or 33..52); they are moved onto the sweep's stream.

What a sweep engine is apart from its kernel and its members' preparation: sweep_base.py.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import torch

from ..ops import native
from ..parallel.topology import Placement
from .chain_engine import EngineRun, NativeChainEngine
from .sweep_base import SweepEngineBase, per_member


def sweep_capacity() -> int:
    """Solves one sweep launch takes (gadmm_chain_blocked_sweep_capacity)."""
    return int(native.require().gadmm_chain_blocked_sweep_capacity())


class ChainSweepEngine(SweepEngineBase):
    capacity = staticmethod(sweep_capacity)

    def _member_defect(self, m):
        return " has no chain installed (set_path)" if m.plan is None else None

    @classmethod
    def rho_sweep(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int,
                  rhos: Sequence[float], obj0: float = 0.0, tols=1e-4, max_iters=1000, precomputed=None,
                  placement: Optional[Placement] = None, residual: bool = False, xcd: int = 2) -> "ChainSweepEngine":
        """Members = the same shards at every rho of ``rhos``. ``tols`` / ``max_iters``: one value or one
        per member. ``precomputed``: an ``(A, b, yy)`` Gram to share (else computed here, once)."""
        K, n_total = len(rhos), int(n_total)
        X, y, stream, shared = cls._shared_tables(X, y, local_ids, n_total, rhos, K, "values of rho", precomputed)
        tols = per_member(tols, K, float, "tols / max_iters: one value, or one per rho")
        max_iters = per_member(max_iters, K, int, "tols / max_iters: one value, or one per rho")
        A, b, yy, _, Minv, _, V = shared
        pl = placement if placement is not None else Placement.contiguous(n_total, 1)
        members = []
        for j, rho in enumerate(rhos):
            m = NativeChainEngine(X, y, local_ids, n_total, "linear", rho=float(rho), obj0=obj0, tol=tols[j],
                                  max_iter=max_iters[j], stream=stream, precomputed=(A, b, yy), residual=residual,
                                  xcd=xcd, inverses=(Minv, K * V, (j * V, j * V, j * V + V - 1)))
            m.set_path(list(range(n_total)), pl, 0)
            members.append(m)
        self = cls(members, stream=stream)
        self._shared = shared
        return self

    def blocks(self) -> List[int]:
        """Workgroups of every member (worker + objective workgroups + the monitor)."""
        out = []
        for j, m in enumerate(self.members):
            plan = m.blocked_plan()
            if plan is None or plan[3] != 1:
                raise ValueError("member %d has no 12-wave blocked plan (n=%d, d=%d)" % (j, m.n_total, m.d))
            out.append(plan[2] + (m.n_total + 11) // 12 + 1)
        return out

    def run(self, lag: int = 4, timeout_s: float = 20.0, fetch_trace: bool = True) -> List[EngineRun]:
        """Reset every member and run all of them in one launch; one ``EngineRun`` per member. Each
        member then answers ``traces`` / ``objective_trace`` / ``time_trace`` / ``local_theta`` /
        ``ctl_state`` as after its own ``run_persistent``; ``last_placed`` holds each member's placement
        verdict. ``ResidencyError``: the launcher refused before launching (the workgroups cannot all
        be resident); ``ValueError``: a member is not eligible; ``HandoffTimeout`` names the slot."""
        K = len(self.members)
        for m in self.members:
            m.reset()
        batch = (native.PersistArgs * K)()
        plans = []
        for j, m in enumerate(self.members):
            try:
                batch[j], plan = m.prepare_blocked(lag=lag, timeout_s=timeout_s)
            except ValueError as e:
                raise ValueError("sweep member %d: %s" % (j, e))
            plans.append(plan)
        self.last_kernel = "blocked-sweep(K=%d,k=%s,L=%s)" % (
            K, "/".join(sorted({str(p[0]) for p in plans})), "/".join(sorted({str(p[1]) for p in plans})))
        for m in self.members:
            m.last_kernel = self.last_kernel
        t0 = time.perf_counter()
        self._launch(self.lib.gadmm_chain_blocked_sweep_launch, batch, K, "chain_blocked_sweep_launch")
        fetch, _ = self._collect(self.members, fetch_trace, t0)
        return [m.finish_blocked(1, self.last_wall_ms, f, "blocked sweep kernel: slot %d" % j)
                for j, (m, f) in enumerate(zip(self.members, fetch))]
