"""Up to eight independent Q-GADMM solves in ONE launch of the persistent Q kernel's body, one solve per
XCD (csrc/kernels/chain_quant.hip: chain_persistent_q_sweep_kernel).

Q-GADMM is the one algorithm here whose result depends on a random draw, so a useful run of it is a
batch: several bit widths, several rho, several quantizer seeds. The single solve (one wave per worker
plus the monitor) is packed onto one of the MI355X's eight XCDs by an 8x wider grid whose blocks
``b % 8 != 0`` exit at once; here slot ``j`` of a launch runs member ``j`` on the blocks ``b % 8 == j``.
A member is a ``NativeChainEngine`` with ``quant`` set (its own public models, duals, true iterates,
message table, control block, trace, rings and placement-check buffer); the members share one stream,
so every reset, zero-fill and table allocation of every member is ordered ahead of the one launch, and
only read-only inputs (the Gram and one table of inverses) are shared between slots.

Two ways to build one:

* ``QuantSweepEngine.build(X, y, local_ids, n_total, configs, ...)`` with ``configs = [(rho, bits,
  seed), ...]``: the same shards under every config -- one Gram, ONE ``spd_inverse`` launch for the
  distinct rho x degree shifts (members with the same rho read the same variants of the shared table);
  ``refresh(X, y)`` recomputes both in place;
* ``QuantSweepEngine(members)``: already-built engines (different data, N, d within one register class
  of the kernel -- d <= 52 or 53..64 -- and bits); they are moved onto the sweep's stream.

CQ-GADMM members (``censor=(tau0, xi)``): a sweep with at least one censored member runs on
``chain_persistent_cq_sweep_kernel``; its uncensored members bring an all-zero threshold table, under
which the censored body computes Q-GADMM bit for bit. A sweep without one keeps the Q kernel.

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


def quant_sweep_capacity() -> int:
    """Solves one Q sweep launch takes (gadmm_chain_persistent_q_sweep_capacity)."""
    return int(native.require().gadmm_chain_persistent_q_sweep_capacity())


class QuantSweepEngine(SweepEngineBase):
    _SPLIT = 52
    _CLASSES = "d <= 52 and 53..64"
    _SOLVES = "Q-GADMM solves with d <= 64"
    _WHAT = "persistent Q sweep kernel"

    capacity = staticmethod(quant_sweep_capacity)

    def _member_defect(self, m):
        if m.quant is None:
            return " is not a Q-GADMM engine (quant=(bits, seed))"
        if m.d > 64:
            return ": one-GPU linear %s only" % self._SOLVES
        return " has no chain installed (set_path)" if m.plan is None else None

    @classmethod
    def build(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int, configs: Sequence,
              obj0: float = 0.0, tols=1e-4, max_iters=1000, precomputed=None,
              placement: Optional[Placement] = None, xcd: int = 2, censors: Optional[Sequence] = None
              ) -> "QuantSweepEngine":
        """Members = the same shards under every ``(rho, bits, seed)`` of ``configs``. ``tols`` /
        ``max_iters``: one value or one per member. ``precomputed``: an ``(A, b, yy)`` Gram to share (else
        computed here, once). ``censors``: one ``(tau0, xi)`` or None per config (CQ-GADMM members)."""
        configs = [(float(r), int(b), int(s)) for r, b, s in configs]
        K, n_total = len(configs), int(n_total)
        censors = [None] * K if censors is None else list(censors)
        if len(censors) != K:
            raise ValueError("censors: one (tau0, xi) or None per config")
        if int(X.shape[2]) > 64:
            raise ValueError("the persistent Q kernel takes d <= 64 (d = %d)" % int(X.shape[2]))
        rhos = list(dict.fromkeys(r for r, _, _ in configs))  # members with the same rho read the same variants
        X, y, stream, shared = cls._shared_tables(X, y, local_ids, n_total, rhos, K, "configs", precomputed)
        tols = per_member(tols, K, float, "tols / max_iters: one value, or one per config")
        max_iters = per_member(max_iters, K, int, "tols / max_iters: one value, or one per config")
        A, b, yy, _, Minv, _, V = shared
        pl = placement if placement is not None else Placement.contiguous(n_total, 1)
        members = []
        for j, (rho, bits, seed) in enumerate(configs):
            i = rhos.index(rho)
            m = NativeChainEngine(X, y, local_ids, n_total, "linear", rho=rho, obj0=obj0, tol=tols[j],
                                  max_iter=max_iters[j], stream=stream, precomputed=(A, b, yy), xcd=xcd,
                                  inverses=(Minv, len(rhos) * V, (i * V, i * V, i * V + V - 1)), quant=(bits, seed),
                                  censor=censors[j])
            m.set_path(list(range(n_total)), pl, 0)
            members.append(m)
        self = cls(members, stream=stream)
        self._shared = shared
        return self

    def blocks(self) -> List[int]:
        """Workgroups of every member (one wave per worker + the monitor)."""
        return [m.n_total + 1 for m in self.members]

    def run(self, lag: int = 4, timeout_s: float = 20.0, fetch_trace: bool = True) -> List[EngineRun]:
        """Reset every member and run all of them in one launch; one ``EngineRun`` per member. Each
        member then answers ``traces`` / ``objective_trace`` / ``time_trace`` / ``theta`` /
        ``theta_true`` / ``ctl_state`` as after its own ``run_persistent``; ``last_placed`` holds each
        member's placement verdict. ``ResidencyError``: the launcher refused before launching (the
        workgroups cannot all be resident); ``ValueError``: a member is not eligible;
        ``HandoffTimeout`` names the slot."""
        K = len(self.members)
        for m in self.members:
            m.reset()
        batch = (native.PersistArgs * K)()
        cens = any(m.censor is not None for m in self.members)  # one censored member: the censored kernel for all
        for j, m in enumerate(self.members):
            try:
                batch[j] = m.prepare_persistent_q(lag=lag, timeout_s=timeout_s, censored=cens)
            except ValueError as e:
                raise ValueError("sweep member %d: %s" % (j, e))
        self.last_kernel = "persistent-%s-sweep(K=%d)" % ("CQ" if cens else "Q", K)
        for m in self.members:
            m.last_kernel = self.last_kernel
        launch = self.lib.gadmm_chain_persistent_cq_sweep_launch if cens else self.lib.gadmm_chain_persistent_q_sweep_launch
        t0 = time.perf_counter()
        self._launch(launch, batch, K, "chain_persistent_q_sweep_launch")
        fetch, _ = self._collect(self.members, fetch_trace, t0)
        return [m.finish_persistent_q(self.last_wall_ms, f, "persistent Q sweep kernel: slot %d" % j)
                for j, (m, f) in enumerate(zip(self.members, fetch))]
