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
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Optional, Sequence

import torch

from ..ops import native
from ..ops.linalg import gram, spd_inverse
from ..parallel.topology import Placement
from .chain_engine import EngineRun, HandoffTimeout, NativeChainEngine, ResidencyError


def quant_sweep_capacity() -> int:
    """Solves one Q sweep launch takes (gadmm_chain_persistent_q_sweep_capacity)."""
    return int(native.require().gadmm_chain_persistent_q_sweep_capacity())


class QuantSweepEngine:
    def __init__(self, members: Sequence[NativeChainEngine], stream: Optional[torch.cuda.Stream] = None):
        members = list(members)
        if not members:
            raise ValueError("a sweep needs at least one member")
        cap = quant_sweep_capacity()
        if len(members) > cap:
            raise ValueError("%d members: one sweep launch takes at most %d" % (len(members), cap))
        if len({id(m) for m in members}) != len(members):
            raise ValueError("a member appears twice (every slot needs its own state)")
        dev = members[0].device
        if any(m.device != dev for m in members):
            raise ValueError("the members of a sweep live on one device")
        for j, m in enumerate(members):
            if m.quant is None:
                raise ValueError("member %d is not a Q-GADMM engine (quant=(bits, seed))" % j)
            if m.model != "linear" or m.nranks != 1 or m.n_local != m.n_total or m.d > 64:
                raise ValueError("member %d: one-GPU linear Q-GADMM solves with d <= 64 only" % j)
            if m.plan is None:
                raise ValueError("member %d has no chain installed (set_path)" % j)
        if len({m.d <= 52 for m in members}) != 1:
            raise ValueError("members of different register classes (d <= 52 and 53..64) cannot share a launch")
        self.lib = native.require()
        self.device = dev
        self.members = members
        self.stream = stream if stream is not None else members[0].stream
        for m in members:  # one stream: every member's resets and zero-fills precede the launch
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

    # ---------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, X: torch.Tensor, y: torch.Tensor, local_ids: Sequence[int], n_total: int, configs: Sequence,
              obj0: float = 0.0, tols=1e-4, max_iters=1000, precomputed=None,
              placement: Optional[Placement] = None, xcd: int = 2, censors: Optional[Sequence] = None
              ) -> "QuantSweepEngine":
        """Members = the same shards under every ``(rho, bits, seed)`` of ``configs``. ``tols`` /
        ``max_iters``: one value or one per member. ``precomputed``: an ``(A, b, yy)`` Gram to share (else
        computed here, once). ``censors``: one ``(tau0, xi)`` or None per config (CQ-GADMM members)."""
        if not X.is_cuda:
            raise ValueError("QuantSweepEngine runs on a HIP device")
        configs = [(float(r), int(b), int(s)) for r, b, s in configs]
        K = len(configs)
        censors = [None] * K if censors is None else list(censors)
        if len(censors) != K:
            raise ValueError("censors: one (tau0, xi) or None per config")
        if K < 1 or K > quant_sweep_capacity():
            raise ValueError("%d configs: one sweep launch takes 1..%d" % (K, quant_sweep_capacity()))
        tols = [float(tols)] * K if not isinstance(tols, (list, tuple)) else [float(t) for t in tols]
        max_iters = [int(max_iters)] * K if not isinstance(max_iters, (list, tuple)) else [int(v) for v in max_iters]
        if len(tols) != K or len(max_iters) != K:
            raise ValueError("tols / max_iters: one value, or one per config")
        X = X.to(torch.float64).contiguous()
        y = y.to(torch.float64).contiguous()
        n_total = int(n_total)
        if len(local_ids) != n_total:
            raise ValueError("a sweep member holds every worker of its chain (one GPU)")
        if n_total < 2:
            raise ValueError("a chain needs at least two workers")
        if int(X.shape[2]) > 64:
            raise ValueError("the persistent Q kernel takes d <= 64 (d = %d)" % int(X.shape[2]))
        dev = X.device
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        # degree-1 and degree-2 shifts per DISTINCT rho, as NativeChainEngine._build_inverses picks them
        rhos = list(dict.fromkeys(r for r, _, _ in configs))
        per = [[r] if n_total == 2 else [r, 2.0 * r] for r in rhos]
        V = len(per[0])
        with torch.cuda.stream(stream):
            A, b, yy = precomputed if precomputed is not None else gram(X, y)
            shifts = torch.tensor([s for p in per for s in p], dtype=torch.float64, device=dev).unsqueeze(0).expand(
                A.shape[0], -1).contiguous()
            Minv = spd_inverse(A, shifts)  # ONE launch for all distinct rho x V shifts (checks positive definiteness)
        pl = placement if placement is not None else Placement.contiguous(n_total, 1)
        members = []
        for j, (rho, bits, seed) in enumerate(configs):
            i = rhos.index(rho)
            dtv = (i * V, i * V, i * V + V - 1)
            m = NativeChainEngine(X, y, local_ids, n_total, "linear", rho=rho, obj0=obj0, tol=tols[j],
                                  max_iter=max_iters[j], stream=stream, precomputed=(A, b, yy), xcd=xcd,
                                  inverses=(Minv, len(rhos) * V, dtv), quant=(bits, seed), censor=censors[j])
            m.set_path(list(range(n_total)), pl, 0)
            members.append(m)
        self = cls(members, stream=stream)
        self._shared = (A, b, yy, shifts, Minv, torch.zeros((1,), dtype=torch.int32, device=dev))
        return self

    def refresh(self, X: torch.Tensor, y: torch.Tensor):
        """Recompute the shared Gram and the shared table of inverses from the raw shards, in place, on
        the sweep's stream: one Gram and one inverse launch for the whole sweep (``build`` engines)."""
        if self._shared is None:
            raise RuntimeError("refresh: members built elsewhere refresh themselves")
        A, b, yy, shifts, Minv, status = self._shared
        with torch.cuda.stream(self.stream):
            gram(X, y, out=(A, b, yy))
            spd_inverse(A, shifts, out=Minv, check_status=False, status=status)
        for m in self.members:
            m._minv_version += 1

    def set_targets(self, obj0: float, tols) -> None:
        tols = [float(tols)] * len(self.members) if not isinstance(tols, (list, tuple)) else list(tols)
        for m, t in zip(self.members, tols):
            m.set_targets(obj0, float(t))

    # ---------------------------------------------------------------------------------------------
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
        rc = int(launch(batch, K, self._stage_host.data_ptr(), self._stage_dev.data_ptr(), self.stream.cuda_stream))
        if rc == -2:
            raise ResidencyError(self.lib.gadmm_last_error().decode())
        if rc == -1:
            raise ValueError(self.lib.gadmm_last_error().decode())
        native.check(rc, "chain_persistent_q_sweep_launch")
        fetch = [m._queue_readback(fetch_trace) for m in self.members]
        self.stream.synchronize()
        self.last_wall_ms = (time.perf_counter() - t0) * 1e3
        # every control block first (host memory only), then the verdicts: after a timeout nothing more
        # is started on the GPU in this call
        codes = [m._ctl_host.tolist() for m in self.members]
        self.last_placed = [c[6] for c in codes]
        bad = [j for j, c in enumerate(codes) if c[1] == 4]
        if bad:
            for m, c in zip(self.members, codes):
                m.last_placed = c[6]
            raise HandoffTimeout("persistent Q sweep kernel: slot %d timed out (hand-off never completed)" % bad[0])
        return [m.finish_persistent_q(self.last_wall_ms, f, "persistent Q sweep kernel: slot %d" % j)
                for j, (m, f) in enumerate(zip(self.members, fetch))]

    def stop_ticks(self, runs: Sequence[EngineRun]) -> List[int]:
        """Device clock (s_memrealtime, 100 MHz) of each member's stop decision in the last run, read
        from the pinned read-back block (``run(fetch_trace=True)``); 0 where no decision was stamped."""
        out = []
        for m, r in zip(self.members, runs):
            nt = m.trace.numel()
            if not getattr(m, "_tr_valid", False) or r.iters < 1 or r.iters > nt:
                out.append(0)
                continue
            out.append(int(m._rb_host_np[8 + nt + r.iters - 1:8 + nt + r.iters].view("int64")[0]))
        return out

    def close(self):
        for m in self.members:
            m.close()
