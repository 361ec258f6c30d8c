"""Up to eight independent GGADMM (or Q-GGADMM) solves in ONE launch of the persistent graph kernel's
body, one solve per XCD (csrc/kernels/graph_persistent.hip: graph_persistent_sweep_kernel;
csrc/kernels/graph_quant.hip: graph_persistent_q_sweep_kernel).

GGADMM is used as a batch: the same shards over several graphs and rho (``LinearRegression_Topologies``
solves chain, ring, grid, star and complete bipartite at every rho), and Q-GGADMM's result depends on a
random draw, so a useful run of it is graphs x bit widths x seeds. The single solve (one wave per worker
plus the monitor) is packed onto one of the MI355X's eight XCDs by an 8x wider grid whose blocks
``b % 8 != 0`` exit at once; here slot ``j`` of a launch runs member ``j`` on the blocks ``b % 8 == j``.
A member is a ``NativeGraphEngine`` (its own theta, duals, granule or message table, control block,
trace, rings, placement-check buffer, CSR arrays and tag salt); the members share one stream, so every
reset, zero-fill and table allocation of every member is ordered ahead of the one launch, and only
read-only inputs (the Gram, and one allocation of inverses of which each member reads its own slice) are
shared between slots. A launch is all unquantized or all quantized. Slots may differ in graph, n, d
(within one register class of the kernel: d <= 52 or 53..64), rho, bits and seed; every slot runs the
poll code of the degree class its own single launch would take. One slot holds at most the CUs of an
XCD in workgroups (32 on an MI355X): a graph of more than 31 workers is refused (``ResidencyError``).

Two ways to build one:

* ``GraphSweepEngine.build(X, y, members, ...)`` with ``members = [(graph, rho), ...]`` or
  ``[(graph, rho, bits, seed), ...]``: the same shards under every member -- one Gram and ONE
  ``spd_inverse`` launch for all the members' ``rho * degree`` shifts; ``refresh(X, y)`` recomputes both
  in place;
* ``GraphSweepEngine(members)``: already-built engines (different data, graphs, N and d); they are moved
  onto the sweep's stream.

What a sweep engine is apart from its kernel and its members' preparation: sweep_base.py.
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Sequence

import torch

from ..ops import native
from ..ops.linalg import gram, spd_inverse
from .chain_engine import EngineRun
from .graph_engine import NativeGraphEngine
from .sweep_base import SweepEngineBase, per_member


def graph_sweep_capacity() -> int:
    """Solves one graph sweep launch takes (gadmm_graph_persistent_sweep_capacity; the Q launch takes as many)."""
    return int(native.require().gadmm_graph_persistent_sweep_capacity())


def parse_member(mem) -> tuple:
    """A sweep member ``(graph, rho)`` or ``(graph, rho, bits, seed)`` as ``(graph, rho, quant or None)``."""
    from ..parallel.topology import BipartiteGraph
    mem = tuple(mem)
    if len(mem) not in (2, 4) or not isinstance(mem[0], BipartiteGraph):
        raise ValueError("a graph sweep member is (graph, rho) or (graph, rho, bits, seed), got %r" % (mem,))
    if len(mem) == 2:
        return mem[0], float(mem[1]), None
    from ..algorithms.quantize import check_bits
    return mem[0], float(mem[1]), (check_bits(mem[2]), int(mem[3]))


class GraphSweepEngine(SweepEngineBase):
    _SPLIT = 52
    _CLASSES = "d <= 52 and 53..64"
    _SOLVES = "GGADMM solves with d <= 64"
    _WHAT = "persistent graph sweep kernel"

    capacity = staticmethod(graph_sweep_capacity)

    def _member_defect(self, m):
        if not isinstance(m, NativeGraphEngine):
            return " is not a NativeGraphEngine"
        if m.d > NativeGraphEngine.MAX_D:
            return ": one-GPU linear %s only" % self._SOLVES
        return None

    def __init__(self, members: Sequence[NativeGraphEngine], stream=None):
        super().__init__(members, stream)
        if len({m.quant is not None for m in self.members}) != 1:
            raise ValueError("a graph sweep launch is all unquantized or all quantized (GGADMM or Q-GGADMM members)")
        self.quantized = self.members[0].quant is not None
        self._args_t = native.GraphQArgs if self.quantized else native.GraphArgs
        native.check_graph_abi(self.lib)
        if self.quantized:
            native.check_graph_q_abi(self.lib)
        # the launcher's staging pair holds the slots' GraphArgs / GraphQArgs
        nbytes = self.capacity() * ctypes.sizeof(self._args_t)
        if nbytes > self._stage_host.numel():
            self._stage_host = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
            self._stage_dev = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)

    @classmethod
    def build(cls, X: torch.Tensor, y: torch.Tensor, members: Sequence, obj0: float = 0.0, tols=1e-4,
              max_iters=1000, precomputed=None, xcd: int = 2, residual: bool = True) -> "GraphSweepEngine":
        """Members = the same shards ``X`` (n, m, d), ``y`` (n, m) under every ``(graph, rho)`` or
        ``(graph, rho, bits, seed)`` of ``members`` (all of one kind). ``tols`` / ``max_iters``: one value
        or one per member. ``precomputed``: an ``(A, b, yy)`` Gram to share (else computed here, once).
        Member ``j`` reads the contiguous ``(n, d, d)`` slice ``j`` of one table of inverses, worker ``w``'s
        at the shift ``rho_j * deg_j(w)``: ONE ``spd_inverse`` launch over the Gram repeated K times."""
        if not X.is_cuda:
            raise ValueError("%s runs on a HIP device" % cls.__name__)
        parsed = [parse_member(m) for m in members]
        K = len(parsed)
        if K < 1 or K > cls.capacity():
            raise ValueError("%d members: one sweep launch takes 1..%d" % (K, cls.capacity()))
        if len({q is not None for _, _, q in parsed}) != 1:
            raise ValueError("a graph sweep launch is all unquantized or all quantized (GGADMM or Q-GGADMM members)")
        n, d = int(X.shape[0]), int(X.shape[2])
        if d > NativeGraphEngine.MAX_D:
            raise ValueError("the persistent graph kernel takes d <= 64 (d = %d)" % d)
        for j, (g, _, _) in enumerate(parsed):
            if g.n != n:
                raise ValueError("member %d: the graph has %d workers, the data %d shards" % (j, g.n, n))
        tols = per_member(tols, K, float, "tols / max_iters: one value, or one per member")
        max_iters = per_member(max_iters, K, int, "tols / max_iters: one value, or one per member")
        X = X.to(torch.float64).contiguous()
        y = y.to(torch.float64).contiguous()
        dev = X.device
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            A, b, yy = precomputed if precomputed is not None else gram(X, y)
            shifts = torch.tensor([[rho * deg] for g, rho, _ in parsed for deg in g.degree], dtype=torch.float64,
                                  device=dev)
            A_rep = A.repeat(K, 1, 1)  # (K n, d, d): member j's copy at rows j n .. j n + n - 1
            Minv = spd_inverse(A_rep, shifts)  # ONE launch for every member (checks positive definiteness)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        engines = [NativeGraphEngine(X, y, g, rho, obj0, tols[j], max_iters[j], precomputed=(A, b, yy), xcd=xcd,
                                     residual=residual, quant=q, stream=stream, inverses=Minv[j * n:(j + 1) * n, 0])
                   for j, (g, rho, q) in enumerate(parsed)]
        self = cls(engines, stream=stream)
        self._shared = (A, b, yy, shifts, Minv, status, A_rep)
        return self

    def refresh(self, X: torch.Tensor, y: torch.Tensor):
        """Recompute the shared Gram and every member's inverses from the raw shards, in place, on the
        sweep's stream: one Gram and one inverse launch for the whole sweep (engines of ``build``)."""
        if self._shared is None:
            raise RuntimeError("refresh: members built elsewhere refresh themselves")
        A, b, yy, shifts, Minv, status, A_rep = self._shared
        K = len(self.members)
        with torch.cuda.stream(self.stream):
            gram(X.to(torch.float64).contiguous(), y.to(torch.float64).contiguous(), out=(A, b, yy))
            A_rep.view(K, *A.shape).copy_(A.unsqueeze(0).expand(K, *A.shape))
            spd_inverse(A_rep, shifts, out=Minv, check_status=False, status=status)

    def blocks(self) -> List[int]:
        """Workgroups of every member (one wave per worker + the monitor)."""
        return [m.n + 1 for m in self.members]

    def reset(self):
        for m in self.members:
            m.reset()

    def run(self, fetch_trace: bool = True, timeout_s: float = 20.0) -> List[EngineRun]:
        """Reset every member and run all of them in one launch, one synchronize; one ``EngineRun`` per
        member. Each member then answers ``traces`` / ``theta`` / ``mu`` / ``rres`` / ``ctl_state`` (and
        ``theta_true`` / ``q_msg``) as after its own ``run``; ``last_placed`` holds each member's placement
        verdict. ``ResidencyError``: the launcher refused before launching (the workgroups cannot all be
        resident, or one member's do not fit on an XCD); ``ValueError``: a member is not eligible;
        ``HandoffTimeout`` names the slot, and nothing more is started on the GPU in that call."""
        K = len(self.members)
        self.reset()
        batch = (self._args_t * K)()
        for j, m in enumerate(self.members):
            try:
                batch[j] = m.prepare(timeout_s)
            except RuntimeError as e:
                raise ValueError("sweep member %d: %s" % (j, e))
        self.last_kernel = "persistent-graph-%ssweep(K=%d)" % ("Q-" if self.quantized else "", K)
        for m in self.members:
            m.last_kernel = self.last_kernel
        launch = (self.lib.gadmm_graph_persistent_q_sweep_launch if self.quantized
                  else self.lib.gadmm_graph_persistent_sweep_launch)
        t0 = time.perf_counter()
        self._launch(launch, batch, K, "graph_persistent_sweep_launch")
        fetch, _ = self._collect(self.members, fetch_trace, t0)
        return [m.finish(self.last_wall_ms, f, "%s: slot %d" % (self._WHAT, j))
                for j, (m, f) in enumerate(zip(self.members, fetch))]
