"""Up to eight independent logistic GGADMM solves (inner-GD local solves) in ONE launch of the persistent
logistic graph kernel's body, one solve per XCD (csrc/kernels/graph_persistent_logistic.hip:
graph_logistic_sweep_kernel).

Logistic GGADMM is used as a batch over topologies (``LogisticRegression_Topologies`` solves chain, ring,
grid, star and complete bipartite on the same shards), and its solves are the longest here: a worker wave
runs up to ``max_inner`` dependent GEMV pairs per phase. The single solve (one wave per worker plus the
monitor) is packed onto one of the MI355X's eight XCDs by an 8x wider grid whose blocks ``b % 8 != 0`` exit
at once; here slot ``j`` of a launch runs member ``j`` on the blocks ``b % 8 == j``. A member is a
``NativeGraphLogisticEngine`` (its own theta, duals, granule table, control block, trace, rings, step
counts, placement-check buffer, CSR arrays and tag salt); the members share one stream, so every reset
and table allocation of every member is ordered ahead of the one launch, and only the shards are shared
between slots, read-only. Slots may differ in graph, n, d, m (within one register class of the kernel:
max(d, m) <= 52 or 53..64), rho, step, ``max_inner`` and ``inner_tol``; every slot runs the poll code of the
degree class its own single launch would take. One slot holds at most the CUs of an XCD in workgroups (32
on an MI355X): a graph of more than 31 workers is refused (``ResidencyError``).

Two ways to build one:

* ``GraphLogisticSweepEngine.build(X, y, members, lam, step, ...)`` with ``members = [(graph, rho), ...]``
  or ``[(graph, rho, step, max_inner, inner_tol), ...]``: the same shards under every member (there is no
  Gram and there are no inverses to share);
* ``GraphLogisticSweepEngine(members)``: already-built engines (different data, graphs, N, d and m); they
  are moved onto the sweep's stream.

What a sweep engine is apart from its kernel and its members' preparation: sweep_base.py.
"""
from __future__ import annotations

import time
from typing import List, Sequence

import torch

from ..ops import native
from .chain_engine import EngineRun
from .graph_logistic_engine import NativeGraphLogisticEngine
from .sweep_base import SweepEngineBase, per_member


def graph_logistic_sweep_capacity() -> int:
    """Solves one logistic graph sweep launch takes (gadmm_graph_logistic_sweep_capacity)."""
    return int(native.require().gadmm_graph_logistic_sweep_capacity())


def parse_member(mem, step: float, max_inner: int, inner_tol: float) -> tuple:
    """A sweep member ``(graph, rho)`` or ``(graph, rho, step, max_inner, inner_tol)`` as the latter; the
    defaults are the call's."""
    from ..parallel.topology import BipartiteGraph
    mem = tuple(mem) if isinstance(mem, (tuple, list)) else (mem,)
    if len(mem) not in (2, 5) or not isinstance(mem[0], BipartiteGraph):
        raise ValueError("a logistic graph sweep member is (graph, rho) or (graph, rho, step, max_inner, inner_tol), "
                         "got %r" % (mem,))
    if len(mem) == 2:
        return mem[0], float(mem[1]), float(step), int(max_inner), float(inner_tol)
    if int(mem[3]) < 1 or int(mem[3]) != mem[3] or float(mem[4]) < 0.0:
        raise ValueError("a logistic graph sweep member needs an integer max_inner >= 1 and inner_tol >= 0, got %r"
                         % (mem,))
    return mem[0], float(mem[1]), float(mem[2]), int(mem[3]), float(mem[4])


class GraphLogisticSweepEngine(SweepEngineBase):
    _SPLIT = 52
    _CLASSES = "max(d, m) <= 52 and 53..64"
    _SOLVES = "logistic GGADMM solves with max(d, m) <= 64"
    _WHAT = "persistent graph logistic sweep kernel"
    _MODEL = "logistic"
    _ARGS = native.GraphLogiArgs

    capacity = staticmethod(graph_logistic_sweep_capacity)

    @staticmethod
    def _size(m) -> int:
        return max(m.d, m.m)

    def _member_defect(self, m):
        if not isinstance(m, NativeGraphLogisticEngine):
            return " is not a NativeGraphLogisticEngine"
        if max(m.d, m.m) > NativeGraphLogisticEngine.MAX_DM:
            return ": one-GPU %s only" % self._SOLVES
        return None

    def __init__(self, members: Sequence[NativeGraphLogisticEngine], stream=None):
        super().__init__(members, stream)
        native.check_graph_abi(self.lib)
        native.check_graph_logistic_abi(self.lib)

    @classmethod
    def build(cls, X: torch.Tensor, y: torch.Tensor, members: Sequence, lam: float, step: float, max_inner: int = 100,
              inner_tol: float = 1e-4, obj0: float = 0.0, tols=1e-4, max_iters=1000, xcd: int = 2,
              residual: bool = True) -> "GraphLogisticSweepEngine":
        """Members = the same shards ``X`` (n, m, d), ``y`` (n, m) under every ``(graph, rho)`` or ``(graph,
        rho, step, max_inner, inner_tol)`` of ``members`` (``step`` / ``max_inner`` / ``inner_tol``: of a
        member given as ``(graph, rho)``). ``tols`` / ``max_iters``: one value or one per member."""
        if not X.is_cuda:
            raise ValueError("%s runs on a HIP device" % cls.__name__)
        parsed = [parse_member(m, step, max_inner, inner_tol) for m in members]
        K = len(parsed)
        if K < 1 or K > cls.capacity():
            raise ValueError("%d members: one sweep launch takes 1..%d" % (K, cls.capacity()))
        n, m, d = (int(v) for v in X.shape)
        if max(d, m) > NativeGraphLogisticEngine.MAX_DM:
            raise ValueError("the persistent graph logistic kernel takes max(d, m) <= 64 (d = %d, m = %d)" % (d, m))
        for j, mem in enumerate(parsed):
            if mem[0].n != n:
                raise ValueError("member %d: the graph has %d workers, the data %d shards" % (j, mem[0].n, n))
        tols = per_member(tols, K, float, "tols / max_iters: one value, or one per member")
        max_iters = per_member(max_iters, K, int, "tols / max_iters: one value, or one per member")
        X = X.to(torch.float64).contiguous()  # every member reads these two tensors
        y = y.to(torch.float64).contiguous()
        stream = torch.cuda.Stream(X.device)
        stream.wait_stream(torch.cuda.current_stream(X.device))
        engines = [NativeGraphLogisticEngine(X, y, g, rho, obj0, tols[j], max_iters[j], lam, st, mi, it, xcd=xcd,
                                             residual=residual, stream=stream)
                   for j, (g, rho, st, mi, it) in enumerate(parsed)]
        return cls(engines, stream=stream)

    def blocks(self) -> List[int]:
        """Workgroups of every member (one wave per worker + the monitor)."""
        return [m.n + 1 for m in self.members]

    def reset(self):
        for m in self.members:
            m.reset()

    def run(self, fetch_trace: bool = True, timeout_s: float = 20.0) -> List[EngineRun]:
        """Reset every member and run all of them in one launch, one synchronize; one ``EngineRun`` per
        member. Each member then answers ``traces`` / ``theta`` / ``mu`` / ``rres`` / ``inner_iters`` /
        ``ctl_state`` as after its own ``run``; ``last_placed`` holds each member's placement verdict.
        ``ResidencyError``: the launcher refused before launching (the workgroups cannot all be resident, or
        one member's do not fit on an XCD); ``ValueError``: a member is not eligible; ``HandoffTimeout``
        names the slot, and nothing more is started on the GPU in that call."""
        K = len(self.members)
        self.reset()
        batch = (native.GraphLogiArgs * K)()
        for j, m in enumerate(self.members):
            try:
                batch[j] = m.prepare(timeout_s)
            except RuntimeError as e:
                raise ValueError("sweep member %d: %s" % (j, e))
        self.last_kernel = "persistent-graph-logistic-sweep(K=%d)" % K
        for m in self.members:
            m.last_kernel = self.last_kernel
        t0 = time.perf_counter()
        self._launch(self.lib.gadmm_graph_logistic_sweep_launch, batch, K, "graph_logistic_sweep_launch")
        fetch, _ = self._collect(self.members, fetch_trace, t0)
        return [m.finish(self.last_wall_ms, f, "%s: slot %d" % (self._WHAT, j))
                for j, (m, f) in enumerate(zip(self.members, fetch))]
