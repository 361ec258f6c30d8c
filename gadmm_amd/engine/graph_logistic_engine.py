"""Python front-end of the persistent logistic GGADMM kernel (csrc/kernels/graph_persistent_logistic.hip).

Logistic regression with the reference's inexact local solver (inner GD) on any connected bipartite graph
as one launch on one GPU, ``max(d, m) <= 64``: every worker is a resident wave that keeps its shard twice
in VGPRs (for the margins and for the gradient); theta travels as tagged granules, one table row per
worker; the stop rule runs on the device. The specification is ``algorithms/ggadmm.py``
(``graph_admm_logistic``).

The buffers, the read-back, ``finish``, ``traces`` and the residual rows are ``NativeGraphEngine``'s; what
differs is the launch (``GraphLogiArgs``: no Gram form, no inverses) and ``inner_iters``.
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional

import torch

from ..ops import native
from ..utils.env import getenv
from .chain_engine import EngineRun, ResidencyError
from .graph_engine import NativeGraphEngine


class NativeGraphLogisticEngine(NativeGraphEngine):
    MAX_DM = 64
    TOP = 8  # the largest poll group; past it a worker walks its neighbours in groups of that size

    model = "logistic"
    quant = None

    def __init__(self, X: torch.Tensor, y: torch.Tensor, graph, rho: float, obj0: float, tol: float, max_iter: int,
                 lam: float, step: float, max_inner: int = 100, inner_tol: float = 1e-4, xcd: int = 2,
                 residual: bool = True, stream=None):
        """``X`` (n, m, d), ``y`` (n, m) in {-1, +1}: every worker's shard, in worker order. ``lam``: the
        ridge weight of every worker's loss; ``step`` / ``max_inner`` / ``inner_tol``: the inner GD of
        ``LogisticRegression.inexact_gd``. ``xcd`` / ``residual`` / ``stream``: as ``NativeGraphEngine``."""
        if not X.is_cuda:
            raise ValueError("NativeGraphLogisticEngine runs on a HIP device; use "
                             "graph_admm_logistic(backend='torch') on CPU")
        self.lib = native.require()
        native.check_graph_abi(self.lib)
        native.check_graph_logistic_abi(self.lib)
        self._setup(graph, X, rho, obj0, tol, max_iter, xcd, stream)
        self.m = int(X.shape[1])
        self.lam, self.step = float(lam), float(step)
        self.max_inner, self.inner_tol = int(max_inner), float(inner_tol)
        if self.max_inner < 1:
            raise ValueError("max_inner: at least one inner step")
        with torch.cuda.stream(self.stream):
            self.X = X.to(torch.float64).contiguous()
            self.y = y.to(torch.float64).contiguous()
            self._alloc(residual)
            self.inner_iters = torch.zeros((self.n,), dtype=torch.int32, device=self.device)
        self._start()

    # ---------------------------------------------------------------------------------------------
    def _l_args(self, timeout_s: float = 20.0) -> native.GraphLogiArgs:
        ga = native.GraphLogiArgs()
        ga.g = self._args(timeout_s)
        ga.l.X, ga.l.Y, ga.l.m, ga.l.max_inner = self.X.data_ptr(), self.y.data_ptr(), self.m, self.max_inner
        ga.l.lam, ga.l.step, ga.l.inner_tol = self.lam, self.step, self.inner_tol
        ga.l.inner_iters = self.inner_iters.data_ptr()
        return ga

    def kernel_class(self) -> int:
        """Neighbours the launch polls back to back (2, 4 or 8); 0: the shape is not eligible."""
        return int(self.lib.gadmm_graph_logistic_class(ctypes.byref(self._l_args())))

    def resident_capacity(self) -> int:
        key = ("cap", getenv("GADMM_CU_BUDGET"))
        memo = self.__dict__.setdefault("_cap_memo", {})
        if key not in memo:
            memo[key] = int(self.lib.gadmm_graph_logistic_capacity(ctypes.byref(self._l_args())))
        return memo[key]

    def _lds_bytes(self) -> int:
        return int(self.lib.gadmm_graph_logistic_lds(self.n, self.graph.max_degree))

    def refusal(self) -> Optional[str]:
        """Why the persistent kernel does not take this engine, decided without a launch; None: it does."""
        if max(self.d, self.m) > self.MAX_DM:
            return "max(d, m) > 64"
        return NativeGraphEngine.refusal(self)

    def _class_bound(self) -> int:
        k, g = self.kernel_class(), self.graph.max_degree
        return k if g <= k else self.TOP * ((g + self.TOP - 1) // self.TOP)

    def prepare(self, timeout_s: float = 20.0) -> native.GraphLogiArgs:
        """The ``GraphLogiArgs`` of the next launch under a fresh tag salt (as ``NativeGraphEngine.prepare``)."""
        why = self.refusal()
        if why is not None and not why.startswith("ResidencyError"):
            raise RuntimeError("persistent graph logistic kernel not eligible: %s" % why)
        self._epoch = self._epoch % 4095 + 1
        return self._l_args(timeout_s)

    def run(self, fetch_trace: bool = True, timeout_s: float = 20.0) -> EngineRun:
        """One launch: the whole solve from the state ``reset()`` left. Raises ``ResidencyError`` when the
        launcher refuses (nothing was launched) and ``HandoffTimeout`` when a hand-off passed its
        deadline (done == 4)."""
        a = self.prepare(timeout_s)
        self.last_kernel = "persistent-graph-logistic(deg<=%d)" % self._class_bound()
        t0 = time.perf_counter()
        rc = int(self.lib.gadmm_graph_logistic_launch(ctypes.byref(a), self.stream.cuda_stream))
        if rc == -2:
            raise ResidencyError(self.lib.gadmm_last_error().decode())
        native.check(rc, "graph_logistic_launch")
        fetch = self._queue_readback(fetch_trace)
        self.stream.synchronize()
        return self.finish((time.perf_counter() - t0) * 1e3, fetch, "persistent graph logistic kernel")
