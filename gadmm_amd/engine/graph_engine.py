"""Python front-end of the persistent GGADMM kernel (csrc/kernels/graph_persistent.hip).

Group ADMM on any connected bipartite graph (``parallel.topology.BipartiteGraph``) as one launch on
one GPU: every worker is a resident wave that holds its cached inverse ``(A_n + rho deg_n I)^{-1}``
and its Gram in VGPRs; theta travels as tagged granules, one table row per worker; the stop rule runs
on the device (the monitor workgroup). The specification is ``algorithms/ggadmm.py``.

With ``quant=(bits, seed)`` the launch is Q-GGADMM (csrc/kernels/graph_quant.hip): the exchange is the
quantized difference to each worker's public model, packed as in Q-GADMM (``algorithms/quantize.py``);
``theta`` then holds the public models and ``theta_true`` the true iterates.

Every device buffer is allocated and filled on the engine's own stream, the stream of the launch, so
no fill can land while the kernel's workgroups already post their granules.
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional

import numpy as np
import torch

from ..ops import native
from ..ops.linalg import gram, spd_inverse
from ..utils.env import getenv
from .chain_engine import EngineRun, HandoffTimeout, ResidencyError


class NativeGraphEngine:
    LAG = 4
    MAX_D = 64

    model = "linear"         # what a sweep (engine/sweep_base.py) asks of a member: a one-GPU linear solve
    nranks = 1
    obj_mode_name = "exact"  # the objective the monitor sums is the true one

    def __init__(self, X: torch.Tensor, y: torch.Tensor, graph, rho: float, obj0: float, tol: float, max_iter: int,
                 precomputed=None, xcd: int = 2, residual: bool = True, quant=None, stream=None, inverses=None):
        """``X`` (n, m, d), ``y`` (n, m): every worker's shard, in worker order (``graph.n`` of them).
        ``precomputed``: ``(A, b, yy)`` of those shards (the Gram is then not recomputed). ``xcd``: as
        ``NativeChainEngine`` (0 default grid, 1 packed onto one XCD, 2 also L2-resident plain stores
        once the kernel has verified the placement; speed only). ``residual``: the tails also emit the
        K4 primal residual rows (``rres``, ``primal_residual``). ``quant``: ``(bits, seed)``, ``bits`` in
        {4, 8, 16} -- Q-GGADMM: ``theta`` receives the public models, ``theta_true`` the true iterates,
        ``q_msg`` shows every worker's last message, the K4 rows are taken on the public models.
        ``stream`` / ``inverses``: for a sweep's builder (engine/graph_sweep.py) -- the stream the engine
        lives on (default: its own) and a contiguous ``(n, d, d)`` table of this member's inverses, each
        worker's at ``rho`` times its own degree, computed by the caller (default: computed here)."""
        if not X.is_cuda:
            raise ValueError("NativeGraphEngine runs on a HIP device; use graph_admm(backend='torch') on CPU")
        self.lib = native.require()
        native.check_graph_abi(self.lib)
        self.quant = None
        if quant is not None:
            from ..algorithms.quantize import check_bits, granules_per_row
            native.check_graph_q_abi(self.lib)
            self.quant = (check_bits(quant[0]), int(quant[1]))
        self.graph = graph
        self.device = X.device
        self.n, self.d = int(X.shape[0]), int(X.shape[2])
        if self.n != graph.n:
            raise ValueError("the graph has %d workers, the data %d shards" % (graph.n, self.n))
        self.rho, self.obj0, self.tol, self.max_iter = float(rho), float(obj0), float(tol), int(max_iter)
        self.xcd = int(xcd)
        self.n_local = self.n_total = self.n
        self.ring = self.LAG + 4
        self.stream = stream if stream is not None else torch.cuda.Stream(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        dev, f64, n, d, mi = self.device, torch.float64, self.n, self.d, self.max_iter
        ptr, idx = graph.csr()
        with torch.cuda.stream(self.stream):
            if precomputed is not None:
                self.A, self.b, self.yy = precomputed
            else:
                self.A, self.b, self.yy = gram(X.to(f64), y.to(f64))
            # every worker's inverse at its OWN degree: one variant per worker
            if inverses is not None:
                if tuple(inverses.shape) != (n, d, d) or not inverses.is_contiguous():
                    raise ValueError("inverses: a contiguous (n, d, d) table")
                self._shifts, self.Minv = None, inverses
            else:
                self._shifts = torch.tensor([[self.rho * g] for g in graph.degree], dtype=f64, device=dev)
                self.Minv = spd_inverse(self.A, self._shifts)
            self.theta = torch.zeros((n, d), dtype=f64, device=dev)
            self.mu = torch.zeros((n, d), dtype=f64, device=dev)
            # read-back block, as NativeChainEngine: [ctl (8 x i32) | t0stamp | pad x 3 | trace | tstamp]
            self._rb = torch.zeros((8 + 2 * mi,), dtype=f64, device=dev)
            self.ctl = self._rb[0:4].view(torch.int32)
            self.t0stamp = self._rb[4:5].view(torch.int64)
            self.trace = self._rb[8:8 + mi]
            self.trace.fill_(float("nan"))
            self.tstamp = self._rb[8 + mi:8 + 2 * mi].view(torch.int64)
            self._rres = torch.zeros((mi * n,), dtype=f64, device=dev) if residual else None
            self._nb_ptr = torch.from_numpy(ptr).to(dev)
            self._nb_idx = torch.from_numpy(idx).to(dev)
            self._wid = torch.tensor(graph.order, dtype=torch.int32, device=dev)
            self._is_head = torch.tensor([1 if graph.is_head[w] else 0 for w in graph.order], dtype=torch.int32,
                                         device=dev)
            # granule tables: zeroed once, tags are salted per launch (never re-zeroed)
            self._thg = torch.zeros((n * d * 4,), dtype=torch.int32, device=dev)
            self._objg = torch.zeros((self.ring * n * 4,), dtype=torch.int32, device=dev)
            self._decg = torch.zeros((self.ring,), dtype=torch.int64, device=dev)
            self._dec_push = torch.tensor([self._decg.data_ptr()], dtype=torch.int64, device=dev)
            self._xchk = torch.zeros((256 * 4,), dtype=torch.int32, device=dev)
            if self.quant is not None:
                # the message table, zeroed once like thg (tags are salted per launch), and the true iterates
                self.q_granules = granules_per_row(d, self.quant[0])
                self._qg = torch.zeros((n * self.q_granules * 4,), dtype=torch.int32, device=dev)
                self.theta_true = torch.zeros((n, d), dtype=f64, device=dev)
        self.stream.synchronize()
        self._epoch = 0
        self._rb_host = None
        self._tr_valid = False
        self.last_placed = 0
        self.last_kernel = None
        self.reset()

    # ---------------------------------------------------------------------------------------------
    def _args(self, timeout_s: float = 20.0) -> native.GraphArgs:
        a = native.GraphArgs()
        a.d, a.n, a.n_local, a.start_iter = self.d, self.n, self.n, 1
        a.max_iter, a.lag, a.ring, a.nranks = self.max_iter, self.LAG, self.ring, 1
        a.epoch, a.max_degree = self._epoch, self.graph.max_degree
        a.rho, a.obj0, a.tol = self.rho, self.obj0, self.tol
        a.timeout_ticks = int(timeout_s * 1e8)
        a.nb_ptr, a.nb_idx = self._nb_ptr.data_ptr(), self._nb_idx.data_ptr()
        a.wid, a.is_head = self._wid.data_ptr(), self._is_head.data_ptr()
        a.Minv, a.A, a.b, a.yy = self.Minv.data_ptr(), self.A.data_ptr(), self.b.data_ptr(), self.yy.data_ptr()
        a.theta, a.mu = self.theta.data_ptr(), self.mu.data_ptr()
        a.thg, a.objg, a.decg = self._thg.data_ptr(), self._objg.data_ptr(), self._decg.data_ptr()
        a.dec_push = self._dec_push.data_ptr()
        a.trace, a.tstamp, a.ctl = self.trace.data_ptr(), self.tstamp.data_ptr(), self.ctl.data_ptr()
        a.rres = native.ptr(self._rres)
        a.xchk, a.xcd = self._xchk.data_ptr(), self.xcd
        return a

    def _q_args(self, timeout_s: float = 20.0) -> native.GraphQArgs:
        q = native.GraphQArgs()
        q.g = self._args(timeout_s)
        q.qg, q.q_bits, q.q_seed = self._qg.data_ptr(), self.quant[0], self.quant[1] & ((1 << 64) - 1)
        q.q_true = self.theta_true.data_ptr()
        return q

    def kernel_class(self) -> int:
        """Neighbours the launch polls back to back (2, 4, 8, 16 or 32; with ``quant`` at most 16, two
        granules each); 0: the shape is not eligible."""
        if self.quant is not None:
            return int(self.lib.gadmm_graph_persistent_q_class(ctypes.byref(self._q_args())))
        return int(self.lib.gadmm_graph_persistent_class(ctypes.byref(self._args())))

    def resident_capacity(self) -> int:
        key = ("cap", getenv("GADMM_CU_BUDGET"))
        memo = self.__dict__.setdefault("_cap_memo", {})
        if key not in memo:
            if self.quant is not None:
                memo[key] = int(self.lib.gadmm_graph_persistent_q_capacity(ctypes.byref(self._q_args())))
            else:
                memo[key] = int(self.lib.gadmm_graph_persistent_capacity(ctypes.byref(self._args())))
        return memo[key]

    def _lds_bytes(self) -> int:
        fn = self.lib.gadmm_graph_persistent_q_lds if self.quant is not None else self.lib.gadmm_graph_persistent_lds
        return int(fn(self.n, self.graph.max_degree))

    def refusal(self) -> Optional[str]:
        """Why the persistent kernel does not take this engine, decided without a launch; None: it does."""
        if self.d > self.MAX_D:
            return "d > 64"
        if self._lds_bytes() > 65536:
            return "max_degree %d: the neighbour staging does not fit in LDS" % self.graph.max_degree
        if self.max_iter + self.LAG + 1 >= (1 << 20):
            return "max_iter past the 2^20 iteration tags"
        cap = self.resident_capacity()
        if self.n + 1 > cap:
            return "ResidencyError: %d workgroups but only %d can be resident" % (self.n + 1, cap)
        return None

    def eligible(self) -> bool:
        return self.refusal() is None

    def set_targets(self, obj0: float, tol: float):
        self.obj0, self.tol = float(obj0), float(tol)

    def reset(self):
        """theta = mu = 0, residual rows = 0, trace = NaN, the control block and the clock start: one
        launch on the engine's stream."""
        self._tr_valid = False
        rr = self._rres
        native.check(self.lib.gadmm_chain_reset_state_stamp(
            self.ctl.data_ptr(), 1, 0, self.theta.data_ptr(), self.theta.numel(), self.mu.data_ptr(), self.mu.numel(),
            self.trace.data_ptr(), self.trace.numel(), native.ptr(rr), rr.numel() if rr is not None else 0,
            self.t0stamp.data_ptr(), self.stream.cuda_stream), "reset_state")

    def run(self, fetch_trace: bool = True, timeout_s: float = 20.0) -> EngineRun:
        """One launch: the whole solve from the state ``reset()`` left. Raises ``ResidencyError`` when the
        launcher refuses (nothing was launched) and ``HandoffTimeout`` when a hand-off passed its
        deadline (done == 4)."""
        a = self.prepare(timeout_s)
        if self.quant is not None:
            self.last_kernel = "persistent-graph-Q(deg<=%d,b=%d)" % (self._class_bound(), self.quant[0])
            launch = self.lib.gadmm_graph_persistent_q_launch
        else:
            self.last_kernel = "persistent-graph(deg<=%d)" % self._class_bound()
            launch = self.lib.gadmm_graph_persistent_launch
        t0 = time.perf_counter()
        rc = int(launch(ctypes.byref(a), self.stream.cuda_stream))
        if rc == -2:
            raise ResidencyError(self.lib.gadmm_last_error().decode())
        native.check(rc, "graph_persistent_launch")
        fetch = self._queue_readback(fetch_trace)
        self.stream.synchronize()
        return self.finish((time.perf_counter() - t0) * 1e3, fetch, "persistent graph kernel")

    def prepare(self, timeout_s: float = 20.0):
        """The arguments of the next launch (``GraphArgs``, or ``GraphQArgs`` with ``quant``) under a fresh
        tag salt: the granule tables of the last solve never match, so they are never re-zeroed.
        ``RuntimeError``: the kernel does not take the shape (a residency refusal is the launcher's)."""
        why = self.refusal()
        if why is not None and not why.startswith("ResidencyError"):
            raise RuntimeError("persistent graph kernel not eligible: %s" % why)
        self._epoch = self._epoch % 4095 + 1
        return self._q_args(timeout_s) if self.quant is not None else self._args(timeout_s)

    def _queue_readback(self, fetch_trace: bool) -> bool:
        """Queue the read-back of the control block (with ``fetch_trace`` and a short trace: of the whole
        read-back block) behind the launch on the engine's stream, through readback.hip's path; True if
        the traces come along."""
        nt = self.trace.numel()
        fetch = bool(fetch_trace) and nt <= 16384
        if self._rb_host is None:
            self._rb_host = torch.empty(self._rb.shape, dtype=torch.float64, pin_memory=True)
            self._rb_host_np = self._rb_host.numpy()
            self._ctl_host = self._rb_host[0:4].view(torch.int32)
        nb = self._rb.numel() * 8 if fetch else 32
        native.check(self.lib.gadmm_readback_d2h(self._rb_host.data_ptr(), self._rb.data_ptr(), nb,
                                                 self.stream.cuda_stream), "readback")
        return fetch

    def finish(self, wall_ms: float, fetch: bool, what: str) -> EngineRun:
        """The ``EngineRun`` of a launch whose read-back (``_queue_readback``) has completed. A hand-off
        timeout (done == 4) raises."""
        self._tr_valid = fetch
        c = self._ctl_host.tolist()
        done, conv, nxt = c[1], c[2], c[0]
        self.last_placed = c[6]
        if done == 4:
            raise HandoffTimeout("%s timed out (hand-off never completed)" % what)
        return EngineRun(conv, done, nxt - 1, 1, wall_ms, 0, 0, 0, 0)

    def adopt_stream(self, stream: torch.cuda.Stream):
        """Move the engine onto ``stream`` (ordered behind everything queued on its old one): its resets
        and launches then share that stream with the other members of a sweep."""
        stream.wait_stream(self.stream)
        self.stream = stream

    def _class_bound(self) -> int:
        k, g = self.kernel_class(), self.graph.max_degree
        top = 16 if self.quant is not None else 32  # the largest poll group; past it, groups of that size
        return k if g <= k else top * ((g + top - 1) // top)

    # ---------------------------------------------------------------------------------------------
    def traces(self, upto: int):
        """(objective trace, measured clock) of iterations 1..upto."""
        if upto <= 0:
            return np.zeros((0,), dtype=np.float64), np.zeros((0,), dtype=np.float64)
        nt = self.trace.numel()
        if self._tr_valid and upto <= nt:  # the pinned copy of the last run
            h = self._rb_host_np
            t = h[8 + nt:8 + nt + upto].view(np.int64)
            tt = (t - int(h[4:5].view(np.int64)[0])) * 1e-8
            tt[t <= 0] = 0.0
            return h[8:8 + upto].copy(), tt
        with torch.cuda.stream(self.stream):
            buf = torch.cat([self.trace[:upto], self.tstamp[:upto].view(torch.float64),
                             self.t0stamp.view(torch.float64)]).cpu().numpy()
        t = buf[upto:2 * upto].view(np.int64)
        t0 = int(buf[2 * upto:].view(np.int64)[0])
        return buf[:upto].copy(), np.where(t > 0, (t - t0) * 1e-8, 0.0)

    @property
    def rres(self) -> Optional[torch.Tensor]:
        """(max_iter, n) K4 rows by worker id: a tail's entry is the squared distance over its edges,
        a head's stays 0. None unless built with ``residual=True``."""
        return None if self._rres is None else self._rres.view(self.max_iter, self.n)

    @property
    def q_msg(self) -> Optional[torch.Tensor]:
        """(n, G) uint64 words of every worker's last message as it sits in the message table (word 0 the
        bits of R, then the code words), tags stripped; None without ``quant``. Shown as int64 (torch has no
        arithmetic on uint64): ``.cpu().numpy().view(numpy.uint64)``."""
        if self.quant is None:
            return None
        self.stream.synchronize()
        g = self._qg.view(self.n, self.q_granules, 4).to(torch.int64) & 0xffffffff
        return (g[:, :, 3] << 32) | g[:, :, 1]

    def primal_residual(self, upto: int) -> Optional[np.ndarray]:
        if self._rres is None or upto <= 0:
            return None
        self.stream.synchronize()
        return self._rres[: upto * self.n].view(upto, self.n).cpu().numpy().sum(axis=1)

    def ctl_state(self) -> dict:
        self.stream.synchronize()
        c = self.ctl.cpu().tolist()
        return {"iter": c[0], "done": c[1], "conv_iter": c[2], "pending": c[3], "ticket": c[4], "monitored": c[5],
                "placed": c[6], "inner_fail": c[7]}

    def close(self):
        pass
