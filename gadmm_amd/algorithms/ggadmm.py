"""GGADMM: group ADMM on any connected bipartite graph (Ben Issaid et al., arXiv:2009.06459).

The workers form two groups, heads and tails, and every edge joins a head to a tail
(``parallel.topology.BipartiteGraph``). GADMM is the special case of a chain. The duals are kept per
worker, ``mu_n = sum over n's edges of (+-) lambda_edge``, the form the chain engines already use.

Specification. Iteration ``it`` (1-based), ``N(n)`` the neighbours of n in ASCENDING worker id, every
line one rounded float64 operation per coordinate, in this order:

    heads, all at once:  r = b_n - mu_n;  for k in N(n): r = r + rho theta_k       (tails' theta^{it-1})
                         theta_n = (A_n + rho deg_n I)^{-1} r
    tails, all at once:  the same with the heads' theta^{it}
    every worker:        for k in N(n): mu_n = mu_n + rho (theta_n - theta_k)
    objective            sum_n f_n(theta_n) in worker order; stop rule: |objective - obj0| < tol
    primal residual      sum over edges ||theta_h - theta_t||^2   (each edge once; its tail owns it)

Accounting: every worker broadcasts one model per iteration, ``comm_units[k] = (k + 1) N``; each
broadcast is delivered to every neighbour, ``extra['deliveries'] = iters * 2 |E|``.

Q-GGADMM, ``quantize=(bits, seed)``: the quantized exchange of Q-GADMM (Elgabli et al.,
arXiv:1910.10453; the quantizer's specification is algorithms/quantize.py) on the graph. Every worker
keeps a public model ``hat_n``, zero at the start, of which each neighbour holds an identical copy, and
broadcasts the quantized difference of its new iterate to it; every neighbour applies that message to
its copy exactly once. Each line one rounded float64 operation per coordinate:

    heads, all at once:  r = b_n - mu_n;  for k in N(n) ascending: r = r + rho hat_k   (tails' hat^{it-1})
                         theta_n = (A_n + rho deg_n I)^{-1} r                           (the TRUE iterate)
                         (R, q, hat_n) = quantize_rows(theta_n, hat_n, bits, u01(seed, it, N, n, d))
    tails, all at once:  the same with the heads' hat^{it}
    every worker:        for k in N(n) ascending: mu_n = mu_n + rho (hat_n - hat_k)     (public models)
    objective            of the TRUE theta; primal residual over edges on the public models

This is ``chain_admm(quantize=)`` with the chain's two neighbours replaced by ``N(n)`` (bit for bit that
run's torch path on a chain graph). No censoring: every worker transmits every iteration,
``extra['transmissions'] = iters * N`` of ``bits * d + 64`` payload bits each (``_quant_accounting`` of
algorithms/gadmm.py), ``deliveries`` as above.

Two executions: ``backend='torch'``, a batched loop in the style of the chain's torch path (bit for bit
that path on a chain graph), and the native persistent kernel on one HIP device
(engine/graph_engine.py, csrc/kernels/graph_persistent.hip; quantized: csrc/kernels/graph_quant.hip). The linear model with closed-form solves,
one process, every worker local; anything else raises ``NotImplementedError``.
"""
from __future__ import annotations

import time
from typing import Optional, Sequence

import numpy as np
import torch

from ..parallel.comm import LocalComm
from ..parallel.topology import BipartiteGraph
from ..utils.timing import roctx_range
from .base import RunResult, Stopper, global_objective_and_residual


def _check_case(model, graph, comm) -> None:
    if not isinstance(graph, BipartiteGraph):
        raise TypeError("graph_admm: graph must be a BipartiteGraph (parallel.topology)")
    if getattr(model, "kind", None) != "linear":
        raise NotImplementedError("graph_admm: the linear model with closed-form local solves only "
                                  "(got model kind %r)" % getattr(model, "kind", None))
    if comm is not None and getattr(comm, "nranks", 1) != 1:
        raise NotImplementedError("graph_admm: one process, every worker local (got %d ranks)" % comm.nranks)
    if int(model.n_local) != graph.n:
        raise NotImplementedError("graph_admm: every worker local -- the model holds %d shards, the graph has %d "
                                  "workers" % (int(model.n_local), graph.n))


def graph_admm(model, graph: BipartiteGraph, rho: float, obj0: float, tol: float, max_iter: int,
               backend: str = "auto", name: str = "GGADMM", engine_opts: Optional[dict] = None,
               record_theta: bool = False, comm=None, quantize: Optional[Sequence] = None,
               censor: Optional[Sequence] = None) -> RunResult:
    """One GGADMM solve of ``model`` (shard n belongs to worker n) over ``graph``.

    ``backend``: ``'torch'`` the batched loop (any device); ``'auto'`` the native kernel on a HIP
    device when the engine accepts the shape, else the torch path with the reason in
    ``extra['graph_fallback']``; ``'native'`` raises ``RuntimeError`` on a refusal. A residency refusal
    or a hand-off timeout of the native launch re-runs on the torch path (reason recorded likewise).
    ``engine_opts``: ``cache`` (keep the engine on the model, default True), ``xcd`` (0 / 1 / 2, default 2),
    ``residual`` (K4 rows from the kernel, default True), ``timeout_s``.
    The torch path returns ``extra['state'] = (theta, mu, next_iter)``; the native path does not.
    ``comm``: only to refuse several ranks.
    ``quantize``: ``(bits, seed)``, ``bits`` in {4, 8, 16} -- Q-GGADMM (module docstring). ``theta`` of the
    result and ``extra['state'][0]`` of the torch path are then the PUBLIC models and
    ``extra['theta_true']`` the true iterates (the torch path also keeps every worker's last message,
    ``extra['q_msg'] = (R (n,), codes (n, d))``); the accounting is that of a chain Q run. None: every path
    as without it. ``censor``: not offered on graphs (``NotImplementedError``)."""
    _check_case(model, graph, comm)
    if censor is not None:
        raise NotImplementedError("censoring on graphs is not offered")
    quant = None
    if quantize is not None:
        from .quantize import check_bits
        if len(quantize) != 2:
            raise ValueError("quantize: (bits, seed)")
        quant = (check_bits(quantize[0]), int(quantize[1]))
    if backend not in ("auto", "torch", "native"):
        raise ValueError("unknown backend %r" % backend)
    opts = dict(engine_opts or {})
    why = None
    if backend == "torch":
        why = "torch backend"
    elif model.device.type != "cuda":
        why = "cpu tensors"
    elif model.d > 64:
        why = "d > 64"
    else:
        from ..ops import native
        if not native.available():
            why = "native library unavailable"
    if why is None:
        res, why = _graph_admm_native(model, graph, rho, obj0, tol, max_iter, name, opts, quant)
        if res is not None:
            if record_theta:
                res.theta = res.extra["engine_obj"].theta.cpu().numpy()
            return res
    if backend == "native":
        raise RuntimeError("graph_admm: the native backend does not cover this case (%s)" % why)
    res = _graph_admm_torch(model, graph, rho, obj0, tol, max_iter, name, record_theta, quant)
    if backend != "torch":
        res.extra["graph_fallback"] = why
    return res


generalized_group_admm = graph_admm


def quantized_graph_admm(model, graph: BipartiteGraph, rho: float, obj0: float, tol: float, max_iter: int, bits: int,
                         seed: int = 1234, **kw) -> RunResult:
    """Q-GGADMM: ``graph_admm(..., quantize=(bits, seed))`` under its own name."""
    kw.setdefault("name", "Q-GGADMM")
    return graph_admm(model, graph, rho, obj0, tol, max_iter, quantize=(bits, seed), **kw)


def _padded_neighbours(graph: BipartiteGraph, workers, dev):
    """Per neighbour slot j < max degree of ``workers``: (index tensor, mask tensor) of each worker's
    j-th neighbour in ascending id (index 0 / mask 0 where it has fewer)."""
    width = max(graph.degree[w] for w in workers)
    out = []
    for j in range(width):
        ids = [graph.neighbours(w)[j] if j < graph.degree[w] else -1 for w in workers]
        idx = torch.tensor([max(i, 0) for i in ids], dtype=torch.long, device=dev)
        mask = torch.tensor([1.0 if i >= 0 else 0.0 for i in ids], dtype=torch.float64, device=dev)
        out.append((idx, mask.unsqueeze(-1)))
    return out


def _graph_admm_torch(model, graph, rho, obj0, tol, max_iter, name, record_theta, quant=None) -> RunResult:
    n, d, dev = graph.n, model.d, model.device
    theta = torch.zeros((n, d), dtype=torch.float64, device=dev)  # quantized: the table of PUBLIC models
    mu = torch.zeros((n, d), dtype=torch.float64, device=dev)
    th_true = None
    min_margin = float("inf")
    if quant is not None:
        from . import quantize as Q
        th_true = torch.zeros((n, d), dtype=torch.float64, device=dev)
        last_R, last_q = np.zeros(n), np.zeros((n, d), dtype=np.int64)  # every worker's last message
    groups = []
    for workers in (graph.heads, graph.tails):
        li = torch.tensor(workers, dtype=torch.long, device=dev)
        deg = torch.tensor([float(graph.degree[w]) for w in workers], dtype=torch.float64, device=dev)
        groups.append((li, deg, _padded_neighbours(graph, workers, dev)))
    eh = torch.tensor([e[0] for e in graph.edges], dtype=torch.long, device=dev)
    et = torch.tensor([e[1] for e in graph.edges], dtype=torch.long, device=dev)
    ids = list(range(n))
    comm = LocalComm()
    stop = Stopper(obj0, tol, max_iter)
    primal = []
    iters, converged = max_iter, False
    for it in range(1, max_iter + 1):
        for li, deg, nbs in groups:  # heads (the tails' theta of the last iteration), then tails
            rhs = model.b.index_select(0, li) - mu.index_select(0, li)
            for idx, mask in nbs:
                rhs = rhs + rho * (theta.index_select(0, idx) * mask)
            new = model.prox_solve(li, rhs, deg * rho)
            if quant is not None:  # the true iterate stays beside the table; the table moves by the message
                th_true[li] = new
                ids_np = li.cpu().numpy()
                last_R[ids_np], last_q[ids_np], hat, mg = Q.quantize_rows(
                    new.cpu().numpy(), theta.index_select(0, li).cpu().numpy(), quant[0],
                    Q.u01(quant[1], it, n, ids_np, d))
                min_margin = min(min_margin, mg)
                new = torch.from_numpy(hat).to(dev)
            theta[li] = new
        for li, deg, nbs in groups:  # every worker's dual, neighbours in ascending id
            thw = theta.index_select(0, li)
            m = mu.index_select(0, li)
            for idx, mask in nbs:
                m = m + rho * (thw - theta.index_select(0, idx)) * mask
            mu[li] = m
        f = model.objective(theta if quant is None else th_true)
        dl = theta.index_select(0, eh) - theta.index_select(0, et)
        res_loc = torch.zeros(n, dtype=torch.float64, device=dev)
        res_loc.index_add_(0, et, (dl * dl).sum(-1))  # each edge once, filed under its tail
        f_all, r_all = global_objective_and_residual(comm, f, res_loc, ids, n)
        primal.append(r_all)
        if stop.record(f_all):
            iters, converged = it, True
            break
    obj, loss, times = stop.arrays()
    n_it = len(obj)
    done_it = iters if converged else n_it
    res = RunResult(algorithm=name, obj=obj, loss=loss, iters=done_it, converged=converged,
                    wall_s=float(times[-1]) if n_it else 0.0, time_trace=times,
                    comm_units=np.arange(1, n_it + 1, dtype=np.float64) * n, com_cost=np.zeros(n_it),
                    bytes_sent=0, bytes_total=0, primal_res=np.asarray(primal),
                    extra={"backend": "torch", "engine": "torch", "kernel": "torch", "rank": 0, "nranks": 1,
                           "solver": "closed", "monitor_bytes": 0, "transport": "local",
                           "graph": graph.describe(), "deliveries": done_it * 2 * len(graph.edges)})
    res.extra["state"] = (theta, mu, done_it + 1)
    if quant is not None:
        from .gadmm import _quant_accounting
        _quant_accounting(res, quant[0], quant[1], n, d)
        res.extra.update(transmissions=done_it * n, min_flip_margin=min_margin, theta_true=th_true,
                         q_msg=(last_R, last_q))
    if record_theta:
        res.theta = theta.cpu().numpy()
    return res


def _graph_admm_native(model, graph, rho, obj0, tol, max_iter, name, opts, quant=None):
    """``(RunResult, None)`` from the persistent kernel, or ``(None, reason)`` when the engine refuses
    the shape, the launcher the residency, or a hand-off timed out."""
    from ..engine.chain_engine import HandoffTimeout, ResidencyError
    from ..engine.graph_engine import NativeGraphEngine

    xcd = int(opts.get("xcd", 2))
    residual = bool(opts.get("residual", True))
    key = ("graph", graph.key(), float(rho), int(max_iter), xcd, residual) + (() if quant is None else quant)
    cache = getattr(model, "_chain_engines", None)
    eng = cache.get(key) if cache is not None else None
    fresh = eng is None
    if eng is None:
        eng = NativeGraphEngine(model.X, model.y, graph, rho, obj0, tol, max_iter,
                                precomputed=(model.A, model.b, model.yy), xcd=xcd, residual=residual, quant=quant)
        if opts.get("cache", True):
            if cache is None:
                cache = {}
                model._chain_engines = cache
            cache[key] = eng
    else:
        eng.set_targets(obj0, tol)
    why = eng.refusal()
    if why is not None:
        return None, why
    eng.reset()
    if fresh:
        torch.cuda.synchronize(model.device)  # a new engine's set-up is complete before the solve
    t0 = time.perf_counter()
    try:
        with roctx_range("%s native-graph%s N=%d E=%d" % (name, "" if quant is None else "-Q", graph.n,
                                                          len(graph.edges))):
            r = eng.run(fetch_trace=True, timeout_s=float(opts.get("timeout_s", 20.0)))
    except ResidencyError as e:
        return None, "ResidencyError: %s" % e
    except HandoffTimeout as e:
        return None, "HandoffTimeout: %s" % e
    wall = time.perf_counter() - t0
    iters, done = int(r.iters), int(r.done)
    tr, tt = eng.traces(iters)
    res = RunResult(algorithm=name, obj=tr, loss=np.abs(tr - obj0), iters=iters, converged=(done == 1), wall_s=wall,
                    time_trace=tt, comm_units=np.arange(1, iters + 1, dtype=np.float64) * graph.n,
                    com_cost=np.zeros(iters), bytes_sent=0, bytes_total=0, primal_res=eng.primal_residual(iters),
                    extra={"backend": "native", "engine": "persistent", "kernel": eng.last_kernel, "rank": 0,
                           "nranks": 1, "solver": "closed", "monitor_bytes": 0, "wire_bytes": 0,
                           "transport": "local", "placed": int(eng.last_placed), "engine_obj": eng,
                           "graph": graph.describe(), "deliveries": iters * 2 * len(graph.edges)})
    if quant is not None:
        from .gadmm import _quant_accounting
        from .quantize import granules_per_row
        G = granules_per_row(model.d, quant[0])
        _quant_accounting(res, quant[0], quant[1], graph.n, model.d)
        res.extra.update(transmissions=iters * graph.n, q_granules=G, q_wire_bytes=iters * graph.n * G * 16,
                         theta_true=eng.theta_true)
    return res, None
