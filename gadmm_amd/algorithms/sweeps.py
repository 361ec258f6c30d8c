"""Sweeps: many solves of one chain-ADMM problem, on one HIP device up to eight per kernel launch, one per
XCD (engine/sweep_base.py and the three engines on it); anywhere else the loop of single solves.

  ``chain_admm_sweep``            static-chain GADMM at several rho (engine/chain_sweep.py)
  ``quantized_group_admm_sweep``  Q-GADMM / CQ-GADMM under several (rho, bits, seed[, tau0, xi]) (engine/quant_sweep.py)
  ``dynamic_group_admm_sweep``    D-GADMM at several coherences (engine/dyn_sweep.py)
  ``graph_admm_sweep``            GGADMM / Q-GGADMM over several (graph, rho[, bits, seed]) (engine/graph_sweep.py)

They are one driver (``_run_sweep``: the gates that send a call to the loop, the groups of one
launch, the fall-back when a launch is refused) around what each sweep knows: its gates and their
reasons, how a group's engine is built and run, and what a member's ``RunResult`` carries on top of the
common part (``_member_result``). ``algorithms.gadmm``, where they used to live, re-exports them.
"""
from __future__ import annotations

import time
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from ..parallel.comm import Comm
from ..parallel.topology import PathSchedule, Placement
from ..utils import timing as _timing
from ..utils.env import getenv
from ..utils.timing import roctx_range
from .base import RunResult
from .gadmm import _quant_accounting, _static_schedule, chain_admm, dynamic_group_admm


def sweep_groups(n: int, width: int) -> List[List[int]]:
    """Indices 0..n-1 in consecutive groups of at most ``width`` (one group per sweep launch)."""
    if width < 1:
        raise ValueError("sweep width must be >= 1")
    return [list(range(i, min(i + width, n))) for i in range(0, n, width)]


def run_in_groups(items: Sequence, width: int, run_group) -> list:
    """``run_group(group_items, group_indices)`` per ``sweep_groups`` group; the results in input order."""
    out = [None] * len(items)
    for g in sweep_groups(len(items), width):
        res = run_group([items[i] for i in g], g)
        if len(res) != len(g):
            raise RuntimeError("a sweep group of %d returned %d results" % (len(g), len(res)))
        for i, r in zip(g, res):
            out[i] = r
    return out


def _run_sweep(members: Sequence, sequential_one: Callable, gates: Sequence, capacity: Callable[[], int],
               run_group: Callable, label: str) -> List[RunResult]:
    """One ``RunResult`` per member, in the order given. ``gates``: the sweep's ``(condition, reason)``
    pairs in its order; the first that holds -- or no native library, or a launcher that refuses a group
    (``ResidencyError``: the device cannot hold its workgroups; ``ValueError``: a shape the kernel does not
    take) -- makes the call the loop of ``sequential_one(member)``, every result recording
    ``extra['sweep_fallback'] = reason``. Else ``run_group(group_members, group_indices)`` per group of
    ``capacity()`` members, under the roctx range ``label``."""
    def sequential(reason: str) -> List[RunResult]:
        out = []
        for mem in members:
            r = sequential_one(mem)
            r.extra["sweep_fallback"] = reason
            out.append(r)
        return out

    if not members:
        return []
    for cond, reason in gates:
        if cond:
            return sequential(reason)
    from ..ops import native
    if not native.available():
        return sequential("native library unavailable")
    from ..engine.chain_engine import ResidencyError
    try:
        with roctx_range(label):
            return run_in_groups(members, capacity(), run_group)
    except ResidencyError as e:
        return sequential("ResidencyError: %s" % e)
    except ValueError as e:  # a shape the sweep kernel does not take (d past its classes, no blocked plan, ...)
        return sequential("not eligible: %s" % e)


def _group_engine(model, key: tuple, opts: dict, build: Callable, targets: tuple, refresh: bool = False):
    """The sweep engine of a group: the one cached under ``key`` in ``model._chain_engines`` with new
    ``set_targets(*targets)``, or ``build()``, its set-up complete, cached unless ``opts['cache']`` is
    off. ``refresh``: the Gram and the inverses are recomputed from the raw shards first."""
    cache = getattr(model, "_chain_engines", None)
    sw = cache.get(key) if cache is not None else None
    if sw is not None:
        sw.set_targets(*targets)
        if refresh:
            sw.refresh(model.X, model.y)
        return sw
    if refresh:
        from ..ops.linalg import gram
        gram(model.X, model.y, out=(model.A, model.b, model.yy))  # the new engine inverts the fresh Gram
    sw = build()
    torch.cuda.synchronize(model.device)  # a new engine's set-up is complete before the solve
    if opts.get("cache", True):
        if cache is None:
            cache = {}
            model._chain_engines = cache
        cache[key] = sw
    return sw


def _member_result(name: str, sw, slot: int, width: int, iters: int, done: int, obj0: float, n_total: int,
                   wall_s: float, tail_ticks: int, placed: int, engine: str = "persistent", com_cost=None,
                   primal: bool = True) -> RunResult:
    """The ``RunResult`` of member ``slot`` of the sweep engine ``sw``. ``wall_s``: the wall clock of the
    launches it took part in; its OWN time is that less ``tail_ticks``, the device time (100 MHz) between
    its stop decision and the end of its last launch."""
    m = sw.members[slot]
    iters = int(iters)
    tr, tt = m.traces(iters)
    return RunResult(algorithm=name, obj=tr, loss=np.abs(tr - obj0), iters=iters, converged=(int(done) == 1),
                     wall_s=wall_s - tail_ticks * 1e-8, time_trace=tt,
                     comm_units=np.arange(1, iters + 1, dtype=np.float64) * n_total,
                     com_cost=np.arange(1, iters + 1) * 0.0 if com_cost is None else com_cost,
                     bytes_sent=0, bytes_total=0, primal_res=m.primal_residual(iters) if primal else None,
                     extra={"backend": "native", "engine": engine, "rank": 0, "nranks": 1, "solver": "closed",
                            "monitor_bytes": 0, "wire_bytes": 0, "transport": "local", "obj_mode": m.obj_mode_name,
                            "engine_obj": m,
                            "sweep": {"width": width, "slot": slot, "kernel": sw.last_kernel, "placed": int(placed),
                                      "wall_ms_launch": sw.last_wall_ms},
                            "sweep_kernel": sw.last_kernel, "sweep_slot": slot})


def _one_launch_results(name: str, sw, t_begin: float, obj0: float, n_total: int, primal: bool = True,
                        **run_kw) -> List[RunResult]:
    """Run ``sw`` (one launch, ``sw.run(**run_kw)``) and return its members' results; ``t_begin``: when the
    group's set-up began."""
    runs = sw.run(**run_kw)
    wall = time.perf_counter() - t_begin
    ticks = sw.stop_ticks(runs)
    last = max(ticks)
    return [_member_result(name, sw, j, len(runs), r.iters, r.done, obj0, n_total, wall,
                           last - ticks[j] if ticks[j] > 0 else 0, sw.last_placed[j], primal=primal)
            for j, r in enumerate(runs)]


def chain_admm_sweep(model, local_ids: Sequence[int], n_total: int, rhos: Sequence[float], obj0: float, tol: float,
                     max_iter: int, *, tols: Optional[Sequence[float]] = None, placement: Optional[Placement] = None,
                     backend: str = "auto", name: str = "GADMM", engine_opts: Optional[dict] = None,
                     comm: Optional[Comm] = None) -> List[RunResult]:
    """The static-chain closed-form GADMM solve at every rho of ``rhos``: one ``RunResult`` per rho, in
    the order given, equal to ``[chain_admm(model, ..., rho, ...) for rho in rhos]``. On one HIP device
    the solves run side by side, up to eight per kernel launch, one per XCD
    (engine/chain_sweep.py; more values run in groups), each to its own stop: ``tols`` gives one
    tolerance per rho (default ``tol`` for all). Each result then carries ``extra['sweep'] = {width,
    slot, kernel, placed, wall_ms_launch}`` and its ``wall_s`` is that solve's OWN time: the wall
    clock of its launch (set-up, launch, read-back) less the device time between its stop decision and
    the last member's, so the slowest member's equals the launch's; ``time_trace`` is each curve's own
    device clock. ``extra['state']`` is not produced (a caller that checkpoints runs ``chain_admm``).
    Anywhere else -- CPU tensors, ``backend='torch'``, several ranks, a shape the sweep kernel does not
    take, or a device that cannot hold the group's workgroups -- it IS that loop, and every result
    records ``extra['sweep_fallback'] = reason``. ``engine_opts``: ``refresh`` (recompute Gram +
    inverses from the raw shards first), ``residual``, ``cache``, as in ``chain_admm``."""
    rhos = [float(r) for r in rhos]
    opts = dict(engine_opts or {})
    tols = [float(tol)] * len(rhos) if tols is None else [float(t) for t in tols]
    if len(tols) != len(rhos):
        raise ValueError("tols: one per rho")
    refresh = bool(opts.get("refresh", False))
    residual = bool(opts.get("residual", True))

    def sequential_one(mem):
        return chain_admm(model, local_ids, n_total, mem[0], obj0, mem[1], max_iter, comm=comm, placement=placement,
                          backend=backend, name=name, engine_opts=engine_opts)

    def run_group(group, idx):
        from ..engine.chain_sweep import ChainSweepEngine
        t_begin = time.perf_counter()
        g_rhos, g_tols = [g[0] for g in group], [g[1] for g in group]
        key = ("sweep", n_total, tuple(map(int, local_ids)), tuple(g_rhos), int(max_iter), residual)
        sw = _group_engine(model, key, opts, lambda: ChainSweepEngine.rho_sweep(
            model.X, model.y, local_ids, n_total, g_rhos, obj0=obj0, tols=g_tols, max_iters=max_iter,
            precomputed=(model.A, model.b, model.yy), placement=placement, residual=residual), (obj0, g_tols), refresh)
        return _one_launch_results(name, sw, t_begin, obj0, n_total)

    def capacity():
        from ..engine.chain_sweep import sweep_capacity
        return sweep_capacity()

    gates = [(model.device.type != "cuda", "cpu tensors"), (backend == "torch", "torch backend"),
             (comm is not None and comm.nranks > 1, "several ranks"),
             (model.kind != "linear" or sorted(int(w) for w in local_ids) != list(range(n_total)),
              "not a one-GPU linear closed-form chain"),
             (getenv("GADMM_CHECK_EXCHANGE", "0") == "1", "exchange checker")]
    return _run_sweep(list(zip(rhos, tols)), sequential_one, gates, capacity, run_group,
                      "%s sweep native N=%d K=%d" % (name, n_total, len(rhos)))


def _sweep_member(cfg):
    """A sweep member ``(rho, bits, seed)`` or ``(rho, bits, seed, tau0, xi)`` as ``((rho, bits, seed),
    censor or None)``."""
    from .quantize import check_censor
    if len(cfg) == 3:
        return (float(cfg[0]), int(cfg[1]), int(cfg[2])), None
    if len(cfg) == 5:
        return (float(cfg[0]), int(cfg[1]), int(cfg[2])), check_censor(cfg[3:])
    raise ValueError("a Q sweep member is (rho, bits, seed) or (rho, bits, seed, tau0, xi), got %r" % (tuple(cfg),))


def quantized_group_admm_sweep(model, configs: Sequence, obj0: float, tol: float, max_iter: int, *,
                               tols: Optional[Sequence[float]] = None, placement: Optional[Placement] = None,
                               backend: str = "auto", name: str = "Q-GADMM", engine_opts: Optional[dict] = None,
                               comm: Optional[Comm] = None, n_total: Optional[int] = None,
                               local_ids: Optional[Sequence[int]] = None) -> List[RunResult]:
    """Q-GADMM on a static chain under every ``(rho, bits, seed)`` of ``configs``: one ``RunResult`` per
    config, in the order given, equal to ``[chain_admm(model, ..., rho, ..., quantize=(bits, seed)) for
    ...]``. On one HIP device the solves run side by side, up to eight per kernel launch, one per XCD
    (engine/quant_sweep.py; more configs run in groups), each to its own stop: ``tols`` gives one
    tolerance per config (default ``tol`` for all). Each result then carries the single native Q
    solve's fields plus ``extra['sweep'] = {width, slot, kernel, placed, wall_ms_launch}``, and its
    ``wall_s`` is that solve's OWN time (as ``chain_admm_sweep``: the wall clock of its launch less the
    device time between its stop decision and the last member's). ``extra['state']`` is not produced.
    Anywhere else -- CPU tensors, ``backend='torch'``, several ranks, the exchange checker, no native
    library, a non-linear model, not every worker local, d > 64, or a device that cannot hold the
    group's workgroups -- it IS that loop, and every result records ``extra['sweep_fallback'] =
    reason``. A hand-off timeout propagates. ``engine_opts``: ``cache``, ``xcd``, as in ``chain_admm``.
    A member may also be ``(rho, bits, seed, tau0, xi)``: CQ-GADMM, equal to its own ``chain_admm(...,
    quantize=(bits, seed), censor=(tau0, xi))``. A group with at least one censored member runs on the
    censored sweep kernel, where an uncensored member gets an all-zero threshold table and so stays
    Q-GADMM bit for bit; a group without one runs on the Q sweep kernel as before."""
    parsed = [_sweep_member(c) for c in configs]
    opts = dict(engine_opts or {})
    n_total = model.n_local if n_total is None else int(n_total)
    local_ids = list(range(model.n_local)) if local_ids is None else [int(w) for w in local_ids]
    tols = [float(tol)] * len(parsed) if tols is None else [float(t) for t in tols]
    if len(tols) != len(parsed):
        raise ValueError("tols: one per config")
    xcd = int(opts.get("xcd", 2))

    def sequential_one(mem):
        (rho, bits, seed), cen, t = mem
        return chain_admm(model, local_ids, n_total, rho, obj0, t, max_iter, comm=comm, placement=placement,
                          backend=backend, name=name, engine_opts=engine_opts, quantize=(bits, seed), censor=cen)

    def run_group(group, idx):
        from ..engine import quant_sweep  # (the engine by its name in that module, at call time)
        from . import quantize as Q
        t_begin = time.perf_counter()
        g_cfgs, g_cens, g_tols = [g[0] for g in group], [g[1] for g in group], [g[2] for g in group]
        key = ("qsweep", n_total, tuple(local_ids), tuple(g_cfgs), int(max_iter), xcd, tuple(g_cens))
        sw = _group_engine(model, key, opts, lambda: quant_sweep.QuantSweepEngine.build(
            model.X, model.y, local_ids, n_total, g_cfgs, obj0=obj0, tols=g_tols, max_iters=max_iter,
            precomputed=(model.A, model.b, model.yy), placement=placement, xcd=xcd, censors=g_cens), (obj0, g_tols))
        out = _one_launch_results(name, sw, t_begin, obj0, n_total, primal=False)
        for res, m, (rho, bits, seed), cen in zip(out, sw.members, g_cfgs, g_cens):
            G = Q.granules_per_row(model.d, bits)
            res.extra.update(kernel=sw.last_kernel, placed=res.extra["sweep"]["placed"], q_granules=G,
                             q_wire_bytes=res.iters * n_total * G * 16)
            _quant_accounting(res, bits, seed, n_total, model.d,
                              sent=m.sent_trace(res.iters) if cen is not None else None, censor=cen)
            if cen is not None:
                res.extra["q_wire_bytes"] = res.extra["transmissions"] * G * 16 + res.extra["censored"] * 16
        return out

    def capacity():
        from ..engine import quant_sweep
        return quant_sweep.quant_sweep_capacity()

    gates = [(model.device.type != "cuda", "cpu tensors"), (backend == "torch", "torch backend"),
             (comm is not None and comm.nranks > 1, "several ranks"),
             (getenv("GADMM_CHECK_EXCHANGE", "0") == "1", "exchange checker"),
             (model.kind != "linear", "not the linear closed-form model"),
             (sorted(local_ids) != list(range(n_total)), "not every worker local"), (model.d > 64, "d > 64")]
    return _run_sweep([(cfg, cen, t) for (cfg, cen), t in zip(parsed, tols)], sequential_one, gates, capacity,
                      run_group, "%s sweep native-Q N=%d K=%d" % (name, n_total, len(parsed)))


def graph_admm_sweep(model, members: Sequence, obj0: float, tol: float, max_iter: int, *,
                     tols: Optional[Sequence[float]] = None, backend: str = "auto", name: str = "GGADMM",
                     engine_opts: Optional[dict] = None, comm: Optional[Comm] = None) -> List[RunResult]:
    """GGADMM / Q-GGADMM of ``model`` under every member of ``members`` -- ``(graph, rho)`` or ``(graph, rho,
    bits, seed)`` -- one ``RunResult`` per member, in the order given, equal to ``[graph_admm(model, graph,
    rho, ...[, quantize=(bits, seed)]) ...]`` in iterations, objective trace, ``comm_units``, primal residual
    and ``converged``, for a quantized member also in ``extra['theta_true']`` and the bit accounting. On one
    HIP device the solves run side by side, up to eight per kernel launch, one per XCD
    (engine/graph_sweep.py; more members run in groups), each to its own stop: ``tols`` gives one tolerance
    per member (default ``tol`` for all). A launch is all unquantized or all quantized, so a mixed list is
    split by kind (the results keep the input order). Each result then carries the single native solve's
    fields plus ``extra['sweep'] = {width, slot, kernel, placed, wall_ms_launch}`` and ``extra['kernel']``
    (the sweep's), and its ``wall_s`` is that solve's OWN time (as ``chain_admm_sweep``: the wall clock of
    its launch less the device time between its stop decision and the last member's). ``extra['state']``
    is not produced. Anywhere else -- CPU tensors, ``backend='torch'``, several ranks, a non-linear model,
    d > 64, a member graph whose ``n`` is not the model's, no native library, or a launcher that refuses
    the group (``ResidencyError``: a graph of more than 31 workers does not fit one XCD's slot; a shape it
    does not take) -- it IS that loop, and every result records ``extra['sweep_fallback'] = reason``. A
    hand-off timeout propagates. ``engine_opts``: ``cache``, ``xcd``, ``residual``, ``timeout_s`` as in ``graph_admm``."""
    from ..engine.graph_sweep import parse_member  # (no device code is touched by the import)
    parsed = [parse_member(m) for m in members]
    opts = dict(engine_opts or {})
    tols = [float(tol)] * len(parsed) if tols is None else [float(t) for t in tols]
    if len(tols) != len(parsed):
        raise ValueError("tols: one per member")
    xcd = int(opts.get("xcd", 2))
    residual = bool(opts.get("residual", True))
    n_model = int(model.n_local)

    def sequential_one(mem):
        from .ggadmm import graph_admm
        (g, rho, quant), t = mem
        return graph_admm(model, g, rho, obj0, t, max_iter, backend=backend, name=name, engine_opts=engine_opts,
                          comm=comm, quantize=quant)

    def run_group(group, idx):
        from ..engine.graph_sweep import GraphSweepEngine
        from . import quantize as Q
        t_begin = time.perf_counter()
        g_mems = [g[0] for g in group]
        g_tols = [g[1] for g in group]
        key = ("graph-sweep", tuple((g.key(), rho) + (q or ()) for g, rho, q in g_mems), int(max_iter), xcd, residual)
        sw = _group_engine(model, key, opts, lambda: GraphSweepEngine.build(
            model.X, model.y, [(g, rho) + (q or ()) for g, rho, q in g_mems], obj0=obj0, tols=g_tols,
            max_iters=max_iter, precomputed=(model.A, model.b, model.yy), xcd=xcd, residual=residual), (obj0, g_tols))
        out = _one_launch_results(name, sw, t_begin, obj0, n_model, timeout_s=float(opts.get("timeout_s", 20.0)))
        for res, m, (g, rho, q) in zip(out, sw.members, g_mems):
            res.extra.update(kernel=sw.last_kernel, placed=res.extra["sweep"]["placed"], graph=g.describe(),
                             deliveries=res.iters * 2 * len(g.edges))
            if q is not None:
                G = Q.granules_per_row(model.d, q[0])
                _quant_accounting(res, q[0], q[1], g.n, model.d)
                res.extra.update(transmissions=res.iters * g.n, q_granules=G, q_wire_bytes=res.iters * g.n * G * 16,
                                 theta_true=m.theta_true)
        return out

    def capacity():
        from ..engine.graph_sweep import graph_sweep_capacity
        return graph_sweep_capacity()

    gates = [(backend == "torch", "torch backend"), (model.device.type != "cuda", "cpu tensors"),
             (comm is not None and comm.nranks > 1, "several ranks"),
             (getattr(model, "kind", None) != "linear", "not the linear closed-form model"), (model.d > 64, "d > 64"),
             (any(g.n != n_model for g, _, _ in parsed), "a member graph's n differs from the model's")]
    out: List[Optional[RunResult]] = [None] * len(parsed)
    for quantized in (False, True):  # one launch is homogeneous: the plain members, then the quantized ones
        idx = [i for i, (_, _, q) in enumerate(parsed) if (q is not None) == quantized]
        if not idx:
            continue
        res = _run_sweep([(parsed[i], tols[i]) for i in idx], sequential_one, gates, capacity, run_group,
                         "%s sweep native-graph%s N=%d K=%d" % (name, "-Q" if quantized else "", n_model, len(idx)))
        for i, r in zip(idx, res):
            out[i] = r
    return out


def dynamic_group_admm_sweep(model, rho, obj0, acc, max_iter, path, path_cost, coherences, seeds, kind="findPath2",
                             max_iters: Optional[Sequence[int]] = None, backend: str = "auto",
                             engine_opts: Optional[dict] = None, comm: Optional[Comm] = None, **kw) -> List[RunResult]:
    """``dynamic_group_admm`` at every coherence of ``coherences`` (member j re-chains from its own
    ``PathSchedule`` seeded ``seeds[j]``): one ``RunResult`` per coherence, in the order given, equal to
    ``[dynamic_group_admm(model, ..., coh, seed=s) for coh, s in zip(coherences, seeds)]`` in iterations,
    objective trace, ``com_cost``, ``comm_units``, primal residual and ``converged``. On one HIP device
    the solves run side by side, up to eight per kernel launch, one per XCD (engine/dyn_sweep.py; more
    run in groups): every member on the blocked kernel's dynamic mode, in rounds of epoch chunks, each
    to its own stop; a member that never re-chains within ``max_iter`` runs as a one-epoch slot. Only
    the chains a member reaches are drawn. Each result carries ``extra['sweep'] = {width, slot, kernel,
    placed, launches, wall_ms_launch}``; its ``wall_s`` is that solve's OWN time: the wall clock of the
    rounds it took part in less the device time between its stop decision and the end of its last
    round. ``extra['state']`` is not produced. ``max_iters``: one cap per member (default ``max_iter``).
    Anywhere else -- CPU tensors, ``backend='torch'``, several ranks, ``GADMM_CHECK_EXCHANGE=1``, no
    native library, a shape the kernel does not take, or a device that cannot hold the group's
    workgroups -- it IS that loop, and every result records ``extra['sweep_fallback'] = reason``.
    ``engine_opts``: ``refresh``, ``residual``, ``cache``, ``epoch_chunk`` as in ``chain_admm``."""
    coherences, seeds = list(coherences), list(seeds)
    if len(coherences) != len(seeds):
        raise ValueError("seeds: one per coherence (%d coherences, %d seeds)" % (len(coherences), len(seeds)))
    caps = [int(max_iter)] * len(coherences) if max_iters is None else [int(v) for v in max_iters]
    if len(caps) != len(coherences):
        raise ValueError("max_iters: one per coherence")
    n_total = kw.pop("n_total", model.n_local)
    local_ids = kw.pop("local_ids", list(range(model.n_local)))
    opts = dict(engine_opts or {})
    refresh = bool(opts.get("refresh", False))
    residual = bool(opts.get("residual", True))
    n_heads = (n_total + 1) // 2
    scale = n_heads if kw.get("cost_quirk", True) else 1

    def sequential_one(mem):
        coh, s, mi = mem
        return dynamic_group_admm(model, rho, obj0, acc, mi, path, path_cost, coh, seed=s, kind=kind, n_total=n_total,
                                  local_ids=local_ids, backend=backend, engine_opts=engine_opts, comm=comm, **kw)

    def run_group(group, idx):
        from ..engine.dyn_sweep import DynSweepEngine
        _timing.host_stamp("dsw:begin")
        g_caps = [g[2] for g in group]
        key = ("dyn-sweep", n_total, tuple(map(int, local_ids)), float(rho), len(group), tuple(g_caps), residual)
        sw = _group_engine(model, key, opts, lambda: DynSweepEngine.coherence_sweep(
            model.X, model.y, local_ids, n_total, rho, len(group), obj0=obj0, tol=acc, max_iters=g_caps,
            precomputed=(model.A, model.b, model.yy), residual=residual), (obj0, acc), refresh)
        placement = kw.get("placement") or Placement.contiguous(n_total, 1)
        scheds = []
        for m, (coh, seed, _) in zip(sw.members, group):
            sc = PathSchedule(n_total, path, path_cost, coh, kind=kind, seed=seed)
            m.set_path(sc.path, placement, 0)
            scheds.append(sc)
        runs = sw.run(scheds, epoch_chunk=opts.get("epoch_chunk"))
        out = []
        for j, (r, (coh, _, cap)) in enumerate(zip(runs, group)):
            iters = int(r.iters)
            if _static_schedule(scheds[j], cap):  # chain_admm's static-chain accounting
                com = np.arange(1, iters + 1) * (float(np.sum(r.cost0)) * scale)
            else:
                com = _dyn_com_cost(r, n_total, scale)[:iters]
            res = _member_result("D-GADMM(coh=%s)" % coh, sw, j, len(group), iters, r.done, obj0, n_total,
                                 sum(sw.last_round_ms[:r.rounds]) * 1e-3, r.tail_ticks, r.placed,
                                 engine="persistent-dynamic", com_cost=np.asarray(com[:iters]))
            res.extra["sweep"]["launches"] = res.extra["sweep_launches"] = int(r.rounds)
            out.append(res)
        _timing.host_stamp("dsw:end")
        return out

    def capacity():
        from ..engine.chain_sweep import sweep_capacity
        return sweep_capacity()

    check = kw.get("check_exchange")
    gates = [(model.device.type != "cuda", "cpu tensors"), (backend == "torch", "torch backend"),
             (comm is not None and comm.nranks > 1, "several ranks"),
             (model.kind != "linear" or sorted(int(w) for w in local_ids) != list(range(n_total))
              or kw.get("local_solver") not in (None, "closed") or kw.get("state") is not None or bool(kw.get("failures")),
              "not a one-GPU linear closed-form chain"),
             (check or (check is None and getenv("GADMM_CHECK_EXCHANGE", "0") == "1"), "exchange checker")]
    return _run_sweep(list(zip(coherences, seeds, caps)), sequential_one, gates, capacity, run_group,
                      "D-GADMM sweep native N=%d K=%d" % (n_total, len(coherences)))


def _dyn_com_cost(r, n_total: int, scale: int) -> np.ndarray:
    """Cumulative ``com_cost`` of the iterations covered by the epochs a sweep member drew, with the
    arithmetic of ``_chain_admm_native``'s ``cost_arrays`` (per-epoch hop-cost sums, scaled, one cumsum)."""
    drawn_C, nd = r.costs, len(r.starts)
    if drawn_C and any(c.dtype == object for c in drawn_C):
        Cn = np.empty(sum(len(c) for c in drawn_C), dtype=object)
        Cn[:] = [c for cc in drawn_C for c in cc]
    else:
        Cn = np.concatenate(drawn_C) if drawn_C else np.zeros((0, max(n_total - 1, 0)))
    csum = Cn.sum(axis=1) if (len(Cn) and Cn.dtype != object) else np.asarray([float(np.sum(c)) for c in Cn])
    per_it = np.concatenate([[float(np.sum(r.cost0))], csum]) * scale
    which = np.searchsorted(r.starts[:nd], np.arange(1, int(r.span) + 1), side="right") - 1
    return np.cumsum(per_it[which])
