"""G3 (beyond the reference) -- logistic GGADMM over bipartite graphs: the E3 data (N = 24 workers, 50 x 50
shards, lam = 1e-5), the reference's inexact local solver (inner GD, ``gd_step`` = 2.2, at most ``max_inner``
= 100 steps), acc = 1e-4, one solve per graph of ``graphs`` (chain, ring, 4 x 6 grid, star around worker 0,
complete bipartite even vs odd ids) and rho through ``graph_admm_logistic`` (algorithms/ggadmm.py). The chain
is ``group_admm_logistic_gd``. Outputs one run per graph x rho, ``GGADMM-logistic_<graph>_rho<rho>``, with
the usual summary, per-iteration traces and the three panels; each summary names its engine, kernel and
graph, and ``graph_fallback`` where the torch path ran.

rho = 2e-4 (E3's second value, the chain's 53 iterations) reaches the gap on every graph inside
``gadmm_iters`` = 400: on the torch path on the CPU the chain takes 53 iterations, the ring 212, the 4 x 6 grid
128, the star 134 and the complete bipartite graph 257.

``sweep=concurrent`` on one GPU runs the whole list side by side, up to eight solves per kernel launch, one
per XCD (``graph_admm_logistic_sweep``): the same runs, each summary also naming its sweep kernel and slot.

    python -m gadmm_amd LogisticRegression_Topologies
    python -m gadmm_amd LogisticRegression_Topologies --quick --device cpu
    python -m gadmm_amd LogisticRegression_Topologies --set graphs=ring,grid:3x8 rhos=2e-4,3e-4
    python -m gadmm_amd LogisticRegression_Topologies --set sweep=concurrent
"""
from .common import Problem, attach_modelled_clock, run_entry

ENTRY = "LogisticRegression_Topologies"


def body(cfg, sess, args, writer):
    from ..algorithms import graph_admm_logistic
    from ..parallel.topology import parse_graph
    from ..utils.timing import roctx_range

    if sess.world != 1:
        raise NotImplementedError("%s: one process (graph_admm_logistic keeps every worker local)" % ENTRY)
    prob = Problem(cfg, sess)
    sess.log("  obj0 = %.13f (Newton on the stacked problem)" % prob.obj0)
    runs = {}

    def keep(r, spec, graph, rho):
        for k in ("engine_obj", "state"):
            r.extra.pop(k, None)
        r.extra.update(graph_name=str(spec), graph_edges=len(graph.edges), graph_max_degree=graph.max_degree,
                       rho=float(rho))
        runs["GGADMM-logistic_%s_rho%g" % (spec, rho)] = attach_modelled_clock(r, prob.model, rho, sess)

    # --set sweep=concurrent on a one-GPU session (the exclusions of LinearRegression_Topologies): the graphs x
    # rho list side by side, up to eight solves per launch, one per XCD (graph_admm_logistic_sweep: same run
    # keys, names and iteration counts; where that call is the sequential loop, the summaries carry
    # sweep_fallback)
    if (cfg.sweep == "concurrent" and sess.device.type == "cuda" and args.backend != "torch" and len(cfg.rhos) > 0
            and len(cfg.graphs) > 0):
        from ..algorithms import graph_admm_logistic_sweep

        todo = [(spec, parse_graph(spec, prob.n_total), rho) for spec in cfg.graphs for rho in cfg.rhos]
        with roctx_range("ggadmm-logistic sweep concurrent"):
            rs = graph_admm_logistic_sweep(prob.model, [(g, rho) for _, g, rho in todo], prob.obj0, cfg.acc,
                                           cfg.gadmm_iters, cfg.gd_step, max_inner=cfg.max_inner, backend=args.backend)
        for (spec, graph, rho), r in zip(todo, rs):
            r.algorithm = "GGADMM-logistic(%s,rho=%g)" % (spec, rho)
            keep(r, spec, graph, rho)
        return {"runs": runs, "obj0": prob.obj0, "dataset": prob.dataset_meta, "figure_groups": {ENTRY: runs}}
    for spec in cfg.graphs:
        graph = parse_graph(spec, prob.n_total)
        for rho in cfg.rhos:
            with roctx_range("ggadmm-logistic %s rho=%g" % (spec, rho)):
                r = graph_admm_logistic(prob.model, graph, rho, prob.obj0, cfg.acc, cfg.gadmm_iters, cfg.gd_step,
                                        max_inner=cfg.max_inner, backend=args.backend,
                                        name="GGADMM-logistic(%s,rho=%g)" % (spec, rho))
            keep(r, spec, graph, rho)
    return {"runs": runs, "obj0": prob.obj0, "dataset": prob.dataset_meta, "figure_groups": {ENTRY: runs}}


def main(argv=None):
    return run_entry(ENTRY, body, argv)


if __name__ == "__main__":
    main()
