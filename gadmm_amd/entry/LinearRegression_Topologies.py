"""G1 (beyond the reference) -- GGADMM over bipartite graphs: the E1 data (N = 24 workers, 50 x 50
shards), rho = 3, acc = 1e-4, one solve per graph of ``graphs`` (chain, ring, 4 x 6 grid, star around
worker 0, complete bipartite even vs odd ids) and rho. The chain is GADMM; the other graphs reach the
same gap in a fraction of its iterations (algorithms/ggadmm.py). Outputs one run per graph x rho,
``GGADMM_<graph>_rho<rho>``, with the usual summary, per-iteration traces and the three panels (gap
against iteration / cumulative communication / clock); each summary names its engine, kernel and graph.
``quant_bits`` (4, 8, 16; seed ``quant_seed``) adds a Q-GGADMM run per graph x rho x bit width next to
them, ``Q-GGADMM_b<bits>_<graph>_rho<rho>``: the quantized exchange of Q-GADMM on the graph, its
communication counted in equivalent full-precision messages. ``sweep=concurrent`` on one GPU runs the
whole list side by side, up to eight solves per kernel launch, one per XCD (``graph_admm_sweep``): the
same runs, each summary also naming its sweep kernel and slot.

    python -m gadmm_amd LinearRegression_Topologies
    python -m gadmm_amd LinearRegression_Topologies --quick --device cpu
    python -m gadmm_amd LinearRegression_Topologies --set graphs=ring,grid:3x8 rhos=1,3
    python -m gadmm_amd LinearRegression_Topologies --set quant_bits=8,4
    python -m gadmm_amd LinearRegression_Topologies --set sweep=concurrent quant_bits=8
"""
from .common import Problem, attach_modelled_clock, run_entry

ENTRY = "LinearRegression_Topologies"


def body(cfg, sess, args, writer):
    from ..algorithms import graph_admm
    from ..parallel.topology import parse_graph
    from ..utils.timing import roctx_range

    if sess.world != 1:
        raise NotImplementedError("%s: one process (graph_admm keeps every worker local)" % ENTRY)
    prob = Problem(cfg, sess)
    sess.log("  obj0 = %.13f (normal equations, opt_sol_closedForm.m)" % prob.obj0)
    runs = {}

    def keep(key, r, spec, graph, rho):
        for k in ("engine_obj", "state", "theta_true", "q_msg"):
            r.extra.pop(k, None)
        r.extra.update(graph_name=str(spec), graph_edges=len(graph.edges), graph_max_degree=graph.max_degree,
                       rho=float(rho))
        runs[key] = attach_modelled_clock(r, prob.model, rho, sess)

    # --set sweep=concurrent on a one-GPU session (the exclusions of common.gadmm_sweep): the graphs x rho
    # list, and with quant_bits the bits x graphs x rho list, side by side, up to eight solves per launch,
    # one per XCD (graph_admm_sweep: same run keys, names and iteration counts; where that call is the
    # sequential loop, the summaries carry sweep_fallback)
    concurrent = (cfg.sweep == "concurrent" and cfg.model == "linear" and sess.device.type == "cuda"
                  and args.backend != "torch" and len(cfg.rhos) > 0 and len(cfg.graphs) > 0)
    if concurrent:
        from ..algorithms import graph_admm_sweep

        plain = [(spec, parse_graph(spec, prob.n_total), rho) for spec in cfg.graphs for rho in cfg.rhos]
        with roctx_range("ggadmm sweep concurrent"):
            rs = graph_admm_sweep(prob.model, [(g, rho) for _, g, rho in plain], prob.obj0, cfg.acc, cfg.gadmm_iters,
                                  backend=args.backend)
        for (spec, graph, rho), r in zip(plain, rs):
            r.algorithm = "GGADMM(%s,rho=%g)" % (spec, rho)
            keep("GGADMM_%s_rho%g" % (spec, rho), r, spec, graph, rho)
        quant = [(int(bits), spec, graph, rho) for bits in cfg.quant_bits for spec, graph, rho in plain]
        if quant:
            with roctx_range("q-ggadmm sweep concurrent"):
                rs = graph_admm_sweep(prob.model, [(g, rho, bits, cfg.quant_seed) for bits, _, g, rho in quant],
                                      prob.obj0, cfg.acc, cfg.gadmm_iters, backend=args.backend, name="Q-GGADMM")
            for (bits, spec, graph, rho), r in zip(quant, rs):
                r.algorithm = "Q-GGADMM(b=%d,%s,rho=%g)" % (bits, spec, rho)
                keep("Q-GGADMM_b%d_%s_rho%g" % (bits, spec, rho), r, spec, graph, rho)
        return {"runs": runs, "obj0": prob.obj0, "dataset": prob.dataset_meta,
                "figure_groups": {"LinearRegression_Topologies": runs}}
    for spec in cfg.graphs:
        graph = parse_graph(spec, prob.n_total)
        for rho in cfg.rhos:
            with roctx_range("ggadmm %s rho=%g" % (spec, rho)):
                r = graph_admm(prob.model, graph, rho, prob.obj0, cfg.acc, cfg.gadmm_iters, backend=args.backend,
                               name="GGADMM(%s,rho=%g)" % (spec, rho))
            keep("GGADMM_%s_rho%g" % (spec, rho), r, spec, graph, rho)
    for bits in cfg.quant_bits:  # Q-GGADMM next to them
        for spec in cfg.graphs:
            graph = parse_graph(spec, prob.n_total)
            for rho in cfg.rhos:
                with roctx_range("q-ggadmm b=%d %s rho=%g" % (int(bits), spec, rho)):
                    r = graph_admm(prob.model, graph, rho, prob.obj0, cfg.acc, cfg.gadmm_iters, backend=args.backend,
                                   name="Q-GGADMM(b=%d,%s,rho=%g)" % (int(bits), spec, rho),
                                   quantize=(int(bits), cfg.quant_seed))
                keep("Q-GGADMM_b%d_%s_rho%g" % (int(bits), spec, rho), r, spec, graph, rho)
    return {"runs": runs, "obj0": prob.obj0, "dataset": prob.dataset_meta,
            "figure_groups": {"LinearRegression_Topologies": runs}}


def main(argv=None):
    return run_entry(ENTRY, body, argv)


if __name__ == "__main__":
    main()
