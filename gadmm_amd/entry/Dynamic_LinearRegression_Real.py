"""E6 — ``dynamic_LinearRegression_Real.m``: Body Fat (10 workers x 25 rows), rho = 0.1,
D-GADMM with coherence 50 (<= 20,000 iterations). The reference's second curve calls the missing
``dynamic_group_ADMM_closedForm_v2`` and is not reproducible; only the A4 run is."""
import numpy as np

from ..parallel import topology as T
from .common import Problem, dgadmm_coherences, run_entry

ENTRY = "Dynamic_LinearRegression_Real"


def body(cfg, sess, args, writer):
    prob = Problem(cfg, sess)
    rng = np.random.default_rng(cfg.path_seed)
    path, cost, _ = T.find_path(prob.n_total, rng)
    runs = {}
    # (--set sweep=concurrent on one GPU: the coherences side by side, one per XCD)
    runs.update(dgadmm_coherences(prob, sess, args, cfg.rhos[0], path, cost, [cfg.path_seed] * len(cfg.coherences)))
    for r in runs.values():
        r.extra.pop("engine_obj", None)
        r.extra.pop("state", None)
    return {"runs": runs, "obj0": prob.obj0, "dataset": prob.dataset_meta,
            "note": "dynamic_group_ADMM_closedForm_v2 is referenced but not shipped (SURVEY.md D8)",
            "figure_groups": {"Dynamic_LinearRegression_Real": runs}}


def main(argv=None):
    return run_entry(ENTRY, body, argv)


if __name__ == "__main__":
    main()
