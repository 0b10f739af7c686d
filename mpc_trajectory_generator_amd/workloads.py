"""The BASELINE batch of a configuration and what "the same bits" means, for every probe and test that quotes a number.

bench.py's ``make_batch`` is the contract; tests/test_workloads.py holds ``baseline_batch`` to it array for array."""
import numpy as np

from .config import named_config
from .frontend import random_routes
from .harness import synthetic_batch

# what the generator adds per configuration: config 3 a synthetic circle field, config 4 random moving ellipses
_GENERATOR_FLAGS = {"cfg3": dict(synthetic_circles=True), "nobs50": dict(synthetic_circles=True),
                    "cfg4": dict(random_dyn=True), "smooth_velocity": dict(random_dyn=True)}

# the status fields two solves of one instance must agree on (solve_time_ms is a clock, reserved the kernel's pass counter)
PARITY_FIELDS = ("exit_status", "num_outer_iterations", "num_inner_iterations", "num_cost_evals",
                 "num_grad_evals", "last_problem_norm_fpr", "delta_y_norm_over_c", "f2_norm", "penalty", "cost")


def baseline_batch(name, B=8192, seed=0, *, scene=11, routes=32):
    """-> (cfg, P [B, n_p]): the batch bench.py times for ``--config name --batch B`` on rank ``seed``.
    ``routes`` start/goal pairs planned with seed 1000 + seed; 0: the scene's own route."""
    cfg = named_config(name)
    planned = random_routes(cfg, scene, routes, seed=1000 + seed) if routes > 0 else None
    return cfg, synthetic_batch(cfg, scene, B, seed=seed, routes=planned, **_GENERATOR_FLAGS.get(name, {}))


def differing(a, b, rows=None):
    """Names ("u", "y", status fields in PARITY_FIELDS order) on which the (u, y, status) triples ``a`` and ``b`` are not
    bit-equal; ``a`` is indexed by ``rows`` first (a permutation against a permuted re-solve, a sample against its own solve)."""
    (ua, ya, sa), (ub, yb, sb) = a, b
    if rows is not None:
        ua, ya, sa = ua[rows], ya[rows], sa[rows]
    pairs = [(f, sa[f], sb[f]) for f in PARITY_FIELDS] + [("u", ua, ub), ("y", ya, yb)]
    return [n for n, x, y in pairs if not np.array_equal(x, y)]
