"""CPU: the ALM outer loop against its literal rules, off default options (tests/alm_reference.py).

Every GPU test compares the solve kernels with the oracle bit for bit, and oracle and kernels are edited together; only
the cost layer is pinned to the reference.  Here the oracle's outer steps are recomputed from a plain long-double F1 / F2
and the rules of SURVEY.md App. C.3 / DESIGN.md section 9 under six option sets that move every ALM knob away from its
default: the epsilon_nu schedule and the third exit criterion, penalties below 1 with nonzero multipliers, the Pi_Y clamp,
stalls and penalty growth, the budget exit.  Plus the ranges nmpc_new and the oracle accept for those knobs."""
import numpy as np
import pytest

import alm_reference as ar
from conftest import VARIANTS, oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.harness import synthetic_batch
from test_gpu_parity import SHAPES

RTOL = 1e-12
B = 24
# the two solve-kernel classes: cfg 1 (N_hor = 20, one stage per lane) and its obstacles at N_hor = 33 (two stages per lane)
LOOP_SHAPES = {"cfg1": lambda: named_config("cfg1"), "n33": lambda: load_config(N_hor=33)}


def _close(a, b, rtol=RTOL):
    if np.size(b) == 0:
        return np.size(a) == 0
    return np.max(np.abs(a - b)) <= rtol * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_plain_cost_layer_matches_the_reference_goldens(golden, name):
    """f, F1, F2 of the plain evaluator against the vectors the reference's own MpcModule produced."""
    d, cfg = golden[name], named_config(VARIANTS[name])
    f = ar.plain_f(cfg, d["p"], d["u"])
    F1, F2 = ar.plain_f1_f2(cfg, d["p"], d["u"])
    assert np.max(np.abs(f - d["f"]) / np.abs(d["f"])) <= RTOL
    assert _close(F1, d["F1"]) and _close(F2, d["F2"])
    assert np.max(d["F2"]) > 0.0                                   # the obstacle terms are active in the goldens


def _shape_case(N, nobs, ndyn, B=6):
    """A batch of the shape with controls anywhere in U, circles dropped around the start position in half of the
    instances and ellipses over the start in the other half, so that F2 is not all zeros."""
    cfg = load_config(N_hor=N, Nobs=nobs, Ndynobs=ndyn)
    P = synthetic_batch(cfg, 11, B, 31 * N + 7 * nobs + ndyn, random_dyn=ndyn > 0)
    rng = np.random.default_rng(N + 100 * nobs + 1000 * ndyn)
    U = np.empty((B, cfg.n_u))
    U[:, 0::2] = rng.uniform(cfg.lin_vel_min, cfg.lin_vel_max, (B, N))
    U[:, 1::2] = rng.uniform(-cfg.ang_vel_max, cfg.ang_vel_max, (B, N))
    c0, d0 = 20 + N, 20 + N + 3 * nobs
    for b in range(B):
        for k in range(nobs):
            if b % 2 == 0:
                P[b, c0 + 3 * k:c0 + 3 * k + 3] = (P[b, 0] + rng.normal(0, 0.3), P[b, 1] + rng.normal(0, 0.3), rng.uniform(0.3, 1.5))
        for k in range(ndyn):
            if b % 2 == 1:
                for t in range(N):
                    o = d0 + (k * N + t) * 5
                    P[b, o:o + 5] = (P[b, 0] + rng.normal(0, 0.2), P[b, 1] + rng.normal(0, 0.2), rng.uniform(0.5, 3.0),
                                     rng.uniform(0.3, 2.0), rng.uniform(-np.pi, np.pi))
    return cfg, P, U


@pytest.mark.parametrize("N,nobs,ndyn", SHAPES)
def test_plain_f1_f2_matches_the_oracle_at_every_served_shape(N, nobs, ndyn):
    """The shapes of the GPU shape sweep, empty obstacle tables included."""
    cfg, P, U = _shape_case(N, nobs, ndyn)
    o = oracle_for(cfg)
    F1, F2 = ar.plain_f1_f2(cfg, P, U)
    f = ar.plain_f(cfg, P, U)
    assert F1.shape == (len(P), 2 * N) and F2.shape == (len(P), nobs + ndyn)
    for i in range(len(P)):
        fo, _, F1o, F2o = o.eval(P[i], U[i], grad=False)
        assert _close(F1[i], F1o) and _close(F2[i], F2o), i
        assert abs(f[i] - fo) <= RTOL * abs(fo), i
    if nobs:
        assert np.max(F2[0::2, :nobs]) > 0.0
    if ndyn:
        assert np.max(F2[1::2, nobs:]) > 0.0


@pytest.fixture(scope="module")
def literal():
    """(set, shape) -> (summary, records, runs) of the oracle's outer loop, each computed once."""
    done = {}

    def get(set_name, shape):
        if (set_name, shape) not in done:
            cfg = LOOP_SHAPES[shape]()
            P = synthetic_batch(cfg, 11, B, 2024 + cfg.N_hor)
            y0, c0 = ar.set_inputs(set_name, B, cfg.n1, 7 + cfg.N_hor)
            opts = ar.OPTION_SETS[set_name]

            def make(o):
                orc = oracle_for(cfg, **o)
                return lambda P, u0, y0, c0: orc.solve_batch(P, u0=u0, y0=y0, c0=c0, threads=8)
            records, runs = ar.reconstruct(make, cfg, P, y0=y0, c0=c0, opts=opts)
            done[set_name, shape] = ar.summary(records), records, runs
        return done[set_name, shape]
    return get


def check_literal(summ, records, runs, set_name):
    """The assertions every (solver, option set) pair must pass."""
    assert not summ["problems"], summ["problems"][:10]
    assert summ["ambiguous"] <= 0.01 * summ["decisions"], (summ["ambiguous"], summ["decisions"])
    if set_name in ar.FIRST_NU_CRIT3:                   # crit3: nothing converges before epsilon_nu has come down to epsilon
        first = ar.FIRST_NU_CRIT3[set_name]
        assert all(r["crit3"] == (r["nu"] >= first) for r in records)
        assert all(r["nu"] >= first for r in records if r["ends"] == "converged")
    st = runs[max(runs)][2]
    if set_name == "budget":
        assert np.all(st["num_inner_iterations"] <= 600)


@pytest.mark.parametrize("shape", list(LOOP_SHAPES))
@pytest.mark.parametrize("set_name", list(ar.OPTION_SETS))
def test_oracle_outer_loop_follows_the_literal_rules(literal, set_name, shape):
    summ, records, runs = literal(set_name, shape)
    check_literal(summ, records, runs, set_name)


def test_option_sets_exercise_every_branch(literal):
    """No vacuous pass: across the sets, every branch of the outer loop was taken."""
    summs = {(s, k): literal(s, k)[0] for s in ar.OPTION_SETS for k in LOOP_SHAPES}
    total = {key: sum(s[key] for s in summs.values()) for key in ("growth", "stall", "budget", "clamped", "small_c_with_y")}
    assert total["growth"] > 0 and total["stall"] > 0, total            # penalty growth and a stall at nu >= 1
    assert len({nu for s in summs.values() for nu in s["converged_nu"]}) >= 2
    assert total["clamped"] > 0 and total["small_c_with_y"] > 0, total
    assert total["budget"] > 0
    runs = [literal("budget", k)[2] for k in LOOP_SHAPES]
    assert any((r[max(r)][2]["exit_status"] == 2).any() for r in runs)          # NotConvergedOutOfTime under the full cap
    for k in LOOP_SHAPES:                               # loose: convergence early in the loop
        assert min(summs["loose", k]["converged_nu"]) <= 2


BAD_OPTIONS = [("tolerance", 0.0), ("tolerance", -1e-4), ("tolerance", np.nan), ("tolerance", np.inf),
               ("initial_tolerance", np.nan), ("initial_tolerance", 1e-5), ("initial_tolerance", np.inf),
               ("delta_tolerance", 0.0), ("delta_tolerance", np.nan), ("delta_tolerance", np.inf),
               ("initial_penalty", 0.0), ("initial_penalty", -1.0), ("initial_penalty", np.nan), ("initial_penalty", np.inf),
               ("penalty_update", 1.0), ("penalty_update", 0.5), ("penalty_update", np.nan), ("penalty_update", np.inf),
               ("tolerance_update", 0.0), ("tolerance_update", 1.0), ("tolerance_update", np.nan),
               ("sufficient_decrease", 0.0), ("sufficient_decrease", 1.0), ("sufficient_decrease", np.nan)]
GOOD_EDGES = [dict(initial_tolerance=1e-4), dict(penalty_update=1.0 + 1e-9), dict(tolerance_update=1e-9),
              dict(sufficient_decrease=1.0 - 1e-9), dict(initial_penalty=1e-300), dict(tolerance=1e-3, initial_tolerance=1e-3)]


@pytest.mark.parametrize("field,value", BAD_OPTIONS, ids=[f"{f}={v}" for f, v in BAD_OPTIONS])
def test_out_of_range_alm_options_are_refused(field, value):
    """include/nmpc_solver.h states the ranges; nmpc_new checks them before it asks for a device (NMPC_ERR_BAD_OPTS, not
    NO_DEVICE), the oracle's binding and orc_solve itself refuse them as well."""
    from mpc_trajectory_generator_amd.solver import BatchSolver, SolverError
    cfg = named_config("cfg1")
    with pytest.raises(SolverError) as e:
        BatchSolver(cfg, max_batch=4, **{field: value})
    assert e.value.code == -2
    with pytest.raises(RuntimeError):
        oracle_for(cfg, **{field: value})
    o = oracle_for(cfg)
    setattr(o.opts, field, value)                       # past the binding: orc_solve's own check
    with pytest.raises(RuntimeError, match="-6"):
        o.solve_batch(synthetic_batch(cfg, 11, 2, 3))


@pytest.mark.parametrize("opts", GOOD_EDGES, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_alm_options_at_the_edges_of_their_ranges_are_accepted(opts):
    from mpc_trajectory_generator_amd.solver import BatchSolver, SolverError
    cfg = named_config("cfg1")
    try:
        BatchSolver(cfg, max_batch=4, **opts).close()
    except SolverError as e:
        assert e.code == -4                             # no device here: the options passed
    u, y, st = oracle_for(cfg, **opts, max_outer=2, max_inner=20).solve_batch(synthetic_batch(cfg, 11, 2, 3))
    assert np.all(np.isfinite(u))
