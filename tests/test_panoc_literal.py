"""CPU: the PANOC inner iteration against its literal rules (tests/panoc_reference.py).

The oracle's every PANOC step is recorded by ``Oracle.solve_traced`` and recomputed in long double from the published
rules: the Lipschitz probe, the back-off condition and its caps, the buffer resets, the sy-epsilon and C-BFGS tests in
their literal forms, the two-loop recursion, the FBE line search, the exit on ||r|| < epsilon and the literal AKKT
residual under each akkt_gradient.  Option sets and crafted instances push every branch to its edge.

Measured ambiguous fractions (decisions inside their rounding bound, where the replay follows the oracle), per set and
shape: at most 2.5 % (mem3 at N = 20) on every set but "inside", nearly all of them line-search tests in the tail where the
FBE decrease sits at psi's rounding; up to 21.9 % on "inside", whose penalty of 1e9 makes psi's rounding scale 1e9 times
its value.  The bounds below are 3 % and 25 %.  A branch counts as taken only on a step whose decisions behind it were
all decided."""
import numpy as np
import pytest

import alm_reference as ar
import panoc_reference as pr
from conftest import VARIANTS, oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.config import load_config
from test_alm_literal import _shape_case
from test_gpu_parity import SHAPES

B = 4
PANOC_SHAPES = {"n20": lambda: named_config("cfg1"),
                "n17o50": lambda: load_config(N_hor=17, Nobs=50, Ndynobs=3),
                "n33": lambda: load_config(N_hor=33, Nobs=0, Ndynobs=3),
                "n40": lambda: load_config(N_hor=40, Nobs=0, Ndynobs=0)}
# the largest ambiguous fraction a set may show (measured: see the module docstring)
AMBIGUOUS_MAX = dict({k: 0.03 for k in pr.OPTION_SETS}, inside=0.25)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_plain_psi_and_gradient_match_the_reference_goldens(golden, name):
    """grad f and, at each of the three (c, y), psi and grad psi against what the reference's own MpcModule produced."""
    d, cfg = golden[name], named_config(VARIANTS[name])
    f, g, _ = pr.psi_grad(cfg, d["p"], d["u"])
    assert _rel(f, d["f"]) <= 1e-13 and _rel(g, d["grad_f"]) <= 1e-12
    for j, (c, y) in enumerate(zip(d["xi_c"], d["xi_y"])):
        psi, g, _ = pr.psi_grad(cfg, d["p"], d["u"], c, y)
        assert _rel(psi, d["psi"][:, j]) <= 1e-13
        assert _rel(g, d["grad_psi"][:, j]) <= 1e-12, j


@pytest.mark.parametrize("N,nobs,ndyn", SHAPES)
def test_plain_psi_and_gradient_match_the_oracle_at_every_shape(N, nobs, ndyn):
    cfg, P, U = _shape_case(N, nobs, ndyn)
    rng = np.random.default_rng(N)
    c = np.array([0.5, 7.0, 125.0, 1.0, 3000.0, 0.25])[:len(P)]
    Y = rng.normal(0.0, 2.0, (len(P), cfg.n1))
    psi, g, kink, gs, ps = pr.psi_grad(cfg, P, U, c, Y, scale=True)
    o = oracle_for(cfg)
    for i in range(len(P)):
        po, go, _, _ = o.eval(P[i], U[i], c[i], Y[i])
        assert abs(po - float(psi[i])) <= pr.PSI_RTOL * ps[i], i
        if kink[i] >= pr.KINK_RTOL:
            assert np.max(np.abs(go - g[i].astype(np.float64))) <= pr.G_RTOL * gs[i], i


@pytest.fixture(scope="module")
def literal():
    """(set, shape) -> (cfg, opts, case, runs, replays), each computed once."""
    done = {}

    def get(set_name, shape):
        if (set_name, shape) not in done:
            cfg = PANOC_SHAPES[shape]()
            opts = pr.OPTION_SETS[set_name][0]
            case = pr.set_case(set_name, cfg, B, 797 + cfg.N_hor)
            P, u0, y0, c0 = case
            o = oracle_for(cfg, **opts)
            runs = [o.solve_traced(P[b], None if u0 is None else u0[b], None if y0 is None else y0[b],
                                   None if c0 is None else c0[b]) for b in range(B)]
            reps = [pr.replay(cfg, opts, P[b], runs[b][3]) for b in range(B)]
            done[set_name, shape] = cfg, opts, case, runs, reps
        return done[set_name, shape]
    return get


@pytest.mark.parametrize("set_name", list(pr.OPTION_SETS))
def test_the_trace_leaves_the_bits_unchanged(literal, set_name):
    cfg, opts, (P, u0, y0, c0), runs, _ = literal(set_name, "n20")
    u, y, st = oracle_for(cfg, **opts).solve_batch(P, u0=u0, y0=y0, c0=c0, threads=4)
    for b, (ub, yb, sb, steps) in enumerate(runs):
        assert np.array_equal(u[b], ub) and np.array_equal(y[b], yb)
        for f in ar.STATUS_COPY:
            assert np.array_equal(st[f][b], sb[f]), f
        # every inner solve calls step() once more than it counts iterations: the call that exits or meets the cap
        assert len(steps) == int(sb["num_inner_iterations"]) + int(sb["num_outer_iterations"])


@pytest.mark.parametrize("shape", list(PANOC_SHAPES))
@pytest.mark.parametrize("set_name", list(pr.OPTION_SETS))
def test_oracle_inner_loop_follows_the_literal_rules(literal, set_name, shape):
    *_, reps = literal(set_name, shape)
    problems = [(b, p) for b, r in enumerate(reps) for p in r["problems"]]
    assert not problems, problems[:10]
    dec, amb = sum(r["decisions"] for r in reps), sum(r["ambiguous"] for r in reps)
    print(f"{set_name}/{shape}: {dec} decisions, {amb} ambiguous ({100 * amb / dec:.2f} %)")
    assert dec > 0 and amb <= AMBIGUOUS_MAX[set_name] * dec, (amb, dec)


def test_option_sets_reach_every_edge(literal):
    """No vacuous pass: across the sets, every branch of the step was taken on a decided step, the C-BFGS rejection
    ("flat") and an AKKT test passed on a g_prev carried over from the previous inner solve ("akkt0") included."""
    seen = {}
    for s in pr.OPTION_SETS:
        for k in PANOC_SHAPES:
            for r in literal(s, k)[4]:
                for key, n in r["seen"].items():
                    seen[key] = seen.get(key, 0) + n
    need = ["exit", "fpr_pass_akkt_fail", "backoffs_0", "backoffs_1", "backoffs_10", "L_stop", "L_clamp", "pushed",
            "rejected_sy", "rejected_cbfgs", "wrap_m1", "wrap_m10", "accept_tau1", "accept_tau_lt1", "exhausted_ls0",
            "exhausted_ls1", "reset_nonempty", "akkt_carried_pass"]
    missing = [k for k in need if not seen.get(k)]
    assert not missing, (missing, seen)
    for s in ("akkt0", "akkt2"):                          # an exit under each AKKT form that has one
        assert sum(r["seen"].get("exit", 0) for k in PANOC_SHAPES for r in literal(s, k)[4]) > 0, s
