"""GPU: the solve kernels' PANOC inner iteration against the oracle bit for bit and against the literal step
(tests/panoc_reference.py) directly.

Full solves at every option set of panoc_reference.OPTION_SETS must give the oracle's bits.  Then a cap sweep: max_outer
= 1 and max_inner = 1 .. K.  The cap only enters the loop's end test, so every capped kernel run is a prefix of the
longer ones and equals the capped oracle run bit for bit.  Between consecutive caps the counters give the kernel's own
count of back-offs (1 + back-offs cost evaluations per step) and of line-search trials (gradient evaluations, + 1 for an
exhausted search under ls_failure = 1), and last_problem_norm_fpr and cost give ||r_k|| and psi(u_{k+1}).  Each must
equal the literal replay's decided value at that step."""
import numpy as np
import pytest

import panoc_reference as pr
from conftest import oracle_for
from test_gpu_alm_literal import KERNELS
from test_gpu_parity import assert_same_solution

pytestmark = pytest.mark.gpu

K = 16
SWEEP_SETS = ["default", "lsfail1", "bigc"]


def _case(kernel, set_name):
    make_cfg, kernel_name, B, kw = KERNELS[kernel]
    cfg = make_cfg()
    return cfg, kernel_name, B, pr.set_case(set_name, cfg, B, 311 + cfg.N_hor)


def _solve(cfg, kernel_name, B, case, opts, **env_kw):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    P, u0, y0, c0 = case
    s = BatchSolver(cfg, max_batch=B, **env_kw, **opts)
    try:
        if kernel_name is not None:
            assert s.kernel_name == kernel_name
        return s.solve(P, u0=u0, y0=y0, c0=c0), s.oracle_opts()
    finally:
        s.close()


@pytest.mark.parametrize("set_name", list(pr.OPTION_SETS))
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_full_solves_are_the_oracles(kernel, set_name):
    cfg, kernel_name, B, case = _case(kernel, set_name)
    P, u0, y0, c0 = case
    gpu, oo = _solve(cfg, kernel_name, B, case, pr.OPTION_SETS[set_name][0])
    assert_same_solution(gpu, oracle_for(cfg, **oo).solve_batch(P, u0=u0, y0=y0, c0=c0, threads=8))


@pytest.mark.parametrize("owners", ["1", "4"])
def test_team_modes_at_the_crafted_back_off_set(monkeypatch, owners):
    from mpc_trajectory_generator_amd import named_config
    cfg = named_config("cfg1")
    B = 160
    case = pr.set_case("inside", cfg, B, 2718)
    monkeypatch.setenv("NMPC_TEAM_OWNERS", owners)
    gpu, oo = _solve(cfg, None, B, case, pr.OPTION_SETS["inside"][0], experiments=True)
    P, u0, y0, c0 = case
    assert_same_solution(gpu, oracle_for(cfg, **oo).solve_batch(P, u0=u0, y0=y0, c0=c0, threads=8))


@pytest.mark.parametrize("set_name", SWEEP_SETS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_steps_follow_the_literal_rules(kernel, set_name):
    cfg, kernel_name, B, case = _case(kernel, set_name)
    P, u0, y0, c0 = case
    base = dict(pr.OPTION_SETS[set_name][0], max_outer=1)
    lsf = int(base.get("ls_failure", 0))
    runs = {}
    for cap in range(1, K + 1):
        opts = dict(base, max_inner=cap)
        gpu, oo = _solve(cfg, kernel_name, B, case, opts)
        assert_same_solution(gpu, oracle_for(cfg, **oo).solve_batch(P, u0=u0, y0=y0, c0=c0, threads=8))
        runs[cap] = gpu[2]
    o = oracle_for(cfg, **dict(base, max_inner=K))
    checked = 0
    for b in range(B):
        steps = o.solve_traced(P[b], None if u0 is None else u0[b], None if y0 is None else y0[b],
                               None if c0 is None else c0[b])[3]
        rep = pr.replay(cfg, dict(base, max_inner=K), P[b], steps)
        assert not rep["problems"], rep["problems"][:5]
        vals = rep["values"]
        for cap in range(2, K + 1):
            if cap >= len(vals) or vals[cap]["exit"]:
                break
            v, st, prev = vals[cap], runs[cap][b], runs[cap - 1][b]
            dcost = int(st["num_cost_evals"]) - int(prev["num_cost_evals"])
            dgrad = int(st["num_grad_evals"]) - int(prev["num_grad_evals"])
            if v["n_back"] is not None:
                assert dcost == 1 + v["n_back"], (b, cap)
            if v["n_trials"] is not None:
                if lsf == 1:
                    assert dgrad == v["n_trials"] + int(v["exhausted"]), (b, cap)
                else:
                    assert dgrad == v["n_trials"], (b, cap)
            if v["norm_r"] is not None:
                nr, tol = v["norm_r"]
                assert abs(float(st["last_problem_norm_fpr"]) - nr) <= tol, (b, cap)
            if v["psi_next"] is not None:
                ps, tol = v["psi_next"]
                assert abs(float(st["cost"]) - ps) <= tol, (b, cap)
            checked += 1
    assert checked >= B
