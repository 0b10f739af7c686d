"""GPU: the solve kernels' ALM outer loop off default options -- bit-exact against the oracle, and each outer step of the
kernels' own outputs recomputed with the literal rules (tests/alm_reference.py), so that the kernels are checked against
the plain reference and not only against the oracle they are edited together with.

Every option set of alm_reference.OPTION_SETS runs on every solve kernel: the epsilon_nu schedule and the third exit
criterion, penalties below 1 with nonzero multipliers and the Pi_Y clamp, stalls, growth and the budget exit.  The
instances that wait in pools between outer iterations (migration) or are helped by other waves (teams) carry epsilon_nu
with them: under a real schedule they must still give the oracle's bits."""
import numpy as np
import pytest

import alm_reference as ar
from conftest import oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.harness import synthetic_batch
from test_alm_literal import check_literal
from test_gpu_parity import assert_same_solution

pytestmark = pytest.mark.gpu

# name -> (config, kernel, batch, synthetic_batch keywords)
KERNELS = {
    "hyb-default": (lambda: named_config("cfg1"), "nmpc_solve_hyb_kernel<ShapeDefault>", 32, {}),
    "hyb-nobs50": (lambda: named_config("cfg3"), "nmpc_solve_hyb_kernel<ShapeNobs50>", 32, dict(synthetic_circles=True)),
    "hyb2-n40": (lambda: named_config("cfg2"), "nmpc_solve_hyb2_kernel<ShapeN40>", 16, {}),
    "any-n17": (lambda: load_config(N_hor=17, Nobs=4, Ndynobs=1), "nmpc_solve_hyb_kernel<ShapeAny>", 32, dict(random_dyn=True)),
    "any-n33": (lambda: load_config(N_hor=33), "nmpc_solve_hyb2_kernel<ShapeAny>", 16, {}),
}


@pytest.mark.parametrize("set_name", list(ar.OPTION_SETS))
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_outer_loop_is_the_oracles_and_the_literal_one(kernel, set_name):
    make_cfg, kernel_name, B, kw = KERNELS[kernel]
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg = make_cfg()
    P = synthetic_batch(cfg, 11, B, 606 + cfg.N_hor, **kw)
    y0, c0 = ar.set_inputs(set_name, B, cfg.n1, 17 + cfg.N_hor)
    handles = []

    def make(o):
        s = BatchSolver(cfg, max_batch=B, **o)
        handles.append(s)
        assert s.kernel_name == kernel_name
        return s.solve
    try:
        records, runs = ar.reconstruct(make, cfg, P, y0=y0, c0=c0, opts=ar.OPTION_SETS[set_name])
        oracle_opts = handles[-1].oracle_opts()                # the full cap: the last handle made
    finally:
        for s in handles:
            s.close()
    cpu = oracle_for(cfg, **oracle_opts).solve_batch(P, y0=y0, c0=c0, threads=8)
    assert_same_solution(runs[max(runs)], cpu)
    check_literal(ar.summary(records), records, runs, set_name)


@pytest.mark.parametrize("set_name", ["schedule", "ladder"])
def test_migration_under_an_epsilon_schedule(monkeypatch, set_name):
    """test_migration_between_wave_slots_is_invisible's recipe with epsilon_nu moving: parked instances carry it."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg, B = named_config("cfg1"), 2600
    P = synthetic_batch(cfg, 11, B, 99)
    y0, c0 = ar.set_inputs(set_name, B, cfg.n1, 99)
    monkeypatch.setenv("NMPC_PARK_MIN", "20")
    monkeypatch.setenv("NMPC_PARK_DEPTH", "64")
    s = BatchSolver(cfg, max_batch=B, experiments=True, **ar.OPTION_SETS[set_name])
    try:
        gpu = s.solve(P, y0=y0, c0=c0)
        opts = s.oracle_opts()
    finally:
        s.close()
    assert_same_solution(gpu, oracle_for(cfg, **opts).solve_batch(P, y0=y0, c0=c0, threads=8))
    assert (gpu[2]["num_outer_iterations"] >= 5).sum() >= B // 4


@pytest.mark.parametrize("set_name", ["schedule", "ladder"])
@pytest.mark.parametrize("owners", ["1", "4"])
@pytest.mark.parametrize("name,B", [("cfg1", 160), ("cfg2", 24)])
def test_team_modes_under_an_epsilon_schedule(monkeypatch, name, B, owners, set_name):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg = named_config(name)
    P = synthetic_batch(cfg, 11, B, 2718)
    y0, c0 = ar.set_inputs(set_name, B, cfg.n1, 2718)
    monkeypatch.setenv("NMPC_TEAM_OWNERS", owners)
    s = BatchSolver(cfg, max_batch=B, experiments=True, **ar.OPTION_SETS[set_name])
    try:
        gpu = s.solve(P, y0=y0, c0=c0)
        opts = s.oracle_opts()
    finally:
        s.close()
    cpu = oracle_for(cfg, **opts).solve_batch(P, y0=y0, c0=c0, threads=8)
    assert_same_solution(gpu, cpu)
    assert np.array_equal(gpu[2]["reserved"], cpu[2]["reserved"])


def test_full_batch_f2_norm_is_the_plain_norm_of_F2():
    """The bench's own cfg 1 batch: what every instance reports as f2_norm is ||F2(u)|| of the u it returns."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.workloads import baseline_batch
    cfg, P = baseline_batch("cfg1")
    s = BatchSolver(cfg, max_batch=len(P))
    try:
        u, y, st = s.solve(P)
    finally:
        s.close()
    _, F2, S2 = ar.plain_f1_f2(cfg, P, u, scale=True)
    f2 = np.sqrt((F2.astype(np.longdouble) ** 2).sum(axis=1)).astype(np.float64)
    tol = ar.F2_RTOL * f2 + ar.F2_ABS * np.sqrt((S2 ** 2).sum(axis=1))
    bad = np.abs(st["f2_norm"] - f2) > tol
    assert not bad.any(), (bad.sum(), np.flatnonzero(bad)[:10])
    assert (f2 > 0).sum() >= len(P) // 100                  # obstacles are touched on a share of the batch
