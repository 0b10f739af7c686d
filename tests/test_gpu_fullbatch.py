"""GPU: every BASELINE configuration at FULL batch size under the driver (`pytest -m gpu`), on the bench's own
workload recipe (32 randomised start/goal routes planned by the visibility-graph front-end; cfg3: synthetic
50-circle field; cfg4: per-instance random moving ellipses).  At these sizes the oracle cannot solve the whole
batch in seconds, so the checks are the size-independent properties the domain offers -- input bounds,
(epsilon, delta)-AKKT exit conditions on the converged instances, permutation invariance (an instance's bits do
not depend on its slot, its wave-mates or the launch order) -- plus bit-exact oracle parity on a random sample."""
import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import harness, named_config
from mpc_trajectory_generator_amd.workloads import baseline_batch, differing, route_fleet

pytestmark = pytest.mark.gpu
B = 8192


@pytest.mark.parametrize("name,kernel,sample,B", [("cfg1", "nmpc_solve_hyb_kernel<ShapeDefault>", 64, 8192),
                                                  ("cfg2", "nmpc_solve_hyb2_kernel<ShapeN40>", 24, 8192),
                                                  ("cfg3", "nmpc_solve_hyb_kernel<ShapeNobs50>", 48, 8192),
                                                  ("cfg4", "nmpc_solve_hyb_kernel<ShapeDefault>", 48, 8192),
                                                  # BASELINE config 3 at its STATED total batch (65 536 over 8 GPUs; here on one): 8 waves of work per slot
                                                  ("cfg3", "nmpc_solve_hyb_kernel<ShapeNobs50>", 48, 65536)],
                         ids=["cfg1", "cfg2", "cfg3", "cfg4", "cfg3-65536"])
def test_full_batch_properties_and_sampled_parity(name, kernel, sample, B):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg, P = baseline_batch(name, B)
    s = BatchSolver(cfg, max_batch=B)
    try:
        assert s.kernel_name == kernel
        u, y, st = s.solve(P)
        # bounds U (src/mpc/mpc_generator.py:151-153): PANOC returns the projected half step
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(y))
        assert u[:, 0::2].min() >= cfg.lin_vel_min and u[:, 0::2].max() <= cfg.lin_vel_max
        assert np.abs(u[:, 1::2]).max() <= cfg.ang_vel_max
        # exit conditions on the converged ones: ||F2|| <= delta, ||y+ - y|| / c <= delta, and the iteration caps on all
        conv = st["exit_status"] == 0
        assert np.all(st["f2_norm"][conv] <= 1e-4 + 1e-12) and np.all(st["delta_y_norm_over_c"][conv] <= 1e-4 + 1e-12)
        assert np.all(st["last_problem_norm_fpr"][conv] < 1e-4)
        assert st["num_inner_iterations"].max() <= 5000 and st["num_outer_iterations"].max() <= 10
        assert set(np.unique(st["exit_status"])) <= {0, 1}
        # the acceleration constraints F1 in C (mpc_generator.py:157-168) hold to the ALM tolerance on converged solves
        acc = np.diff(np.concatenate([P[:, 3:4], u[:, 0::2]], axis=1), axis=1) / cfg.ts
        assert acc[conv].max() <= cfg.lin_acc_max + 5e-3 and acc[conv].min() >= cfg.lin_acc_min - 5e-3
        # permutation invariance
        perm = np.random.default_rng(0).permutation(B)
        assert not differing((u, y, st), s.solve(P[perm]), perm)
        # sampled oracle parity, bit for bit
        idx = np.random.default_rng(1).choice(B, sample, replace=False)
        assert not differing((u, y, st), oracle_for(cfg).solve_batch(P[idx], threads=8), idx)
    finally:
        s.close()


@pytest.mark.parametrize("name,seed", [("cfg2", 1), ("cfg2", 2), ("cfg1", 1), ("cfg4", 1)])
def test_full_batch_repeatable_on_other_seeds(name, seed):
    """A second launch on the permuted batch gives the same bits, on seeds the kernels were not tuned on.  This is the test that
    catches a build whose results depend on the schedule: the two-stage kernel runs at the limit of the register file, and two
    scheduler settings have produced such builds of it (csrc/Makefile, NMPC_WIN2 in nmpc_solve_hyb2.h); scripts/determinism_check.py
    is the long form (all configs, more seeds, sampled oracle parity)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg, P = baseline_batch(name, B, seed)
    s = BatchSolver(cfg, max_batch=B)
    try:
        u, y, st = s.solve(P)
        perm = np.random.default_rng(seed).permutation(B)
        assert not differing((u, y, st), s.solve(P[perm]), perm)
        idx = np.random.default_rng(100 + seed).choice(B, 12, replace=False)
        uo, yo, sto = oracle_for(cfg).solve_batch(P[idx], threads=8)
        assert np.array_equal(u[idx], uo) and np.array_equal(y[idx], yo)
    finally:
        s.close()


@pytest.mark.parametrize("steps,n_mirror", [(10, 24), (100, 8)], ids=["10steps-24robots", "100steps-8robots"])
def test_cfg4_device_loop_full_fleet(steps, n_mirror):
    """BASELINE config 4 at fleet size: 8192 robots x 10 receding-horizon steps -- and the configuration's stated 100
    steps (configs/smooth_velocity.yaml:17 num_steps_taken = 2; src/path_generator.py:290-403) -- entirely on device (assembly,
    warm-started solve, state advance), checked against the host mirror on a sample of robots -- a robot's
    parameter vectors, states and controls depend on nobody else in the fleet, so the mirror can run the sample
    alone and must reproduce it bit for bit."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, VectorizedRecedingHorizon
    cfg = named_config("cfg4")
    route = harness.scene_route(cfg, 11)
    i0, starts, dyn = route_fleet(route, B, 0, cfg.Ndynobs, back=60)
    ids = np.sort(np.random.default_rng(2).choice(B, n_mirror, replace=False))
    o = oracle_for(cfg)
    s = BatchSolver(cfg, max_batch=B)
    try:
        dev = DeviceRecedingHorizon(s, route, starts, dyn, max_steps=steps, idx0=i0)
        host = VectorizedRecedingHorizon(route, starts[ids], tuple(a[ids] for a in dyn), sincos=o.sincos_array, idx0=i0[ids])
        for k in range(steps):
            dev.step()
            P, st = host.step(o.warm_solve())
            if k in (0, 1, steps // 2, steps - 1):
                Pd, Ud, Yd = dev.params()
                assert np.array_equal(Pd[ids], P), f"step {k}"
                assert np.array_equal(Ud[ids], host.U) and np.array_equal(Yd[ids], host.Y)
        state, last_u, idx, done, std = dev.read()
        assert np.array_equal(state[ids], host.state) and np.array_equal(idx[ids], host.idx)
        assert np.all(np.isfinite(state))
        assert np.abs(last_u[:, 0]).max() <= cfg.lin_vel_max and np.abs(last_u[:, 1]).max() <= cfg.ang_vel_max
        T = dev.trajectory()
        assert T.shape == (steps * cfg.num_steps_taken + 1, B, 3)
        # every robot moved along its Euler model: consecutive poses are at most v_max * ts apart
        step_len = np.hypot(np.diff(T[:, :, 0], axis=0), np.diff(T[:, :, 1], axis=0))
        assert step_len.max() <= cfg.lin_vel_max * cfg.ts + 1e-12
        dev.close()
    finally:
        s.close()
