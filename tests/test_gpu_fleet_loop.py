"""GPU: the receding-horizon loop on device with a fleet on many routes (nmpc_loop_new_routes) against its
host mirror ``FleetRecedingHorizon`` -- the ``VectorizedRecedingHorizon`` step with each robot's route looked up through
``route_of[b]``, itself pinned to the reference's goldens through tests/test_harness.py and tests/test_fleet_mirror.py -- driven by the oracle and given the kernels' sin / cos:
parameter vectors, states, reference indices, solver counters and trajectories must agree bit for bit, step
after step, whatever route each robot is on."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, step_differing, trajectory_differing

pytestmark = pytest.mark.gpu

B = 24


# (config, scene, K, steps, sinusoidal obstacle); "nobs3": fewer circle slots than some routes have vertices -> the
# closest-vertex window; "cfg2": N_hor = 40, the two-stages-per-lane kernel inside the loop
CASES = [("cfg4", 11, 3, 8, False), ("cfg1", 11, 0, 6, False), ("nobs3", 11, 1, 5, False), ("cfg2", 11, 2, 4, False),
         ("cfg4", 11, 3, 6, True)]


@pytest.mark.parametrize("R", [1, 3, B])
@pytest.mark.parametrize("name,scene,K,steps,sinus", CASES)
def test_fleet_loop_equals_host_mirror(name, scene, K, steps, sinus, R):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = load_config(Nobs=3) if name == "nobs3" else named_config(name)
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, scene, R, B, seed=31 + R)
    if R == B:
        assert sorted(route_of.tolist()) == list(range(B))          # every robot on a route of its own
    dyn = fleet_ellipses(routes, route_of, i0, K, 7 + R)
    o = oracle_for(cfg)
    s = BatchSolver(cfg, max_batch=32)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, sinus_object=sinus, route_of=route_of)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, sinus_object=sinus, idx0=i0)
        for k in range(steps):
            bad = step_differing(dev, host, o.warm_solve())[0]
            assert not bad, f"step {k}: {bad}"
        assert not trajectory_differing(dev, host, steps)
        dev.close()
    finally:
        s.close()


def test_fleet_routes_of_different_lengths_brake_and_finish_apart():
    """Routes of different lengths, robots started at different distances before their ends: some enter the
    braking branch and reach the goal while others still travel, and the device keeps the mirror's bits."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = named_config("cfg1")
    routes = [harness.scene_route(cfg, 1)] + frontend.random_routes(cfg, 1, 3, seed=5)
    n = np.array([len(r.x_ref) for r in routes])
    assert len(set(n.tolist())) > 1
    back = np.array([2, 5, 12, 40])
    route_of = np.repeat(np.arange(len(routes)), len(back)).astype(np.int32)
    i0 = np.maximum(0, n[route_of] - np.tile(back, len(routes))).astype(np.int32)
    starts = np.stack([[routes[r].x_ref[i], routes[r].y_ref[i], routes[r].theta_ref[i]] for r, i in zip(route_of, i0)])
    o = oracle_for(cfg)
    steps = 60
    mixed = []
    s = BatchSolver(cfg, max_batch=16)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        host = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0)
        for k in range(steps):
            bad, _, done = step_differing(dev, host, o.warm_solve())
            assert not bad, f"step {k}: {bad}"
            mixed.append(0 < done.sum() < len(done))
        assert not trajectory_differing(dev, host, steps)
        assert any(mixed), "no step with some robots at their goals and others not"
        dev.close()
    finally:
        s.close()


def test_both_entry_points_same_bits():
    """nmpc_loop_new_routes with one route and route_of = NULL is nmpc_loop_new."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg4")
    routes, _, starts, i0 = frontend.random_fleet(cfg, 11, 1, B, seed=3)
    dyn = fleet_ellipses(routes, np.zeros(B, dtype=np.int32), i0, 3, 4)
    steps = 6
    s1, s2 = BatchSolver(cfg, max_batch=32), BatchSolver(cfg, max_batch=32)
    try:
        a = DeviceRecedingHorizon(s1, routes[0], starts, dyn, max_steps=steps, idx0=i0)
        b = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=steps, idx0=i0)
        assert b.route_of is None
        for k in range(steps):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
            sa, sb = a.read()[4], b.read()[4]
            for f in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "penalty"):
                assert np.array_equal(sa[f], sb[f]), (k, f)
        assert np.array_equal(a.trajectory(), b.trajectory())
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_fleet_arguments_validated():
    """Every rejected case returns NMPC_ERR_BAD_ARG with a message and hands out no loop; the handle then still
    solves a batch exactly like the oracle."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import _fill_route
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 8, seed=2)
    n = np.array([len(r.x_ref) for r in routes])
    s = BatchSolver(cfg, max_batch=16)
    lib = s.lib
    i32 = C.POINTER(C.c_int32)
    starts = np.ascontiguousarray(starts)
    try:
        def call(R=3, rof=route_of, idx=i0, edit=None):
            keep = []
            rs = (_lib.NmpcRoute * 3)()
            for r, rt in zip(rs, routes):
                _fill_route(r, rt, keep)
            if edit:
                edit(rs)
            rof = None if rof is None else np.ascontiguousarray(rof, dtype=np.int32)
            idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
            out = C.c_void_p()
            rc = lib.nmpc_loop_new_routes(s._h, rs, R, None if rof is None else rof.ctypes.data_as(i32), len(starts),
                                          _lib.as_dp(starts), None if idx is None else idx.ctypes.data_as(i32), 0, None, 0,
                                          C.byref(out))
            return rc, out.value, lib.nmpc_last_error(s._h).decode()

        bad_route_of = route_of.copy()
        bad_route_of[3] = 3
        neg_route_of = route_of.copy()
        neg_route_of[0] = -1
        short = int(np.argmin(n))
        b_short = int(np.nonzero(route_of == short)[0][0])
        bad_idx = i0.copy()
        bad_idx[b_short] = n[short]                    # inside a longer route, outside its own

        def steps_differ(rs):
            rs[1].num_steps_taken = rs[0].num_steps_taken + 1

        def no_brake(rs):
            rs[2].n_brake = 0

        def no_ref(rs):
            rs[1].x_ref = None
        cases = {"R = 0": dict(R=0), "route_of out of range": dict(rof=bad_route_of), "route_of negative": dict(rof=neg_route_of),
                 "route_of NULL with R > 1": dict(rof=None), "num_steps_taken differs": dict(edit=steps_differ),
                 "route without braking table": dict(edit=no_brake), "route without x_ref": dict(edit=no_ref),
                 "idx0 outside its own route": dict(idx=bad_idx)}
        for what, kw in cases.items():
            rc, out, msg = call(**kw)
            assert rc == -3, what
            assert out is None, what
            assert msg, what
        rc, out, _ = call()                            # the same arguments, unedited, are accepted
        assert rc == 0 and out
        lib.nmpc_loop_free(C.c_void_p(out))
        P = harness.synthetic_batch(cfg, 11, 8, 77)
        u, y, st = s.solve(P)
        uo, yo, sto = oracle_for(cfg).solve_batch(P, threads=8)
        assert np.array_equal(u, uo) and np.array_equal(y, yo)
        assert np.array_equal(st["num_inner_iterations"], sto["num_inner_iterations"])
    finally:
        s.close()
