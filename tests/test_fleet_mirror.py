"""The host mirror of a fleet on many routes (``FleetRecedingHorizon``) against the single-route mirror
(``VectorizedRecedingHorizon``, pinned by tests/test_harness.py to ``BatchedRecedingHorizon`` and with it
to the goldens recorded from the reference's PathGenerator.run), with the oracle solving: a fleet's robots must get exactly the bits they
get on their own route, and ``frontend.random_fleet`` must deal robots and starts reproducibly."""
import numpy as np

from conftest import oracle_for
from mpc_trajectory_generator_amd import frontend, harness, named_config
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, VectorizedRecedingHorizon
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, route_fleet


def test_one_route_equals_vectorized_mirror():
    cfg = named_config("cfg4")
    route = harness.scene_route(cfg, 11)
    B, K, steps = 12, 3, 8
    i0, starts, _ = route_fleet(route, B, 3)
    route_of = np.zeros(B, dtype=np.int32)
    dyn = fleet_ellipses([route], route_of, i0, K, 4)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon([route], route_of, starts, dyn, sincos=o.sincos_array, idx0=i0)
    host = VectorizedRecedingHorizon(route, starts, dyn, sincos=o.sincos_array, idx0=i0)
    for k in range(steps):
        Pf, stf = fleet.step(o.warm_solve())
        Ph, sth = host.step(o.warm_solve())
        assert np.array_equal(Pf, Ph), f"step {k}"
        assert np.array_equal(fleet.U, host.U) and np.array_equal(fleet.Y, host.Y)
        assert np.array_equal(fleet.state, host.state) and np.array_equal(fleet.last_u, host.last_u)
        assert np.array_equal(fleet.idx, host.idx) and np.array_equal(fleet.done, host.done)
        assert np.array_equal(stf["num_inner_iterations"], sth["num_inner_iterations"])
    assert np.array_equal(np.stack(fleet.traj), np.stack(host.traj))


def test_three_routes_equal_three_separate_mirrors():
    cfg = named_config("cfg4")
    routes, _, _, _ = frontend.random_fleet(cfg, 11, 3, 3, seed=21)
    B, K, steps = 12, 2, 6
    route_of = np.arange(B) % 3                                     # interleaved: robot b on route b mod 3
    rng = np.random.default_rng(5)
    i0 = np.array([rng.integers(0, max(1, len(routes[r].x_ref) - 25)) for r in route_of])
    starts = np.stack([[routes[r].x_ref[i], routes[r].y_ref[i], routes[r].theta_ref[i]] for r, i in zip(route_of, i0)])
    starts = starts + rng.normal(0, 0.05, starts.shape)
    dyn = fleet_ellipses(routes, route_of, i0, K, 6)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0)
    alone = []
    for r, route in enumerate(routes):
        ids = np.nonzero(route_of == r)[0]
        h = VectorizedRecedingHorizon(route, starts[ids], tuple(a[ids] for a in dyn), sincos=o.sincos_array, idx0=i0[ids])
        alone.append((ids, h))
    for k in range(steps):
        P, _ = fleet.step(o.warm_solve())
        for ids, h in alone:
            Ph, _ = h.step(o.warm_solve(threads=4))
            assert np.array_equal(P[ids], Ph), f"step {k}"
            assert np.array_equal(fleet.U[ids], h.U) and np.array_equal(fleet.Y[ids], h.Y)
            assert np.array_equal(fleet.state[ids], h.state) and np.array_equal(fleet.idx[ids], h.idx)
            assert np.array_equal(fleet.done[ids], h.done)
    T = np.stack(fleet.traj)
    for ids, h in alone:
        assert np.array_equal(T[:, ids], np.stack(h.traj))


def test_random_fleet_is_deterministic_and_in_range():
    cfg = named_config("cfg4")
    a = frontend.random_fleet(cfg, 11, 5, 40, seed=9)
    b = frontend.random_fleet(cfg, 11, 5, 40, seed=9)
    c = frontend.random_fleet(cfg, 11, 5, 40, seed=10)
    routes, route_of, starts, idx0 = a
    assert len(routes) == 5 and route_of.shape == (40,) and starts.shape == (40, 3) and idx0.shape == (40,)
    assert np.array_equal(route_of, b[1]) and np.array_equal(starts, b[2]) and np.array_equal(idx0, b[3])
    assert all(np.array_equal(r.x_ref, q.x_ref) for r, q in zip(routes, b[0]))
    assert not np.array_equal(starts, c[2])
    assert set(route_of.tolist()) == set(range(5))                 # every route gets robots when B >= R
    n = np.array([len(r.x_ref) for r in routes])
    assert ((idx0 >= 0) & (idx0 < n[route_of])).all()
    ref = np.stack([[routes[r].x_ref[i], routes[r].y_ref[i]] for r, i in zip(route_of, idx0)])
    assert np.abs(starts[:, :2] - ref).max() < 0.5                 # a sample of the robot's own route plus noise
