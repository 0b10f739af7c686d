"""The host mirror of a fleet on many routes (``FleetRecedingHorizon``) against the single-route mirror
(``VectorizedRecedingHorizon``, pinned by tests/test_harness.py to ``BatchedRecedingHorizon`` and with it
to the goldens recorded from the reference's PathGenerator.run), with the oracle solving: a fleet's robots must get exactly the bits they
get on their own route, and ``frontend.random_fleet`` must deal robots and starts reproducibly.

The two mirrors are one step over flat per-robot arrays, the single-route one its case of one route, so that comparison tests the
lookup through ``route_of`` and nothing else.  ``test_mixed_routes_equal_the_per_robot_loop`` therefore holds a fleet on routes of
very different tables directly to ``BatchedRecedingHorizon``, the literal per-robot step."""
import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import frontend, harness, named_config
from mpc_trajectory_generator_amd.trajectory import BatchedRecedingHorizon, FleetRecedingHorizon, VectorizedRecedingHorizon
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, handmade_route, route_fleet
from test_loop_shapes_mirror import _lists


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


@pytest.mark.parametrize("K,sinus", [(2, False), (3, True)])
def test_mixed_routes_equal_the_per_robot_loop(K, sinus):
    """Twelve robots interleaved over four routes whose tables differ in every length: the scene's (6 vertices, fewer than Nobs), a
    handmade one with 14 vertices (more than Nobs: the closest-vertex window), a handmade one of a few samples without vertices, and a
    planned one.  Robots 2, 8 and 25 samples before the scene route's end brake and get inside the last sample; K = 2 of Ndynobs = 3
    leaves a padding slot that inherits stale ellipses of obstacle 0, K = 3 with the sinusoidal law fills them all (robots 3 and 10 of
    that case have obstacle directions on which ``np.arctan2`` can differ from ``math.atan2`` in the last bit: the mirror takes libm's)."""
    cfg = named_config("cfg4")
    rng = np.random.default_rng(31)
    many = [(2.0 + 0.45 * k, 2.9 + 0.2 * (k % 3)) for k in range(14)]
    routes = [harness.scene_route(cfg, 11), handmade_route(cfg, [(2.0, 2.0), (8.0, 2.0), (8.0, 6.0)], many),
              handmade_route(cfg, [(2.0, 2.0), (3.5, 2.0)]), frontend.random_routes(cfg, 11, 1, seed=8)[0]]
    n = np.array([len(r.x_ref) for r in routes])
    assert cfg.Ndynobs == 3 and len(routes[0].vertices) <= cfg.Nobs < len(routes[1].vertices)
    assert routes[2].vertices == [] and n[2] < cfg.N_hor and n[0] > 25 and n[1] > 25 and n[3] > 25
    B, R, steps = 12, 4, 6
    route_of = np.arange(B) % R                                     # interleaved: robot b on route b mod 4
    back = np.array([2, 30, n[2], 40, 8, 2, 1, 25, 25, 12, 3, 60])    # samples before the own route's end
    i0 = np.maximum(0, n[route_of] - back)
    assert list(n[0] - i0[route_of == 0]) == [2, 8, 25]
    starts = np.stack([[routes[r].x_ref[i], routes[r].y_ref[i], routes[r].theta_ref[i]] for r, i in zip(route_of, i0)])
    starts[3:] += rng.normal(0, 0.05, starts[3:].shape)             # the first robot of the first three routes stands on its sample
    dyn = fleet_ellipses(routes, route_of, i0, K, 6)
    o = oracle_for(cfg, max_inner=40, max_outer=2)                  # cheap solves: the assembly is what is tested
    solve = o.warm_solve(threads=4)
    fleet = FleetRecedingHorizon(routes, route_of, starts, dyn, sinus_object=sinus, idx0=i0)
    loops = []
    for r, route in enumerate(routes):
        ids = np.nonzero(route_of == r)[0]
        loops.append((ids, BatchedRecedingHorizon(route, starts[ids], _lists(tuple(a[ids] for a in dyn), len(ids)), sinus_object=sinus,
                                                  idx0=i0[ids])))
    inside = 0
    for k in range(steps):
        P, _ = fleet.step(solve)
        for ids, loop in loops:
            Pl, _ = loop.step(solve)
            assert np.array_equal(P[ids], Pl), (k, ids, np.argwhere(P[ids] != Pl)[:5])
            assert np.array_equal(fleet.idx[ids], loop.idx), k
        inside += int((fleet.idx == n[route_of] - 1).sum())
    assert inside, "no robot inside the last sample of its route: the distance-based braking never ran"
    for ids, loop in loops:
        assert np.array_equal(fleet.state[ids], np.array([s[-3:] for s in loop.states]))
        assert np.array_equal(fleet.done[ids], loop.done)


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
