"""GPU: the on-device loop with walls (nmpc_loop_set_walls, nmpc_loop_walls; ``nmpc_loop_walls_kernel``)
against its host mirror ``FleetRecedingHorizon(..., walls=...)`` -- itself pinned to a literal per-robot, per-edge, per-stage loop of
the rule by tests/test_walls_mirror.py -- driven by the oracle and given the kernels' sin / cos: parameter vectors, controls,
multipliers, states, reference indices, solver counters and trajectories, and the walls' edges and stages, must agree bit for bit, step
after step."""

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config
from mpc_trajectory_generator_amd.workloads import (clearance_differing, crowd_ellipses, fleet_ellipses, map_clearance_differing, mission_fleet,
                                                    plant_differing, staggered_fleet, step_differing, trajectory_differing, walls_differing)
from test_loop_shapes_mirror import CASES as SHAPES
from test_walls_mirror import B, NAN_ROBOT, PLANT, fleet24, nan_fleet, radius, retiring_until, scene_map, walls_of

pytestmark = pytest.mark.gpu


def run_pair(cfg, routes, route_of, starts, i0, dyn, walls, steps, until=None, sinus_object=False, **kw):
    """Step a device loop and its mirror ``steps`` times (or while ``until(host)`` says so, ``steps`` at the most), comparing
    everything at every step -> (the mirror, per step the edges chosen, per step the device's parameter vectors)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    o = oracle_for(cfg)
    seen, Ps = [], []
    s = BatchSolver(cfg, max_batch=32)
    dev = None
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of, sinus_object=sinus_object, walls=walls, **kw)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, sinus_object=sinus_object, idx0=i0, walls=walls, **kw)
        while host.steps < steps and (until is None or until(host)):
            k = host.steps
            bad, Pd, _ = step_differing(dev, host, o.warm_solve())
            assert not bad, f"step {k}: {bad}"
            bad = walls_differing(dev, host)
            assert not bad, f"step {k}: {bad}"
            if kw.get("monitor") is not None:
                assert not clearance_differing(dev, host), f"step {k}"
            if kw.get("map_monitor") is not None:
                assert not map_clearance_differing(dev, host), f"step {k}"
            if kw.get("plant") is not None:
                assert not plant_differing(dev, host), f"step {k}"
            seen.append(host.wall_edge.copy())
            Ps.append(Pd)
        assert not trajectory_differing(dev, host, host.steps)
    finally:
        if dev is not None:                    # before its solver: a loop must not outlive the handle it was made on
            dev.close()
        s.close()
    return host, seen, Ps


def test_scene_map_leaves_lanes_without_an_edge():
    """26 edges: 38 lanes of the wave hold none; from the second step on robots with no, one, two and three walls in reach."""
    cfg = named_config("cfg1")
    _, seen, _ = run_pair(cfg, *fleet24(cfg), None, walls_of(cfg), 4)
    assert set((seen[1] >= 0).sum(axis=1).tolist()) == {0, 1, 2, 3}


def test_cut_in_four_with_spacing_and_both_monitors():
    """104 edges: a lane's second edge, candidates skipped for spacing, the clearance monitor seeing wall circles and the map monitor
    beside them."""
    from mpc_trajectory_generator_amd.trajectory import MapMonitor, Monitor
    cfg = named_config("cfg1")
    host, seen, _ = run_pair(cfg, *fleet24(cfg), None, walls_of(cfg, pieces=4, spacing=1.0), 4, monitor=Monitor(),
                             map_monitor=MapMonitor(*scene_map(cfg, 4)))
    assert (np.stack(seen) >= 64).any() and np.isfinite(host.clearance["circle"]).all()


def test_cut_in_39_sixteen_edges_per_lane_at_the_long_horizon():
    """1014 edges, the limit of 16 per lane, at N = 40 with the two-stage solve kernel inside the loop."""
    cfg = named_config("cfg2")
    assert cfg.N_hor == 40
    walls = walls_of(cfg, pieces=39, spacing=1.0)
    assert len(walls.edges) == 1014
    _, seen, _ = run_pair(cfg, *fleet24(cfg), None, walls, 3)
    assert (np.stack(seen) >= 512).any()                                   # an edge from deep in a lane's list


@pytest.mark.parametrize("which", ["n33-s7", "s20"])
def test_shapes(which):
    """N = 33 with 7 steps taken, and s = N = 20: K = 2 scripted ellipses, four wall slots behind the route's six vertices."""
    from mpc_trajectory_generator_amd.trajectory import Walls
    c = SHAPES[which]()
    n = len(c.starts)
    assert len(c.route.vertices) == 6 and c.cfg.Nobs == 10 and c.K == 2
    walls = Walls(scene_map(c.cfg)[0], 4, radius(c.cfg), 3.0)
    _, seen, _ = run_pair(c.cfg, [c.route], np.zeros(n, dtype=np.int32), c.starts, c.idx0, c.dyn, walls, c.steps, sinus_object=c.sinus)
    assert (np.stack(seen) >= 0).any()


def test_beside_a_crowd_and_grid_peers():
    """cfg4 with a crowd slot and a grid peer slot: circle and ellipse overlays in one step."""
    from mpc_trajectory_generator_amd.trajectory import Crowd, Peers
    cfg = named_config("cfg4")
    routes, route_of, starts, i0 = fleet24(cfg)
    dyn = fleet_ellipses(routes, route_of, i0, 1, 9)
    crowd = Crowd(crowd_ellipses(cfg, 11, 70, 23), 1, 1e3)
    peers = Peers(slots=1, rx=0.37, ry=0.53, range=1e3, cell=1.0)
    host, seen, _ = run_pair(cfg, routes, route_of, starts, i0, dyn, walls_of(cfg, pieces=4, spacing=1.0), 3, crowd=crowd, peers=peers)
    assert (np.stack(seen) >= 0).any() and (host.crowd_seen >= 0).all() and (host.peer_index >= 0).all()


def test_retiring_fleet():
    """Robots retire one after the other: a retired robot keeps p and its record, and steps with nobody active launch nothing."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg, back=(2, 5, 9))
    host, seen, Ps = run_pair(cfg, routes, route_of, starts, i0, None, walls_of(cfg, rng_=3.0, scene=1), 45, until=retiring_until(), retire=True)
    at = host.retired_at
    assert host.n_active == 0 and len(set(at.tolist())) > 2 and host.steps == at.max() + 2
    assert np.array_equal(Ps[-1], Ps[-3]) and np.array_equal(seen[-1], seen[-3])
    first = int(np.argmin(at))
    assert at[first] < at.max() and all(np.array_equal(P[first], Ps[at[first] - 1][first]) for P in Ps[at[first]:])


def test_missions_redispatch_gets_fresh_walls():
    """Missions of one, two and three legs inside a box of walls: a re-dispatched robot's next p carries the new route's vertices and walls found from where it stands."""
    from mpc_trajectory_generator_amd.trajectory import Missions, Walls
    cfg = named_config("cfg1")
    corners = [(2.0, 2.0), (3.2, 2.0), (3.2, 3.1), (2.2, 3.1)]         # legs of about a metre: a leg ends within a few steps
    offsets = [(0.02, -0.03, 0.05), (0.0, 0.0, 0.0), (-0.04, 0.03, -0.1)]
    routes, route_of, starts, i0, legs = mission_fleet(cfg, corners, n_legs=(1, 2, 3), first=(2, 1, 0), offsets=offsets,
                                                       vertices=[(2.6, 2.5), (2.7, 2.6)])
    edges = np.array([[0.5, 1.0, 4.7, 1.0], [4.2, 0.5, 4.2, 4.6], [0.5, 4.1, 4.7, 4.1], [1.0, 4.6, 1.0, 0.5], [4.0, 1.2, 4.3, 1.5]])      # a box a metre off the legs
    walls = Walls(edges, 3, radius(cfg), 1.3, 0.2)
    host, seen, Ps = run_pair(cfg, routes, route_of, starts, i0, None, walls, 90, until=lambda h: h.n_active > 0, retire=True,
                              missions=Missions(legs))
    assert host.n_active == 0 and (host.leg_at[2] >= 0).all()
    seen = np.stack(seen)
    assert (seen >= 0).any() and len({tuple(r) for r in seen[:, 2].tolist()}) > 1       # robot 2's walls change along its three legs
    at = 20 + cfg.N_hor
    assert all(np.array_equal(P[2, at:at + 6], [2.6, 2.5, routes[0].radius, 2.7, 2.6, routes[0].radius]) for P in Ps[:host.retired_at[2]])


def test_plant_walls_follow_the_measured_view():
    cfg = named_config("cfg1")
    host, seen, _ = run_pair(cfg, *fleet24(cfg), None, walls_of(cfg, rng_=3.0), 4, plant=PLANT)
    assert (np.stack(seen) >= 0).any() and not np.array_equal(host.measured(), host.state)


def test_nan_pose():
    """One robot with a NaN x: it gets no wall, every one of its entries is -1 and its parameter vector is the mirror's with NaN = NaN;
    every other robot keeps the mirror's bits.  (What the solve makes of a NaN is tests/test_gpu_parity.py's subject: the NaN robot's U,
    Y and status are not compared, as in tests/test_gpu_loop_shapes.py.)"""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = nan_fleet(cfg)
    walls = walls_of(cfg, rng_=3.0)
    o = oracle_for(cfg)
    keep = np.arange(len(starts)) != NAN_ROBOT
    s = BatchSolver(cfg, max_batch=16)
    dev = None
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=3, idx0=i0, route_of=route_of, walls=walls)
        host = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, walls=walls)
        for k in range(3):
            dev.step()
            P, st = host.step(o.warm_solve())
            Pd, Ud, Yd = dev.params()
            state, last_u, idx, done, std = dev.read()
            pairs = [("P", Pd, P), ("U", Ud, host.U), ("Y", Yd, host.Y), ("state", state, host.state), ("last_u", last_u, host.last_u),
                     ("done", done, host.done)] + [(f, std[f], st[f]) for f in ("num_inner_iterations", "exit_status")]
            bad = [n for n, x, y in pairs if not np.array_equal(x[keep], y[keep])]
            assert not bad, f"step {k}: {bad}"
            assert np.array_equal(idx, host.idx), f"step {k}"
            assert np.isnan(Pd[NAN_ROBOT, 0]) and np.array_equal(Pd[NAN_ROBOT], P[NAN_ROBOT], equal_nan=True), f"step {k}"
            assert not walls_differing(dev, host), f"step {k}"
            edge, stage = dev.walls()
            assert (edge[NAN_ROBOT] == -1).all() and (stage[NAN_ROBOT] == -1).all() and (edge[keep] >= 0).any(), f"step {k}"
        T, Th = dev.trajectory(), np.stack(host.traj)
        assert T.shape == Th.shape and np.array_equal(T[:, keep], Th[:, keep])
    finally:
        if dev is not None:
            dev.close()
        s.close()


def test_without_walls_the_loop_is_the_plain_one():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg4")
    routes, route_of, starts, i0 = fleet24(cfg)
    dyn = fleet_ellipses(routes, route_of, i0, 2, 9)
    s1, s2 = BatchSolver(cfg, max_batch=32), BatchSolver(cfg, max_batch=32)
    try:
        a = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of, walls=None)
        b = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of)
        for k in range(3):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
        assert s1.lib.nmpc_loop_walls(a._l, None, None) == -3 and b"no walls" in s1.lib.nmpc_last_error(s1._h)
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_walls_arguments_validated():
    """Every rejected call returns NMPC_ERR_BAD_ARG with the function's name in the message and changes nothing: the loop then steps
    exactly like one that never had the call.  A valid call is accepted once, and only before the first step."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    n, steps = 8, 2
    routes, route_of, starts, i0 = fleet24(cfg, n)
    nv = [len(r.vertices) for r in routes]
    assert max(nv) == 7 and cfg.Nobs == 10
    edges = np.ascontiguousarray(scene_map(cfg)[0])
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    lib = s1.lib
    inf, nan = float("inf"), float("nan")
    nan_, inf_ = edges.copy(), edges.copy()
    nan_[3, 2], inf_[25, 0] = nan, -inf

    def call(loop, E=len(edges), tab=edges, M=3, rc_=0.5, rng_=2.0, sp=0.0):
        rc = lib.nmpc_loop_set_walls(loop._l, E, _lib.as_dp(tab), M, rc_, rng_, sp)
        return rc, lib.nmpc_last_error(loop.solver._h).decode()

    try:
        a = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        b = DeviceRecedingHorizon(s2, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        cases = {"edge NULL": dict(tab=None), "n_edge = 0": dict(E=0), "n_edge > 1024": dict(E=1025), "a NaN coordinate": dict(tab=nan_),
                 "an infinite coordinate": dict(tab=inf_), "M = 0": dict(M=0), "M > Nobs": dict(M=11), "a route of 7 vertices": dict(M=4),
                 "radius = 0": dict(rc_=0.0), "radius negative": dict(rc_=-1.0), "radius infinite": dict(rc_=inf), "radius NaN": dict(rc_=nan),
                 "range = 0": dict(rng_=0.0), "range negative": dict(rng_=-1.0), "range infinite": dict(rng_=inf), "range NaN": dict(rng_=nan),
                 "spacing negative": dict(sp=-0.1), "spacing infinite": dict(sp=inf), "spacing NaN": dict(sp=nan)}
        for what, kw in cases.items():
            rc, msg = call(a, **kw)
            assert rc == -3 and "nmpc_loop_set_walls" in msg, what
        assert f"route {nv.index(7)}" in call(a, M=4)[1]
        assert lib.nmpc_loop_set_walls(None, len(edges), _lib.as_dp(edges), 3, 0.5, 2.0, 0.0) == -3
        for k in range(steps):                         # still the loop without walls
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
        rc, msg = call(a)
        assert rc == -3 and "step" in msg              # after a step
        assert lib.nmpc_loop_walls(a._l, None, None) == -3 and b"no walls" in lib.nmpc_last_error(s1._h)
        a.close()
        b.close()
        c = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=0, idx0=i0, route_of=route_of)
        assert call(c)[0] == 0
        rc, msg = call(c)
        assert rc == -3 and "already" in msg           # a second call
        assert lib.nmpc_loop_walls(c._l, None, None) == -3 and b"first step" in lib.nmpc_last_error(s1._h)
        c.step()
        we, ws = np.empty((n, 3), dtype=np.int32), np.empty((n, 3), dtype=np.int32)
        assert lib.nmpc_loop_walls(c._l, _lib.as_i32p(we), None) == 0 and lib.nmpc_loop_walls(c._l, None, _lib.as_i32p(ws)) == 0
        assert ((we >= 0) == (ws >= 0)).all() and (we < len(edges)).all() and (ws < cfg.N_hor).all()
        c.close()
    finally:
        s1.close()
        s2.close()
