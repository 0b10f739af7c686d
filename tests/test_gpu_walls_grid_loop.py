"""GPU: the on-device loop with walls found through a grid (nmpc_loop_set_walls_grid, nmpc_loop_wall_grid;
``nmpc_loop_walls_grid_kernel``) against its host mirror ``FleetRecedingHorizon(..., walls=Walls(..., cell=H))``,
whose results are the all-edges rule's (tests/test_walls_grid_mirror.py, tests/test_walls_mirror.py): parameter vectors, controls,
multipliers, states, reference indices, solver counters and trajectories, the walls' edges and stages and the number of edges each robot
looked at must agree bit for bit, step after step, and the grid read out once must be ``trajectory.wall_grid``'s."""
import dataclasses

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config
from mpc_trajectory_generator_amd.workloads import (clearance_differing, crowd_ellipses, fleet_ellipses, map_clearance_differing, mission_fleet,
                                                    plant_differing, staggered_fleet, step_differing, trajectory_differing, wall_grid_differing,
                                                    walls_differing)
from test_loop_shapes_mirror import CASES as SHAPES
from test_walls_mirror import NAN_ROBOT, PLANT, fleet24, nan_fleet, radius, retiring_until, scene_map, walls_of

pytestmark = pytest.mark.gpu


def grid_walls(cfg, cell, **kw):
    return dataclasses.replace(walls_of(cfg, **kw), cell=cell)


def run_pair(cfg, routes, route_of, starts, i0, dyn, walls, steps, until=None, sinus_object=False, **kw):
    """Step a device loop and its mirror ``steps`` times (or while ``until(host)`` says so, ``steps`` at the most), comparing
    everything at every step -> (the mirror, per step the edges chosen, per step the device's parameter vectors, per step looked)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    assert walls.cell is not None
    o = oracle_for(cfg)
    seen, Ps, looked = [], [], []
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
            if k == 0:
                bad = wall_grid_differing(dev, host)                # the grid, once
                assert not bad, f"step {k}: {bad}"
            got = dev.wall_grid()[3]
            assert got.dtype == np.int32 and np.array_equal(got, host.wall_looked), f"step {k}: looked {got.tolist()} not {host.wall_looked.tolist()}"
            if kw.get("monitor") is not None:
                assert not clearance_differing(dev, host), f"step {k}"
            if kw.get("map_monitor") is not None:
                assert not map_clearance_differing(dev, host), f"step {k}"
            if kw.get("plant") is not None:
                assert not plant_differing(dev, host), f"step {k}"
            seen.append(host.wall_edge.copy())
            Ps.append(Pd)
            looked.append(host.wall_looked.copy())
        assert not trajectory_differing(dev, host, host.steps)
    finally:
        if dev is not None:                    # before its solver: a loop must not outlive the handle it was made on
            dev.close()
        s.close()
    return host, seen, Ps, looked


def test_scene_map_windows_of_one_cell():
    """26 edges, cell 1 m, range 2 m: most lanes hold no edge; some robot looks at fewer edges than the map has, and nobody with a wall
    looked at none.  With a cell of 8 m some robot's window is a single cell."""
    cfg = named_config("cfg1")
    host, seen, _, looked = run_pair(cfg, *fleet24(cfg), None, grid_walls(cfg, 1.0), 4)
    assert set((seen[1] >= 0).sum(axis=1).tolist()) == {0, 1, 2, 3}
    for e, n in zip(seen, looked):
        assert (n < 26).any() and (n[(e >= 0).any(axis=1)] > 0).all()
    host, seen, _, looked = run_pair(cfg, *fleet24(cfg), None, grid_walls(cfg, 8.0), 2)
    pred = host.predict()
    one = [b for b in range(len(pred)) if (lambda w: w[0] == w[1] and w[2] == w[3])(host.wall_grid.window(pred[b], 2.0))]
    assert one and host.wall_grid.nx * host.wall_grid.ny > 1


def test_cut_in_four_with_spacing_and_both_monitors():
    from mpc_trajectory_generator_amd.trajectory import MapMonitor, Monitor
    cfg = named_config("cfg1")
    host, seen, _, _ = run_pair(cfg, *fleet24(cfg), None, grid_walls(cfg, 0.5, pieces=4, spacing=1.0), 4, monitor=Monitor(),
                                map_monitor=MapMonitor(*scene_map(cfg, 4)))
    assert (np.stack(seen) >= 64).any() and np.isfinite(host.clearance["circle"]).all()


def test_1040_edges_beyond_the_all_edges_limit():
    """40 pieces: 1040 edges, which nmpc_loop_set_walls refuses.  No robot measures the whole map."""
    cfg = named_config("cfg1")
    walls = grid_walls(cfg, 1.0, pieces=40)
    assert len(walls.edges) == 1040
    _, seen, _, looked = run_pair(cfg, *fleet24(cfg), None, walls, 3)
    assert (np.stack(seen) >= 0).any() and np.stack(looked).max() < 1040


def test_1040_edges_all_candidates_take_the_rounds():
    """N = 40, range 1 km: every edge is a candidate of every robot and the window is the whole grid -- four times what the LDS list
    holds, so the selection runs in rounds that measure again; spacing 1 m passes many candidates over."""
    cfg = named_config("cfg2")
    assert cfg.N_hor == 40
    walls = grid_walls(cfg, 1.0, pieces=40, rng_=1e3, spacing=1.0)
    _, seen, _, looked = run_pair(cfg, *fleet24(cfg), None, walls, 3)
    assert (np.stack(looked) == 1040).all() and (np.stack(seen) >= 0).all()


@pytest.mark.parametrize("copies", [200, 300])
def test_coincident_edges_tie_by_index(copies):
    """Many copies of one short edge 5 cm from robot 0: one cell holds more than a wave's lanes, every copy has the same D, and the
    smallest indices win -- from the LDS list at 200 copies, in the rounds that measure again at 300, more than the list holds."""
    from mpc_trajectory_generator_amd.trajectory import Walls
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = fleet24(cfg)
    p = np.array(starts[0][:2]) + [0.05, 0.0]
    edges = np.concatenate([scene_map(cfg)[0], np.tile([[p[0], p[1], p[0], p[1] + 0.1]], (copies, 1))])
    walls = Walls(edges, 3, radius(cfg), 2.0, 0.0, cell=1.0)
    host, seen, _, looked = run_pair(cfg, routes, route_of, starts, i0, None, walls, 3)
    assert seen[0][0].tolist() == [26, 27, 28] and looked[0][0] >= copies
    assert (np.diff(host.wall_grid.cell_off) >= copies).any()


@pytest.mark.parametrize("cell", [1e3, 0.01])
def test_one_cell_and_the_capped_grid(cell):
    cfg = named_config("cfg1")
    host, seen, _, looked = run_pair(cfg, *fleet24(cfg), None, grid_walls(cfg, cell, pieces=4, spacing=1.0), 3)
    g = host.wall_grid
    assert (g.nx, g.ny) == ((1, 1) if cell == 1e3 else (512, 512))
    assert (np.stack(seen) >= 0).any() and ((np.stack(looked) == 104).all() if cell == 1e3 else (np.stack(looked) < 104).any())


def test_shape_n33_s7():
    """N = 33 with 7 steps taken: K = 2 scripted ellipses, four wall slots behind the route's six vertices."""
    from mpc_trajectory_generator_amd.trajectory import Walls
    c = SHAPES["n33-s7"]()
    n = len(c.starts)
    assert len(c.route.vertices) == 6 and c.cfg.Nobs == 10 and c.K == 2
    walls = Walls(scene_map(c.cfg)[0], 4, radius(c.cfg), 3.0, cell=1.0)
    _, seen, _, _ = run_pair(c.cfg, [c.route], np.zeros(n, dtype=np.int32), c.starts, c.idx0, c.dyn, walls, c.steps, sinus_object=c.sinus)
    assert (np.stack(seen) >= 0).any()


def test_beside_a_crowd_and_grid_peers():
    from mpc_trajectory_generator_amd.trajectory import Crowd, Peers
    cfg = named_config("cfg4")
    routes, route_of, starts, i0 = fleet24(cfg)
    dyn = fleet_ellipses(routes, route_of, i0, 1, 9)
    crowd = Crowd(crowd_ellipses(cfg, 11, 70, 23), 1, 1e3)
    peers = Peers(slots=1, rx=0.37, ry=0.53, range=1e3, cell=1.0)
    host, seen, _, _ = run_pair(cfg, routes, route_of, starts, i0, dyn, grid_walls(cfg, 1.0, pieces=4, spacing=1.0), 3, crowd=crowd, peers=peers)
    assert (np.stack(seen) >= 0).any() and (host.crowd_seen >= 0).all() and (host.peer_index >= 0).all()


def test_retiring_fleet():
    """A retired robot keeps p, its record and its looked; steps with nobody active launch nothing."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg, back=(2, 5, 9))
    host, seen, Ps, looked = run_pair(cfg, routes, route_of, starts, i0, None, grid_walls(cfg, 1.0, rng_=3.0, scene=1), 45, until=retiring_until(),
                                      retire=True)
    at = host.retired_at
    assert host.n_active == 0 and len(set(at.tolist())) > 2 and host.steps == at.max() + 2
    assert np.array_equal(Ps[-1], Ps[-3]) and np.array_equal(seen[-1], seen[-3]) and np.array_equal(looked[-1], looked[-3])
    first = int(np.argmin(at))
    assert at[first] < at.max() and all(np.array_equal(P[first], Ps[at[first] - 1][first]) for P in Ps[at[first]:])


def test_missions_redispatch_gets_fresh_walls():
    from mpc_trajectory_generator_amd.trajectory import Missions, Walls
    cfg = named_config("cfg1")
    corners = [(2.0, 2.0), (3.2, 2.0), (3.2, 3.1), (2.2, 3.1)]
    offsets = [(0.02, -0.03, 0.05), (0.0, 0.0, 0.0), (-0.04, 0.03, -0.1)]
    routes, route_of, starts, i0, legs = mission_fleet(cfg, corners, n_legs=(1, 2, 3), first=(2, 1, 0), offsets=offsets,
                                                       vertices=[(2.6, 2.5), (2.7, 2.6)])
    edges = np.array([[0.5, 1.0, 4.7, 1.0], [4.2, 0.5, 4.2, 4.6], [0.5, 4.1, 4.7, 4.1], [1.0, 4.6, 1.0, 0.5], [4.0, 1.2, 4.3, 1.5]])
    walls = Walls(edges, 3, radius(cfg), 1.3, 0.2, cell=0.7)
    host, seen, Ps, _ = run_pair(cfg, routes, route_of, starts, i0, None, walls, 90, until=lambda h: h.n_active > 0, retire=True,
                                 missions=Missions(legs))
    assert host.n_active == 0 and (host.leg_at[2] >= 0).all()
    seen = np.stack(seen)
    assert (seen >= 0).any() and len({tuple(r) for r in seen[:, 2].tolist()}) > 1


def test_plant_walls_follow_the_measured_view():
    cfg = named_config("cfg1")
    host, seen, _, _ = run_pair(cfg, *fleet24(cfg), None, grid_walls(cfg, 1.0, rng_=3.0), 4, plant=PLANT)
    assert (np.stack(seen) >= 0).any() and not np.array_equal(host.measured(), host.state)


def test_nan_pose():
    """One robot with a NaN x: it looks at nothing, every one of its entries is -1 and its parameter vector is the mirror's with NaN =
    NaN; every other robot keeps the mirror's bits (the NaN robot's U, Y and status are not compared, as in tests/test_gpu_walls_loop.py)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = nan_fleet(cfg)
    walls = grid_walls(cfg, 1.0, rng_=3.0)
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
            assert not walls_differing(dev, host) and not wall_grid_differing(dev, host), f"step {k}"
            edge, stage = dev.walls()
            looked = dev.wall_grid()[3]
            assert (edge[NAN_ROBOT] == -1).all() and (stage[NAN_ROBOT] == -1).all() and looked[NAN_ROBOT] == 0, f"step {k}"
            assert (edge[keep] >= 0).any() and (looked[keep] > 0).any(), f"step {k}"
    finally:
        if dev is not None:
            dev.close()
        s.close()


def test_without_the_call_the_loop_is_the_plain_one():
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
        assert s1.lib.nmpc_loop_wall_grid(a._l, None, None, None, None) == -3 and b"no walls grid" in s1.lib.nmpc_last_error(s1._h)
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_walls_grid_arguments_validated():
    """Every rejected call returns NMPC_ERR_BAD_ARG with the function's name in the message and changes nothing: the loop then steps
    exactly like one that never had the call.  Either setter after the other is refused; the grid's reader refuses a loop without the grid
    and ``looked`` before the first step."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    n, steps = 8, 2
    routes, route_of, starts, i0 = fleet24(cfg, n)
    nv = [len(r.vertices) for r in routes]
    assert max(nv) == 7 and cfg.Nobs == 10
    edges = np.ascontiguousarray(scene_map(cfg)[0])
    diag = np.ascontiguousarray(np.tile([[0.0, 0.0, 100.0, 100.0]], (40, 1)))      # 40 x 512 x 512 filings at a cell of 1 cm
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    lib = s1.lib
    inf, nan = float("inf"), float("nan")
    nan_, inf_ = edges.copy(), edges.copy()
    nan_[3, 2], inf_[25, 0] = nan, -inf

    def call(loop, E=len(edges), tab=edges, M=3, rc_=0.5, rng_=2.0, sp=0.0, cell=1.0):
        rc = lib.nmpc_loop_set_walls_grid(loop._l, E, _lib.as_dp(tab), M, rc_, rng_, sp, cell)
        return rc, lib.nmpc_last_error(loop.solver._h).decode()

    def plain(loop):
        rc = lib.nmpc_loop_set_walls(loop._l, len(edges), _lib.as_dp(edges), 3, 0.5, 2.0, 0.0)
        return rc, lib.nmpc_last_error(loop.solver._h).decode()

    try:
        a = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        b = DeviceRecedingHorizon(s2, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        cases = {"edge NULL": dict(tab=None), "n_edge = 0": dict(E=0), "n_edge > 1048576": dict(E=1048577), "a NaN coordinate": dict(tab=nan_),
                 "an infinite coordinate": dict(tab=inf_), "M = 0": dict(M=0), "M > Nobs": dict(M=11), "a route of 7 vertices": dict(M=4),
                 "radius = 0": dict(rc_=0.0), "radius negative": dict(rc_=-1.0), "radius infinite": dict(rc_=inf), "radius NaN": dict(rc_=nan),
                 "range = 0": dict(rng_=0.0), "range negative": dict(rng_=-1.0), "range infinite": dict(rng_=inf), "range NaN": dict(rng_=nan),
                 "spacing negative": dict(sp=-0.1), "spacing infinite": dict(sp=inf), "spacing NaN": dict(sp=nan),
                 "cell = 0": dict(cell=0.0), "cell negative": dict(cell=-1.0), "cell infinite": dict(cell=inf), "cell NaN": dict(cell=nan),
                 "too many filings": dict(E=len(diag), tab=diag, cell=0.01)}
        for what, kw in cases.items():
            rc, msg = call(a, **kw)
            assert rc == -3 and "nmpc_loop_set_walls_grid" in msg, what
        assert f"route {nv.index(7)}" in call(a, M=4)[1]
        assert "larger cell or shorter edges" in call(a, E=len(diag), tab=diag, cell=0.01)[1]
        assert lib.nmpc_loop_set_walls_grid(None, len(edges), _lib.as_dp(edges), 3, 0.5, 2.0, 0.0, 1.0) == -3
        for k in range(steps):                         # still the loop without walls
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
        rc, msg = call(a)
        assert rc == -3 and "step" in msg              # after a step
        assert lib.nmpc_loop_wall_grid(a._l, None, None, None, None) == -3 and b"no walls grid" in lib.nmpc_last_error(s1._h)
        a.close()
        b.close()
        c = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=0, idx0=i0, route_of=route_of)
        assert call(c)[0] == 0
        rc, msg = call(c)
        assert rc == -3 and "already" in msg           # a second call
        rc, msg = plain(c)
        assert rc == -3 and "nmpc_loop_set_walls:" in msg and "already" in msg      # the all-edges setter after the grid's
        looked = np.empty(n, dtype=np.int32)
        hdr = np.zeros((), dtype=_lib.WALL_GRID_DTYPE)
        assert lib.nmpc_loop_wall_grid(c._l, hdr.ctypes.data, None, None, None) == 0 and hdr["entries"] >= len(edges)      # the grid is there at once
        assert lib.nmpc_loop_wall_grid(c._l, None, None, None, _lib.as_i32p(looked)) == -3 and b"first step" in lib.nmpc_last_error(s1._h)
        c.step()
        assert lib.nmpc_loop_wall_grid(c._l, None, None, None, _lib.as_i32p(looked)) == 0 and (looked >= 0).all() and (looked <= len(edges)).all()
        we = np.empty((n, 3), dtype=np.int32)
        assert lib.nmpc_loop_walls(c._l, _lib.as_i32p(we), None) == 0 and (we < len(edges)).all()      # nmpc_loop_walls reads either setter's
        c.close()
        d = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=0, idx0=i0, route_of=route_of)
        assert plain(d)[0] == 0
        rc, msg = call(d)
        assert rc == -3 and "nmpc_loop_set_walls_grid" in msg and "already" in msg      # the grid's setter after the all-edges one
        assert lib.nmpc_loop_wall_grid(d._l, None, None, None, None) == -3 and b"no walls grid" in lib.nmpc_last_error(s1._h)
        d.close()
    finally:
        s1.close()
        s2.close()
