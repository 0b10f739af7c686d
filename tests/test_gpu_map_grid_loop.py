"""GPU: the map monitor through a grid (nmpc_loop_set_map_monitor_grid, nmpc_loop_map_grid, ``nmpc_loop_map_grid_kernel``; DESIGN.md
section 5.9) against its host mirror ``FleetRecedingHorizon(..., map_monitor=MapMonitor(..., cell=H, range=R))`` -- itself held to the
all-edges rule by tests/test_map_grid_mirror.py -- driven by the oracle and given the kernels' sin / cos.  After EVERY step the loop's
arrays (``step_differing``), the seven fields of every robot's record (``map_clearance_differing``) and the grid with ``looked``
(``map_grid_differing``) must be the mirror's; the trajectories are compared at the end.  The fleets are those of
tests/test_gpu_map_monitor_loop.py.

What each case makes the kernel do:

* ``scene11``: scene 11's own map, 26 edges, cell 1 m and range 2 m: windows of a few cells, most edges not looked at.
* ``squares1160``: 17 x 17 squares and a boundary, 1160 edges and 290 polygons, the smallest such lattice past the all-edges limit: hits
  against obstacles and against the boundary; a ray to the right meets up to 34 obstacle edges.
* ``pieces64``: scene 11 cut into 64 pieces per edge, 1664 edges: the filings of a long polygon share cells, and a ray meets several
  edges of ONE polygon, whose parity is taken over all of them.
* ``fence``: 300 thin rectangles in a row (tests/test_map_grid_mirror.py), robot 0 started inside the eleventh: its ray meets 579
  obstacle edges, more than the kernel's list of 512 holds, and the exact rounds name rectangle 10 and nothing else.
* ``thin-wall``: a 0.02 m thick obstacle between two of robot 0's rows: a hit by the crossing test alone.
* ``one-cell``: a cell larger than the map: every row looks at every edge; ``capped``: a cell of 1 cm, 512 cells per axis.
* ``cfg2-s3``: three rows per step, each with its own window; ``staggered-peers-retire``: through the raw setters, the map grid first;
  ``missions``: records across a re-dispatch; ``one-robot``: B = 1; ``B131``: 131 robots.
* ``triangles349525``: 1048575 edges in 349525 polygons, the most a map can have: 349524 small triangles on a lattice inside a large one,
  robot 0 started inside the last obstacle, polygon 349523; the boundary's long diagonal is filed in every cell."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, harness, named_config
from mpc_trajectory_generator_amd.workloads import (clearance_differing, map_clearance_differing, map_grid_differing, step_differing, subdivided_map,
                                                    trajectory_differing)
from test_gpu_map_monitor_loop import _fleet as plain_fleet, scene_struct
from test_map_grid_mirror import fence_map, lattice_map
from test_map_monitor_mirror import BAD_MAPS, _square, scene_map
from test_monitor_mirror import near_goal_cfg4_fleet

pytestmark = pytest.mark.gpu


def with_cell(m, cell, range_):
    from mpc_trajectory_generator_amd.trajectory import MapMonitor
    return MapMonitor(m.edges, m.poly_off, cell=cell, range=range_)


def driven_rows(f, steps):
    """-> the trajectory [steps * s + 1, B, 3] of the fleet ``f`` without any stage, by the host mirror and the oracle"""
    from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon
    o = oracle_for(f["cfg"])
    host = FleetRecedingHorizon(f["routes"], f["route_of"], f["starts"], f["dyn"], sincos=o.sincos_array, idx0=f["idx0"])
    for _ in range(steps):
        host.step(o.warm_solve(threads=16))
    return np.stack(host.traj)


def thin_wall_map(T, row):
    """A rectangle 0.02 m thick and 1 m long across robot 0's way from row ``row`` - 1 to row ``row`` of ``T``, in a room around everybody"""
    from mpc_trajectory_generator_amd.trajectory import MapMonitor
    a, p = T[row - 1, 0, :2], T[row, 0, :2]
    d = (p - a) / np.hypot(*(p - a))
    n, mid = np.array([-d[1], d[0]]), 0.5 * (a + p)
    c = [mid - 0.01 * d - 0.5 * n, mid + 0.01 * d - 0.5 * n, mid + 0.01 * d + 0.5 * n, mid - 0.01 * d + 0.5 * n]
    wall = [[*c[i], *c[(i + 1) % 4]] for i in range(4)]
    lo, hi = T[:, :, :2].reshape(-1, 2).min(axis=0) - 5, T[:, :, :2].reshape(-1, 2).max(axis=0) + 5
    return MapMonitor(np.array(wall + _square(lo[0], lo[1], hi[0], hi[1]), dtype=np.float64), [0, 4, 8])


THIN_WALL_ROW = 3


def triangles_map(n=349524, cols=591):
    """``n`` right triangles with legs of 0.15 m on a 0.25 m lattice of ``cols`` columns, row after row, inside the triangle (-10, -10),
    (400, -10), (-10, 400) -> (edges [3 n + 3, 4], poly_off); triangle k has its right angle at (0.25 (k % cols), 0.25 (k // cols))"""
    k = np.arange(n)
    x0, y0 = 0.25 * (k % cols), 0.25 * (k // cols)
    a, b, c = np.stack([x0, y0], 1), np.stack([x0 + 0.15, y0], 1), np.stack([x0, y0 + 0.15], 1)
    tri = np.stack([np.concatenate([a, b], 1), np.concatenate([b, c], 1), np.concatenate([c, a], 1)], axis=1).reshape(-1, 4)
    outer = np.array([[-10, -10, 400, -10], [400, -10, -10, 400], [-10, 400, -10, -10]], dtype=np.float64)
    return np.concatenate([tri, outer]), np.arange(0, 3 * n + 4, 3, dtype=np.int32)


def _fleet(which):
    """-> the fleet of tests/test_gpu_map_monitor_loop.py that the case runs, its ``map`` a ``MapMonitor`` with a cell"""
    from mpc_trajectory_generator_amd.trajectory import MapMonitor
    if which in ("scene11", "one-cell", "capped"):
        f = plain_fleet("cfg1-three-routes")
        cell = {"scene11": 1.0, "one-cell": 1e3, "capped": 0.01}[which]
        return {**f, "map": with_cell(f["map"], cell, 2.0), "steps": 8 if which == "scene11" else 3}
    if which in ("squares1160", "pieces64", "fence", "thin-wall", "triangles349525"):
        f = plain_fleet("triangle")
        if which == "squares1160":
            edges, off = lattice_map(17, 17)
            assert len(edges) == 1160 and len(off) - 1 == 290
            edges = edges + np.tile(f["starts"][0, :2] - (32.5, 32.5), 2)   # robot 0 starts in the middle of the last square
            m = MapMonitor(edges, off, cell=1.0, range=2.0)
        elif which == "pieces64":
            plain = scene_map(f["cfg"], 11)
            m = MapMonitor(*subdivided_map(plain.edges, plain.poly_off, 64), cell=1.0, range=2.0)
            assert len(m.edges) == 1664
        elif which == "fence":
            edges, off = fence_map(300)
            edges = edges + np.tile(f["starts"][0, :2] - (1.02, 0.5), 2)    # robot 0 starts in the middle of rectangle 10
            m = MapMonitor(edges, off, cell=1.0, range=2.0)
        elif which == "triangles349525":
            edges, off = triangles_map()
            assert len(edges) == 1048575 and len(off) - 1 == 349525
            last = edges[-6, :2] + 0.04                                     # a point inside the last obstacle
            m = MapMonitor(edges + np.tile(f["starts"][0, :2] - last, 2), off, cell=1.0, range=2.0)
        else:
            m = with_cell(thin_wall_map(driven_rows(f, 4), THIN_WALL_ROW), 1.0, 2.0)
        return {**f, "map": m, "steps": 2 if which == "triangles349525" else 4}
    name = {"cfg2-s3": "cfg2-s3", "staggered-peers-retire": "staggered-peers-retire-setters-map-first", "missions": "missions", "one-robot": "one-robot",
            "B131": "B131"}[which]
    f = plain_fleet(name)
    return {**f, "map": with_cell(f["map"], 1.0, 2.0)}


FLEETS = ["scene11", "squares1160", "pieces64", "fence", "thin-wall", "one-cell", "capped", "cfg2-s3", "staggered-peers-retire", "missions",
          "one-robot", "B131", "triangles349525"]


def set_map_grid(lib, dev, m, keep):
    sc = scene_struct(m, keep)
    return lib.nmpc_loop_set_map_monitor_grid(dev._l, C.byref(sc), float(m.range), float(m.cell))


def _bare_loop_then_setters(s, f, monitor):
    """-> the fleet's device loop, created with no stage and given the map monitor's grid, the clearance monitor, retirement and peers
    in that order through the C ABI"""
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    dev = DeviceRecedingHorizon(s, f["routes"], f["starts"], f["dyn"], max_steps=f["steps"], route_of=f["route_of"], idx0=f["idx0"],
                                sinus_object=f["sinus"])
    lib, peers = s.lib, f["peers"]
    mon_groups, peer_groups = (np.ascontiguousarray(g, dtype=np.int32) for g in (monitor.group_of, peers.group_of))
    assert set_map_grid(lib, dev, f["map"], []) == 0
    assert lib.nmpc_loop_set_monitor(dev._l, _lib.as_i32p(mon_groups)) == 0
    assert lib.nmpc_loop_set_retire(dev._l, 1) == 0
    assert lib.nmpc_loop_set_peers(dev._l, _lib.as_i32p(peer_groups), peers.slots, peers.rx, peers.ry, peers.range) == 0
    return dev


@pytest.mark.parametrize("which", FLEETS)
def test_map_grid_loop_equals_host_mirror(which):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon, Missions, Monitor, no_map_clearance
    f = _fleet(which)
    cfg, B, s_taken, m = f["cfg"], len(f["starts"]), f["cfg"].num_steps_taken, f["map"]
    E, n_poly = len(m.edges), len(m.poly_off) - 1
    o = oracle_for(cfg)
    monitor = Monitor(group_of=f["groups"]) if f["peers"] is not None else None
    common = dict(idx0=f["idx0"], sinus_object=f["sinus"], peers=f["peers"], retire=f["retire"], monitor=monitor, map_monitor=m,
                  missions=None if f["legs"] is None else Missions(f["legs"]))
    s = BatchSolver(cfg, max_batch=B)
    try:
        if f["raw_setters"]:
            dev = _bare_loop_then_setters(s, f, monitor)
        else:
            dev = DeviceRecedingHorizon(s, f["routes"], f["starts"], f["dyn"], max_steps=f["steps"], route_of=f["route_of"], **common)
        host = FleetRecedingHorizon(f["routes"], f["route_of"], f["starts"], f["dyn"], sincos=o.sincos_array, **common)
        assert not map_clearance_differing(dev, no_map_clearance(B))           # before the first step: the initial record
        moved, looked, redispatched_at = 0, [], {}
        for k in range(f["steps"]):
            before = host.map_clearance.copy()
            leg = None if f["legs"] is None else host.leg.copy()
            bad = step_differing(dev, host, o.warm_solve(threads=16))[0] + map_clearance_differing(dev, host) + map_grid_differing(dev, host)
            if monitor is not None:
                bad += clearance_differing(dev, host)
            assert not bad, f"step {k}: {bad}"
            moved += int((host.map_clearance != before).sum())
            looked.append(host.map_looked.copy())
            if leg is not None:
                for b in np.nonzero(host.leg != leg)[0]:
                    redispatched_at.setdefault(int(b), k + 1)
        assert not trajectory_differing(dev, host, f["steps"])
        rec, rows = host.map_clearance, np.stack(host.traj)
        dev.close()
    finally:
        s.close()
    looked = np.array(looked)
    print(which, E, "edges; records changed", moved, "times; looked per robot and step: mean", float(looked.mean()), "max", int(looked.max()),
          "; robots with hits", int((rec["hits"] > 0).sum()), "polygons first hit", sorted(set(rec["hit_poly"][rec["hits"] > 0].tolist())))
    assert moved > 0 and (looked >= 0).all() and (looked <= s_taken * E).all()
    if which == "scene11":
        assert looked.mean() < E / 2 and np.isfinite(rec["wall2"]).any()
    if which == "one-cell":
        assert (looked == s_taken * E).all()
    if which == "capped":
        assert max(m.grid.nx, m.grid.ny) == 512
    if which == "squares1160":
        assert rec["hits"].sum() > 0 and (rec["hit_poly"] == n_poly - 1).any() and ((rec["hit_poly"] >= 0) & (rec["hit_poly"] < n_poly - 1)).any()
        assert rec["hit_poly"][0] == n_poly - 2 and rec["hit_row"][0] == 1
    if which == "fence":
        assert rec["hit_poly"][0] == 10 and rec["hit_row"][0] == 1
        e = np.asarray(m.edges)[:-4]
        met = [int((((e[:, 1] > y) != (e[:, 3] > y)) & (e[:, 0] > x)).sum()) for x, y in rows[1:, 0, :2]]
        assert min(met) > 512, f"robot 0's ray meets {met} obstacle edges: the kernel's list holds them"
    if which == "triangles349525":
        assert (rec["hit_poly"][0], rec["hit_row"][0]) == (349523, 1) and looked.max() < 5000
    if which == "thin-wall":
        # the wall is 1 cm from the middle between the two rows, which are further apart than its thickness: no pose stands in it
        assert (rec["hits"][0], rec["hit_row"][0], rec["hit_poly"][0]) == (1, THIN_WALL_ROW, 0)
    if which == "missions":
        assert redispatched_at, "nobody was re-dispatched"
        assert any(rec["wall_row"][b] > at * s_taken for b, at in redispatched_at.items()), "no record moved after a re-dispatch"


def test_grid_and_all_edges_loops_keep_the_same_records():
    """Scene 11's fleet as two device loops side by side, ``MapMonitor(edges, off)`` and ``MapMonitor(edges, off, cell=1.0, range=1e3)``:
    the records are equal bit for bit at every step."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    f = plain_fleet("cfg1-three-routes")
    B = len(f["starts"])
    s1, s2 = BatchSolver(f["cfg"], max_batch=B), BatchSolver(f["cfg"], max_batch=B)
    try:
        a, b = (DeviceRecedingHorizon(s, f["routes"], f["starts"], None, max_steps=8, idx0=f["idx0"], route_of=f["route_of"], map_monitor=m)
                for s, m in ((s1, f["map"]), (s2, with_cell(f["map"], 1.0, 1e3))))
        for k in range(8):
            a.step()
            b.step()
            bad = map_clearance_differing(b, a.map_clearance())
            assert not bad, f"step {k}: {bad}"
        rec = a.map_clearance()
        assert np.isfinite(rec["wall2"]).all() and (rec["wall_row"] >= 1).all()
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_map_grid_loop_is_the_loop_without_it():
    """A device loop with the stage and one without it over one fleet (scripted ellipses, peers, retirement and the clearance monitor
    on): p, u, y, state, last_u, idx, done, the status counters, retired_at, the clearance records and the trajectory are equal at every
    step."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, Monitor, Peers, no_map_clearance
    cfg, routes, route_of, starts, i0, dyn = near_goal_cfg4_fleet(K=2)
    steps = 8
    peers = Peers(slots=1, rx=0.37, ry=0.53, range=5.0)
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    try:
        a, b = (DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of, peers=peers, retire=True,
                                      monitor=Monitor(group_of=route_of), map_monitor=m)
                for s, m in ((s1, with_cell(scene_map(cfg, 11), 1.0, 2.0)), (s2, None)))
        for k in range(steps):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
            sa, sb = a.read()[4], b.read()[4]
            for f in ("exit_status", "num_inner_iterations", "num_outer_iterations", "num_cost_evals", "num_grad_evals", "cost", "penalty"):
                assert np.array_equal(sa[f], sb[f]), (k, f)
            assert np.array_equal(a.active()[1], b.active()[1])
            assert not clearance_differing(a, b.clearance()), f"step {k}"
            assert np.array_equal(a.trajectory(), b.trajectory()), f"step {k}"
        assert np.isfinite(a.map_clearance()["wall2"]).any() and (a.map_grid()[3] > 0).any()
        assert not map_clearance_differing(b, no_map_clearance(len(starts)))       # without the stage: the initial record everywhere
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_map_grid_arguments_validated():
    """Everything nmpc_loop_set_map_monitor refuses, a range or a cell that is not finite and positive, too many filings, either setter
    after the other, a second call and a call after a step: NMPC_ERR_BAD_ARG with the function's name in the message and nothing changed --
    the loop still steps, a refused loop reports the initial record, the grid's reader refuses a loop without the grid and ``looked``
    before the first step, and the handle then solves a batch exactly like the oracle."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, MapMonitor, no_map_clearance
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 8, seed=2)
    good = scene_map(cfg, 11)
    s = BatchSolver(cfg, max_batch=16)
    lib = s.lib
    inf, nan = float("inf"), float("nan")
    keep = []

    def refused(loop, sc, range_=2.0, cell=1.0, fn="nmpc_loop_set_map_monitor_grid"):
        ref = None if sc is None else C.byref(sc)
        rc = lib.nmpc_loop_set_map_monitor(loop._l, ref) if fn == "nmpc_loop_set_map_monitor" else lib.nmpc_loop_set_map_monitor_grid(loop._l, ref, range_, cell)
        msg = lib.nmpc_last_error(s._h).decode()
        assert rc == -3 and msg and fn + ":" in msg, (rc, msg)
        return msg

    def raw(edges, off, E=None, n_poly=None):
        edges, off = np.ascontiguousarray(edges, dtype=np.float64), np.ascontiguousarray(off, dtype=np.int32)
        keep.extend([edges, off])
        return _lib.NmpcScene(0, len(edges) if E is None else E, len(off) - 1 if n_poly is None else n_poly, 0, None, _lib.as_dp(edges), _lib.as_i32p(off))

    try:
        ok = scene_struct(good, keep)
        assert lib.nmpc_loop_set_map_monitor_grid(None, C.byref(ok), 2.0, 1.0) == -3 and lib.nmpc_loop_map_grid(None, None, None, None, None) == -3
        a = DeviceRecedingHorizon(s, routes, starts, None, max_steps=4, idx0=i0, route_of=route_of)
        assert "NULL" in refused(a, None)
        for what, (edges, off) in BAD_MAPS.items():
            if what != "1025 edges":               # (this setter takes them)
                refused(a, raw(edges, off))
        refused(a, raw(good.edges, good.poly_off, n_poly=0))
        refused(a, raw(good.edges, good.poly_off, E=2))
        assert "1048576" in refused(a, raw(good.edges, good.poly_off, E=1048577))
        for bad in (0.0, -1.0, inf, nan):
            assert "finite and positive" in refused(a, ok, range_=bad)
            assert "finite and positive" in refused(a, ok, cell=bad)
        diag = raw(np.tile([[0.0, 0.0, 100.0, 100.0]], (42, 1)), [0, 42])      # 42 x 512 x 512 filings at a cell of 1 cm
        assert "larger cell or shorter edges" in refused(a, diag, cell=0.01)
        assert lib.nmpc_loop_map_grid(a._l, None, None, None, None) == -3 and b"no map monitor grid" in lib.nmpc_last_error(s._h)
        a.step()
        assert "step" in refused(a, ok)
        a.step()
        assert not map_clearance_differing(a, no_map_clearance(8))
        a.close()
        b = DeviceRecedingHorizon(s, routes, starts, None, idx0=i0, route_of=route_of)             # max_steps = 0
        assert "trajectory" in refused(b, ok)
        b.close()
        with pytest.raises(ValueError):
            DeviceRecedingHorizon(s, routes, starts, None, max_steps=4, idx0=i0, route_of=route_of, map_monitor=MapMonitor(good.edges, good.poly_off, cell=0.0, range=1.0))
        c = DeviceRecedingHorizon(s, routes, starts, None, max_steps=4, idx0=i0, route_of=route_of, map_monitor=with_cell(good, 1.0, 2.0))
        assert "already" in refused(c, ok)                                                         # a second call
        assert "already" in refused(c, ok, fn="nmpc_loop_set_map_monitor")                         # the all-edges setter after the grid's
        hdr, looked = np.zeros((), dtype=_lib.WALL_GRID_DTYPE), np.empty(8, dtype=np.int32)
        assert lib.nmpc_loop_map_grid(c._l, hdr.ctypes.data, None, None, None) == 0 and hdr["entries"] >= 26      # the grid is there at once
        assert lib.nmpc_loop_map_grid(c._l, None, None, None, _lib.as_i32p(looked)) == -3 and b"first step" in lib.nmpc_last_error(s._h)
        c.step()
        c.step()
        assert lib.nmpc_loop_map_grid(c._l, None, None, None, _lib.as_i32p(looked)) == 0 and (looked > 0).all() and (looked <= 26).all()
        rec = c.map_clearance()
        assert (rec["wall_row"][np.isfinite(rec["wall2"])] >= 1).all()
        c.close()
        d = DeviceRecedingHorizon(s, routes, starts, None, max_steps=4, idx0=i0, route_of=route_of, map_monitor=good)
        assert "already" in refused(d, ok)                                                         # the grid's setter after the all-edges one
        assert lib.nmpc_loop_map_grid(d._l, None, None, None, None) == -3 and b"no map monitor grid" in lib.nmpc_last_error(s._h)
        d.close()
        P = harness.synthetic_batch(cfg, 11, 8, 77)
        u, y, st = s.solve(P)
        uo, yo, sto = oracle_for(cfg).solve_batch(P, threads=8)
        assert np.array_equal(u, uo) and np.array_equal(y, yo)
        assert np.array_equal(st["num_inner_iterations"], sto["num_inner_iterations"])
    finally:
        s.close()
