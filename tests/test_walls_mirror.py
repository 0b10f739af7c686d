"""The walls on the host (``FleetRecedingHorizon(..., walls=Walls(...))``), with the oracle solving.

The mirror's vectorised rule against a literal per-robot, per-edge, per-stage loop of the rule written here in plain floats (the robot's
Euler prediction, the wall distance stage by stage on a strict ``<``, the (D, e) sort, the walk with its spacing test and the
placement from circle slot Nobs - M on), bit for bit on p, ``wall_edge`` and ``wall_stage`` over several steps: scene 11's map of 26
edges, the same map cut in 4 and in 39, a retiring fleet, a measuring plant with the clearance monitor, a NaN pose; ties, an edge of
zero length, what ``Walls.checked`` refuses, ``workloads.subdivided_map`` and the two functions of the C ABI.

The fleets and maps built here are the ones tests/test_gpu_walls_loop.py runs on the device."""
import copy
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, MapMonitor, Monitor, Plant, Walls
from mpc_trajectory_generator_amd.workloads import staggered_fleet, subdivided_map
from test_loop_shapes_mirror import CASES as SHAPES

B = 24
NAN_ROBOT = 5
PLANT = Plant(seed=11, proc=(0.002, 0.002, 0.001), meas=(0.03, 0.03, 0.02))


def scene_map(cfg, pieces=1, scene=11):
    """-> (edges, poly_off): the scene's true walls, every edge cut into ``pieces``."""
    return subdivided_map(*frontend.map_edges(frontend.scene_planner(cfg, scene)), pieces)


def radius(cfg):
    return cfg.vehicle_width / 2 + cfg.vehicle_margin


def walls_of(cfg, pieces=1, M=3, rng_=2.0, spacing=0.0, scene=11):
    return Walls(scene_map(cfg, pieces, scene)[0], M, radius(cfg), rng_, spacing)


def fleet24(cfg, n=B):
    """-> (routes, route_of, starts, idx0): 24 robots on three planned routes of scene 11."""
    return frontend.random_fleet(cfg, 11, 3, n, seed=41)


def nan_fleet(cfg):
    """``fleet24`` with a NaN x in robot ``NAN_ROBOT``."""
    routes, route_of, starts, i0 = fleet24(cfg, 12)
    starts = np.array(starts, dtype=np.float64)
    starts[NAN_ROBOT, 0] = np.nan
    return routes, route_of, starts, i0


def circle_col(cfg, slot):
    """Where circle slot ``slot`` starts in a parameter vector."""
    return 20 + cfg.N_hor + 3 * slot


def centres(cfg, P, M):
    """-> [B, M, 3]: the last M circle slots of the parameter vectors."""
    return P[:, circle_col(cfg, cfg.Nobs - M):circle_col(cfg, cfg.Nobs)].reshape(len(P), M, 3)


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the literal rule ----
def literal_walls(cfg, wl, P, told, U, sincos, active, edge, stage):
    """Section 5.9 robot by robot, edge by edge and stage by stage in Python floats, for the active robots: P [B, n_p] as the
    assembly left it, ``told`` [B, 3] the poses the step was given, U the previous plans; ``edge`` and ``stage`` [B][M] are the records
    before the step.  -> (P overlaid, edge, stage, candidates skipped for spacing)."""
    N, s, ts, M = cfg.N_hor, cfg.num_steps_taken, cfg.ts, wl.slots
    r2, s2 = wl.range * wl.range, wl.spacing * wl.spacing
    E = [tuple(float(v) for v in row) for row in np.asarray(wl.edges)]
    P = P.copy()
    edge, stage = [list(r) for r in edge], [list(r) for r in stage]
    skipped = 0
    for b in range(len(told)):
        if not active[b]:
            continue
        x, y, th = (float(v) for v in told[b])
        pred = []
        for k in range(N):
            c = s + k if s + k < N else N - 1
            v, w = float(U[b][2 * c]), float(U[b][2 * c + 1])
            sn, cs = sincos(np.array([th]))
            x, y, th = x + ts * (v * float(cs[0])), y + ts * (v * float(sn[0])), th + ts * w
            pred.append((x, y))
        cand = []
        for e, (x1, y1, x2, y2) in enumerate(E):
            ex, ey = x2 - x1, y2 - y1
            L2 = ex * ex + ey * ey
            D, best = math.inf, None
            for k, (X, Y) in enumerate(pred):
                t = 0.0
                if L2 > 0:
                    t = ((X - x1) * ex + (Y - y1) * ey) / L2
                    if t < 0:
                        t = 0.0
                    if t > 1:
                        t = 1.0
                cx, cy = x1 + t * ex, y1 + t * ey
                dx, dy = X - cx, Y - cy
                v = dx * dx + dy * dy
                if v < D:
                    D, best = v, (k, cx, cy)
            if D < r2:
                cand.append((D, e, best))
        cand.sort(key=lambda c: (c[0], c[1]))
        taken = []
        for D, e, (k, cx, cy) in cand:
            if len(taken) == M:
                break
            if any((cx - tx) * (cx - tx) + (cy - ty) * (cy - ty) < s2 for _, _, tx, ty in taken):
                skipped += 1
                continue
            taken.append((e, k, cx, cy))
        edge[b], stage[b] = [-1] * M, [-1] * M
        for m, (e, k, cx, cy) in enumerate(taken):
            at = circle_col(cfg, cfg.Nobs - M + m)
            P[b, at], P[b, at + 1], P[b, at + 2] = cx, cy, wl.radius
            edge[b][m], stage[b][m] = e, k
    return P, edge, stage, skipped


def _twin_without_walls(fleet):
    """The same fleet at the same states and plans, without its walls; assembling it leaves ``fleet`` alone."""
    twin = copy.copy(fleet)
    twin.walls = None
    twin.dyn = fleet.dyn.copy()
    if fleet.active is not None:
        twin.P = fleet.P.copy()
    if fleet.plant is not None:
        twin._told = fleet._told.copy()
    return twin


def run_against_literal(cfg, fleet_args, wl, steps, until=None, **kw):
    """Step a mirror with walls ``steps`` times (or while ``until(fleet)`` says so), holding every step to the literal rule -> (the
    mirror, per step: the parameter vectors, the fill counts of the robots the step ran over, the candidates skipped)."""
    o = oracle_for(cfg)
    routes, route_of, starts, i0 = fleet_args
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, walls=wl, **kw)
    M, n = wl.slots, len(starts)
    edge, stage = [[-1] * M] * n, [[-1] * M] * n
    Ps, fills, skips = [], [], []
    while fleet.steps < steps and (until is None or until(fleet)):
        k = fleet.steps
        active = np.ones(n, dtype=bool) if fleet.active is None else fleet.active.copy()
        U = fleet.U.copy()
        P0 = _twin_without_walls(fleet).assemble().copy()
        assert not centres(cfg, P0, M)[active].any(), f"step {k}: the last {M} circle slots are not free"
        want, edge, stage, skipped = literal_walls(cfg, wl, P0, P0[:, 0:3], U, o.sincos_array, active, edge, stage)
        P, _ = fleet.step(o.warm_solve())
        assert same_bits(P, want), f"step {k}: columns {np.unique(np.nonzero(P != want)[1])[:10]}"
        assert fleet.wall_edge.tolist() == edge and fleet.wall_stage.tolist() == stage, f"step {k}"
        assert fleet.wall_edge.dtype == np.int32 and fleet.wall_edge.shape == (n, M) == fleet.wall_stage.shape
        got = fleet.wall_edge >= 0
        assert (centres(cfg, P, M)[..., 2][got] == wl.radius).all() and not centres(cfg, P, M)[~got].any()
        assert not (np.diff(got.astype(int), axis=1) > 0).any()            # a robot's slots fill from the first on
        Ps.append(P.copy())
        fills.append(got.sum(axis=1)[active])
        skips.append(skipped)
    return fleet, Ps, fills, skips


def test_scene_map_equals_literal_rule():
    """26 edges, three slots, range 2 m, four steps.  Robots with no, one, two and three walls in reach occur from the second step on:
    at step 0 nobody has a plan, every predicted pose is the start pose, and on this map no robot then has three edges within 2 m.  (The
    step-0 spread over all four fill counts belongs to the 104-edge map with spacing 0, where the pieces of one wall fill the slots:
    test_cut_in_four_without_spacing_spends_slots_on_one_point asserts it there.)"""
    cfg = named_config("cfg1")
    wl = walls_of(cfg)
    assert len(wl.edges) == 26
    _, _, fills, skips = run_against_literal(cfg, fleet24(cfg), wl, 4)
    assert set(fills[0].tolist()) >= {0, 1, 2}
    assert all(set(f.tolist()) == {0, 1, 2, 3} for f in fills[1:])
    assert not any(skips)                                                  # spacing 0 skips nothing


def test_cut_in_four_spacing_skips_candidates():
    """104 edges with a spacing of 1 m: the pieces of one wall compete, and some are passed over."""
    cfg = named_config("cfg1")
    wl = walls_of(cfg, pieces=4, spacing=1.0)
    assert len(wl.edges) == 104
    fleet, Ps, _, skips = run_against_literal(cfg, fleet24(cfg), wl, 4)
    assert skips[0] >= 1
    for b in np.nonzero((fleet.wall_edge >= 0).sum(axis=1) >= 2)[0]:       # the taken centres keep the spacing
        n = int((fleet.wall_edge[b] >= 0).sum())
        c = centres(cfg, Ps[-1], 3)[b, :n, :2]
        d = np.linalg.norm(c[:, None] - c[None, :], axis=2)[np.triu_indices(n, 1)]
        assert (d >= 1.0 - 1e-12).all()


def test_cut_in_four_without_spacing_spends_slots_on_one_point():
    """What ``spacing`` is for: with 0 some robot holds two centres less than 1 m apart."""
    cfg = named_config("cfg1")
    fleet, Ps, _, _ = run_against_literal(cfg, fleet24(cfg), walls_of(cfg, pieces=4), 1)
    c = centres(cfg, Ps[0], 3)
    close = [b for b in range(B) if (fleet.wall_edge[b, :2] >= 0).all() and np.linalg.norm(c[b, 0, :2] - c[b, 1, :2]) < 1.0]
    assert close
    assert set((fleet.wall_edge >= 0).sum(axis=1).tolist()) == {0, 1, 2, 3}      # step 0 on this map: every fill count occurs


def test_cut_in_39_at_the_long_horizon():
    """1014 edges, the most a lane of the device's kernel holds (16), at N = 40."""
    cfg = named_config("cfg2")
    assert cfg.N_hor == 40
    wl = walls_of(cfg, pieces=39, spacing=1.0)
    assert len(wl.edges) == 1014
    _, _, fills, skips = run_against_literal(cfg, fleet24(cfg), wl, 4)
    assert skips[0] >= 1 and max(f.max() for f in fills) == 3


def retiring_until(extra=2):
    """-> until(fleet): while somebody is active, and ``extra`` steps more."""
    left = [extra]

    def until(fleet):
        if fleet.n_active:
            return True
        left[0] -= 1
        return left[0] >= 0
    return until


def test_retiring_fleet_keeps_p_and_record():
    cfg = named_config("cfg1")
    fleet_args = staggered_fleet(cfg, back=(2, 5, 9))
    wl = walls_of(cfg, M=3, rng_=3.0, scene=1)
    fleet, Ps, _, _ = run_against_literal(cfg, fleet_args, wl, 45, until=retiring_until(), retire=True)
    at = fleet.retired_at
    assert fleet.n_active == 0 and len(set(at.tolist())) > 2 and fleet.steps == at.max() + 2
    assert same_bits(Ps[-1], Ps[-3])
    first = int(np.argmin(at))                                  # retired long before the end: its row never moved again
    assert at[first] < at.max() and all(same_bits(P[first], Ps[at[first] - 1][first]) for P in Ps[at[first]:])
    assert (fleet.wall_edge >= 0).any()


def test_plant_and_clearance_monitor_see_the_walls():
    """A measuring plant: the walls follow the measured view (the literal rule starts from p[0 .. 3)).  The clearance monitor reads p as
    the solve did: its circle record sees the wall circles."""
    cfg = named_config("cfg1")
    fleet_args = fleet24(cfg, 12)
    wl = walls_of(cfg, rng_=3.0)
    with_, _, _, _ = run_against_literal(cfg, fleet_args, wl, 4, plant=PLANT, monitor=Monitor())
    assert not np.array_equal(with_.measured()[:, :2], with_.state[:, :2])
    o = oracle_for(cfg)
    routes, route_of, starts, i0 = fleet_args
    without = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, plant=PLANT, monitor=Monitor())
    for _ in range(4):
        without.step(o.warm_solve())
    assert (with_.clearance["circle"] != without.clearance["circle"]).any()


def test_nan_pose_gets_no_wall():
    cfg = named_config("cfg1")
    fleet, _, _, _ = run_against_literal(cfg, nan_fleet(cfg), walls_of(cfg, rng_=3.0), 3)
    assert (fleet.wall_edge[NAN_ROBOT] == -1).all() and (fleet.wall_stage[NAN_ROBOT] == -1).all()
    assert (np.delete(fleet.wall_edge, NAN_ROBOT, axis=0) >= 0).any()


def test_ties_and_an_edge_of_zero_length():
    """Two coincident edges go to the smaller index first; an edge of zero length has t = 0: its centre is its first end point."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = fleet24(cfg, 12)
    edges = scene_map(cfg)[0]
    make = lambda e: FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, walls=Walls(e, 3, radius(cfg), 1e3))      # noqa: E731
    probe = make(edges)
    probe.assemble()
    near = int(probe.wall_edge[0, 0])
    point = np.array(starts[1][:2]) + np.array([0.01, 0.0])
    fleet = make(np.concatenate([edges, edges[near:near + 1], [[*point, *point]]]))
    P = fleet.assemble()
    assert fleet.wall_edge[0, :2].tolist() == [near, 26]
    assert same_bits(centres(cfg, P, 3)[0, 0], centres(cfg, P, 3)[0, 1])
    assert fleet.wall_edge[1, 0] == 27 and same_bits(centres(cfg, P, 3)[1, 0, :2], point)
    assert (fleet.wall_stage >= 0).all() and (fleet.wall_stage < cfg.N_hor).all()


def test_walls_none_is_the_plain_mirror():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = fleet24(cfg, 12)
    o = oracle_for(cfg)
    a = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, walls=None)
    b = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0)
    for k in range(3):
        Pa, Pb = a.step(o.warm_solve())[0], b.step(o.warm_solve())[0]
        assert same_bits(Pa, Pb) and same_bits(a.U, b.U) and same_bits(a.state, b.state), f"step {k}"
    assert not hasattr(a, "wall_edge")


def test_walls_checked_refuses():
    cfg = named_config("cfg1")
    routes = fleet24(cfg)[0]
    assert max(len(r.vertices) for r in routes) == 7 and cfg.Nobs == 10
    edges = scene_map(cfg)[0]
    ok = dict(edges=edges, slots=3, radius=0.5, range=2.0, spacing=0.0)
    assert same_bits(Walls(**ok).checked(cfg, routes), edges)
    Walls(**{**ok, "spacing": 1.0}).checked(cfg, routes)
    nan_, inf_ = edges.copy(), edges.copy()
    nan_[3, 2], inf_[25, 0] = math.nan, -math.inf
    bad = [dict(slots=0), dict(slots=4), dict(slots=11), dict(edges=edges[:0]), dict(edges=scene_map(cfg, 40)[0]), dict(edges=edges[:, :3]),
           dict(edges=nan_), dict(edges=inf_), dict(radius=0.0), dict(radius=-1.0), dict(radius=math.inf), dict(radius=math.nan),
           dict(range=0.0), dict(range=-2.0), dict(range=math.inf), dict(range=math.nan), dict(spacing=-0.1), dict(spacing=math.inf),
           dict(spacing=math.nan)]
    for kw in bad:
        with pytest.raises(ValueError):
            Walls(**{**ok, **kw}).checked(cfg, routes)
    assert len(scene_map(cfg, 40)[0]) == 1040
    with pytest.raises(ValueError, match="route 0"):                       # 150 vertices: the assembly's window fills every slot
        c = SHAPES["verts150-nobs10"]()
        Walls(**{**ok, "slots": 1}).checked(c.cfg, [c.route])
    none = load_config(Nobs=0, Ndynobs=0)
    with pytest.raises(ValueError):
        Walls(**{**ok, "slots": 1}).checked(none, [])
    with pytest.raises(ValueError):                                        # through the constructor
        routes, route_of, starts, i0 = fleet24(cfg)
        FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, walls=Walls(**{**ok, "slots": 4}))


def test_subdivided_map():
    cfg = named_config("cfg1")
    edges, off = frontend.map_edges(frontend.scene_planner(cfg, 11))
    e1, o1 = subdivided_map(edges, off, 1)
    assert same_bits(e1, edges) and np.array_equal(o1, off) and o1.dtype == np.int32
    for pieces in (4, 39):
        e, o = subdivided_map(edges, off, pieces)
        assert e.shape == (26 * pieces, 4) and np.array_equal(o, off * pieces)
        assert same_bits(e[::pieces, 0:2], edges[:, 0:2]) and same_bits(e[pieces - 1::pieces, 2:4], edges[:, 2:4])
        assert same_bits(e[1:, 0:2].reshape(-1, 2)[np.arange(len(e) - 1) % pieces != pieces - 1],
                         e[:-1, 2:4].reshape(-1, 2)[np.arange(len(e) - 1) % pieces != pieces - 1])      # a piece starts where the one before ends
        d, full = e[:, 2:4] - e[:, 0:2], np.repeat(edges[:, 2:4] - edges[:, 0:2], pieces, axis=0)
        assert np.allclose(d * pieces, full, atol=1e-12)                   # collinear, in the edge's direction
        MapMonitor(e, o).checked()
        assert same_bits(MapMonitor(e, o).checked()[0], e)
    with pytest.raises(ValueError):
        subdivided_map(edges, off, 0)
    with pytest.raises(ValueError):
        MapMonitor(*subdivided_map(edges, off, 40)).checked()


def test_walls_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_walls", "nmpc_loop_walls"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
    assert lib.nmpc_loop_set_walls(None, 1, None, 1, 1.0, 1.0, 0.0) == -3 and lib.nmpc_loop_walls(None, None, None) == -3
