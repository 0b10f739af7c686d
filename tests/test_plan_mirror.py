"""CPU: the batched planner's host mirror (``frontend.plan_batch_mirror``) against the literal
``VisibilityPlanner``: every visibility equals ``_free``, reachability equals ``shortest_path``, lengths agree to 1e-9 relative (the two
sum the same legs with ``hypot`` against ``sqrt``), every mirror path is valid under the literal rule, and a waypoint sequence may
differ from A*'s only at an exact tie.  tests/test_gpu_plan.py then pins the kernels to the mirror bit for bit, on the queries built here."""
import functools
import math

import numpy as np
import pytest

from mpc_trajectory_generator_amd import frontend, named_config, workloads
from mpc_trajectory_generator_amd.frontend import PlanResult, plan_batch_mirror, plan_routes, plan_scene, scene_planner

QUERY_SCENES = (1, 2, 3, 4, 7, 11, 12)
REL = 1e-9


@functools.lru_cache(maxsize=None)
def planner_of(scene):
    return scene_planner(named_config("cfg1"), scene)


def grid_planner(cols=5, rows=4, boundary=None):
    return workloads.square_grid_planner(named_config("cfg1"), cols, rows, boundary)


@functools.lru_cache(maxsize=None)
def grid80():
    return grid_planner()


@functools.lru_cache(maxsize=None)
def grid80_round():
    """The 80-node grid inside a regular 200-gon: no more nodes (the boundary's corners are all convex), 280 edges."""
    c, r = (8.5, 7.0), 13.0
    return grid_planner(boundary=[(c[0] + r * math.cos(2 * math.pi * k / 200), c[1] + r * math.sin(2 * math.pi * k / 200)) for k in range(200)])


def seeded_queries(pl, seed, count):
    """-> (starts, goals) [count, 2], uniform in the bounding box of the deflated boundary: per query x then y of the start, then x
    then y of the goal, from ``np.random.default_rng(seed)``."""
    rng = np.random.default_rng(seed)
    xs, ys = [p[0] for p in pl.boundary], [p[1] for p in pl.boundary]
    q = np.array([[rng.uniform(min(xs), max(xs)), rng.uniform(min(ys), max(ys)), rng.uniform(min(xs), max(xs)), rng.uniform(min(ys), max(ys))]
                  for _ in range(count)])
    return q[:, :2].copy(), q[:, 2:].copy()


@functools.lru_cache(maxsize=None)
def scene_queries(scene):
    return seeded_queries(planner_of(scene), scene, 150)


@functools.lru_cache(maxsize=None)
def grid_queries():
    return seeded_queries(grid80(), 80, 130)


def edge_queries(pl, scene=11):
    """-> (names, starts, goals): the edges of the rule on a scene's planner, from / to the scene's own start and end."""
    s = frontend.SCENE_POLYGONS[scene]
    a, b = s["start"][:2], s["end"][:2]
    o = pl.obstacles[0]
    inside = tuple(np.mean(np.array(pl.original_obstacles[0]), axis=0))
    xs, ys = [p[0] for p in pl.boundary], [p[1] for p in pl.boundary]
    cases = [("start == goal", a, a), ("start on a node", pl.nodes[0], b),
             ("start on an inflated obstacle's edge", (0.5 * (o[0][0] + o[1][0]), 0.5 * (o[0][1] + o[1][1])), b),
             ("goal inside an obstacle", a, inside), ("start outside the boundary", (min(xs) - 5.0, min(ys) - 5.0), b),
             ("NaN start", (math.nan, a[1]), b), ("NaN goal", a, (b[0], math.nan)), ("infinite start", (math.inf, a[1]), b),
             ("infinite goal", a, (-math.inf, math.inf)), ("the scene's own", a, b)]
    return [c[0] for c in cases], np.array([c[1] for c in cases], dtype=np.float64), np.array([c[2] for c in cases], dtype=np.float64)


def literal_path(pl, s, g):
    """``shortest_path`` -> (waypoints, length), (None, inf) for its ValueError"""
    try:
        return pl.shortest_path(tuple(s), tuple(g))
    except ValueError:
        return None, math.inf


def mirror_waypoints(pl, res, starts, goals, q):
    pts = [tuple(map(float, starts[q])), tuple(map(float, goals[q]))] + pl.nodes
    return [pts[j] for j in res.wp[q, :res.n_wp[q]]]


def check_against_literal(pl, starts, goals, res=None):
    """Everything the module docstring lists, for the queries (starts, goals) on ``pl``; -> (reachable, queries whose sequences differ)."""
    res = plan_batch_mirror(pl, starts, goals) if res is None else res
    V = len(pl.nodes)
    assert res.wp.shape == (len(starts), V + 2) and res.vis.shape == (len(starts), 2 * V + 1)
    reachable, differ = 0, []
    for q in range(len(starts)):
        s, g = tuple(map(float, starts[q])), tuple(map(float, goals[q]))
        lit = [pl._free(s, k) for k in pl.nodes] + [pl._free(g, k) for k in pl.nodes] + [pl._free(s, g)]
        assert res.vis[q].astype(bool).tolist() == lit, f"query {q}: visibility"
        path, length = literal_path(pl, s, g)
        assert (path is None) == (res.n_wp[q] == 0), f"query {q}: reachability"
        assert (res.wp[q, res.n_wp[q]:] == -1).all()
        if path is None:
            assert res.length[q] == math.inf
            continue
        reachable += 1
        assert abs(res.length[q] - length) <= REL * length, f"query {q}: lengths {res.length[q]!r} {length!r}"
        mine = mirror_waypoints(pl, res, starts, goals, q)
        # valid under the literal rule: from the start to the goal, consecutive waypoints free, the legs summing to the length
        assert mine[0] == s and mine[-1] == g and len(set(res.wp[q, :res.n_wp[q]].tolist())) == res.n_wp[q]
        assert all(pl._free(u, v) for u, v in zip(mine, mine[1:]))
        total = sum(math.hypot(u[0] - v[0], u[1] - v[1]) for u, v in zip(mine, mine[1:]))
        assert abs(total - res.length[q]) <= REL * max(total, 1e-300)
        if mine != path:
            differ.append(q)      # a tie: an equally short path (the lengths agree, both are valid)
    return reachable, differ


@pytest.mark.parametrize("scene", range(13))
def test_node_visibility_equals_free(scene):
    pl = planner_of(scene)
    sc = plan_scene(pl)
    V = len(pl.nodes)
    assert sc.visibility.shape == (V, V) and sc.edges.shape[1] == 4 and sc.poly_off[-1] == len(sc.edges)
    lit = np.array([[pl._free(a, b) for b in pl.nodes] for a in pl.nodes], dtype=bool).reshape(V, V)
    assert np.array_equal(sc.visibility.astype(bool), lit)
    assert sc.node_vertex.shape == (V, 2) and [tuple(v) for v in sc.node_vertex] == [pl.original_vertices([None, c, None])[0] for c in pl.nodes]


@pytest.mark.parametrize("scene", QUERY_SCENES)
def test_seeded_queries_equal_the_literal_planner(scene):
    """150 seeded queries per scene (of all 1050: 388 reachable; one sequence differs, scene 12 query 105, whose two lengths are
    95.97011191262234 and 95.97011191262231)."""
    reachable, differ = check_against_literal(planner_of(scene), *scene_queries(scene))
    print(f"scene {scene}: {reachable} of 150 reachable, {len(differ)} sequences differ from A*'s: {differ}")
    assert reachable > 0


@pytest.mark.parametrize("scene", range(13))
def test_scene_own_route_is_identical(scene):
    pl = planner_of(scene)
    s = frontend.SCENE_POLYGONS[scene]
    starts, goals = np.array([s["start"][:2]], dtype=np.float64), np.array([s["end"][:2]], dtype=np.float64)
    reachable, differ = check_against_literal(pl, starts, goals)
    assert reachable == 1 and not differ


def test_edges_of_the_rule():
    pl = planner_of(11)
    names, starts, goals = edge_queries(pl)
    res = plan_batch_mirror(pl, starts, goals)                       # (returns: the rounds are counted)
    check_against_literal(pl, starts, goals, res)
    got = dict(zip(names, zip(res.n_wp.tolist(), res.length.tolist())))
    assert got["start == goal"] == (2, 0.0) and res.wp[0, :2].tolist() == [0, 1]
    assert got["start on a node"][0] >= 2 and got["start on an inflated obstacle's edge"][0] >= 2 and got["the scene's own"][0] >= 2
    for name in ("goal inside an obstacle", "start outside the boundary", "NaN start", "NaN goal", "infinite start", "infinite goal"):
        assert got[name] == (0, math.inf), name
    # one query alone, and none
    one = plan_batch_mirror(pl, starts[-1:], goals[-1:])
    assert np.array_equal(one.wp, res.wp[-1:]) and one.length.tobytes() == res.length[-1:].tobytes()
    none = plan_batch_mirror(pl, np.zeros((0, 2)), np.zeros((0, 2)))
    assert none.n_wp.shape == (0,) and none.wp.shape == (0, len(pl.nodes) + 2)


def test_scene_without_nodes():
    """Scene 5: V = 0, a query's points are the start and the goal alone."""
    pl = planner_of(5)
    assert len(pl.nodes) == 0
    starts, goals = seeded_queries(pl, 5, 20)
    s = frontend.SCENE_POLYGONS[5]
    starts[0], goals[0] = s["start"][:2], s["end"][:2]
    res = plan_batch_mirror(pl, starts, goals)
    assert res.wp.shape == (20, 2) and res.vis.shape == (20, 1)
    reachable, differ = check_against_literal(pl, starts, goals, res)
    assert reachable >= 1 and not differ and set(res.n_wp.tolist()) <= {0, 2}


def test_grid_of_80_nodes():
    """n = 82 > 64 points and E = 84 > 64 edges: what the kernels stride over."""
    pl = grid80()
    sc = plan_scene(pl)
    assert len(sc.nodes) == 80 and len(sc.edges) == 84
    lit = np.array([[pl._free(a, b) for b in pl.nodes] for a in pl.nodes], dtype=bool)
    assert np.array_equal(sc.visibility.astype(bool), lit)
    reachable, differ = check_against_literal(pl, *grid_queries())
    print(f"grid: {reachable} of 130 reachable, {len(differ)} sequences differ from A*'s: {differ}")
    assert reachable >= 30
    rsc = plan_scene(grid80_round())
    assert len(rsc.nodes) == 80 and len(rsc.edges) == 280


def test_routes_equal_the_literal_planner():
    """``plan_routes`` (the host part of ``DevicePlanner.routes``) on a mirror result builds what ``VisibilityPlanner.route`` builds."""
    pl = planner_of(1)
    starts, goals = scene_queries(1)
    res = plan_batch_mirror(pl, starts, goals)
    ok = np.nonzero((res.n_wp > 0) & (res.length > 1.0))[0][:12]
    assert len(ok) == 12
    s3 = np.column_stack([starts[ok], np.linspace(-1, 1, 12)])
    e3 = np.column_stack([goals[ok], np.linspace(1, -1, 12)])
    sub = PlanResult(res.n_wp[ok], res.wp[ok], res.length[ok], res.vis[ok])
    compared = 0
    for r, s, e in zip(plan_routes(pl, sub, s3, e3), s3, e3):
        lit = pl.route(tuple(s), tuple(e))
        if r.waypoints != lit.waypoints:
            continue
        compared += 1
        assert r.start == lit.start and r.end == lit.end and r.vertices == lit.vertices and r.dyn_obs_list == lit.dyn_obs_list
        assert r.x_ref == lit.x_ref and r.y_ref == lit.y_ref and r.theta_ref == lit.theta_ref
    assert compared >= 11
    bad = PlanResult(np.array([2, 0, 0], dtype=np.int32), np.tile(np.array([0, 1] + [-1] * len(pl.nodes), dtype=np.int32), (3, 1)), None, None)
    with pytest.raises(ValueError, match="robot 1"):
        plan_routes(pl, bad, s3[:3], e3[:3])


def test_own_route_fleet_contract():
    from mpc_trajectory_generator_amd.trajectory import Missions
    cfg = named_config("cfg1")
    calls = []

    def plan(s, g):
        calls.append(len(s))
        return plan_batch_mirror(planner_of(1), s, g)
    routes, route_of, starts, idx0, legs = workloads.own_route_fleet(cfg, 1, 5, seed=3, legs=3, plan=plan)
    assert len(routes) == 15 and route_of.dtype == np.int32 and route_of.tolist() == [0, 3, 6, 9, 12]
    assert starts.shape == (5, 3) and idx0.dtype == np.int32 and idx0.tolist() == [0] * 5
    assert legs == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14]] and calls[0] == 5
    off, leg_route = Missions(legs).checked(5, len(routes), route_of)
    assert off.tolist() == [0, 3, 6, 9, 12, 15] and leg_route.tolist() == list(range(15))
    pl = planner_of(1)
    for b in range(5):
        assert tuple(starts[b]) == routes[3 * b].start
        for k in range(3):
            r = routes[3 * b + k]
            assert r.waypoints[0] == r.start[:2] and r.waypoints[-1] == r.end[:2]
            if k:
                assert r.start[:2] == routes[3 * b + k - 1].end[:2]                       # a leg starts where the one before ends
            total = sum(math.hypot(u[0] - v[0], u[1] - v[1]) for u, v in zip(r.waypoints, r.waypoints[1:]))
            assert total >= 12.0 * (1 - REL) and all(pl._free(u, v) for u, v in zip(r.waypoints, r.waypoints[1:]))
            assert r.start[2] == math.atan2(r.waypoints[1][1] - r.waypoints[0][1], r.waypoints[1][0] - r.waypoints[0][0])
    # the default plan is the mirror, and the draw is a function of the seed
    again = workloads.own_route_fleet(cfg, 1, 5, seed=3, legs=3)
    assert [r.waypoints for r in again[0]] == [r.waypoints for r in routes] and np.array_equal(again[2], starts)
    other = workloads.own_route_fleet(cfg, 1, 5, seed=4)
    assert len(other[0]) == 5 and other[4] == [[b] for b in range(5)] and not np.array_equal(other[2], starts)


def test_limits_raise():
    cfg = named_config("cfg1")
    with pytest.raises(ValueError, match="nodes"):
        plan_scene(grid_planner(8, 8))                    # 256 nodes
    many = [(20.0 + 30 * math.cos(2 * math.pi * k / 1100), 20.0 + 30 * math.sin(2 * math.pi * k / 1100)) for k in range(1100)]
    with pytest.raises(ValueError, match="edges"):
        plan_batch_mirror(frontend.VisibilityPlanner(cfg, many, []), np.zeros((1, 2)), np.ones((1, 2)))
    with pytest.raises(ValueError, match="starts"):
        plan_batch_mirror(planner_of(1), np.zeros((2, 2)), np.zeros((3, 2)))


def test_planner_abi_refuses_bad_scenes_without_a_device():
    """Argument checks come before the device is looked for: NMPC_ERR_BAD_ARG (-3) here as on a GPU box, nothing allocated."""
    import ctypes as C
    from mpc_trajectory_generator_amd import _lib
    lib = _lib.load_library()
    sc = plan_scene(planner_of(1))
    nodes, edges = np.ascontiguousarray(sc.nodes), np.ascontiguousarray(sc.edges)

    def new(n_node=len(nodes), n_edge=len(edges), off=sc.poly_off, max_batch=16, edge=edges):
        off = np.ascontiguousarray(off, dtype=np.int32)
        s = _lib.NmpcScene(n_node, n_edge, len(off) - 1, 0, _lib.as_dp(nodes), _lib.as_dp(edge), _lib.as_i32p(off))
        h = C.c_void_p()
        rc = lib.nmpc_planner_new(C.byref(s), 0, max_batch, C.byref(h))
        if rc == 0:
            lib.nmpc_planner_free(h)
        else:
            assert not h.value
        return rc
    off = sc.poly_off.copy()
    assert new(n_node=255) == -3 and new(n_edge=1025) == -3 and new(n_node=-1) == -3 and new(n_edge=2) == -3
    assert new(max_batch=0) == -3 and new(max_batch=(1 << 20) + 1) == -3 and new(edge=None) == -3
    assert new(off=off + 1) == -3                         # does not start at 0
    assert new(off=off[:-1]) == -3                        # does not end at n_edge
    bad = off.copy()
    bad[1] = bad[0] + 2
    assert new(off=bad) == -3                             # a polygon of two edges
    bad = off.copy()
    bad[1] = bad[2] + 1
    assert new(off=bad) == -3                             # not ascending
    assert lib.nmpc_planner_new(None, 0, 16, C.byref(C.c_void_p())) == -3
    assert new() in (0, -4)                               # the scene itself is fine: a device, or none
