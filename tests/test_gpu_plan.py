"""GPU: the planner kernels (``frontend.DevicePlanner``: nmpc_planner_* / nmpc_plan_batch_*, csrc/nmpc_plan.h)
against the host mirror ``frontend.plan_batch_mirror`` -- itself pinned to the literal ``VisibilityPlanner`` by
tests/test_plan_mirror.py, whose queries these are -- bit for bit: ``n_wp``, ``wp``, ``length`` by its bytes, the 2V + 1 visibility
bytes of every query, and the node-node matrix ``visibility()``."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config, workloads
from mpc_trajectory_generator_amd.frontend import DevicePlanner, plan_batch_mirror, plan_scene
from test_plan_mirror import edge_queries, grid80, grid80_round, grid_queries, planner_of, scene_queries, seeded_queries

pytestmark = pytest.mark.gpu


def differing(dev, host):
    """The fields of two ``PlanResult`` that are not the same bits (a length compares by its bytes: +inf equals itself)."""
    pairs = [("n_wp", dev.n_wp, host.n_wp), ("wp", dev.wp, host.wp), ("length", dev.length, host.length), ("vis", dev.vis, host.vis)]
    return [n for n, x, y in pairs if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes()]


@functools.lru_cache(maxsize=None)
def mirror_of(name):
    """-> (planner, starts, goals, the mirror's result), computed once per workload"""
    if name == "scene 11, B = 257":
        pl, (s, g) = planner_of(11), scene_queries(11)
        rows = np.arange(257) % 150
        s, g = s[rows], g[rows]
    elif name == "scene 1, B = 1025":
        pl, (s, g) = planner_of(1), scene_queries(1)
        rows = np.arange(1025) % 150
        s, g = s[rows], g[rows]
    elif name == "grid, B = 130":
        pl, (s, g) = grid80(), grid_queries()
    elif name == "round grid, B = 130":
        pl, (s, g) = grid80_round(), grid_queries()
    elif name == "scene 5, B = 3":
        pl = planner_of(5)
        s, g = seeded_queries(pl, 5, 3)
        s[0], g[0] = frontend.SCENE_POLYGONS[5]["start"][:2], frontend.SCENE_POLYGONS[5]["end"][:2]
    elif name == "scene 12, B = 1":
        pl, (s, g) = planner_of(12), scene_queries(12)
        s, g = s[105:106], g[105:106]                      # the query whose A* answer is another, equally short path
    else:
        assert name == "edges of the rule"
        pl = planner_of(11)
        _, s, g = edge_queries(pl)
    return pl, s, g, plan_batch_mirror(pl, s, g)


def run(name, max_batch=None):
    pl, s, g, want = mirror_of(name)
    dp = DevicePlanner(pl, max_batch=max_batch or len(s))
    try:
        got = dp.plan(s, g)
        assert not differing(got, want), name
        assert np.array_equal(dp.visibility(), plan_scene(pl).visibility)
        assert dp.last_ms > 0.0
    finally:
        dp.close()
    return got


def test_scene_11_tiled_queries():
    """B = 257 queries on the scene of the BASELINE workloads: V = 19, 39 segments per query, 10023 segments in 40 workgroups."""
    got = run("scene 11, B = 257")
    assert 0 < (got.n_wp > 0).sum() < 257


def test_grid_of_80_nodes():
    """V = 80, n = 82 points, E = 84 edges, 21 polygons (csrc/nmpc_plan.h).  nmpc_plan_path_kernel: the loops over `j = lane; j < n; j += 64`
    (points to LDS, wp out) and over the 161 visibility bytes run more than once, and slot k = 1 of every lane's `dist[k]` / `settled[k]`
    holds a point for lanes 0..17 and is beyond n for the others, so the pick, the settle and the relax loops over k take both branches
    of `settled[k] = lane + 64 * k >= n`; paths bend around nodes whose index is above 63.  nmpc_plan_visible_kernel: the query list
    has 130 * 161 = 20930 segments, 82 workgroups with the last one partly empty; the polygon loop runs 21 times."""
    pl, s, g, want = mirror_of("grid, B = 130")
    got = run("grid, B = 130")
    assert (got.n_wp > 0).sum() >= 30 and got.wp.max() > 63 and got.n_wp.max() >= 4


def test_more_edges_than_a_workgroup_has_threads():
    """The 80-node grid inside a 200-gon: E = 280 > 256 = PLAN_VIS_BLOCK, so nmpc_plan_visible_kernel's staging loop
    `for (e = threadIdx.x; e < E; e += PLAN_VIS_BLOCK)` runs twice for threads 0..23, and the boundary polygon alone has 200 edges."""
    got = run("round grid, B = 130")
    assert (got.n_wp > 0).sum() >= 30


def test_scene_without_nodes():
    """Scene 5: V = 0, n = 2, one segment per query; planner creation launches no node-node kernel and `visibility()` is [0, 0]."""
    got = run("scene 5, B = 3")
    assert got.wp.shape == (3, 2) and got.n_wp[0] == 2


def test_one_query():
    got = run("scene 12, B = 1", max_batch=1)
    assert got.n_wp[0] >= 3


def test_last_workgroup_partly_empty():
    """B = 1025 on scene 1 (V = 12): 25625 segments, 100 full workgroups and one of 25 threads' work."""
    run("scene 1, B = 1025")


def test_edges_of_the_rule_in_one_batch():
    """start == goal, a start on a node, on an inflated edge, a goal inside an obstacle, a start outside the boundary, NaN and infinite
    coordinates: one batch, the mirror's bits, and the call returns."""
    got = run("edges of the rule")
    assert got.n_wp.tolist()[:1] == [2] and got.length[0] == 0.0 and (got.n_wp[3:9] == 0).all() and np.isinf(got.length[3:9]).all()


def test_batch_size_limits_through_the_abi():
    pl, s, g, want = mirror_of("scene 5, B = 3")
    dp = DevicePlanner(pl, max_batch=3)
    try:
        lib, h = dp.lib, dp._pl
        n_wp, wp, length = np.full(4, 7, dtype=np.int32), np.full((4, 2), 7, dtype=np.int32), np.full(4, 7.0)
        s4, g4 = np.concatenate([s, s[:1]]), np.concatenate([g, g[:1]])
        args = (_lib.as_dp(s4), _lib.as_dp(g4), _lib.as_i32p(n_wp), _lib.as_i32p(wp), _lib.as_dp(length), None)
        assert lib.nmpc_plan_batch_host(h, 0, *args) == 0 and lib.nmpc_plan_batch_host(h, 0, None, None, None, None, None, None) == 0
        assert lib.nmpc_plan_batch_device(h, 0, None, None, None, None, None, None, None) == 0
        assert lib.nmpc_plan_batch_host(h, 4, *args) == -3 and lib.nmpc_plan_batch_host(h, -1, *args) == -3
        assert lib.nmpc_plan_batch_device(h, 4, None, None, None, None, None, None, None) == -3
        assert lib.nmpc_plan_batch_host(h, 3, None, *args[1:]) == -3 and lib.nmpc_plan_batch_host(h, 3, *args[:4], None, None) == -3
        assert lib.nmpc_plan_batch_host(None, 3, *args) == -3 and lib.nmpc_planner_visibility(h, None) == -3
        assert (n_wp == 7).all() and (wp == 7).all() and (length == 7.0).all()          # nothing was written
        with pytest.raises(frontend.SolverError):
            dp.plan(s4, g4)
        assert lib.nmpc_plan_batch_host(h, 3, *args) == 0                                # vis == NULL: kept in the planner
        assert np.array_equal(n_wp[:3], want.n_wp) and np.array_equal(wp[:3], want.wp) and length[:3].tobytes() == want.length.tobytes()
        assert n_wp[3] == 7 and length[3] == 7.0
    finally:
        dp.close()


def test_two_planners_alive_at_once():
    a, b = mirror_of("scene 11, B = 257"), mirror_of("grid, B = 130")
    pa, pb = DevicePlanner(a[0], max_batch=300), DevicePlanner(b[0], max_batch=130)
    try:
        ra1, rb1, ra2 = pa.plan(a[1], a[2]), pb.plan(b[1], b[2]), pa.plan(a[1], a[2])
        assert not differing(ra1, a[3]) and not differing(rb1, b[3]) and not differing(ra2, a[3])
        assert np.array_equal(pa.visibility(), plan_scene(a[0]).visibility) and np.array_equal(pb.visibility(), plan_scene(b[0]).visibility)
    finally:
        pa.close()
        pb.close()


def _hip():
    """the HIP runtime the library itself runs on (the one already mapped into this process), through ctypes"""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def test_device_entry_point_on_a_stream():
    """nmpc_plan_batch_device with operands in device memory on a stream of its own, with and without a d_vis of the caller's."""
    pl, s, g, want = mirror_of("grid, B = 130")
    B, V = len(s), len(pl.nodes)
    dp = DevicePlanner(pl, max_batch=B)
    hip = _hip()
    out = [np.zeros(B, dtype=np.int32), np.zeros((B, V + 2), dtype=np.int32), np.zeros(B), np.zeros((B, 2 * V + 1), dtype=np.uint8)]
    d = [C.c_void_p() for _ in range(6)]
    stream = C.c_void_p()
    try:
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        for ptr, a in zip(d, [s, g] + out):
            assert hip.hipMalloc(C.byref(ptr), a.nbytes) == 0
        assert hip.hipMemcpy(d[0], s.ctypes.data, s.nbytes, 1) == 0 and hip.hipMemcpy(d[1], g.ctypes.data, g.nbytes, 1) == 0
        for keep_vis in (True, False):
            for ptr, a in zip(d[2:], out):
                assert hip.hipMemset(ptr, 7, a.nbytes) == 0
            assert hip.hipDeviceSynchronize() == 0
            assert dp.lib.nmpc_plan_batch_device(dp._pl, B, d[0], d[1], d[2], d[3], d[4], d[5] if keep_vis else None, stream) == 0
            assert hip.hipStreamSynchronize(stream) == 0
            for ptr, a in zip(d[2:], out):
                assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
            assert keep_vis or (out[3] == 7).all()
            assert not differing(frontend.PlanResult(out[0], out[1], out[2], out[3] if keep_vis else want.vis), want)
    finally:
        for ptr in d:
            if ptr.value:
                hip.hipFree(ptr)
        if stream.value:
            hip.hipStreamDestroy(stream)
        dp.close()


def test_routes_of_a_device_plan():
    pl = planner_of(1)
    s, g = scene_queries(1)
    want = plan_batch_mirror(pl, s, g)
    ok = np.nonzero((want.n_wp > 0) & (want.length > 1.0))[0][:8]
    s3, e3 = np.column_stack([s[ok], np.zeros(8)]), np.column_stack([g[ok], np.ones(8)])
    dp = DevicePlanner(pl, max_batch=150)
    try:
        routes = dp.routes(s3, e3)
        sub = frontend.PlanResult(want.n_wp[ok], want.wp[ok], want.length[ok], want.vis[ok])
        for r, m in zip(routes, frontend.plan_routes(pl, sub, s3, e3)):
            assert r.waypoints == m.waypoints and r.vertices == m.vertices and r.x_ref == m.x_ref and r.theta_ref == m.theta_ref
        bad = int(np.nonzero(want.n_wp == 0)[0][0])
        with pytest.raises(ValueError, match="robot 1"):
            dp.routes([s3[0], (*s[bad], 0.0)], [e3[0], (*g[bad], 0.0)])
    finally:
        dp.close()


def test_own_route_fleet_drives_the_loop():
    """Every robot its own two-leg mission planned on the device (R = 32 routes for B = 16 robots), driven by the retiring loop with
    missions: 4 steps, everything ``step_differing`` compares equal to the host mirror's."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon, Missions
    cfg = named_config("cfg1")
    dp = DevicePlanner(frontend.scene_planner(cfg, 11), max_batch=16)
    try:
        fleet = workloads.own_route_fleet(cfg, 11, 16, seed=7, legs=2, plan=dp.plan)
    finally:
        dp.close()
    mirror = workloads.own_route_fleet(cfg, 11, 16, seed=7, legs=2)
    routes, route_of, starts, idx0, legs = fleet
    assert len(routes) == 32 and [r.waypoints for r in routes] == [r.waypoints for r in mirror[0]] and np.array_equal(starts, mirror[2])
    o = oracle_for(cfg)
    host = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=idx0, retire=True, missions=Missions(legs))
    s = BatchSolver(cfg, max_batch=16)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=4, idx0=idx0, route_of=route_of, retire=True, missions=Missions(legs))
        for step in range(4):
            bad = workloads.step_differing(dev, host, o.warm_solve(threads=16))[0]
            assert not bad, f"step {step}: {bad}"
        dev.close()
    finally:
        s.close()
