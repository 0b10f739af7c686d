"""The BASELINE batch of a configuration, the fleets of the receding-horizon loop and what "the same bits" means, for every probe
and test that quotes a number.

bench.py's ``make_batch`` is the contract; tests/test_workloads.py holds ``baseline_batch`` to it array for array."""
import math

import numpy as np

from .config import named_config
from .frontend import (PlanResult, VisibilityPlanner, _point_in_polygon, offset_polygon, plan_batch_mirror, plan_routes, random_routes, scene_planner)
from .harness import Route, scene_route, synthetic_batch

# what the generator adds per configuration: config 3 a synthetic circle field, config 4 random moving ellipses
_GENERATOR_FLAGS = {"cfg3": dict(synthetic_circles=True), "nobs50": dict(synthetic_circles=True),
                    "cfg4": dict(random_dyn=True), "smooth_velocity": dict(random_dyn=True)}

# the status fields two solves of one instance must agree on (solve_time_ms is a clock, reserved the kernel's pass counter)
PARITY_FIELDS = ("exit_status", "num_outer_iterations", "num_inner_iterations", "num_cost_evals",
                 "num_grad_evals", "last_problem_norm_fpr", "delta_y_norm_over_c", "f2_norm", "penalty", "cost")


def baseline_batch(name, B=8192, seed=0, *, scene=11, routes=32):
    """-> (cfg, P [B, n_p]): the batch bench.py times for ``--config name --batch B`` on rank ``seed``.
    ``routes`` start/goal pairs planned with seed 1000 + seed; 0: the scene's own route."""
    cfg = named_config(name)
    planned = random_routes(cfg, scene, routes, seed=1000 + seed) if routes > 0 else None
    return cfg, synthetic_batch(cfg, scene, B, seed=seed, routes=planned, **_GENERATOR_FLAGS.get(name, {}))


def differing(a, b, rows=None):
    """Names ("u", "y", status fields in PARITY_FIELDS order) on which the (u, y, status) triples ``a`` and ``b`` are not
    bit-equal; ``a`` is indexed by ``rows`` first (a permutation against a permuted re-solve, a sample against its own solve)."""
    (ua, ya, sa), (ub, yb, sb) = a, b
    if rows is not None:
        ua, ya, sa = ua[rows], ya[rows], sa[rows]
    pairs = [(f, sa[f], sb[f]) for f in PARITY_FIELDS] + [("u", ua, ub), ("y", ya, yb)]
    return [n for n, x, y in pairs if not np.array_equal(x, y)]


def moving_ellipses(centres, rng):
    """centres [B, K, 2] -> the six arrays ``VectorizedRecedingHorizon`` takes as ``dyn_obs``: two end points within 5 m per axis of
    the centre, a frequency, two radii, an angle; drawn from ``rng`` in that order."""
    c, s = centres, centres.shape[:2]
    return (c + rng.uniform(-5, 5, c.shape), c + rng.uniform(-5, 5, c.shape), rng.uniform(0.05, 0.1, s),
            rng.uniform(0.3, 1.0, s), rng.uniform(0.3, 1.0, s), rng.uniform(0, np.pi, s))


def route_fleet(route, B, seed, K=0, back=25):
    """-> (idx0 [B], starts [B, 3], dyn): B robots started along one route, at samples at least ``back`` before its end, off it by
    noise (sigma 0.05 m, 0.05 m, 0.1 rad); dyn: K moving ellipses per robot around samples 0..29 ahead of its start, None for K = 0.
    One stream: (idx0, starts) do not depend on K."""
    rng = np.random.default_rng(seed)
    n = len(route.x_ref)
    xr, yr, tr = np.array(route.x_ref), np.array(route.y_ref), np.array(route.theta_ref)
    i0 = rng.integers(0, max(1, n - back), B)
    starts = np.stack([xr[i0] + rng.normal(0, 0.05, B), yr[i0] + rng.normal(0, 0.05, B), tr[i0] + rng.normal(0, 0.1, B)], axis=1)
    if not K:
        return i0, starts, None
    jj = np.minimum(n - 1, i0[:, None] + rng.integers(0, 30, (B, K)))
    return i0, starts, moving_ellipses(np.stack([xr[jj], yr[jj]], axis=2), rng)


def fleet_ellipses(routes, route_of, idx0, K, seed):
    """-> dyn: K moving ellipses per robot around samples 0..29 ahead of ``idx0`` on the robot's own route (clipped to its end),
    None for K = 0.  The samples are drawn robot by robot, in fleet order."""
    if not K:
        return None
    rng = np.random.default_rng(seed)
    c = np.empty((len(route_of), K, 2))
    for b, r in enumerate(route_of):
        x, y = np.array(routes[r].x_ref), np.array(routes[r].y_ref)
        jj = np.minimum(len(x) - 1, idx0[b] + rng.integers(0, 30, K))
        c[b] = np.stack([x[jj], y[jj]], axis=1)
    return moving_ellipses(c, rng)


def staggered_fleet(cfg, scene=1, planned=3, seed=5, back=(2, 5, 12, 40)):
    """-> (routes, route_of, starts, idx0): the scene's own route and ``planned`` random ones (``random_routes`` with ``seed``), and on
    each route one robot per entry of ``back``, standing on the route that many samples before its end.  The robots reach their goals
    many steps apart: the fleet of the retirement tests."""
    routes = [scene_route(cfg, scene)] + random_routes(cfg, scene, planned, seed=seed)
    n = np.array([len(r.x_ref) for r in routes])
    route_of = np.repeat(np.arange(len(routes)), len(back)).astype(np.int32)
    i0 = np.maximum(0, n[route_of] - np.tile(np.array(back), len(routes))).astype(np.int32)
    starts = np.stack([[routes[r].x_ref[i], routes[r].y_ref[i], routes[r].theta_ref[i]] for r, i in zip(route_of, i0)])
    return routes, route_of, starts, i0


def handmade_route(cfg, waypoints, vertices=()):
    """-> a ``harness.Route`` through the literal ``waypoints`` [(x, y), ...] (two at least, the first two apart) with the circle centres
    ``vertices``: the start heading points along the first segment, the end heading is 0.  Routes no planner gives: of a few samples,
    of one, with many vertices, with none."""
    w = [(float(x), float(y)) for x, y in waypoints]
    th0 = math.atan2(w[1][1] - w[0][1], w[1][0] - w[0][0])
    return Route(cfg, (w[0][0], w[0][1], th0), (w[-1][0], w[-1][1], 0.0), w, [(float(x), float(y)) for x, y in vertices])


def mission_fleet(cfg, corners, n_legs, first=None, offsets=None, vertices=()):
    """-> (routes, route_of, starts, idx0, legs): ``routes[i]`` = ``handmade_route`` from ``corners[i]`` to ``corners[i + 1]`` (a leg's first
    waypoint is the goal of the leg before; ``vertices`` on every one), and one robot per entry of ``n_legs`` whose mission is that many
    consecutive routes from ``first[b]`` on (default 0).  Robot b starts at the first corner of its mission, heading along the leg,
    moved by ``offsets[b]`` = (dx, dy, dtheta) if given; idx0 is 0 as the reference's.  ``legs`` is what ``trajectory.Missions`` takes."""
    c = [(float(x), float(y)) for x, y in corners]
    routes = [handmade_route(cfg, [c[i], c[i + 1]], vertices) for i in range(len(c) - 1)]
    B = len(n_legs)
    first = [0] * B if first is None else list(first)
    legs = [list(range(f, f + n)) for f, n in zip(first, n_legs)]
    assert all(n >= 1 and m[-1] < len(routes) for n, m in zip(n_legs, legs))
    starts = np.array([routes[f].start for f in first], dtype=np.float64).reshape(B, 3)
    if offsets is not None:
        starts = starts + np.asarray(offsets, dtype=np.float64).reshape(B, 3)
    return routes, np.array(first, dtype=np.int32), starts, np.zeros(B, dtype=np.int32), legs


def square_grid_planner(cfg, cols=5, rows=4, boundary=None):
    """A planner on cols x rows unit squares on a 3 m grid inside a rectangle (or inside ``boundary``): a synthetic scene with 4 cols rows
    nodes and as many edges plus the boundary's; 5 x 4 gives 80 nodes and 84 edges, more points than a wave has lanes."""
    obstacles = [[(3.0 * i + 2, 3.0 * j + 2), (3.0 * i + 3, 3.0 * j + 2), (3.0 * i + 3, 3.0 * j + 3), (3.0 * i + 2, 3.0 * j + 3)]
                 for i in range(cols) for j in range(rows)]
    boundary = boundary or [(0.0, 0.0), (3.0 * cols + 2, 0.0), (3.0 * cols + 2, 3.0 * rows + 2), (0.0, 3.0 * rows + 2)]
    return VisibilityPlanner(cfg, boundary, obstacles)


def free_point_sampler(pl, rng):
    """-> a function drawing one collision-free point of the planner's scene from ``rng``, as ``random_routes`` draws them: uniform in
    the bounding box of the deflated boundary, strictly inside it and not within 0.25 m of an inflated obstacle."""
    xs, ys = [p[0] for p in pl.boundary], [p[1] for p in pl.boundary]
    grown = [offset_polygon(o, 0.25) for o in pl.obstacles]

    def sample():
        while True:
            p = (rng.uniform(min(xs), max(xs)), rng.uniform(min(ys), max(ys)))
            if _point_in_polygon(p, pl.boundary, strict=True) and not any(_point_in_polygon(p, o, strict=False) for o in grown):
                return p
    return sample


def crowd_ellipses(cfg, scene, D, seed):
    """-> the six arrays ``trajectory.Crowd`` takes as ``obstacles``: D moving ellipses of the scene's world, each going back and forth
    between two collision-free points drawn as ``random_routes`` draws its end points (obstacle by obstacle, p1 then p2), with a
    frequency, two radii and an angle drawn as ``moving_ellipses`` draws them, from one stream seeded with ``seed``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sample = free_point_sampler(scene_planner(cfg, scene), rng)
    ends = np.array([[sample(), sample()] for _ in range(D)], dtype=np.float64).reshape(D, 2, 2)
    s = (D,)
    return (ends[:, 0].copy(), ends[:, 1].copy(), rng.uniform(0.05, 0.1, s), rng.uniform(0.3, 1.0, s), rng.uniform(0.3, 1.0, s),
            rng.uniform(0, np.pi, s))


def own_route_fleet(cfg, scene, B, seed, legs=1, plan=None, min_length=12.0):
    """-> (routes, route_of, starts, idx0, legs): every robot its own start and goal, and ``legs`` legs each: B * legs routes, robot b's
    the routes b * legs .. b * legs + legs - 1, a leg starting at the goal of the leg before.  ``route_of`` [B] is each robot's first
    route, ``starts`` [B, 3] its start pose heading along the first segment, ``idx0`` 0 as the reference's, and the last entry is what
    ``trajectory.Missions`` takes.  The points are collision free, drawn as ``random_routes`` draws them; ``plan`` =
    ``(starts [n, 2], goals [n, 2]) -> frontend.PlanResult`` answers a leg's queries at once: ``frontend.plan_batch_mirror`` on the scene's
    planner by default, or the ``plan`` of a ``DevicePlanner`` built on ``scene_planner(cfg, scene)``.  A query without a path or
    shorter than ``min_length`` is drawn again (both ends on the first leg, the goal on a later one), in robot order."""
    pl = scene_planner(cfg, scene)
    if plan is None:
        plan = lambda s, g: plan_batch_mirror(pl, s, g)      # noqa: E731
    sample = free_point_sampler(pl, np.random.Generator(np.random.PCG64(seed)))
    points = np.empty((B, legs + 1, 2))
    wp, n_wp = [None] * legs, [None] * legs
    for k in range(legs):
        todo = np.arange(B)
        wp[k], n_wp[k] = np.empty((B, len(pl.nodes) + 2), dtype=np.int32), np.empty(B, dtype=np.int32)
        for attempt in range(200):
            for b in todo:
                if k == 0:
                    points[b, 0] = sample()
                points[b, k + 1] = sample()
            res = plan(points[todo, k], points[todo, k + 1])
            wp[k][todo], n_wp[k][todo] = res.wp, res.n_wp
            todo = todo[(res.n_wp == 0) | ~(res.length >= min_length)]
            if not len(todo):
                break
        else:
            raise RuntimeError(f"own_route_fleet: no route of {min_length} m from where robot {int(todo[0])} stands after 200 draws")
    nodes = np.array(pl.nodes, dtype=np.float64).reshape(-1, 2)
    routes = []
    for b in range(B):
        for k in range(legs):
            pts = np.concatenate([points[b, k:k + 2], nodes])[wp[k][b, :n_wp[k][b]]]
            th0 = math.atan2(pts[1][1] - pts[0][1], pts[1][0] - pts[0][0])
            th1 = math.atan2(pts[-1][1] - pts[-2][1], pts[-1][0] - pts[-2][0])
            one = PlanResult(n_wp[k][b:b + 1], wp[k][b:b + 1], None, None)
            routes += plan_routes(pl, one, [(*points[b, k], th0)], [(*points[b, k + 1], th1)])
    route_of = (np.arange(B) * legs).astype(np.int32)
    starts = np.array([routes[r].start for r in route_of], dtype=np.float64).reshape(B, 3)
    return routes, route_of, starts, np.zeros(B, dtype=np.int32), [list(range(r, r + legs)) for r in route_of]


def tiled_fleet(routes, route_of, starts, idx0, copies):
    """-> (routes, route_of, starts, idx0) of the fleet repeated: round(m * copies) robots, m = the robots given (``copies`` may be
    fractional), robot b a copy of base robot b % m.  Without peers the robots of a loop do not depend on each other, so row b of a
    loop over the tiled fleet is row b % m of a loop over the base fleet."""
    m = len(starts)
    rows = np.arange(int(round(m * copies))) % m
    return list(routes), np.asarray(route_of)[rows].astype(np.int32), np.array(starts, dtype=np.float64)[rows], \
        np.asarray(idx0)[rows].astype(np.int32)


def placed_fleet(routes, route_of, starts, idx0, places):
    """-> (routes, route_of, starts, idx0) of the same robots in another order: ``places`` = {position: robot} puts each named robot
    at its position by swapping it with whoever stands there, in the order given (a robot named twice follows its swaps).  Without
    peers and plant ids the robots of a loop do not depend on each other, so only the index a robot is known by changes: the way to
    put a robot chosen on a dry run where a kernel's strides and chunks meet it."""
    order = np.arange(len(starts))
    for pos, robot in places.items():
        at = int(np.nonzero(order == robot)[0][0])
        order[[pos, at]] = order[[at, pos]]
    return list(routes), np.asarray(route_of)[order].astype(np.int32), np.array(starts, dtype=np.float64)[order], \
        np.asarray(idx0)[order].astype(np.int32)


def ensemble_fleet(route, start, B, idx0=0):
    """-> (routes, route_of, starts, idx0): B copies of one robot on ``route``, at the pose ``start`` and reference sample ``idx0``.
    Without a plant every row of a loop over it is the same; under a ``trajectory.Plant`` robot b draws the disturbances of id b: the
    Monte-Carlo study of one controller in one run."""
    starts = np.tile(np.array(start, dtype=np.float64).reshape(1, 3), (B, 1))
    return [route], np.zeros(B, dtype=np.int32), starts, np.full(B, int(idx0), dtype=np.int32)


def grouped_ensemble(routes, route_of, starts, idx0, copies):
    """-> (routes, route_of, starts, idx0, group_of): every robot of a base fleet of m repeated ``copies`` times, robot b a copy of base
    robot b % m (as ``tiled_fleet``) and ``group_of[b]`` = that base robot, so the copies of one robot are interleaved with everybody
    else's and no group's members are contiguous.  Under a ``trajectory.Plant`` with ``trajectory.Ensemble(group_of, groups=m)`` each
    group is the Monte-Carlo study of one robot -- one route, one tuning -- and the loop compares m of them in one run."""
    m = len(starts)
    routes, route_of, starts, idx0 = tiled_fleet(routes, route_of, starts, idx0, int(copies))
    return routes, route_of, starts, idx0, (np.arange(len(starts)) % m).astype(np.int32)


def stale_idx0(idx0, behind):
    """-> the start indices moved back by ``behind`` samples, clipped at 0: robots whose window search starts that far behind where
    they stand, so that the closest sample lies deep inside the first window."""
    return np.maximum(0, np.asarray(idx0) - behind).astype(np.int32)


def move_near_goal(routes, route_of, starts, idx0, back):
    """-> (starts, idx0) with robot b, for b < len(back), standing on its route ``back[b]`` samples before the end: robots that
    arrive within a few steps, among the others of a ``random_fleet``."""
    starts, idx0 = np.array(starts, dtype=np.float64), np.array(idx0, dtype=np.int32)
    for b, k in enumerate(back):
        r = routes[route_of[b]]
        idx0[b] = max(0, len(r.x_ref) - k)
        starts[b] = [r.x_ref[idx0[b]], r.y_ref[idx0[b]], r.theta_ref[idx0[b]]]
    return starts, idx0


def step_differing(dev, host, solve, dev_step=None, rows=None):
    """Step a ``DeviceRecedingHorizon`` (``dev_step(dev)`` if given, else ``dev.step()``) and its host mirror (``solve``: the mirror's
    solve function) once.  ``rows`` [dev.B]: the device runs a ``tiled_fleet`` of the mirror's, its robot b is the mirror's rows[b].
    -> (names, P, done): the names out of P, U, Y, state, last_u, idx, done, num_inner_iterations, exit_status on which the two are
    not bit-equal ("P" with its first differing columns), the device's parameter vectors and its ``done``.  A retiring pair
    (``retire=True``: the mirror's ``solve`` sees the active rows only) is also compared on retired_at and n_active, a pair with
    missions on leg, route_of and leg_at."""
    dev.step() if dev_step is None else dev_step(dev)
    P, st = host.step(solve)
    Pd, Ud, Yd = dev.params()
    state, last_u, idx, done, std = dev.read()
    pairs = [("P", Pd, P), ("U", Ud, host.U), ("Y", Yd, host.Y), ("state", state, host.state), ("last_u", last_u, host.last_u),
             ("idx", idx, host.idx), ("done", done, host.done)] + [(f, std[f], st[f]) for f in ("num_inner_iterations", "exit_status")]
    if host.active is not None:
        n_active, retired_at = dev.active()
        pairs.append(("retired_at", retired_at, host.retired_at))
    if getattr(host, "missions", None) is not None:
        pairs += list(zip(("leg", "route_of", "leg_at"), dev.legs(), (host.leg, host.route_of, host.leg_at)))
    if rows is not None:
        pairs = [(n, x, y[rows]) for n, x, y in pairs]
    if host.active is not None:
        pairs.append(("n_active", n_active, host.n_active if rows is None else int(host.active[rows].sum())))
    names = [n for n, x, y in pairs if not np.array_equal(x, y)]
    if "P" in names:
        names[0] = f"P at columns {np.unique(np.nonzero(Pd != pairs[0][2])[1])[:10]}"
    return names, Pd, done


def clearance_differing(dev, host):
    """The fields of the clearance records (``dev``: a ``DeviceRecedingHorizon`` with a monitor or its ``clearance()``, ``host``: its
    mirror or the mirror's ``clearance``) that are not bit-equal; a value compares by its bytes, so -0.0 is not 0.0 and a NaN equals
    itself."""
    a = dev.clearance() if callable(getattr(dev, "clearance", None)) else dev
    b = getattr(host, "clearance", host)
    return [f for f in a.dtype.names if a[f].tobytes() != np.asarray(b[f], dtype=a[f].dtype).tobytes() or a[f].shape != b[f].shape]


def map_clearance_differing(dev, host):
    """``clearance_differing`` for the map monitor's records (``dev``: a ``DeviceRecedingHorizon`` with a map monitor or its
    ``map_clearance()``, ``host``: its mirror or the mirror's ``map_clearance``): the fields that are not bit-equal."""
    a = dev.map_clearance() if callable(getattr(dev, "map_clearance", None)) else dev
    b = getattr(host, "map_clearance", host)
    return [f for f in a.dtype.names if a[f].tobytes() != np.asarray(b[f], dtype=a[f].dtype).tobytes() or a[f].shape != b[f].shape]


def tracking_differing(dev, host):
    """``clearance_differing`` for the track monitor's records (``dev``: a ``DeviceRecedingHorizon`` with a track monitor or its
    ``tracking()``, ``host``: its mirror or the mirror's ``tracking()``): the fields that are not bit-equal."""
    a = dev.tracking() if callable(getattr(dev, "tracking", None)) else dev
    b = host.tracking() if callable(getattr(host, "tracking", None)) else host
    return [f for f in a.dtype.names if a[f].tobytes() != np.asarray(b[f], dtype=a[f].dtype).tobytes() or a[f].shape != b[f].shape]


def plant_differing(dev, host):
    """What a plant keeps (``dev``: a ``DeviceRecedingHorizon``, ``host``: its mirror, both with ``applied()`` and ``measured()``) -> the
    names that are not bit-equal: a value compares by its bytes, so -0.0 is not 0.0 and a NaN equals itself."""
    bad = []
    for name in ("applied", "measured"):
        a, b = getattr(dev, name)(), getattr(host, name)()
        if a.shape != b.shape:
            bad.append(f"{name} of shape {a.shape}, not {b.shape}")
        elif a.tobytes() != np.ascontiguousarray(b, dtype=a.dtype).tobytes():
            bad.append(name)
    return bad


def ensemble_differing(dev, host):
    """``clearance_differing`` for the ensemble's records (``dev``: a ``DeviceRecedingHorizon`` with an ensemble or its
    ``ensemble_stats()``, ``host``: its mirror or the mirror's ``ensemble_stats()``): the fields that are not byte-equal, or the shapes
    if they differ."""
    a = dev.ensemble_stats() if callable(getattr(dev, "ensemble_stats", None)) else np.asarray(dev)
    b = host.ensemble_stats() if callable(getattr(host, "ensemble_stats", None)) else np.asarray(host)
    if a.shape != b.shape:
        return [f"ensemble_stats of shape {a.shape}, not {b.shape}"]
    return [f for f in a.dtype.names if a[f].tobytes() != np.ascontiguousarray(b[f], dtype=a[f].dtype).tobytes()]


def walls_differing(dev, host):
    """What the walls keep (``dev``: a ``DeviceRecedingHorizon`` with walls, ``host``: its mirror) -> the names out of wall_edge and
    wall_stage that are not equal (the circles themselves are part of P)."""
    got = dict(zip(("wall_edge", "wall_stage"), dev.walls()))
    return [n for n, a in got.items() if a.shape != getattr(host, n).shape or not np.array_equal(a, getattr(host, n))]


def wall_grid_differing(dev, host):
    """What walls with a ``cell`` keep beside ``walls_differing`` (``dev``: a ``DeviceRecedingHorizon`` with such walls and a step
    taken, ``host``: its mirror) -> the names out of the grid's header fields, cell_off, cell_edge and looked that differ from the
    mirror's ``wall_grid`` and ``wall_looked``."""
    hdr, off, edge, looked = dev.wall_grid()
    g, want = host.wall_grid, host.wall_grid.header()
    bad = [f for f in ("origin", "h", "nx", "ny", "entries") if hdr[f].tobytes() != want[f].tobytes()]
    pairs = (("cell_off", off, g.cell_off), ("cell_edge", edge, g.cell_edge), ("looked", looked, host.wall_looked))
    return bad + [n for n, a, b in pairs if a.shape != b.shape or not np.array_equal(a, b)]


def map_grid_differing(dev, host):
    """``wall_grid_differing`` for a map monitor with a ``cell`` (``dev``: a ``DeviceRecedingHorizon`` with one and a step taken, ``host``:
    its mirror) -> the names out of the grid's header fields, cell_off, cell_edge and looked that differ from the mirror's
    ``map_monitor.grid`` and ``map_looked``."""
    hdr, off, edge, looked = dev.map_grid()
    g = host.map_monitor.grid
    want = g.header()
    bad = [f for f in ("origin", "h", "nx", "ny", "entries") if hdr[f].tobytes() != want[f].tobytes()]
    pairs = (("cell_off", off, g.cell_off), ("cell_edge", edge, g.cell_edge), ("looked", looked, host.map_looked))
    return bad + [n for n, a, b in pairs if a.shape != b.shape or not np.array_equal(a, b)]


def crowd_grid_differing(dev, grid, looked=None):
    """What a crowd with a ``cell`` keeps beside its table and ``seen`` (``dev``: a ``DeviceRecedingHorizon`` with such a crowd and a
    step taken, ``grid``: a ``trajectory.CrowdGrid`` in which the same step's table is filed, ``looked`` [B]: what it counts for each
    robot's last step, or None) -> the names out of the header's fields, cell_of and looked that differ.  The order inside a cell is
    not the device's to keep, so ``cell_mem`` is not compared: ``cell_of`` fixes every cell's members."""
    hdr, cell_of, looked_dev = dev.crowd_grid()
    want = grid.header()
    bad = [f for f in want.dtype.names if hdr[f].tobytes() != want[f].tobytes()]
    pairs = [("cell_of", cell_of, grid.cell_of)] + ([] if looked is None else [("looked", looked_dev, np.asarray(looked))])
    return bad + [n for n, a, b in pairs if a.shape != b.shape or not np.array_equal(a, b)]


def subdivided_map(edges, poly_off, pieces):
    """-> (edges [E * pieces, 4], poly_off): every edge of a map (``frontend.map_edges``) cut into ``pieces`` collinear pieces, in the
    edge's direction, polygon by polygon as before: piece i runs from a + (i / pieces) * (b - a) to the next piece's start, and the last
    ends exactly at the original end point b.  ``pieces`` = 1 gives the map back.  For tests and benchmarks with many edges;
    ``trajectory.MapMonitor`` and ``trajectory.Walls`` take the result."""
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 4)
    pieces = int(pieces)
    if pieces < 1:
        raise ValueError("subdivided_map: pieces < 1")
    a, b = edges[:, None, 0:2], edges[:, None, 2:4]
    f = (np.arange(pieces + 1, dtype=np.float64) / float(pieces))[None, :, None]
    pts = a + f * (b - a)                                                   # [E, pieces + 1, 2]
    pts[:, 0], pts[:, -1] = edges[:, 0:2], edges[:, 2:4]
    out = np.concatenate([pts[:, :-1], pts[:, 1:]], axis=2).reshape(-1, 4)
    return np.ascontiguousarray(out), (np.asarray(poly_off, dtype=np.int64) * pieces).astype(np.int32)


LOG_PRODUCTS = ("controls", "step_records", "drive_summary", "step_totals")
LOG_CLOCK_FIELDS = ("solve_time_ms", "solve_ms_max")      # read from a clock: no two runs agree on them


def log_differing(dev, host):
    """The drive log's four products (``dev``: a ``DeviceRecedingHorizon`` with a log or a dict of its ``controls()``, ``step_records()``,
    ``drive_summary()`` and ``step_totals()``; ``host``: its mirror, or such a dict) -> the names, "product.field", that are not
    bit-equal: a value compares by its bytes, so -0.0 is not 0.0 and a NaN equals itself.  Every field but the two a clock gives."""
    def product(x, name):
        if isinstance(x, dict):
            return x[name]
        v = getattr(x, name)
        return v() if callable(v) else v
    bad = []
    for name in LOG_PRODUCTS:
        a, b = np.asarray(product(dev, name)), np.asarray(product(host, name))
        if a.shape != b.shape:
            bad.append(f"{name} of shape {a.shape}, not {b.shape}")
        elif a.dtype.names is None:
            if a.tobytes() != np.asarray(b, dtype=a.dtype).tobytes():
                bad.append(name)
        else:
            bad += [f"{name}.{f}" for f in a.dtype.names
                    if f not in LOG_CLOCK_FIELDS and a[f].tobytes() != np.asarray(b[f], dtype=a[f].dtype).tobytes()]
    return bad


def trajectory_differing(dev, host, steps, rows=None):
    """After ``steps`` steps of both: [] if the device's trajectory is [steps * num_steps_taken + 1, B, 3] and the mirror's bits
    (``rows`` as in ``step_differing``)."""
    T = dev.trajectory()
    if T.shape != (steps * host.cfg.num_steps_taken + 1, dev.B, 3):
        return [f"trajectory of shape {T.shape}"]
    Th = np.stack(host.traj)
    return [] if np.array_equal(T, Th if rows is None else Th[:, rows]) else ["trajectory"]
