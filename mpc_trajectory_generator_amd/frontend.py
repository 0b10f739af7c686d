"""Route front-end: polygon inflation + visibility-graph shortest path.

The reference gets its route from third-party code: ``pyclipper`` inflates every obstacle by the
vehicle width with mitred joins and deflates the boundary (src/visibility/visibility.py:49-67,
90-105), ``extremitypathfinder`` builds a visibility graph over the inflated polygons and runs A*
(:69-88), and the path corners are mapped back to the nearest original vertices, which become the
NMPC's circle centres (:126-139).  Neither package is available here, so this module is an own
implementation of the same geometry -- **unpinned** against the reference's dependencies
(validated geometrically: tests/test_frontend.py).  ``VisibilityPlanner`` runs once per trajectory on the CPU.  A fleet whose
robots each have their own start and goal plans on the device instead: ``DevicePlanner`` answers a batch of queries with two
kernels (csrc/nmpc_plan.h), bit for bit what ``plan_batch_mirror`` computes here with NumPy.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import heapq
import math

import numpy as np

from . import _lib, harness
from .config import Config
from .solver import SolverError

_EPS = 1e-9


def _signed_area(poly):
    a = 0.0
    for i in range(len(poly)):
        x1, y1 = poly[i]
        x2, y2 = poly[(i + 1) % len(poly)]
        a += x1 * y2 - x2 * y1
    return 0.5 * a


def offset_polygon(poly, delta, miter_limit=2.0):
    """Mitred offset of a simple polygon by ``delta`` (> 0 grows it, < 0 shrinks it), the join
    style the reference asks pyclipper for (JT_MITER, visibility.py:92).  A corner whose mitre
    would reach further than ``miter_limit * |delta|`` is squared off with two points."""
    pts = [(float(x), float(y)) for x, y in poly]
    if _signed_area(pts) < 0:                      # work counter-clockwise; restore the order at the end
        pts = pts[::-1]
        flipped = True
    else:
        flipped = False
    n = len(pts)
    out = []
    for i in range(n):
        p0, p1, p2 = pts[i - 1], pts[i], pts[(i + 1) % n]
        e1 = (p1[0] - p0[0], p1[1] - p0[1])
        e2 = (p2[0] - p1[0], p2[1] - p1[1])
        l1, l2 = math.hypot(*e1), math.hypot(*e2)
        n1 = (e1[1] / l1, -e1[0] / l1)             # outward normals of a CCW polygon
        n2 = (e2[1] / l2, -e2[0] / l2)
        cos_t = n1[0] * n2[0] + n1[1] * n2[1]
        denom = 1.0 + cos_t
        if denom < 1e-12:                          # 180 degree turn-back: square off
            out.append((p1[0] + delta * n1[0], p1[1] + delta * n1[1]))
            out.append((p1[0] + delta * n2[0], p1[1] + delta * n2[1]))
            continue
        mx, my = (n1[0] + n2[0]) / denom, (n1[1] + n2[1]) / denom      # mitre vector per unit delta
        if math.hypot(mx, my) > miter_limit:
            out.append((p1[0] + delta * n1[0], p1[1] + delta * n1[1]))
            out.append((p1[0] + delta * n2[0], p1[1] + delta * n2[1]))
        else:
            out.append((p1[0] + delta * mx, p1[1] + delta * my))
    return out[::-1] if flipped else out


def _seg_intersect_strict(a, b, c, d):
    """Proper crossing of open segments ab and cd (touching at endpoints / collinear overlap is not a crossing)."""
    def orient(p, q, r):
        return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
    o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
    return (o1 * o2 < -_EPS) and (o3 * o4 < -_EPS)


def _point_in_polygon(p, poly, strict=True):
    """Even-odd test; points on the boundary count as outside when ``strict``."""
    x, y = p
    n = len(poly)
    for i in range(n):                              # on an edge?
        x1, y1 = poly[i]
        x2, y2 = poly[(i + 1) % n]
        cross = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
        if abs(cross) <= 1e-9 * max(1.0, math.hypot(x2 - x1, y2 - y1)):
            if min(x1, x2) - 1e-9 <= x <= max(x1, x2) + 1e-9 and min(y1, y2) - 1e-9 <= y <= max(y1, y2) + 1e-9:
                return not strict
    inside = False
    for i in range(n):
        x1, y1 = poly[i]
        x2, y2 = poly[(i + 1) % n]
        if (y1 > y) != (y2 > y):
            xi = x1 + (y - y1) * (x2 - x1) / (y2 - y1)
            if xi > x:
                inside = not inside
    return inside


class VisibilityPlanner:
    """Counterpart of ``PathPreProcessor.prepare`` + ``get_initial_guess`` (visibility.py:49-88,126-139)."""

    def __init__(self, cfg: Config, boundary, obstacles, dyn_obs_list=()):
        self.cfg = cfg
        self.original_boundary = [tuple(map(float, p)) for p in boundary]
        self.original_obstacles = [[tuple(map(float, p)) for p in o] for o in obstacles]
        self.dyn_obs_list = list(dyn_obs_list)
        w = float(cfg.vehicle_width)
        self.obstacles = [offset_polygon(o, +w) for o in self.original_obstacles]          # (:97)
        self.boundary = offset_polygon(self.original_boundary, -w)                          # (:59-61)
        self.nodes = []
        for poly in self.obstacles:
            self.nodes += self._extremities(poly, hole=True)
        self.nodes += self._extremities(self.boundary, hole=False)

    @staticmethod
    def _extremities(poly, hole):
        """Corners a shortest path can bend around: convex corners of obstacles, reflex corners of the boundary."""
        ccw = _signed_area(poly) > 0
        out = []
        n = len(poly)
        for i in range(n):
            p0, p1, p2 = poly[i - 1], poly[i], poly[(i + 1) % n]
            cross = (p1[0] - p0[0]) * (p2[1] - p1[1]) - (p1[1] - p0[1]) * (p2[0] - p1[0])
            convex = cross > 1e-12 if ccw else cross < -1e-12
            if convex == hole:
                out.append(p1)
        return out

    def _free(self, a, b):
        """Is the open segment ab collision free (outside every inflated obstacle, inside the boundary)?"""
        if math.hypot(a[0] - b[0], a[1] - b[1]) < 1e-12:
            return True
        polys = self.obstacles + [self.boundary]
        for poly in polys:
            n = len(poly)
            for i in range(n):
                if _seg_intersect_strict(a, b, poly[i], poly[(i + 1) % n]):
                    return False
        for s in (0.5, 0.25, 0.75, 0.0625, 0.9375):          # sample the interior against containment
            m = (a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]))
            if any(_point_in_polygon(m, o, strict=True) for o in self.obstacles):
                return False
            if not _point_in_polygon(m, self.boundary, strict=False):
                return False
        return True

    def shortest_path(self, start, goal):
        """A* over the visibility graph; -> (waypoints incl. start and goal, length)."""
        s, g = (float(start[0]), float(start[1])), (float(goal[0]), float(goal[1]))
        pts = [s, g] + self.nodes
        n = len(pts)
        vis = {}

        def visible(i, j):
            key = (i, j) if i < j else (j, i)
            if key not in vis:
                vis[key] = self._free(pts[i], pts[j])
            return vis[key]

        def h(i):
            return math.hypot(pts[i][0] - g[0], pts[i][1] - g[1])
        dist = {0: 0.0}
        prev = {}
        heap = [(h(0), 0)]
        done = set()
        while heap:
            _, i = heapq.heappop(heap)
            if i in done:
                continue
            done.add(i)
            if i == 1:
                break
            for j in range(n):
                if j == i or j in done or not visible(i, j):
                    continue
                d = dist[i] + math.hypot(pts[i][0] - pts[j][0], pts[i][1] - pts[j][1])
                if d < dist.get(j, math.inf) - 1e-12:
                    dist[j], prev[j] = d, i
                    heapq.heappush(heap, (d + h(j), j))
        if 1 not in dist:
            raise ValueError("no collision-free path between start and goal")
        path, i = [], 1
        while True:
            path.append(pts[i])
            if i == 0:
                break
            i = prev[i]
        return path[::-1], dist[1]

    def original_vertices(self, path):
        """Closest original (un-inflated) vertex, obstacles and boundary alike, for each interior
        path corner (visibility.py:126-139)."""
        if len(path) <= 2:
            return []
        allv = [v for o in self.original_obstacles for v in o] + list(self.original_boundary)
        return [allv[harness.closest_index(c, allv)] for c in path[1:-1]]

    def route(self, start, end, sinus_object=False) -> harness.Route:
        path, _ = self.shortest_path(start[:2], end[:2])
        return harness.Route(self.cfg, tuple(start), tuple(end), path, self.original_vertices(path),
                             self.dyn_obs_list, sinus_object)


# scene data of the reference's 13 maps (src/visibility/graphs.py:21-191): boundary, obstacle polygons, default
# start / end poses and dynamic-obstacle lists -- a table of coordinates (scenes.json beside this file, written by
# tests/golden/make_scene_fixtures.py)
def _load_scenes():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "scenes.json")) as fh:
        raw = json.load(fh)
    out = {}
    for g in raw:
        out[g["index"]] = dict(boundary=[tuple(p) for p in g["boundary"]],
                               obstacles=[[tuple(p) for p in o] for o in g["obstacles"]],
                               start=tuple(g["start"]), end=tuple(g["end"]),
                               dyn_obs_list=[[tuple(o[0]), tuple(o[1])] + list(o[2:]) for o in g["dyn_obs_list"]])
    return out


SCENE_POLYGONS = _load_scenes()


def scene_planner(cfg: Config, scene: int) -> VisibilityPlanner:
    """Planner on scene 0..12 of the reference (``Graphs().get_graph(complexity)``, graphs.py:199-203)."""
    s = SCENE_POLYGONS[scene]
    return VisibilityPlanner(cfg, s["boundary"], s["obstacles"], s["dyn_obs_list"])


def random_routes(cfg: Config, scene: int, n: int, seed: int, min_length: float = 12.0):
    """``n`` routes between random collision-free start / goal points of a scene (BASELINE config 1:
    "randomized start/goal"), planned on the inflated polygons like the reference's front-end."""
    pl = scene_planner(cfg, scene)
    rng = np.random.Generator(np.random.PCG64(seed))
    xs = [p[0] for p in pl.boundary]
    ys = [p[1] for p in pl.boundary]

    def sample():
        while True:
            p = (rng.uniform(min(xs), max(xs)), rng.uniform(min(ys), max(ys)))
            if not _point_in_polygon(p, pl.boundary, strict=True):
                continue
            if any(_point_in_polygon(p, offset_polygon(o, 0.25), strict=False) for o in pl.obstacles):
                continue                                   # keep a little clear of the inflated obstacles
            return p
    out = []
    while len(out) < n:
        s, g = sample(), sample()
        try:
            path, length = pl.shortest_path(s, g)
        except ValueError:
            continue
        if length < min_length:
            continue
        th0 = math.atan2(path[1][1] - path[0][1], path[1][0] - path[0][0])
        th1 = math.atan2(path[-1][1] - path[-2][1], path[-1][0] - path[-2][0])
        out.append(harness.Route(cfg, (s[0], s[1], th0), (g[0], g[1], th1), path, pl.original_vertices(path)))
    return out


def random_fleet(cfg: Config, scene: int, R: int, B: int, seed: int):
    """A fleet of B robots on R routes of a scene, for ``DeviceRecedingHorizon`` / ``FleetRecedingHorizon``
    -> (routes, route_of [B] int32, starts [B, 3], idx0 [B] int32).

    ``random_routes(cfg, scene, R, seed)`` plans the routes; the robots are dealt to them as evenly as B allows
    (every route gets a robot when B >= R), in an order drawn from the seed.  Robot b starts at a reference
    sample idx0[b] of its own route (at least 25 samples before the end where the route is that long), with
    N(0, 0.05^2) m noise in x and y and N(0, 0.1^2) in the heading."""
    routes = random_routes(cfg, scene, R, seed)
    rng = np.random.Generator(np.random.PCG64([seed, 1]))
    route_of = rng.permutation(np.arange(B) % R).astype(np.int32)
    n = np.array([len(r.x_ref) for r in routes])[route_of]
    idx0 = rng.integers(0, np.maximum(1, n - 25)).astype(np.int32)
    ref = [np.stack([r.x_ref, r.y_ref, r.theta_ref], axis=1) for r in routes]
    base = np.stack([ref[r][i] for r, i in zip(route_of, idx0)]) if B else np.zeros((0, 3))
    starts = base + np.stack([rng.normal(0, 0.05, B), rng.normal(0, 0.05, B), rng.normal(0, 0.1, B)], axis=1)
    return routes, route_of, starts, idx0


# ---- batched planning: the rule of ``VisibilityPlanner._free`` / ``shortest_path`` in arithmetic the device reproduces bit for bit
# (unfused f64 + - * / and sqrt).  ``plan_batch_mirror`` is the NumPy statement, ``DevicePlanner`` the kernels.
PLAN_MAX_NODES = 254        # V: a query has V + 2 points, four per lane of a wave at the most
PLAN_MAX_EDGES = 1024       # E: the edges are staged in LDS
_SAMPLES = (0.5, 0.25, 0.75, 0.0625, 0.9375)


@dataclasses.dataclass
class PlanScene:
    """What the planner kernels read of a ``VisibilityPlanner``: ``nodes`` [V, 2], every polygon edge ``edges`` [E, 4] = (x1, y1, x2, y2)
    with the obstacles first and the deflated boundary last, ``poly_off`` [n_poly + 1] and ``node_vertex`` [V, 2], the closest
    original vertex of each node (``original_vertices`` per node: static, so computed here)."""
    nodes: np.ndarray
    edges: np.ndarray
    poly_off: np.ndarray
    node_vertex: np.ndarray
    _nn: object = None

    @property
    def visibility(self):
        """Node-node visibility [V, V] uint8 by the mirror's segment test: entry (i, j) judges the segment from node i to node j."""
        if self._nn is None:
            V = len(self.nodes)
            i, j = np.divmod(np.arange(V * V), max(V, 1))
            self._nn = _free_batch(self, self.nodes[i], self.nodes[j]).reshape(V, V).astype(np.uint8)
        return self._nn


def plan_scene(planner: VisibilityPlanner) -> PlanScene:
    """The ``PlanScene`` of a planner (kept on the planner: it is static); ValueError beyond V <= 254 nodes or E <= 1024 edges."""
    sc = getattr(planner, "_plan_scene", None)
    if sc is not None:
        return sc
    edges, off = map_edges(planner, inflated=True)
    V, E = len(planner.nodes), len(edges)
    if V > PLAN_MAX_NODES or E > PLAN_MAX_EDGES:
        raise ValueError(f"scene with {V} nodes and {E} edges: the batched planner takes {PLAN_MAX_NODES} and {PLAN_MAX_EDGES} at the most")
    nodes = np.array(planner.nodes, dtype=np.float64).reshape(V, 2)
    allv = [v for o in planner.original_obstacles for v in o] + list(planner.original_boundary)
    nv = np.array([allv[harness.closest_index(c, allv)] for c in planner.nodes], dtype=np.float64).reshape(V, 2)
    sc = planner._plan_scene = PlanScene(nodes, edges, off, nv)
    return sc


def map_edges(planner: VisibilityPlanner, inflated: bool = False):
    """-> (edges [E, 4] = (x1, y1, x2, y2), poly_off [n_poly + 1] int32) of a planner's scene in the ``nmpc_scene`` layout, the obstacles
    first and the boundary last: what ``trajectory.MapMonitor`` takes.  By default the ORIGINAL obstacles and boundary, the true walls;
    ``inflated=True``: the polygons the planner plans on, where a hit means "closer than ``vehicle_width``"."""
    if inflated:
        polys = list(planner.obstacles) + [planner.boundary]
    else:
        polys = list(planner.original_obstacles) + [planner.original_boundary]
    edges = np.array([[*poly[i], *poly[(i + 1) % len(poly)]] for poly in polys for i in range(len(poly))], dtype=np.float64).reshape(-1, 4)
    off = np.zeros(len(polys) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in polys])
    return edges, off


def _free_batch(sc: PlanScene, a, b, chunk=8192):
    """``VisibilityPlanner._free`` for S segments a[s] -> b[s] at once -> bool [S].  Every comparison keeps the sense it has in the
    literal code, so one that is false because of a NaN has the same consequence."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 2), np.asarray(b, dtype=np.float64).reshape(-1, 2)
    if len(a) > chunk:
        return np.concatenate([_free_batch(sc, a[i:i + chunk], b[i:i + chunk], chunk) for i in range(0, len(a), chunk)])
    x1, y1, x2, y2 = (sc.edges[:, k][None, :] for k in range(4))
    ex, ey = x2 - x1, y2 - y1
    with np.errstate(all="ignore"):
        ax, ay, bx, by = a[:, 0:1], a[:, 1:2], b[:, 0:1], b[:, 1:2]
        dx, dy = ax - bx, ay - by
        short = (np.sqrt(dx * dx + dy * dy) < 1e-12)[:, 0]
        # proper crossing with any edge (_seg_intersect_strict)
        ux, uy = bx - ax, by - ay
        o1 = ux * (y1 - ay) - uy * (x1 - ax)
        o2 = ux * (y2 - ay) - uy * (x2 - ax)
        o3 = ex * (ay - y1) - ey * (ax - x1)
        o4 = ex * (by - y1) - ey * (bx - x1)
        blocked = ((o1 * o2 < -_EPS) & (o3 * o4 < -_EPS)).any(axis=1)
        # the interior samples against containment (_point_in_polygon: on an edge first, then the even-odd crossing)
        h = np.sqrt(ex * ex + ey * ey)
        tol = 1e-9 * np.where(h > 1.0, h, 1.0)
        xlo, xhi = np.where(x2 < x1, x2, x1) - 1e-9, np.where(x2 > x1, x2, x1) + 1e-9
        ylo, yhi = np.where(y2 < y1, y2, y1) - 1e-9, np.where(y2 > y1, y2, y1) + 1e-9
        n_poly = len(sc.poly_off) - 1
        for s in _SAMPLES:
            x, y = ax + s * (bx - ax), ay + s * (by - ay)
            cross = ex * (y - y1) - ey * (x - x1)
            on = (np.abs(cross) <= tol) & (xlo <= x) & (x <= xhi) & (ylo <= y) & (y <= yhi)
            straddle = (y1 > y) != (y2 > y)
            xi = x1 + ((y - y1) * ex) / np.where(straddle, ey, 1.0)
            hit = straddle & (xi > x)
            for k in range(n_poly):
                lo, hi = sc.poly_off[k], sc.poly_off[k + 1]
                on_k = on[:, lo:hi].any(axis=1)
                inside = (hit[:, lo:hi].sum(axis=1) & 1).astype(bool)
                if k < n_poly - 1:
                    blocked |= ~on_k & inside              # strictly inside an obstacle
                else:
                    blocked |= ~(on_k | inside)            # not inside the boundary, its edges counting as inside
    return short | ~blocked


@dataclasses.dataclass
class PlanResult:
    """B queries' answers.  The points of a query are [start, goal] + nodes, n = V + 2:
    ``n_wp`` [B] int32 waypoints of the path, 0 = no path; ``wp`` [B, n] int32 their point indices from 0 to 1, -1 behind them;
    ``length`` [B] the path's length (+inf: no path); ``vis`` [B, 2V + 1] uint8 the visibility of the query's own segments
    (start, node k), (goal, node k), (start, goal)."""
    n_wp: np.ndarray
    wp: np.ndarray
    length: np.ndarray
    vis: np.ndarray


def _query_points(starts, goals):
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 2))
    goals = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(-1, 2))
    if len(starts) != len(goals):
        raise ValueError(f"{len(starts)} starts for {len(goals)} goals")
    return starts, goals


def plan_batch_mirror(planner: VisibilityPlanner, starts, goals) -> PlanResult:
    """Shortest visibility-graph paths for B queries at once (starts, goals [B, 2]), the host mirror of ``DevicePlanner.plan``.
    Segments are judged by ``_free``'s rule (``_free_batch``); the search is Dijkstra with a fixed tie rule in place of
    ``shortest_path``'s A*: at most n rounds, each settling the unsettled point with the smallest (dist, index), stopping when that
    distance is not finite (no path) or the point is the goal, and relaxing every unsettled visible j on the strict
    ``dist[i] + sqrt(dx*dx + dy*dy) < dist[j]``."""
    sc = plan_scene(planner)
    starts, goals = _query_points(starts, goals)
    B, V = len(starts), len(sc.nodes)
    n = V + 2
    # the query's own segments: (start, node k), (goal, node k), (start, goal)
    a = np.concatenate([np.repeat(starts[:, None], V, 1), np.repeat(goals[:, None], V, 1), starts[:, None]], axis=1)
    b = np.concatenate([np.broadcast_to(sc.nodes[None], (B, V, 2))] * 2 + [goals[:, None]], axis=1)
    vis = _free_batch(sc, a.reshape(-1, 2), b.reshape(-1, 2)).reshape(B, 2 * V + 1).astype(np.uint8)
    nn = sc.visibility.astype(bool)
    nn = np.where(np.arange(V)[:, None] <= np.arange(V)[None, :], nn, nn.T)      # a pair is judged from its lower index, as `visible` does
    pts = np.concatenate([starts[:, None], goals[:, None], np.broadcast_to(sc.nodes[None], (B, V, 2))], axis=1)
    dist = np.full((B, n), np.inf)
    dist[:, 0] = 0.0
    prev = np.full((B, n), -1, dtype=np.int32)
    settled = np.zeros((B, n), dtype=bool)
    live = np.ones(B, dtype=bool)
    rows = np.arange(B)
    # who the start, the goal and (below) a node see among the n points; a point's own entry is never read
    sg, no = vis[:, 2 * V:] != 0, np.zeros((B, 1), dtype=bool)
    row_s = np.concatenate([no, sg, vis[:, :V] != 0], axis=1)
    row_g = np.concatenate([sg, no, vis[:, V:2 * V] != 0], axis=1)
    with np.errstate(all="ignore"):
        for _ in range(n):
            if not live.any():
                break
            masked = np.where(settled, np.inf, dist)
            i = np.argmin(masked, axis=1)                                         # the first minimum: (dist, index) order
            d = masked[rows, i]
            live &= d < np.inf                                                    # nothing reachable is left: no path
            settled[rows[live], i[live]] = True
            live &= i != 1
            row = np.where((i == 0)[:, None], row_s, row_g)
            if V:
                k = np.maximum(i - 2, 0)
                row_n = np.concatenate([vis[rows, k][:, None] != 0, vis[rows, V + k][:, None] != 0, nn[k]], axis=1)
                row = np.where((i >= 2)[:, None], row_n, row)
            dx, dy = pts[rows, i, 0:1] - pts[:, :, 0], pts[rows, i, 1:2] - pts[:, :, 1]
            cand = d[:, None] + np.sqrt(dx * dx + dy * dy)
            take = live[:, None] & ~settled & row & (cand < dist)
            dist[take] = cand[take]
            prev[take] = np.broadcast_to(i[:, None].astype(np.int32), (B, n))[take]
    n_wp = np.zeros(B, dtype=np.int32)
    wp = np.full((B, n), -1, dtype=np.int32)
    for q in np.nonzero(settled[:, 1])[0]:
        path, j = [1], 1
        for _ in range(n):                                                        # the walk back is bounded like the device's
            if j == 0:
                break
            j = int(prev[q, j])
            path.append(j)
        n_wp[q] = len(path)
        wp[q, :len(path)] = path[::-1]
    return PlanResult(n_wp, wp, dist[:, 1].copy(), vis)


def plan_routes(planner: VisibilityPlanner, res: PlanResult, starts, ends, sinus_object=False):
    """The ``harness.Route`` of every query of a ``PlanResult`` (starts, ends [B, 3] poses whose (x, y) were the queries), what
    ``VisibilityPlanner.route`` builds from ``shortest_path``: waypoints = the coordinates of ``wp``, vertices = ``node_vertex`` of the
    interior waypoints, the planner's ``dyn_obs_list``.  ValueError naming the first robot without a path."""
    sc = plan_scene(planner)
    starts, ends = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    bad = np.nonzero(res.n_wp == 0)[0]
    if len(bad):
        raise ValueError(f"robot {int(bad[0])}: no collision-free path between start and goal")
    nv = [tuple(map(float, v)) for v in sc.node_vertex]
    out = []
    for b in range(len(starts)):
        s, e = tuple(map(float, starts[b])), tuple(map(float, ends[b]))
        pts = [s[:2], e[:2]] + planner.nodes
        idx = [int(j) for j in res.wp[b, :res.n_wp[b]]]
        out.append(harness.Route(planner.cfg, s, e, [pts[j] for j in idx], [nv[j - 2] for j in idx[1:-1]], planner.dyn_obs_list, sinus_object))
    return out


class DevicePlanner:
    """``plan_batch_mirror`` on the GPU: the planner kernels of libnmpc_hip.so (``nmpc_planner_*`` / ``nmpc_plan_batch_*``,
    include/nmpc_solver.h; csrc/nmpc_plan.h), bit for bit the mirror's answers (tests/test_gpu_plan.py).  The scene goes to the device
    once, where its node-node visibility is judged; ``plan`` then answers up to ``max_batch`` queries per call.  There is no CPU
    fall-back: without a HIP device the constructor raises."""

    def __init__(self, planner: VisibilityPlanner, device: int = 0, max_batch: int = 8192):
        self.planner, self.scene = planner, plan_scene(planner)
        self.max_batch = int(max_batch)
        self.lib = _lib.load_library()
        sc = self.scene
        self.V = len(sc.nodes)
        nodes, edges, off = (np.ascontiguousarray(sc.nodes, dtype=np.float64), np.ascontiguousarray(sc.edges, dtype=np.float64),
                             np.ascontiguousarray(sc.poly_off, dtype=np.int32))
        s = _lib.NmpcScene(self.V, len(edges), len(off) - 1, 0, _lib.as_dp(nodes), _lib.as_dp(edges), _lib.as_i32p(off))
        h = C.c_void_p()
        rc = self.lib.nmpc_planner_new(C.byref(s), int(device), self.max_batch, C.byref(h))
        if rc != 0:
            raise SolverError(rc, f"nmpc_planner_new failed: {_lib.ERRORS.get(rc, rc)} (this package needs a HIP device; there is no CPU fallback)")
        self._pl = h

    def _check(self, rc, what):
        if rc != 0:
            raise SolverError(rc, f"{what}: {_lib.ERRORS.get(rc, rc)}")

    def close(self):
        if getattr(self, "_pl", None):
            self.lib.nmpc_planner_free(self._pl)
            self._pl = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def last_ms(self):
        """Kernel time of the last ``plan`` call, in ms (HIP events around its two launches)."""
        return float(self.lib.nmpc_planner_last_ms(self._pl))

    def visibility(self):
        """The node-node visibility [V, V] uint8 as the device judged it."""
        vis = np.zeros((self.V, self.V), dtype=np.uint8)
        self._check(self.lib.nmpc_planner_visibility(self._pl, vis.ctypes.data_as(C.POINTER(C.c_uint8))), "nmpc_planner_visibility")
        return vis

    def plan(self, starts, goals) -> PlanResult:
        """starts, goals [B, 2] -> ``PlanResult``, B <= max_batch."""
        starts, goals = _query_points(starts, goals)
        B, n = len(starts), self.V + 2
        res = PlanResult(np.zeros(B, dtype=np.int32), np.full((B, n), -1, dtype=np.int32), np.full(B, np.inf), np.zeros((B, 2 * self.V + 1), dtype=np.uint8))
        self._check(self.lib.nmpc_plan_batch_host(self._pl, B, _lib.as_dp(starts), _lib.as_dp(goals), _lib.as_i32p(res.n_wp), _lib.as_i32p(res.wp),
                                                  _lib.as_dp(res.length), res.vis.ctypes.data_as(C.POINTER(C.c_uint8))), "nmpc_plan_batch_host")
        return res

    def routes(self, starts, ends, sinus_object=False):
        """starts, ends [B, 3] poses -> a ``harness.Route`` per robot from its start to its end (``plan_routes`` of ``plan``), as
        ``VisibilityPlanner.route`` builds one; ValueError naming the first robot without a path."""
        starts, ends = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(ends, dtype=np.float64).reshape(-1, 3)
        return plan_routes(self.planner, self.plan(starts[:, :2], ends[:, :2]), starts, ends, sinus_object)
