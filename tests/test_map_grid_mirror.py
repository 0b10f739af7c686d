"""The map monitor through a grid on the host (``MapMonitor(edges, poly_off, cell=H, range=R)``, ``MapMonitor.rows_grid``; DESIGN.md
section 5.9).

The three claims of the section, on every map used here: the failing polygon is the all-edges rule's, the wall record is the all-edges
rule's wherever a wall is closer than ``range`` (+inf elsewhere), and with a ``range`` beyond every distance ``scan`` gives the all-edges
records bit for bit.  The all-edges rule is ``MapMonitor.rows`` without a ``cell`` up to its 1024 edges (pinned to the literal rule by
tests/test_map_monitor_mirror.py) and, for the maps no all-edges call accepts, ``brute_rows``: the literal rule of the section over every
edge, written here.  tests/test_gpu_map_grid_loop.py runs the device against this mirror."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mpc_trajectory_generator_amd import _lib, named_config
from mpc_trajectory_generator_amd import trajectory
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, MapMonitor, wall_grid
from mpc_trajectory_generator_amd.workloads import map_clearance_differing, subdivided_map
from test_map_monitor_mirror import _square, grid_map, scene_map, three_routes_fleet

CELLS = (0.3, 1.0, 7.0, 1e3, 0.01)      # the last one would need more than 512 cells per axis: the cap sets h
RANGES = (0.25, 2.0, 1e3)
HIT_LIST = 512                          # MAP_GRID_HITS of csrc/nmpc_loop.h: the ray hits on obstacle edges the kernel's LDS list holds


def gon61_map():
    """An obstacle of 61 edges in the middle of scene 11's extent and a rectangle around it."""
    a = 2 * np.pi * np.arange(61) / 61
    c = np.stack([30 + 2 * np.cos(a), 30 + 2 * np.sin(a)], axis=1)
    gon = [[*c[i], *c[(i + 1) % 61]] for i in range(61)]
    return MapMonitor(np.array(gon + _square(2.5, 0, 60, 60), dtype=np.float64), [0, 61, 65])


def small_maps():
    """name -> a ``MapMonitor`` without a cell: all 13 scenes, the 1024-edge lattice, the 61-gon, scene 11 cut into 4 and 39 pieces"""
    cfg = named_config("cfg1")
    out = {f"scene{k}": scene_map(cfg, k) for k in range(13)}
    out["grid1024"] = grid_map((28.5, 32.5))
    out["gon61"] = gon61_map()
    m = scene_map(cfg, 11)
    for pieces in (4, 39):
        out[f"scene11x{pieces}"] = MapMonitor(*subdivided_map(m.edges, m.poly_off, pieces))
    return out


MAPS = small_maps()


def brute_rows(edges, off, ax, ay, x, y, chunk=16):
    """The all-edges rule of DESIGN.md section 5.9 for n row pairs, ``chunk`` of them at a time against every edge -> (v, e, poly) as
    ``MapMonitor.rows`` returns them; no limit on the edges."""
    edges, off = np.asarray(edges, dtype=np.float64), np.asarray(off, dtype=np.intp)
    x1, y1, x2, y2 = (edges[:, k][None, :] for k in range(4))
    ex, ey = x2 - x1, y2 - y1
    L2 = ex * ex + ey * ey
    vs, es, polys = [], [], []
    with np.errstate(all="ignore"):
        for i in range(0, len(x), chunk):
            X, Y, AX, AY = (np.asarray(a, dtype=np.float64)[i:i + chunk, None] for a in (x, y, ax, ay))
            t = ((X - x1) * ex + (Y - y1) * ey) / np.where(L2 > 0, L2, 1.0)
            t = np.where(t < 0, 0.0, t)
            t = np.where(t > 1, 1.0, t)
            t = np.where(L2 > 0, t, 0.0)
            dx, dy = X - (x1 + t * ex), Y - (y1 + t * ey)
            v = dx * dx + dy * dy
            v = np.where(np.isnan(v), np.inf, v)
            e = np.argmin(v, axis=1)
            ux, uy = X - AX, Y - AY
            o1 = ux * (y1 - AY) - uy * (x1 - AX)
            o2 = ux * (y2 - AY) - uy * (x2 - AX)
            o3 = ex * (AY - y1) - ey * (AX - x1)
            o4 = ex * (Y - y1) - ey * (X - x1)
            crossed = (o1 * o2 < -1e-9) & (o3 * o4 < -1e-9)
            straddle = (y1 > Y) != (y2 > Y)
            xi = x1 + ((Y - y1) * (x2 - x1)) / np.where(straddle, y2 - y1, 1.0)
            fails = (np.add.reduceat((straddle & (xi > X)).astype(np.int32), off[:-1], axis=1) & 1).astype(bool)
            fails[:, -1] = ~fails[:, -1]
            fails |= np.add.reduceat(crossed.astype(np.int32), off[:-1], axis=1) > 0
            vs.append(v[np.arange(len(e)), e])
            es.append(e)
            polys.append(np.where(fails.any(axis=1), np.argmax(fails, axis=1), -1))
    return np.concatenate(vs), np.concatenate(es).astype(np.int32), np.concatenate(polys).astype(np.int32)


def placed_pairs(m, rng):
    """-> (ax, ay, x, y) [n]: seeded row pairs over the map ``m`` -- random ones, and poses on a vertex, on an edge, level with a vertex,
    on the cell borders of every grid of ``CELLS``, far outside, pairs that jump through a wall, and NaN and +-inf in each coordinate"""
    edges = np.asarray(m.edges, dtype=np.float64)
    lo, hi = edges.reshape(-1, 2).min(axis=0), edges.reshape(-1, 2).max(axis=0)
    P = [rng.uniform(lo - 1.5, hi + 1.5) for _ in range(40)]
    A = [p + rng.uniform(-0.4, 0.4, 2) for p in P]
    pick = rng.integers(0, len(edges), 6)
    for e in edges[pick]:
        c, d = e[:2], e[2:]
        mid = 0.5 * (c + d)
        nrm = np.array([-(d - c)[1], (d - c)[0]]) / max(np.hypot(*(d - c)), 1e-300)
        P += [c.copy(), mid, np.array([rng.uniform(lo[0], hi[0]), c[1]]), mid + 0.3 * nrm, mid + 0.01 * nrm]
        A += [c + rng.uniform(-0.3, 0.3, 2), mid - 0.2 * nrm, mid, mid - 0.3 * nrm, mid - 0.01 * nrm]
    for cell in CELLS:                  # exactly on a border of the grid of this cell, in x and in y
        g = wall_grid(edges, cell)
        for k in (1, max(1, g.nx // 2)):
            P.append(np.array([g.origin[0] + k * g.h[0], rng.uniform(lo[1], hi[1])]))
            A.append(P[-1] + rng.uniform(-0.3, 0.3, 2))
        for k in (1, max(1, g.ny // 2)):
            P.append(np.array([rng.uniform(lo[0], hi[0]), g.origin[1] + k * g.h[1]]))
            A.append(P[-1] + rng.uniform(-0.3, 0.3, 2))
    for far in ((1e4, 0.0), (-3e3, 2e3), (0.0, -1e6), (1e7, 1e7)):
        P.append(hi + np.array(far))
        A.append(P[-1] + 0.1)
    inside = 0.5 * (lo + hi)
    for bad in (math.nan, math.inf, -math.inf):
        for k in range(4):
            q = [inside[0] + 0.1, inside[1], inside[0], inside[1] + 0.2]
            q[k] = bad
            A.append(np.array(q[:2]))
            P.append(np.array(q[2:]))
    A, P = np.array(A), np.array(P)
    return A[:, 0].copy(), A[:, 1].copy(), P[:, 0].copy(), P[:, 1].copy()


def assert_grid_rows_equal(got, want, r2, what):
    """``got`` = (v, e, poly) of the grid rule, ``want`` of the all-edges rule: the polygon everywhere, (v, e) wherever v < range^2"""
    (v, e, poly), (wv, we, wpoly) = got, want
    bad = np.nonzero(poly != wpoly)[0]
    assert not len(bad), f"{what}: failing polygon differs at pairs {bad[:8]}: {poly[bad[:8]]} != {wpoly[bad[:8]]}"
    near = wv < r2
    assert np.array_equal(v[near], wv[near]) and np.array_equal(e[near], we[near]), f"{what}: wall record differs"
    assert (v[~near] == np.inf).all(), f"{what}: a wall beyond the range was recorded"


@pytest.mark.parametrize("name", list(MAPS))
def test_grid_rule_equals_all_edges_rule(name):
    m = MAPS[name]
    pairs = placed_pairs(m, np.random.default_rng(sorted(MAPS).index(name)))
    want = m.rows(*pairs)
    assert (want[2] >= 0).any() and (want[2] < 0).any() and np.isfinite(want[0]).any()
    n = len(pairs[0])
    looked = []
    for cell in CELLS:
        for rng_ in RANGES:
            g = MapMonitor(m.edges, m.poly_off, cell=cell, range=rng_)
            v, e, poly, seen = g.rows_grid(*pairs)
            assert_grid_rows_equal((v, e, poly), want, rng_ * rng_, f"{name} cell {cell} range {rng_}")
            assert ((seen >= 0) & (seen <= len(m.edges))).all()
            looked.append(seen.mean())
        # a range beyond every distance of the near poses: scan is the all-edges scan, bit for bit (4 robots, rows in the pairs' order;
        # row r against row r - 1 of the table, so the table is scanned as it stands)
        T = np.zeros((n // 4, 4, 3))
        T[:, :, 0], T[:, :, 1] = pairs[2][:4 * (n // 4)].reshape(-1, 4), pairs[3][:4 * (n // 4)].reshape(-1, 4)
        bad = map_clearance_differing(MapMonitor(m.edges, m.poly_off, cell=cell, range=1e3).scan(T), m.scan(T))
        assert not bad, f"{name} cell {cell}: scan differs in {bad}"
    g = MapMonitor(m.edges, m.poly_off, cell=0.01, range=1.0).grid
    assert max(g.nx, g.ny) == trajectory.WALL_GRID_CAP and g.h.max() > 0.01
    print(name, len(m.edges), "edges; mean looked per (cell, range):", [round(float(q), 1) for q in looked])
    assert looked[0] < len(m.edges), "the finest grid looked at every edge on average"


def lattice_map(nx, ny):
    """nx x ny unit squares on a 2 m pitch inside a rectangle a metre around them -> (edges [4 nx ny + 4, 4], poly_off)"""
    i, j = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"))
    x0, y0 = 2 * i, 2 * j
    sq = np.stack([np.stack([x0, y0, x0 + 1, y0], 1), np.stack([x0 + 1, y0, x0 + 1, y0 + 1], 1),
                   np.stack([x0 + 1, y0 + 1, x0, y0 + 1], 1), np.stack([x0, y0 + 1, x0, y0], 1)], axis=1).reshape(-1, 4)
    edges = np.concatenate([sq, np.array(_square(-1, -1, 2 * nx, 2 * ny), dtype=np.float64)])
    return edges, np.arange(0, len(edges) + 1, 4, dtype=np.int32)


def test_a_map_no_all_edges_call_accepts():
    """160 x 160 squares and a boundary, 102404 edges and 25601 polygons, against the literal rule over every edge on 256 seeded pairs."""
    edges, off = lattice_map(160, 160)
    assert len(edges) == 102404 and len(off) - 1 == 25601
    with pytest.raises(ValueError):
        MapMonitor(edges, off).checked()
    rng = np.random.default_rng(7)
    P = rng.uniform(-3.0, 322.0, (256, 2))
    A = P + rng.uniform(-0.6, 0.6, (256, 2))
    want = brute_rows(edges, off, A[:, 0], A[:, 1], P[:, 0], P[:, 1])
    n_obst, n_out = int(((want[2] >= 0) & (want[2] < 25600)).sum()), int((want[2] == 25600).sum())
    print("pairs failing an obstacle", n_obst, "the boundary", n_out, "none", int((want[2] < 0).sum()))
    assert n_obst > 20 and n_out > 0 and (want[2] < 0).sum() > 20
    for cell, rng_ in ((2.0, 1.0), (0.3, 0.25)):
        m = MapMonitor(edges, off, cell=cell, range=rng_)
        v, e, poly, seen = m.rows_grid(A[:, 0], A[:, 1], P[:, 0], P[:, 1])
        assert_grid_rows_equal((v, e, poly), want, rng_ * rng_, f"cell {cell}")
        assert seen.max() < 200, "a pose looked at a large part of the map"


def fence_map(n=300):
    """``n`` rectangles 0.04 m thick and 1 m tall, 0.1 m apart, in a room -> (edges, poly_off); rectangle k spans x = 0.1 k .. 0.1 k + 0.04"""
    edges = [e for k in range(n) for e in _square(0.1 * k, 0.0, 0.1 * k + 0.04, 1.0)] + _square(-2.0, -2.0, 0.1 * n + 2.0, 3.0)
    return np.array(edges, dtype=np.float64), np.arange(0, 4 * n + 5, 4, dtype=np.int32)


def test_a_fence_of_more_rectangles_than_half_the_hit_list():
    """The ray of a pose left of 300 rectangles meets 600 obstacle edges, more than ``HIT_LIST``: only the rectangle a pose stands in may
    fail."""
    n, k = 300, 137
    assert 2 * n > HIT_LIST
    edges, off = fence_map(n)
    x = np.array([-0.5, 0.1 * k + 0.02, 0.1 * k + 0.07])
    y = np.full(3, 0.5)
    want = brute_rows(edges, off, x, y, x, y)
    assert want[2].tolist() == [-1, k, -1]
    assert int(((edges[:-4, 1] > 0.5) != (edges[:-4, 3] > 0.5)).sum()) == 2 * n          # what the first pose's ray meets
    for cell in (1.0, 0.05, 1e3):
        m = MapMonitor(edges, off, cell=cell, range=0.5)
        assert_grid_rows_equal(m.rows(x, y, x, y), want, 0.25, f"cell {cell}")


def test_fleet_mirror_with_a_cell_keeps_the_all_edges_records():
    """The stepping mirror with and without a cell over scene 11: the records bit for bit at every step (range beyond every distance), and
    ``map_looked`` counts fewer edges than the map has."""
    cfg = named_config("cfg1")
    m = scene_map(cfg, 11)
    _, o, plain = three_routes_fleet(m)
    _, _, grid = three_routes_fleet(MapMonitor(m.edges, m.poly_off, cell=1.0, range=1e3))
    _, _, near = three_routes_fleet(MapMonitor(m.edges, m.poly_off, cell=1.0, range=2.0))
    for k in range(4):
        for f in (plain, grid, near):
            f.step(o.warm_solve())
        assert not map_clearance_differing(grid.map_clearance, plain.map_clearance), f"step {k}"
        assert np.array_equal(near.map_clearance["hits"], plain.map_clearance["hits"])
        assert (grid.map_looked == 26).all() and (near.map_looked > 0).all() and (near.map_looked < 26).any()
    close = plain.map_clearance["wall2"] < 4.0
    assert close.any() and np.array_equal(near.map_clearance[close], plain.map_clearance[close])
    assert (near.map_clearance["wall2"][~close] == np.inf).all()


def test_checked_refusals_with_a_cell():
    tri = np.array([[0, 0, 4, 0], [4, 0, 0, 4], [0, 4, 0, 0]], dtype=np.float64)
    MapMonitor(tri, [0, 3], cell=1.0, range=2.0).checked()
    MapMonitor(np.zeros((1 << 20, 4)), [0, 1 << 20], cell=1.0, range=1.0).checked()
    with pytest.raises(ValueError, match="edges"):
        MapMonitor(np.zeros(((1 << 20) + 1, 4)), [0, (1 << 20) + 1], cell=1.0, range=1.0).checked()
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="finite and positive"):
            MapMonitor(tri, [0, 3], cell=bad, range=2.0).checked()
        with pytest.raises(ValueError, match="finite and positive"):
            MapMonitor(tri, [0, 3], cell=1.0, range=bad).checked()
    for kw in (dict(cell=1.0), dict(range=1.0)):
        with pytest.raises(ValueError, match="together"):
            MapMonitor(tri, [0, 3], **kw).checked()
    diagonals = np.tile([[0.0, 0.0, 100.0, 100.0]], (42, 1))                # each filed in 512 x 512 cells
    assert 42 * 512 * 512 > trajectory.WALL_GRID_MAX_ENTRIES == 1 << 23
    with pytest.raises(ValueError, match="larger cell or shorter edges"):
        MapMonitor(diagonals, [0, 42], cell=0.01, range=1.0).checked()
    MapMonitor(diagonals, [0, 42], cell=1.0, range=1.0).checked()


def test_map_grid_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_map_monitor_grid", "nmpc_loop_map_grid"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3 and re.search(r"#define\s+NMPC_ABI_VERSION\s+3\b", header)
    assert lib.nmpc_loop_set_map_monitor_grid(None, None, 1.0, 1.0) == -3 and lib.nmpc_loop_map_grid(None, None, None, None, None) == -3
