"""Walls found through a grid on the host (``Walls(..., cell=H)``, ``trajectory.wall_grid``).

The grid's structure against a literal per-edge, per-cell loop; on every map and cell, every edge the literal all-edges rule
(``test_walls_mirror.literal_walls``) finds within ``range`` is among the edges the robot looks at, and the mirror with a ``cell`` equals
the mirror without, bit for bit; hand-made edges and poses at the places where a grid can go wrong, each held to the literal rule; what
``Walls.checked`` accepts and refuses with a ``cell``; the two functions of the C ABI.

The fleets and maps are those of tests/test_walls_mirror.py, and tests/test_gpu_walls_grid_loop.py runs them on the device."""
import dataclasses
import math
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, named_config
from mpc_trajectory_generator_amd import trajectory
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, Walls, wall_grid
from test_walls_mirror import NAN_ROBOT, fleet24, literal_walls, nan_fleet, radius, same_bits, scene_map, walls_of

CELLS = (0.5, 2.0, 1e3)
PIECES = (1, 4, 40)


# ---- the grid's structure ----
def literal_cellof(v, o, h, n):
    t = (v - o) / h
    if not t > 0.0:
        return 0
    if t >= n:
        return n - 1
    return int(math.floor(t))


def check_structure(edges, cell):
    """``wall_grid`` against a loop over the edges and the cells of each one's rectangle -> the grid."""
    g = wall_grid(edges, cell)
    E = [tuple(float(v) for v in row) for row in edges]
    ox, oy = min(min(e[0], e[2]) for e in E), min(min(e[1], e[3]) for e in E)
    assert (float(g.origin[0]), float(g.origin[1])) == (ox, oy)
    for ax, o in ((0, ox), (1, oy)):
        ext = max(max(e[ax], e[ax + 2]) for e in E) - o
        n = (g.nx, g.ny)[ax]
        if ext / cell < trajectory.WALL_GRID_CAP:
            assert n == int(ext / cell) + 1 and g.h[ax] == cell
        else:
            assert n == trajectory.WALL_GRID_CAP and g.h[ax] == ext / trajectory.WALL_GRID_CAP
        assert n >= 1
    cells = [[] for _ in range(g.nx * g.ny)]
    for e, (x1, y1, x2, y2) in enumerate(E):
        c0, c1 = literal_cellof(min(x1, x2), ox, float(g.h[0]), g.nx), literal_cellof(max(x1, x2), ox, float(g.h[0]), g.nx)
        r0, r1 = literal_cellof(min(y1, y2), oy, float(g.h[1]), g.ny), literal_cellof(max(y1, y2), oy, float(g.h[1]), g.ny)
        assert g.rect[e].tolist() == [c0, c1, r0, r1]
        for j in range(r0, r1 + 1):
            for i in range(c0, c1 + 1):
                cells[j * g.nx + i].append(e)
    off = g.cell_off
    assert off.dtype == np.int32 == g.cell_edge.dtype and off.shape == (g.nx * g.ny + 1,)
    assert off[0] == 0 and off[-1] == g.entries == len(g.cell_edge) == sum(len(c) for c in cells) and (np.diff(off) >= 0).all()
    for c, want in enumerate(cells):                                       # exactly its rectangle's cells; ascending inside a cell
        assert g.cell_edge[off[c]:off[c + 1]].tolist() == want, c
    hdr = g.header()
    assert hdr.dtype == _lib.WALL_GRID_DTYPE and (int(hdr["nx"]), int(hdr["ny"]), int(hdr["entries"])) == (g.nx, g.ny, g.entries)
    return g


@pytest.mark.parametrize("pieces", PIECES)
def test_grid_structure_equals_literal_filing(pieces):
    cfg = named_config("cfg1")
    edges = scene_map(cfg, pieces)[0]
    assert len(edges) == 26 * pieces
    for cell in CELLS:
        g = check_structure(edges, cell)
        assert (g.nx * g.ny == 1) == (cell == 1e3)
    assert check_structure(edges, 0.5).entries > len(edges)                # some edge lies in several cells


def test_grid_structure_at_the_cap():
    """A cell of 1 cm would need more than ``WALL_GRID_CAP`` cells per axis: h grows, and cellof stays the one function."""
    cfg = named_config("cfg1")
    edges = scene_map(cfg, 4)[0]
    g = check_structure(edges, 0.01)
    assert g.nx == g.ny == trajectory.WALL_GRID_CAP == 512 and (g.h > 0.01).all()


def test_too_many_filings_are_refused():
    """Long diagonals over a fine grid: every edge is filed in 512 x 512 cells."""
    edges = np.tile([[0.0, 0.0, 100.0, 100.0]], (40, 1))
    with pytest.raises(ValueError, match="larger cell or shorter edges"):
        wall_grid(edges, 0.01)
    assert 40 * 512 * 512 > trajectory.WALL_GRID_MAX_ENTRIES == 1 << 23


# ---- nobody missed, nothing changed ----
def stepped(cfg, fleet_args, wl, steps, compare=True, **kw):
    """Step the mirror with a ``cell`` (and, if ``compare``, the one without beside it, held bit-equal) -> per step (the mirror's P, the
    told poses, U before the step, the predictions, wall_edge, wall_stage, wall_looked)."""
    o = oracle_for(cfg)
    routes, route_of, starts, i0 = fleet_args
    make = lambda w: FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, walls=w, **kw)      # noqa: E731
    grid, plain = make(wl), make(dataclasses.replace(wl, cell=None)) if compare else None
    out = []
    for k in range(steps):
        U = grid.U.copy()
        P, _ = grid.step(o.warm_solve())
        if compare:
            Pp, _ = plain.step(o.warm_solve())
            assert same_bits(P, Pp) and same_bits(grid.wall_edge, plain.wall_edge) and same_bits(grid.wall_stage, plain.wall_stage), f"step {k}"
            assert same_bits(grid.U, plain.U) and same_bits(grid.state, plain.state), f"step {k}"
        out.append((P.copy(), U, grid.wall_edge.copy(), grid.wall_stage.copy(), grid.wall_looked.copy()))
    return grid, out


def literal_candidates(cfg, wl, told, U, sincos):
    """-> per robot the set of edges with D < range^2 under the literal rule: its slots asked for are as many as the edges, its spacing 0,
    so every candidate is taken."""
    E, n, N = len(wl.edges), len(told), cfg.N_hor
    big = dataclasses.replace(wl, slots=E, spacing=0.0, cell=None)
    pad = np.zeros((n, 20 + N + 3 * E))
    fake = types.SimpleNamespace(N_hor=N, num_steps_taken=cfg.num_steps_taken, ts=cfg.ts, Nobs=E)     # E circle slots: room for every candidate
    _, edge, _, _ = literal_walls(fake, big, pad, told, U, sincos, np.ones(n, dtype=bool), [[-1] * E] * n, [[-1] * E] * n)
    return [set(e for e in row if e >= 0) for row in edge]


@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("rng_", [2.0, 3.0])
def test_nobody_missed_nothing_changed(pieces, rng_):
    """Four steps of ``fleet24``: at every step, every edge within ``range`` of a robot under the literal rule is among the edges its
    window holds, for every cell; and for E <= 1024 the mirror with a ``cell`` is the mirror without, bit for bit."""
    cfg = named_config("cfg1")
    o = oracle_for(cfg)
    base = walls_of(cfg, pieces=pieces, rng_=rng_, spacing=1.0 if pieces > 1 else 0.0)
    E = len(base.edges)
    grids = {cell: wall_grid(base.edges, cell) for cell in CELLS + (0.01,)}
    fleet, steps = stepped(cfg, fleet24(cfg), dataclasses.replace(base, cell=CELLS[0]), 4, compare=E <= 1024)
    some = 0
    for k, (P, U, _, _, looked) in enumerate(steps):
        told = P[:, 0:3]
        sub = np.arange(len(told))
        cand = literal_candidates(cfg, base, told[sub], U[sub], o.sincos_array)
        pred = _predictions(cfg, told, U, o.sincos_array)
        for b, want in zip(sub, cand):
            some += len(want)
            for cell, g in grids.items():
                seen = g.looks_at(pred[b], rng_)
                assert want <= set(seen.tolist()), f"step {k} robot {b} cell {cell}: {sorted(want - set(seen.tolist()))[:5]} hidden"
                assert len(set(seen.tolist())) == len(seen) and (np.diff(seen) > 0).all()
                if cell == CELLS[0]:
                    assert looked[b] == len(seen)
                if cell == 1e3:
                    assert len(seen) == E
    assert some > 0
    assert (fleet.wall_looked < E).any() and fleet.wall_looked.dtype == np.int32


def _predictions(cfg, told, U, sincos):
    """The robots' predicted poses as ``literal_walls`` forms them -> [B, N, 2]."""
    N, s, ts = cfg.N_hor, cfg.num_steps_taken, cfg.ts
    out = np.zeros((len(told), N, 2))
    for b in range(len(told)):
        x, y, th = (float(v) for v in told[b])
        for k in range(N):
            c = s + k if s + k < N else N - 1
            v, w = float(U[b][2 * c]), float(U[b][2 * c + 1])
            sn, cs = sincos(np.array([th]))
            x, y, th = x + ts * (v * float(cs[0])), y + ts * (v * float(sn[0])), th + ts * w
            out[b, k] = x, y
    return out


# ---- adversarial placement ----
def literal_D(edge, pred):
    """D(e) of the rule in Python floats."""
    x1, y1, x2, y2 = (float(v) for v in edge)
    ex, ey = x2 - x1, y2 - y1
    L2 = ex * ex + ey * ey
    D = math.inf
    for X, Y in pred:
        X, Y = float(X), float(Y)
        t = 0.0
        if L2 > 0:
            t = ((X - x1) * ex + (Y - y1) * ey) / L2
            t = 0.0 if t < 0 else t
            t = 1.0 if t > 1 else t
        dx, dy = X - (x1 + t * ex), Y - (y1 + t * ey)
        v = dx * dx + dy * dy
        if v < D:
            D = v
    return D


def held_to_the_rule(edges, cell, pred, rng_):
    """-> (the edges within ``range`` by the literal D, the edges looked at); asserts that none of the former is hidden and none of the
    latter is doubled."""
    edges = np.asarray(edges, dtype=np.float64)
    g = wall_grid(edges, cell)
    seen = g.looks_at(pred, rng_)
    want = [e for e in range(len(edges)) if literal_D(edges[e], pred) < rng_ * rng_]
    assert set(want) <= set(seen.tolist()) and len(set(seen.tolist())) == len(seen)
    return want, seen.tolist()


def test_a_closest_point_one_ulp_inside_and_outside_range():
    """A pose on a cell border (x = 0 with origin -4 and cell 1) and a vertical wall whose closest point lies at nextafter(range, 0) from
    it, exactly: a candidate, and looked at.  At nextafter(range, inf) it is none, by the rule."""
    rng_ = 2.0
    for side in (-1.0, 1.0):
        for d, is_cand in ((math.nextafter(rng_, 0.0), True), (math.nextafter(rng_, math.inf), False)):
            x = side * d
            edges = [[-4.0, 0.0, 4.0, 0.0], [x, 5.0, x, 7.0], [-4.0, 8.0, -3.5, 8.0]]      # the first and last span the grid
            want, seen = held_to_the_rule(edges, 1.0, [(0.0, 6.0)], rng_)
            assert (1 in want) == is_cand, (side, d)
            assert not is_cand or 1 in seen


def test_axis_aligned_edges_on_cell_borders():
    edges = [[0.0, 0.0, 6.0, 0.0], [0.0, 0.0, 0.0, 6.0], [2.0, 1.0, 2.0, 3.0], [1.0, 2.0, 4.0, 2.0], [6.0, 0.0, 6.0, 6.0], [0.0, 6.0, 6.0, 6.0]]
    g = check_structure(np.array(edges), 1.0)
    assert g.rect[2].tolist() == [2, 2, 1, 3] and g.rect[4].tolist() == [6, 6, 0, 6]     # a border belongs to the cell above it
    for pose in [(2.0, 2.0), (1.0, 1.0), (3.0, 3.0), (0.0, 0.0), (6.0, 6.0), (1.5, 2.0)]:
        for rng_ in (1.0, math.nextafter(1.0, 2.0), 0.5):
            held_to_the_rule(edges, 1.0, [pose], rng_)
    want, _ = held_to_the_rule(edges, 1.0, [(3.0, 3.0)], math.nextafter(1.0, 2.0))
    assert want == [2, 3]


def test_an_edge_of_zero_length():
    edges = [[0.0, 0.0, 4.0, 0.0], [2.5, 2.5, 2.5, 2.5], [0.0, 4.0, 4.0, 4.0]]
    g = check_structure(np.array(edges), 1.0)
    assert g.rect[1].tolist() == [2, 2, 2, 2]
    assert held_to_the_rule(edges, 1.0, [(2.0, 2.0)], 1.0)[0] == [1]
    assert held_to_the_rule(edges, 1.0, [(1.0, 1.0)], 1.0)[0] == []


def test_200_coincident_edges_in_one_cell():
    """One cell holds more than a wave's lanes: all of them are candidates, the smallest indices win."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = fleet24(cfg, 12)
    p = np.array(starts[0][:2]) + [0.05, 0.0]
    edges = np.concatenate([scene_map(cfg)[0], np.tile([[*p, p[0], p[1] + 0.1]], (200, 1))])
    wl = Walls(edges, 3, radius(cfg), 2.0, 0.0, cell=1.0)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, walls=wl)
    fleet.assemble()
    assert fleet.wall_edge[0].tolist() == [26, 27, 28] and fleet.wall_looked[0] >= 200
    g = fleet.wall_grid
    assert (np.diff(g.cell_off) >= 200).any()
    want, seen = held_to_the_rule(edges, 1.0, fleet.predict()[0][:, :2], 2.0)
    assert set(range(26, 226)) <= set(want)


def test_an_edge_crossing_40_cells_is_looked_at_once():
    edges = [[0.0, 0.0, 40.5, 0.3], [0.0, 5.0, 1.0, 5.0]]
    g = check_structure(np.array(edges), 1.0)
    assert g.rect[0].tolist() == [0, 40, 0, 0] and g.entries == 43
    pred = [(18.0, 1.0), (22.0, 1.0)]
    assert g.window(pred, 2.0)[:2] == (15, 24)
    want, seen = held_to_the_rule(edges, 1.0, pred, 2.0)
    assert want == [0] and seen == [0]


def test_far_outside_the_grid():
    """Positions at 1e12 m clamp in double: no overflow of an int, and nothing within a range of 2 m; from 5 m outside, a range of 6 m
    reaches in."""
    cfg = named_config("cfg1")
    edges = scene_map(cfg, 4)[0]
    g = wall_grid(edges, 0.5)
    for far in [(1e12, 1e12), (-1e12, 3.0), (3.0, -1e300), (1e308, -1e308)]:
        w = g.window([far], 2.0)
        assert all(0 <= c < n for c, n in zip(w, (g.nx, g.nx, g.ny, g.ny)))
        assert held_to_the_rule(edges, 0.5, [far], 2.0)[0] == []
    x0 = float(edges[:, [0, 2]].min())
    ymid = float(edges[:, [1, 3]].mean())
    want, seen = held_to_the_rule(edges, 0.5, [(x0 - 5.0, ymid)], 6.0)
    assert want and len(seen) < len(edges)
    assert held_to_the_rule(edges, 0.5, [(x0 - 5.0, ymid)], 4.0)[0] == []


def test_nan_robot_looks_at_nothing():
    cfg = named_config("cfg1")
    wl = dataclasses.replace(walls_of(cfg, rng_=3.0), cell=1.0)
    fleet, steps = stepped(cfg, nan_fleet(cfg), wl, 3, compare=False)
    assert (fleet.wall_edge[NAN_ROBOT] == -1).all() and (fleet.wall_stage[NAN_ROBOT] == -1).all() and fleet.wall_looked[NAN_ROBOT] == 0
    assert (np.delete(fleet.wall_looked, NAN_ROBOT) > 0).any() and (np.delete(fleet.wall_edge, NAN_ROBOT, axis=0) >= 0).any()
    g = fleet.wall_grid
    assert g.window([(math.nan, 1.0), (1.0, math.inf)], 3.0) is None
    assert g.window([(math.nan, 1.0), (2.0, 2.0)], 3.0) == g.window([(2.0, 2.0)], 3.0)      # the finite stages alone make the window


# ---- validation ----
def test_walls_checked_with_a_cell():
    cfg = named_config("cfg1")
    routes = fleet24(cfg)[0]
    e1040 = scene_map(cfg, 40)[0]
    assert len(e1040) == 1040
    ok = dict(edges=e1040, slots=3, radius=0.5, range=2.0, spacing=0.0)
    assert same_bits(Walls(**ok, cell=1.0).checked(cfg, routes), e1040)
    for cell in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="cell"):
            Walls(**ok, cell=cell).checked(cfg, routes)
    with pytest.raises(ValueError, match="1 to 1024"):
        Walls(**ok).checked(cfg, routes)
    with pytest.raises(ValueError, match="1 to 1024"):
        Walls(**{**ok, "edges": e1040[:1025]}).checked(cfg, routes)
    assert trajectory.WALL_GRID_MAX_EDGES == 1048576
    many = np.broadcast_to(e1040[0], (1048577, 4))                         # a view: nothing of that size is run
    with pytest.raises(ValueError, match="1 to 1048576"):
        Walls(**{**ok, "edges": many}, cell=1.0).checked(cfg, routes)
    with pytest.raises(ValueError):                                        # everything a loop without a cell refuses
        Walls(**{**ok, "slots": 4}, cell=1.0).checked(cfg, routes)
    assert Walls(**ok).cell is None


def test_walls_grid_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_walls_grid", "nmpc_loop_wall_grid"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"typedef struct nmpc_wall_grid\s*\{[^}]*origin\[2\], h\[2\];[^}]*nx, ny, entries, reserved;", header)
    assert _lib.WALL_GRID_DTYPE.names == ("origin", "h", "nx", "ny", "entries", "reserved") and _lib.WALL_GRID_DTYPE.itemsize == 48
    assert lib.nmpc_abi_version() == 3
    assert lib.nmpc_loop_set_walls_grid(None, 1, None, 1, 1.0, 1.0, 0.0, 1.0) == -3
    assert lib.nmpc_loop_wall_grid(None, None, None, None, None) == -3
