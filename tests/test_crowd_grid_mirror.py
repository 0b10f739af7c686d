"""CPU: the crowd found through a grid in space and stage (``Crowd(..., cell=...)``, ``trajectory.crowd_grid``).

The rule is written here once more, entry by entry in Python floats (``kept_through_grid``), on top of ``CrowdGrid``'s filing and
windows, and held to the all-obstacles expression of tests/test_crowd_mirror.py: for every robot the same set of obstacles, each kept
once, every C the same bytes -- on crowds and fleets built for the grid's edges.  Then the mirror with a ``cell`` against the mirror
without, in closed loop with the oracle solving; the pruning, as a condition; and the arguments.

The fleets and crowds of the closed loops are the ones tests/test_gpu_crowd_grid_loop.py runs on the device."""
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.trajectory import (CROWD_GRID_CAP, CROWD_GRID_MAX, Crowd, FleetRecedingHorizon, Peers, Plant, crowd_grid,
                                                     grid_cellof)
from mpc_trajectory_generator_amd.workloads import staggered_fleet
from test_crowd_mirror import NAN_OBSTACLE, RX, RY, arranged, fleet12, narrow_range, scattered
from test_loop_shapes_mirror import NAN_ROBOT, _nan_pose

N = 12          # stages of the hand-made crowds
B = 10


# ---- the two rules, literally ----
def closeness_of_all(pred, tab):
    """The all-obstacles expression -> C [B, D]: the minimum over the stages in ascending order, taken on a strict <."""
    C = np.full((len(pred), len(tab)), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(tab.shape[1]):
            dx, dy = pred[:, None, k, 0] - tab[None, :, k, 0], pred[:, None, k, 1] - tab[None, :, k, 1]
            d = dx * dx + dy * dy
            C = np.where(d < C, d, C)
    return C


def kept_through_grid(grid, pred_b, tab, rng_):
    """The grid's rule for one robot, entry by entry -> [(d, C)] in the order the entries are visited (a d twice = kept twice)."""
    r2 = float(rng_) * float(rng_)
    own = [(float(p[0]), float(p[1])) for p in pred_b]

    def dist2(d, k):
        dx, dy = own[k][0] - float(tab[d, k, 0]), own[k][1] - float(tab[d, k, 1])
        return dx * dx + dy * dy

    out = []
    for d, k in zip(*(a.tolist() for a in grid.candidates(pred_b, rng_))):
        if not dist2(d, k) < r2:
            continue
        if any(dist2(d, j) < r2 for j in range(k)):
            continue
        C = math.inf
        for j in range(len(own)):
            v = dist2(d, j)
            if v < C:
                C = v
        out.append((d, C))
    return out


def check_rule(obs, tab, pred, rng_, cell):
    """Every robot of ``pred`` against the crowd ``obs`` with the table ``tab`` -> (the grid with the table filed, kept per robot)."""
    grid = crowd_grid(obs, tab.shape[1], cell)
    cell_of = grid.file(tab)
    fin = np.isfinite(tab[:, :, :2]).all(axis=2)
    assert np.array_equal(cell_of >= 0, fin) and grid.filed == int(fin.sum())
    cells = grid.layers * grid.nx * grid.ny
    assert cell_of.max() < cells and len(grid.cell_off) == cells + 1 and grid.cell_off[-1] == grid.filed == len(grid.cell_mem)
    k_of = np.broadcast_to(np.arange(tab.shape[1])[None, :], cell_of.shape)
    assert (cell_of[fin] // (grid.nx * grid.ny) == k_of[fin]).all(), "an entry outside its stage's layer"
    for c in np.unique(cell_of[fin]):                                       # every cell: its members once, ascending
        mem = grid.cell_mem[grid.cell_off[c]:grid.cell_off[c + 1]]
        assert np.array_equal(mem, np.nonzero(cell_of[:, c // (grid.nx * grid.ny)] == c)[0])
    C = closeness_of_all(pred, tab)
    r2 = float(rng_) * float(rng_)
    kept = []
    for b in range(len(pred)):
        got = kept_through_grid(grid, pred[b], tab, rng_)
        want = np.nonzero(C[b] < r2)[0]
        assert sorted(d for d, _ in got) == want.tolist(), f"robot {b}: kept {sorted(d for d, _ in got)}, in range {want.tolist()}"
        assert all(np.float64(c).tobytes() == C[b, d].tobytes() for d, c in got), f"robot {b}: a C differs"
        assert grid.looked(pred[b], rng_) == len(grid.candidates(pred[b], rng_)[0]) <= grid.filed
        kept.append(got)
    return grid, kept


# ---- crowds and fleets made for the grid's edges ----
def moving(seed, D=60, side=60.0, at=0.0, reach=25.0):
    """-> (obs, tab [D, N, 5]): obstacles between random end points of a square, each at its own pace along p1 -> p2 and a little
    beyond p2 (outside the extent of the end points)."""
    rng = np.random.default_rng(seed)
    p1 = at + rng.uniform(0.0, side, (D, 2))
    p2 = p1 + rng.uniform(-reach, reach, (D, 2))
    w = rng.uniform(0.0, 1.3, (D, 1)) * np.linspace(0.0, 1.0, N)[None, :]
    tab = np.zeros((D, N, 5))
    tab[:, :, :2] = p1[:, None, :] + w[:, :, None] * (p2 - p1)[:, None, :]
    tab[:, :, 2:4] = 0.5
    return (p1, p2) + tuple(np.zeros(D) for _ in range(4)), tab


def walkers(seed, n=B, side=60.0, at=0.0, step=0.4):
    rng = np.random.default_rng(seed)
    pred = np.zeros((n, N, 3))
    pred[:, :, :2] = at + rng.uniform(0.0, side, (n, 1, 2)) + np.cumsum(rng.uniform(-step, step, (n, N, 2)), axis=1)
    return pred


def _spoiled():
    """Obstacle 3 with a NaN in p1, 4 with a NaN in p2 only, 5 at 1e9; robot 2 with a NaN stage, robot 3 with an infinite one."""
    obs, tab = moving(31)
    obs[0][3, 0], obs[1][4, 1] = np.nan, np.nan
    tab[3, :, 0], tab[4, :, 1] = np.nan, np.nan
    obs[0][5], obs[1][5] = (1e9, 1e9), (1e9, 1e9)
    tab[5, :, :2] = 1e9
    pred = walkers(32)
    pred[2, 4, 0], pred[3, 7, 1], pred[4, :, :2] = np.nan, np.inf, np.nan
    pred[5, :, :2] = tab[6, :, :2] + 0.25                                   # somebody near obstacle 6 all along
    return obs, tab, pred


def _outside():
    """Robots beyond the extent on each side, within range of obstacles that stand in the grid's edge cells."""
    obs, tab = moving(33, D=40, side=20.0, reach=0.0)
    for d, p in enumerate([(0.0, 10.0), (20.0, 10.0), (10.0, 0.0), (10.0, 20.0), (0.0, 0.0), (20.0, 20.0)]):
        obs[0][d], obs[1][d], tab[d, :, :2] = p, p, p
    lo, hi = np.concatenate(obs[:2]).min(axis=0), np.concatenate(obs[:2]).max(axis=0)
    assert np.array_equal(lo, (0.0, 0.0)) and np.array_equal(hi, (20.0, 20.0))
    pred = np.zeros((8, N, 3))
    for i, (x, y) in enumerate([(lo[0] - 1.0, 10.0), (hi[0] + 1.0, 10.0), (10.0, lo[1] - 1.0), (10.0, hi[1] + 1.0),
                                (lo[0] - 1.0, lo[1] - 1.0), (hi[0] + 1.0, hi[1] + 1.0), (lo[0] - 50.0, 10.0), (hi[0] + 1e6, hi[1] + 1e6)]):
        pred[i, :, :2] = (x, y)
    return obs, tab, pred


def _range_edge():
    """Robot 0 standing still at the origin; obstacle 0 at exactly range = 2, obstacle 1 at nextafter(2, 0), obstacle 2 in range at
    every stage (kept once), obstacle 3 in range at the last stage only, obstacle 4 never."""
    D = 5
    p = np.array([[2.0, 0.0], [0.0, -math.nextafter(2.0, 0.0)], [0.5, 0.5], [-9.0, 3.0], [7.0, -7.0]])
    tab = np.zeros((D, N, 5))
    tab[:, :, :2] = p[:, None, :]
    tab[3, N - 1, :2] = (-1.0, 1.0)
    q = p.copy()
    q[3] = (-1.0, 1.0)
    return (p, q) + tuple(np.zeros(D) for _ in range(4)), tab, np.zeros((1, N, 3))


def _on_borders():
    obs, tab = moving(35)
    obs = tuple(np.round(a * 2.0) / 2.0 if a.ndim == 2 else a for a in obs)
    tab[:, :, :2] = np.round(tab[:, :, :2] * 2.0) / 2.0
    tab[:, 0, :2] = obs[0]
    return obs, tab, np.round(walkers(36) * 2.0) / 2.0


def _one_point():
    D = 9
    p = np.tile([3.25, -1.5], (D, 1))
    tab = np.zeros((D, N, 5))
    tab[:, :, :2] = p[:, None, :]
    pred = walkers(37, side=4.0, at=-2.0)
    return (p, p.copy()) + tuple(np.zeros(D) for _ in range(4)), tab, pred


# name -> (obs, tab, pred, range, cell)
CROWDS = {
    "60 m, range 2, cell 1": lambda: moving(21) + (walkers(22), 2.0, 1.0),
    "60 m, range 10, cell 4": lambda: moving(23) + (walkers(24), 10.0, 4.0),
    "cell 0.1: the cap": lambda: moving(25) + (walkers(26), 2.0, 0.1),
    "one cell": lambda: moving(27) + (walkers(28), 3.0, 1e3),
    "negative coordinates": lambda: moving(29, at=-45.0) + (walkers(30, at=-45.0), 2.0, 1.0),
    "NaN, inf, far": lambda: _spoiled() + (2.0, 1.0),
    "NaN, inf, far, coarse": lambda: _spoiled() + (4.0, 30.0),
    "robots outside the extent": lambda: _outside() + (3.0, 1.0),
    "on cell borders": lambda: _on_borders() + (2.0, 0.5),
    "exactly range": lambda: _range_edge() + (2.0, 0.5),
    "exactly range, cell = range": lambda: _range_edge() + (2.0, 2.0),
    "one point": lambda: _one_point() + (2.0, 1.0),
}


@pytest.mark.parametrize("name", list(CROWDS))
def test_grid_rule_keeps_what_the_all_obstacles_rule_keeps(name):
    obs, tab, pred, rng_, cell = CROWDS[name]()
    grid, kept = check_rule(obs, tab, pred, rng_, cell)
    hdr = grid.header()
    assert hdr["layers"] == N and hdr["filed"] == grid.filed and (hdr["nx"], hdr["ny"]) == (grid.nx, grid.ny)
    n = sum(len(k) for k in kept)
    if name == "cell 0.1: the cap":
        assert (grid.nx, grid.ny) == (CROWD_GRID_CAP, CROWD_GRID_CAP) and (grid.h > 0.1).all()
    if name == "one cell":
        assert (grid.nx, grid.ny) == (1, 1) and all(grid.looked(p, rng_) == grid.filed for p in pred) and n
    if name == "one point":
        assert (grid.nx, grid.ny) == (1, 1) and np.array_equal(grid.origin, (3.25, -1.5)) and n
    if name.startswith("NaN"):
        assert grid.filed == (len(tab) - 2) * N and (grid.cell_of[3] == -1).all() and (grid.cell_of[4] == -1).all()
        ends = np.concatenate([np.delete(obs[0], 3, axis=0), np.delete(obs[1], 4, axis=0)])
        assert np.array_equal(grid.origin, ends.min(axis=0)), "an end point with a NaN beside it counts, one with a NaN does not"
        assert grid.cell_of[5, 0] % (grid.nx * grid.ny) == grid.nx * grid.ny - 1                       # the far one: the last cell
        assert not kept[4] and grid.looked(pred[4], rng_) == 0                                          # a robot without a finite stage
        assert grid.window(np.nan, 1.0, rng_) is None and grid.window(1.0, np.inf, rng_) is None
        assert any(d == 6 for d, _ in kept[5])
    if name == "robots outside the extent":
        w = [grid.window(p[0, 0], p[0, 1], rng_) for p in pred]
        assert w[0][0] == 0 and w[1][1] == grid.nx - 1 and w[2][2] == 0 and w[3][3] == grid.ny - 1
        assert w[6][:2] == (0, 0) and w[7] == (grid.nx - 1, grid.nx - 1, grid.ny - 1, grid.ny - 1)
        assert all(i in [d for d, _ in kept[i]] for i in range(6)), "the obstacle in the edge cell, not found from outside the extent"
        assert not kept[6] and not kept[7]
    if name == "on cell borders":
        assert np.array_equal((tab[:, :, :2] - grid.origin) / 0.5 % 1.0, np.zeros(tab[:, :, :2].shape))
    if name.startswith("exactly range"):
        assert sorted(d for d, _ in kept[0]) == [1, 2, 3]                    # not the one at exactly 2.0, the standing one once
        d, k = grid.candidates(pred[0], rng_)
        assert (d == 0).sum() == N and (d == 2).sum() == N and k[d == 3].tolist() == [N - 1] and not (d == 4).any()


def test_window_is_the_cell_function_of_the_filing():
    obs, tab = moving(41)
    g = crowd_grid(obs, N, 1.0)
    for x, y, r in [(3.0, 4.0, 2.0), (-100.0, 500.0, 2.0), (17.25, 0.5, 0.25)]:
        assert g.window(x, y, r) == tuple(int(grid_cellof(v, g.origin[ax], g.h[ax], (g.nx, g.ny)[ax]))
                                          for v, ax in ((x - r, 0), (x + r, 0), (y - r, 1), (y + r, 1)))


# ---- closed loop: the mirror with a cell against the mirror without ----
def _pair(cfg, routes, route_of, starts, i0, dyn, crowd, cell, o, **kw):
    assert crowd.cell is None
    make = lambda c: FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, crowd=c, **kw)      # noqa: E731
    return make(dataclasses.replace(crowd, cell=cell)), make(crowd)


def _run(grid, plain, o, steps, until=None):
    """Step both mirrors; everything the crowd touches must agree by bytes -> per step the looked counts."""
    looked = []
    while plain.steps < steps and (until is None or until(plain)):
        k = plain.steps
        P, st = plain.step(o.warm_solve())
        Q, sq = grid.step(o.warm_solve())
        assert P.tobytes() == Q.tobytes(), f"step {k}: P at columns {np.unique(np.nonzero(P != Q)[1])[:10]}"
        assert np.array_equal(plain.crowd_seen, grid.crowd_seen), f"step {k}: seen"
        for name in ("state", "U", "Y", "last_u", "idx", "done"):
            assert getattr(plain, name).tobytes() == getattr(grid, name).tobytes(), f"step {k}: {name}"
        assert plain.crowd_table().tobytes() == grid.crowd_table().tobytes()
        a, b = plain.crowd_clearance(), grid.crowd_clearance()
        assert all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names), f"step {k}: the observer"
        if plain.active is not None:
            assert np.array_equal(plain.active, grid.active) and np.array_equal(plain.retired_at, grid.retired_at)
        looked.append(grid.crowd_looked.copy())
    assert np.stack(plain.traj).tobytes() == np.stack(grid.traj).tobytes()
    return looked


CLOSED = ["cfg1", "cfg4-K1", "cfg2", "s2", "peers", "peers-grid", "plant"]


@pytest.mark.parametrize("which", CLOSED)
def test_mirror_with_a_cell_equals_mirror_without(which):
    cfg = {"cfg4-K1": named_config("cfg4"), "cfg2": named_config("cfg2"), "s2": load_config(num_steps_taken=2)}.get(which, named_config("cfg1"))
    K = 1 if which == "cfg4-K1" else 0
    routes, route_of, starts, i0, dyn = fleet12(cfg, K)
    obs, sinus = arranged(cfg, starts)
    kw = {}
    if which.startswith("peers"):
        kw["peers"] = Peers(slots=1, rx=RX, ry=RY, range=3.0, cell=1.0 if which == "peers-grid" else None)
    if which == "plant":
        kw["plant"] = Plant(seed=7, meas=(0.01, 0.012, 0.02))
    M = 2 if K or kw.get("peers") else 3
    o = oracle_for(cfg)
    make = lambda r: FleetRecedingHorizon(routes, route_of, starts, dyn, idx0=i0, crowd=Crowd(obs, M, r, sinus=sinus))      # noqa: E731
    rng_ = 3.0 * narrow_range(make)
    grid, plain = _pair(cfg, routes, route_of, starts, i0, dyn, Crowd(obs, M, rng_, sinus=sinus, watch=True), 0.5, o, **kw)
    looked = _run(grid, plain, o, 3)
    D = len(obs[2])
    assert grid.crowd_grid.nx * grid.crowd_grid.ny > 1 and grid.crowd_grid.layers == cfg.N_hor
    assert grid.crowd_grid.filed == (D - 1) * cfg.N_hor                      # the NaN obstacle is unfiled
    assert 0 < np.stack(looked).max() < D * cfg.N_hor
    seen = grid.crowd_seen
    assert (seen >= 0).any() and not (seen == NAN_OBSTACLE).any()


def test_retiring_fleet_keeps_looked():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg, back=(2, 5, 9))
    obs, sinus = scattered(cfg, 40)
    o = oracle_for(cfg)
    grid, plain = _pair(cfg, routes, route_of, starts, i0, None, Crowd(obs, 2, 6.0, sinus=sinus, watch=True), 1.0, o, retire=True)
    extra = [2]

    def until(host):
        if host.n_active:
            return True
        extra[0] -= 1
        return extra[0] >= 0

    looked = _run(grid, plain, o, 45, until=until)
    at = plain.retired_at
    assert plain.n_active == 0 and len(set(at.tolist())) > 2 and plain.steps == at.max() + 2
    first = int(np.argmin(at))
    assert all(lk[first] == looked[at[first] - 1][first] for lk in looked[at[first]:]), "a retired robot's looked moved"
    assert np.array_equal(looked[-1], looked[-3])
    filed = grid.crowd_grid.cell_of.copy()                                  # nobody active: the table advances, the filing stays
    grid.step(o.warm_solve())
    assert np.array_equal(grid.crowd_grid.cell_of, filed)


def test_a_nan_pose_looks_at_nothing():
    c = _nan_pose()
    n = len(c.starts)
    obs, sinus = scattered(c.cfg, 40)
    o = oracle_for(c.cfg)
    grid, plain = _pair(c.cfg, [c.route], np.zeros(n, dtype=np.int32), c.starts, c.idx0, c.dyn, Crowd(obs, 1, 1e3, sinus=sinus), 1.0, o)
    keep = np.arange(n) != NAN_ROBOT
    for k in range(2):
        P, _ = plain.step(o.warm_solve())
        Q, _ = grid.step(o.warm_solve())
        assert P[keep].tobytes() == Q[keep].tobytes() and np.array_equal(plain.crowd_seen, grid.crowd_seen)
        assert grid.crowd_looked[NAN_ROBOT] == 0 and (grid.crowd_seen[NAN_ROBOT] == -1).all()
        assert (grid.crowd_looked[keep] == grid.crowd_grid.filed).all() and (grid.crowd_seen[keep] >= 0).all()      # range 1 km: every cell


# ---- pruning, as a condition ----
@pytest.mark.parametrize("D", [300, 2100])
@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_a_robot_looks_at_a_tenth_of_the_table_at_most(name, D):
    """Scene 11, range 2 m, cell 1 m, three steps: the all-obstacles rule looks at D * N entries per robot."""
    from test_gpu_crowd_loop import _fleet
    cfg = named_config(name)
    routes, route_of, starts, i0, dyn = _fleet(cfg, 0)
    obs, sinus = scattered(cfg, D)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, crowd=Crowd(obs, 3, 2.0, sinus=sinus, cell=1.0))
    for k in range(3):
        fleet.step(o.warm_solve(threads=8))
        share = fleet.crowd_looked.max() / (D * cfg.N_hor)
        print(f"{name} D = {D} step {k}: looked at most {fleet.crowd_looked.max()} of {D * cfg.N_hor} ({100 * share:.2f} %), mean {fleet.crowd_looked.mean():.0f}")
        assert fleet.crowd_looked.max() <= D * cfg.N_hor / 10
    assert fleet.crowd_looked.max() > 0 and (fleet.crowd_seen >= 0).any()


# ---- arguments and the C ABI ----
def test_checked_takes_a_larger_crowd_with_a_cell():
    def crowd(D, **kw):
        return Crowd((np.zeros((D, 2)), np.ones((D, 2))) + tuple(np.zeros(D) for _ in range(4)), 1, 5.0, **kw)
    assert CROWD_GRID_MAX == 131072
    crowd(16385, cell=1.0).checked(12, 0, 3)
    crowd(CROWD_GRID_MAX, cell=0.5).checked(12, 0, 3)
    with pytest.raises(ValueError):
        crowd(16385).checked(12, 0, 3)
    with pytest.raises(ValueError):
        crowd(CROWD_GRID_MAX + 1, cell=1.0).checked(12, 0, 3)
    for bad in (0, 0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            crowd(5, cell=bad).checked(12, 0, 3)
    crowd(5, cell=1.0).checked(12, 0, 3)


def test_crowd_grid_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_crowd_grid", "nmpc_loop_crowd_grid"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
    m = re.search(r"typedef struct nmpc_crowd_grid \{[^\n]*\n\s*double\s+([^;]+);\n\s*int32_t ([^;]+);\n\} nmpc_crowd_grid;", header)
    fields = [re.sub(r"\[\d+\]", "", f).strip() for f in (m.group(1) + "," + m.group(2)).split(",")]
    assert fields == list(_lib.CROWD_GRID_DTYPE.names) and _lib.CROWD_GRID_DTYPE.itemsize == 48
    assert lib.nmpc_loop_set_crowd_grid(None, 1, None, 0.0, 1, 1.0, 1.0) == -3 and lib.nmpc_loop_crowd_grid(None, None, None, None) == -3
