"""The crowd on the host (``FleetRecedingHorizon(..., crowd=Crowd(...))``), with the oracle solving.

The mirror's vectorised rule against a literal per-robot, per-obstacle loop of the rule written here (every obstacle's horizon from the
single-robot restatement ``harness.dyn_obstacle``, the robot's Euler prediction, closeness stage by stage, the (C, d) sort, the overlay
and the observer), bit for bit over several steps; the table against the block a plain loop carries for scripted obstacles with the
same parameters; the slot order of scripted obstacles, crowd and peers; ties, one lane's whole list and a NaN obstacle; a range that
leaves filled and unfilled slots; and the five functions of the C ABI.

The fleets and crowds built here are the ones tests/test_gpu_crowd_loop.py runs on the device."""
import copy
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.trajectory import Crowd, FleetRecedingHorizon, Peers, no_crowd_clearance
from mpc_trajectory_generator_amd.workloads import crowd_ellipses, fleet_ellipses

RX, RY = 0.37, 0.53          # radii no scripted, padding or crowd ellipse has: a slot that shows them holds a peer
LANE = (5, 69, 133)          # one lane's whole list on the device: the lanes stride over d by 64
TWINS = (149, 150)           # two obstacles with identical parameters
NAN_OBSTACLE = 7


def _slot0(cfg):
    """Where the dynamic block starts in a parameter vector."""
    return 20 + cfg.N_hor + 3 * cfg.Nobs


def scattered(cfg, D, seed=23):
    """-> (obstacles, sinus): D obstacles of scene 11 (``crowd_ellipses``), every seventh on the sinusoidal law."""
    return crowd_ellipses(cfg, 11, D, seed), np.arange(D) % 7 == 3


def arranged(cfg, starts, D=200, seed=29):
    """-> (obstacles, sinus): ``scattered`` with the three obstacles ``LANE`` standing 1, 2 and 3 cm from robot 0's start, the two
    ``TWINS`` alike in every parameter and standing 2 cm from robot 1's start, and a NaN in obstacle ``NAN_OBSTACLE``."""
    (p1, p2, freq, rx, ry, ang), sinus = scattered(cfg, D, seed)
    sinus = sinus.copy()
    for n, d in enumerate(LANE):
        p1[d] = p2[d] = starts[0, :2] + np.array([0.01 * (n + 1), 0.0])
        sinus[d] = False
    a, b = TWINS
    p1[a] = p2[a] = p1[b] = p2[b] = starts[1, :2] + np.array([0.0, 0.02])
    freq[b], rx[b], ry[b], ang[b], sinus[a], sinus[b] = freq[a], rx[a], ry[a], ang[a], False, False
    p1[NAN_OBSTACLE, 0], sinus[NAN_OBSTACLE] = np.nan, False
    return (p1, p2, freq, rx, ry, ang), sinus


def closeness_at_start(host):
    """-> C [B, D] of a mirror that has not stepped (everybody stands still): what its first step will rank.  Leaves it assembled."""
    host.assemble()
    tab, pred = host.crowd_table(), host.predict()
    with np.errstate(invalid="ignore"):
        dx, dy = pred[:, None, :, 0] - tab[None, :, :, 0], pred[:, None, :, 1] - tab[None, :, :, 1]
        d = dx * dx + dy * dy
    return np.where(np.isnan(d), np.inf, d).min(axis=2)


def narrow_range(make_host):
    """The median over robots of the smallest C at the start, as a range: about half of the robots find an obstacle within it.
    ``make_host(range)`` -> a fresh mirror."""
    return float(math.sqrt(np.median(closeness_at_start(make_host(1e6)).min(axis=1))))


def filled(seen):
    return np.asarray(seen) >= 0


# ---- the literal rule ----
def literal_horizon(cfg, obs, sinus, d, t, H):
    """Obstacle d's ellipses at ``linspace(t, t + H ts, H)`` from the single-robot restatement -> [H] tuples of 5 floats."""
    one = [list(map(float, obs[0][d])), list(map(float, obs[1][d]))] + [float(a[d]) for a in obs[2:]]
    if sinus[d]:           # the restatement's sinusoidal obstacle is the one at index 2
        return harness.dyn_obstacle(cfg, [one, one, one], t, H, sinus_object=True)[2]
    return harness.dyn_obstacle(cfg, [one], t, H)[0]


class LiteralCrowd:
    """Section 5.9 robot by robot and obstacle by obstacle in Python floats."""

    def __init__(self, cfg, obs, sinus, M, rng_, K, B):
        self.cfg, self.obs, self.sinus, self.M, self.r2, self.K = cfg, obs, sinus, M, rng_ * rng_, K
        self.D = len(obs[2])
        self.rows = None
        self.rec = [(math.inf, -1, -1)] * B

    def advance(self, t):
        cfg, N, s = self.cfg, self.cfg.N_hor, self.cfg.num_steps_taken
        if t == 0:
            self.rows = [literal_horizon(cfg, self.obs, self.sinus, d, 0.0, N) for d in range(self.D)]
        else:
            self.rows = [self.rows[d][s:] + literal_horizon(cfg, self.obs, self.sinus, d, (t + N - s) * cfg.ts, s) for d in range(self.D)]

    def overlay(self, P, state, U):
        """-> (P overlaid, seen [B][M])"""
        cfg = self.cfg
        B, N, s, ts = len(state), cfg.N_hor, cfg.num_steps_taken, cfg.ts
        P = P.copy()
        seen = []
        for b in range(B):
            x, y, th = (float(v) for v in state[b])
            pred = []
            for k in range(N):
                c = s + k if s + k < N else N - 1
                v, w = float(U[b][2 * c]), float(U[b][2 * c + 1])
                x, y, th = x + ts * (v * math.cos(th)), y + ts * (v * math.sin(th)), th + ts * w
                pred.append((x, y))
            cand = []
            for d in range(self.D):
                C = math.inf
                for k in range(N):
                    dx, dy = pred[k][0] - self.rows[d][k][0], pred[k][1] - self.rows[d][k][1]
                    v = dx * dx + dy * dy
                    if v < C:
                        C = v
                if C < self.r2:
                    cand.append((C, d))
            cand.sort()
            seen.append([d for _, d in cand[:self.M]] + [-1] * max(0, self.M - len(cand)))
            for m, d in enumerate(seen[-1]):
                if d >= 0:
                    at = _slot0(cfg) + (self.K + m) * 5 * N
                    P[b, at:at + 5 * N] = np.array(self.rows[d], dtype=np.float64).reshape(-1)
        return P, seen

    def observe(self, rows, first):
        """The step's trajectory rows [s][B][3], the first of them row ``first`` of the trajectory."""
        for i, pose in enumerate(rows):
            for b in range(len(pose)):
                for d in range(self.D):
                    ex, ey, rx, ry, ang = self.rows[d][i]
                    dx, dy = float(pose[b][0]) - ex, float(pose[b][1]) - ey
                    sn, cs = math.sin(ang), math.cos(ang)
                    a, c = dx * cs + dy * sn, dx * sn - dy * cs
                    v = (a * a) / (rx * rx) + (c * c) / (ry * ry)
                    if (v, first + i, d) < self.rec[b]:
                        self.rec[b] = (v, first + i, d)


def _twin_without_crowd(fleet):
    """The same fleet at the same states, plans and carried blocks, without its crowd; assembling it leaves ``fleet`` alone."""
    twin = copy.copy(fleet)
    twin.crowd, twin._Mc = None, 0
    twin.dyn = fleet.dyn.copy()
    return twin


def records(rec):
    out = no_crowd_clearance(len(rec))
    for b, (v, r, d) in enumerate(rec):
        out[b] = (v, r, d)
    return out


def fleet12(cfg, K=0, seed=41):
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=seed)
    return routes, route_of, starts, i0, fleet_ellipses(routes, route_of, i0, K, 9)


@pytest.mark.parametrize("D", [1, 5, 70, 200])
def test_mirror_equals_literal_rule(D):
    cfg = named_config("cfg4")
    K, M, steps = 1, 2, 4
    routes, route_of, starts, i0, dyn = fleet12(cfg, K)
    obs, sinus = scattered(cfg, D)
    make = lambda r: FleetRecedingHorizon(routes, route_of, starts, dyn, idx0=i0, crowd=Crowd(obs, M, r, sinus=sinus, watch=True))      # noqa: E731
    rng_ = narrow_range(make) * 1.5 if D >= 70 else 1e3                 # few obstacles: everybody sees them all
    fleet, lit = make(rng_), LiteralCrowd(cfg, obs, sinus, M, rng_, K, len(starts))
    o = oracle_for(cfg)
    s, N = cfg.num_steps_taken, cfg.N_hor
    lo, hi = _slot0(cfg) + K * 5 * N, _slot0(cfg) + (K + M) * 5 * N
    n = []
    for k in range(steps):
        twin = _twin_without_crowd(fleet)
        state, U = fleet.state, fleet.U.copy()
        P0 = twin.assemble()
        lit.advance(fleet.t)
        want, seen = lit.overlay(P0, state, U)
        P, _ = fleet.step(o.warm_solve())
        assert np.array_equal(fleet.crowd_table(), np.array(lit.rows)), f"step {k}: the table"
        assert np.array_equal(P, want), f"step {k}: columns {np.unique(np.nonzero(P != want)[1])[:10]}"
        assert np.array_equal(P[:, :lo], P0[:, :lo]) and np.array_equal(P[:, hi:], P0[:, hi:]), f"step {k}"
        assert np.array_equal(fleet.dyn, twin.dyn), f"step {k}: the carried block saw the crowd"
        assert fleet.crowd_seen.tolist() == seen, f"step {k}"
        lit.observe(fleet.traj[-s:], k * s + 1)
        got, exp = fleet.crowd_clearance(), records(lit.rec)
        assert all(got[f].tobytes() == exp[f].tobytes() for f in got.dtype.names), f"step {k}: the observer"
        n += [sum(d >= 0 for d in row) for row in seen]
    assert max(n) == min(M, D)
    if D >= 70:
        assert min(n) < M, "the range must leave an unfilled slot somewhere"


@pytest.mark.parametrize("s", [1, 2, 20])
def test_table_row_equals_the_carried_block_of_a_scripted_obstacle(s):
    """Three scripted obstacles, the same for every robot, index 2 on the sinusoidal law, against the same three as a crowd: the
    table's row d is slot d of a plain loop's p, bit for bit, with H == 1 in ``linspace`` (s = 1), the ordinary case (s = 2) and a
    row that is fresh every step (s = N)."""
    cfg = load_config(num_steps_taken=s)
    assert cfg.N_hor == 20 and cfg.Ndynobs == 3
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 2, 3, seed=13)
    one = fleet_ellipses(routes[:1], route_of[:1] * 0, i0[:1], 3, 4)                        # [1, 3, ...]
    dyn = tuple(np.repeat(a, len(starts), axis=0) for a in one)
    obs = tuple(a[0] for a in one)
    o = oracle_for(cfg, max_inner=40, max_outer=2)                                           # cheap solves: the assembly is what is tested
    plain = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, sinus_object=True, idx0=i0)
    crowd = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0,
                                 crowd=Crowd(obs, 1, 5.0, sinus=[False, False, True]))
    N = cfg.N_hor
    for k in range(6):
        P, _ = plain.step(o.warm_solve(threads=2))
        crowd.step(o.warm_solve(threads=2))
        block = P[0, _slot0(cfg):_slot0(cfg) + 3 * 5 * N].reshape(3, N, 5)
        assert np.array_equal(crowd.crowd_table(), block), f"step {k}"
        assert np.array_equal(plain.dyn[0], block)


def test_slot_order_and_limits():
    """K = 1, one crowd slot, one peer slot: each kind in its own slot; the peers' slot holds what a loop without a crowd puts into
    slot K; a loop given ``crowd=None`` is the loop that was not given the argument; and what ``Crowd.checked`` refuses."""
    cfg = named_config("cfg4")
    K, N = 1, cfg.N_hor
    routes, route_of, starts, i0, dyn = fleet12(cfg, K)
    obs, sinus = scattered(cfg, 5)
    peers = Peers(slots=1, rx=RX, ry=RY, range=1e3)
    o = oracle_for(cfg)
    both = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers, crowd=Crowd(obs, 1, 1e3, sinus=sinus))
    only = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers)
    none = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers, crowd=None)
    at = _slot0(cfg) + np.arange(3) * 5 * N
    for k in range(3):
        first = k == 0
        Pb, Po = both.step(o.warm_solve())[0].copy(), only.step(o.warm_solve())[0].copy()
        Pn = none.step(o.warm_solve())[0]
        assert np.array_equal(Po, Pn), f"step {k}"
        tab, seen = both.crowd_table(), both.crowd_seen
        assert (seen >= 0).all() and (both.peer_index >= 0).all()
        assert np.array_equal(Pb[:, at[0]:at[1]], both.dyn[:, 0].reshape(len(starts), -1))             # scripted
        assert np.array_equal(Pb[:, at[1]:at[2]], tab[seen[:, 0]].reshape(len(starts), -1))            # crowd
        assert (Pb[:, at[2] + 2] == RX).all() and (Pb[:, at[2] + 3] == RY).all()                        # peers
        assert not (Pb[:, at[1] + 2] == RX).any()
        if first:              # the same states and plans: the peers' slot is the other loop's slot K
            assert np.array_equal(Pb[:, at[2]:at[2] + 5 * N], Po[:, at[1]:at[1] + 5 * N])
            assert np.array_equal(both.peer_index, only.peer_index)
    ok = dict(obstacles=obs, slots=1, range=5.0)
    Crowd(**ok).checked(12, 1, 3, 1)
    nan = tuple(np.where(np.arange(5) == 2, np.nan, a) if a.ndim == 1 else a for a in obs)
    Crowd(**{**ok, "obstacles": nan}).checked(12, 1, 3, 1)                                             # values are not checked
    many = tuple(np.zeros((16385, 2)) if a.ndim == 2 else np.zeros(16385) for a in obs)
    none_ = tuple(a[:0] for a in obs)
    for bad in (dict(slots=0), dict(slots=2), dict(range=0.0), dict(range=math.inf), dict(range=math.nan), dict(obstacles=many),
                dict(obstacles=none_), dict(obstacles=obs[:5]), dict(sinus=[True, False]), dict(obstacles=(obs[0][:3],) + obs[1:])):
        with pytest.raises(ValueError):
            Crowd(**{**ok, **bad}).checked(12, 1, 3, 1)
    with pytest.raises(ValueError):
        Crowd(**ok).checked(12, 2, 3, 1)
    with pytest.raises(ValueError):                                                                    # through the constructor, with peers
        FleetRecedingHorizon(routes, route_of, starts, dyn, idx0=i0, peers=Peers(slots=2, rx=RX, ry=RY, range=5.0), crowd=Crowd(**ok))


def arranged_fleet(cfg, B=12):
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, B, seed=41)
    return routes, route_of, starts, i0, arranged(cfg, starts)


def reach_arranged(seen, first):
    """What the arranged crowd is there for, on the chosen obstacles [B, 3] of a step run with a range that excludes nobody."""
    seen = np.asarray(seen)
    assert not (seen == NAN_OBSTACLE).any(), "the NaN obstacle was seen"
    assert (seen >= 0).all()
    for row in seen.tolist():              # equally close to everybody, always: the higher twin directly behind the lower
        assert TWINS[1] not in row or row.index(TWINS[0]) + 1 == row.index(TWINS[1]), "the twins: the lower index first"
    assert TWINS[0] in seen[1] and TWINS[1] in seen[1]
    if first:                              # everybody stands where the arrangement was made (later the robots have moved on)
        assert seen[0].tolist() == list(LANE), "robot 0 does not see one lane's whole list, in order"
        assert seen[1].tolist()[:2] == list(TWINS)


def test_order_and_corner_cases():
    """Identical obstacles: the lower index wins.  The three closest at d, d + 64, d + 128: all three, in order.  A NaN obstacle is
    never seen, and the choices and parameter vectors are those of a crowd in which it stands far away from everybody."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, (obs, sinus) = arranged_fleet(cfg)
    far = tuple(a.copy() for a in obs)
    far[0][NAN_OBSTACLE], far[1][NAN_OBSTACLE] = (1e9, 1e9), (1e9, 1e9)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, crowd=Crowd(obs, 3, 1e6, sinus=sinus, watch=True))
    other = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, crowd=Crowd(far, 3, 1e6, sinus=sinus, watch=True))
    assert np.isnan(obs[0][NAN_OBSTACLE, 0])
    for k in range(3):
        P, _ = fleet.step(o.warm_solve())
        Q, _ = other.step(o.warm_solve())
        reach_arranged(fleet.crowd_seen, k == 0)
        assert np.array_equal(P, Q) and np.array_equal(fleet.crowd_seen, other.crowd_seen), f"step {k}"
        assert np.isnan(fleet.crowd_table()[NAN_OBSTACLE, :, 0]).all() and not np.isnan(np.delete(fleet.crowd_table(), NAN_OBSTACLE, axis=0)).any()
        a, b = fleet.crowd_clearance(), other.crowd_clearance()
        assert all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names) and not (a["obstacle"] == NAN_OBSTACLE).any()
    assert (fleet.crowd_clearance()["row"] >= 1).all()


def test_narrow_range_leaves_filled_and_unfilled_slots():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, (obs, sinus) = arranged_fleet(cfg)
    make = lambda r: FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, crowd=Crowd(obs, 3, r, sinus=sinus))      # noqa: E731
    rng_ = narrow_range(make)
    assert 0.0 < rng_ < 1e3
    fleet, o = make(rng_), oracle_for(cfg)
    seen = []
    for k in range(3):
        fleet.step(o.warm_solve())
        seen.append(filled(fleet.crowd_seen))
    seen = np.stack(seen)
    assert seen.any() and not seen.all(), "the narrow range must leave filled and unfilled slots"
    assert not (np.diff(seen.astype(int), axis=2) > 0).any()            # a robot's slots fill from the first on


def test_table_advances_whoever_is_active():
    """Nobody active: the step still counts for the table, and a retired robot keeps p, seen and its record."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 2, 4, seed=3)
    obs, sinus = scattered(cfg, 5)
    o = oracle_for(cfg, max_inner=40, max_outer=2)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, retire=True, crowd=Crowd(obs, 2, 1e3, sinus=sinus, watch=True))
    free = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, crowd=Crowd(obs, 2, 1e3, sinus=sinus))
    fleet.step(o.warm_solve())
    free.step(o.warm_solve())
    fleet.active[:] = False                                     # everybody leaves at once
    P, seen, rec = fleet.P.copy(), fleet.crowd_seen.copy(), fleet.crowd_clearance().copy()
    for k in range(2):
        fleet.step(o.warm_solve())
        free.step(o.warm_solve())
        assert np.array_equal(fleet.crowd_table(), free.crowd_table())
        assert np.array_equal(fleet.P, P) and np.array_equal(fleet.crowd_seen, seen) and fleet.crowd_clearance().tobytes() == rec.tobytes()


def test_crowd_ellipses_move_between_free_points_of_the_scene():
    cfg = named_config("cfg4")
    pl = frontend.scene_planner(cfg, 11)
    p1, p2, freq, rx, ry, ang = crowd_ellipses(cfg, 11, 40, 7)
    assert p1.shape == p2.shape == (40, 2) and all(a.shape == (40,) for a in (freq, rx, ry, ang))
    grown = [frontend.offset_polygon(o, 0.25) for o in pl.obstacles]
    for p in np.concatenate([p1, p2]):
        assert frontend._point_in_polygon(tuple(p), pl.boundary, strict=True)
        assert not any(frontend._point_in_polygon(tuple(p), o, strict=False) for o in grown)
    assert ((freq >= 0.05) & (freq < 0.1)).all() and ((rx >= 0.3) & (rx < 1.0) & (ry >= 0.3) & (ry < 1.0)).all() and ((ang >= 0) & (ang < np.pi)).all()
    again = crowd_ellipses(cfg, 11, 40, 7)
    assert all(np.array_equal(a, b) for a, b in zip((p1, p2, freq, rx, ry, ang), again))
    assert not np.array_equal(p1, crowd_ellipses(cfg, 11, 40, 8)[0])


def test_crowd_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_crowd", "nmpc_loop_crowd", "nmpc_loop_set_crowd_monitor", "nmpc_loop_crowd_clearance"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
    m = re.search(r"typedef struct nmpc_crowd_clearance \{[^\n]*\n\s*double\s+([^;]+);\n\s*int32_t ([^;]+);\n\} nmpc_crowd_clearance;", header)
    assert m and [f.strip() for f in (m.group(1) + "," + m.group(2)).split(",")] == list(_lib.CROWD_CLEARANCE_DTYPE.names)
    assert _lib.CROWD_CLEARANCE_DTYPE.itemsize == 16
    assert lib.nmpc_loop_set_crowd(None, 1, None, 0.0, 1, 1.0) == -3 and lib.nmpc_loop_set_crowd_monitor(None) == -3
    assert lib.nmpc_loop_crowd(None, None, None) == -3 and lib.nmpc_loop_crowd_clearance(None, None) == -3
    rec = no_crowd_clearance(3)
    assert (rec["level"] == np.inf).all() and (rec["row"] == -1).all() and (rec["obstacle"] == -1).all()
