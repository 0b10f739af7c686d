"""The clearance monitor on the host (``FleetRecedingHorizon(..., monitor=Monitor(...))``), with the oracle
solving, and the C ABI that carries it to the device (``nmpc_loop_set_monitor``, ``nmpc_loop_clearance``).

The mirror's vectorised rule against a literal triple loop over robots, rows and obstacles written here in Python floats
(``LiteralMonitor``), byte for byte on the records after every step; the peer fields against pairwise distances taken with numpy from
the recorded trajectory; the two robots on reversed routes of tests/test_peers_mirror.py; the kinds of obstacle a fleet does not have;
and that a monitored mirror computes what the unmonitored one computes.

Measured with the oracle on the CPU: the case that records robots inside something (``INSIDE_CASE``) is the cfg 4 fleet with scripted
ellipses: after 10 steps 3 of its 12 robots have been inside a padded ellipse (smallest level 0.148, where 1 is the boundary).  On the
staggered fleet, whose robots of a route drive to one goal where the first to arrive parks, 8 of 16 robots come closer to a groupmate
than the two peer radii together (0.9 m; the closest pair 0.467 m) and nobody enters a circle (smallest clearance 0.066 m)."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, harness, named_config
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, Monitor, Peers, no_clearance
from mpc_trajectory_generator_amd.workloads import (PARITY_FIELDS, clearance_differing, fleet_ellipses, handmade_route, move_near_goal,
                                                    staggered_fleet)
from test_peers_mirror import HEAD_ON
from test_retire_mirror import PEERS

INF = math.inf


class LiteralMonitor:
    """The rule of section 5.9, robot by robot, row by row, obstacle by obstacle, in Python floats with ``math.sqrt`` and the oracle's
    sin / cos.  ``rec[b]`` = [circle, ellipse, peer2, circle_row, ellipse_row, peer_row, peer]."""

    def __init__(self, cfg, B, K, group_of, sincos1):
        self.cfg, self.B, self.K, self.sincos1 = cfg, B, K, sincos1
        self.group_of = [0] * B if group_of is None else [int(g) for g in group_of]
        self.rec = [[INF, INF, INF, -1, -1, -1, -1] for _ in range(B)]

    def update(self, step, P, rows, drove):
        """``rows`` [s][B][3]: the trajectory rows step ``step`` (0-based) appended; ``P`` [B][n_p] as its solve read them; ``drove`` [B]:
        the robots the step drove (a robot retired before it stands where its rows repeat)."""
        cfg, K = self.cfg, self.K
        N, Nobs, s = cfg.N_hor, cfg.Nobs, cfg.num_steps_taken
        assert len(rows) == s
        for b in range(self.B):
            if not drove[b]:
                continue
            rec = self.rec[b]
            p = [float(v) for v in P[b]]
            for i in range(s):
                r = step * s + 1 + i
                x, y = float(rows[i][b][0]), float(rows[i][b][1])
                for c in range(Nobs):
                    xc, yc, rc = p[20 + N + 3 * c], p[20 + N + 3 * c + 1], p[20 + N + 3 * c + 2]
                    if rc > 0:
                        dx = x - xc
                        dy = y - yc
                        v = math.sqrt(dx * dx + dy * dy) - rc
                        if v < rec[0] or (v == rec[0] and r < rec[3]):
                            rec[0], rec[3] = v, r
                for k in range(K):
                    at = 20 + N + 3 * Nobs + (k * N + i) * 5
                    ex, ey, rx, ry, A = p[at:at + 5]
                    dx = x - ex
                    dy = y - ey
                    sn, cs = self.sincos1(A)
                    a = dx * cs + dy * sn
                    c = dx * sn - dy * cs
                    v = (a * a) / (rx * rx) + (c * c) / (ry * ry)
                    if v < rec[1] or (v == rec[1] and r < rec[4]):
                        rec[1], rec[4] = v, r
                for j in range(self.B):
                    if j == b or self.group_of[j] != self.group_of[b]:
                        continue
                    dx = x - float(rows[i][j][0])
                    dy = y - float(rows[i][j][1])
                    v = dx * dx + dy * dy
                    if v < rec[2] or (v == rec[2] and (r < rec[5] or (r == rec[5] and j < rec[6]))):
                        rec[2], rec[5], rec[6] = v, r, j

    def records(self):
        out = np.empty(self.B, dtype=_lib.CLEARANCE_DTYPE)
        for b, rec in enumerate(self.rec):
            out[b] = tuple(rec)
        return out


def _stepped_against_literal(fleet, o, K, group_of, until):
    """Step ``fleet`` with the oracle until ``until(fleet)``; after every step its records must be the literal rule's bytes."""
    cfg, s = fleet.cfg, fleet.cfg.num_steps_taken
    lit = LiteralMonitor(cfg, fleet.B, K, group_of, o.sincos)
    assert not clearance_differing(fleet.clearance, no_clearance(fleet.B))
    while not until(fleet):
        drove = np.ones(fleet.B, dtype=bool) if fleet.active is None else fleet.active.copy()
        k = fleet.steps
        P, _ = fleet.step(o.warm_solve())
        lit.update(k, P, fleet.traj[-s:], drove)
        bad = clearance_differing(fleet.clearance, lit.records())
        assert not bad, f"step {k}: {bad}"
    return lit


def _staggered(monitor=True, **kw):
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, retire=True,
                                 peers=Peers(group_of=route_of, **PEERS), monitor=Monitor(group_of=route_of) if monitor else None, **kw)
    return cfg, o, route_of, fleet


def near_goal_cfg4_fleet(K=3):
    """12 robots on 3 planned routes of scene 11 under cfg 4, robots 0 to 3 started 2, 3, 5 and 8 samples before their routes' ends,
    K scripted ellipses each: -> (cfg, routes, route_of, starts, idx0, dyn)."""
    cfg = named_config("cfg4")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=31)
    starts, i0 = move_near_goal(routes, route_of, starts, i0, (2, 3, 5, 8))
    return cfg, routes, route_of, starts, i0, fleet_ellipses(routes, route_of, i0, K, 7)


INSIDE_CASE = "cfg4-ellipses"    # the case that records robots inside something: test_mirror_equals_literal_rule_with_scripted_ellipses


def test_mirror_equals_literal_rule_on_the_staggered_fleet():
    """Peers and retirement on, monitor groups = the routes, until three robots have retired and the others have passed them for a
    few steps: robots that retire in the step that still updates them, and parked robots seen by the others."""
    cfg, o, route_of, fleet = _staggered()
    _stepped_against_literal(fleet, o, 0, route_of, lambda f: (f.retired_at >= 0).sum() >= 3 and f.steps >= 14 or f.steps >= 40)
    at = fleet.retired_at
    assert (at >= 0).sum() >= 3 and fleet.n_active > 0
    rec = fleet.clearance
    print("retired_at", at.tolist(), "closest pair", float(np.sqrt(rec["peer2"].min())), "closest circle", float(rec["circle"].min()))
    # a robot's record stops with its retirement, and it is still seen afterwards: a record of an active robot names a parked one
    s = cfg.num_steps_taken
    for b in np.nonzero(at >= 0)[0]:
        assert max(rec["circle_row"][b], rec["peer_row"][b]) <= at[b] * s
    parked = np.nonzero(at >= 0)[0]
    seen = [b for b in range(fleet.B) if rec["peer"][b] in parked and rec["peer_row"][b] > at[rec["peer"][b]] * s]
    assert seen, "no record names a groupmate at a row after that groupmate's retirement"
    assert (rec["ellipse"] == INF).all() and (rec["ellipse_row"] == -1).all()                   # K = 0
    two_radii = PEERS["rx"] + PEERS["ry"]
    inside = rec["peer2"] < two_radii * two_radii
    print("robots closer to a groupmate than", two_radii, "m:", int(inside.sum()), "of", fleet.B)
    assert inside.any(), "nobody came closer to a groupmate than the sum of the peer radii"
    assert (rec["circle"] > 0).all()


def test_mirror_equals_literal_rule_with_scripted_ellipses():
    """cfg 4, K = 3 with the sinusoidal law, retirement, one monitor group, 10 steps."""
    cfg, routes, route_of, starts, i0, dyn = near_goal_cfg4_fleet()
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, sinus_object=True, idx0=i0, retire=True,
                                 monitor=Monitor())
    _stepped_against_literal(fleet, o, 3, None, lambda f: f.steps >= 10)
    rec = fleet.clearance
    print("retired_at", fleet.retired_at.tolist(), "smallest ellipse level", float(rec["ellipse"].min()),
          "robots inside an ellipse", int((rec["ellipse"] < 1).sum()))
    assert 0 < fleet.n_active < fleet.B, "no step with some robots retired and others active"
    assert (rec["ellipse_row"] >= 1).all() and (rec["circle_row"] >= 1).all() and (rec["peer_row"] >= 1).all()
    assert np.isfinite(rec["ellipse"]).all() and (rec["ellipse"] >= 0).all()
    assert len(set(rec["ellipse_row"].tolist())) > 1
    assert INSIDE_CASE == "cfg4-ellipses" and (rec["ellipse"] < 1).any(), "no robot was ever inside a padded ellipse"


def test_peer_fields_equal_pairwise_distances_of_the_trajectory():
    """Without retirement: peer2[b] = the minimum over the rows T[1:] and the groupmates j of |T[r, b] - T[r, j]|^2, and
    (peer_row, peer) its first arg-min in (row, robot) order."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=5)
    o = oracle_for(cfg)
    group_of = (np.arange(12) % 2 * 7).astype(np.int32)                  # two groups of six, ids 0 and 7
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, monitor=Monitor(group_of=group_of))
    for _ in range(8):
        fleet.step(o.warm_solve())
    T = np.stack(fleet.traj)
    rec = fleet.clearance
    for b in range(12):
        dx, dy = T[1:, b, None, 0] - T[1:, :, 0], T[1:, b, None, 1] - T[1:, :, 1]
        d = dx * dx + dy * dy                                            # [rows, B]
        d[:, (group_of != group_of[b]) | (np.arange(12) == b)] = np.inf
        r, j = np.unravel_index(np.argmin(d), d.shape)
        assert (rec["peer2"][b], rec["peer_row"][b], rec["peer"][b]) == (d[r, j], r + 1, j), b


def _head_on_with_monitor(peers):
    """``test_peers_mirror._head_on`` with a monitor: -> (the smallest separation over the rows >= 1 as that test computes it, the record)."""
    cfg = named_config("cfg1")
    pl = frontend.scene_planner(cfg, 5)
    a, b = HEAD_ON["a"], HEAD_ON["b"]
    there = pl.route(a, b)
    back = pl.route((b[0], b[1], math.pi), (a[0], a[1], math.pi))
    o = oracle_for(cfg)
    starts = np.array([there.start, back.start])
    fleet = FleetRecedingHorizon([there, back], [0, 1], starts, None, sincos=o.sincos_array, monitor=Monitor(),
                                 peers=Peers(slots=1, rx=HEAD_ON["rx"], ry=HEAD_ON["ry"], range=HEAD_ON["range"]) if peers else None)
    for _ in range(400):
        fleet.step(o.warm_solve(threads=2))
        s = fleet.state
        if s[0, 0] > s[1, 0] + 1.0:                                        # both past the meeting point
            break
    else:
        raise AssertionError("the robots never passed each other")
    T = np.stack(fleet.traj)
    return float(np.linalg.norm(T[1:, 0, :2] - T[1:, 1, :2], axis=1).min()), fleet.clearance


def test_robots_on_reversed_routes_record_their_separation():
    """The monitor's sqrt(peer2) is test_robots_on_reversed_routes_keep_apart's own figure taken over the rows >= 1 (the monitor does
    not look at the start row), the same for both robots, and smaller without peers than with."""
    sep = {}
    for peers in (False, True):
        want, rec = _head_on_with_monitor(peers)
        got = np.sqrt(rec["peer2"])
        assert got[0] == got[1] == want, (peers, got, want)
        assert rec["peer"].tolist() == [1, 0] and rec["peer_row"][0] == rec["peer_row"][1] >= 1
        sep[peers] = float(got[0])
    print(f"smallest separation by the monitor: without peers {sep[False]:.4f} m, with peers {sep[True]:.4f} m")
    assert sep[False] < HEAD_ON["ry"]
    assert sep[False] < sep[True]


def test_kinds_a_fleet_does_not_have_keep_the_initial_record():
    cfg = named_config("cfg1")
    o = oracle_for(cfg, max_inner=40, max_outer=2)
    none = no_clearance(1)[0]
    # K = 0 and groups of one: scene 1's route has vertices
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 1, 2, 6, seed=3)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0,
                                 monitor=Monitor(group_of=np.arange(6, dtype=np.int32)[::-1].copy()))
    for _ in range(3):
        fleet.step(o.warm_solve())
    rec = fleet.clearance
    for f in ("ellipse", "ellipse_row", "peer2", "peer_row", "peer"):
        assert (rec[f] == none[f]).all(), f
    assert np.isfinite(rec["circle"]).all() and (rec["circle_row"] >= 1).all()
    # a route without vertices: every circle slot has radius 0
    route = handmade_route(cfg, harness.SCENES[1]["waypoints"])
    assert len(route.vertices) == 0
    starts = np.array([[route.x_ref[k], route.y_ref[k], route.theta_ref[k]] for k in (0, 10, 20)])
    fleet = FleetRecedingHorizon([route], np.zeros(3, dtype=np.int32), starts, None, sincos=o.sincos_array, idx0=[0, 10, 20], monitor=Monitor())
    for _ in range(3):
        P, _ = fleet.step(o.warm_solve())
    assert (P[:, 20 + cfg.N_hor:20 + cfg.N_hor + 3 * cfg.Nobs] == 0).all()
    rec = fleet.clearance
    for f in ("circle", "circle_row", "ellipse", "ellipse_row"):
        assert (rec[f] == none[f]).all(), f
    assert np.isfinite(rec["peer2"]).all() and (rec["peer"] >= 0).all()


def test_monitor_observes_only():
    """P, U, Y, states and trajectory of a monitored mirror are the unmonitored one's at every step (peers, retirement and scripted
    ellipses on)."""
    cfg, routes, route_of, starts, i0, dyn = near_goal_cfg4_fleet(K=2)
    o = oracle_for(cfg)
    peers = Peers(slots=1, rx=0.37, ry=0.53, range=5.0)
    a, b = (FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, retire=True, peers=peers, monitor=m)
            for m in (Monitor(group_of=route_of), None))
    for k in range(8):
        Pa, sa = a.step(o.warm_solve())
        Pb, sb = b.step(o.warm_solve())
        for x, y in ((Pa, Pb), (a.U, b.U), (a.Y, b.Y), (a.state, b.state), (a.last_u, b.last_u), (a.idx, b.idx), (a.done, b.done),
                     (a.retired_at, b.retired_at)) + tuple((sa[f], sb[f]) for f in PARITY_FIELDS):
            assert x.tobytes() == y.tobytes(), k
    assert np.array_equal(np.stack(a.traj), np.stack(b.traj))
    assert np.isfinite(a.clearance["peer2"]).all() and not hasattr(b, "clearance")


def test_monitor_groups_checked():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 1, 4, seed=3)
    FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, monitor=Monitor(group_of=[3, 3, 0, 1]))
    for bad in ([0, 1, 4, 0], [0, -1, 0, 0]):
        with pytest.raises(ValueError):
            FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, monitor=Monitor(group_of=bad))


def test_monitor_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_monitor", "nmpc_loop_clearance"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
    m = re.search(r"typedef struct nmpc_clearance \{[^\n]*\n\s*double ([^;]+);\n\s*int32_t ([^;]+);\n\} nmpc_clearance;", header)
    assert m and [f.strip() for f in (m.group(1) + "," + m.group(2)).split(",")] == list(_lib.CLEARANCE_DTYPE.names)
    assert _lib.CLEARANCE_DTYPE.itemsize == 40
    assert lib.nmpc_loop_set_monitor(None, None) == -3 and lib.nmpc_loop_clearance(None, None) == -3
