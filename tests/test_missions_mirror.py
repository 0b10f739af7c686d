"""Missions on the host (``FleetRecedingHorizon(..., retire=True, missions=Missions(...))``), with the oracle
solving, and the C ABI that carries them to the device (``nmpc_loop_set_missions``, ``nmpc_loop_legs``).

The rule is the reference's, per robot: its user calls ``PathGenerator.run(graph, start, end)`` again from where the robot stands
(src/main.py:23, src/path_generator.py:197-290).  So with K = 0 a mission robot must equal, bit for bit, its legs driven one after
another as ``TrajectoryGenerator.run`` drives one robot -- a fresh ``RecedingHorizonRobot`` per leg from the final pose of the leg
before, the oracle at B = 1 from u = y = 0, until ``terminal()``.  With scripted ellipses, peers and the monitor a literal per-robot
loop of the rule is written here.

The square (``SQUARE``, cfg 1): measured with the oracle on the CPU (libm sin / cos), one robot from (2, 2, 0) takes 33, 41, 69 and
36 steps for the four legs and reaches every goal."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, named_config
from mpc_trajectory_generator_amd.trajectory import (FleetRecedingHorizon, Missions, Monitor, Peers, RecedingHorizonRobot,
                                                     VectorizedRecedingHorizon)
from mpc_trajectory_generator_amd.workloads import clearance_differing, handmade_route, mission_fleet
from test_monitor_mirror import LiteralMonitor
from test_retire_mirror import literal_parked_peers

LEG_LIMIT = 150      # steps within which every leg must end

SQUARE = [(2.0, 2.0), (5.0, 2.0), (5.0, 4.5), (2.5, 4.5), (2.5, 2.5)]


def square_fleet(cfg):
    """-> (routes, route_of, starts, idx0, legs): four robots on the square with missions of 1, 2, 3 and 4 legs, started at corners
    3, 0, 1 and 0, each off its corner by an offset of its own, so that the re-dispatches fall in different steps."""
    offsets = [(0.02, -0.03, 0.05), (0.0, 0.0, 0.0), (-0.04, 0.03, -0.1), (0.03, 0.04, 0.15)]
    return mission_fleet(cfg, SQUARE, n_legs=(1, 2, 3, 4), first=(3, 0, 1, 0), offsets=offsets)


def _legs_alone(cfg, routes, legs, start, o):
    """One robot's legs one after another, each as ``TrajectoryGenerator.run`` drives a robot, the oracle in the manager's place:
    -> (P of every step, idx of every step, states [rows, 3], last_u, the step counts at which the legs ended)."""
    Ps, idx, ends = [], [], []
    states, pose, last_u = [np.array(start, dtype=np.float64)], start, None
    for r in legs:
        robot = RecedingHorizonRobot(routes[r], pose, [], idx0=0)
        u, y = np.zeros((1, cfg.n_u)), np.zeros((1, cfg.n1))
        terminal, n = False, 0
        while not terminal and n < LEG_LIMIT:
            p = np.array(robot.parameters(), dtype=np.float64)[None, :]
            Ps.append(p[0])
            idx.append(robot.idx)
            u, y, _ = o.solve_batch(p, u0=u, y0=y)
            robot.apply(u[0])
            terminal = robot.terminal()
            robot.t += cfg.num_steps_taken
            n += 1
        assert terminal, f"a leg did not end within {LEG_LIMIT} steps"
        ends.append(len(Ps))
        states += list(np.array(robot.states).reshape(-1, 3)[1:])
        pose, last_u = robot.states[-3:], robot.system_input[-2:]
    return Ps, idx, np.array(states), last_u, ends


def test_mission_fleet_equals_its_legs_driven_alone():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, legs = square_fleet(cfg)
    o = oracle_for(cfg)
    B, s = len(starts), cfg.num_steps_taken
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, retire=True, missions=Missions(legs))
    assert (fleet.leg == 0).all() and (fleet.leg_at == -1).all() and fleet.leg_at.shape == (B, 4)
    Ps, idxs, moved = [], [], []
    warm = o.warm_solve()

    def solve(P, U, Y):
        idxs.append(fleet.idx.copy())                      # the window search's answer of this step (a re-dispatch zeroes it after the advance)
        return warm(P, U, Y)

    while fleet.n_active and fleet.steps < 4 * LEG_LIMIT:
        before = fleet.leg.copy()
        P, _ = fleet.step(solve)
        Ps.append(P.copy())
        moved.append(np.nonzero(fleet.leg != before)[0].tolist())
    assert fleet.n_active == 0
    print("leg_at", fleet.leg_at.tolist(), "retired_at", fleet.retired_at.tolist())
    assert fleet.leg.tolist() == [0, 1, 2, 3] and fleet.route_of.tolist() == [3, 1, 3, 3]
    steps_moved = [k for k, m in enumerate(moved) if m]
    assert len(steps_moved) == 6, "the six re-dispatches do not fall in six different steps"
    T = np.stack(fleet.traj)
    assert T.shape == (fleet.steps * s + 1, B, 3)
    for b in range(B):
        Pb, idx_b, states, last_u, ends = _legs_alone(cfg, routes, legs[b], starts[b], o)
        n = len(Pb)
        assert fleet.leg_at[b].tolist() == ends + [-1] * (4 - len(ends)), f"robot {b}: leg_at"
        assert fleet.retired_at[b] == n, f"robot {b}: retired_at"
        assert np.array_equal(T[:n * s + 1, b], states), f"robot {b}: states"
        assert np.array_equal(T[n * s:, b], np.tile(states[-1], (len(T) - n * s, 1))), f"robot {b}: rows after retirement"
        assert np.array_equal(fleet.state[b], states[-1]) and fleet.done[b]
        for k in range(fleet.steps):
            assert np.array_equal(Ps[k][b], Pb[min(k, n - 1)]), f"robot {b}, step {k}: P"
            assert int(idxs[k][b]) == idx_b[min(k, n - 1)], f"robot {b}, step {k}: idx"
        assert np.array_equal(fleet.last_u[b], last_u), f"robot {b}: last_u"


# ---- scripted ellipses, peers and the monitor: a literal per-robot loop ----
# Two groups of two robots that never see each other, the second group a twin of the first (same starts, same ellipses), except that
# robot 2 has one leg where its twin, robot 0, has two.  Robots 0 and 2 therefore end their first leg in the same step: 0 is
# re-dispatched while 2 retires.  Robots 1 and 3 drive a longer leg 0.8 m beside, within the peers' range all the way: in the next step
# robot 1 finds the re-dispatched robot 0 standing still at every stage.
PAIR_CORNERS = ([(2.0, 2.0), (5.0, 2.0), (5.0, 4.5)], [(2.0, 1.2), (6.5, 1.2), (6.5, 3.0)])
PAIR_LEGS = [[0, 1], [2, 3], [0], [2, 3]]
PAIR_PEERS = dict(slots=1, rx=0.37, ry=0.53, range=3.0)
PAIR_GROUPS = np.array([0, 0, 1, 1], dtype=np.int32)
PAIR_STEPS_AFTER = 4


def pair_fleet(cfg):
    """-> (routes, route_of, starts, idx0, legs, dyn): the fleet above, one scripted ellipse per robot crossing beyond the first legs."""
    a, b = (mission_fleet(cfg, c, n_legs=(2,)) for c in PAIR_CORNERS)
    routes = a[0] + b[0]
    route_of = np.array([m[0] for m in PAIR_LEGS], dtype=np.int32)
    starts = np.array([routes[r].start for r in route_of], dtype=np.float64)
    B = len(starts)
    p1 = np.tile(np.array([[[3.5, 3.6]]]), (B, 1, 1))
    p2 = np.tile(np.array([[[6.5, 3.2]]]), (B, 1, 1))
    one = np.ones((B, 1))
    return routes, route_of, starts, np.zeros(B, dtype=np.int32), PAIR_LEGS, (p1, p2, 0.07 * one, 0.4 * one, 0.6 * one, 0.3 * one)


class LiteralMissions:
    """The rule of section 5.9 robot by robot: every robot is a one-robot ``VectorizedRecedingHorizon`` on its current route (the loop the
    other tests pin), peers by ``literal_parked_peers``, the monitor by ``LiteralMonitor``, and the dispatch written out below."""

    def __init__(self, cfg, routes, starts, legs, dyn, o, group_of, peers):
        self.cfg, self.routes, self.legs, self.dyn, self.o = cfg, routes, legs, dyn, o
        self.B = B = len(starts)
        self.group_of, self.peers = group_of, peers
        self.K = dyn[0].shape[1]
        self.robots = [self._fresh(b, legs[b][0], starts[b]) for b in range(B)]
        self.U, self.Y = np.zeros((B, cfg.n_u)), np.zeros((B, cfg.n1))
        self.P = np.zeros((B, cfg.n_p))
        self.active, self.retired_at = [True] * B, [-1] * B
        self.leg, self.route_of = [0] * B, [m[0] for m in legs]
        self.leg_at = [[-1] * len(m) for m in legs]
        self.steps = 0
        self.traj = [np.array(starts, dtype=np.float64)]
        self.monitor = LiteralMonitor(cfg, B, self.K, group_of, o.sincos)
        self.chosen = [[] for _ in range(B)]

    def _fresh(self, b, r, pose):
        return VectorizedRecedingHorizon(self.routes[r], [pose], tuple(a[b:b + 1] for a in self.dyn), sincos=self.o.sincos_array)

    def step(self):
        cfg, B, s = self.cfg, self.B, self.cfg.num_steps_taken
        drove = list(self.active)
        for b in range(B):
            if self.active[b]:
                self.P[b] = self.robots[b].assemble()[0]
        state = np.array([r.state[0] for r in self.robots])
        pe = self.peers
        self.P, self.chosen = literal_parked_peers(cfg, self.P, state, self.U, self.active, self.K, self.group_of, pe["slots"], pe["rx"],
                                                   pe["ry"], pe["range"], self.o.sincos)
        for b in range(B):
            if self.active[b]:
                u, y, _ = self.o.solve_batch(self.P[b:b + 1], u0=self.U[b:b + 1], y0=self.Y[b:b + 1])
                self.U[b], self.Y[b] = u[0], y[0]
                self.robots[b].advance(self.U[b:b + 1])
        rows = []
        for i in range(s):
            rows.append(np.array([r.traj[len(r.traj) - s + i][0] if drove[b] else r.state[0] for b, r in enumerate(self.robots)]))
        self.traj += rows
        self.monitor.update(self.steps, self.P, rows, drove)
        self.steps += 1
        for b in range(B):                                         # the rule
            robot = self.robots[b]
            if not (self.active[b] and robot.done[0]):
                continue
            self.leg_at[b][self.leg[b]] = self.steps
            if self.leg[b] + 1 < len(self.legs[b]):
                self.leg[b] += 1
                self.route_of[b] = self.legs[b][self.leg[b]]
                new = self._fresh(b, self.route_of[b], robot.state[0])           # idx = 0, last_u = (0, 0), done = 0
                new.t, new.dyn = robot.t, robot.dyn                               # the world's clock and the carried block go on
                self.robots[b] = new
                self.U[b], self.Y[b] = 0.0, 0.0
            else:
                self.active[b], self.retired_at[b] = False, self.steps


def _same_bytes(fleet, lit):
    """The names on which the mirror and the literal loop differ."""
    B = fleet.B
    pad = fleet.leg_at.shape[1]
    pairs = [("P", fleet.P, lit.P), ("U", fleet.U, lit.U), ("Y", fleet.Y, lit.Y),
             ("state", fleet.state, np.array([r.state[0] for r in lit.robots])),
             ("last_u", fleet.last_u, np.array([r.last_u[0] for r in lit.robots])),
             ("idx", fleet.idx, np.array([r.idx[0] for r in lit.robots])),
             ("done", fleet.done, np.array([r.done[0] for r in lit.robots])),
             ("active", fleet.active, np.array(lit.active)), ("retired_at", fleet.retired_at, np.array(lit.retired_at, dtype=np.int32)),
             ("leg", fleet.leg, np.array(lit.leg, dtype=np.int32)), ("route_of", fleet.route_of, np.array(lit.route_of)),
             ("leg_at", fleet.leg_at, np.array([m + [-1] * (pad - len(m)) for m in lit.leg_at], dtype=np.int32)),
             ("traj", np.stack(fleet.traj), np.stack(lit.traj))]
    bad = [n for n, x, y in pairs if np.asarray(x).tobytes() != np.asarray(y, dtype=np.asarray(x).dtype).tobytes()]
    return bad + clearance_differing(fleet.clearance, lit.monitor.records())


def run_pair_fleet(fleet, step):
    """Step the mirror of ``pair_fleet`` (``step(fleet)`` steps it once, and whatever is compared with it) until ``PAIR_STEPS_AFTER``
    steps after the one in which robot 0 is re-dispatched while robot 2 retires; -> that step.  That it came, and that robot 1 chose
    the re-dispatched robot 0 as its peer in the step after, are asserted."""
    both, chosen = None, False
    while fleet.steps < LEG_LIMIT and (both is None or fleet.steps < both + 1 + PAIR_STEPS_AFTER):
        leg, at = fleet.leg.copy(), fleet.retired_at.copy()
        step(fleet)
        if both is not None and fleet.steps == both + 2:
            chosen = fleet.peer_index[1, 0] == 0
        if fleet.leg[0] == leg[0] + 1 and at[2] < 0 <= fleet.retired_at[2]:
            both = fleet.steps - 1
            assert not fleet.U[0].any() and not fleet.Y[0].any() and fleet.active[0] and not fleet.done[0]
    assert both is not None, "no step in which one robot is re-dispatched while another retires"
    assert chosen, "the re-dispatched robot was not the chosen peer of the robot behind it"
    return both


def test_mission_fleet_with_ellipses_peers_and_monitor_equals_the_literal_rule():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, legs, dyn = pair_fleet(cfg)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, retire=True,
                                 peers=Peers(group_of=PAIR_GROUPS, **PAIR_PEERS), monitor=Monitor(group_of=PAIR_GROUPS),
                                 missions=Missions(legs))
    lit = LiteralMissions(cfg, routes, starts, legs, dyn, o, PAIR_GROUPS.tolist(), PAIR_PEERS)

    def step(fleet):
        fleet.step(o.warm_solve())
        lit.step()
        bad = _same_bytes(fleet, lit)
        assert not bad, f"step {fleet.steps - 1}: {bad}"
        sel = [[j for j in row if j >= 0] for row in fleet.peer_index.tolist()]
        assert sel == lit.chosen, f"step {fleet.steps - 1}"

    both = run_pair_fleet(fleet, step)
    print("re-dispatch and retirement in step", both, "leg_at", fleet.leg_at.tolist(), "retired_at", fleet.retired_at.tolist())
    assert np.isfinite(fleet.clearance["ellipse"]).all() and (fleet.clearance["ellipse_row"] >= 1).all()
    assert fleet.leg[0] == 1 and fleet.leg[2] == 0 and fleet.retired_at[2] == both + 1


# ---- a leg of a few centimetres ----
SHORT_CORNERS = [(2.0, 2.0), (4.0, 2.0), (4.02, 2.01), (4.0, 4.0)]
SHORT_LEG_STEPS = 1          # the steps the short leg takes: the robot stands within the tolerance of its goal, the cold solve keeps it there


def short_leg_fleet(cfg):
    return mission_fleet(cfg, SHORT_CORNERS, n_legs=(3,))


def test_a_leg_of_a_few_centimetres():
    """Its goal lies within the terminal tolerance of where the robot stands when it is re-dispatched: the leg is solved once and ends,
    a re-dispatch one step after another."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, legs = short_leg_fleet(cfg)
    o = oracle_for(cfg)
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, retire=True, missions=Missions(legs))
    while fleet.n_active and fleet.steps < 2 * LEG_LIMIT:
        fleet.step(o.warm_solve())
        if fleet.leg[0] == 1:
            st, end = fleet.state[0], routes[1].end
            assert abs(st[0] - end[0]) <= 0.05 and abs(st[1] - end[1]) <= 0.05, "the short leg's goal is not within the tolerance"
    at = fleet.leg_at[0]
    print("leg_at", at.tolist())
    assert fleet.n_active == 0 and (at > 0).all()
    assert at[1] - at[0] == SHORT_LEG_STEPS
    assert fleet.retired_at[0] == at[2] > at[1] + 1
    Pb, idx_b, states, last_u, ends = _legs_alone(cfg, routes, legs[0], starts[0], o)
    assert ends == at.tolist() and np.array_equal(np.stack(fleet.traj)[:, 0], states)


# ---- the interface ----
def test_missions_checked():
    m = Missions([[0, 1], [1]])
    off, route = m.checked(2, 2, [0, 1])
    assert off.tolist() == [0, 2, 3] and route.tolist() == [0, 1, 1] and off.dtype == route.dtype == np.int32
    for legs, B, R, route_of in (([[0, 1]], 2, 2, [0, 1]),              # a mission missing
                                 ([[0, 1], []], 2, 2, [0, 1]),          # a robot with no leg
                                 ([[0, 2], [1]], 2, 2, [0, 1]),         # a route out of range
                                 ([[0, -1], [1]], 2, 2, [0, 1]),
                                 ([[1, 0], [1]], 2, 2, [0, 1])):        # a first leg that is not route_of
        with pytest.raises(ValueError):
            Missions(legs).checked(B, R, route_of)
    cfg = named_config("cfg1")
    routes, route_of, starts, i0, legs = square_fleet(cfg)
    with pytest.raises(ValueError):
        FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, missions=Missions(legs))      # missions need retire=True


def test_mission_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    want = {"nmpc_loop_set_missions": ["nmpc_loop *l", "const int32_t *leg_off", "const int32_t *leg_route"],
            "nmpc_loop_legs": ["nmpc_loop *l", "int32_t *leg", "int32_t *route_of", "int32_t *leg_at"]}
    for name, params in want.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == params
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(params), name
    # additive: the ABI version stays
    assert re.search(r"#define NMPC_ABI_VERSION 3\b", header) and lib.nmpc_abi_version() == 3
    # a NULL loop is an argument error, before anything touches a device
    assert lib.nmpc_loop_set_missions(None, None, None) == -3 and lib.nmpc_loop_legs(None, None, None, None) == -3
