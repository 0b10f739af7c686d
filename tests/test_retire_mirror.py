"""Retirement on the host (``FleetRecedingHorizon(..., retire=True)``), with the oracle solving, and the C ABI
that carries it to the device (``nmpc_loop_set_retire``, ``nmpc_loop_active``, ``nmpc_loop_run``).

The rule is the reference's, per robot: ``PathGenerator.run`` drives one robot ``while not terminal`` (src/path_generator.py:290,397).
So a retiring fleet must equal, bit for bit, its robots driven one by one as ``TrajectoryGenerator.run`` drives one -- a
``RecedingHorizonRobot``, the oracle at B = 1, warm-started, until ``terminal()``.  With peers, a literal per-robot loop of the
four rules of section 5.9 plus the parked rule is written here.

The fleet (``workloads.staggered_fleet``): cfg 1, scene 1's own route and three planned ones, four robots per route standing 2, 5,
12 and 40 samples before its end.  Measured with the oracle on the CPU (libm sin / cos): the 16 robots retire after 10, 21, 35, 67,
6, 21, 34, 67, 14, 23, 35, 68, 6, 21, 34 and 90 steps (``retired_at``): 552 solves in 90 steps,
where lock step takes 1440; without retirement a robot leaves ``done`` again 13 times in 120 steps."""
import copy
import math
import os
import re

import numpy as np

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, named_config
from mpc_trajectory_generator_amd.trajectory import FleetRecedingHorizon, Peers, RecedingHorizonRobot
from mpc_trajectory_generator_amd.workloads import staggered_fleet

LIMIT = 120          # steps within which every robot of the fleet must have retired


def _alone(cfg, route, start, i0, o):
    """One robot as ``TrajectoryGenerator.run`` drives it, the oracle in the manager's place: -> (robot, P and idx of every step)."""
    robot = RecedingHorizonRobot(route, start, [], idx0=i0)
    u, y = np.zeros((1, cfg.n_u)), np.zeros((1, cfg.n1))
    terminal, Ps, idx = False, [], []
    while not terminal and len(Ps) < LIMIT:
        p = np.array(robot.parameters(), dtype=np.float64)[None, :]
        Ps.append(p[0])
        idx.append(robot.idx)
        u, y, _ = o.solve_batch(p, u0=u, y0=y)
        robot.apply(u[0])
        terminal = robot.terminal()
        robot.t += cfg.num_steps_taken
    assert terminal, "a robot of the fleet did not reach its goal"
    return robot, Ps, idx


def test_retiring_fleet_equals_its_robots_driven_alone():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    o = oracle_for(cfg)
    B, s = len(starts), cfg.num_steps_taken
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, retire=True)
    assert fleet.n_active == B and (fleet.retired_at == -1).all()
    Ps, idxs, n_solved = [], [], 0
    while fleet.n_active and fleet.steps < LIMIT:
        n_solved += fleet.n_active
        P, _ = fleet.step(o.warm_solve())
        Ps.append(P.copy())
        idxs.append(fleet.idx.copy())
    assert fleet.n_active == 0, f"{fleet.n_active} robots still active after {LIMIT} steps"
    at = fleet.retired_at
    print("retired_at", at.tolist(), "steps", fleet.steps, "solves", n_solved)
    assert len(set(at.tolist())) >= 3 and at.min() >= 1 and at.max() == fleet.steps
    assert n_solved == at.sum()
    T = np.stack(fleet.traj)
    assert T.shape == (fleet.steps * s + 1, B, 3)
    for b in range(B):
        robot, Pb, idx_b = _alone(cfg, routes[route_of[b]], starts[b], int(i0[b]), o)
        n = len(Pb)
        assert at[b] == n, f"robot {b}: retired after {at[b]} steps, alone it takes {n}"
        states = np.array(robot.states).reshape(n * s + 1, 3)
        assert np.array_equal(T[:n * s + 1, b], states), f"robot {b}: states"
        assert np.array_equal(T[n * s:, b], np.tile(states[-1], (len(T) - n * s, 1))), f"robot {b}: rows after retirement"
        assert np.array_equal(fleet.state[b], states[-1]) and fleet.done[b]
        for k in range(fleet.steps):                       # every P and idx, the last ones held from then on
            assert np.array_equal(Ps[k][b], Pb[min(k, n - 1)]), f"robot {b}, step {k}: P"
            assert int(idxs[k][b]) == idx_b[min(k, n - 1)], f"robot {b}, step {k}: idx"
        # the inputs: the plan the robot holds is its last solve's, whose first s controls are the last ones applied
        assert np.array_equal(fleet.U[b, :2 * s], robot.system_input[-2 * s:]), f"robot {b}: inputs"
        assert np.array_equal(fleet.last_u[b], robot.system_input[-2:]), f"robot {b}: last_u"


def test_retirement_latches():
    """Without retirement a robot that reached its goal leaves ``done`` again; with it nobody does."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    o = oracle_for(cfg)
    left = {}
    for retire in (False, True):
        fleet = FleetRecedingHorizon(routes, route_of, starts, None, idx0=i0, retire=retire)
        was, n = np.zeros(len(starts), dtype=bool), 0
        for _ in range(LIMIT):
            fleet.step(o.warm_solve())
            n += int((was & ~fleet.done).sum())
            was = fleet.done.copy()
        left[retire] = n
    print("robots leaving done:", left)
    assert left[False] >= 1
    assert left[True] == 0


def _slot0(cfg):
    return 20 + cfg.N_hor + 3 * cfg.Nobs


def literal_parked_peers(cfg, P, state, U, active, K, group_of, M, rx, ry, rng_, sincos1):
    """Section 5.9 robot by robot in Python floats, with the parked rule: a retired robot is predicted at its state at every stage,
    stays a candidate, and its own p is left alone.  -> (P overlaid, chosen [B][<= M])."""
    B, N, s, ts = len(state), cfg.N_hor, cfg.num_steps_taken, cfg.ts
    pred = []
    for j in range(B):
        x, y, th = (float(v) for v in state[j])
        if not active[j]:
            pred.append([(x, y, th)] * N)
            continue
        row = []
        for k in range(N):
            c = s + k if s + k < N else N - 1
            v, w = float(U[j][2 * c]), float(U[j][2 * c + 1])
            sn, cs = sincos1(th)
            x = x + ts * (v * cs)
            y = y + ts * (v * sn)
            th = th + ts * w
            row.append((x, y, th))
        pred.append(row)
    P = P.copy()
    chosen = []
    for b in range(B):
        if not active[b]:
            chosen.append([])
            continue
        cand = []
        for j in range(B):
            if j == b or group_of[j] != group_of[b]:
                continue
            D = math.inf
            for k in range(N):
                dx = pred[b][k][0] - pred[j][k][0]
                dy = pred[b][k][1] - pred[j][k][1]
                d = dx * dx + dy * dy
                if d < D:
                    D = d
            if D < rng_ * rng_:
                cand.append((D, j))
        cand.sort()
        chosen.append([j for _, j in cand[:M]])
        for m, j in enumerate(chosen[-1]):
            at = _slot0(cfg) + (K + m) * 5 * N
            for k in range(N):
                P[b, at + 5 * k:at + 5 * k + 5] = (pred[j][k][0], pred[j][k][1], rx, ry, pred[j][k][2])
    return P, chosen


def _twin_without_peers(fleet):
    """The same fleet at the same states, plans, carried blocks and active set, without peers; stepping it leaves ``fleet`` alone."""
    twin = copy.copy(fleet)
    twin.peers = None
    twin.P = fleet.P.copy()
    twin.dyn = fleet.dyn.copy()
    return twin


# the peers of the retirement tests, CPU and GPU: the robots of a route are a group (they drive to one goal, where the first to arrive
# parks in the way of the others), radii no padding ellipse has
PEERS = dict(slots=2, rx=0.37, ry=0.53, range=3.0)
PEER_STEPS = 40


def test_retiring_fleet_with_peers_equals_the_literal_rule():
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    o = oracle_for(cfg)
    B, K, M = len(starts), 0, PEERS["slots"]
    fleet = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, retire=True,
                                 peers=Peers(group_of=route_of, **PEERS))
    active = [True] * B                                    # the literal rule: everybody at first, out for good once terminal after a step
    retired_at = [-1] * B
    parked_seen = 0
    for k in range(PEER_STEPS):
        assert fleet.active.tolist() == active and fleet.retired_at.tolist() == retired_at, f"step {k}"
        twin = _twin_without_peers(fleet)
        held = (fleet.state, fleet.last_u, fleet.idx, fleet.U.copy(), fleet.Y.copy(), fleet.P.copy())
        P0 = twin.assemble().copy()
        want, chosen = literal_parked_peers(cfg, P0, fleet.state, fleet.U, active, K, route_of, M, PEERS["rx"], PEERS["ry"],
                                            PEERS["range"], o.sincos)
        P, _ = fleet.step(o.warm_solve())
        assert np.array_equal(P, want), f"step {k}: columns {np.unique(np.nonzero(P != want)[1])[:10]}"
        sel = [[j for j in row if j >= 0] for row in fleet.peer_index.tolist()]
        assert sel == chosen, f"step {k}"
        parked_seen += sum(1 for b in range(B) for j in chosen[b] if not active[j])
        out = [b for b in range(B) if not active[b]]       # a retired robot keeps every value of its last step
        for now, then in zip((fleet.state, fleet.last_u, fleet.idx, fleet.U, fleet.Y, fleet.P), held):
            assert np.array_equal(now[out], then[out]), f"step {k}"
        for b in range(B):
            end = routes[route_of[b]].end
            terminal = (abs(fleet.state[b, 0] - end[0]) <= 0.05 and abs(fleet.state[b, 1] - end[1]) <= 0.05
                        and abs(fleet.last_u[b, 0]) < 0.005)
            if active[b] and terminal:
                active[b], retired_at[b] = False, k + 1
    print("retired_at", retired_at, "parked robots chosen as peers:", parked_seen)
    assert 0 < sum(active) < B
    assert parked_seen > 0, "no retired robot was ever within range of an active groupmate"


def test_retire_functions_declared_exported_and_bound():
    names = ("nmpc_loop_set_retire", "nmpc_loop_active", "nmpc_loop_run")
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
