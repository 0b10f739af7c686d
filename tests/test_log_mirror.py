"""The drive log on the host (``FleetRecedingHorizon(..., log=DriveLog())``), with the oracle solving, and the C
ABI that carries it to the device (``nmpc_loop_set_log``, ``nmpc_loop_log``, ``nmpc_loop_drive_summary``, ``nmpc_loop_step_totals``).

The controls and exit statuses against ``TrajectoryGenerator.run`` -- the reference's own loop -- given the same solver; the mirror's
vectorised rule against a literal loop over robots written here in Python floats (``LiteralLog``), byte for byte on all four products
after every step, on every fleet tests/test_gpu_log_loop.py drives (``log_fleet``); that a logged mirror computes what the unlogged one
computes; and, on the oracle, that those fleets contain what the device cases are there for: a solve that does not converge, a robot
that retires among active ones, a leg boundary, a solve out of its iteration budget and an ``inner_max`` decided by a tie.

Clock fields (``solve_time_ms``, ``solve_ms_max``) are copied, not computed: they are compared here too (the mirror and the literal
loop read the same statuses), and left out by ``log_differing`` where a device is compared."""
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, harness, named_config
from mpc_trajectory_generator_amd.config import JCONF_3, load_config
from mpc_trajectory_generator_amd.trajectory import (DriveLog, FleetRecedingHorizon, Missions, Monitor, Peers, TrajectoryGenerator,
                                                     no_drive_summary, no_step_records, no_step_totals)
from mpc_trajectory_generator_amd.workloads import (LOG_PRODUCTS, PARITY_FIELDS, fleet_ellipses, log_differing, mission_fleet, staggered_fleet)
from test_loop_shapes_mirror import large_group_fleet
from test_monitor_mirror import near_goal_cfg4_fleet
from test_retire_mirror import PEERS

# ---- the fleets of the device cases (tests/test_gpu_log_loop.py), each the smallest that reaches what its name says ----
MISSION_CORNERS = [(2.0, 2.0), (3.2, 2.0), (3.2, 3.1), (2.2, 3.1)]      # legs of about a metre: a leg ends within a few steps
TIE_ROBOT, TIE_TWIN = 230, 299       # group300: robot 299 is made a twin of 230, whose first solve is the fleet's longest (measured on the oracle)
BUDGET = 40


def log_fleet(which):
    """-> dict(cfg, routes, route_of, starts, idx0, dyn, sinus, peers, retire, missions, opts, steps): ``opts`` = the solver options
    (``BatchSolver`` and the oracle take the same names)."""
    base = dict(dyn=None, sinus=False, peers=None, retire=False, missions=None, opts={})
    if which == "one-robot":
        cfg = named_config("cfg4")
        routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 1, 1, seed=9)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, dyn=fleet_ellipses(routes, route_of, i0, 2, 4),
                               steps=5)}
    if which == "cfg1-three-routes":
        cfg = named_config("cfg1")
        routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=5)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, steps=8)}
    if which == "cfg4-ellipses-retire":
        cfg, routes, route_of, starts, i0, dyn = near_goal_cfg4_fleet()
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, dyn=dyn, sinus=True, retire=True, steps=10)}
    if which == "staggered-peers":
        cfg = named_config("cfg1")
        routes, route_of, starts, i0 = staggered_fleet(cfg)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, peers=Peers(group_of=route_of, **PEERS),
                               retire=True, steps=14)}
    if which == "missions-3-legs":
        cfg = named_config("cfg1")
        offsets = [(0.02, -0.03, 0.05), (0.0, 0.0, 0.0), (-0.04, 0.03, -0.1)]
        routes, route_of, starts, i0, legs = mission_fleet(cfg, MISSION_CORNERS, n_legs=(1, 2, 3), first=(2, 1, 0), offsets=offsets)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, retire=True, missions=Missions(legs), steps=None)}
    if which == "cfg2-s3":
        cfg = load_config(**{**JCONF_3, "N_hor": 40, "num_steps_taken": 3})
        routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 2, 8, seed=13)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, steps=6)}
    if which == "group300":
        cfg, routes, route_of, starts, i0, _ = large_group_fleet()
        route_of, starts, i0 = route_of.copy(), starts.copy(), i0.copy()
        route_of[TIE_TWIN], starts[TIE_TWIN], i0[TIE_TWIN] = route_of[TIE_ROBOT], starts[TIE_ROBOT], i0[TIE_ROBOT]
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, steps=3)}
    if which == "budget40":
        cfg = named_config("cfg1")
        routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=5)
        return {**base, **dict(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=i0, opts={"max_total_inner": BUDGET}, steps=4)}
    raise KeyError(which)


LOG_FLEETS = ["one-robot", "cfg1-three-routes", "cfg4-ellipses-retire", "staggered-peers", "missions-3-legs", "cfg2-s3", "group300", "budget40"]
MISSION_STEP_LIMIT = 120      # steps within which the three-leg mission must be over


def mirror_of(f, o, log=True, **more):
    """-> the fleet's host mirror; ``o`` gives the kernels' sin / cos"""
    return FleetRecedingHorizon(f["routes"], f["route_of"], f["starts"], f["dyn"], sincos=o.sincos_array, idx0=f["idx0"], sinus_object=f["sinus"],
                                peers=f["peers"], retire=f["retire"], missions=f["missions"], log=DriveLog() if log else None, **more)


def run_over(f, host):
    """Has the fleet's run ended after the steps ``host`` took?  (the missions run until everybody has retired)"""
    if f["steps"] is not None:
        return host.steps >= f["steps"]
    assert host.steps < MISSION_STEP_LIMIT, f"the mission is not over after {MISSION_STEP_LIMIT} steps"
    return host.n_active == 0


class LiteralLog:
    """The rule of section 5.9 robot by robot in Python scalars: floats, ``math.sqrt``, ``abs`` and comparisons, word for word."""

    def __init__(self, cfg, B):
        self.cfg, self.B = cfg, B
        self.ctrl, self.rec, self.tot = [], [], []
        self.sum = [dict(steps=0, rows=0, exits=[0] * 5, inner_max=0, inner_total=0, inner_max_step=-1, f2_max_step=-1, length=0.0,
                         v_abs_max=0.0, w_abs_max=0.0, acc_abs_max=0.0, wacc_abs_max=0.0, acc_sq_sum=0.0, wacc_sq_sum=0.0, f2_max=0.0)
                    for _ in range(B)]

    def update(self, step, P, U, st, rows, drove, leg):
        """``step``: 1-based; ``P`` [B][n_p] as the solve read them, ``U`` [B][n_u] as the advance applied them, ``st`` [B] the step's
        statuses, ``rows`` [s + 1][B][3] the trajectory from the row before the step's first, ``drove`` [B], ``leg`` [B] before the dispatch."""
        s, ts, B = self.cfg.num_steps_taken, self.cfg.ts, self.B
        ctrl = [[[0.0, 0.0] for _ in range(B)] for _ in range(s)]
        rec = [(-1, 0, 0, 0, 0.0, 0.0, 0.0)] * B
        tot = dict(solved=0, exits=[0] * 5, inner_max=0, inner_max_robot=0, inner_total=0, solve_ms_max=0.0)
        for b in range(B):
            if not drove[b]:
                continue
            e, inner, outer = int(st["exit_status"][b]), int(st["num_inner_iterations"][b]), int(st["num_outer_iterations"][b])
            cost, f2, ms = float(st["cost"][b]), float(st["f2_norm"][b]), float(st["solve_time_ms"][b])
            rec[b] = (e, int(leg[b]), inner, outer, cost, f2, ms)
            m = self.sum[b]
            m["steps"] += 1
            m["rows"] += s
            m["exits"][e] += 1
            m["inner_total"] += inner
            if inner > m["inner_max"]:
                m["inner_max"], m["inner_max_step"] = inner, step
            if f2 > m["f2_max"]:
                m["f2_max"], m["f2_max_step"] = f2, step
            v_prev, w_prev = float(P[b][3]), float(P[b][4])
            for i in range(s):
                v, w = float(U[b][2 * i]), float(U[b][2 * i + 1])
                ctrl[i][b] = [v, w]
                dx = float(rows[i + 1][b][0]) - float(rows[i][b][0])
                dy = float(rows[i + 1][b][1]) - float(rows[i][b][1])
                m["length"] = m["length"] + math.sqrt(dx * dx + dy * dy)
                if abs(v) > m["v_abs_max"]:
                    m["v_abs_max"] = abs(v)
                if abs(w) > m["w_abs_max"]:
                    m["w_abs_max"] = abs(w)
                a = (v - v_prev) / ts
                wa = (w - w_prev) / ts
                if abs(a) > m["acc_abs_max"]:
                    m["acc_abs_max"] = abs(a)
                if abs(wa) > m["wacc_abs_max"]:
                    m["wacc_abs_max"] = abs(wa)
                m["acc_sq_sum"] = m["acc_sq_sum"] + a * a
                m["wacc_sq_sum"] = m["wacc_sq_sum"] + wa * wa
                v_prev, w_prev = v, w
            # the totals: robots come in ascending index, so a strictly larger count is the only way to take the record over
            if tot["solved"] == 0 or inner > tot["inner_max"]:
                tot["inner_max"], tot["inner_max_robot"] = inner, b
            tot["solved"] += 1
            tot["exits"][e] += 1
            tot["inner_total"] += inner
            if ms > tot["solve_ms_max"]:
                tot["solve_ms_max"] = ms
        self.ctrl += ctrl
        self.rec.append(rec)
        self.tot.append(tot)

    def products(self):
        """-> the four products as the arrays ``log_differing`` takes"""
        steps, B = len(self.rec), self.B
        rec = no_step_records(steps, B)
        for k in range(steps):
            for b in range(B):
                rec[k, b] = self.rec[k][b]
        summary = no_drive_summary(B)
        for b, m in enumerate(self.sum):
            for f in summary.dtype.names:
                summary[f][b] = m[f]
        tot = no_step_totals(steps)
        for k, t in enumerate(self.tot):
            for f in tot.dtype.names:
                tot[f][k] = t[f]
        return {"controls": np.array(self.ctrl, dtype=np.float64).reshape(-1, B, 2), "step_records": rec, "drive_summary": summary, "step_totals": tot}


def clock_fields_differing(a, b):
    """The two fields ``log_differing`` leaves out, for two hosts that read the same statuses"""
    return [n for n, x, y in (("solve_time_ms", a["step_records"]["solve_time_ms"], b["step_records"]["solve_time_ms"]),
                              ("solve_ms_max", a["step_totals"]["solve_ms_max"], b["step_totals"]["solve_ms_max"])) if x.tobytes() != y.tobytes()]


def host_products(host):
    return {name: getattr(host, name) for name in LOG_PRODUCTS}


# what a run must have contained, per fleet (checked on the oracle: the device cases cannot pass emptily)
def _covers_retirement(host, seen):
    assert seen["retired_among_active"], "no step with some robots retired and others active"
    at, rec, ctrl, s = host.retired_at, host.step_records, host.controls, host.cfg.num_steps_taken
    b = int(np.nonzero(at >= 0)[0][0])
    assert rec["exit_status"][at[b] - 1, b] >= 0, "a robot is not logged in the step that retires it"
    assert (rec["exit_status"][at[b]:, b] == -1).all() and not ctrl[at[b] * s:, b].any() and not np.signbit(ctrl[at[b] * s:, b]).any()
    assert host.drive_summary["steps"][b] == at[b] and host.drive_summary["rows"][b] == at[b] * s
    assert host.step_totals["solved"][-1] < host.B and (np.diff(host.step_totals["solved"]) <= 0).all()


def _covers_missions(host, seen):
    rec, ctrl, s = host.step_records, host.controls, host.cfg.num_steps_taken
    assert host.leg.tolist() == [0, 1, 2] and host.n_active == 0
    crossed = 0
    for b in range(host.B):
        for at in host.leg_at[b][:host.leg[b]]:                 # the steps (1-based) at which a leg ended and another began
            crossed += 1
            assert rec["leg"][at, b] == rec["leg"][at - 1, b] + 1, "leg does not step up by one behind a leg boundary"
            assert ctrl[at * s - 1, b].any(), "the last control of the leg is 0"
            assert (seen["P"][at][b, 3:5] == 0).all(), "p[3:5] is not 0 in the step after a re-dispatch"
    assert crossed == 3


def _covers_budget(host, seen):
    assert host.drive_summary["exits"][:, 2].sum() > 0, "no solve ran out of its iteration budget"
    assert host.drive_summary["inner_max"].max() == BUDGET
    assert seen["ties"] > 0


def _covers_tie(host, seen):
    tot, rec = host.step_totals, host.step_records
    assert tot["inner_max_robot"][0] == TIE_ROBOT and rec["num_inner_iterations"][0, TIE_TWIN] == tot["inner_max"][0], \
        "TIE_ROBOT's first solve is not the fleet's longest: choose the robot that has it"
    assert seen["ties"] > 0


COVERS = {"cfg4-ellipses-retire": _covers_retirement, "staggered-peers": _covers_retirement, "missions-3-legs": _covers_missions,
          "budget40": _covers_budget, "group300": _covers_tie}


@pytest.mark.parametrize("which", LOG_FLEETS)
def test_mirror_equals_literal_rule(which):
    """All four products after every step, byte for byte, on every fleet of the device cases; then what the fleet is there for."""
    f = log_fleet(which)
    cfg, s = f["cfg"], f["cfg"].num_steps_taken
    o = oracle_for(cfg, **f["opts"])
    host = mirror_of(f, o)
    lit = LiteralLog(cfg, host.B)
    assert not log_differing(host_products(host), {"controls": np.zeros((0, host.B, 2)), "step_records": no_step_records(0, host.B),
                                                   "drive_summary": no_drive_summary(host.B), "step_totals": no_step_totals(0)})
    seen = dict(retired_among_active=False, ties=0, P=[], not_converged=0)
    warm, applied = o.warm_solve(threads=16), [None]

    def solve(P, U, Y):
        out = warm(P, U, Y)
        applied[0] = out[0].copy()                              # the controls the advance applies, for the rows solved
        return out

    while not run_over(f, host):
        drove = np.ones(host.B, dtype=bool) if host.active is None else host.active.copy()
        leg = host.leg.copy() if f["missions"] is not None else np.zeros(host.B, dtype=np.int32)
        before = host.drive_summary.copy()
        P, st = host.step(solve)
        seen["P"].append(P.copy())
        U = np.zeros((host.B, cfg.n_u))
        U[drove] = applied[0]                                   # (a re-dispatch has zeroed the mirror's own rows by now)
        lit.update(host.steps, P, U, st, host.traj[-s - 1:], drove, leg)
        got, want = host_products(host), lit.products()
        bad = log_differing(got, want) + clock_fields_differing(got, want)
        assert not bad, f"step {host.steps}: {bad}"
        assert host.drive_summary[~drove].tobytes() == before[~drove].tobytes(), "a retired robot's summary moved"
        seen["retired_among_active"] |= bool(0 < drove.sum() < host.B)
        inner = st["num_inner_iterations"][drove]
        seen["ties"] += int(drove.any() and (inner == inner.max()).sum() > 1)
        seen["not_converged"] += int((st["exit_status"][drove] != 0).sum())
    tot, summary = host.step_totals, host.drive_summary
    print(which, "steps", host.steps, "solves", int(tot["solved"].sum()), "exits", tot["exits"].sum(axis=0).tolist(), "steps with a tie at the top",
          seen["ties"], "longest path", float(summary["length"].max()), "largest |a|", float(summary["acc_abs_max"].max()))
    assert tot["solved"].sum() == summary["steps"].sum() and (tot["exits"].sum(axis=0) == summary["exits"].sum(axis=0)).all()
    assert tot["inner_total"].sum() == summary["inner_total"].sum()
    assert (summary["length"] > 0).all() and (summary["v_abs_max"] > 0).all() and (summary["inner_max_step"] >= 1).all()
    if which in COVERS:
        COVERS[which](host, seen)


def test_some_solve_of_the_fleets_does_not_converge():
    """On the oracle, with default options: the exit counters of the device cases are not all ``Converged``."""
    f = log_fleet("cfg4-ellipses-retire")
    o = oracle_for(f["cfg"])
    host = mirror_of(f, o)
    while not run_over(f, host):
        host.step(o.warm_solve(threads=16))
    exits = host.step_totals["exits"].sum(axis=0)
    print("exits", exits.tolist())
    assert exits[1:].sum() > 0 and exits[0] > 0


class OracleManager:
    """The oracle in the place of the reference's TCP manager: one solve per call, warm-started from the call before (the server's
    behaviour), answering as ``mpc_step`` reads it.  Keeps the statuses it handed out."""

    class _Response:
        def __init__(self, data):
            self._data = data

        def is_ok(self):
            return True

        def get(self):
            return self._data

    def __init__(self, o):
        self.o, self.u, self.y, self.statuses = o, None, None, []

    def start(self):
        pass

    def ping(self):
        return {"Pong": 1}

    def kill(self):
        pass

    def call(self, p):
        p = np.array(p, dtype=np.float64)[None, :]
        self.u, self.y, st = self.o.solve_batch(p, u0=self.u, y0=self.y)
        self.statuses.append(st[0].copy())

        class Data:
            solution = [float(v) for v in self.u[0]]
            exit_status = _lib.EXIT_STATUS[int(st["exit_status"][0])]
            solve_time_ms = float(st["solve_time_ms"][0])
        return self._Response(Data)


@pytest.mark.parametrize("name, controls", [("cfg1", 24), ("cfg4", 24)])
def test_controls_and_exits_equal_the_reference_driver(name, controls):
    """One robot on scene 1 (cfg 1: s = 1; cfg 4: s = 2): ``controls[:, 0]`` is ``TrajectoryGenerator.run``'s (uv, uomega), the records'
    exit statuses are the statuses that driver saw, and the solve times the ones it returned."""
    cfg = named_config(name)
    assert cfg.num_steps_taken == (2 if name == "cfg4" else 1)
    route = dataclasses.replace(harness.scene_route(cfg, 1), dyn_obs_list=[])
    o = oracle_for(cfg)
    mng = OracleManager(o)
    gen = TrajectoryGenerator(cfg, manager_factory=lambda: mng)
    xx, xy, uv, uomega, solver_times, _ = gen.run(route, max_steps=controls)
    steps = controls // cfg.num_steps_taken
    assert len(uv) == controls and len(mng.statuses) == steps
    host = FleetRecedingHorizon([route], [0], [route.start], None, log=DriveLog())
    for _ in range(steps):
        host.step(o.warm_solve(threads=1))
    ctrl, rec = host.controls, host.step_records
    assert ctrl.shape == (controls, 1, 2)
    assert ctrl[:, 0, 0].tolist() == uv and ctrl[:, 0, 1].tolist() == uomega
    assert rec["exit_status"][:, 0].tolist() == [int(st["exit_status"]) for st in mng.statuses]
    for f in ("num_inner_iterations", "num_outer_iterations", "cost", "f2_norm"):
        assert rec[f][:, 0].tobytes() == np.array([st[f] for st in mng.statuses], dtype=rec[f].dtype).tobytes(), f
    T = np.stack(host.traj)
    assert T[:, 0, 0].tolist() == xx and T[:, 0, 1].tolist() == xy
    # report.fleet_runs gives the driver's tuple back
    from mpc_trajectory_generator_amd import report
    run, = report.fleet_runs(host)
    assert run[:4] == (xx, xy, uv, uomega) and len(run[4]) == len(solver_times) == steps
    assert "Solver calls" in report.fleet_runtime_text(host)


def test_log_observes_only():
    """P, U, Y, states, statuses and trajectory of a logged mirror are the unlogged one's at every step (peers, retirement, monitor and
    scripted ellipses on)."""
    cfg, routes, route_of, starts, i0, dyn = near_goal_cfg4_fleet(K=2)
    o = oracle_for(cfg)
    peers = Peers(slots=1, rx=0.37, ry=0.53, range=5.0)
    a, b = (FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, retire=True, peers=peers,
                                 monitor=Monitor(group_of=route_of), log=log) for log in (DriveLog(), None))
    for k in range(8):
        Pa, sa = a.step(o.warm_solve())
        Pb, sb = b.step(o.warm_solve())
        for x, y in ((Pa, Pb), (a.U, b.U), (a.Y, b.Y), (a.state, b.state), (a.last_u, b.last_u), (a.idx, b.idx), (a.done, b.done),
                     (a.retired_at, b.retired_at), (a.clearance, b.clearance)) + tuple((sa[f], sb[f]) for f in PARITY_FIELDS):
            assert x.tobytes() == y.tobytes(), k
    assert np.array_equal(np.stack(a.traj), np.stack(b.traj))
    assert a.step_totals["solved"].sum() > 0 and not hasattr(b, "drive_summary")


def test_report_cuts_a_run_at_the_robots_last_driven_row():
    from mpc_trajectory_generator_amd import report
    f = log_fleet("cfg4-ellipses-retire")
    o = oracle_for(f["cfg"])
    host = mirror_of(f, o)
    while not run_over(f, host):
        host.step(o.warm_solve(threads=16))
    runs, s = report.fleet_runs(host), f["cfg"].num_steps_taken
    T = np.stack(host.traj)
    for b, (xx, xy, uv, uomega, times) in enumerate(runs):
        n = host.steps if host.retired_at[b] < 0 else int(host.retired_at[b])
        assert len(xx) == len(xy) == n * s + 1 and len(uv) == len(uomega) == n * s and len(times) == n
        assert xx == T[:n * s + 1, b, 0].tolist() and uv == host.controls[:n * s, b, 0].tolist()
    assert min(len(r[4]) for r in runs) < host.steps
    text = report.fleet_runtime_text(host)
    assert "Solver calls" in text and "Converged" in text and "PANOC iterations" in text
    with pytest.raises(ValueError):
        report.fleet_runs(mirror_of(f, o, log=False))


def test_log_functions_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    lib = _lib.load_library()
    for name in ("nmpc_loop_set_log", "nmpc_loop_log", "nmpc_loop_drive_summary", "nmpc_loop_step_totals"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.nmpc_abi_version() == 3
    for struct, dtype, size in (("nmpc_step_record", _lib.STEP_RECORD_DTYPE, 40), ("nmpc_drive_summary", _lib.DRIVE_SUMMARY_DTYPE, 112),
                                ("nmpc_step_totals", _lib.STEP_TOTALS_DTYPE, 48)):
        m = re.search(r"typedef struct " + struct + r" \{[^\n]*\n(.*?)\n\} " + struct + ";", header, re.S)
        assert m, struct
        fields = []
        for line in m.group(1).split("\n"):
            decl = re.sub(r"/\*.*?\*/", "", line).strip().rstrip(";")
            fields += [re.sub(r"\[\d+\]", "", v).strip() for v in decl.split(None, 1)[1].split(",")]
        assert fields == list(dtype.names), (struct, fields)
        assert dtype.itemsize == size and f"sizeof({struct}) == {size}" in header
    assert lib.nmpc_loop_set_log(None) == -3 and lib.nmpc_loop_drive_summary(None, None) == -3
    assert lib.nmpc_loop_log(None, None, None, 0) == -3 and lib.nmpc_loop_step_totals(None, None, 0) == -3
