"""Receding-horizon drivers on top of the solver handle.

``RecedingHorizonRobot`` is the per-robot step of the reference's ``PathGenerator.run`` loop
(src/path_generator.py:290-403), written once and line for line: parameter assembly, control and Euler
advance (``_euler_advance``, src/mpc/mpc_generator.py:223-235), terminal test.  Two drivers run it, and the
goldens recorded from the reference's own loop pin it through both (tests/test_harness.py):

``TrajectoryGenerator.run`` follows ``PathGenerator.run`` (:197-437) call for call -- manager start /
ping, per-step parameters, ``mpc_step`` (= ``MpcModule.run``, src/mpc/mpc_generator.py:204-237), terminal
test, kill -- so a user of the reference finds the same control flow, with the OpEn TCP manager replaced
by ``tcp_shim.OptimizerTcpManager``.  The visibility-graph A* front-end (extremitypathfinder /
pyclipper) is outside this project's scope; a ``harness.Route`` (waypoints + NMPC vertices) is
what ``run`` starts from.

``BatchedRecedingHorizon`` is the batched counterpart for BASELINE config 4: B such robots advance in
lock step, one batched solve per step, controls and multipliers carried as warm starts.
``VectorizedRecedingHorizon`` is its NumPy mirror (bit-identical parameter vectors demanded): one step over flat per-robot arrays,
each robot's route looked up in a table, as the device loop has it.  ``FleetRecedingHorizon`` (host, that same step) and
``DeviceRecedingHorizon`` given a list of routes run a fleet whose robots follow routes of their own.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
import time

import numpy as np

from . import _lib, harness
from .config import Config
from .tcp_shim import OptimizerTcpManager


def _euler_advance(cfg: Config, u, take_steps, system_input, states):
    """Append the controls taken and the poses they lead to: src/mpc/mpc_generator.py:223-235."""
    system_input += [float(v) for v in u[:cfg.nu * take_steps]]              # :223
    for i in range(take_steps):                                              # :225-235, Euler diff-drive
        u_v, u_omega = u[i * cfg.nu], u[1 + i * cfg.nu]
        x, y, theta = states[-3], states[-2], states[-1]
        states += [x + cfg.ts * (u_v * math.cos(theta)), y + cfg.ts * (u_v * math.sin(theta)),
                   theta + cfg.ts * u_omega]


def mpc_step(cfg: Config, parameters, mng, take_steps, system_input, states):
    """One NMPC solve + state advance: src/mpc/mpc_generator.py:204-237."""
    solution = mng.call(parameters)                                          # :206
    if solution.is_ok():                                                     # :209-214
        data = solution.get()
        u, exit_status, solver_time = data.solution, data.exit_status, data.solve_time_ms
    else:                                                                    # :215-221
        err = solution.get()
        mng.kill()
        raise RuntimeError(f"MPC Solver error: {err.message}")
    _euler_advance(cfg, u, take_steps, system_input, states)
    return exit_status, solver_time


class RecedingHorizonRobot:
    """What the reference's loop keeps per robot (src/path_generator.py:262-280) and its three uses of it per
    step.  ``idx0`` = the reference sample the window search starts at (0 in the reference); the clock ``t``
    is advanced by the driver (:401)."""

    def __init__(self, route: harness.Route, start, dyn_obs_list, sinus_object=False, idx0=0):
        cfg = self.cfg = route.cfg
        self.route, self.dyn_obs_list, self.sinus_object = route, dyn_obs_list, sinus_object
        self.t, self.idx = 0, int(idx0)
        self.system_input = []                                               # :265
        self.states = list(map(float, start))                                # :267, flat [x, y, theta, ...]
        self.constraints = [0.0] * cfg.Nobs * cfg.nobs                       # :273
        self.dyn_constraints = harness.initial_dyn_constraints(cfg)          # :274-280

    def parameters(self):
        """The parameter list of this step: src/path_generator.py:293-379."""
        cfg, route, t = self.cfg, self.route, self.t
        x_init = self.states[-cfg.nx:]                                       # :293
        if len(route.vertices):                                              # :295-304
            self.constraints = harness.static_constraints(route, (x_init[0], x_init[1]))
        per, k = cfg.N_hor * cfg.ndynobs, cfg.ndynobs * cfg.num_steps_taken
        if t == 0:                                                           # :306-309
            for i, obs in enumerate(harness.dyn_obstacle_flat(cfg, self.dyn_obs_list, t * cfg.ts, cfg.N_hor,
                                                              self.sinus_object)):
                self.dyn_constraints[i * per:(i + 1) * per] = obs
        else:                                                                # :310-316 rotate the whole list left, refresh the tails
            self.dyn_constraints = self.dyn_constraints[k:] + self.dyn_constraints[:k]
            for i, obs in enumerate(harness.dyn_obstacle_flat(cfg, self.dyn_obs_list,
                                                              (t + cfg.N_hor - cfg.num_steps_taken) * cfg.ts,
                                                              cfg.num_steps_taken, self.sinus_object)):
                self.dyn_constraints[(i + 1) * per - k:(i + 1) * per] = obs
        lb_idx = max(0, self.idx - 1 * cfg.num_steps_taken)                  # :320-325
        ub_idx = min(len(route.x_ref), self.idx + 5 * cfg.num_steps_taken)
        self.idx = harness.closest_index((x_init[0], x_init[1]), route.ref_points[lb_idx:ub_idx]) + lb_idx
        last_u = self.system_input[-cfg.nu:] if len(self.system_input) else [0.0] * cfg.nu     # :371-374
        return harness.assemble_params(route, x_init, last_u, self.idx, self.constraints, self.dyn_constraints)

    def apply(self, u):
        _euler_advance(self.cfg, u, self.cfg.num_steps_taken, self.system_input, self.states)

    def terminal(self):
        return bool(np.allclose(self.states[-3:-1], self.route.end[0:2], atol=0.05, rtol=0)
                    and abs(self.system_input[-2]) < 0.005)                  # :397


class TrajectoryGenerator:
    """Counterpart of the reference's ``PathGenerator`` (plots and reports omitted)."""

    def __init__(self, config: Config, build: bool = False, verbose: bool = False, sinus_object: bool = False,
                 manager_factory=None):
        self.config, self.verbose, self.sinus_object = config, verbose, sinus_object
        self.time_dict, self.solver_times, self.overhead_times = {}, [], []
        self._factory = manager_factory or (lambda: OptimizerTcpManager(
            config.build_directory + "/" + config.optimizer_name, config=config))
        # build=True triggers OpEn code generation in the reference (:33-34); here the kernels are
        # compiled when the library is first loaded, nothing to do.

    def _result(self, robot):
        nx = self.config.nx
        return (robot.states[0::nx], robot.states[1::nx], robot.system_input[0::2], robot.system_input[1::2],
                self.solver_times, self.overhead_times)

    def run(self, route: harness.Route, max_steps: int | None = None, record_parameters: list | None = None):
        """-> (xx, xy, uv, uomega, solver_times, overhead_times), src/path_generator.py:197-437."""
        cfg = self.config
        t_temp = time.time()
        mng = self._factory()                                                 # :218-222
        mng.start()
        mng.ping()
        self.time_dict["opt_launch"] = int(1000 * (time.time() - t_temp))
        tt = time.time()
        terminal = False
        self.solver_times, self.overhead_times = [], []
        robot = RecedingHorizonRobot(route, route.start, route.dyn_obs_list, self.sinus_object)
        limit = 500.0 / cfg.ts if max_steps is None else max_steps
        t_temp = time.time()
        try:
            while (not terminal) and robot.t < limit:                             # :290
                t_overhead = time.time()
                parameters = robot.parameters()
                if record_parameters is not None:
                    record_parameters.append(list(parameters))
                try:                                                              # :384-391
                    exit_status, solver_time = mpc_step(cfg, parameters, mng, cfg.num_steps_taken, robot.system_input,
                                                        robot.states)
                    self.solver_times.append(solver_time)
                except RuntimeError as err:
                    if self.verbose:
                        print(err)
                    return None
                if exit_status in cfg.bad_exit_codes and self.verbose:            # :393-394
                    print(f"[MPC] Bad converge status: {exit_status}")
                terminal = robot.terminal()
                robot.t += cfg.num_steps_taken                                    # :401
                self.overhead_times.append((time.time() - t_overhead) * 1000.0 - solver_time)
        except KeyboardInterrupt:                                             # :405-415: kill the server, return what was driven so far
            if self.verbose:
                print("[MPC] killing TCP connection to MCP solver...")
            mng.kill()
            return self._result(robot)
        mng.kill()                                                            # :417
        self.time_dict["mpc_time"] = int(1000 * (time.time() - t_temp))
        self.time_dict["solver_time"] = sum(self.solver_times)
        self.time_dict["mean_solver_time"] = float(np.mean(self.solver_times)) if self.solver_times else 0.0
        self.time_dict["total_time"] = int(1000 * (time.time() - tt))
        return self._result(robot)


class _HostLoop:
    """What the host drivers share: one step = assemble -> ``solve_fn(P, u0, y0) -> (U, Y, status)`` -> advance.

    A driver that retires its robots (``FleetRecedingHorizon(retire=True)``) has ``active`` [B] bool: ``solve_fn`` then gets the
    active rows only, in ascending robot index, every other row of ``U``, ``Y`` and the status keeps what it held, and the step
    ends with ``retire()``; it returns the parameter vectors and statuses of all B robots, a retired one's from its last step."""
    active = None

    def step(self, solve_fn):
        P = self.assemble()
        if self.active is None:
            self.U, self.Y, st = solve_fn(P, self.U, self.Y)
            self._st_step = st                                               # this step's statuses: the drive log's
            self.advance(self.U)
            return P, st
        rows = np.nonzero(self.active)[0]
        if len(rows):
            U, Y, st = solve_fn(P[rows], self.U[rows], self.Y[rows])
            if self.status is None:
                self.status = np.zeros(len(self.active), dtype=st.dtype)
            self.U[rows], self.Y[rows], self.status[rows] = U, Y, st
        self._st_step = self.status
        self.advance(self.U)
        self.retire()
        return P, self.status


class BatchedRecedingHorizon(_HostLoop):
    """B robots on one route, advanced in lock step with one batched solve per step.

    Each robot is a ``RecedingHorizonRobot`` with its own dynamic obstacles (``dyn_obs_lists``, default the
    route's) and its own first reference sample (``idx0``, default 0 as the reference), so its parameter vector
    is filled as ``TrajectoryGenerator.run`` fills it.  ``solve_fn`` is the batched solver
    (``BatchSolver.solve``); controls and multipliers are carried over as warm starts, the penalty restarts at
    its initial value, like the sequential path.
    """

    def __init__(self, route: harness.Route, starts, dyn_obs_lists=None, sinus_object=False, idx0=None):
        self.route, self.cfg = route, route.cfg
        self.B = len(starts)
        self.robots = [RecedingHorizonRobot(route, s, route.dyn_obs_list if dyn_obs_lists is None else dyn_obs_lists[b],
                                            sinus_object, 0 if idx0 is None else idx0[b]) for b, s in enumerate(starts)]
        self.t = 0
        self.U = np.zeros((self.B, self.cfg.n_u))
        self.Y = np.zeros((self.B, self.cfg.n1))
        self.done = np.zeros(self.B, dtype=bool)

    # per robot: the flat pose list, the flat control list, the reference sample.  Tuples, so that an item
    # assignment fails instead of changing a temporary (the robots' own lists are the elements).
    states = property(lambda self: tuple(r.states for r in self.robots))
    inputs = property(lambda self: tuple(r.system_input for r in self.robots))
    idx = property(lambda self: tuple(r.idx for r in self.robots))

    def assemble(self):
        return np.array([r.parameters() for r in self.robots], dtype=np.float64).reshape(self.B, self.cfg.n_p)

    def advance(self, U):
        for b, r in enumerate(self.robots):
            r.apply(U[b])
            self.done[b] = r.terminal()
            r.t += self.cfg.num_steps_taken                                   # :401
        self.t += self.cfg.num_steps_taken


def _atan2(y, x):
    """``math.atan2`` element by element: the reference's, and the per-robot loop's (visibility.py:184).  ``np.arctan2`` is not
    libm's on every machine, and where it is not it differs from it in the last bits of some results."""
    return np.array([math.atan2(a, b) for a, b in zip(y.ravel(), x.ravel())], dtype=np.float64).reshape(y.shape)


def _predict_ellipses(cfg, sincos, obs, sinus, t0, horizon):
    """The closed-form obstacle predictor (visibility.py:156-166,199-216) for any number of obstacles at once: ``obs`` =
    ``(p1 [..., 2], p2 [..., 2], freq [...], rx [...], ry [...], angle [...])``, ``sinus`` [...] bool = who follows the sinusoidal law
    (:183-196, amplitude 1.5) -> [..., horizon, 5] = (x, y, rx + pad, ry + pad, angle) at ``linspace(t0, t0 + horizon ts, horizon)``."""
    p1, p2, freq, rx, ry, ang = obs
    times = np.linspace(t0, t0 + horizon * cfg.ts, horizon)                       # (:204)
    s = np.abs(sincos(freq[..., None] * times)[0])                                 # [..., H]
    pos = s[..., None] * p1[..., None, :] + (1 - s[..., None]) * p2[..., None, :]
    if sinus.any():
        a, b, f, at = p1[sinus], p2[sinus], freq[sinus], pos[sinus]                # [n, 2], [n, 2], [n], [n, H, 2]
        ang_d = _atan2(b[:, 1] - a[:, 1], b[:, 0] - a[:, 0])[:, None]              # [n, 1]
        add = 1.5 * sincos((10 * f[:, None]) * times[None, :])[1]                  # [n, H]
        sa, ca = sincos(ang_d)
        dx, dy = at[:, :, 0] - a[:, None, 0], at[:, :, 1] - a[:, None, 1]
        ex = ca * dx - sa * dy
        ey = sa * dx + ca * dy
        ey = ey + add
        sm, cm = sincos(-ang_d)
        qx = cm * (ex - 0.0) - sm * (ey - 0.0)
        qy = sm * (ex - 0.0) + cm * (ey - 0.0)
        at[:, :, 0] = qx + a[:, None, 0]
        at[:, :, 1] = qy + a[:, None, 1]
        pos[sinus] = at
    pad = cfg.vehicle_width / 2 + cfg.vehicle_margin
    out = np.empty(pos.shape[:-1] + (5,))
    out[..., 0:2] = pos
    out[..., 2] = (rx + pad)[..., None]
    out[..., 3] = (ry + pad)[..., None]
    out[..., 4] = ang[..., None]
    return out


class _RouteTable:
    """What a step reads of R routes, side by side (the device's ``LoopRoute`` table, csrc/nmpc_loop_host.h): row r = route r, padded to
    the longest route's, with each route's own lengths ``n``, ``nv``, ``nb`` [R]; ``end`` [R, 3], ``base`` (speed) and ``radius`` [R].
    ``ref`` [R * width, 3] = the reference samples (x, y, theta), ``width`` rows per route; row ``n`` of a route, one past its last
    sample, is its goal pose: what a horizon reads beyond the route.  ``bv`` goes on with N_hor zeros past the longest braking table:
    what a horizon reads beyond a table.  ``head`` [R, Nobs, nobs] = the circles a route of no more than Nobs vertices always shows."""

    def __init__(self, routes, cfg):
        def pad(rows, fill=0.0, more=0, tail=()):
            """-> (the rows side by side, ``more`` entries longer than the longest, ``fill`` past a row's own; the lengths [R])"""
            rows = [np.array(v, dtype=np.float64).reshape((-1,) + tail) for v in rows]
            out = np.empty((len(rows), max(len(v) for v in rows) + more) + tail)
            out[:] = fill
            for r, v in enumerate(rows):
                out[r, :len(v)] = v
            return out, np.array([len(v) for v in rows], dtype=np.int64)
        self.end = np.array([r.end for r in routes], dtype=np.float64).reshape(-1, 3)
        ref, self.n = pad([np.stack([r.x_ref, r.y_ref, r.theta_ref], axis=1) for r in routes], self.end[:, None, :], 1, (3,))
        self.ref, self.width = ref.reshape(-1, 3), ref.shape[1]
        self.vert, self.nv = pad([r.vertices for r in routes], tail=(2,))
        self.bv, self.nb = pad([r.brake_velocities for r in routes], more=cfg.N_hor)
        self.bd = pad([r.brake_distances for r in routes])[0]
        self.base = np.array([r.base_speed for r in routes], dtype=np.float64)
        self.radius = np.array([r.radius for r in routes], dtype=np.float64)
        self.head = np.zeros((len(routes), cfg.Nobs, cfg.nobs))
        for r, m in enumerate(np.minimum(self.nv, cfg.Nobs)):
            self.head[r, :m, 0:2], self.head[r, :m, 2] = self.vert[r, :m], self.radius[r]


class VectorizedRecedingHorizon(_HostLoop):
    """``BatchedRecedingHorizon`` with the per-robot Python loops replaced by NumPy array operations
    (BASELINE config 4: 8192 robots x 100 steps).  Same quantities, same order of operations per
    robot -- the test suite demands bit-identical parameter vectors against the loop version.

    Everything is kept per robot in flat [B] arrays, as the device loop keeps it, and a robot's route is looked up through
    ``route_of[b]`` in a ``_RouteTable``: here all robots share the one route (``route_of`` = 0), ``FleetRecedingHorizon`` is the
    same step on many.  Dynamic obstacles are per robot: ``dyn_obs`` is ``None`` or a tuple of
    arrays ``(p1 [B, K, 2], p2 [B, K, 2], freq [B, K], rx [B, K], ry [B, K], angle [B, K])``; ``idx0`` = the
    reference sample each robot starts its window search at (default 0, as the reference).
    """

    def __init__(self, route: harness.Route, starts, dyn_obs=None, sincos=None, sinus_object=False, idx0=None):
        self.route = route
        self._init_robots([route], np.zeros(len(starts), dtype=np.int64), starts, dyn_obs, sincos, sinus_object, idx0)

    def _init_robots(self, routes, route_of, starts, dyn_obs, sincos, sinus_object, idx0):
        cfg = self.cfg = routes[0].cfg
        self.tab, self.route_of = _RouteTable(routes, cfg), route_of
        self.sinus_object = bool(sinus_object)     # obstacle index 2 follows the sinusoidal law (visibility.py:183-196,210-212)
        # sin / cos used by the state advance and the obstacle predictor: libm's (as the reference) unless
        # a replacement is given -- the device loop's bit-level mirror passes the kernels' own sin / cos
        self.sincos = sincos if sincos is not None else (lambda x: (np.sin(x), np.cos(x)))
        self.B = B = len(starts)
        self.state = np.array(starts, dtype=np.float64).reshape(B, 3)
        self.traj = [self.state.copy()]
        self.last_u = np.zeros((B, cfg.nu))
        self.idx = np.zeros(B, dtype=np.int64) if idx0 is None else np.array(idx0, dtype=np.int64).reshape(B)
        self.t = 0
        self.dyn_obs = dyn_obs
        K = 0 if dyn_obs is None else dyn_obs[0].shape[1]
        assert K <= cfg.Ndynobs
        self.K = K
        d = np.zeros((B, cfg.Ndynobs, cfg.N_hor, cfg.ndynobs))
        d[..., 2] = 1.0
        d[..., 3] = 1.0                                           # padding: unit radii (path_generator.py:274-280)
        self.dyn = d
        self.U = np.zeros((B, cfg.n_u))
        self.Y = np.zeros((B, cfg.n1))
        self.done = np.zeros(B, dtype=bool)

    # dynamic-obstacle prediction for all robots: visibility.py:156-166,199-216 (linear law)
    def _predict(self, t0, horizon):
        sinus = np.zeros(self.dyn_obs[2].shape, dtype=bool)
        if self.sinus_object and sinus.shape[1] > 2:
            sinus[:, 2] = True
        return _predict_ellipses(self.cfg, self.sincos, self.dyn_obs, sinus, t0, horizon)

    def assemble(self, active=None):
        """-> P [B, n_p].  ``active`` [B] bool (default: everybody): the other robots keep everything they carry (reference sample,
        dynamic block), and their rows of P mean nothing."""
        cfg, T, rt, B, N = self.cfg, self.tab, self.route_of, self.B, self.cfg.N_hor
        s = cfg.num_steps_taken
        n, at = T.n[rt], rt * T.width                            # each robot's route: its samples, its first row of T.ref
        x, y = self.state[:, 0], self.state[:, 1]
        # static circles (path_generator.py:295-304 + visibility.py:141-148 with look-back 0): the route's first Nobs vertices; on a
        # route with more, those from the closest one on, up to slot Nobs
        cons = T.head[rt]
        more = np.nonzero(T.nv[rt] > cfg.Nobs)[0]
        if len(more):
            r, nv = rt[more, None], T.nv[rt[more], None]
            dist = np.linalg.norm(T.vert[rt[more]] - self.state[more, None, 0:2], axis=2)
            lb = np.argmin(np.where(np.arange(T.vert.shape[1])[None, :] < nv, dist, np.inf), axis=1)     # not the padding
            j = lb[:, None] + np.arange(cfg.Nobs)[None, :]
            ok = j < cfg.Nobs
            jj = np.minimum(j, nv - 1)
            cons[more, :, 0:2] = np.where(ok[..., None], T.vert[r, jj], 0.0)
            cons[more, :, 2] = np.where(ok, T.radius[r], 0.0)
        # dynamic ellipses (path_generator.py:306-316)
        if self.K:
            if self.t == 0:
                self.dyn[:, :self.K] = self._predict(0.0, N)
            else:
                # the reference rotates the WHOLE flat list left by ndynobs * s entries (:312): inside a block that is a
                # shift by s stages, and a block's last s stages take the next block's first s (the last block's take
                # block 0's -- a padding slot can so inherit stale ellipses of obstacle 0 when 0 < K < Ndynobs)
                flat, held = self.dyn.reshape(B, -1), self.dyn
                self.dyn = np.roll(flat, -cfg.ndynobs * s, axis=1).reshape(self.dyn.shape)
                self.dyn[:, :self.K, N - s:] = self._predict((self.t + N - s) * cfg.ts, s)
                if active is not None:
                    self.dyn[~active] = held[~active]
        # closest reference sample in the sliding window (:320-325)
        lb = np.maximum(0, self.idx - s)
        ub = np.minimum(n, self.idx + 5 * s)
        w = np.arange(6 * s)
        j = lb[:, None] + w[None, :]
        ok = j < ub[:, None]
        p = T.ref.take(at[:, None] + np.minimum(j, n[:, None] - 1), axis=0)
        d = np.linalg.norm(np.stack([p[..., 0] - x[:, None], p[..., 1] - y[:, None]], axis=2), axis=2)
        d = np.where(ok, d, np.inf)
        self.idx = lb + np.argmin(d, axis=1) if active is None else np.where(active, lb + np.argmin(d, axis=1), self.idx)
        idx = self.idx
        # horizon references and target (:326-341): beyond the route's last sample its goal pose, the table's entry n
        refs = T.ref.take(np.minimum((at + idx)[:, None] + np.arange(N)[None, :], (at + n)[:, None]), axis=0)
        xf = T.ref.take(np.minimum(at + idx + N, at + n), axis=0)
        # velocity reference with the braking profile (:343-361)
        base = T.base[rt, None]
        brake = (idx + N) >= n - T.bd[rt, 0] / T.base[rt]
        num_base = np.minimum(n - idx - 1, N)
        k = np.arange(N)[None, :]
        nb = num_base[:, None]
        tail = T.bv.reshape(-1).take((rt * T.bv.shape[1])[:, None] + np.clip(k - nb, 0, T.bv.shape[1] - 1))     # zeros beyond a route's own
        vel_b = np.where(k < nb, base, tail)
        vel = np.where(brake[:, None], vel_b, base)
        for b in np.where(brake & (num_base == 0))[0]:                      # inside the last sample: distance-based (:347-351)
            r = rt[b]
            dist_to_goal = math.sqrt((self.state[b, 0] - T.end[r, 0]) ** 2 + (self.state[b, 1] - T.end[r, 1]) ** 2)
            vr = [v for (v, dd) in zip(T.bv[r, :T.nb[r]], T.bd[r, :T.nb[r]]) if dd <= dist_to_goal][:N]
            vel[b] = np.array(vr + [0.0] * (N - len(vr)))
        W = np.tile(np.array(cfg.weights()), (B, 1))
        P = np.concatenate([self.state, self.last_u, xf, self.last_u, W, vel, cons.reshape(B, -1),
                            self.dyn.reshape(B, -1), refs.reshape(B, -1)], axis=1)
        assert P.shape[1] == cfg.n_p
        return P

    def advance(self, U, active=None):
        """``active`` as in ``assemble``: the other robots stay where they are (their trajectory rows repeat their pose) and keep
        their ``last_u`` and ``done``."""
        cfg = self.cfg
        s = cfg.num_steps_taken
        st = self.state.copy()
        for i in range(s):                                                  # mpc_generator.py:225-235
            v, w = U[:, i * cfg.nu], U[:, 1 + i * cfg.nu]
            th = st[:, 2]
            # per robot: x + ts*(v*cos(theta)) with math.cos -> np.cos is the same libm call
            sn, cs = self.sincos(np.ascontiguousarray(th))
            new = np.stack([st[:, 0] + cfg.ts * (v * cs), st[:, 1] + cfg.ts * (v * sn),
                            th + cfg.ts * w], axis=1)
            st = new if active is None else np.where(active[:, None], new, st)
            self.traj.append(st.copy())
        self.state = st
        last_u = U[:, (s - 1) * cfg.nu:s * cfg.nu].copy()
        self.last_u = last_u if active is None else np.where(active[:, None], last_u, self.last_u)
        end = self.tab.end[self.route_of]
        done = (np.abs(st[:, 0] - end[:, 0]) <= 0.05) & (np.abs(st[:, 1] - end[:, 1]) <= 0.05) & (np.abs(self.last_u[:, 0]) < 0.005)
        self.done = done if active is None else np.where(active, done, self.done)
        self.t += s


def _checked_groups(who, group_of, B):
    """-> ``group_of`` [B] as an int32 array with values in [0, B), or None (one group); ValueError otherwise."""
    if group_of is None:
        return None
    g = np.ascontiguousarray(group_of, dtype=np.int32).reshape(B)
    if ((g < 0) | (g >= B)).any():
        raise ValueError(f"{who}: group_of out of range")
    return g


@dataclasses.dataclass(frozen=True)
class Peers:
    """How the robots of a fleet see each other, for ``FleetRecedingHorizon`` and
    ``DeviceRecedingHorizon`` alike: every step, the ``slots`` robots of a robot's group whose predicted
    positions come closest to its own, closer than ``range``, take ellipse slots K .. K + slots - 1 of its
    parameter vector (K = its scripted obstacles) as ellipses of radii ``rx``, ``ry`` -- the radii the cost
    reads, nothing is added to them -- at their predicted poses.  ``group_of`` [B] = the group of each robot,
    values in [0, B) (``None``: one group); robots of different groups never see each other.

    ``cell`` (metres; ``None``: all pairs of a group) finds the same peers through a grid (``peer_grid``,
    ``nmpc_loop_set_peers_grid``): a robot forms its distances to the robots filed near it only, which is what lets a whole
    fleet be one group.  No result depends on it."""
    slots: int
    rx: float
    ry: float
    range: float
    group_of: object = None
    cell: float = None

    def checked(self, B: int, K: int, Ndynobs: int):
        """-> group_of as an int32 array or None; ValueError for what ``nmpc_loop_set_peers`` / ``nmpc_loop_set_peers_grid`` refuses."""
        if self.slots < 1 or K + self.slots > Ndynobs:
            raise ValueError(f"peers: slots = {self.slots} with {K} scripted obstacles and Ndynobs = {Ndynobs}")
        for v in (self.rx, self.ry, self.range):
            if not (math.isfinite(v) and v > 0):
                raise ValueError("peers: rx, ry and range must be finite and positive")
        if self.cell is not None and not (math.isfinite(self.cell) and self.cell > 0):
            raise ValueError("peers: cell must be finite and positive")
        return _checked_groups("peers", self.group_of, B)


CROWD_MAX = 16384            # D of a crowd at the most (nmpc_loop_set_crowd)
CROWD_GRID_MAX = 131072      # ... with a ``cell`` (nmpc_loop_set_crowd_grid)
CROWD_GRID_CAP = 128         # cells per axis at the most (csrc/nmpc_loop.h)


@dataclasses.dataclass(frozen=True)
class Crowd:
    """D moving obstacles that belong to the world and are shared by the whole fleet, for
    ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: one table of every obstacle's ellipses over the horizon is advanced
    once per step, and every step the ``slots`` obstacles that come closest to a robot's predicted positions, closer than ``range``,
    take ellipse slots K .. K + slots - 1 of its parameter vector (K = its scripted obstacles; peers follow from K + slots on).
    ``obstacles`` = ``(p1 [D, 2], p2 [D, 2], freq [D], rx [D], ry [D], angle [D])`` as one robot's ``dyn_obs``; ``sinus`` [D] bool =
    who follows the sinusoidal law (``None``: nobody).  The values are not checked: an obstacle with a NaN is never chosen.
    ``watch=True`` (the device needs ``max_steps`` > 0): ``crowd_clearance`` [B] keeps every robot's closest approach to ANY obstacle
    of the crowd, chosen or not (a ``_lib.CROWD_CLEARANCE_DTYPE`` array).  It observes only.

    ``cell`` (metres; ``None``: every obstacle against every robot, 16384 obstacles at the most) finds the same obstacles through a
    grid in space and stage (``crowd_grid``, ``nmpc_loop_set_crowd_grid``): up to 131072 obstacles, at a cost that grows with what is
    near a robot, not with the world.  No result depends on it; ``crowd_looked`` [B] counts the table's entries each robot looked at
    at its last step (all obstacles: D * N).  The observer stays all obstacles."""
    obstacles: object
    slots: int
    range: float
    sinus: object = None
    watch: bool = False
    cell: float = None

    def checked(self, B: int, K: int, Ndynobs: int, Mp: int = 0):
        """-> (obstacles as six contiguous float64 arrays, sinus [D] bool); ValueError for what ``nmpc_loop_set_crowd`` refuses
        (``Mp``: the slots of the loop's peers)."""
        if len(self.obstacles) != 6:
            raise ValueError("crowd: obstacles = (p1, p2, freq, rx, ry, angle)")
        p1, p2, freq, rx, ry, ang = (np.ascontiguousarray(a, dtype=np.float64) for a in self.obstacles)
        D = len(freq)
        most = CROWD_MAX if self.cell is None else CROWD_GRID_MAX
        if D < 1 or D > most:
            raise ValueError(f"crowd: {D} obstacles, 1 to {most} are taken")
        if self.cell is not None and not (math.isfinite(self.cell) and self.cell > 0):
            raise ValueError("crowd: cell must be finite and positive")
        if p1.shape != (D, 2) or p2.shape != (D, 2) or any(a.shape != (D,) for a in (freq, rx, ry, ang)):
            raise ValueError("crowd: obstacles of shapes other than [D, 2], [D, 2], [D], [D], [D], [D]")
        if self.slots < 1 or K + self.slots + Mp > Ndynobs:
            raise ValueError(f"crowd: slots = {self.slots} with {K} scripted obstacles, {Mp} peer slots and Ndynobs = {Ndynobs}")
        if not (math.isfinite(self.range) and self.range > 0):
            raise ValueError("crowd: range must be finite and positive")
        sinus = np.zeros(D, dtype=bool) if self.sinus is None else np.ascontiguousarray(self.sinus, dtype=bool)
        if sinus.shape != (D,):
            raise ValueError("crowd: sinus of a shape other than [D]")
        return (p1, p2, freq, rx, ry, ang), sinus


WALLS_MAX_EDGES = 1024       # E of a loop's walls at the most (nmpc_loop_set_walls)
WALL_GRID_MAX_EDGES = 1 << 20        # ... with a ``cell`` (nmpc_loop_set_walls_grid)
WALL_GRID_MAX_ENTRIES = 1 << 23      # filings of all edges at the most
WALL_GRID_CAP = 512                  # cells per axis at the most (csrc/nmpc_loop.h)


# ---- the loop's geometry (csrc/nmpc_geom.h): unfused f64, the same operations in the same order as the header's functions ----
def segment_closest(x, y, x1, y1, x2, y2, clamp_below=True):
    """The points of the segments (x1, y1) -> (x2, y2) closest to the positions (x, y), all broadcast against each other -> (v, cx, cy):
    the squared distance and the point (segment_closest of csrc/nmpc_geom.h).  A segment without length is its first end; a NaN clamps
    nothing.  ``clamp_below`` (a flag, or an array of them) False lets a segment run on backwards beyond its first end."""
    with np.errstate(all="ignore"):
        ex, ey = x2 - x1, y2 - y1
        L2 = ex * ex + ey * ey
        pos = L2 > 0
        t = ((x - x1) * ex + (y - y1) * ey) / np.where(pos, L2, 1.0)
        t = np.where((t < 0) & clamp_below, 0.0, t)
        t = np.where(t > 1, 1.0, t)
        t = np.where(pos, t, 0.0)
        cx, cy = x1 + t * ex, y1 + t * ey
        dx, dy = x - cx, y - cy
        return dx * dx + dy * dy, cx, cy


def grid_cellof(v, o, h, n):
    """The cells (int64) of the coordinates ``v`` on an axis of ``n`` cells of edge ``h`` from ``o``: monotone non-decreasing in ``v``,
    clamped before the conversion (cellof of csrc/nmpc_geom.h).  Filing and looking up, in both grids, use this one function."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(v, dtype=np.float64) - o) / h
    t = np.where(t > 0.0, t, 0.0)                                           # (a NaN goes to 0)
    return np.where(t >= float(n), n - 1, np.minimum(t, float(n)).astype(np.int64)).astype(np.int64)


def grid_axis(extent, cell, cap):
    """An axis of a grid -> (n, h): floor(extent / cell) + 1 cells of edge ``cell``, or ``cap`` cells of edge extent / ``cap`` where that
    would be more (grid_axis of csrc/nmpc_geom.h)."""
    with np.errstate(all="ignore"):
        q = np.float64(extent) / np.float64(cell)
        return (int(q) + 1, np.float64(cell)) if q < float(cap) else (cap, np.float64(extent) / float(cap))


class _Grid:
    """What ``WallGrid``, ``PeerGrid`` and ``CrowdGrid`` share: ``origin`` [2], ``h`` [2], ``nx``, ``ny`` and the cell of a coordinate."""

    def _cellof(self, v, axis):
        """The cell of coordinate ``v`` on ``axis`` (``grid_cellof``)."""
        return int(grid_cellof(v, self.origin[axis], self.h[axis], (self.nx, self.ny)[axis]))


@dataclasses.dataclass(frozen=True)
class Walls:
    """How the robots of a loop see the map's walls, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon``
    alike: every step, each active robot's closest points on the wall segments ``edges`` [E, 4] = (x1, y1, x2, y2), measured against its
    predicted positions, closer than ``range`` and, among themselves, no closer than ``spacing``, take the LAST ``slots`` static-circle
    slots of its parameter vector as circles of ``radius``.  No polygon structure is needed (``frontend.map_edges(...)[0]`` gives a
    scene's edges, ``workloads.subdivided_map`` a finer cut).  Every route of the loop must leave the slots free: n_vert + slots <=
    Nobs.  ``wall_edge`` and ``wall_stage`` [B, slots] name the edge in each slot and the stage at which it came closest (-1: none).

    ``cell`` (metres; ``None``: every edge against every robot, 1024 edges at the most) finds the edges a robot measures through a
    static grid (``wall_grid``, ``nmpc_loop_set_walls_grid``): up to 1048576 edges, at a cost that grows with what is near a robot, not
    with the map.  No result depends on it; ``wall_looked`` [B] counts the distinct edges each robot measured at its last step."""
    edges: object
    slots: int
    radius: float
    range: float
    spacing: float = 0.0
    cell: float = None

    def checked(self, cfg, routes):
        """-> edges [E, 4] float64, contiguous; ValueError for what ``nmpc_loop_set_walls`` refuses (``routes``: every route of the
        loop, a mission's later legs included)."""
        edges = np.ascontiguousarray(self.edges, dtype=np.float64)
        if edges.ndim != 2 or edges.shape[1] != 4:
            raise ValueError(f"walls: edges of shape {edges.shape}, not [E, 4]")
        E = len(edges)
        most = WALLS_MAX_EDGES if self.cell is None else WALL_GRID_MAX_EDGES
        if E < 1 or E > most:
            raise ValueError(f"walls: {E} edges, 1 to {most} are taken")
        if self.cell is not None and not (math.isfinite(self.cell) and self.cell > 0):
            raise ValueError("walls: cell must be finite and positive")
        if not np.isfinite(edges).all():
            raise ValueError("walls: a coordinate that is not finite")
        if self.slots < 1 or self.slots > cfg.Nobs:
            raise ValueError(f"walls: slots = {self.slots} with Nobs = {cfg.Nobs}")
        for i, r in enumerate(routes):
            if len(r.vertices) + self.slots > cfg.Nobs:
                raise ValueError(f"walls: route {i} has {len(r.vertices)} vertices, slots = {self.slots} and Nobs = {cfg.Nobs}: no free circle slot")
        for v in (self.radius, self.range):
            if not (math.isfinite(v) and v > 0):
                raise ValueError("walls: radius and range must be finite and positive")
        if not (math.isfinite(self.spacing) and self.spacing >= 0):
            raise ValueError("walls: spacing must be finite and not negative")
        return edges


class WallGrid(_Grid):
    """The static grid of a map's wall segments (``wall_grid``): ``origin`` [2], ``h`` [2] the cells' edges, ``nx``, ``ny``, ``entries``
    (what ``nmpc_loop_wall_grid`` returns as its header), the CSR arrays ``cell_off`` [nx * ny + 1] and ``cell_edge`` [entries] int32
    (cells row-major, y * nx + x; edge indices ascending inside a cell), every edge's rectangle of cells ``rect`` [E, 4] = (first column,
    last column, first row, last row), ``window(pred_b, range)`` and ``looks_at(pred_b, range)``."""

    def header(self):
        """-> the header as one ``_lib.WALL_GRID_DTYPE`` record, as the device reports it."""
        rec = np.zeros((), dtype=_lib.WALL_GRID_DTYPE)
        rec["origin"], rec["h"] = self.origin, self.h
        rec["nx"], rec["ny"], rec["entries"] = self.nx, self.ny, self.entries
        return rec

    def window(self, pred_b, range):
        """-> (cx0, cx1, cy0, cy1), inclusive: the cells a robot with the predicted positions ``pred_b`` [N, >= 2] looks at; None for
        a robot without a stage at which both coordinates are finite."""
        xy = np.asarray(pred_b, dtype=np.float64)[:, :2]
        xy = xy[np.isfinite(xy).all(axis=1)]
        if not len(xy):
            return None
        lo, hi, r, tm = xy.min(axis=0), xy.max(axis=0), np.float64(range), np.float64(2.0 ** -40)
        slack = tm * (r + self.amax) + np.float64(2.0 ** -500)
        with np.errstate(over="ignore"):
            a = [(lo[ax] - r) - (slack + tm * abs(lo[ax])) for ax in (0, 1)]
            z = [(hi[ax] + r) + (slack + tm * abs(hi[ax])) for ax in (0, 1)]
        return self._cellof(a[0], 0), self._cellof(z[0], 0), self._cellof(a[1], 1), self._cellof(z[1], 1)

    def looks_at(self, pred_b, range):
        """-> the distinct edges filed in the cells of the robot's window, ascending (none for a robot without a window)."""
        w = self.window(pred_b, range)
        if w is None:
            return np.zeros(0, dtype=np.int32)
        cx0, cx1, cy0, cy1 = w
        r = self.rect
        return np.nonzero((r[:, 0] <= cx1) & (r[:, 1] >= cx0) & (r[:, 2] <= cy1) & (r[:, 3] >= cy0))[0].astype(np.int32)


def wall_grid(edges, cell):
    """The static grid of the walls rule with a ``cell`` over ``edges`` [E, 4], in the setter's arithmetic: -> a
    ``WallGrid``.

    ``origin`` is the minimum over all end points per axis; an axis has floor(extent / cell) + 1 cells of edge ``cell``, or
    ``WALL_GRID_CAP`` cells of edge extent / ``WALL_GRID_CAP`` where that would be more.  Edge e is filed in every cell of the rectangle
    cellof(min(x1, x2)) .. cellof(max(x1, x2)) x cellof(min(y1, y2)) .. cellof(max(y1, y2)).  A robot looks at the cells from that of
    ``(lo - range) - m(lo)`` to that of ``(hi + range) + m(hi)`` per axis, lo and hi the extremes of its finite predicted positions and
    m(v) = slack + 2^-40 |v|, slack = 2^-40 (range + the largest |coordinate| of an edge) + 2^-500: every edge with D < range^2 is filed
    there.  ValueError if the filings exceed ``WALL_GRID_MAX_ENTRIES``."""
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    E = len(edges)
    g = WallGrid()
    g.cell = float(cell)
    xs, ys = edges[:, [0, 2]], edges[:, [1, 3]]
    g.origin = np.array([xs.min(), ys.min()])
    g.amax = np.float64(np.abs(edges).max())
    with np.errstate(over="ignore"):
        ext = np.array([xs.max(), ys.max()]) - g.origin
    (g.nx, hx), (g.ny, hy) = (grid_axis(ext[ax], g.cell, WALL_GRID_CAP) for ax in (0, 1))
    g.h = np.array([hx, hy])

    def cells(v, ax):
        return grid_cellof(v, g.origin[ax], g.h[ax], (g.nx, g.ny)[ax])
    g.rect = np.stack([cells(xs.min(axis=1), 0), cells(xs.max(axis=1), 0), cells(ys.min(axis=1), 1), cells(ys.max(axis=1), 1)], axis=1)
    w, hgt = g.rect[:, 1] - g.rect[:, 0] + 1, g.rect[:, 3] - g.rect[:, 2] + 1
    g.entries = int((w * hgt).sum())
    if g.entries > WALL_GRID_MAX_ENTRIES:
        raise ValueError(f"walls: the edges are filed in {g.entries} cells in all, more than {WALL_GRID_MAX_ENTRIES}: use a larger cell or shorter edges")
    # every filing (e, cell), edge after edge; a stable sort by cell keeps the edges ascending inside a cell
    e_of = np.repeat(np.arange(E, dtype=np.int64), w * hgt)
    k = np.arange(g.entries, dtype=np.int64) - np.repeat(np.cumsum(w * hgt) - w * hgt, w * hgt)      # the filing's number inside its edge
    we = w[e_of]
    c_of = (g.rect[e_of, 2] + k // we) * g.nx + g.rect[e_of, 0] + k % we
    order = np.argsort(c_of, kind="stable")
    g.cell_edge = e_of[order].astype(np.int32)
    g.cell_off = np.concatenate([[0], np.cumsum(np.bincount(c_of, minlength=g.nx * g.ny))]).astype(np.int32)
    return g


PEER_GRID_CAP = 128          # cells per axis at the most (csrc/nmpc_loop.h)


class PeerGrid(_Grid):
    """The grid of one step (``peer_grid``): ``origin`` [2], ``h`` [2] the cells' edges, ``W`` [2] the largest box extent, ``nx``,
    ``ny``, ``filed`` (what ``nmpc_loop_peer_grid`` returns as its header), ``cell_of`` [B] int32 (row-major, y * nx + x; -1 =
    unfiled), the boxes ``lo``, ``hi`` [B, 2] and ``candidates(b)``."""

    def header(self):
        """-> the header as one ``_lib.PEER_GRID_DTYPE`` record, as the device reports it."""
        rec = np.zeros((), dtype=_lib.PEER_GRID_DTYPE)
        rec["origin"], rec["h"], rec["W"] = self.origin, self.h, self.W
        rec["nx"], rec["ny"], rec["filed"] = self.nx, self.ny, self.filed
        return rec

    def window(self, b):
        """-> (cx0, cx1, cy0, cy1), inclusive: the cells robot b looks at; None for an unfiled robot."""
        if self.cell_of[b] < 0:
            return None
        lo, hi, r = self.lo[b], self.hi[b], np.float64(self.range)
        with np.errstate(invalid="ignore", over="ignore"):
            return (self._cellof((lo[0] - r) - self.W[0], 0), self._cellof(hi[0] + r, 0),
                    self._cellof((lo[1] - r) - self.W[1], 1), self._cellof(hi[1] + r, 1))

    def row_ranges(self, b):
        """-> [(i0, i1)] per row of b's window: the row's cells are ``cell_mem[i0:i1]``."""
        w = self.window(b)
        if w is None:
            return []
        cx0, cx1, cy0, cy1 = w
        return [(int(self.cell_off[row * self.nx + cx0]), int(self.cell_off[row * self.nx + cx1 + 1])) for row in range(cy0, cy1 + 1)]

    def candidates(self, b):
        """-> the robots filed in the cells of b's window (b itself among them), row after row, ascending inside a cell."""
        rr = self.row_ranges(b)
        return np.concatenate([self.cell_mem[i0:i1] for i0, i1 in rr]) if rr else np.zeros(0, dtype=np.int64)


def peer_grid(pred, range, cell):
    """The broad phase of the peers rule for the predictions ``pred`` [B, N, >= 2] of one step, in the device's
    arithmetic (unfused f64, the same operations in the same order): -> a ``PeerGrid``.

    A robot's box is the minimum and maximum of its positions over the stages at which both coordinates are finite; a robot without
    such a stage is unfiled.  The grid starts at the minimum of the filed boxes' lower corners and has cells of edge ``cell``, or
    ``PEER_GRID_CAP`` cells of edge extent / ``PEER_GRID_CAP`` on an axis that would need more; a robot is filed under the cell of its
    box's lower corner.  Robot b looks at the cells from that of ``(lo_b - range) - W`` to that of ``hi_b + range``, ``W`` the largest
    box extent (rounded up): every j with D(b, j) < range^2 is filed there."""
    pred = np.asarray(pred, dtype=np.float64)
    B = pred.shape[0]
    g = PeerGrid()
    g.range, g.cell = float(range), float(cell)
    xy = pred[:, :, :2]
    ok = np.isfinite(xy).all(axis=2)                                        # [B, N]: the stages that count
    g.lo = np.where(ok[..., None], xy, np.inf).min(axis=1)
    g.hi = np.where(ok[..., None], xy, -np.inf).max(axis=1)
    filed = ok.any(axis=1)
    g.filed = int(filed.sum())
    g.nx = g.ny = 1
    g.h = np.array([g.cell, g.cell])
    g.origin, g.W = np.zeros(2), np.zeros(2)
    g.cell_of = np.full(B, -1, dtype=np.int32)
    if g.filed:
        lo, hi = g.lo[filed], g.hi[filed]
        with np.errstate(over="ignore"):
            w = hi - lo
            ex = lo.max(axis=0) - lo.min(axis=0)
        up = (w.view(np.int64) + 1).view(np.float64)                       # the next double above: never below the real hi - lo
        g.W = np.where(w < np.inf, up, w).max(axis=0)
        g.origin = lo.min(axis=0)
        (g.nx, hx), (g.ny, hy) = (grid_axis(ex[ax], g.cell, PEER_GRID_CAP) for ax in (0, 1))
        g.h = np.array([hx, hy])
        for b in np.nonzero(filed)[0]:
            g.cell_of[b] = g._cellof(g.lo[b, 1], 1) * g.nx + g._cellof(g.lo[b, 0], 0)
    cells = g.nx * g.ny
    who = np.nonzero(filed)[0]
    order = who[np.argsort(g.cell_of[who], kind="stable")]                  # ascending robot index inside a cell
    g.cell_mem = order.astype(np.int64)
    g.cell_off = np.concatenate([[0], np.cumsum(np.bincount(g.cell_of[who], minlength=cells))]).astype(np.int64)
    return g


class CrowdGrid(_Grid):
    """The crowd's grid in space and stage (``crowd_grid``): ``origin`` [2], ``h`` [2] the cells' edges, ``nx``, ``ny``, ``layers`` (N)
    and ``filed`` (what ``nmpc_loop_crowd_grid`` returns as its header), fixed by the obstacles' end points; ``file(table)`` files one
    step's table: ``cell_of`` [D, N] int32 (layer * nx * ny + y * nx + x; -1 = unfiled), ``cell_off`` [layers * nx * ny + 1] and
    ``cell_mem`` [filed] (the obstacle of each filed entry, ascending inside a cell); ``window(x, y, range)``,
    ``candidates(pred_b, range)`` and ``looked(pred_b, range)``."""

    def header(self):
        """-> the header as one ``_lib.CROWD_GRID_DTYPE`` record, as the device reports it (``filed``: of the last ``file``, 0 before)."""
        rec = np.zeros((), dtype=_lib.CROWD_GRID_DTYPE)
        rec["origin"], rec["h"] = self.origin, self.h
        rec["nx"], rec["ny"], rec["layers"], rec["filed"] = self.nx, self.ny, self.layers, self.filed
        return rec

    def file(self, table):
        """File the entries of ``table`` [D, layers, >= 2]: entry (d, k) under the cell of its position in layer k, unfiled if a
        coordinate is not finite -> ``cell_of`` [D, layers] int32."""
        table = np.asarray(table, dtype=np.float64)
        D, N = table.shape[:2]
        assert N == self.layers
        x, y = table[:, :, 0], table[:, :, 1]
        ok = np.isfinite(x) & np.isfinite(y)
        key = (np.arange(N, dtype=np.int64)[None, :] * self.ny + grid_cellof(y, self.origin[1], self.h[1], self.ny)) * self.nx \
            + grid_cellof(x, self.origin[0], self.h[0], self.nx)
        self.cell_of = np.where(ok, key, -1).astype(np.int32)
        flat = self.cell_of.reshape(-1)
        who = np.nonzero(flat >= 0)[0]                                      # entries e = d * layers + k, ascending
        self.filed = len(who)
        order = who[np.argsort(flat[who], kind="stable")]                   # ascending d inside a cell (its k is the layer's)
        self.cell_mem = (order // N).astype(np.int64)
        self.cell_off = np.concatenate([[0], np.cumsum(np.bincount(flat[who], minlength=self.layers * self.nx * self.ny))]).astype(np.int64)
        return self.cell_of

    def window(self, x, y, range):
        """-> (cx0, cx1, cy0, cy1), inclusive: the cells of a layer that a robot at (x, y) looks at; None unless both are finite."""
        x, y, r = np.float64(x), np.float64(y), np.float64(range)
        if not (np.isfinite(x) and np.isfinite(y)):
            return None
        with np.errstate(over="ignore"):
            return self._cellof(x - r, 0), self._cellof(x + r, 0), self._cellof(y - r, 1), self._cellof(y + r, 1)

    def row_ranges(self, pred_b, range):
        """-> [(k, i0, i1)] per row of the robot's windows, stage after stage: the row's entries are ``cell_mem[i0:i1]`` at stage k."""
        out = []
        for k in np.arange(self.layers):
            w = self.window(pred_b[k][0], pred_b[k][1], range)
            if w is None:
                continue
            cx0, cx1, cy0, cy1 = w
            for row in np.arange(cy0, cy1 + 1):
                at = (k * self.ny + row) * self.nx
                out.append((k, int(self.cell_off[at + cx0]), int(self.cell_off[at + cx1 + 1])))
        return out

    def candidates(self, pred_b, range):
        """-> (d, k): the filed entries in the windows of a robot with the predicted positions ``pred_b`` [layers, >= 2], row after
        row and stage after stage, as two int64 arrays."""
        rr = self.row_ranges(pred_b, range)
        if not rr:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return (np.concatenate([self.cell_mem[i0:i1] for _, i0, i1 in rr]),
                np.concatenate([np.full(i1 - i0, k, dtype=np.int64) for k, i0, i1 in rr]))

    def looked(self, pred_b, range):
        """-> the number of filed entries in the robot's windows (what the device reports as ``looked``)."""
        return sum(i1 - i0 for _, i0, i1 in self.row_ranges(pred_b, range))


def crowd_grid(obstacles, N, cell):
    """The geometry of the crowd's rule with a ``cell`` for ``obstacles`` = (p1 [D, 2], p2 [D, 2], ...) and a
    horizon of ``N`` stages, in the setter's arithmetic: -> a ``CrowdGrid``, nothing filed yet.

    ``origin`` is the minimum per axis over the end points p1, p2 whose two coordinates are finite; an axis has floor(extent / cell) + 1
    cells of edge ``cell``, or ``CROWD_GRID_CAP`` cells of edge extent / ``CROWD_GRID_CAP`` where that would be more; without a finite
    end point the grid is one cell at (0, 0).  There are N layers.  Entry (d, k) of a step's table is filed under the cell of its
    position in layer k; a robot looks, at stage k, at the cells from that of ``x - range`` to that of ``x + range`` per axis: every
    entry with d_k < range^2 is filed there, inside the extent or not, because the cell of a coordinate is clamped and monotone."""
    ends = np.concatenate([np.asarray(obstacles[0], dtype=np.float64).reshape(-1, 2), np.asarray(obstacles[1], dtype=np.float64).reshape(-1, 2)])
    ends = ends[np.isfinite(ends).all(axis=1)]
    g = CrowdGrid()
    g.cell, g.layers, g.filed = float(cell), int(N), 0
    g.nx = g.ny = 1
    g.origin, g.h = np.zeros(2), np.array([g.cell, g.cell])
    if len(ends):
        g.origin = ends.min(axis=0)
        with np.errstate(over="ignore"):
            ext = ends.max(axis=0) - g.origin
        (g.nx, hx), (g.ny, hy) = (grid_axis(ext[ax], g.cell, CROWD_GRID_CAP) for ax in (0, 1))
        g.h = np.array([hx, hy])
    return g


@dataclasses.dataclass(frozen=True)
class Monitor:
    """The clearance monitor, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: per robot,
    the closest approach to the static circles, to the scripted ellipses and to the other robots of its monitor group over the
    poses driven so far, and the trajectory row of each (``clearance``, a ``_lib.CLEARANCE_DTYPE`` array [B]).  It observes only.
    ``group_of`` [B] = the monitor group of each robot, values in [0, B) (``None``: one group of all B), whatever ``Peers`` says."""
    group_of: object = None

    def checked(self, B: int):
        """-> group_of as an int32 array or None; ValueError for what ``nmpc_loop_set_monitor`` refuses."""
        return _checked_groups("monitor", self.group_of, B)


@dataclasses.dataclass(frozen=True)
class Missions:
    """A sequence of routes per robot, driven leg after leg, for ``FleetRecedingHorizon`` and
    ``DeviceRecedingHorizon`` alike, both with ``retire=True``: ``legs[b]`` = the indices of robot b's routes in the order it drives
    them, the first one its ``route_of``.  A robot whose terminal test holds takes up its next leg in the same step, as the
    reference's user calls ``PathGenerator.run`` again from where the robot stands, and retires after its last."""
    legs: object

    def checked(self, B: int, R: int, route_of):
        """-> (leg_off [B + 1], leg_route [leg_off[B]]) as int32 arrays; ValueError for what ``nmpc_loop_set_missions`` refuses."""
        legs = [np.asarray(m, dtype=np.int64).reshape(-1) for m in self.legs]
        if len(legs) != B:
            raise ValueError(f"missions: {len(legs)} missions for {B} robots")
        if any(len(m) < 1 for m in legs):
            raise ValueError("missions: a robot with no leg")
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(m) for m in legs])
        route = np.concatenate(legs)
        if ((route < 0) | (route >= R)).any():
            raise ValueError("missions: a leg's route out of range")
        first = np.zeros(B, dtype=np.int64) if route_of is None else np.asarray(route_of, dtype=np.int64).reshape(B)
        if not np.array_equal(route[off[:-1]], first):
            raise ValueError("missions: a robot's first leg is not its route_of")
        return off, np.ascontiguousarray(route, dtype=np.int32)


def no_clearance(B: int):
    """-> the initial records [B]: +inf, row -1, peer -1."""
    rec = np.empty(B, dtype=_lib.CLEARANCE_DTYPE)
    rec["circle"] = rec["ellipse"] = rec["peer2"] = np.inf
    rec["circle_row"] = rec["ellipse_row"] = rec["peer_row"] = rec["peer"] = -1
    return rec


def no_crowd_clearance(B: int):
    """-> the crowd observer's initial records [B]: +inf, row -1, obstacle -1."""
    rec = np.empty(B, dtype=_lib.CROWD_CLEARANCE_DTYPE)
    rec["level"] = np.inf
    rec["row"] = rec["obstacle"] = -1
    return rec


MAP_MAX_EDGES = 1024        # E of a map monitor's map (nmpc_loop_set_map_monitor)


def no_map_clearance(B: int):
    """-> the initial map records [B]: wall2 +inf, rows, edge and polygon -1, no hits."""
    rec = np.zeros(B, dtype=_lib.MAP_CLEARANCE_DTYPE)
    rec["wall2"] = np.inf
    rec["wall_row"] = rec["wall_edge"] = rec["hit_row"] = rec["hit_poly"] = -1
    return rec


@dataclasses.dataclass(frozen=True)
class MapMonitor:
    """The map monitor, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: per robot, the closest
    approach to the walls of a polygon map over the poses driven so far, and the rows at which it stood inside an obstacle, outside the
    boundary or went through an edge between two rows (``map_clearance``, a ``_lib.MAP_CLEARANCE_DTYPE`` array [B]).  It observes only.
    ``edges`` [E, 4] = (x1, y1, x2, y2) polygon by polygon, the obstacles first and the boundary last; ``poly_off`` [n_poly + 1]: polygon
    k owns the edges poly_off[k] .. poly_off[k + 1] (``frontend.map_edges`` gives both for a planner's scene).

    ``cell`` and ``range`` (metres, both or neither; ``None``: every pose against every edge, 1024 edges at the most) find the edges a
    row is judged against through the walls grid (``wall_grid``, ``nmpc_loop_set_map_monitor_grid``): up to 1048576 edges.  Hits are the
    all-edges rule's; the wall record keeps only distances below ``range`` (``rows_grid``)."""
    edges: object
    poly_off: object
    cell: float = None
    range: float = None

    def checked(self):
        """-> (edges [E, 4] float64, poly_off [n_poly + 1] int32), contiguous; ValueError for what ``nmpc_loop_set_map_monitor``, or with
        a ``cell`` ``nmpc_loop_set_map_monitor_grid``, refuses."""
        edges = np.ascontiguousarray(self.edges, dtype=np.float64)
        off = np.ascontiguousarray(self.poly_off, dtype=np.int32).reshape(-1)
        if edges.ndim != 2 or edges.shape[1] != 4:
            raise ValueError(f"map monitor: edges of shape {edges.shape}, not [E, 4]")
        E, n_poly = len(edges), len(off) - 1
        most = MAP_MAX_EDGES if self.cell is None else WALL_GRID_MAX_EDGES
        if E < 3 or E > most:
            raise ValueError(f"map monitor: {E} edges, 3 to {most} are taken")
        if n_poly < 1 or n_poly > E // 3:
            raise ValueError(f"map monitor: {n_poly} polygons for {E} edges")
        if off[0] != 0 or off[-1] != E or (np.diff(off) < 3).any():
            raise ValueError("map monitor: poly_off must ascend from 0 to E in steps of three edges at least")
        if not np.isfinite(edges).all():
            raise ValueError("map monitor: a coordinate that is not finite")
        if (self.cell is None) != (self.range is None):
            raise ValueError("map monitor: cell and range go together")
        if self.cell is not None:
            for v in (self.cell, self.range):
                if not (math.isfinite(v) and v > 0):
                    raise ValueError("map monitor: cell and range must be finite and positive")
            self.grid                                                       # (ValueError for more filings than the grid takes)
        return edges, off

    @functools.cached_property
    def grid(self):
        """The walls grid over the map's edges (``wall_grid(edges, cell)``), built at the first use."""
        return wall_grid(self.edges, self.cell)

    @functools.cached_property
    def _edge_poly(self):
        off = np.asarray(self.poly_off, dtype=np.int64).reshape(-1)
        return np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off))

    def rows_grid(self, ax, ay, x, y):
        """The rule with a ``cell`` for n poses, one at a time over the edges its cells hold -> (v, e, poly, looked)
        [n]: as ``rows``, but v is +inf (and e -1) unless a wall of the window is closer than ``range``; ``looked`` counts the distinct
        edges of each row's window W(r), all E for a row with a coordinate that is not finite."""
        edges, off = self.checked()
        g, owner, n_poly = self.grid, self._edge_poly, len(off) - 1
        ax, ay, x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ax, ay, x, y))
        n, E = len(x), len(edges)
        rng, tm = np.float64(self.range), np.float64(2.0 ** -40)
        slack = tm * (rng + g.amax) + np.float64(2.0 ** -500)
        r2 = rng * rng
        v_out, e_out = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        poly_out, looked = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)

        def filed(cx0, cx1, cy0, cy1):
            """the distinct edges filed in the cells cx0 .. cx1 x cy0 .. cy1, ascending"""
            at = np.arange(cy0, cy1 + 1) * g.nx
            lo, hi = g.cell_off[at + cx0], g.cell_off[at + cx1 + 1]
            if (hi - lo).sum() > E:                                         # cheaper by the edges' rectangles: the same set
                r = g.rect
                return np.nonzero((r[:, 0] <= cx1) & (r[:, 1] >= cx0) & (r[:, 2] <= cy1) & (r[:, 3] >= cy0))[0]
            return np.unique(np.concatenate([g.cell_edge[a:b] for a, b in zip(lo, hi)]))

        def m(v):
            return slack + tm * abs(v)
        with np.errstate(all="ignore"):
            for i in range(n):
                X, Y, AX, AY = x[i], y[i], ax[i], ay[i]
                if np.isfinite([X, Y, AX, AY]).all():
                    lo, hi = (min(X, AX), min(Y, AY)), (max(X, AX), max(Y, AY))
                    win = filed(g._cellof((lo[0] - rng) - m(lo[0]), 0), g._cellof((hi[0] + rng) + m(hi[0]), 0),
                                g._cellof((lo[1] - rng) - m(lo[1]), 1), g._cellof((hi[1] + rng) + m(hi[1]), 1))
                    cy = g._cellof(Y, 1)
                    ray = filed(g._cellof(X - m(X), 0), g.nx - 1, cy, cy)
                else:
                    win = ray = np.arange(E)
                looked[i] = len(win)
                x1, y1, x2, y2 = (edges[win, k] for k in range(4))
                v = segment_closest(X, Y, x1, y1, x2, y2)[0]
                v = np.where(v < r2, v, np.inf)                             # (a NaN is no candidate)
                if len(v) and v.min() < np.inf:
                    k = int(np.argmin(v))                                   # the first of equal values: the edges ascend
                    v_out[i], e_out[i] = v[k], win[k]
                ex, ey = x2 - x1, y2 - y1
                ux, uy = X - AX, Y - AY
                o1 = ux * (y1 - AY) - uy * (x1 - AX)
                o2 = ux * (y2 - AY) - uy * (x2 - AX)
                o3 = ex * (AY - y1) - ey * (AX - x1)
                o4 = ex * (Y - y1) - ey * (X - x1)
                fails = np.zeros(n_poly, dtype=bool)
                fails[owner[win[(o1 * o2 < -1e-9) & (o3 * o4 < -1e-9)]]] = True
                x1, y1, x2, y2 = (edges[ray, k] for k in range(4))
                straddle = (y1 > Y) != (y2 > Y)
                xi = x1 + ((Y - y1) * (x2 - x1)) / np.where(straddle, y2 - y1, 1.0)
                odd = (np.bincount(owner[ray[straddle & (xi > X)]], minlength=n_poly) & 1).astype(bool)
                odd[-1] = ~odd[-1]                                          # the boundary fails on an even count
                fails |= odd
                if fails.any():
                    poly_out[i] = np.argmax(fails)
        return v_out, e_out, poly_out, looked

    def rows(self, ax, ay, x, y):
        """The rule for n poses (x, y) [n], each with the pose (ax, ay) of the row before -> (v [n], e [n], poly [n]): the smallest squared
        wall distance that is not NaN (+inf without any) and the first edge that has it, and the smallest failing polygon index, -1
        if none fails.  Unfused f64 in the order DESIGN.md section 5.9 writes.  With a ``cell``: ``rows_grid`` without its count."""
        if self.cell is not None:
            return self.rows_grid(ax, ay, x, y)[:3]
        edges, off = self.checked()
        ax, ay, x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ax, ay, x, y))
        n, chunk = len(x), max(1, (1 << 20) // len(edges))
        if n > chunk:
            parts = [self.rows(ax[i:i + chunk], ay[i:i + chunk], x[i:i + chunk], y[i:i + chunk]) for i in range(0, n, chunk)]
            return tuple(np.concatenate(c) for c in zip(*parts))
        x1, y1, x2, y2 = (edges[:, k][None, :] for k in range(4))
        X, Y, AX, AY = x[:, None], y[:, None], ax[:, None], ay[:, None]
        at = np.arange(n)
        v = segment_closest(X, Y, x1, y1, x2, y2)[0]
        v = np.where(np.isnan(v), np.inf, v)
        e = np.argmin(v, axis=1)
        with np.errstate(all="ignore"):
            # crossing between the two rows (frontend._seg_intersect_strict)
            ex, ey = x2 - x1, y2 - y1
            ux, uy = X - AX, Y - AY
            o1 = ux * (y1 - AY) - uy * (x1 - AX)
            o2 = ux * (y2 - AY) - uy * (x2 - AX)
            o3 = ex * (AY - y1) - ey * (AX - x1)
            o4 = ex * (Y - y1) - ey * (X - x1)
            crossed = (o1 * o2 < -1e-9) & (o3 * o4 < -1e-9)
            # containment: even-odd count per polygon
            straddle = (y1 > Y) != (y2 > Y)
            xi = x1 + ((Y - y1) * ex) / np.where(straddle, ey, 1.0)
            hit = straddle & (xi > X)
        first = off[:-1].astype(np.intp)
        fails = (np.add.reduceat(hit.astype(np.int32), first, axis=1) & 1).astype(bool)          # [n, n_poly]: an odd count
        fails[:, -1] = ~fails[:, -1]                                                            # the boundary fails on an even one
        fails |= np.add.reduceat(crossed.astype(np.int32), first, axis=1) > 0
        poly = np.where(fails.any(axis=1), np.argmax(fails, axis=1), -1).astype(np.int32)
        return v[at, e], e.astype(np.int32), poly

    def scan(self, traj):
        """The rule over the rows >= 1 of a recorded trajectory table [rows, B, 3] (row r against row r - 1) -> the records [B] a monitor
        would hold for robots driven over all those rows."""
        T = np.asarray(traj, dtype=np.float64)
        R, B = T.shape[0], T.shape[1]
        rec = no_map_clearance(B)
        if R < 2 or B == 0:
            return rec
        a, b = T[:-1].reshape(-1, 3), T[1:].reshape(-1, 3)
        v, e, poly = (q.reshape(R - 1, B) for q in self.rows(a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
        at = np.arange(B)
        k = np.argmin(v, axis=0)                                            # the first row with the smallest value
        seen = v[k, at] < np.inf
        rec["wall2"][seen], rec["wall_row"][seen], rec["wall_edge"][seen] = v[k, at][seen], k[seen] + 1, e[k, at][seen]
        hit = poly >= 0
        k = np.argmax(hit, axis=0)
        some = hit.any(axis=0)
        rec["hits"] = hit.sum(axis=0)
        rec["hit_row"][some], rec["hit_poly"][some] = k[some] + 1, poly[k, at][some]
        return rec


def no_tracking(B: int):
    """-> the track monitor's initial records [B]: sums, maxima and counts 0, rows and segments -1."""
    rec = np.zeros(B, dtype=_lib.TRACKING_DTYPE)
    rec["cte_row"] = rec["cte_seg"] = rec["dth_row"] = rec["last_seg"] = rec["off_row"] = -1
    return rec


@dataclasses.dataclass(frozen=True)
class TrackMonitor:
    """The track monitor, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: per robot, how far the
    poses driven so far were from the route it was asked to follow -- the largest and the summed squared distance to the polyline through
    the route's reference samples, the largest and the summed squared heading error against the sample at the end of the closest segment,
    the rows at which the maxima occurred, the closest segment of the newest row (progress along the route) and the rows further than
    ``tol`` metres from the route (``tracking()``, a ``_lib.TRACKING_DTYPE`` array [B]).  The heading error is NOT wrapped: the cost does
    not wrap either (``cost_fn``, src/mpc/mpc_generator.py:59-63), so it is the error the controller itself sees.  It observes only."""
    tol: float = 0.5

    def checked(self):
        """-> ``tol`` as a float; ValueError for what ``nmpc_loop_set_track_monitor`` refuses."""
        try:
            tol = float(self.tol)
        except (TypeError, ValueError):
            raise ValueError(f"track monitor: tol = {self.tol!r} is not a number") from None
        if not (tol >= 0.0) or not math.isfinite(tol):
            raise ValueError(f"track monitor: tol = {tol} must be finite and not negative")
        return tol

    @staticmethod
    def table(routes):
        """-> (ref [R, W, 3], n [R]): every route's reference samples (x, y, theta) side by side, W the longest route's, a row padded with
        its last sample; each route's own length.  ``routes``: objects with ``x_ref``, ``y_ref`` and ``theta_ref`` (``harness.Route``)."""
        rows = [np.stack([np.asarray(r.x_ref, dtype=np.float64), np.asarray(r.y_ref, dtype=np.float64),
                          np.asarray(r.theta_ref, dtype=np.float64)], axis=1) for r in routes]
        n = np.array([len(v) for v in rows], dtype=np.int64)
        assert (n >= 1).all()
        ref = np.empty((len(rows), int(n.max()), 3))
        for r, v in enumerate(rows):
            ref[r, :len(v)], ref[r, len(v):] = v, v[-1]
        return ref, n

    @staticmethod
    def rows(table, route_of, x, y):
        """The rule's distance for m poses (x, y) [m], pose i against route ``route_of[i]`` of ``table`` -> (v [m], j [m]): the smallest
        squared distance to a segment that is not NaN and the first segment that has it; (+inf, -1) where there is none.  Unfused f64 in
        the order DESIGN.md section 5.9 writes; segment 0 is not clamped below."""
        ref, n = table
        route_of = np.asarray(route_of, dtype=np.int64).reshape(-1)
        x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
        m, S = len(x), max(ref.shape[1] - 1, 1)
        chunk = max(1, (1 << 20) // S)
        if m > chunk:
            parts = [TrackMonitor.rows(table, route_of[i:i + chunk], x[i:i + chunk], y[i:i + chunk]) for i in range(0, m, chunk)]
            return tuple(np.concatenate(c) for c in zip(*parts))
        nr = n[route_of][:, None]
        j = np.arange(S)[None, :]
        valid = j < np.maximum(nr - 1, 1)
        rt = route_of[:, None]
        a, e = np.minimum(j, nr - 1), np.minimum(j + 1, nr - 1)
        x1, y1, x2, y2 = ref[rt, a, 0], ref[rt, a, 1], ref[rt, e, 0], ref[rt, e, 1]
        X, Y = x[:, None], y[:, None]
        v = segment_closest(X, Y, x1, y1, x2, y2, clamp_below=j > 0)[0]
        v = np.where(np.isnan(v) | ~valid, np.inf, v)
        k = np.argmin(v, axis=1)                                            # the first segment with the smallest value
        best = v[np.arange(m), k]
        return best, np.where(best < np.inf, k, -1).astype(np.int32)

    def fold(self, rec, who, r, table, route_of, pose):
        """Trajectory row ``r`` of the robots ``who`` [m] (distinct), their poses ``pose`` [m, 3] against the routes ``route_of`` [m] of
        ``table``, into the records ``rec`` [B], in place: the rule's update, both maxima strict."""
        tol = self.checked()
        ref, n = table
        who, route_of = np.asarray(who, dtype=np.int64), np.asarray(route_of, dtype=np.int64).reshape(-1)
        pose = np.asarray(pose, dtype=np.float64).reshape(-1, 3)
        v, j = self.rows(table, route_of, pose[:, 0], pose[:, 1])
        rec["rows"][who] += 1
        ok = j >= 0
        b, v, j, rt, th = who[ok], v[ok], j[ok], route_of[ok], pose[ok, 2]
        e = np.minimum(j + 1, n[rt] - 1)
        with np.errstate(all="ignore"):
            d = th - ref[rt, e, 2]
            a = np.where(d < 0, -d, d)
            rec["cte2_sum"][b] = rec["cte2_sum"][b] + v
            rec["dth2_sum"][b] = rec["dth2_sum"][b] + d * d
            up = v > rec["cte2_max"][b]
            rec["cte2_max"][b[up]], rec["cte_row"][b[up]], rec["cte_seg"][b[up]] = v[up], r, j[up]
            up = a > rec["dth_max"][b]
            rec["dth_max"][b[up]], rec["dth_row"][b[up]] = a[up], r
            rec["last_seg"][b] = j
            off = v > tol * tol
        first = off & (rec["off_row"][b] == -1)
        rec["off_row"][b[first]] = r
        rec["off_rows"][b[off]] += 1

    def scan(self, traj, routes, route_of=None):
        """The rule over the rows >= 1 of a recorded trajectory table [rows, B, 3] (x, y, theta), robot b against the fixed route
        ``routes[route_of[b]]`` (default: route 0) -> the records [B] a monitor would hold for robots driven over all those rows."""
        T = np.asarray(traj, dtype=np.float64)
        B = T.shape[1]
        rec = no_tracking(B)
        route_of = np.zeros(B, dtype=np.int64) if route_of is None else np.asarray(route_of, dtype=np.int64).reshape(B)
        table, who = self.table(routes), np.arange(B)
        for r in range(1, T.shape[0]):
            self.fold(rec, who, r, table, route_of, T[r])
        return rec


@dataclasses.dataclass(frozen=True)
class DriveLog:
    """The drive log, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: the controls every robot
    applied, one record per robot and step of how its solve ended, a cumulative summary per robot and the fleet's totals per step
    (``controls``, ``step_records``, ``drive_summary``, ``step_totals``).  It observes only."""


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32, _SH32 = np.uint64(0xFFFFFFFF), np.uint64(32)
PLANT_XI_SCALE = float.fromhex("0x1.bb67ae8584caap-32")       # the double nearest sqrt(3), scaled exactly by 2^-32


def philox4x32_10(counter, key):
    """Philox4x32-10 as published (csrc/nmpc_rng.h), vectorised: ``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words (broadcast
    against each other) -> the four output words [..., 4] uint32.  The words are carried in uint64, so that a product keeps its high
    half."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ k0, p1 & _U32, (p0 >> _SH32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def plant_xi(seed, ids, row, channel):
    """One disturbance per entry of ``ids`` (csrc/nmpc_rng.h): the counter is (id, row, channel, 0), the key
    (seed & 0xffffffff, seed >> 32), S the sum of the four output words and xi = float(S + 2 - 2^33) * ``PLANT_XI_SCALE``.  Everything
    before the one multiplication is exact: the device's double, bit for bit.  Mean 0, variance 1, |xi| <= 2 sqrt(3)."""
    ids = np.asarray(ids, dtype=np.uint64)
    counter = np.zeros(ids.shape + (4,), dtype=np.uint64)
    counter[..., 0], counter[..., 1], counter[..., 2] = ids, np.uint64(row), np.uint64(channel)
    words = philox4x32_10(counter, [int(seed) & 0xFFFFFFFF, int(seed) >> 32])
    S = words.astype(np.int64).sum(axis=-1)
    return (S + np.int64(2 - 2 ** 33)).astype(np.float64) * PLANT_XI_SCALE


@dataclasses.dataclass(frozen=True)
class Plant:
    """A disturbed plant, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` alike: the world does not
    do what the model says.  Every disturbance is ``sigma * plant_xi(seed, id, row, channel)``, so a robot's depend on the seed, its
    id and the trajectory row, never on who else is active or on how a fleet is split.
    ``act_gain``, ``act_add`` (v, omega): the control that acts is ``u + (act_gain * u + act_add) * xi``; ``proc`` (x, y, theta): added
    to the pose after every control; ``meas`` (x, y, theta): added to the pose the assembly and the predictions start from, the true
    pose untouched.  ``ids`` [B] uint32 (``None``: robot b has id b).  ``keep_applied`` (the device needs ``max_steps`` > 0):
    ``applied()`` keeps the controls that acted.  ``last_u`` and the drive log hold the commanded controls; the trajectory, the
    monitors and retirement see the true pose.  A plant of zeros changes no bit."""
    seed: int = 0
    act_gain: tuple = (0.0, 0.0)
    act_add: tuple = (0.0, 0.0)
    proc: tuple = (0.0, 0.0, 0.0)
    meas: tuple = (0.0, 0.0, 0.0)
    ids: object = None
    keep_applied: bool = False

    def checked(self, B: int):
        """-> (act_gain [2], act_add [2], proc [3], meas [3] as float64 arrays, ids [B] uint32 or None); ValueError for what
        ``nmpc_loop_set_plant`` refuses, a seed outside 64 bits and ``ids`` of another length."""
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError("plant: the seed is an unsigned 64-bit integer")
        out = []
        for name, n in (("act_gain", 2), ("act_add", 2), ("proc", 3), ("meas", 3)):
            v = np.array(getattr(self, name), dtype=np.float64).reshape(-1)
            if v.shape != (n,):
                raise ValueError(f"plant: {name} takes {n} values")
            if not (np.isfinite(v) & (v >= 0)).all():
                raise ValueError(f"plant: {name} must be finite and >= 0")
            out.append(v)
        ids = None
        if self.ids is not None:
            ids = np.asarray(self.ids).reshape(-1)
            if ids.shape != (B,):
                raise ValueError(f"plant: {len(ids)} ids for {B} robots")
            if not np.issubdtype(ids.dtype, np.integer) or ((ids < 0) | (ids > 0xFFFFFFFF)).any():
                raise ValueError("plant: ids are unsigned 32-bit integers")
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
        return (*out, ids)


ENSEMBLE_MAX_GROUPS = 65536  # G of an ensemble at the most (nmpc_loop_set_ensemble)


@dataclasses.dataclass(frozen=True)
class Ensemble:
    """Per-group pose statistics after every step, for ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon``
    alike: the robots are partitioned into ``groups`` groups, ``group_of`` [B] = the group of each robot (``None``: one group of
    everybody; ``groups`` defaults to ``max(group_of) + 1``, or 1), and after every step one ``_lib.ENSEMBLE_DTYPE`` record per group
    holds the member count, how many have arrived, the mean pose, the population covariance of the position and the variance of the
    heading against that mean, and the member furthest from the mean position (``ensemble_stats()`` [steps, G]).  Every member counts,
    active or retired, with its true pose; sums are taken by the fixed tree of ``ensemble_sum``.  A group may be empty.  It observes
    only."""
    group_of: object = None
    groups: int = None

    def checked(self, B: int):
        """-> (group_of [B] as an int32 array or None, G); ValueError for what ``nmpc_loop_set_ensemble`` refuses and for a
        ``group_of`` of another length."""
        g = None
        if self.group_of is not None:
            g = np.ascontiguousarray(self.group_of, dtype=np.int32).reshape(-1)
            if g.shape != (B,):
                raise ValueError(f"ensemble: {len(g)} group ids for {B} robots")
        G = self.groups
        if G is None:
            G = 1 if g is None or not len(g) else int(g.max()) + 1
        G = int(G)
        if G < 1 or G > ENSEMBLE_MAX_GROUPS:
            raise ValueError(f"ensemble: {G} groups, 1 to {ENSEMBLE_MAX_GROUPS} are taken")
        if g is None and G != 1:
            raise ValueError("ensemble: groups != 1 without group_of")
        if g is not None and ((g < 0) | (g >= G)).any():
            raise ValueError("ensemble: group_of out of range")
        return g, G


def ensemble_sum(v):
    """The ensemble's sum of one value per member, ``v`` [n] -> a float, or ``v`` [n, k] -> [k], column by
    column: slot t of 256 starts at +0.0 and takes ``acc = acc + v[i]`` for i = t, t + 256, ... in ascending i; within each block of
    64 slots, for off = 32, 16, 8, 4, 2, 1, ``a[l] = a[l] + a[l + off]`` for l < off; the four block sums give ``((w0 + w1) + w2) + w3``.
    The device's bits: its workgroup of 256 threads and its wave reductions add in this order."""
    v = np.asarray(v, dtype=np.float64)
    flat = v.ndim == 1
    v = v[:, None] if flat else v
    n, k = v.shape
    acc = np.zeros((256, k))
    with np.errstate(all="ignore"):
        for i in range(0, n, 256):
            m = min(256, n - i)
            acc[:m] = acc[:m] + v[i:i + m]
        a = acc.reshape(4, 64, k)
        off = 32
        while off >= 1:
            a[:, :off] = a[:, :off] + a[:, off:2 * off]
            off >>= 1
        w = a[:, 0]
        out = ((w[0] + w[1]) + w[2]) + w[3]
    return float(out[0]) if flat else out


def no_ensemble_stats(steps: int, G: int):
    """-> the records [steps, G] of empty groups: zeros, ``far2`` -1.0 and ``far_robot`` -1."""
    rec = np.zeros((steps, G), dtype=_lib.ENSEMBLE_DTYPE)
    rec["far2"], rec["far_robot"] = -1.0, -1
    return rec


def no_step_records(steps: int, B: int):
    """-> the initial records [steps, B]: exit_status -1, everything else 0."""
    rec = np.zeros((steps, B), dtype=_lib.STEP_RECORD_DTYPE)
    rec["exit_status"] = -1
    return rec


def no_drive_summary(B: int):
    """-> the initial summaries [B]: zeros, the two ``*_step`` fields -1."""
    rec = np.zeros(B, dtype=_lib.DRIVE_SUMMARY_DTYPE)
    rec["inner_max_step"] = rec["f2_max_step"] = -1
    return rec


def no_step_totals(steps: int):
    """-> the totals of ``steps`` steps with nobody active: zeros."""
    return np.zeros(steps, dtype=_lib.STEP_TOTALS_DTYPE)


class FleetRecedingHorizon(VectorizedRecedingHorizon):
    """``VectorizedRecedingHorizon`` for a fleet on R routes: robot b follows ``routes[route_of[b]]``.

    The step is ``VectorizedRecedingHorizon``'s, which reads everything of a route through ``route_of[b]``, so each robot's quantities
    are exactly those of the single-route mirror for its route; one ``solve_fn(P, u0, y0) -> (U, Y, status)`` call covers the whole
    fleet per step.  This class adds what is the fleet's: peers, retirement, the monitor and missions.  ``dyn_obs``, ``sincos`` and
    ``sinus_object`` as in ``VectorizedRecedingHorizon``; ``idx0`` = the reference sample each robot starts at, on its own route
    (default 0).

    ``peers`` (a ``Peers``) lets the robots of a group see each other: ``assemble`` overlays the chosen peers on the parameter
    vectors it returns, never on the carried dynamic blocks.  With ``peers.cell`` the distances are formed over
    ``peer_grid(...).candidates`` only (``grid`` keeps the step's ``PeerGrid``): the same peers, at a cost that lets a fleet be one group.

    ``retire=True``: a robot whose terminal test holds after an advance leaves the loop for good, as the reference's
    ``while not terminal`` ends for one robot.  Everybody is ``active`` at the first step; a retired robot
    is not assembled, solved or advanced again, keeps every value of its last step (``done`` stays True, its trajectory rows repeat
    its final pose), and ``retired_at[b]`` = the steps (solves) it took, -1 while it is active.  For peers it is a parked obstacle:
    predicted at its state at every stage, a candidate for the others, given no peers itself.  ``step`` solves the active rows only.

    ``monitor`` (a ``Monitor``): ``clearance`` [B] holds every robot's closest approaches, updated by
    ``advance`` from the rows it appends to ``traj`` and the parameter vectors ``assemble`` returned for this step, for the robots
    the step drove.  Nothing else reads it.

    ``map_monitor`` (a ``MapMonitor``): ``map_clearance`` [B] holds every robot's closest approach to the map's walls and its hits
    (DESIGN.md section 5.9), updated by ``advance`` from the rows it appends to ``traj``, for the robots the step drove.  With a ``cell``
    the rule is the grid's (``MapMonitor.rows_grid``) and ``map_looked`` [B] counts the distinct edges of the windows of each robot's
    last step.

    ``missions`` (a ``Missions``, needs ``retire=True``): ``retire`` re-dispatches an active robot that is done and has another leg
    instead of retiring it: ``leg`` [B] and ``route_of`` [B] move on, ``leg_at`` [B, Lmax] takes the step count
    at which each leg ended (-1: not yet, or no such leg), the robot's reference sample, ``last_u``, ``U`` and ``Y`` rows are zeroed
    and ``done`` cleared, in place; its state, carried dynamic block and trajectory are not touched.

    ``log`` (a ``DriveLog``): ``controls`` [steps * s, B, 2], ``step_records`` [steps, B], ``drive_summary`` [B] and ``step_totals``
    [steps] (the ``_lib.*_DTYPE`` records of the device), updated by ``advance`` -- before ``retire``, so a
    record names the leg its solve belonged to -- from the controls it applied, the statuses ``step`` got from its ``solve_fn``, the
    rows it appended to ``traj`` and the parameter vectors ``assemble`` returned for this step, for the robots the step drove.

    ``crowd`` (a ``Crowd``): D moving obstacles of the world.  ``assemble`` advances their table
    (``crowd_table()`` [D, N, 5]), every step and whoever is active, and overlays each active robot's closest ones on the parameter
    vectors it returns, in front of the peers and never on the carried dynamic blocks; ``crowd_seen`` [B, slots] names them (a retired
    robot keeps its last); ``crowd_who`` and ``crowd_pred`` [B, N, 3] keep the robots the last selection ran for and the predictions
    it read.  With ``crowd.watch``, ``advance`` updates ``crowd_clearance()`` [B] for the robots the step drove.  With
    ``crowd.cell`` C is formed through ``crowd_grid`` only (the ``CrowdGrid``, filed anew every step with an active robot): the same
    obstacles, and ``crowd_looked`` [B] counts the entries each robot looked at; without it this class stays the all-obstacles yardstick.

    ``plant`` (a ``Plant``): seeded actuation, process and measurement noise.  ``assemble`` and ``predict``
    start from the measured poses (``measured()`` [B, 3]) and nothing else does; ``advance`` applies the disturbed controls and adds
    the process noise, ``state`` and ``traj`` are the true poses, ``last_u`` and the drive log the commanded controls;
    ``applied()`` [steps * s, B, 2] = the controls that acted, with ``plant.keep_applied``.

    ``ensemble`` (an ``Ensemble``): ``ensemble_stats()`` [steps, G] holds one ``_lib.ENSEMBLE_DTYPE`` record per group and step
    (DESIGN.md section 5.9), appended by ``step`` when everything else of the step is over -- behind ``advance`` and, on a retiring
    fleet, ``retire`` -- from the true poses of all members, ``retired_at`` (a retiring fleet) or ``done``.  Nothing else reads it.

    ``track`` (a ``TrackMonitor``): ``tracking()`` [B] holds how far every robot was from its route, in position and heading
    (DESIGN.md section 5.9), updated by ``advance`` -- before ``retire``, so a row is measured against the leg it was driven on --
    from the rows it appends to ``traj`` (under a plant the true poses), for the robots the step drove.
    """

    def __init__(self, routes, route_of, starts, dyn_obs=None, sincos=None, sinus_object=False, idx0=None, peers=None, retire=False,
                 monitor=None, missions=None, map_monitor=None, log=None, crowd=None, plant=None, ensemble=None, walls=None, track=None):
        self.routes = list(routes)
        cfg, B = self.routes[0].cfg, len(starts)
        route_of = np.asarray(route_of, dtype=np.int64).reshape(B)
        assert all(r.cfg is cfg or r.cfg == cfg for r in self.routes)
        assert ((route_of >= 0) & (route_of < len(self.routes))).all()
        self._init_robots(self.routes, route_of, starts, dyn_obs, sincos, sinus_object, idx0)
        self.missions = missions
        if missions is not None:
            if not retire:
                raise ValueError("missions need retire=True")
            off, route = missions.checked(B, len(self.routes), self.route_of)
            self.legs = [route[off[b]:off[b + 1]].astype(np.int64) for b in range(B)]
            self.n_legs = np.diff(off).astype(np.int64)
            self.leg = np.zeros(B, dtype=np.int32)
            self.leg_at = np.full((B, int(self.n_legs.max())), -1, dtype=np.int32)
            self.route_of = self.route_of.copy()
        self.crowd = crowd
        self._Mc = 0 if crowd is None else crowd.slots                        # the peers' slots follow the crowd's
        if crowd is not None:
            self._crowd_obs, self._crowd_sinus = crowd.checked(B, self.K, cfg.Ndynobs, 0 if peers is None else peers.slots)
            self._crowd_tab = None                                            # [D, N, 5] as the last step wrote it
            self.crowd_seen = np.full((B, crowd.slots), -1, dtype=np.int32)   # the obstacle in slot K + m of robot b's p (-1: none)
            self._crowd_rec = no_crowd_clearance(B)
            if crowd.cell is not None:
                self.crowd_grid = crowd_grid(self._crowd_obs, cfg.N_hor, crowd.cell)      # filed anew every step with an active robot
                self.crowd_looked = np.zeros(B, dtype=np.int32)               # the filed entries in each robot's windows at its last step
        self.peers = peers
        if peers is not None:
            g = peers.checked(B, self.K + self._Mc, cfg.Ndynobs)
            g = np.zeros(B, dtype=np.int32) if g is None else g
            self.group_of = g
            self.groups = [np.nonzero(g == v)[0] for v in np.unique(g)]       # members in ascending robot index
        self.steps = 0
        if retire:
            self.active = np.ones(B, dtype=bool)
            self.retired_at = np.full(B, -1, dtype=np.int32)
            self.P = np.zeros((B, cfg.n_p))                                   # a retired robot's row: of its last step
            self.status = None                                                # [B], made by the first solve (its dtype is the solver's)
        self.monitor = monitor
        if monitor is not None:
            g = monitor.checked(B)
            g = np.zeros(B, dtype=np.int32) if g is None else g
            self.monitor_groups = [np.nonzero(g == v)[0] for v in np.unique(g)]   # members in ascending robot index
            self.clearance = no_clearance(B)
        self.map_monitor = map_monitor
        if map_monitor is not None:
            map_monitor.checked()
            self.map_clearance = no_map_clearance(B)
            if map_monitor.cell is not None:
                self.map_looked = np.zeros(B, dtype=np.int32)                 # the distinct edges of W(r) over the rows of each robot's last step
        self.log = log
        if log is not None:
            self._ctrl, self._rec, self._tot = [], [], []                     # per step: [s, B, 2], [B], one record
            self.drive_summary = no_drive_summary(B)
        self.plant = plant
        if plant is not None:
            self._act_gain, self._act_add, self._proc, self._meas, ids = plant.checked(B)
            self._ids = np.arange(B, dtype=np.uint32) if ids is None else ids
            self._told = self.state.copy()                                    # [B, 3]: the measured poses, the start states at first
            self._applied = []                                                # per trajectory row: [B, 2]
        self.ensemble = ensemble
        if ensemble is not None:
            g, self._ens_G = ensemble.checked(B)
            g = np.zeros(B, dtype=np.int32) if g is None else g
            self._ens_members = [(int(v), np.nonzero(g == v)[0]) for v in np.unique(g)]      # members in ascending robot index
            self._ens = []                                                    # per step: [G] records
        self.walls = walls
        if walls is not None:
            self._wall_edges = walls.checked(cfg, self.routes)
            self.wall_edge = np.full((B, walls.slots), -1, dtype=np.int32)    # the edge in circle slot Nobs - slots + m of robot b's p (-1: none)
            self.wall_stage = np.full((B, walls.slots), -1, dtype=np.int32)   # the stage at which it came closest
            if walls.cell is not None:
                self.wall_grid = wall_grid(self._wall_edges, walls.cell)
                self.wall_looked = np.zeros(B, dtype=np.int32)                # the distinct edges each robot measured at its last step
        self.track = track
        if track is not None:
            track.checked()
            self._track_tab = TrackMonitor.table(self.routes)
            self._track_rec = no_tracking(B)

    def tracking(self):
        """-> the track monitor's records [B] (``_lib.TRACKING_DTYPE``), a copy; needs a ``track``."""
        if self.track is None:
            raise ValueError("the fleet has no track monitor (track=TrackMonitor(...))")
        return self._track_rec.copy()

    def step(self, solve_fn):
        out = super().step(solve_fn)
        if self.ensemble is not None:
            self._ensemble_update()
        return out

    def _ensemble_update(self):
        """The ensemble's rule at the end of a step, for every group with a member: unfused f64, the sums by
        ``ensemble_sum``, each product rounded before it enters the tree, and a furthest member that a false comparison (a NaN)
        leaves alone; the members ascend, so the first largest r2 is the smallest robot index."""
        rec = no_ensemble_stats(1, self._ens_G)[0]
        arrived = self.done != 0 if self.active is None else self.retired_at >= 0
        with np.errstate(all="ignore"):
            for g, mem in self._ens_members:
                n, pose = len(mem), self.state[mem]
                mean = ensemble_sum(pose) / float(n)
                d = pose - mean
                dx, dy, dth = d[:, 0], d[:, 1], d[:, 2]
                prod = np.stack([dx * dx, dx * dy, dy * dy, dth * dth], axis=1)
                rec["n"][g], rec["arrived"][g] = n, int(arrived[mem].sum())
                rec["mean"][g], rec["cov"][g] = mean, ensemble_sum(prod) / float(n)
                r2 = prod[:, 0] + prod[:, 2]
                seen = ~np.isnan(r2)
                if seen.any():
                    k = int(np.argmax(np.where(seen, r2, -1.0)))
                    rec["far2"][g], rec["far_robot"][g] = r2[k], mem[k]
        self._ens.append(rec)

    def ensemble_stats(self):
        """-> [steps, G] (``_lib.ENSEMBLE_DTYPE``): every group's record after every step taken; no steps without an ``ensemble``."""
        return np.stack(self._ens) if self.ensemble is not None and self._ens else no_ensemble_stats(0, getattr(self, "_ens_G", 1))

    @property
    def controls(self):
        """-> [steps * s, B, 2]: the (v, omega) applied between trajectory rows c and c + 1; +0.0 where a robot was not driven."""
        return np.concatenate(self._ctrl) if self._ctrl else np.zeros((0, self.B, 2))

    @property
    def step_records(self):
        return np.stack(self._rec) if self._rec else no_step_records(0, self.B)

    @property
    def step_totals(self):
        return np.concatenate(self._tot) if self._tot else no_step_totals(0)

    @property
    def n_active(self):
        return self.B if self.active is None else int(self.active.sum())

    def retire(self):
        """After an advance: the active robots that are done leave; with missions, those with another leg start it instead."""
        now = self.active & self.done
        if self.missions is not None:
            self.leg_at[now, self.leg[now]] = self.steps
            go = now & (self.leg + 1 < self.n_legs)
            if go.any():
                self.leg[go] += 1
                self.route_of[go] = [self.legs[b][self.leg[b]] for b in np.nonzero(go)[0]]
                self.U[go], self.Y[go] = 0.0, 0.0
                self.last_u[go], self.idx[go], self.done[go] = 0.0, 0, False
            now = now & ~go
        self.retired_at[now] = self.steps
        self.active &= ~now

    def assemble(self):
        """With a plant that measures, everything below -- the parameter vectors and the predictions of crowd and peers -- starts
        from the measured poses: they stand in ``state`` for the length of the call."""
        if self.plant is None or not (self._meas > 0).any():
            return self._assemble()
        true = self.state
        self.state = self._measure()
        try:
            return self._assemble()
        finally:
            self.state = true

    def _measure(self):
        """The measurement rule for the active robots, m = the row of the pose measured -> what the step is
        told [B, 3]: a retired robot's true pose (its row of ``measured()`` stays its last measurement)."""
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        m = self.steps * self.cfg.num_steps_taken
        told = self.state.copy()
        for c in range(3):
            if self._meas[c] != 0:
                told[who, c] = self.state[who, c] + self._meas[c] * plant_xi(self.plant.seed, self._ids[who], m, 5 + c)
        self._told[who] = told[who]
        return told

    def measured(self):
        """-> [B, 3]: what the last step's solves were given as poses (``nmpc_loop_plant_measured``): the measured poses where the plant
        has a ``meas`` > 0 (a retired robot's: of its last step), else columns 0 .. 2 of the parameter vectors; the start states before
        the first step."""
        if self.plant is not None and (self._meas > 0).any():
            return self._told.copy()
        return self._P_step[:, 0:3].copy() if self.steps else self.state.copy()

    def applied(self):
        """-> [steps * s, B, 2]: the controls that acted, +0.0 where a robot was not driven; no rows without ``plant.keep_applied``."""
        if self.plant is None or not self.plant.keep_applied or not self._applied:
            return np.zeros((0, self.B, 2))
        return np.stack(self._applied)

    def _assemble(self):
        P = super().assemble(self.active)
        if self.active is not None:                                          # a retired robot's row stays its last step's
            self.P[self.active] = P[self.active]
            P = self.P
        if self.crowd is not None:
            self._crowd_advance()
            self._overlay_crowd(P)
        if self.peers is not None:
            self._overlay_peers(P)
        if self.walls is not None:
            self._overlay_walls(P)
        self._P_step = P                                                     # what this step's solve reads: the monitor's p
        return P

    def _overlay_walls(self, P):
        """The walls' rule on the parameter vectors of the active robots, in place.  Per edge and stage the map
        monitor's wall distance (``MapMonitor.rows``) against the predicted positions; D(e) = the smallest over the stages, taken on a
        strict ``<`` in ascending stage (a NaN never lowers it, the first of equal stages stays), with that stage and its closest point;
        the candidates D < range^2 walked in (D, e) order, one skipped if its point lies closer than ``spacing`` to a point already
        taken, until ``slots`` are taken; the m-th over circle slot Nobs - slots + m as (cx, cy, radius)."""
        cfg, wl, edges = self.cfg, self.walls, self._wall_edges
        N, M, E = cfg.N_hor, wl.slots, len(edges)
        base = cfg.n_p - cfg.nx * N - cfg.Ndynobs * cfg.ndynobs * N - cfg.Nobs * cfg.nobs + (cfg.Nobs - M) * cfg.nobs
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        if not len(who):
            return
        pred = self.predict()
        if wl.cell is not None:                                              # the results below are the all-edges rule's: the grid only counts
            self.wall_looked[who] = [len(self.wall_grid.looks_at(pred[b], wl.range)) for b in who]
        r2, s2 = wl.range * wl.range, wl.spacing * wl.spacing
        x1, y1, x2, y2 = (edges[:, k][None, :] for k in range(4))
        self.wall_edge[who], self.wall_stage[who] = -1, -1
        rows = max(1, (1 << 21) // E)                                        # robots per pass: bounds the [rows, E] tables
        for r0 in range(0, len(who), rows):
            me = who[r0:r0 + rows]
            n, at = len(me), np.arange(len(me))
            D, ks = np.full((n, E), np.inf), np.full((n, E), -1, dtype=np.int32)
            CX, CY = np.zeros((n, E)), np.zeros((n, E))
            with np.errstate(invalid="ignore"):
                for k in range(N):                                           # min over the stages, in order
                    v, cx, cy = segment_closest(pred[me, k, 0][:, None], pred[me, k, 1][:, None], x1, y1, x2, y2)
                    lower = v < D
                    D, ks = np.where(lower, v, D), np.where(lower, np.int32(k), ks)
                    CX, CY = np.where(lower, cx, CX), np.where(lower, cy, CY)
                ok = D < r2
            order = np.argsort(np.where(ok, D, np.inf), axis=1, kind="stable")       # (D, e)
            ncand = ok.sum(axis=1)
            taken = np.zeros(n, dtype=np.int64)
            tx, ty = np.full((n, M), np.nan), np.full((n, M), np.nan)        # the centres taken (a NaN: not yet, nothing is close to it)
            for r in range(int(ncand.max()) if n else 0):
                live = (r < ncand) & (taken < M)
                if not live.any():
                    break
                e = order[:, r]
                cx, cy = CX[at, e], CY[at, e]
                with np.errstate(invalid="ignore"):
                    ddx, ddy = cx[:, None] - tx, cy[:, None] - ty
                    close = (ddx * ddx + ddy * ddy < s2).any(axis=1)
                take = live & ~close
                i, m = at[take], taken[take]
                b = me[i]
                tx[i, m], ty[i, m] = cx[i], cy[i]
                self.wall_edge[b, m], self.wall_stage[b, m] = e[i], ks[i, e[i]]
                col = base + m * cfg.nobs
                P[b, col], P[b, col + 1], P[b, col + 2] = cx[i], cy[i], wl.radius
                taken[take] += 1

    def crowd_table(self):
        """-> [D, N, 5]: every obstacle of the crowd over the horizon as the last step wrote it (a step taken)."""
        return self._crowd_tab

    def crowd_clearance(self):
        """-> the crowd observer's records [B] (``_lib.CROWD_CLEARANCE_DTYPE``); without ``watch`` the initial record everywhere."""
        return self._crowd_rec if self.crowd is not None else no_crowd_clearance(self.B)

    def _crowd_advance(self):
        """The world's table, once per step whoever is active: all stages fresh at the first step, later every obstacle's row
        shifted by the s stages taken and its last s stages fresh -- what ``VectorizedRecedingHorizon.assemble`` does to a
        scripted slot."""
        cfg = self.cfg
        N, s = cfg.N_hor, cfg.num_steps_taken
        if self.t == 0:
            self._crowd_tab = _predict_ellipses(cfg, self.sincos, self._crowd_obs, self._crowd_sinus, 0.0, N)
        else:
            fresh = _predict_ellipses(cfg, self.sincos, self._crowd_obs, self._crowd_sinus, (self.t + N - s) * cfg.ts, s)
            self._crowd_tab = np.concatenate([self._crowd_tab[:, s:], fresh], axis=1)

    def _overlay_crowd(self, P):
        """The crowd's rule on the parameter vectors of the active robots, in place: C(b, d) = the smallest
        squared distance over the stages between b's predicted positions and obstacle d's (a NaN never lowers it), the first
        ``slots`` of the obstacles with C < range^2 in (C, d) order, each one's row of the table over one ellipse slot."""
        cfg, cr, tab = self.cfg, self.crowd, self._crowd_tab
        N, M, D = cfg.N_hor, cr.slots, len(tab)
        per = cfg.ndynobs * N
        base = cfg.n_p - cfg.nx * N - cfg.Ndynobs * per + self.K * per       # slot K of the dynamic block
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        self.crowd_who = who                                                 # whom this step's selection ran for
        if not len(who):
            return
        self.crowd_pred = pred = self.predict()                              # what it read
        r2 = cr.range * cr.range
        self.crowd_seen[who] = -1
        if cr.cell is not None:
            self._overlay_crowd_grid(P, pred, who, base, per, r2)
            return
        rows = max(1, (1 << 22) // D)                                       # robots per pass: bounds the [rows, D] tables
        for r0 in range(0, len(who), rows):
            me = who[r0:r0 + rows]
            C = np.full((len(me), D), np.inf)
            with np.errstate(invalid="ignore", over="ignore"):
                for k in range(N):                                           # min over the stages, in order
                    dx, dy = pred[me, None, k, 0] - tab[None, :, k, 0], pred[me, None, k, 1] - tab[None, :, k, 1]
                    d = dx * dx + dy * dy
                    C = np.where(d < C, d, C)
                ok = C < r2
            order = np.argsort(np.where(ok, C, np.inf), axis=1, kind="stable")       # (C, d)
            for m in range(min(M, D)):
                j = order[:, m]
                got = ok[np.arange(len(me)), j]
                b, src = me[got], j[got]
                self.crowd_seen[b, m] = src
                P[b, base + m * per:base + (m + 1) * per] = tab[src].reshape(len(b), per)

    def _overlay_crowd_grid(self, P, pred, who, base, per, r2):
        """``_overlay_crowd`` with C formed through ``crowd_grid`` only: this step's table is filed, and robot
        by robot an entry (d, k) of its windows makes d a candidate if d_k < range^2 and no earlier stage has d_j < range^2, with C
        over all stages as the all-obstacles rule forms it; the same (C, d) order and overlay."""
        cr, tab, grid = self.crowd, self._crowd_tab, self.crowd_grid
        grid.file(tab)
        for b in who:
            d, k = grid.candidates(pred[b], cr.range)
            self.crowd_looked[b] = len(d)
            if not len(d):
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy = pred[b, k, 0] - tab[d, k, 0], pred[b, k, 1] - tab[d, k, 1]
                near = dx * dx + dy * dy < r2
                d, k = d[near], k[near]
                dx, dy = pred[b][None, :, 0] - tab[d, :, 0], pred[b][None, :, 1] - tab[d, :, 1]
                dd = dx * dx + dy * dy                                        # [n, N]
                first = np.argmax(dd < r2, axis=1) == k                       # the entry's stage is d's first in range
            d, dd = d[first], dd[first]
            C = np.where(np.isnan(dd), np.inf, dd).min(axis=1)                # min over the stages, a NaN passed over
            for m, src in enumerate(d[np.lexsort((d, C))][:cr.slots]):        # (C, d)
                self.crowd_seen[b, m] = src
                P[b, base + m * per:base + (m + 1) * per] = tab[src].reshape(per)

    def _crowd_update(self):
        """The crowd observer's rule on the s rows this step appended, for the robots it drove: row
        ``first + i`` against entry i of every obstacle's row of this step's table.  Rows ascend and ``argmin`` names the first
        obstacle, so a strictly smaller level is the only way to win; a NaN level is passed over."""
        s, rec, tab = self.cfg.num_steps_taken, self._crowd_rec, self._crowd_tab
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        if not len(who):
            return
        for i in range(s):
            r = self.steps * s + 1 + i
            pose = self.traj[len(self.traj) - s + i]
            e = tab[:, i, :]                                                 # [D, 5]
            with np.errstate(all="ignore"):
                dx, dy = pose[who, None, 0] - e[None, :, 0], pose[who, None, 1] - e[None, :, 1]
                sn, cs = self.sincos(np.ascontiguousarray(e[:, 4]))
                a, c = dx * cs + dy * sn, dx * sn - dy * cs
                v = (a * a) / (e[:, 2] * e[:, 2]) + (c * c) / (e[:, 3] * e[:, 3])
            v = np.where(np.isnan(v), np.inf, v)
            d = np.argmin(v, axis=1)
            v = v[np.arange(len(who)), d]
            better = v < rec["level"][who]
            b = who[better]
            rec["level"][b], rec["row"][b], rec["obstacle"][b] = v[better], r, d[better]

    def predict(self):
        """-> pred [B, N, 3]: pred[j, k] = robot j's pose after k + 1 Euler steps (the expression of ``advance``) from
        its state, under its previous plan shifted by the controls already applied: control k is U[j, s + k], and
        the plan's last control beyond its end.  A retired robot is parked: pred[j, k] = its state, a copy."""
        cfg = self.cfg
        N, s, nu = cfg.N_hor, cfg.num_steps_taken, cfg.nu
        st = self.state
        x, y, th = st[:, 0], st[:, 1], st[:, 2]
        pred = np.empty((self.B, N, 3))
        for k in range(N):
            c = min(s + k, N - 1)
            v, w = self.U[:, c * nu], self.U[:, 1 + c * nu]
            sn, cs = self.sincos(np.ascontiguousarray(th))
            x, y, th = x + cfg.ts * (v * cs), y + cfg.ts * (v * sn), th + cfg.ts * w
            pred[:, k, 0], pred[:, k, 1], pred[:, k, 2] = x, y, th
        if self.active is not None:
            pred[~self.active] = st[~self.active, None, :]
        return pred

    def _overlay_peers(self, P):
        """The peers rule on the parameter vectors, in place."""
        cfg, pe = self.cfg, self.peers
        N, M = cfg.N_hor, pe.slots
        per = cfg.ndynobs * N
        base = cfg.n_p - cfg.nx * N - cfg.Ndynobs * per + (self.K + self._Mc) * per      # the peers' first slot: behind the crowd's
        pred = self.predict()
        r2 = pe.range * pe.range
        self.peer_index = np.full((self.B, M), -1)                           # who fills slot K + m of robot b at this step (-1: nobody)
        if pe.cell is not None:
            self._overlay_peers_grid(P, pred, base, per, r2)
            return
        for mem in self.groups:
            G = len(mem)
            if G < 2:
                continue
            px, py = pred[mem, :, 0], pred[mem, :, 1]                        # [G, N]
            rows = max(1, (1 << 22) // G)                                    # robots of the group per pass: bounds the [rows, G] tables
            for r0 in range(0, G, rows):
                me = np.arange(r0, min(G, r0 + rows))
                D = np.full((len(me), G), np.inf)
                for k in range(N):                                           # min over the stages, in order
                    dx, dy = px[me, None, k] - px[None, :, k], py[me, None, k] - py[None, :, k]
                    d = dx * dx + dy * dy
                    D = np.where(d < D, d, D)
                ok = D < r2
                ok[np.arange(len(me)), me] = False                           # not oneself
                order = np.argsort(np.where(ok, D, np.inf), axis=1, kind="stable")   # (D, j): members are in ascending j
                for m in range(min(M, G - 1)):
                    j = order[:, m]
                    got = ok[np.arange(len(me)), j]
                    if self.active is not None:
                        got &= self.active[mem[me]]                          # a retired robot's p is not touched
                    b, src = mem[me[got]], mem[j[got]]
                    blk = np.empty((len(b), N, cfg.ndynobs))
                    blk[..., 0], blk[..., 1], blk[..., 4] = pred[src, :, 0], pred[src, :, 1], pred[src, :, 2]
                    blk[..., 2], blk[..., 3] = pe.rx, pe.ry
                    self.peer_index[b, m] = src
                    P[b, base + m * per:base + (m + 1) * per] = blk.reshape(len(b), per)

    def _overlay_peers_grid(self, P, pred, base, per, r2):
        """``_overlay_peers`` with D formed over ``peer_grid(...).candidates`` only: robot by robot, the same closeness, (D, j)
        order and overlay."""
        cfg, pe = self.cfg, self.peers
        N, M = cfg.N_hor, pe.slots
        self.grid = grid = peer_grid(pred, pe.range, pe.cell)
        px, py = pred[:, :, 0], pred[:, :, 1]
        for b in range(self.B):
            if self.active is not None and not self.active[b]:                # a retired robot's p is not touched
                continue
            c = grid.candidates(b)
            c = c[(c != b) & (self.group_of[c] == self.group_of[b])]
            if not len(c):
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy = px[b][None, :] - px[c], py[b][None, :] - py[c]
                d = dx * dx + dy * dy                                         # [C, N]
            D = np.where(np.isnan(d), np.inf, d).min(axis=1)                  # min over the stages, a NaN passed over
            c, D = c[D < r2], D[D < r2]
            for m, j in enumerate(c[np.lexsort((c, D))][:M]):                 # (D, j)
                blk = np.empty((N, cfg.ndynobs))
                blk[:, 0], blk[:, 1], blk[:, 4] = pred[j, :, 0], pred[j, :, 1], pred[j, :, 2]
                blk[:, 2], blk[:, 3] = pe.rx, pe.ry
                self.peer_index[b, m] = j
                P[b, base + m * per:base + (m + 1) * per] = blk.reshape(per)

    def _plant_advance(self, U):
        """``VectorizedRecedingHorizon.advance`` with the plant rule in the place of its Euler step: unfused, in
        the rule's order; a statement whose sigmas are 0 is skipped, so a plant of zeros is that advance.  Draws are pure functions of
        (seed, id, row, channel): taken for everybody, kept for the active."""
        cfg, active, seed, ids = self.cfg, self.active, self.plant.seed, self._ids
        s, gain, add, proc = cfg.num_steps_taken, self._act_gain, self._act_add, self._proc
        st = self.state.copy()
        for i in range(s):
            r = self.steps * s + 1 + i
            va, wa = U[:, i * cfg.nu], U[:, 1 + i * cfg.nu]
            if gain[0] != 0 or add[0] != 0:
                t = gain[0] * va
                t = t + add[0]
                va = va + t * plant_xi(seed, ids, r, 0)
            if gain[1] != 0 or add[1] != 0:
                t = gain[1] * wa
                t = t + add[1]
                wa = wa + t * plant_xi(seed, ids, r, 1)
            th = st[:, 2]
            sn, cs = self.sincos(np.ascontiguousarray(th))
            x, y, tn = st[:, 0] + cfg.ts * (va * cs), st[:, 1] + cfg.ts * (va * sn), th + cfg.ts * wa
            if proc[0] != 0:
                x = x + proc[0] * plant_xi(seed, ids, r, 2)
            if proc[1] != 0:
                y = y + proc[1] * plant_xi(seed, ids, r, 3)
            if proc[2] != 0:
                tn = tn + proc[2] * plant_xi(seed, ids, r, 4)
            new, acted = np.stack([x, y, tn], axis=1), np.stack([va, wa], axis=1)
            st = new if active is None else np.where(active[:, None], new, st)
            self.traj.append(st.copy())
            self._applied.append(acted if active is None else np.where(active[:, None], acted, 0.0))
        self.state = st
        last_u = U[:, (s - 1) * cfg.nu:s * cfg.nu].copy()                     # the commanded control: what the controller knows it sent
        self.last_u = last_u if active is None else np.where(active[:, None], last_u, self.last_u)
        end = self.tab.end[self.route_of]
        done = (np.abs(st[:, 0] - end[:, 0]) <= 0.05) & (np.abs(st[:, 1] - end[:, 1]) <= 0.05) & (np.abs(self.last_u[:, 0]) < 0.005)
        self.done = done if active is None else np.where(active, done, self.done)
        self.t += s

    def advance(self, U):
        if self.plant is None:
            super().advance(U, self.active)
        else:
            self._plant_advance(U)
        if self.monitor is not None:
            self._monitor_update()
        if self.map_monitor is not None:
            self._map_update()
        if self.crowd is not None and self.crowd.watch:
            self._crowd_update()
        if self.track is not None:
            self._track_update()
        if self.log is not None:
            self._log_update(U)
        self.steps += 1

    def _log_update(self, U):
        """The drive log's rule for the robots this step drove (``active`` as the step found it: ``retire``
        comes after, so ``leg`` is the leg the solve belonged to).  Unfused f64, sequential sums, and maxima that a false comparison
        (a NaN) leaves alone."""
        cfg, B, st, P = self.cfg, self.B, self._st_step, self._P_step
        s, nu, step = cfg.num_steps_taken, cfg.nu, self.steps + 1
        drove = np.ones(B, dtype=bool) if self.active is None else self.active.copy()
        who = np.nonzero(drove)[0]
        ctrl, rec, tot = np.zeros((s, B, 2)), no_step_records(1, B)[0], no_step_totals(1)
        self._ctrl.append(ctrl)
        self._rec.append(rec)
        self._tot.append(tot)
        if not len(who):
            return
        st = st[who]
        ctrl[:, who] = U[who, :s * nu].reshape(len(who), s, nu).transpose(1, 0, 2)
        for f in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "f2_norm", "solve_time_ms"):
            rec[f][who] = st[f]
        rec["leg"][who] = self.leg[who] if self.missions is not None else 0
        m = self.drive_summary
        m["steps"][who] += 1
        m["rows"][who] += s
        e, inner, f2 = st["exit_status"], st["num_inner_iterations"], st["f2_norm"]
        ok = (e >= 0) & (e < 5)
        np.add.at(m["exits"], (who[ok], e[ok]), 1)
        m["inner_total"][who] += inner.astype(np.uint64)

        def raise_to(field, x, at=None):
            """``if (x > m) m = x`` on the robots driven, with the step where ``at`` names a field"""
            b = who[x > m[field][who]]
            m[field][b] = x[x > m[field][who]]
            if at is not None:
                m[at][b] = step

        raise_to("inner_max", inner, "inner_max_step")
        raise_to("f2_max", f2, "f2_max_step")
        vp, wp = P[who, 3], P[who, 4]
        with np.errstate(all="ignore"):
            for i in range(s):
                a, b = self.traj[len(self.traj) - s - 1 + i][who], self.traj[len(self.traj) - s + i][who]
                dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
                m["length"][who] = m["length"][who] + np.sqrt(dx * dx + dy * dy)
                v, w = U[who, i * nu], U[who, i * nu + 1]
                raise_to("v_abs_max", np.abs(v))
                raise_to("w_abs_max", np.abs(w))
                acc, wacc = (v - vp) / cfg.ts, (w - wp) / cfg.ts
                raise_to("acc_abs_max", np.abs(acc))
                raise_to("wacc_abs_max", np.abs(wacc))
                m["acc_sq_sum"][who] = m["acc_sq_sum"][who] + acc * acc
                m["wacc_sq_sum"][who] = m["wacc_sq_sum"][who] + wacc * wacc
                vp, wp = v, w
        tot["solved"] = len(who)
        tot["exits"] = np.bincount(e[ok], minlength=5)
        tot["inner_max"], tot["inner_max_robot"] = inner.max(), who[np.argmax(inner)]      # the first maximum: the smallest robot index
        tot["inner_total"] = inner.astype(np.uint64).sum()
        ms = st["solve_time_ms"]
        tot["solve_ms_max"] = np.where(ms > 0, ms, 0.0).max()

    def _track_update(self):
        """The track monitor's rule on the s rows this step appended, for the robots the step drove, each against
        its route as the step found it (``retire`` comes after): ``TrackMonitor.fold``, vectorised over robots and segments."""
        s = self.cfg.num_steps_taken
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        if not len(who):
            return
        for i in range(s):
            pose = self.traj[len(self.traj) - s + i]
            self.track.fold(self._track_rec, who, self.steps * s + 1 + i, self._track_tab, self.route_of[who], pose[who])

    def _map_update(self):
        """The map monitor's rule on the s rows this step appended, each against the row before it, for the robots
        the step drove.  The rows ascend, so a strictly smaller value is the only way to win, and ``rows`` names the first edge."""
        s, rec = self.cfg.num_steps_taken, self.map_clearance
        who = np.arange(self.B) if self.active is None else np.nonzero(self.active)[0]
        if not len(who):
            return
        grid = self.map_monitor.cell is not None
        if grid:
            self.map_looked[who] = 0
        for i in range(s):
            r = self.steps * s + 1 + i
            at = len(self.traj) - s + i
            pose, prev = self.traj[at], self.traj[at - 1]
            if grid:
                v, e, poly, looked = self.map_monitor.rows_grid(prev[who, 0], prev[who, 1], pose[who, 0], pose[who, 1])
                self.map_looked[who] += looked
            else:
                v, e, poly = self.map_monitor.rows(prev[who, 0], prev[who, 1], pose[who, 0], pose[who, 1])
            b, better = who, v < rec["wall2"][who]
            rec["wall2"][b[better]], rec["wall_row"][b[better]], rec["wall_edge"][b[better]] = v[better], r, e[better]
            hit = poly >= 0
            first = hit & (rec["hits"][who] == 0)
            rec["hit_row"][b[first]], rec["hit_poly"][b[first]] = r, poly[first]
            rec["hits"][b[hit]] += 1

    def _monitor_update(self):
        """The monitor's rule on the s rows this step appended, for the robots it drove (``active`` as the
        step found it: ``retire`` comes after).  The rows ascend, so inside a step a strictly smaller value is the only way to win;
        within a row the first minimum over the group's members, who are in ascending index, is the smallest robot index."""
        cfg, rec, P = self.cfg, self.clearance, self._P_step
        B, N, s, K = self.B, cfg.N_hor, cfg.num_steps_taken, self.K
        drove = np.ones(B, dtype=bool) if self.active is None else self.active
        if not drove.any():
            return
        pcirc = 20 + N
        pdyn = pcirc + cfg.nobs * cfg.Nobs
        circ = P[:, pcirc:pdyn].reshape(B, cfg.Nobs, cfg.nobs)
        dyn = P[:, pdyn:pdyn + cfg.Ndynobs * N * cfg.ndynobs].reshape(B, cfg.Ndynobs, N, cfg.ndynobs)

        def lowest(v, seen):
            """-> per robot the smallest value among the seen ones that are not NaN, +inf without any"""
            return np.where(seen & ~np.isnan(v), v, np.inf).min(axis=1, initial=np.inf)

        def take(better, value, row, fields):
            better = better & drove
            rec[fields[0]][better] = value[better]
            rec[fields[1]][better] = row

        for i in range(s):
            r = self.steps * s + 1 + i
            pose = self.traj[len(self.traj) - s + i]
            x, y = pose[:, 0], pose[:, 1]
            dx, dy = x[:, None] - circ[..., 0], y[:, None] - circ[..., 1]
            v = lowest(np.sqrt(dx * dx + dy * dy) - circ[..., 2], circ[..., 2] > 0)
            take(v < rec["circle"], v, r, ("circle", "circle_row"))
            if K:
                e = dyn[:, :K, i, :]
                dx, dy = x[:, None] - e[..., 0], y[:, None] - e[..., 1]
                sn, cs = self.sincos(np.ascontiguousarray(e[..., 4]))
                a, c = dx * cs + dy * sn, dx * sn - dy * cs
                v = lowest((a * a) / (e[..., 2] * e[..., 2]) + (c * c) / (e[..., 3] * e[..., 3]), np.ones((B, K), dtype=bool))
                take(v < rec["ellipse"], v, r, ("ellipse", "ellipse_row"))
            for mem in self.monitor_groups:
                G = len(mem)
                if G < 2:
                    continue
                gx, gy = x[mem], y[mem]
                rows = max(1, (1 << 22) // G)                                # robots of the group per pass: bounds the [rows, G] tables
                for r0 in range(0, G, rows):
                    me = np.arange(r0, min(G, r0 + rows))
                    dx, dy = gx[me, None] - gx[None, :], gy[me, None] - gy[None, :]
                    d = dx * dx + dy * dy
                    d = np.where(np.isnan(d), np.inf, d)
                    d[np.arange(len(me)), me] = np.inf                       # not oneself
                    j = np.argmin(d, axis=1)
                    v = d[np.arange(len(me)), j]
                    better = (v < rec["peer2"][mem[me]]) & drove[mem[me]]
                    b = mem[me[better]]
                    rec["peer2"][b], rec["peer_row"][b], rec["peer"][b] = v[better], r, mem[j[better]]


def _fill_route(r, route: harness.Route, keep: list):
    """Fill the ``nmpc_route`` struct ``r`` from ``route``; the arrays it points to are appended to ``keep``,
    which must outlive the call that reads the struct."""
    cfg = route.cfg

    def arr(v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        return _lib.as_dp(a)
    vert = np.array(route.vertices, dtype=np.float64).reshape(-1, 2)
    r.n_ref, r.n_vert, r.n_brake = len(route.x_ref), len(vert), len(route.brake_velocities)
    r.num_steps_taken = cfg.num_steps_taken
    r.x_ref, r.y_ref, r.theta_ref = arr(route.x_ref), arr(route.y_ref), arr(route.theta_ref)
    r.vert_xy = arr(vert) if len(vert) else None
    r.brake_vel, r.brake_dist = arr(route.brake_velocities), arr(route.brake_distances)
    r.end = (C.c_double * 3)(*[float(v) for v in route.end])
    r.base_speed, r.radius = float(route.base_speed), float(route.radius)
    r.dyn_pad = cfg.vehicle_width / 2 + cfg.vehicle_margin
    r.weights = (C.c_double * 10)(*cfg.weights())


class DeviceRecedingHorizon:
    """``VectorizedRecedingHorizon`` with everything on the GPU: parameter assembly, the batched solve
    and the state advance are kernels of libnmpc_hip.so (``nmpc_loop_*``, include/nmpc_solver.h), and
    nothing crosses PCIe between steps.  Same quantities, same order of operations as the host class;
    sin / cos are the kernels' own (tests/test_gpu_loop.py compares bit for bit against the host class
    given the same sin / cos).

    ``solver`` is the ``BatchSolver`` whose handle runs the solves; ``dyn_obs`` as in
    ``VectorizedRecedingHorizon``; ``max_steps`` > 0 records the trajectory on device; ``idx0`` = the
    reference sample each robot starts at (default 0, as the reference).

    ``route`` is one ``harness.Route`` (``nmpc_loop_new``), or a sequence of R routes with ``route_of`` [B]:
    robot b follows ``route[route_of[b]]`` and ``idx0[b]`` counts on that route (``nmpc_loop_new_routes``;
    ``route_of`` may be omitted for a single route).  Its host mirror is ``FleetRecedingHorizon``
    (tests/test_gpu_fleet_loop.py).

    Wall-clock limits are the handle's: on a ``solver`` with ``batch_budget_ms`` (``BatchSolver.set_time_limits``) every
    step's solve gets that budget from the start of its launch on the device, so a fleet can be re-planned within a control
    period; ``max_duration_ms`` bounds each robot's solve the same way.  Instances the clock stops answer
    ``NotConvergedOutOfTime`` with the feasible half step, and the next step warm-starts from it as from any other solve.

    ``peers`` (a ``Peers``): the robots of a group see each other (``nmpc_loop_set_peers``); two more
    kernels per step, between the assembly and the solve.  Its host mirror is ``FleetRecedingHorizon`` with the same ``peers``
    (tests/test_gpu_peers_loop.py).  With ``peers.cell`` the candidates come from a grid built on the device every step
    (``nmpc_loop_set_peers_grid``): the same results, ``peer_grid()`` reads the last step's grid (tests/test_gpu_peers_grid_loop.py).

    ``monitor`` (a ``Monitor``, needs ``max_steps`` > 0): every robot's closest approach to circles, scripted ellipses and the robots
    of its monitor group is kept on the device (``nmpc_loop_set_monitor``), one more kernel per step after the
    advance; ``clearance()`` reads the records.  Its host mirror is ``FleetRecedingHorizon`` with the same ``monitor``
    (tests/test_gpu_monitor_loop.py).

    ``retire=True``: robots that reach their goal leave the loop (``nmpc_loop_set_retire``); every step solves
    the active robots only, ``active()`` tells who is left and ``run(max_steps)`` steps until nobody is.  ``step`` then waits for the
    step before to have counted its active robots (an event, not the device).  Its host mirror is ``FleetRecedingHorizon`` with
    ``retire=True`` (tests/test_gpu_retire_loop.py).

    ``map_monitor`` (a ``MapMonitor``, needs ``max_steps`` > 0): every robot's closest approach to the walls of a polygon map, and the rows
    at which it was inside an obstacle, outside the boundary or went through an edge, are kept on the device
    (``nmpc_loop_set_map_monitor``), one more kernel per step after the advance; ``map_clearance()`` reads the
    records.  Its host mirror is ``FleetRecedingHorizon`` with the same ``map_monitor`` (tests/test_gpu_map_monitor_loop.py).  A
    ``MapMonitor`` with a ``cell`` finds the edges through the walls grid (``nmpc_loop_set_map_monitor_grid``,
    ``nmpc_loop_map_grid_kernel``): up to 1048576 edges, ``map_grid()`` reads the grid and the edges each robot looked at
    (tests/test_gpu_map_grid_loop.py).

    ``missions`` (a ``Missions``, needs ``retire=True``): every robot drives the routes of its mission leg after leg and retires after
    the last (``nmpc_loop_set_missions``); one more kernel per step, before the active list is rebuilt.
    ``legs()`` tells where everybody is.  Its host mirror is ``FleetRecedingHorizon`` with the same ``missions``
    (tests/test_gpu_missions_loop.py).

    ``log`` (a ``DriveLog``, needs ``max_steps`` > 0): the controls every robot applied, a record of every solve, a summary per robot and
    the fleet's totals per step are kept on the device (``nmpc_loop_set_log``), two more kernels per step after
    the advance; ``controls()``, ``step_records()``, ``drive_summary()`` and ``step_totals()`` read them.  Its host mirror is
    ``FleetRecedingHorizon`` with the same ``log`` (tests/test_gpu_log_loop.py).

    ``crowd`` (a ``Crowd``): D moving obstacles of the world, one table on the device advanced once per step, and every step each
    active robot's closest ones in ellipse slots of its own (``nmpc_loop_set_crowd``): two more kernels per step,
    three with ``crowd.watch`` (needs ``max_steps`` > 0).  ``crowd_table()``, ``crowd_seen()`` and ``crowd_clearance()`` read the
    results.  Its host mirror is ``FleetRecedingHorizon`` with the same ``crowd`` (tests/test_gpu_crowd_loop.py).  With ``crowd.cell``
    the obstacles are found through a grid in space and stage (``nmpc_loop_set_crowd_grid``: up to 131072 obstacles, five more kernels
    per step that file the table): the same results, ``crowd_grid()`` reads the grid and what each robot looked at
    (tests/test_gpu_crowd_grid_loop.py).

    ``plant`` (a ``Plant``): seeded actuation, process and measurement noise drawn on the device (``nmpc_loop_set_plant``, DESIGN.md
    section 5.9): ``nmpc_loop_plant_kernel`` in the place of the advance and, with a ``meas`` > 0, ``nmpc_loop_measure_kernel`` in front of
    the assembly.  ``applied()`` (with ``plant.keep_applied``, needs ``max_steps`` > 0) and ``measured()`` read the results.  Its host
    mirror is ``FleetRecedingHorizon`` with the same ``plant`` (tests/test_gpu_plant_loop.py).

    ``ensemble`` (an ``Ensemble``, needs ``max_steps`` > 0): after every step one record per group -- member count, arrivals, mean pose,
    covariance of the position, variance of the heading, the member furthest from the mean -- is kept on the device
    (``nmpc_loop_set_ensemble``): ``nmpc_loop_ensemble_kernel``, one workgroup per group, the step's last kernel.
    ``ensemble_stats()`` reads the table.  Its host mirror is ``FleetRecedingHorizon`` with the same ``ensemble``
    (tests/test_gpu_ensemble_loop.py).

    ``walls`` (a ``Walls``): every step each active robot's closest points on the map's wall segments, measured against its predicted
    poses, become circles in the last ``slots`` circle slots of its parameter vector (``nmpc_loop_set_walls``):
    ``nmpc_loop_walls_kernel``, one wave per robot, between the peers' kernels and the solve.  ``walls()`` reads the edges and stages
    chosen.  Its host mirror is ``FleetRecedingHorizon`` with the same ``walls`` (tests/test_gpu_walls_loop.py).  With ``walls.cell`` the
    edges a robot measures come from a static grid built by the setter (``nmpc_loop_set_walls_grid``, ``nmpc_loop_walls_grid_kernel``): the
    same results on up to 1048576 edges, ``wall_grid()`` reads the grid and the edges each robot looked at (tests/test_gpu_walls_grid_loop.py).

    ``track`` (a ``TrackMonitor``, needs ``max_steps`` > 0): how far every robot was from the route it was asked to follow, in position
    and (unwrapped) heading, the rows of the largest errors, its progress along the route and the rows further than ``tol`` from it are
    kept on the device (``nmpc_loop_set_track_monitor``): ``nmpc_loop_track_kernel``, one wave per robot, after the
    advance and the other monitors and before the log and the dispatch.  ``tracking()`` reads the records.  Its host mirror is
    ``FleetRecedingHorizon`` with the same ``track`` (tests/test_gpu_track_loop.py).
    """

    def __init__(self, solver, route, starts, dyn_obs=None, max_steps: int = 0, idx0=None, sinus_object=False,
                 route_of=None, peers=None, retire=False, monitor=None, missions=None, map_monitor=None, log=None, crowd=None, plant=None,
                 ensemble=None, walls=None, track=None):
        single = isinstance(route, harness.Route)
        routes = [route] if single else list(route)
        cfg = self.cfg = routes[0].cfg
        self.solver, self.lib = solver, solver.lib
        self.route = route if single else None
        self.routes = routes
        self.B = B = len(starts)
        self.t = 0
        self.steps = 0
        starts = np.ascontiguousarray(np.array(starts, dtype=np.float64).reshape(B, 3))
        K = 0 if dyn_obs is None else dyn_obs[0].shape[1]
        dyn = None
        if K:
            p1, p2, freq, rx, ry, ang = dyn_obs
            sinus = np.zeros((B, K))
            if sinus_object and K > 2:
                sinus[:, 2] = 1.0                  # obstacle index 2 follows the sinusoidal law (visibility.py:210-212)
            direction = _atan2(p2[..., 1] - p1[..., 1], p2[..., 0] - p1[..., 0])
            dyn = np.ascontiguousarray(np.concatenate(
                [p1, p2, freq[..., None], rx[..., None], ry[..., None], ang[..., None], sinus[..., None],
                 direction[..., None]], axis=2), dtype=np.float64)
            assert dyn.shape == (B, K, 10)
        keep = []                                              # arrays the structs point to, until nmpc_loop_new* returns
        rs = (_lib.NmpcRoute * len(routes))()
        for r, rt in zip(rs, routes):
            _fill_route(r, rt, keep)
        h = C.c_void_p()
        i0 = None if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int32)
        if single:
            assert route_of is None, "route_of goes with a list of routes"
            self.route_of = None
            rc = self.lib.nmpc_loop_new(solver._h, rs, B, _lib.as_dp(starts), _lib.as_i32p(i0), K, _lib.as_dp(dyn), int(max_steps), C.byref(h))
        else:
            self.route_of = None if route_of is None else np.ascontiguousarray(route_of, dtype=np.int32).reshape(B)
            rc = self.lib.nmpc_loop_new_routes(solver._h, rs, len(routes), _lib.as_i32p(self.route_of),
                                               B, _lib.as_dp(starts), _lib.as_i32p(i0), K, _lib.as_dp(dyn), int(max_steps), C.byref(h))
        solver._check(rc)
        self._l = h
        self.max_steps = int(max_steps)
        self.crowd = crowd
        if crowd is not None:
            try:
                (p1, p2, freq, rx, ry, ang), sinus = crowd.checked(B, K, cfg.Ndynobs, 0 if peers is None else peers.slots)
            except ValueError:
                self.close()
                raise
            direction = _atan2(p2[:, 1] - p1[:, 1], p2[:, 0] - p1[:, 0])
            obst = np.ascontiguousarray(np.concatenate([p1, p2, freq[:, None], rx[:, None], ry[:, None], ang[:, None],
                                                        sinus.astype(np.float64)[:, None], direction[:, None]], axis=1))
            self._crowd_D = len(obst)
            pad = cfg.vehicle_width / 2 + cfg.vehicle_margin
            if crowd.cell is None:
                self._set(self.lib.nmpc_loop_set_crowd(h, self._crowd_D, _lib.as_dp(obst), pad, int(crowd.slots), float(crowd.range)))
            else:
                self._set(self.lib.nmpc_loop_set_crowd_grid(h, self._crowd_D, _lib.as_dp(obst), pad, int(crowd.slots), float(crowd.range),
                                                            float(crowd.cell)))
            if crowd.watch:
                self._set(self.lib.nmpc_loop_set_crowd_monitor(h))
        self.peers = peers
        if peers is not None:
            g = None if peers.group_of is None else np.ascontiguousarray(peers.group_of, dtype=np.int32).reshape(B)
            if peers.cell is None:
                self._set(self.lib.nmpc_loop_set_peers(h, _lib.as_i32p(g), int(peers.slots), float(peers.rx), float(peers.ry), float(peers.range)))
            else:
                self._set(self.lib.nmpc_loop_set_peers_grid(h, _lib.as_i32p(g), int(peers.slots), float(peers.rx), float(peers.ry),
                                                            float(peers.range), float(peers.cell)))
        self.retire = bool(retire)
        if retire:
            self._set(self.lib.nmpc_loop_set_retire(h, 1))
        self.monitor = monitor
        if monitor is not None:
            g = None if monitor.group_of is None else np.ascontiguousarray(monitor.group_of, dtype=np.int32).reshape(B)
            self._set(self.lib.nmpc_loop_set_monitor(h, _lib.as_i32p(g)))
        self.map_monitor = map_monitor
        if map_monitor is not None:
            try:
                edges, off = map_monitor.checked()
            except ValueError:
                self.close()
                raise
            sc = _lib.NmpcScene(0, len(edges), len(off) - 1, 0, None, _lib.as_dp(edges), _lib.as_i32p(off))
            if map_monitor.cell is None:
                self._set(self.lib.nmpc_loop_set_map_monitor(h, C.byref(sc)))
            else:
                self._set(self.lib.nmpc_loop_set_map_monitor_grid(h, C.byref(sc), float(map_monitor.range), float(map_monitor.cell)))
        self.log = log
        if log is not None:
            self._set(self.lib.nmpc_loop_set_log(h))
        self.plant = plant
        if plant is not None:
            try:
                gain, add, proc, meas, ids = plant.checked(B)
            except ValueError:
                self.close()
                raise
            pl = _lib.NmpcPlant(int(plant.seed), (C.c_double * 2)(*gain), (C.c_double * 2)(*add), (C.c_double * 3)(*proc),
                                (C.c_double * 3)(*meas), int(bool(plant.keep_applied)), 0)
            self._set(self.lib.nmpc_loop_set_plant(h, C.byref(pl), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32))))
        self.ensemble = ensemble
        if ensemble is not None:
            try:
                g, G = ensemble.checked(B)
            except ValueError:
                self.close()
                raise
            self._set(self.lib.nmpc_loop_set_ensemble(h, _lib.as_i32p(g), G))
        self._walls = walls
        if walls is not None:
            try:
                edges = walls.checked(cfg, routes)
            except ValueError:
                self.close()
                raise
            if walls.cell is None:
                self._set(self.lib.nmpc_loop_set_walls(h, len(edges), _lib.as_dp(edges), int(walls.slots), float(walls.radius), float(walls.range),
                                                       float(walls.spacing)))
            else:
                self._set(self.lib.nmpc_loop_set_walls_grid(h, len(edges), _lib.as_dp(edges), int(walls.slots), float(walls.radius),
                                                            float(walls.range), float(walls.spacing), float(walls.cell)))
        self.track = track
        if track is not None:
            try:
                tol = track.checked()
            except ValueError:
                self.close()
                raise
            self._set(self.lib.nmpc_loop_set_track_monitor(h, tol))
        self.missions = missions
        self._leg_off = None
        if missions is not None:
            try:
                if not retire:
                    raise ValueError("missions need retire=True")
                self._leg_off, leg_route = missions.checked(B, len(routes), self.route_of)
            except ValueError:
                self.close()
                raise
            self._set(self.lib.nmpc_loop_set_missions(h, _lib.as_i32p(self._leg_off), _lib.as_i32p(leg_route)))

    def _set(self, rc):
        """A setter's answer during construction: a refusal frees the loop before it is raised."""
        if rc:
            self.close()
            self.solver._check(rc)

    def close(self):
        if getattr(self, "_l", None):
            self.lib.nmpc_loop_free(self._l)
            self._l = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, stream=None):
        """Enqueue one assemble -> solve -> advance; returns without synchronising."""
        self.solver._check(self.lib.nmpc_loop_step(self._l, stream))
        self.t += self.cfg.num_steps_taken
        self.steps += 1

    def run(self, max_steps, stream=None):
        """A retiring loop: step until nobody is active, ``max_steps`` steps are taken or the trajectory buffer is full.
        -> the number of steps taken; does not synchronise after the last."""
        n = self.lib.nmpc_loop_run(self._l, int(max_steps), stream)
        if n < 0:
            self.solver._check(n)
        self.t += n * self.cfg.num_steps_taken
        self.steps += n
        return n

    def active(self):
        """-> (n_active, retired_at [B] int32) after synchronising: the steps each retired robot took, -1 for an active one."""
        n, at = C.c_int32(), np.empty(self.B, dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_active(self._l, C.byref(n), _lib.as_i32p(at)))
        return n.value, at

    def legs(self):
        """-> (leg [B], route_of [B], leg_at [B, Lmax]) int32 after synchronising: the leg each robot is on, its current route, and the
        step count at which each of its legs ended (-1: not yet, or no such leg); without ``missions`` leg 0, the routes of the
        creation and one column of -1."""
        B, off = self.B, self._leg_off
        leg, route_of = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        flat = None if off is None else np.empty(int(off[-1]), dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_legs(self._l, _lib.as_i32p(leg), _lib.as_i32p(route_of), _lib.as_i32p(flat)))
        if off is None:
            return leg, route_of, np.full((B, 1), -1, dtype=np.int32)
        n = np.diff(off)
        leg_at = np.full((B, int(n.max())), -1, dtype=np.int32)
        leg_at[np.arange(leg_at.shape[1])[None, :] < n[:, None]] = flat
        return leg, route_of, leg_at

    def clearance(self):
        """-> the monitor's records [B] (``_lib.CLEARANCE_DTYPE``: circle, ellipse, peer2, circle_row, ellipse_row, peer_row, peer)
        after synchronising; without a ``monitor`` the initial record everywhere."""
        rec = np.empty(self.B, dtype=_lib.CLEARANCE_DTYPE)
        self.solver._check(self.lib.nmpc_loop_clearance(self._l, rec.ctypes.data))
        return rec

    def peer_grid(self):
        """-> (header, cell_of [B] int32) after synchronising: the grid the last step's peers were found through (one
        ``_lib.PEER_GRID_DTYPE`` record: origin, h, W, nx, ny, filed) and the cell each robot was filed under (-1: unfiled).  Needs
        ``peers`` with a ``cell`` and a step taken."""
        hdr, cell_of = np.zeros((), dtype=_lib.PEER_GRID_DTYPE), np.empty(self.B, dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_peer_grid(self._l, hdr.ctypes.data, _lib.as_i32p(cell_of)))
        return hdr, cell_of

    def crowd_table(self):
        """-> [D, N, 5] after synchronising: every obstacle of the crowd over the horizon as the last step wrote it.  Needs a ``crowd``
        and a step taken."""
        tab = np.empty((self._crowd_D, self.cfg.N_hor, 5))
        self.solver._check(self.lib.nmpc_loop_crowd(self._l, _lib.as_dp(tab), None))
        return tab

    def crowd_seen(self):
        """-> [B, slots] int32 after synchronising: the obstacle in ellipse slot K + m of each robot's parameter vector at its last
        step, -1 for none.  Needs a ``crowd`` and a step taken."""
        seen = np.empty((self.B, self.crowd.slots), dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_crowd(self._l, None, _lib.as_i32p(seen)))
        return seen

    def crowd_grid(self):
        """-> (header, cell_of [D, N] int32, looked [B] int32) after synchronising: the grid the crowd's obstacles are found through
        (one ``_lib.CROWD_GRID_DTYPE`` record: origin, h, nx, ny, layers, filed), the cell each entry of the last step's table was
        filed under (-1: unfiled) and the filed entries in each robot's windows at its last step.  Needs a ``crowd`` with a ``cell``
        and a step taken."""
        hdr = np.zeros((), dtype=_lib.CROWD_GRID_DTYPE)
        D = self._crowd_D if self.crowd is not None else 0                   # (without a crowd the library says so)
        cell_of, looked = np.empty((D, self.cfg.N_hor), dtype=np.int32), np.empty(self.B, dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_crowd_grid(self._l, hdr.ctypes.data, _lib.as_i32p(cell_of), _lib.as_i32p(looked)))
        return hdr, cell_of, looked

    def crowd_clearance(self):
        """-> the crowd observer's records [B] (``_lib.CROWD_CLEARANCE_DTYPE``: level, row, obstacle) after synchronising; without
        a watched ``crowd`` the initial record everywhere."""
        rec = np.empty(self.B, dtype=_lib.CROWD_CLEARANCE_DTYPE)
        self.solver._check(self.lib.nmpc_loop_crowd_clearance(self._l, rec.ctypes.data))
        return rec

    def walls(self):
        """-> (wall_edge, wall_stage) [B, slots] int32 after synchronising: the edge in circle slot Nobs - slots + m of each robot's
        parameter vector at its last step and the stage at which it came closest, -1 for none.  Needs ``walls`` and a step taken."""
        M = self._walls.slots if self._walls is not None else 0
        edge, stage = np.empty((self.B, M), dtype=np.int32), np.empty((self.B, M), dtype=np.int32)
        self.solver._check(self.lib.nmpc_loop_walls(self._l, _lib.as_i32p(edge), _lib.as_i32p(stage)))
        return edge, stage

    def wall_grid(self):
        """-> (header, cell_off [nx * ny + 1], cell_edge [entries], looked [B]) after synchronising: the grid the walls' edges are found
        through (one ``_lib.WALL_GRID_DTYPE`` record: origin, h, nx, ny, entries), its CSR arrays (int32) and the distinct edges each robot
        measured at its last step.  Needs ``walls`` with a ``cell`` and a step taken."""
        return self._read_grid(self.lib.nmpc_loop_wall_grid)

    def map_grid(self):
        """-> (header, cell_off, cell_edge, looked [B]) after synchronising, as ``wall_grid``: the grid the map monitor's edges are found
        through and the distinct edges of W(r) summed over the rows of each robot's last step.  Needs a ``map_monitor`` with a ``cell``
        and a step taken."""
        return self._read_grid(self.lib.nmpc_loop_map_grid)

    def _read_grid(self, read):
        """``read``: nmpc_loop_wall_grid or nmpc_loop_map_grid, called for the header and then for the arrays it sizes"""
        hdr = np.zeros((), dtype=_lib.WALL_GRID_DTYPE)
        self.solver._check(read(self._l, hdr.ctypes.data, None, None, None))
        off, edge = np.empty(int(hdr["nx"]) * int(hdr["ny"]) + 1, dtype=np.int32), np.empty(int(hdr["entries"]), dtype=np.int32)
        looked = np.empty(self.B, dtype=np.int32)
        self.solver._check(read(self._l, None, _lib.as_i32p(off), _lib.as_i32p(edge), _lib.as_i32p(looked)))
        return hdr, off, edge, looked

    def map_clearance(self):
        """-> the map monitor's records [B] (``_lib.MAP_CLEARANCE_DTYPE``: wall2, wall_row, wall_edge, hits, hit_row, hit_poly, reserved)
        after synchronising; without a ``map_monitor`` the initial record everywhere."""
        rec = np.empty(self.B, dtype=_lib.MAP_CLEARANCE_DTYPE)
        self.solver._check(self.lib.nmpc_loop_map_clearance(self._l, rec.ctypes.data))
        return rec

    def tracking(self):
        """-> the track monitor's records [B] (``_lib.TRACKING_DTYPE``: cte2_max, cte2_sum, dth_max, dth2_sum, rows, cte_row, cte_seg,
        dth_row, last_seg, off_rows, off_row, reserved) after synchronising; the initial records before the first step.  Needs a ``track``."""
        rec = np.empty(self.B, dtype=_lib.TRACKING_DTYPE)
        self.solver._check(self.lib.nmpc_loop_tracking(self._l, rec.ctypes.data))
        return rec

    def _log(self, want_ctrl):
        ctrl = np.zeros((self.steps * self.cfg.num_steps_taken, self.B, 2)) if want_ctrl else None
        rec = None if want_ctrl else no_step_records(self.steps, self.B)
        n = self.lib.nmpc_loop_log(self._l, _lib.as_dp(ctrl), None if rec is None else rec.ctypes.data, self.steps)
        if n < 0:
            self.solver._check(n)
        return ctrl[:n * self.cfg.num_steps_taken] if want_ctrl else rec[:n]

    def controls(self):
        """-> [steps * s, B, 2] after synchronising: the (v, omega) applied between trajectory rows c and c + 1, +0.0 where a robot was
        not driven (``log=DriveLog()``; without it no rows)."""
        return self._log(True)

    def step_records(self):
        """-> [steps, B] (``_lib.STEP_RECORD_DTYPE``: exit_status, leg, num_inner_iterations, num_outer_iterations, cost, f2_norm,
        solve_time_ms) after synchronising: how each robot's solve of each step ended, exit_status -1 where it was not solved
        (``log=DriveLog()``; without it no steps)."""
        return self._log(False)

    def drive_summary(self):
        """-> the drive log's summaries [B] (``_lib.DRIVE_SUMMARY_DTYPE``) after synchronising; without a ``log`` the initial one everywhere."""
        rec = np.empty(self.B, dtype=_lib.DRIVE_SUMMARY_DTYPE)
        self.solver._check(self.lib.nmpc_loop_drive_summary(self._l, rec.ctypes.data))
        return rec

    def step_totals(self):
        """-> the fleet's totals per step [steps] (``_lib.STEP_TOTALS_DTYPE``) after synchronising (``log=DriveLog()``; without it no steps)."""
        tot = no_step_totals(self.steps)
        n = self.lib.nmpc_loop_step_totals(self._l, tot.ctypes.data, self.steps)
        if n < 0:
            self.solver._check(n)
        return tot[:n]

    def applied(self):
        """-> [steps * s, B, 2] after synchronising: the controls that acted under the plant, +0.0 where a robot was not driven
        (``plant.keep_applied``; without it no rows)."""
        rows = self.steps * self.cfg.num_steps_taken
        out = np.zeros((rows, self.B, 2))
        n = self.lib.nmpc_loop_plant_applied(self._l, _lib.as_dp(out), rows)
        if n < 0:
            self.solver._check(n)
        return out[:n]

    def measured(self):
        """-> [B, 3] after synchronising: what the last step's solves were given as poses: the measured poses under a plant with a
        ``meas`` > 0, else columns 0 .. 2 of the parameter vectors; the start states before the first step."""
        out = np.empty((self.B, 3))
        self.solver._check(self.lib.nmpc_loop_plant_measured(self._l, _lib.as_dp(out)))
        return out

    def ensemble_stats(self):
        """-> [steps, G] (``_lib.ENSEMBLE_DTYPE``: n, arrived, far_robot, reserved, mean [3], cov [4], far2) after synchronising: every
        group's record after every step taken (``ensemble=Ensemble(...)``; without it no steps)."""
        rec = no_ensemble_stats(self.steps, max(1, self.lib.nmpc_loop_ensemble_groups(self._l)))      # (the loop's G: 0 without the stage)
        n = self.lib.nmpc_loop_ensemble(self._l, rec.ctypes.data, self.steps)
        if n < 0:
            self.solver._check(n)
        return rec[:n]

    def read(self):
        """-> (state [B,3], last_u [B,2], idx [B], done [B] bool, status [B]) after synchronising."""
        B = self.B
        state, last_u = np.empty((B, 3)), np.empty((B, 2))
        idx, done = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.uint8)
        st = np.empty(B, dtype=_lib.STATUS_DTYPE)
        self.solver._check(self.lib.nmpc_loop_read(self._l, _lib.as_dp(state), _lib.as_dp(last_u),
                                                   _lib.as_i32p(idx), done.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   st.ctypes.data))
        return state, last_u, idx, done.astype(bool), st

    def params(self):
        """-> (P [B,n_p] of the last step, U [B,n_u], Y [B,n1])."""
        P, U, Y = np.empty((self.B, self.cfg.n_p)), np.empty((self.B, self.cfg.n_u)), np.empty((self.B, self.cfg.n1))
        self.solver._check(self.lib.nmpc_loop_params(self._l, _lib.as_dp(P), _lib.as_dp(U), _lib.as_dp(Y)))
        return P, U, Y

    def trajectory(self):
        """-> [rows, B, 3]: the start poses and every pose reached so far (needs ``max_steps`` > 0)."""
        rows = self.steps * self.cfg.num_steps_taken + 1
        T = np.empty((rows, self.B, 3))
        n = self.lib.nmpc_loop_trajectory(self._l, _lib.as_dp(T), rows)
        if n < 0:
            self.solver._check(n)
        return T
