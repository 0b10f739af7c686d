"""GPU: the on-device loop with a crowd (nmpc_loop_set_crowd, nmpc_loop_set_crowd_monitor; ``nmpc_loop_crowd_advance_kernel``,
``nmpc_loop_crowd_kernel``, ``nmpc_loop_crowd_monitor_kernel``) against its host mirror
``FleetRecedingHorizon(..., crowd=...)`` -- itself pinned to a literal per-robot, per-obstacle loop of the rule by
tests/test_crowd_mirror.py -- driven by the oracle and given the kernels' sin / cos: parameter vectors, controls, multipliers, states,
reference indices, solver counters and trajectories, and the crowd's table, chosen obstacles and observer records, must agree bit for
bit, step after step."""

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, staggered_fleet, step_differing, trajectory_differing
from test_crowd_mirror import NAN_OBSTACLE, RX, RY, arranged, filled, narrow_range, reach_arranged, scattered
from test_loop_shapes_mirror import CASES as SHAPES

pytestmark = pytest.mark.gpu

B = 24


def crowd_differing(dev, host):
    """The crowd's products on which a device loop and its mirror are not bit-equal (a value compares by its bytes)."""
    bad = []
    if dev.crowd_table().tobytes() != np.ascontiguousarray(host.crowd_table()).tobytes():
        bad.append("crowd_table")
    if not np.array_equal(dev.crowd_seen(), host.crowd_seen):
        bad.append("crowd_seen")
    a, b = dev.crowd_clearance(), host.crowd_clearance()
    return bad + [f"crowd_clearance.{f}" for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]


def run_pair(cfg, routes, route_of, starts, i0, dyn, crowd, steps, peers=None, retire=False, sinus_object=False, until=None):
    """Step a device loop and its mirror ``steps`` times (or while ``until(host)`` says so, ``steps`` at the most), comparing
    everything at every step -> (the mirror, per step the chosen obstacles, per step the device's parameter vectors)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    o = oracle_for(cfg)
    seen, Ps = [], []
    s = BatchSolver(cfg, max_batch=32)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of, sinus_object=sinus_object,
                                    peers=peers, retire=retire, crowd=crowd)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, sinus_object=sinus_object, idx0=i0,
                                    peers=peers, retire=retire, crowd=crowd)
        assert all(r == e for r, e in zip(dev.crowd_clearance().tolist(), host.crowd_clearance().tolist()))     # the initial records
        while host.steps < steps and (until is None or until(host)):
            k = host.steps
            bad, Pd, _ = step_differing(dev, host, o.warm_solve())
            assert not bad, f"step {k}: {bad}"
            bad = crowd_differing(dev, host)
            assert not bad, f"step {k}: {bad}"
            seen.append(host.crowd_seen.copy())
            Ps.append(Pd)
        assert not trajectory_differing(dev, host, host.steps)
        dev.close()
    finally:
        s.close()
    return host, seen, Ps


def _fleet(cfg, K):
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, B, seed=41)
    return routes, route_of, starts, i0, fleet_ellipses(routes, route_of, i0, K, 9)


def _narrow(cfg, fleet, obs, sinus, M, factor=1.5):
    from mpc_trajectory_generator_amd.trajectory import Crowd, FleetRecedingHorizon
    routes, route_of, starts, i0, dyn = fleet
    return factor * narrow_range(lambda r: FleetRecedingHorizon(routes, route_of, starts, dyn, idx0=i0, crowd=Crowd(obs, M, r, sinus=sinus)))


def test_few_obstacles_leave_lanes_without_one():
    """D = 5 with K = 1 and two crowd slots: 59 lanes of the selection hold nothing."""
    from mpc_trajectory_generator_amd.trajectory import Crowd
    cfg = named_config("cfg4")
    fleet = _fleet(cfg, 1)
    obs, sinus = scattered(cfg, 5)
    _, seen, _ = run_pair(cfg, *fleet, Crowd(obs, 2, 1e3, sinus=sinus, watch=True), 4)
    assert filled(seen).all()


@pytest.mark.parametrize("grid", [False, True])
def test_slot_order_with_peers(grid):
    """D = 70 (lanes take a second obstacle).  All-pairs peers at cfg4 with K = 1, one crowd slot and one peer slot; grid peers at cfg1
    with K = 0, one crowd slot and two peer slots: the slot base of both peers kernels."""
    from mpc_trajectory_generator_amd.trajectory import Crowd, Peers
    cfg = named_config("cfg1" if grid else "cfg4")
    K, Mc, Mp = (0, 1, 2) if grid else (1, 1, 1)
    fleet = _fleet(cfg, K)
    obs, sinus = scattered(cfg, 70)
    peers = Peers(slots=Mp, rx=RX, ry=RY, range=1e3, cell=1.0 if grid else None)
    host, seen, Ps = run_pair(cfg, *fleet, Crowd(obs, Mc, 1e3, sinus=sinus, watch=True), 4, peers=peers)
    assert filled(seen).all() and (np.stack(seen) >= 64).any()
    N = cfg.N_hor
    at = 20 + N + 3 * cfg.Nobs + np.arange(3) * 5 * N
    for P, chosen in zip(Ps, seen):
        for m in range(3):
            peer = (P[:, at[m] + 2] == RX) & (P[:, at[m] + 3] == RY)
            assert peer.all() if m >= K + Mc else not peer.any(), m
    assert np.array_equal(Ps[-1][:, at[K]:at[K] + 5 * N], host.crowd_table()[seen[-1][:, 0]].reshape(B, -1))


@pytest.mark.parametrize("rng_", ["wide", "narrow"])
def test_one_lanes_whole_list_a_nan_obstacle_and_twins(rng_):
    """D = 200, three slots: the three closest obstacles of robot 0 at d, d + 64 and d + 128, a NaN obstacle, two identical ones."""
    from mpc_trajectory_generator_amd.trajectory import Crowd
    cfg = named_config("cfg1")
    fleet = _fleet(cfg, 0)
    obs, sinus = arranged(cfg, fleet[2])
    r = 1e6 if rng_ == "wide" else _narrow(cfg, fleet, obs, sinus, 3, factor=1.0)
    host, seen, _ = run_pair(cfg, *fleet, Crowd(obs, 3, r, sinus=sinus, watch=True), 3)
    assert not (np.stack(seen) == NAN_OBSTACLE).any() and not (host.crowd_clearance()["obstacle"] == NAN_OBSTACLE).any()
    if rng_ == "wide":
        for k, chosen in enumerate(seen):
            reach_arranged(chosen, k == 0)
    else:
        assert filled(seen).any() and not filled(seen).all(), "the narrow range must leave filled and unfilled slots"


def test_two_stage_solve_and_the_longest_rows():
    """cfg2: N = 40, the two-stage solve kernel inside the loop, rows of 200 doubles."""
    from mpc_trajectory_generator_amd.trajectory import Crowd
    cfg = named_config("cfg2")
    assert cfg.N_hor == 40
    fleet = _fleet(cfg, 0)
    obs, sinus = scattered(cfg, 70)
    _, seen, _ = run_pair(cfg, *fleet, Crowd(obs, 3, _narrow(cfg, fleet, obs, sinus, 3, factor=3.0), sinus=sinus, watch=True), 3)
    assert filled(seen).any()


@pytest.mark.parametrize("which", ["n33-s7", "s20"])
def test_shapes(which):
    """N = 33 with 7 steps taken, and s = N = 20 (every row fresh every step, the observer over 20 rows): K = 2 scripted obstacles,
    one crowd slot."""
    from mpc_trajectory_generator_amd.trajectory import Crowd
    c = SHAPES[which]()
    n = len(c.starts)
    obs, sinus = scattered(c.cfg, 5)
    host, seen, _ = run_pair(c.cfg, [c.route], np.zeros(n, dtype=np.int32), c.starts, c.idx0, c.dyn,
                             Crowd(obs, 1, 1e3, sinus=sinus, watch=True), c.steps, sinus_object=c.sinus)
    assert c.K == 2 and filled(seen).all() and (host.crowd_clearance()["row"] >= 1).all()


def test_retiring_fleet():
    """Robots retire one after the other: the table keeps advancing, a retired robot keeps p, seen and its record (the mirror's, held
    to that by tests/test_crowd_mirror.py), and a step with nobody active still advances the table."""
    from mpc_trajectory_generator_amd.trajectory import Crowd
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg, back=(2, 5, 9))
    obs, sinus = scattered(cfg, 5)
    extra = [2]                                                 # steps after the last retirement

    def until(host):
        if host.n_active:
            return True
        extra[0] -= 1
        return extra[0] >= 0

    host, seen, Ps = run_pair(cfg, routes, route_of, starts, i0, None, Crowd(obs, 2, 1e3, sinus=sinus, watch=True), 45, retire=True, until=until)
    at = host.retired_at
    assert host.n_active == 0 and len(set(at.tolist())) > 2 and host.steps == at.max() + 2
    assert np.array_equal(Ps[-1], Ps[-3]) and np.array_equal(seen[-1], seen[-3])
    first = int(np.argmin(at))                                  # retired long before the end: its row never moved again
    assert at[first] < at.max() and all(np.array_equal(P[first], Ps[at[first] - 1][first]) for P in Ps[at[first]:])


def test_observer_only_observes():
    """With the observer on and off: P, U, Y, states and statuses bit-equal."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import Crowd, DeviceRecedingHorizon, no_crowd_clearance
    cfg = named_config("cfg4")
    routes, route_of, starts, i0, dyn = _fleet(cfg, 1)
    obs, sinus = scattered(cfg, 70)
    s1, s2 = BatchSolver(cfg, max_batch=32), BatchSolver(cfg, max_batch=32)
    try:
        on = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of, crowd=Crowd(obs, 2, 1e3, sinus=sinus, watch=True))
        off = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of, crowd=Crowd(obs, 2, 1e3, sinus=sinus))
        for k in range(3):
            on.step()
            off.step()
            for x, y in zip(on.params() + on.read()[:4], off.params() + off.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
            a, b = on.read()[4], off.read()[4]
            assert all(np.array_equal(a[f], b[f]) for f in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "f2_norm"))
            assert np.array_equal(on.crowd_seen(), off.crowd_seen()) and np.array_equal(on.crowd_table(), off.crowd_table())
        assert off.crowd_clearance().tobytes() == no_crowd_clearance(B).tobytes() and (on.crowd_clearance()["row"] >= 1).all()
        on.close()
        off.close()
    finally:
        s1.close()
        s2.close()


def test_without_a_crowd_the_loop_is_the_plain_one():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, no_crowd_clearance
    cfg = named_config("cfg4")
    routes, route_of, starts, i0, dyn = _fleet(cfg, 2)
    s1, s2 = BatchSolver(cfg, max_batch=32), BatchSolver(cfg, max_batch=32)
    try:
        a = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of, crowd=None)
        b = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=3, idx0=i0, route_of=route_of)
        for k in range(3):
            a.step()
            b.step()
            assert np.array_equal(a.params()[0], b.params()[0]), f"step {k}"
        assert a.crowd_clearance().tobytes() == no_crowd_clearance(B).tobytes()
        assert s1.lib.nmpc_loop_crowd(a._l, None, None) == -3 and b"no crowd" in s1.lib.nmpc_last_error(s1._h)
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()


def test_crowd_arguments_validated():
    """Every rejected call returns NMPC_ERR_BAD_ARG with a message and changes nothing: the loop then steps exactly like one that never
    had the call.  A valid call is accepted once, and only before the first step; the second of the crowd and peers setters checks
    that all three kinds of ellipse fit."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg4")
    n, K, steps = 8, 1, 2
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 2, n, seed=5)
    dyn = fleet_ellipses(routes, route_of, i0, K, 3)
    obst = np.ascontiguousarray(np.random.default_rng(1).uniform(0.1, 5.0, (4, 10)))
    obst[:, 8] = 0.0
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    lib = s1.lib
    inf, nan = float("inf"), float("nan")

    def call(loop, D=4, tab=obst, pad=0.5, M=1, rng_=5.0):
        rc = lib.nmpc_loop_set_crowd(loop._l, D, _lib.as_dp(tab), pad, M, rng_)
        return rc, lib.nmpc_last_error(loop.solver._h).decode()

    try:
        a = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        b = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        cases = {"D = 0": dict(D=0), "D > 16384": dict(D=16385), "obst NULL": dict(tab=None), "M = 0": dict(M=0), "K + M > Ndynobs": dict(M=3),
                 "pad NaN": dict(pad=nan), "pad infinite": dict(pad=-inf), "range = 0": dict(rng_=0.0), "range negative": dict(rng_=-1.0),
                 "range infinite": dict(rng_=inf), "range NaN": dict(rng_=nan)}
        for what, kw in cases.items():
            rc, msg = call(a, **kw)
            assert rc == -3 and "nmpc_loop_set_crowd" in msg, what
        assert lib.nmpc_loop_set_crowd_monitor(a._l) == -3 and b"no crowd" in lib.nmpc_last_error(s1._h)
        for k in range(steps):                         # still the loop without a crowd
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
        rc, msg = call(a)
        assert rc == -3 and "step" in msg              # after a step
        a.close()
        b.close()
        c = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=0, idx0=i0, route_of=route_of)
        assert lib.nmpc_loop_crowd(c._l, None, None) == -3
        assert call(c)[0] == 0
        rc, msg = call(c)
        assert rc == -3 and "already" in msg           # a second call
        assert lib.nmpc_loop_crowd(c._l, None, None) == -3 and b"first step" in lib.nmpc_last_error(s1._h)
        assert lib.nmpc_loop_set_crowd_monitor(c._l) == -3 and b"max_steps" in lib.nmpc_last_error(s1._h)
        assert lib.nmpc_loop_set_peers(c._l, None, 2, 0.5, 0.5, 5.0) == -3 and b"crowd" in lib.nmpc_last_error(s1._h)     # 1 + 1 + 2 > 3
        assert lib.nmpc_loop_set_peers(c._l, None, 1, 0.5, 0.5, 5.0) == 0
        c.step()
        c.read()
        c.close()
        d = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        assert lib.nmpc_loop_set_peers(d._l, None, 2, 0.5, 0.5, 5.0) == 0
        rc, msg = call(d)
        assert rc == -3 and "peers" in msg             # the crowd comes second: 1 + 1 + 2 > 3
        d.close()
        e = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        assert lib.nmpc_loop_set_peers(e._l, None, 1, 0.5, 0.5, 5.0) == 0 and call(e)[0] == 0
        assert lib.nmpc_loop_set_crowd_monitor(e._l) == 0 and lib.nmpc_loop_set_crowd_monitor(e._l) == -3
        e.step()
        e.read()
        e.close()
    finally:
        s1.close()
        s2.close()
