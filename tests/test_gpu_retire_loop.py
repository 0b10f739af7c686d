"""GPU: the on-device loop with retirement (nmpc_loop_set_retire, nmpc_loop_active, nmpc_loop_run) against
its host mirror ``FleetRecedingHorizon(..., retire=True)`` -- itself pinned to robots driven one by one ``while not terminal`` by
tests/test_retire_mirror.py -- driven by the oracle and given the kernels' sin / cos: parameter vectors, controls, multipliers,
states, reference indices, ``done``, solver counters, ``retired_at`` and the active count must agree bit for bit after every step,
and the trajectories at the end."""
import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import frontend, harness, named_config
from mpc_trajectory_generator_amd.workloads import (fleet_ellipses, move_near_goal, route_fleet, staggered_fleet, step_differing,
                                                    trajectory_differing)
from test_retire_mirror import LIMIT, PEERS

pytestmark = pytest.mark.gpu

STEPS_TO_THE_END = 90        # the staggered fleet's last robot retires after 90 steps (tests/test_retire_mirror.py)


def _near_goal_fleet(name, K):
    """12 robots on 3 planned routes of scene 11, four of them started 2, 3, 5 and 8 samples before their routes' ends."""
    cfg = named_config(name)
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 12, seed=31)
    starts, i0 = move_near_goal(routes, route_of, starts, i0, (2, 3, 5, 8))
    return cfg, routes, route_of, starts, i0, fleet_ellipses(routes, route_of, i0, K, 7)


def _case(which):
    """-> (cfg, routes, route_of, starts, idx0, dyn, peers, steps or None = to completion)"""
    from mpc_trajectory_generator_amd.trajectory import Peers
    if which in ("staggered", "peers"):
        cfg = named_config("cfg1")
        routes, route_of, starts, i0 = staggered_fleet(cfg)
        if which == "staggered":
            return cfg, routes, route_of, starts, i0, None, None, None
        return cfg, routes, route_of, starts, i0, None, Peers(group_of=route_of, **PEERS), 14
    name, K, steps = {"cfg4-ellipses": ("cfg4", 3, 10), "cfg2": ("cfg2", 0, 24)}[which]
    return _near_goal_fleet(name, K) + (None, steps)


@pytest.mark.parametrize("which", ["staggered", "cfg4-ellipses", "cfg2", "peers"])
def test_retiring_loop_equals_host_mirror(which):
    """Every step through nmpc_loop_run(l, 1), so that run's own waiting and counting are what is compared; "staggered" runs until
    nobody is active."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg, routes, route_of, starts, i0, dyn, peers, steps = _case(which)
    B = len(starts)
    o = oracle_for(cfg)
    s = BatchSolver(cfg, max_batch=B)
    counts = []

    def one(dev):
        assert dev.run(1) == 1

    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=LIMIT, idx0=i0, route_of=route_of, peers=peers, retire=True)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers, retire=True)
        assert dev.active()[0] == B
        while (host.n_active if steps is None else host.steps < steps) and host.steps < LIMIT:
            bad = step_differing(dev, host, o.warm_solve(threads=16), one)[0]
            assert not bad, f"step {host.steps - 1}: {bad}"
            counts.append(host.n_active)
        assert not trajectory_differing(dev, host, host.steps)
        print(which, "active after each step:", counts, "retired_at", host.retired_at.tolist())
        assert any(0 < n < B for n in counts), "no step with some robots retired and others active"
        if steps is None:
            assert counts[-1] == 0 and dev.run(5) == 0         # nobody left: run takes no step
        if peers is not None:
            parked = ~host.active
            assert parked.any() and np.isin(host.peer_index[host.active], np.nonzero(parked)[0]).any(), \
                "no active robot has a retired groupmate among its peers"
        dev.close()
    finally:
        s.close()


def test_retiring_loop_under_a_batch_budget_replays_every_step():
    """Timed solves are not deterministic, so there is no mirror to follow: every step is checked on its own.  The active robots'
    solves against the replay rule of tests/test_gpu_time_limits.py, from the warm start the loop held; the retired robots' rows
    against what they held; who retires against the terminal test on what the device reports."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    from test_gpu_time_limits import OUT_OF_TIME, THREADS, _check_rule
    cfg = named_config("cfg1")
    route = harness.scene_route(cfg, 11)
    B = 1000
    i0, starts, _ = route_fleet(route, B, 17, back=1)          # robots all along the route, its last samples included
    end = route.end
    s = BatchSolver(cfg, max_batch=B, batch_budget_ms=2.0)
    stopped, counts = 0, []
    try:
        dev = DeviceRecedingHorizon(s, route, starts, None, idx0=i0, retire=True)
        active, retired_at = np.ones(B, dtype=bool), np.full(B, -1, dtype=np.int32)
        for k in range(12):
            P0, U0, Y0 = dev.params()
            before = dev.read()
            dev.step()
            Pk, Uk, Yk = dev.params()
            state, last_u, idx, done, st = dev.read()
            a = np.nonzero(active)[0]
            uU, yU, sU = oracle_for(cfg).solve_batch(Pk[a], u0=U0[a], y0=Y0[a], threads=THREADS)
            _check_rule(cfg, Pk[a], U0[a], Y0[a], (Uk[a], Yk[a], st[a]), (uU, yU, sU))
            stopped += int(np.sum(st[a]["exit_status"] == OUT_OF_TIME))
            r = ~active
            for now, then in zip((Pk, Uk, Yk, state, last_u, idx, done, st), (P0, U0, Y0) + before):
                assert now[r].tobytes() == then[r].tobytes(), f"step {k}: a retired robot's rows moved"
            terminal = (np.abs(state[:, 0] - end[0]) <= 0.05) & (np.abs(state[:, 1] - end[1]) <= 0.05) & (np.abs(last_u[:, 0]) < 0.005)
            assert np.array_equal(done[a], terminal[a]) and done[r].all()
            n, at = dev.active()
            assert np.array_equal(at[r], retired_at[r])
            newly = active & done
            assert (at[newly] == k + 1).all() and (at[active & ~done] == -1).all()
            active &= ~done
            retired_at = at
            assert n == active.sum()
            counts.append(n)
        dev.close()
    finally:
        s.close()
    print("active after each step:", counts, "stopped by the clock:", stopped)
    assert any(0 < n < B for n in counts), "no step with some robots retired and others active"
    assert stopped > 0, "a 2 ms budget stopped no instance of a cold-started fleet of 1000"


def test_each_robot_as_if_alone():
    """Without peers a robot's trajectory in the retiring fleet is that robot's in a retiring loop of its own (B = 1)."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    B, sn = len(starts), cfg.num_steps_taken
    s = BatchSolver(cfg, max_batch=B)
    try:
        fleet = DeviceRecedingHorizon(s, routes, starts, None, max_steps=LIMIT, idx0=i0, route_of=route_of, retire=True)
        steps = fleet.run(LIMIT)
        n, at = fleet.active()
        assert n == 0 and at.max() == steps
        T = fleet.trajectory()
        Pf, Uf, Yf = fleet.params()
        fleet.close()
        for b in range(B):
            one = DeviceRecedingHorizon(s, routes[route_of[b]], starts[b:b + 1], None, max_steps=LIMIT, idx0=i0[b:b + 1], retire=True)
            took = one.run(LIMIT)
            assert took == at[b] and one.active()[1][0] == at[b], f"robot {b}"
            Tb = one.trajectory()
            assert np.array_equal(Tb[:, 0], T[:took * sn + 1, b]), f"robot {b}: trajectory"
            assert np.array_equal(T[took * sn:, b], np.tile(Tb[-1, 0], (len(T) - took * sn, 1))), f"robot {b}: rows after retirement"
            for x, y in zip(one.params(), (Pf, Uf, Yf)):
                assert np.array_equal(x[0], y[b]), f"robot {b}: p, u or y of its last step"
            one.close()
    finally:
        s.close()


def test_run_to_the_end_then_a_step_solves_nothing():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    s = BatchSolver(cfg, max_batch=len(starts))
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=LIMIT, idx0=i0, route_of=route_of, retire=True)
        assert dev.run(40) == 40                               # max_steps ends a run
        assert dev.run(LIMIT) == STEPS_TO_THE_END - 40         # nobody active ends one
        n, at = dev.active()
        assert n == 0 and at.max() == STEPS_TO_THE_END and at.sum() == 552
        before = dev.params() + dev.read()
        dev.step()                                             # counts as a step, launches no solve
        assert dev.steps == STEPS_TO_THE_END + 1
        for x, y in zip(dev.params() + dev.read(), before):
            assert x.tobytes() == y.tobytes()                  # (the statuses whole: counters, norms and clocks)
        T = dev.trajectory()
        assert T.shape[0] == (STEPS_TO_THE_END + 1) * cfg.num_steps_taken + 1
        assert np.array_equal(T[-1], before[3]) and np.array_equal(T[-2], before[3])
        dev.close()
        short = DeviceRecedingHorizon(s, routes, starts, None, max_steps=7, idx0=i0, route_of=route_of, retire=True)
        assert short.run(LIMIT) == 7                           # a full trajectory buffer ends one
        short.close()
    finally:
        s.close()


def test_retire_arguments_validated():
    """A call after a step, a second call, and nmpc_loop_run on a loop that does not retire: NMPC_ERR_BAD_ARG with a message and
    nothing changed; the handle then still solves a batch exactly like the oracle."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 8, seed=2)
    s = BatchSolver(cfg, max_batch=16)
    lib = s.lib

    def msg():
        return lib.nmpc_last_error(s._h).decode()

    try:
        assert lib.nmpc_loop_set_retire(None, 1) == -3
        a = DeviceRecedingHorizon(s, routes, starts, None, idx0=i0, route_of=route_of)
        assert lib.nmpc_loop_run(a._l, 3, None) == -3 and "retire" in msg()
        n, at = a.active()
        assert n == 8 and (at == -1).all()                      # without retirement: B and -1 everywhere
        a.step()
        assert lib.nmpc_loop_set_retire(a._l, 1) == -3 and "step" in msg()
        assert a.active()[0] == 8 and lib.nmpc_loop_run(a._l, 3, None) == -3
        a.close()
        b = DeviceRecedingHorizon(s, routes, starts, None, idx0=i0, route_of=route_of, retire=True)
        assert lib.nmpc_loop_set_retire(b._l, 1) == -3 and msg()          # a second call
        assert lib.nmpc_loop_set_retire(b._l, 0) == -3
        assert lib.nmpc_loop_run(b._l, -1, None) == -3 and msg()
        assert b.run(2) == 2 and b.active()[0] == 8
        b.close()
        P = harness.synthetic_batch(cfg, 11, 8, 77)
        u, y, st = s.solve(P)
        uo, yo, sto = oracle_for(cfg).solve_batch(P, threads=8)
        assert np.array_equal(u, uo) and np.array_equal(y, yo)
        assert np.array_equal(st["num_inner_iterations"], sto["num_inner_iterations"])
    finally:
        s.close()


def test_without_retirement_the_bits_of_a_loop_never_asked():
    """nmpc_loop_set_retire(l, 0) and no call at all: the same loop, to its goals and past them."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = staggered_fleet(cfg)
    steps = 30
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    try:
        a = DeviceRecedingHorizon(s1, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of)
        b = DeviceRecedingHorizon(s2, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of, retire=False)
        assert s2.lib.nmpc_loop_set_retire(b._l, 0) == 0
        for k in range(steps):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
            sa, sb = a.read()[4], b.read()[4]
            for f in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "penalty"):
                assert np.array_equal(sa[f], sb[f]), (k, f)
        n, at = b.active()
        assert a.read()[3].any() and n == 16 and (at == -1).all()      # some are at their goals, and nobody retires
        assert np.array_equal(a.trajectory(), b.trajectory())
        a.close()
        b.close()
    finally:
        s1.close()
        s2.close()
