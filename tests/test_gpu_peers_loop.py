"""GPU: the on-device loop with peers (nmpc_loop_set_peers) against its host mirror
``FleetRecedingHorizon(..., peers=...)`` -- itself pinned to a literal per-robot loop of the rule by
tests/test_peers_mirror.py -- driven by the oracle and given the kernels' sin / cos: parameter vectors, controls,
multipliers, states, reference indices, solver counters and trajectories must agree bit for bit, step after step."""

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import _lib, frontend, named_config
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, step_differing, trajectory_differing

pytestmark = pytest.mark.gpu

B = 24
RX, RY = 0.37, 0.53          # radii no scripted or padding ellipse has: a slot that shows them holds a peer


def _filled(cfg, P, K, M):
    """[B, M] bool: which peer slots of these parameter vectors hold a peer."""
    N = cfg.N_hor
    at = 20 + N + 3 * cfg.Nobs + (K + np.arange(M)) * 5 * N
    return (P[:, at + 2] == RX) & (P[:, at + 3] == RY)


def _groups(kind, n):
    return {"one": None, "three": (np.arange(n) * 5 % 3 + 1).astype(np.int32), "alone": np.arange(n, dtype=np.int32)[::-1].copy()}[kind]


def _narrow(starts, group_of):
    """A range that about half of the robots find somebody of their group within, at the start."""
    g = np.zeros(len(starts), dtype=np.int32) if group_of is None else group_of
    d = np.linalg.norm(starts[:, None, :2] - starts[None, :, :2], axis=2)
    d[(g[:, None] != g[None, :]) | np.eye(len(starts), dtype=bool)] = np.inf
    near = d.min(axis=1)
    return float(np.median(near[np.isfinite(near)])) if np.isfinite(near).any() else 1.0


# (config, K scripted obstacles, M peer slots, steps); cfg2: N_hor = 40, the two-stage kernel inside the loop
CASES = [("cfg4", 1, 2, 6), ("cfg1", 0, 1, 5), ("cfg2", 0, 3, 3)]


@pytest.mark.parametrize("rng_", ["wide", "narrow"])
@pytest.mark.parametrize("groups", ["one", "three", "alone"])
@pytest.mark.parametrize("name,K,M,steps", CASES)
def test_peers_loop_equals_host_mirror(name, K, M, steps, groups, rng_):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon, Peers
    cfg = named_config(name)
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, B, seed=41)
    dyn = fleet_ellipses(routes, route_of, i0, K, 9)
    group_of = _groups(groups, B)
    peers = Peers(slots=M, rx=RX, ry=RY, range=1e3 if rng_ == "wide" else _narrow(starts, group_of), group_of=group_of)
    o = oracle_for(cfg)
    seen = []
    s = BatchSolver(cfg, max_batch=32)
    s0 = BatchSolver(cfg, max_batch=32) if groups == "alone" else None
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of, peers=peers)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers)
        plain = DeviceRecedingHorizon(s0, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of) if s0 else None
        for k in range(steps):
            bad, Pd, _ = step_differing(dev, host, o.warm_solve())
            assert not bad, f"step {k}: {bad}"
            seen.append(_filled(cfg, Pd, K, M))
            if plain:                                  # nobody to see: the loop without peers, bit for bit
                plain.step()
                assert np.array_equal(Pd, plain.params()[0])
        assert not trajectory_differing(dev, host, steps)
        seen = np.stack(seen)
        if groups == "alone":
            assert not seen.any()
        elif rng_ == "wide":
            assert seen.all()                          # every group has more than M members: every slot holds a peer
        else:
            assert seen.any() and not seen.all(), "the narrow range must leave filled and unfilled slots"
        dev.close()
        if plain:
            plain.close()
    finally:
        s.close()
        if s0:
            s0.close()


def test_group_larger_than_a_wave():
    """130 robots in one group and 30 in another: lanes stride past 64 members, and the M rounds pick across lanes' lists."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon, Peers
    cfg = named_config("cfg1")
    n, steps, M = 160, 3, 3
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 4, n, seed=43)
    group_of = np.where(np.arange(n) % 16 < 13, 7, 2).astype(np.int32)
    assert (group_of == 7).sum() == 130
    peers = Peers(slots=M, rx=RX, ry=RY, range=3.0, group_of=group_of)
    o = oracle_for(cfg)
    seen = []
    s = BatchSolver(cfg, max_batch=n)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=steps, idx0=i0, route_of=route_of, peers=peers)
        host = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, peers=peers)
        far = np.nonzero(group_of == 7)[0][64:]                           # members a lane reaches only by striding
        for k in range(steps):
            bad, Pd, _ = step_differing(dev, host, o.warm_solve())
            assert not bad, f"step {k}: {bad}"
            seen.append(_filled(cfg, Pd, 0, M))
            assert np.isin(host.peer_index, far).any()
        assert not trajectory_differing(dev, host, steps)
        seen = np.stack(seen)
        assert seen[..., M - 1].any() and not seen[..., 0].all()          # full lists and empty ones
        dev.close()
    finally:
        s.close()


def test_peers_arguments_validated():
    """Every rejected call returns NMPC_ERR_BAD_ARG with a message and changes nothing: the loop then steps exactly like one
    that never had the call.  A valid call is accepted once, and only before the first step."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg4")
    n, K, steps = 8, 2, 3
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 2, n, seed=5)
    dyn = fleet_ellipses(routes, route_of, i0, K, 3)
    s1, s2 = BatchSolver(cfg, max_batch=16), BatchSolver(cfg, max_batch=16)
    lib = s1.lib
    try:
        a = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        b = DeviceRecedingHorizon(s2, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)

        def call(loop, group_of=None, M=1, rx=0.5, ry=0.5, rng_=5.0):
            g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.int32)
            rc = lib.nmpc_loop_set_peers(loop._l, _lib.as_i32p(g), M, rx, ry, rng_)
            return rc, lib.nmpc_last_error(loop.solver._h).decode()

        high, neg = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        high[3], neg[5] = n, -1
        cases = {"M = 0": dict(M=0), "M < 0": dict(M=-1), "K + M > Ndynobs": dict(M=2), "group_of = B": dict(group_of=high),
                 "group_of negative": dict(group_of=neg), "rx = 0": dict(rx=0.0), "ry negative": dict(ry=-0.5),
                 "range infinite": dict(rng_=float("inf")), "rx NaN": dict(rx=float("nan")), "range = 0": dict(rng_=0.0),
                 "ry infinite": dict(ry=float("inf"))}
        for what, kw in cases.items():
            rc, msg = call(a, **kw)
            assert rc == -3 and msg, what
        for k in range(steps):                         # still the loop without peers
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert np.array_equal(x, y), f"step {k}"
            assert np.array_equal(a.read()[4]["num_inner_iterations"], b.read()[4]["num_inner_iterations"])
        rc, msg = call(a)
        assert rc == -3 and "step" in msg              # after a step
        assert np.array_equal(a.trajectory(), b.trajectory())
        a.close()
        b.close()
        c = DeviceRecedingHorizon(s1, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of)
        assert call(c)[0] == 0
        rc, msg = call(c)
        assert rc == -3 and msg                        # a second call
        c.step()
        c.read()
        c.close()
    finally:
        s1.close()
        s2.close()
