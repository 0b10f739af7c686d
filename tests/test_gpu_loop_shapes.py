"""GPU: the on-device loop's kernels (csrc/nmpc_loop.h) at the shapes where their strided loops, clamps and chunked scan do something
else than in the straight-line case, against the host mirrors -- which tests/test_loop_shapes_mirror.py holds to the literal per-robot
rules at exactly these fleets -- driven by the oracle and given the kernels' sin / cos.  Parameter vectors, controls, multipliers,
states, ``last_u``, reference indices, ``done``, solver counters (``retired_at`` and the active count where retiring) must agree bit for
bit after every step, and the trajectories at the end; there is no tolerance anywhere.

What each case makes a kernel do, and the assertion on the mirror (``REACH`` and the ones below) that guarantees it:

* ``s11-stale``: the reference window ``for (j = lb + lane; j < ub; j += 64)`` takes a second sample per lane and ``wave_argmin`` picks
  across strides -- a new index at window offset >= 64 is one only the second iteration of a lane visits.
* ``s3``, ``s5-sinus``, ``s20``, ``n33-s7``: ``linspace_at``'s interior ``(double)i * step + t0`` with t0 != 0 (H = s >= 3), ``fresh`` at
  ``st >= N - s``, the ``5 * s`` rotation, and s = N_hor where every stage is fresh at every step; checked on the configuration.
* ``verts150-*``: the vertex search ``for (j = lane; j < nv; j += 64)`` strides and must keep the FIRST minimum -- the closest vertex
  has an exact duplicate >= 64 positions later (another stride of the same or a later lane), and lies inside the circle slots, so that
  a wrong choice shows in p.  ``no-vertices``, ``nobs0-ndyn0``: ``nv = 0`` (``ok`` false everywhere) and the empty loops over
  ``a.nobs = 0`` and ``tot = 0`` with the one-element allocations.
* ``route5``, ``route1``: ``n_ref < N_hor``: ``far`` is false and ``ok = j < n`` pads from step 0 on (``idx + N_hor >= n_ref``), and
  ``nbase == 0`` runs the braking-table filter ``cnt == k``.
* ``brake7``, ``brake45``: ``n_brake`` of 8 and 45: ``k - nbase < n_brake`` is false past the table's end for 8, and the filter inside the
  last sample meets more entries than the horizon has stages for 45.
* the tiled staggered fleet: ``nmpc_loop_compact_kernel`` with ``chunk`` 2 and 3 -- a thread counts active and retired robots of its
  own chunk (``mixed_chunks`` > 0 while ``0 < n_active < B``), places them from ``cnt[t] - c``, and the threads past the last robot
  are empty (``lo = B``).
* the group of 272: a lane of ``nmpc_loop_peers_kernel`` meets a fourth and fifth candidate, the ``cd`` / ``cj`` pair falls off the end
  of its list of three (``reach_overflow``: a chosen peer at member position >= 192, in another lane than the robot itself).  Peers at
  three steps taken: ``c = s + k < N ? s + k : N - 1`` in ``nmpc_loop_predict_kernel`` holds the last control for three stages.
* the NaN pose: ``if (d != d) d = -inf`` in both searches (Nobs = 3 against six vertices); without it no lane ever holds a candidate."""
import time

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, staggered_fleet, step_differing, tiled_fleet, trajectory_differing
from test_gpu_peers_loop import _filled
from test_loop_shapes_mirror import CASES, NAN_ROBOT, REACH, _nan_pose, large_group_fleet, mixed_chunks, peers_s3_fleet, reach_overflow

pytestmark = pytest.mark.gpu

BRAKING_LIMIT = 30          # steps within which the robots two samples before the end must be done (cfg 1 takes 10: tests/test_retire_mirror.py)


@pytest.mark.parametrize("which", list(CASES))
def test_loop_equals_host_mirror_at(which):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, VectorizedRecedingHorizon
    c = CASES[which]()
    o = oracle_for(c.cfg)
    limit = BRAKING_LIMIT if c.until_done else c.steps
    trace = []
    t0 = time.perf_counter()
    s = BatchSolver(c.cfg, max_batch=32)
    try:
        dev = DeviceRecedingHorizon(s, c.route, c.starts, c.dyn, max_steps=limit, idx0=c.idx0, sinus_object=c.sinus)
        host = VectorizedRecedingHorizon(c.route, c.starts, c.dyn, sincos=o.sincos_array, sinus_object=c.sinus, idx0=c.idx0)
        steps = 0
        while steps < limit and not (c.until_done and steps >= c.steps and host.done.any()):
            bad = _traced_step_differing(dev, host, o, trace)
            assert not bad, f"step {steps}: {bad}"
            steps += 1
        assert not trajectory_differing(dev, host, steps)
        if c.until_done:
            assert host.done.any() and not host.done.all(), "the first robots are not done, or everybody is"
        dev.close()
    finally:
        s.close()
    print(f"{which}: {steps} steps, {time.perf_counter() - t0:.1f} s")
    if c.reach:
        REACH[c.reach](c, trace)


def _traced_step_differing(dev, host, o, trace):
    """``step_differing`` with the mirror's step recorded for the REACH checks."""
    state, before = host.state.copy(), np.array(host.idx).copy()
    bad = step_differing(dev, host, o.warm_solve(threads=16))[0]
    trace.append((state, before, np.array(host.idx).copy()))
    return bad


@pytest.mark.parametrize("B", [1025, 2050])
def test_compaction_with_several_robots_per_thread(B):
    """The 16 robots of the staggered fleet tiled to B, retiring, every step through nmpc_loop_run(l, 1): robot b must be the 16-robot
    retiring mirror's robot b % 16 in every array, in ``retired_at`` and in the trajectory, and the active count the mirror's scaled."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = named_config("cfg1")
    base = staggered_fleet(cfg)
    routes, route_of, starts, i0 = tiled_fleet(*base, B / 16)
    assert len(starts) == B
    rows = np.arange(B) % 16
    o = oracle_for(cfg)
    limit = 20
    counts, mixed = [], []
    t0 = time.perf_counter()

    def one(dev):
        assert dev.run(1) == 1

    def retirement_steps():
        return set(host.retired_at[host.retired_at >= 0].tolist())

    s = BatchSolver(cfg, max_batch=B)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, None, max_steps=limit, idx0=i0, route_of=route_of, retire=True)
        host = FleetRecedingHorizon(*base[:3], None, sincos=o.sincos_array, idx0=base[3], retire=True)
        assert dev.active()[0] == B
        extra = 1                                                  # one more step after the second retirement: its compaction meets both
        while host.steps < limit and (len(retirement_steps()) < 2 or extra):
            extra -= len(retirement_steps()) >= 2
            bad = step_differing(dev, host, o.warm_solve(threads=16), one, rows)[0]
            assert not bad, f"step {host.steps - 1}: {bad}"
            counts.append(int(host.active[rows].sum()))
            mixed.append(mixed_chunks(host.active[rows]))
        assert not trajectory_differing(dev, host, host.steps, rows)
        T, at = dev.trajectory(), host.retired_at[rows]
        for b in np.nonzero(at >= 0)[0]:                           # retired rows repeat the final pose
            assert (T[at[b]:, b] == T[at[b], b]).all(), f"robot {b}"
        dev.close()
    finally:
        s.close()
    print(f"B = {B}: active after each step {counts}, threads holding both kinds {mixed}, retired_at {host.retired_at.tolist()}, "
          f"{time.perf_counter() - t0:.1f} s")
    assert len(retirement_steps()) >= 2, f"fewer than two different retirement steps within {limit} steps"
    assert any(0 < n < B for n in counts), "no step with some robots retired and others active"
    assert all(m > 0 for n, m in zip(counts, mixed) if 0 < n < B), "a step whose compaction had no thread holding retired and active robots"


def _peers_run(cfg, routes, route_of, starts, i0, K, peers, steps, check):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, FleetRecedingHorizon
    n = len(starts)
    dyn = fleet_ellipses(routes, route_of, i0, K, 9)
    o = oracle_for(cfg)
    t0 = time.perf_counter()
    s = BatchSolver(cfg, max_batch=n)
    try:
        dev = DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, idx0=i0, route_of=route_of, peers=peers)
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, peers=peers)
        for k in range(steps):
            bad, Pd, _ = step_differing(dev, host, o.warm_solve(threads=16))
            assert not bad, f"step {k}: {bad}"
            assert _filled(cfg, Pd, K, peers.slots).all()          # nobody is out of range: every slot holds a peer
            check(host)
        assert not trajectory_differing(dev, host, steps)
        dev.close()
    finally:
        s.close()
    print(f"peers, {n} robots: {time.perf_counter() - t0:.1f} s")


def test_peers_lane_list_overflows():
    cfg, routes, route_of, starts, i0, peers = large_group_fleet()
    _peers_run(cfg, routes, route_of, starts, i0, 0, peers, 3, reach_overflow)


def test_peers_at_three_steps_taken():
    cfg, routes, route_of, starts, i0, K, peers = peers_s3_fleet()
    assert cfg.num_steps_taken == 3 and cfg.N_hor == 20            # the shifted plan's clamp holds for stages 17, 18 and 19
    _peers_run(cfg, routes, route_of, starts, i0, K, peers, 4, lambda host: None)


def test_nan_pose_is_one_robots_own_affair():
    """Every other robot keeps the mirror's bits in all arrays; the NaN robot takes the window's first sample like the mirror, its
    parameter vector is the mirror's with NaN = NaN, and it is not done.  (What the solve makes of a NaN is
    tests/test_gpu_parity.py::test_non_finite_inputs_are_contained's subject: its U, Y and status are not compared.)"""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, VectorizedRecedingHorizon
    c = _nan_pose()
    o = oracle_for(c.cfg)
    keep = np.arange(len(c.starts)) != NAN_ROBOT
    sn = c.cfg.num_steps_taken
    s = BatchSolver(c.cfg, max_batch=16)
    try:
        dev = DeviceRecedingHorizon(s, c.route, c.starts, c.dyn, max_steps=c.steps, idx0=c.idx0)
        host = VectorizedRecedingHorizon(c.route, c.starts, c.dyn, sincos=o.sincos_array, idx0=c.idx0)
        for k in range(c.steps):
            before = host.idx.copy()
            dev.step()
            P, st = host.step(o.warm_solve(threads=16))
            Pd, Ud, Yd = dev.params()
            state, last_u, idx, done, std = dev.read()
            pairs = [("P", Pd, P), ("U", Ud, host.U), ("Y", Yd, host.Y), ("state", state, host.state), ("last_u", last_u, host.last_u),
                     ("done", done, host.done)] + [(f, std[f], st[f]) for f in ("num_inner_iterations", "exit_status")]
            bad = [n for n, x, y in pairs if not np.array_equal(x[keep], y[keep])]
            assert not bad, f"step {k}: {bad}"
            assert np.array_equal(idx, host.idx) and idx[NAN_ROBOT] == max(0, before[NAN_ROBOT] - sn) > 0, f"step {k}"
            assert np.isnan(Pd[NAN_ROBOT, 0]) and np.array_equal(Pd[NAN_ROBOT], P[NAN_ROBOT], equal_nan=True), \
                f"step {k}: columns {np.nonzero(~((Pd[NAN_ROBOT] == P[NAN_ROBOT]) | (np.isnan(Pd[NAN_ROBOT]) & np.isnan(P[NAN_ROBOT]))))[0][:10]}"
            assert not done[NAN_ROBOT] and not host.done[NAN_ROBOT]
        T, Th = dev.trajectory(), np.stack(host.traj)
        assert T.shape == Th.shape and np.array_equal(T[:, keep], Th[:, keep])
        dev.close()
    finally:
        s.close()
