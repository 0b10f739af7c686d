"""GPU: the disturbed plant of the on-device loop (nmpc_loop_set_plant, nmpc_loop_plant_applied, nmpc_loop_plant_measured;
``nmpc_loop_measure_kernel``, ``nmpc_loop_plant_kernel``; csrc/nmpc_rng.h) against its host mirror
``FleetRecedingHorizon(..., plant=Plant(...))`` -- itself pinned to the literal rule by tests/test_plant_mirror.py -- driven by the oracle
and given the kernels' sin / cos.  After EVERY step the loop's arrays (``step_differing``) and what the plant keeps (``plant_differing``:
the controls that acted and the measured poses) must be the mirror's bits, and at the end the trajectory.

What each case (``test_log_mirror.log_fleet``) makes the kernels do:

* ``one-robot``: B = 1, every channel drawn.
* ``cfg1-three-routes``: B = 12, s = 1, actuation noise only: a partial wave, the measure kernel not launched.
* ``cfg2-s3``: N_hor = 40, s = 3, process noise only: three rows per step, so a counter keyed by the step instead of the row differs.
* ``cfg4-ellipses-retire``: measurement noise with the drive log and the clearance monitor on: the log holds the commanded controls,
  its length and the monitor see the true rows; robots retire, their measured poses stay.
* ``staggered-peers``: measurement noise: the peers' predictions start from the measured poses.
* ``missions-3-legs``: every channel across leg boundaries.
* ``group300``: two workgroups of both kernels, the second with a partial wave.
* ``crowd``: measurement noise under a watched crowd: the crowd's choice reads predictions from the measured pose, its observer the
  true rows.
* ``ids``: the device loop over the second half of a fleet with its ids against those rows of the whole fleet's mirror."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.workloads import clearance_differing, log_differing, plant_differing, step_differing, trajectory_differing
from test_crowd_mirror import fleet12, scattered
from test_log_mirror import log_fleet
from test_plant_mirror import PLANT_FLEETS, mirror_of, plant_of, plant_steps

pytestmark = pytest.mark.gpu

CASE_PLANT = {"one-robot": "all", "cfg1-three-routes": "actuation", "cfg2-s3": "process", "cfg4-ellipses-retire": "measurement",
              "staggered-peers": "measurement", "missions-3-legs": "all", "group300": "all"}
MISSION_STEPS = 40       # enough for the first leg boundaries (tests/test_plant_mirror.py drives the missions longer)


_LOOPS = []              # the device loops a test has made: closed before their solvers, whatever the test's end (a loop outlives no handle)


def _opened(dev):
    _LOOPS.append(dev)
    return dev


def _close(*solvers):
    while _LOOPS:
        _LOOPS.pop().close()
    for s in solvers:
        s.close()


def _device_of(s, f, plant, max_steps, **more):
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    return _opened(DeviceRecedingHorizon(s, f["routes"], f["starts"], f["dyn"], max_steps=max_steps, route_of=f["route_of"], idx0=f["idx0"],
                                         sinus_object=f["sinus"], peers=f["peers"], retire=f["retire"], missions=f["missions"], plant=plant,
                                         **more))


@pytest.mark.parametrize("which", PLANT_FLEETS)
def test_planted_loop_equals_host_mirror(which):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DriveLog, Monitor
    f = log_fleet(which)
    cfg, B = f["cfg"], len(f["starts"])
    o = oracle_for(cfg, **f["opts"])
    plant = plant_of(CASE_PLANT[which])
    watched = which == "cfg4-ellipses-retire"
    more = dict(log=DriveLog(), monitor=Monitor(group_of=f["route_of"])) if watched else {}
    steps = min(plant_steps(f), MISSION_STEPS)
    s = BatchSolver(cfg, max_batch=B, **f["opts"])
    try:
        dev, host = _device_of(s, f, plant, steps, **more), mirror_of(f, o, plant, **more)
        assert not plant_differing(dev, host)                              # before the first step: the start states, no rows
        while host.steps < steps and host.n_active > 0:
            bad = step_differing(dev, host, o.warm_solve(threads=16))[0] + plant_differing(dev, host)
            if watched:
                bad += log_differing(dev, host) + clearance_differing(dev, host)
            assert not bad, f"step {host.steps}: {bad}"
        assert not trajectory_differing(dev, host, host.steps)
        acted, told, U = dev.applied(), dev.measured(), dev.params()[1]
    finally:
        _close(s)
    print(which, CASE_PLANT[which], "steps", host.steps, "largest |acted - commanded v|",
          float(np.abs(acted[-cfg.num_steps_taken:, :, 0] - U[:, 0:2 * cfg.num_steps_taken:2].T).max()), "largest |measured - true|",
          float(np.abs(told - host.traj[-cfg.num_steps_taken - 1]).max()))
    assert acted.shape == (host.steps * cfg.num_steps_taken, B, 2)
    if any(plant.meas):
        drove = np.ones(B, dtype=bool) if host.active is None else host.retired_at < 0
        assert (told[drove] != host.traj[-cfg.num_steps_taken - 1][drove]).any()
    if watched:
        assert (host.retired_at >= 0).any() and (host.retired_at < 0).any()
    if f["missions"] is not None:
        assert (host.leg_at >= 0).sum() >= 3


def test_planted_loop_with_a_crowd_equals_host_mirror():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import Crowd, DeviceRecedingHorizon, FleetRecedingHorizon
    cfg = named_config("cfg4")
    routes, route_of, starts, i0, dyn = fleet12(cfg, 1)
    obs, sinus = scattered(cfg, 70)
    crowd, plant, steps = Crowd(obs, 2, 8.0, sinus=sinus, watch=True), plant_of("measurement"), 5
    o = oracle_for(cfg)
    s = BatchSolver(cfg, max_batch=len(starts))
    try:
        dev = _opened(DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=steps, route_of=route_of, idx0=i0, crowd=crowd, plant=plant))
        host = FleetRecedingHorizon(routes, route_of, starts, dyn, sincos=o.sincos_array, idx0=i0, crowd=crowd, plant=plant)
        for k in range(steps):
            bad = step_differing(dev, host, o.warm_solve(threads=16))[0] + plant_differing(dev, host)
            assert not bad, f"step {k}: {bad}"
            assert np.array_equal(dev.crowd_seen(), host.crowd_seen), k
            got, want = dev.crowd_clearance(), host.crowd_clearance()
            assert all(got[n].tobytes() == want[n].tobytes() for n in got.dtype.names), k
        assert not trajectory_differing(dev, host, steps)
        assert (host.crowd_seen >= 0).any()
    finally:
        _close(s)


def test_ids_give_a_half_fleet_the_whole_fleets_disturbances():
    """The device loop over robots 6 .. 11 with ids = 6 .. 11 against rows 6 .. 11 of the mirror of all 12."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    f = log_fleet("cfg1-three-routes")
    cfg, o, steps = f["cfg"], oracle_for(f["cfg"]), 5
    half = {**f, **dict(route_of=f["route_of"][6:], starts=f["starts"][6:], idx0=f["idx0"][6:])}
    host = mirror_of(f, o, plant_of("all"))
    s = BatchSolver(cfg, max_batch=6)
    try:
        dev = _device_of(s, half, plant_of("all", ids=np.arange(6, 12)), steps)
        for k in range(steps):
            dev.step()
            host.step(o.warm_solve(threads=16))
            pairs = [("P", dev.params()[0], host._P_step), ("state", dev.read()[0], host.state), ("applied", dev.applied(), host.applied()),
                     ("measured", dev.measured(), host.measured())]
            bad = [n for n, a, b in pairs if a.tobytes() != np.ascontiguousarray(b[..., 6:, :]).tobytes()]
            assert not bad, f"step {k}: {bad}"
        assert dev.trajectory().tobytes() == np.ascontiguousarray(np.stack(host.traj)[:, 6:]).tobytes()
    finally:
        _close(s)


def test_plant_of_zeros_is_the_loop_without_a_plant():
    """Two device loops over one fleet (scripted ellipses, retirement), one with ``Plant()``: equal bit for bit over five steps."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import Plant
    f = log_fleet("cfg4-ellipses-retire")
    cfg, B, steps = f["cfg"], len(f["starts"]), 5
    s1, s2 = BatchSolver(cfg, max_batch=B), BatchSolver(cfg, max_batch=B)
    try:
        a, b = _device_of(s1, f, Plant(keep_applied=True), steps), _device_of(s2, f, None, steps)
        for k in range(steps):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert x.tobytes() == y.tobytes(), f"step {k}"
            sa, sb = a.read()[4], b.read()[4]
            for n in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "penalty"):
                assert np.array_equal(sa[n], sb[n]), (k, n)
            assert a.trajectory().tobytes() == b.trajectory().tobytes(), f"step {k}"
            assert a.measured().tobytes() == b.measured().tobytes() == a.params()[0][:, 0:3].tobytes()
        assert a.applied().shape == (steps * cfg.num_steps_taken, B, 2) and b.applied().shape == (0, B, 2)
    finally:
        _close(s1, s2)


def test_plant_arguments_validated():
    """A negative sigma, a call after the first step and ``keep_applied`` with ``max_steps`` = 0: NMPC_ERR_BAD_ARG with a message that
    names the function, and the loop steps as before: its bits are those of a loop that was never asked."""
    from mpc_trajectory_generator_amd import _lib
    from mpc_trajectory_generator_amd.solver import BatchSolver
    f = log_fleet("cfg1-three-routes")
    cfg, B = f["cfg"], len(f["starts"])
    s1, s2 = BatchSolver(cfg, max_batch=B), BatchSolver(cfg, max_batch=B)
    lib = s1.lib

    def asked(dev, **fields):
        pl = _lib.NmpcPlant()
        for name, v in fields.items():
            setattr(pl, name, v if isinstance(v, int) else (C.c_double * len(v))(*v))
        rc = lib.nmpc_loop_set_plant(dev._l, C.byref(pl), None)
        msg = lib.nmpc_last_error(s1._h).decode()
        assert rc == -3 and "nmpc_loop_set_plant" in msg, (rc, msg)
        return msg

    try:
        assert lib.nmpc_loop_set_plant(None, None, None) == -3
        a, ref = _device_of(s1, f, None, 3), _device_of(s2, f, None, 3)
        assert lib.nmpc_loop_set_plant(a._l, None, None) == -3 and "plant is NULL" in lib.nmpc_last_error(s1._h).decode()
        asked(a, proc=(0.0, -0.001, 0.0))
        asked(a, meas=(float("nan"), 0.0, 0.0))
        asked(a, act_gain=(float("inf"), 0.0))
        a.step()
        ref.step()
        assert "step" in asked(a, proc=(0.001, 0.001, 0.001))
        a.step()
        ref.step()
        for x, y in zip(a.params() + a.read()[:4] + (a.trajectory(),), ref.params() + ref.read()[:4] + (ref.trajectory(),)):
            assert x.tobytes() == y.tobytes()
        assert a.applied().shape == (0, B, 2)
        a.close()
        ref.close()
        b, ref = _device_of(s1, f, None, 0), _device_of(s2, f, None, 0)          # max_steps = 0
        assert "max_steps" in asked(b, keep_applied=1)
        b.step()
        ref.step()
        for x, y in zip(b.params() + b.read()[:4], ref.params() + ref.read()[:4]):
            assert x.tobytes() == y.tobytes()
        pl = _lib.NmpcPlant(seed=3, proc=(C.c_double * 3)(0.001, 0.001, 0.0))
        c = _device_of(s1, f, None, 0)
        assert lib.nmpc_loop_set_plant(c._l, C.byref(pl), None) == 0            # without keep_applied a loop of max_steps = 0 takes a plant
        assert "already" in asked(c, seed=4)
        c.step()
        assert not np.array_equal(c.read()[0], ref.read()[0])
    finally:
        _close(s1, s2)
