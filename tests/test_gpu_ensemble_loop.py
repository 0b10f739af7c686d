"""GPU: the ensemble stage of the on-device loop (nmpc_loop_set_ensemble, nmpc_loop_ensemble, nmpc_loop_ensemble_groups;
``nmpc_loop_ensemble_kernel``) against its host mirror ``FleetRecedingHorizon(..., ensemble=Ensemble(...))`` --
itself pinned to the literal rule by tests/test_ensemble_mirror.py -- driven by the oracle and given the kernels' sin / cos, under the
plant of tests/test_plant_mirror.py so that the members of a group differ.  After EVERY step the loop's arrays (``step_differing``) and
the records of all steps so far (``ensemble_differing``) must be the mirror's bits, and at the end the trajectory.

What each case (``test_ensemble_mirror.ensemble_case``) makes the kernel do:

* ``one-robot``: B = 1, one workgroup with 255 idle threads, three waves without a member.
* ``cfg1-three-routes``, groups = 4: B = 12, members 4 + 4 + 4 in a partial wave and the workgroup of an empty group.
* ``cfg2-s3``: N_hor = 40, s = 3: one record per step, not per trajectory row.
* ``cfg4-ellipses-retire`` with the drive log and the monitor on: the compaction runs in front of the kernel, ``arrived`` comes from
  ``retired_at``, and the last steps drive few robots.
* ``missions-3-legs``: the dispatch runs in front of the kernel: a robot sent on to its next leg is not counted.
* ``group300``: ``group_of = b % 2``, two groups of 150 whose members are not contiguous, three waves of which the last is partial;
  and on a second loop one group of all 300: the stride loop is taken twice by 44 threads and once by the others.
* identical copies, no plant: every member as far from the mean as every other, so the furthest is decided by the index alone.

Then: the loop with and without the stage, bit for bit; and every refusal through the raw ABI."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd.workloads import (clearance_differing, ensemble_differing, log_differing, step_differing,
                                                    trajectory_differing)
from test_ensemble_mirror import ensemble_case
from test_log_mirror import log_fleet
from test_plant_mirror import mirror_of, plant_of

pytestmark = pytest.mark.gpu

STEPS = {"one-robot": 3, "cfg1-three-routes": 4, "cfg2-s3": 3, "cfg4-ellipses-retire": 40, "missions-3-legs": 40, "group300": 3}

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


@pytest.mark.parametrize("which", list(STEPS))
def test_ensemble_loop_equals_host_mirror(which):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DriveLog, Ensemble, Monitor
    f, ens = ensemble_case(which)
    cfg, B = f["cfg"], len(f["starts"])
    o = oracle_for(cfg, **f["opts"])
    plant, steps = plant_of("all"), STEPS[which]
    watched = which == "cfg4-ellipses-retire"
    more = dict(log=DriveLog(), monitor=Monitor(group_of=f["route_of"])) if watched else {}
    whole = which == "group300"                                            # a second loop: everybody in one group
    s, s2 = BatchSolver(cfg, max_batch=B, **f["opts"]), (BatchSolver(cfg, max_batch=B, **f["opts"]) if whole else None)
    try:
        dev, host = _device_of(s, f, plant, steps, ensemble=ens, **more), mirror_of(f, o, plant, ensemble=ens, **more)
        G = ens.checked(B)[1]
        assert s.lib.nmpc_loop_ensemble_groups(dev._l) == G and dev.ensemble_stats().shape == (0, G)
        if whole:
            dev2, host2 = _device_of(s2, f, plant, steps, ensemble=Ensemble()), mirror_of(f, o, plant, ensemble=Ensemble())
        partly = False
        while host.steps < steps and host.n_active > 0:
            bad = step_differing(dev, host, o.warm_solve(threads=16))[0] + ensemble_differing(dev, host)
            if watched:
                bad += log_differing(dev, host) + clearance_differing(dev, host)
            if whole:
                bad += step_differing(dev2, host2, o.warm_solve(threads=16))[0] + ensemble_differing(dev2, host2)
            assert not bad, f"step {host.steps}: {bad}"
            last = host.ensemble_stats()[-1]
            partly |= bool((0 < last["arrived"][0] < last["n"][0]))
        assert not trajectory_differing(dev, host, host.steps)
        st = dev.ensemble_stats()
    finally:
        _close(*(x for x in (s, s2) if x is not None))
    print(which, "steps", host.steps, "groups", G, "n", st["n"][-1].tolist(), "arrived", st["arrived"][-1].tolist(),
          "largest sd", float(np.sqrt(st["cov"][-1].max())), "furthest", st["far_robot"][-1].tolist())
    assert st.shape == (host.steps, G) and host.steps > 0 and (st["n"].sum(axis=1) == B).all()
    if which == "cfg1-three-routes":
        assert (st["n"][:, 3] == 0).all() and (st["far_robot"][:, 3] == -1).all()
    if watched:
        assert partly and (host.retired_at >= 0).any()
    if f["missions"] is not None:
        assert (host.leg_at >= 0).sum() >= 3
    if whole:
        assert (st["n"] == 150).all() and (host2.ensemble_stats()["n"] == 300).all()


def test_identical_copies_tie_to_the_first_member():
    """300 copies of one robot without a plant, ``group_of = b % 2``: every member of a group is equally far from the mean, within a
    thread, across the lanes of a wave and across the waves, so ``far_robot`` is decided by the index alone: the group's first member."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import Ensemble
    from mpc_trajectory_generator_amd.workloads import ensemble_fleet
    f = log_fleet("one-robot")
    cfg, o, B, steps = f["cfg"], oracle_for(f["cfg"]), 300, 2
    routes, route_of, starts, i0 = ensemble_fleet(f["routes"][0], f["starts"][0], B, f["idx0"][0])
    copies = {**f, **dict(routes=routes, route_of=route_of, starts=starts, idx0=i0, dyn=tuple(np.repeat(a[:1], B, axis=0) for a in f["dyn"]))}
    ens = Ensemble(np.arange(B) % 2)
    s = BatchSolver(cfg, max_batch=B)
    try:
        dev, host = _device_of(s, copies, None, steps, ensemble=ens), mirror_of(copies, o, None, ensemble=ens)
        for k in range(steps):
            bad = step_differing(dev, host, o.warm_solve(threads=16))[0] + ensemble_differing(dev, host)
            assert not bad, f"step {k}: {bad}"
        st = dev.ensemble_stats()
    finally:
        _close(s)
    assert (st["n"] == 150).all() and (st["far_robot"] == np.arange(2)).all()
    assert (st["far2"] == st["far2"][:, :1]).all() and (st["far2"] >= 0).all()


def test_the_stage_observes_only():
    """Two device loops over one fleet, one with the stage: params, read and the trajectory equal bit for bit over three steps."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    f, ens = ensemble_case("cfg1-three-routes")
    cfg, B, steps = f["cfg"], len(f["starts"]), 3
    s1, s2 = BatchSolver(cfg, max_batch=B), BatchSolver(cfg, max_batch=B)
    try:
        a, b = _device_of(s1, f, plant_of("all"), steps, ensemble=ens), _device_of(s2, f, plant_of("all"), steps)
        for k in range(steps):
            a.step()
            b.step()
            for x, y in zip(a.params() + a.read()[:4], b.params() + b.read()[:4]):
                assert x.tobytes() == y.tobytes(), f"step {k}"
            sa, sb = a.read()[4], b.read()[4]
            for n in ("exit_status", "num_inner_iterations", "num_outer_iterations", "cost", "penalty"):
                assert np.array_equal(sa[n], sb[n]), (k, n)
            assert a.trajectory().tobytes() == b.trajectory().tobytes(), f"step {k}"
        assert a.ensemble_stats().shape == (steps, 4) and b.ensemble_stats().shape == (0, 1)
    finally:
        _close(s1, s2)


def test_ensemble_arguments_validated():
    """Every refusal is NMPC_ERR_BAD_ARG with a message that names the function, leaves nmpc_loop_ensemble_groups as it was, and the
    loop steps as before: its bits are those of a loop that was never asked."""
    from mpc_trajectory_generator_amd import _lib
    from mpc_trajectory_generator_amd.solver import BatchSolver
    f = log_fleet("cfg1-three-routes")
    cfg, B = f["cfg"], len(f["starts"])
    s1, s2 = BatchSolver(cfg, max_batch=B), BatchSolver(cfg, max_batch=B)
    lib = s1.lib

    def i32(v):
        return np.ascontiguousarray(v, dtype=np.int32)

    def refused(dev, group_of, G, groups_before=0):
        rc = lib.nmpc_loop_set_ensemble(dev._l, None if group_of is None else _lib.as_i32p(group_of), G)
        msg = lib.nmpc_last_error(s1._h).decode()
        assert rc == -3 and "nmpc_loop_set_ensemble" in msg, (rc, msg)
        assert lib.nmpc_loop_ensemble_groups(dev._l) == groups_before
        return msg

    def same(a, ref):
        for x, y in zip(a.params() + a.read()[:4], ref.params() + ref.read()[:4]):
            assert x.tobytes() == y.tobytes()

    try:
        assert lib.nmpc_loop_set_ensemble(None, None, 1) == -3 and lib.nmpc_loop_ensemble(None, None, 0) == -3
        assert lib.nmpc_loop_ensemble_groups(None) == 0
        a, ref = _device_of(s1, f, None, 3), _device_of(s2, f, None, 3)
        zeros = i32(np.zeros(B))
        refused(a, zeros, 0)
        refused(a, zeros, 65537)
        refused(a, None, 2)
        refused(a, i32([0] * (B - 1) + [2]), 2)                            # an id = G
        refused(a, i32([0, -1] + [0] * (B - 2)), 2)                        # a negative id
        # a loop without the stage: 0 steps, nothing written
        canary = np.full(80, 0x5A, dtype=np.uint8)
        a.step()
        ref.step()
        assert lib.nmpc_loop_ensemble(a._l, canary.ctypes.data, 1) == 0 and (canary == 0x5A).all()
        assert a.ensemble_stats().shape == (0, 1)
        assert "step" in refused(a, zeros, 1)                              # after a step
        a.step()
        ref.step()
        same(a, ref)
        assert a.trajectory().tobytes() == ref.trajectory().tobytes()
        a.close()
        b, ref0 = _device_of(s1, f, None, 0), _device_of(s2, f, None, 0)    # max_steps = 0
        assert "max_steps" in refused(b, zeros, 1)
        b.step()
        ref0.step()
        same(b, ref0)
        b.close()
        c = _device_of(s1, f, None, 3)
        assert lib.nmpc_loop_set_ensemble(c._l, _lib.as_i32p(i32(np.arange(B) % 3)), 3) == 0 and lib.nmpc_loop_ensemble_groups(c._l) == 3
        assert "already" in refused(c, zeros, 1, groups_before=3)           # a second call
        c.step()
        c.step()
        out = np.zeros((1, 3), dtype=_lib.ENSEMBLE_DTYPE)
        assert lib.nmpc_loop_ensemble(c._l, out.ctypes.data, 1) == -3 and "nmpc_loop_ensemble" in lib.nmpc_last_error(s1._h).decode()
        assert not out["n"].any()
        st = c.ensemble_stats()
        assert st.shape == (2, 3) and (st["n"] == 4).all()
        same(c, ref)                                                       # two steps each: the stage and the refusals changed no bit
    finally:
        _close(s1, s2)
