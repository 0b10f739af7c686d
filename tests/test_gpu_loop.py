"""GPU: the receding-horizon loop on device (nmpc_loop_*) against its host
mirror.  The mirror is ``VectorizedRecedingHorizon`` -- itself pinned to ``BatchedRecedingHorizon``, whose
robots run the one literal per-robot step that tests/test_harness.py pins, through that driver and through
``TrajectoryGenerator.run``, to the goldens recorded from the reference's PathGenerator.run -- driven by the
oracle and given the kernels' sin / cos, so parameter vectors, states, reference indices and solver
counters must agree bit for bit, step after step."""
import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.workloads import route_fleet, step_differing, trajectory_differing

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,scene,K,steps,sinus", [("cfg4", 11, 3, 12, False), ("cfg4", 1, 2, 40, False), ("cfg1", 11, 0, 8, False),
                                                       ("nobs3", 11, 1, 6, False), ("cfg4", 11, 3, 10, True),
                                                       ("cfg2", 11, 2, 5, False)])
def test_device_loop_equals_host_mirror(name, scene, K, steps, sinus):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, VectorizedRecedingHorizon
    # "nobs3": fewer circle slots than the scene has vertices -> the closest-vertex window is exercised; "cfg2": N_hor = 40, the
    # two-stages-per-lane kernel inside the loop
    cfg = load_config(Nobs=3) if name == "nobs3" else named_config(name)
    route = harness.scene_route(cfg, scene)
    B = 24
    i0, starts, dyn = route_fleet(route, B, 7 + scene, K)
    o = oracle_for(cfg)
    s = BatchSolver(cfg, max_batch=32)
    try:
        dev = DeviceRecedingHorizon(s, route, starts, dyn, max_steps=steps, idx0=i0, sinus_object=sinus)
        host = VectorizedRecedingHorizon(route, starts, dyn, sincos=o.sincos_array, sinus_object=sinus, idx0=i0)   # (third ellipse: sinusoidal law)
        for k in range(steps):
            bad = step_differing(dev, host, o.warm_solve())[0]
            assert not bad, f"step {k}: {bad}"
        assert not trajectory_differing(dev, host, steps)
        dev.close()
    finally:
        s.close()


def test_device_loop_reaches_goal_and_brakes():
    """Closed loop to the goal on scene 1 (reference config 0): the braking branch (velocity reference
    from the distance table inside the last sample) and the terminal test are reached on device."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon, VectorizedRecedingHorizon
    cfg = named_config("cfg1")
    route = harness.scene_route(cfg, 1)
    o = oracle_for(cfg)
    n = len(route.x_ref)
    B = 6
    i0 = np.array([n - 40, n - 30, n - 22, n - 12, n - 5, n - 2])
    xr, yr, tr = np.array(route.x_ref), np.array(route.y_ref), np.array(route.theta_ref)
    starts = np.stack([xr[i0], yr[i0], tr[i0]], axis=1)
    s = BatchSolver(cfg, max_batch=8)
    try:
        dev = DeviceRecedingHorizon(s, route, starts, None, max_steps=120, idx0=i0)
        host = VectorizedRecedingHorizon(route, starts, None, sincos=o.sincos_array, idx0=i0)
        for k in range(120):
            dev.step()
            P, st = host.step(o.warm_solve(threads=6))
            if k % 10 == 9 or k < 3:
                Pd, _, _ = dev.params()
                assert np.array_equal(Pd, P), f"step {k}"
        state, last_u, idx, done, _ = dev.read()
        assert np.array_equal(state, host.state) and np.array_equal(done, host.done)
        assert done.all()
        dev.close()
    finally:
        s.close()
