"""Three sets of vehicle constants away from the defaults, and two weight presets, for the tests that run oracle, kernels and loop
off the one point of the parameter space every other test stands on (tests/test_vehicle_constants.py, tests/test_gpu_vehicle_constants.py,
the ``fast-`` / ``slow-`` / ``fwd-`` cases of tests/test_loop_shapes_mirror.py).

* ``fast``: ts = 0.1 (1 / ts is not exact), a C box that is not symmetric in v (-2.0 / 0.7), throttle 0.8.
* ``slow``: ts = 0.35, lin_vel_min = 0 (the lower velocity bound becomes active), a narrow U, a braking table of 5 entries.
* ``fwd``: ts = 0.05, lin_vel_min = 0.2 > 0 (the cold start u = 0 lies outside U), a wide U, circle radius 0.55."""
import os

import numpy as np

VEHICLE_SETS = {
    "fast": dict(ts=0.1, lin_vel_min=-1.0, lin_vel_max=2.5, lin_acc_min=-2.0, lin_acc_max=0.7, ang_vel_max=1.3, ang_acc_max=1.1,
                 throttle_ratio=0.8),
    "slow": dict(ts=0.35, lin_vel_min=0.0, lin_vel_max=0.6, lin_acc_min=-0.4, lin_acc_max=0.4, ang_vel_max=0.25, ang_acc_max=7.0,
                 throttle_ratio=0.7, vel_red_steps=5),
    "fwd": dict(ts=0.05, lin_vel_min=0.2, lin_vel_max=4.0, lin_acc_min=-3.0, lin_acc_max=3.0, ang_vel_max=2.0, ang_acc_max=0.5,
                vehicle_width=0.8, vehicle_margin=0.15),
}

WEIGHT_PRESETS = {
    "track": dict(q=2.0, qtheta=0.5, qN=20.0, qthetaN=1.0, cte_penalty=50.0, lin_vel_penalty=0.3, ang_vel_penalty=0.7, qv=3.0,
                  lin_acc_penalty=1.0, ang_acc_penalty=40.0),
    "zeros": dict(qv=0.0, cte_penalty=0.0, lin_acc_penalty=0.0, ang_acc_penalty=0.0, qN=8.0, q=0.5),
}

# the goldens of tests/golden/make_golden.py at these sets: file stem -> (set, shape overrides)
VEHICLE_GOLDENS = {"fast": ("fast", dict(N_hor=20, Nobs=10, Ndynobs=3)),
                   "slow": ("slow", dict(N_hor=40, Nobs=10, Ndynobs=3)),
                   "fwd": ("fwd", dict(N_hor=17, Nobs=50, Ndynobs=3))}

# the kernel rows of tests/test_gpu_vehicle_constants.py: shape -> the kernel the handle must report (chosen by shape alone)
KERNEL_ROWS = {(20, 10, 3): "nmpc_solve_hyb_kernel<ShapeDefault>", (20, 50, 3): "nmpc_solve_hyb_kernel<ShapeNobs50>",
               (40, 10, 3): "nmpc_solve_hyb2_kernel<ShapeN40>", (17, 4, 1): "nmpc_solve_hyb_kernel<ShapeAny>",
               (5, 1, 3): "nmpc_solve_hyb_kernel<ShapeAny>", (33, 10, 3): "nmpc_solve_hyb2_kernel<ShapeAny>",
               (40, 0, 0): "nmpc_solve_hyb2_kernel<ShapeAny>"}


def vehicle_config(name, **shape):
    from mpc_trajectory_generator_amd.config import load_config
    return load_config(**VEHICLE_SETS[name], **shape)


def shape_config(name, shape, **more):
    N, nobs, ndyn = shape
    return vehicle_config(name, N_hor=N, Nobs=nobs, Ndynobs=ndyn, **more)


def load_vehicle_golden(stem):
    """-> (npz, cfg) of tests/golden/cost_<stem>.npz."""
    name, shape = VEHICLE_GOLDENS[stem]
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"cost_{stem}.npz"))
    return d, vehicle_config(name, **shape)


def solve_seed(name, shape):
    """The seed of the batch ``solve_batch_of`` builds: one per (set, shape)."""
    N, nobs, ndyn = shape
    return 4000 + 1000 * list(VEHICLE_SETS).index(name) + 7 * N + nobs + ndyn


def solve_batch_of(name, shape, B=24, **more):
    """-> (cfg, P): the batch the GPU module solves cold at (set, shape), and the CPU module asserts the reach of."""
    from mpc_trajectory_generator_amd.harness import synthetic_batch
    cfg = shape_config(name, shape, **more)
    P = synthetic_batch(cfg, 11, B, solve_seed(name, shape), random_dyn=shape[2] > 0, synthetic_circles=shape[1] == 50)
    return cfg, P
