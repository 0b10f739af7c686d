"""ctypes binding of libnmpc_hip.so (the C ABI of include/nmpc_solver.h).

There is no CPU fallback: if the HIP library is missing it is built with hipcc, and if that is
impossible or no MI355X is visible the constructor of the solver raises.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libnmpc_hip.so")
BUILD_INFO = os.path.join(_CSRC, "build_info.json")      # written by build_library: flags, codegen check, registers / LDS / scratch per kernel

# every symbol include/nmpc_solver.h declares
SYMBOLS = (
    "nmpc_default_opts", "nmpc_n_u", "nmpc_n_p", "nmpc_n1", "nmpc_n2", "nmpc_new", "nmpc_free",
    "nmpc_ping", "nmpc_last_error", "nmpc_abi_version", "nmpc_experiments_build", "nmpc_kernel_name", "nmpc_cull_radius", "nmpc_launch_geometry", "nmpc_solve_batch_device",
    "nmpc_solve_batch_host", "nmpc_last_batch_ms", "nmpc_set_time_limits", "nmpc_eval_batch_device", "nmpc_eval_batch_host",
    "nmpc_test_sincos_host", "nmpc_test_divsqrt_host",
    "nmpc_loop_new", "nmpc_loop_new_routes", "nmpc_loop_set_peers", "nmpc_loop_free", "nmpc_loop_step", "nmpc_loop_read", "nmpc_loop_params",
    "nmpc_loop_trajectory", "nmpc_loop_set_retire", "nmpc_loop_active", "nmpc_loop_run", "nmpc_loop_set_monitor", "nmpc_loop_clearance",
    "nmpc_loop_set_missions", "nmpc_loop_legs", "nmpc_loop_set_map_monitor", "nmpc_loop_map_clearance",
    "nmpc_loop_set_peers_grid", "nmpc_loop_peer_grid",
    "nmpc_loop_set_log", "nmpc_loop_log", "nmpc_loop_drive_summary", "nmpc_loop_step_totals",
    "nmpc_loop_set_crowd", "nmpc_loop_crowd", "nmpc_loop_set_crowd_monitor", "nmpc_loop_crowd_clearance",
    "nmpc_loop_set_crowd_grid", "nmpc_loop_crowd_grid",
    "nmpc_loop_set_plant", "nmpc_loop_plant_applied", "nmpc_loop_plant_measured",
    "nmpc_loop_set_ensemble", "nmpc_loop_ensemble", "nmpc_loop_ensemble_groups",
    "nmpc_loop_set_walls", "nmpc_loop_walls", "nmpc_loop_set_walls_grid", "nmpc_loop_wall_grid",
    "nmpc_loop_set_map_monitor_grid", "nmpc_loop_map_grid",
    "nmpc_loop_set_track_monitor", "nmpc_loop_tracking",
    "nmpc_planner_new", "nmpc_planner_free", "nmpc_planner_visibility", "nmpc_plan_batch_device", "nmpc_plan_batch_host", "nmpc_planner_last_ms",
)

EXPECTED_ABI = 3      # the nmpc_opts / nmpc_status layouts below are written for this version of include/nmpc_solver.h

ERRORS = {0: "ok", -1: "bad problem", -2: "bad opts", -3: "bad argument", -4: "no HIP device",
          -5: "HIP runtime error", -6: "dead handle"}

EXIT_STATUS = ("Converged", "NotConvergedIterations", "NotConvergedOutOfTime", "NotConvergedCost",
               "NotConvergedNotFiniteComputation")


class NmpcProblem(C.Structure):
    _fields_ = [("N", C.c_int32), ("nobs", C.c_int32), ("ndyn", C.c_int32), ("reserved", C.c_int32),
                ("ts", C.c_double), ("vmin", C.c_double), ("vmax", C.c_double), ("wmax", C.c_double),
                ("amin", C.c_double), ("amax", C.c_double), ("awmax", C.c_double)]


class NmpcOpts(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("initial_tolerance", C.c_double),
                ("delta_tolerance", C.c_double), ("initial_penalty", C.c_double),
                ("penalty_update", C.c_double), ("tolerance_update", C.c_double),
                ("sufficient_decrease", C.c_double), ("lbfgs_memory", C.c_int32),
                ("max_inner", C.c_int32), ("max_outer", C.c_int32), ("max_total_inner", C.c_int32),
                ("akkt_gradient", C.c_int32), ("ls_failure", C.c_int32), ("inner_status", C.c_int32),
                ("reserved", C.c_int32)]

# the restatement switches (include/nmpc_solver.h) and what their values mean
VARIANT_FIELDS = {
    "akkt_gradient": ("per_trial", "step_top", "off"),
    "ls_failure": ("take_last_trial", "tau0_fb_step"),
    "inner_status": ("propagate_inner", "converged_if_outer_ok"),
}


class NmpcRoute(C.Structure):
    _dp = C.POINTER(C.c_double)
    _fields_ = [("n_ref", C.c_int32), ("n_vert", C.c_int32), ("n_brake", C.c_int32), ("num_steps_taken", C.c_int32),
                ("x_ref", _dp), ("y_ref", _dp), ("theta_ref", _dp), ("vert_xy", _dp),
                ("brake_vel", _dp), ("brake_dist", _dp),
                ("end", C.c_double * 3), ("base_speed", C.c_double), ("radius", C.c_double),
                ("dyn_pad", C.c_double), ("weights", C.c_double * 10)]


class NmpcScene(C.Structure):
    _fields_ = [("n_node", C.c_int32), ("n_edge", C.c_int32), ("n_poly", C.c_int32), ("reserved", C.c_int32),
                ("node_xy", C.POINTER(C.c_double)), ("edge", C.POINTER(C.c_double)), ("poly_off", C.POINTER(C.c_int32))]


class NmpcPlant(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("act_gain", C.c_double * 2), ("act_add", C.c_double * 2), ("proc", C.c_double * 3),
                ("meas", C.c_double * 3), ("keep_applied", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(NmpcPlant) == 96


class NmpcLaunchInfo(C.Structure):
    _fields_ = [("grid", C.c_int32), ("owners", C.c_int32), ("workgroups", C.c_int32), ("ordered", C.c_int32), ("pools", C.c_int32),
                ("pool_cap", C.c_int32), ("resident_waves", C.c_int32), ("reserved", C.c_int32), ("staging_chunk_bytes", C.c_int64)]


assert C.sizeof(NmpcLaunchInfo) == 40

STATUS_DTYPE = np.dtype([("exit_status", "<i4"), ("num_outer_iterations", "<u4"),
                         ("num_inner_iterations", "<u4"), ("num_cost_evals", "<u4"),
                         ("num_grad_evals", "<u4"), ("reserved", "<u4"),
                         ("last_problem_norm_fpr", "<f8"), ("delta_y_norm_over_c", "<f8"),
                         ("f2_norm", "<f8"), ("penalty", "<f8"), ("cost", "<f8"),
                         ("solve_time_ms", "<f8")])
assert STATUS_DTYPE.itemsize == 72

# nmpc_clearance: a robot's closest approaches and the trajectory rows they happened at (nmpc_loop_set_monitor)
CLEARANCE_DTYPE = np.dtype([("circle", "<f8"), ("ellipse", "<f8"), ("peer2", "<f8"),
                            ("circle_row", "<i4"), ("ellipse_row", "<i4"), ("peer_row", "<i4"), ("peer", "<i4")])
assert CLEARANCE_DTYPE.itemsize == 40

# nmpc_map_clearance: a robot's closest approach to the map's walls and the rows at which a polygon failed (nmpc_loop_set_map_monitor)
MAP_CLEARANCE_DTYPE = np.dtype([("wall2", "<f8"), ("wall_row", "<i4"), ("wall_edge", "<i4"), ("hits", "<i4"),
                                ("hit_row", "<i4"), ("hit_poly", "<i4"), ("reserved", "<i4")])
assert MAP_CLEARANCE_DTYPE.itemsize == 32

# nmpc_tracking: how far a robot was from its route, in position and heading, and the rows at which (nmpc_loop_set_track_monitor)
TRACKING_DTYPE = np.dtype([("cte2_max", "<f8"), ("cte2_sum", "<f8"), ("dth_max", "<f8"), ("dth2_sum", "<f8"),
                           ("rows", "<i4"), ("cte_row", "<i4"), ("cte_seg", "<i4"), ("dth_row", "<i4"), ("last_seg", "<i4"),
                           ("off_rows", "<i4"), ("off_row", "<i4"), ("reserved", "<i4")])
assert TRACKING_DTYPE.itemsize == 64

# nmpc_peer_grid: the grid the peers of a step were found through (nmpc_loop_set_peers_grid)
PEER_GRID_DTYPE = np.dtype([("origin", "<f8", 2), ("h", "<f8", 2), ("W", "<f8", 2), ("nx", "<i4"), ("ny", "<i4"), ("filed", "<i4"), ("reserved", "<i4")])
assert PEER_GRID_DTYPE.itemsize == 64

# nmpc_wall_grid: the grid the walls' edges are found through (nmpc_loop_set_walls_grid)
WALL_GRID_DTYPE = np.dtype([("origin", "<f8", 2), ("h", "<f8", 2), ("nx", "<i4"), ("ny", "<i4"), ("entries", "<i4"), ("reserved", "<i4")])
assert WALL_GRID_DTYPE.itemsize == 48

# nmpc_crowd_grid: the grid in space and stage the crowd's obstacles are found through (nmpc_loop_set_crowd_grid)
CROWD_GRID_DTYPE = np.dtype([("origin", "<f8", 2), ("h", "<f8", 2), ("nx", "<i4"), ("ny", "<i4"), ("layers", "<i4"), ("filed", "<i4")])
assert CROWD_GRID_DTYPE.itemsize == 48

# the drive log (nmpc_loop_set_log): nmpc_step_record, one per robot and step; nmpc_drive_summary, one per robot; nmpc_step_totals, one per step
STEP_RECORD_DTYPE = np.dtype([("exit_status", "<i4"), ("leg", "<i4"), ("num_inner_iterations", "<u4"), ("num_outer_iterations", "<u4"),
                              ("cost", "<f8"), ("f2_norm", "<f8"), ("solve_time_ms", "<f8")])
assert STEP_RECORD_DTYPE.itemsize == 40
DRIVE_SUMMARY_DTYPE = np.dtype([("steps", "<i4"), ("rows", "<i4"), ("exits", "<u4", 5), ("inner_max", "<u4"), ("inner_total", "<u8"),
                                ("inner_max_step", "<i4"), ("f2_max_step", "<i4"), ("length", "<f8"), ("v_abs_max", "<f8"),
                                ("w_abs_max", "<f8"), ("acc_abs_max", "<f8"), ("wacc_abs_max", "<f8"), ("acc_sq_sum", "<f8"),
                                ("wacc_sq_sum", "<f8"), ("f2_max", "<f8")])
assert DRIVE_SUMMARY_DTYPE.itemsize == 112
STEP_TOTALS_DTYPE = np.dtype([("solved", "<i4"), ("exits", "<u4", 5), ("inner_max", "<u4"), ("inner_max_robot", "<i4"),
                              ("inner_total", "<u8"), ("solve_ms_max", "<f8")])
assert STEP_TOTALS_DTYPE.itemsize == 48

# nmpc_crowd_clearance: a robot's closest approach to any obstacle of the crowd (nmpc_loop_set_crowd_monitor)
CROWD_CLEARANCE_DTYPE = np.dtype([("level", "<f8"), ("row", "<i4"), ("obstacle", "<i4")])
assert CROWD_CLEARANCE_DTYPE.itemsize == 16

# nmpc_ensemble_stat: a group's pose statistics after one step (nmpc_loop_set_ensemble)
ENSEMBLE_DTYPE = np.dtype([("n", "<i4"), ("arrived", "<i4"), ("far_robot", "<i4"), ("reserved", "<i4"),
                           ("mean", "<f8", 3), ("cov", "<f8", 4), ("far2", "<f8")])
assert ENSEMBLE_DTYPE.itemsize == 80


def _sources():
    srcs = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".hip", ".h")) or f == "Makefile"]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "nmpc_solver.h"))
    return srcs


def source_hash() -> str:
    """sha256 over the kernel sources: the key profiles/*/traffic.json files are stored under, so that a
    PMC figure measured on one version of the kernels is never quoted for another."""
    import hashlib
    h = hashlib.sha256()
    for s in _sources():
        if not s.endswith("Makefile"):
            with open(s, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


# Every library built from these sources: name -> the csrc/Makefile variables it sets.  PRODUCT is the shipped csrc/libnmpc_hip.so; the others
# go to csrc/variants/libnmpc_<name>.so: the other scheduler strategies (tests/test_gpu_strategies.py: a kernel whose results depend on the
# schedule has a defect, or the compiler has), the experiments build (the only one with the environment knobs of tests and scripts), win0 (the
# cross-track search always as the full scan; tests demand the shipped bits from it) and, ON_DEMAND only, the instrumented builds of scripts/.
PRODUCT, EXPERIMENTS = "product", "experiments"
LIBRARIES = {
    PRODUCT: {},
    "default": {"SCHED": ""},
    "max-memory-clause": {"SCHED": "-mllvm -amdgpu-sched-strategy=max-memory-clause"},
    "max-ilp": {"SCHED": "-mllvm -amdgpu-sched-strategy=max-ilp"},
    EXPERIMENTS: {"EXTRA": "-DNMPC_EXPERIMENTS"},
    "win0": {"EXTRA": "-DNMPC_WIN=0 -DNMPC_WIN2=0"},
    "ws": {"EXTRA": "-DNMPC_WIN_STATS -DNMPC_EXPERIMENTS"},       # certificate fall-back shares (scripts/win_stats.py)
    "prof2": {"EXTRA": "-DNMPC_PROF2 -DNMPC_EXPERIMENTS"},        # cycles by section of the hybrid kernel's loop (scripts/sections.py)
    "prof2e": {"EXTRA": "-DNMPC_PROF2=2 -DNMPC_EXPERIMENTS"},     # the same, by section of the evaluation
    "tl": {"EXTRA": "-DNMPC_TL -DNMPC_EXPERIMENTS"},              # timeline of a helped iteration (scripts/timeline.py)
}
ON_DEMAND = ("ws", "prof2", "prof2e", "tl")
VARIANTS = [n for n in LIBRARIES if n != PRODUCT and n not in ON_DEMAND]      # what build() builds besides the product
STRATEGIES = {n: v["SCHED"].split() for n, v in LIBRARIES.items() if "SCHED" in v}


def variant_path(name: str) -> str:
    return LIB_PATH if name == PRODUCT else os.path.join(_CSRC, "variants", f"libnmpc_{name}.so")


def _build(name: str, force: bool) -> dict:
    """Build LIBRARIES[name] (hipcc --offload-arch=gfx950: cross-compiles without a GPU) and run the code-generation check on the same make
    variables: ROCm 7.2 has produced silently wrong code for these kernels twice.  -> the verdict, written next to the library (the product's:
    build_info.json, which bench.py quotes).  Fresh = built from the same content of the sources, the Makefile and the entry: not rebuilt.
    A refused library is not put in place: the product keeps the one in place, described by build_info.json (the verdict goes to
    build_info.json.refused); a variant's path is left empty.  Several processes may call this at once: the build runs under a file lock into
    a temporary name and is renamed into place."""
    import fcntl
    import hashlib
    from . import codegen_check
    out, make_vars = variant_path(name), LIBRARIES[name]
    verdict = BUILD_INFO if name == PRODUCT else out[:-3] + ".json"
    h = hashlib.sha256(json.dumps(make_vars, sort_keys=True).encode())
    for src in _sources():
        with open(src, "rb") as fh:
            h.update(fh.read())
    key = h.hexdigest()[:16]

    def fresh():
        try:
            with open(verdict) as fh:
                info = json.load(fh)
        except (OSError, ValueError):
            return None
        ok = info.get("codegen_check", {}).get("ok")
        return info if not force and info.get("build_key") == key and (os.path.exists(out) or ok is False) else None

    info = fresh()
    if info is not None:
        return info
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(os.path.join(_CSRC, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            info = fresh()
            if info is not None:
                return info
            tmp = os.path.relpath(out, _CSRC) + f".tmp{os.getpid()}"
            r = subprocess.run(["make", "-C", _CSRC, "-B", tmp, f"OUT={tmp}"] + [f"{k}={v}" for k, v in make_vars.items()],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"building {out} failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
            res = codegen_check.verify(make_vars)
            info = {"source_hash": source_hash(), "flags": res.get("flags"), "codegen_check": {k: v for k, v in res.items() if k != "resources"},
                    "resources": res.get("resources", {}), "build_key": key}
            if res["ok"]:
                os.replace(os.path.join(_CSRC, tmp), out)
            else:
                os.remove(os.path.join(_CSRC, tmp))
                if name != PRODUCT and os.path.exists(out):
                    os.remove(out)
            with open(verdict + (".refused" if name == PRODUCT and not res["ok"] else ""), "w") as fh:      # (under the lock: library and
                json.dump(info, fh, indent=1)                                                               # verdict change together)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return info


def build_library(force: bool = False) -> str:
    """The product library, csrc/libnmpc_hip.so (_build); raises if the code-generation check refuses it."""
    info = _build(PRODUCT, force)
    if not info["codegen_check"]["ok"]:
        raise RuntimeError("libnmpc_hip.so REFUSED: the compiler generated wrong code for these flags (codegen_check): " +
                           json.dumps(info["codegen_check"])[:3000])
    return LIB_PATH


def build_variant(name: str, force: bool = False) -> dict:
    """csrc/variants/libnmpc_<name>.so, LIBRARIES[name] (_build); -> its code-generation check.  A variant the check refuses is not built:
    `ok` is False, and there is no library at variant_path(name)."""
    return _build(name, force)["codegen_check"]


def build_info() -> dict:
    """What the library in use was built with (flags, code-generation check, resources per kernel); {} for a library of unknown origin."""
    try:
        with open(BUILD_INFO) as fh:
            info = json.load(fh)
        return info if info.get("source_hash") == source_hash() else {"stale": True, **info}
    except OSError:
        return {}


_lib = None
_lib_experiments = None


def load_library(experiments: bool = False) -> C.CDLL:
    """Load (building if needed) the HIP library; raises if that is impossible.  experiments=True: the variant with the environment knobs
    (tests and scripts only; the product never asks for it)."""
    global _lib, _lib_experiments
    if experiments:
        if _lib_experiments is None:
            build_library()
            check = build_variant(EXPERIMENTS)
            if not check["ok"]:
                raise RuntimeError(f"{variant_path(EXPERIMENTS)} REFUSED by the code-generation check: " + json.dumps(check)[:2000])
            _lib_experiments = _bind(C.CDLL(variant_path(EXPERIMENTS)), variant_path(EXPERIMENTS))
            assert _lib_experiments.nmpc_experiments_build() == 1
            # the readers of the launch order: this variant's alone, declared nowhere in include/nmpc_solver.h
            u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
            _lib_experiments.nmpc_debug_launch_order.argtypes = [C.c_void_p, i32p, i32p, u8p, i32p]
            _lib_experiments.nmpc_debug_order_of.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), u8p, i32p]
        return _lib_experiments
    if _lib is not None:
        return _lib
    path = os.environ.get("NMPC_LIB_PATH") or build_library()      # (NMPC_LIB_PATH: instrumented builds, scripts/ only)
    _lib = _bind(C.CDLL(path), path)
    return _lib


def _bind(lib: C.CDLL, path: str) -> C.CDLL:
    lib.nmpc_abi_version.restype = C.c_int
    if lib.nmpc_abi_version() != EXPECTED_ABI:      # a stale / foreign .so would silently misread nmpc_opts
        raise RuntimeError(f"{path}: ABI version {lib.nmpc_abi_version()}, this package expects {EXPECTED_ABI} "
                           "(rebuild: make -C mpc_trajectory_generator_amd/csrc -B)")
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    lib.nmpc_default_opts.argtypes = [C.POINTER(NmpcOpts)]
    lib.nmpc_default_opts.restype = None
    for f in ("nmpc_n_u", "nmpc_n_p", "nmpc_n1", "nmpc_n2"):
        getattr(lib, f).argtypes = [C.POINTER(NmpcProblem)]
        getattr(lib, f).restype = C.c_int
    lib.nmpc_new.argtypes = [C.POINTER(NmpcProblem), C.POINTER(NmpcOpts), C.c_int, C.c_int, C.POINTER(vp)]
    lib.nmpc_free.argtypes = [vp]
    lib.nmpc_free.restype = None
    lib.nmpc_ping.argtypes = [vp]
    lib.nmpc_last_error.argtypes = [vp]
    lib.nmpc_last_error.restype = C.c_char_p
    lib.nmpc_kernel_name.argtypes = [vp]
    lib.nmpc_kernel_name.restype = C.c_char_p
    lib.nmpc_cull_radius.argtypes = [vp]
    lib.nmpc_cull_radius.restype = C.c_double
    lib.nmpc_launch_geometry.argtypes = [vp, C.c_int, C.POINTER(NmpcLaunchInfo)]
    lib.nmpc_launch_geometry.restype = C.c_int
    lib.nmpc_last_batch_ms.argtypes = [vp]
    lib.nmpc_last_batch_ms.restype = C.c_double
    lib.nmpc_solve_batch_device.argtypes = [vp, C.c_int] + [vp] * 7
    lib.nmpc_solve_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, vp]
    lib.nmpc_set_time_limits.argtypes = [vp, C.c_double, C.c_double]
    lib.nmpc_set_time_limits.restype = C.c_int
    lib.nmpc_eval_batch_device.argtypes = [vp, C.c_int] + [vp] * 9
    lib.nmpc_eval_batch_host.argtypes = [vp, C.c_int] + [dp] * 8
    lib.nmpc_test_sincos_host.argtypes = [vp, C.c_int, dp, dp, dp]
    lib.nmpc_test_divsqrt_host.argtypes = [vp, C.c_int, dp, dp, dp, dp]
    lib.nmpc_loop_new.argtypes = [vp, C.POINTER(NmpcRoute), C.c_int, dp, C.POINTER(C.c_int32), C.c_int, dp, C.c_int,
                                  C.POINTER(vp)]
    lib.nmpc_loop_new_routes.argtypes = [vp, C.POINTER(NmpcRoute), C.c_int, C.POINTER(C.c_int32), C.c_int, dp, C.POINTER(C.c_int32),
                                         C.c_int, dp, C.c_int, C.POINTER(vp)]
    lib.nmpc_loop_set_peers.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.c_double]
    lib.nmpc_loop_set_peers.restype = C.c_int
    lib.nmpc_loop_set_peers_grid.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.nmpc_loop_set_peers_grid.restype = C.c_int
    lib.nmpc_loop_peer_grid.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.nmpc_loop_peer_grid.restype = C.c_int
    lib.nmpc_loop_set_retire.argtypes = [vp, C.c_int]
    lib.nmpc_loop_set_retire.restype = C.c_int
    lib.nmpc_loop_active.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_active.restype = C.c_int
    lib.nmpc_loop_run.argtypes = [vp, C.c_int, vp]
    lib.nmpc_loop_run.restype = C.c_int
    lib.nmpc_loop_set_monitor.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.nmpc_loop_set_monitor.restype = C.c_int
    lib.nmpc_loop_clearance.argtypes = [vp, vp]
    lib.nmpc_loop_clearance.restype = C.c_int
    lib.nmpc_loop_set_map_monitor.argtypes = [vp, C.POINTER(NmpcScene)]
    lib.nmpc_loop_set_map_monitor.restype = C.c_int
    lib.nmpc_loop_map_clearance.argtypes = [vp, vp]
    lib.nmpc_loop_map_clearance.restype = C.c_int
    lib.nmpc_loop_set_track_monitor.argtypes = [vp, C.c_double]
    lib.nmpc_loop_set_track_monitor.restype = C.c_int
    lib.nmpc_loop_tracking.argtypes = [vp, vp]
    lib.nmpc_loop_tracking.restype = C.c_int
    lib.nmpc_loop_set_missions.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_set_missions.restype = C.c_int
    lib.nmpc_loop_legs.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_legs.restype = C.c_int
    lib.nmpc_loop_set_log.argtypes = [vp]
    lib.nmpc_loop_set_log.restype = C.c_int
    lib.nmpc_loop_log.argtypes = [vp, dp, vp, C.c_int]
    lib.nmpc_loop_log.restype = C.c_int
    lib.nmpc_loop_drive_summary.argtypes = [vp, vp]
    lib.nmpc_loop_drive_summary.restype = C.c_int
    lib.nmpc_loop_step_totals.argtypes = [vp, vp, C.c_int]
    lib.nmpc_loop_step_totals.restype = C.c_int
    lib.nmpc_loop_set_crowd.argtypes = [vp, C.c_int, dp, C.c_double, C.c_int, C.c_double]
    lib.nmpc_loop_set_crowd.restype = C.c_int
    lib.nmpc_loop_crowd.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    lib.nmpc_loop_crowd.restype = C.c_int
    lib.nmpc_loop_set_crowd_grid.argtypes = [vp, C.c_int, dp, C.c_double, C.c_int, C.c_double, C.c_double]
    lib.nmpc_loop_set_crowd_grid.restype = C.c_int
    lib.nmpc_loop_crowd_grid.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_crowd_grid.restype = C.c_int
    lib.nmpc_loop_set_crowd_monitor.argtypes = [vp]
    lib.nmpc_loop_set_crowd_monitor.restype = C.c_int
    lib.nmpc_loop_crowd_clearance.argtypes = [vp, vp]
    lib.nmpc_loop_crowd_clearance.restype = C.c_int
    lib.nmpc_loop_set_plant.argtypes = [vp, C.POINTER(NmpcPlant), C.POINTER(C.c_uint32)]
    lib.nmpc_loop_set_plant.restype = C.c_int
    lib.nmpc_loop_plant_applied.argtypes = [vp, dp, C.c_int]
    lib.nmpc_loop_plant_applied.restype = C.c_int
    lib.nmpc_loop_plant_measured.argtypes = [vp, dp]
    lib.nmpc_loop_plant_measured.restype = C.c_int
    lib.nmpc_loop_set_ensemble.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
    lib.nmpc_loop_set_ensemble.restype = C.c_int
    lib.nmpc_loop_ensemble.argtypes = [vp, vp, C.c_int]
    lib.nmpc_loop_ensemble.restype = C.c_int
    lib.nmpc_loop_ensemble_groups.argtypes = [vp]
    lib.nmpc_loop_ensemble_groups.restype = C.c_int
    lib.nmpc_loop_set_walls.argtypes = [vp, C.c_int, dp, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.nmpc_loop_set_walls.restype = C.c_int
    lib.nmpc_loop_walls.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_walls.restype = C.c_int
    lib.nmpc_loop_set_walls_grid.argtypes = [vp, C.c_int, dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.nmpc_loop_set_walls_grid.restype = C.c_int
    lib.nmpc_loop_wall_grid.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_wall_grid.restype = C.c_int
    lib.nmpc_loop_set_map_monitor_grid.argtypes = [vp, C.POINTER(NmpcScene), C.c_double, C.c_double]
    lib.nmpc_loop_set_map_monitor_grid.restype = C.c_int
    lib.nmpc_loop_map_grid.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.nmpc_loop_map_grid.restype = C.c_int
    lib.nmpc_loop_free.argtypes = [vp]
    lib.nmpc_loop_free.restype = None
    lib.nmpc_planner_new.argtypes = [C.POINTER(NmpcScene), C.c_int, C.c_int, C.POINTER(vp)]
    lib.nmpc_planner_free.argtypes = [vp]
    lib.nmpc_planner_free.restype = None
    lib.nmpc_planner_visibility.argtypes = [vp, C.POINTER(C.c_uint8)]
    lib.nmpc_plan_batch_device.argtypes = [vp, C.c_int] + [vp] * 7
    lib.nmpc_plan_batch_host.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, C.POINTER(C.c_uint8)]
    lib.nmpc_planner_last_ms.argtypes = [vp]
    lib.nmpc_planner_last_ms.restype = C.c_double
    lib.nmpc_loop_step.argtypes = [vp, vp]
    lib.nmpc_loop_read.argtypes = [vp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), vp]
    lib.nmpc_loop_params.argtypes = [vp, dp, dp, dp]
    lib.nmpc_loop_trajectory.argtypes = [vp, dp, C.c_int]
    lib.nmpc_experiments_build.restype = C.c_int
    return lib


def as_dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def as_i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
