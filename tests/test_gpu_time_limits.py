"""GPU: the wall-clock limits (nmpc_set_time_limits, BatchSolver.set_time_limits, OptimizerTcpManager(max_duration_micros=...)).

Timed solves are nondeterministic, but each instance can still be checked bit for bit.  The clock is tested exactly where
opts.max_total_inner is tested, at the end of a PANOC iteration, and a stop takes the budget's exit path.  So an instance stopped
by the clock after T PANOC iterations in total ran the same operations as the deterministic solve with max_total_inner = T; it
reports T as num_inner_iterations.  The rule: every instance's (u, y, status) equals one of two solves on every field of
STATUS_FIELDS (solve_time_ms aside):
  (U) the untimed solve with the handle's options -- the untimed run of the same kernel on the same inputs, which the rest of the
      suite holds to the oracle's bits (and a sample here does too);
  (B) the oracle's solve with max_total_inner = T_i, T_i = the instance's num_inner_iterations.
The oracle solves the (B) candidates one batch per distinct T_i."""
import math

import numpy as np
import pytest

from conftest import STATUS_FIELDS, oracle_for
from mpc_trajectory_generator_amd import harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.workloads import baseline_batch, differing, route_fleet

pytestmark = pytest.mark.gpu
OUT_OF_TIME = 2
THREADS = 16


def _same(u, y, st, u2, y2, st2):
    """per instance: every output and every status field (solve_time_ms aside) bit for bit"""
    eq = np.all(u == u2, axis=1) & np.all(y == y2, axis=1)
    for f in STATUS_FIELDS:
        eq &= st[f] == st2[f]
    return eq


def _check_rule(cfg, P, u0, y0, timed, untimed):
    """-> (in U, in B only) per instance; asserts that every instance is in one of them"""
    u, y, st = timed
    is_u = _same(u, y, st, *untimed)
    is_b = np.zeros(len(P), dtype=bool)
    rest = np.nonzero(~is_u)[0]
    T = st["num_inner_iterations"]
    for t in np.unique(T[rest]):
        idx = rest[T[rest] == t]
        ub, yb, sb = oracle_for(cfg, max_total_inner=int(t)).solve_batch(P[idx], u0=None if u0 is None else u0[idx],
                                                                          y0=None if y0 is None else y0[idx], threads=THREADS)
        is_b[idx] = _same(u[idx], y[idx], st[idx], ub, yb, sb)
    bad = np.nonzero(~(is_u | is_b))[0]
    assert bad.size == 0, (f"{bad.size} instances match neither the untimed solve nor the solve with max_total_inner = their count: "
                           f"{bad[:8]}, exit {st['exit_status'][bad[:8]]}, T {T[bad[:8]]}")
    return is_u, is_b & ~is_u


def _untimed_matches_oracle(cfg, P, untimed, n, u0=None, y0=None):
    idx = np.random.default_rng(3).choice(len(P), min(n, len(P)), replace=False)
    uo, yo, so = oracle_for(cfg).solve_batch(P[idx], u0=None if u0 is None else u0[idx], y0=None if y0 is None else y0[idx],
                                             threads=THREADS)
    assert not differing(untimed, (uo, yo, so), idx)


def _hip():
    """the HIP runtime the solver library itself runs on (the one already mapped into this process), through ctypes"""
    import ctypes as C
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _solve_device(s, P):
    """the device entry point (nmpc_solve_batch_device) on operands in device memory, on the default stream"""
    import ctypes as C
    from mpc_trajectory_generator_amd import _lib
    hip = _hip()
    B = len(P)
    u, y, st = np.zeros((B, s.n_u)), np.zeros((B, s.n1)), np.zeros(B, dtype=_lib.STATUS_DTYPE)
    sizes = (P.nbytes, u.nbytes, y.nbytes, st.nbytes)
    d = [C.c_void_p() for _ in sizes]
    try:
        for ptr, n in zip(d, sizes):
            assert hip.hipMalloc(C.byref(ptr), n) == 0
        assert hip.hipMemcpy(d[0], P.ctypes.data, sizes[0], 1) == 0          # hipMemcpyHostToDevice
        assert hip.hipMemset(d[1], 0, sizes[1]) == 0
        s._check(s.lib.nmpc_solve_batch_device(s._h, B, d[0], d[1], None, None, d[2], d[3], None))
        assert hip.hipDeviceSynchronize() == 0
        for host, ptr, n in zip((u, y, st), d[1:], sizes[1:]):
            assert hip.hipMemcpy(host.ctypes.data, ptr, n, 2) == 0            # hipMemcpyDeviceToHost
    finally:
        for ptr in d:
            if ptr.value:
                hip.hipFree(ptr)
    return u, y, st


# ---------------------------------------------------------------------------------------------- 1. unreachable limits change nothing
@pytest.mark.parametrize("name,B,kernel", [("cfg1", 2500, "nmpc_solve_hyb_kernel<ShapeDefault>"),
                                           ("cfg2", 1500, "nmpc_solve_hyb2_kernel<ShapeN40>"),
                                           ("cfg3", 2500, "nmpc_solve_hyb_kernel<ShapeNobs50>"),
                                           ("n17", 600, "nmpc_solve_hyb_kernel<ShapeAny>"),
                                           ("n33", 600, "nmpc_solve_hyb2_kernel<ShapeAny>")])
def test_unreachable_limits_change_nothing(name, B, kernel):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg = {"n17": lambda: load_config(N_hor=17), "n33": lambda: load_config(N_hor=33)}.get(name, lambda: named_config(name))()
    P = harness.synthetic_batch(cfg, 11, B, seed=5, synthetic_circles=(name == "cfg3"))
    s = BatchSolver(cfg, max_batch=B)
    try:
        assert s.kernel_name == kernel
        ref = s.solve(P)
        s.set_time_limits(1e6, 1e6)
        timed_kernel = kernel.replace("<", "<Timed<", 1) + ">"
        assert s.kernel_name == timed_kernel
        u, y, st = s.solve(P)
        assert not differing((u, y, st), ref)
        assert not np.any(st["exit_status"] == OUT_OF_TIME)
        s.set_time_limits(0, 0)
        assert s.kernel_name == kernel
        assert not differing(s.solve(P), ref)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. per-instance limit (max_duration)
@pytest.mark.parametrize("name,B,path", [("cfg1", 4096, "host"), ("cfg2", 4096, "device"), ("cfg1", 4, "device"), ("cfg2", 4, "host")])
def test_per_instance_limit_replays(name, B, path):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg, P = baseline_batch(name, max(B, 64))
    s = BatchSolver(cfg, max_batch=max(B, 64))
    try:
        if B < 64:
            # latency mode (one instance per team, helpers from the first iteration on): four instances of spread-out solve times
            _, _, st64 = s.solve(P)
            order = np.argsort(st64["solve_time_ms"])
            P = P[order[[0, 21, 42, 63]]]
        solve = s.solve if path == "host" else (lambda P_: _solve_device(s, P_))
        untimed = solve(P)
        limit = float(np.median(untimed[2]["solve_time_ms"]))
        s.set_time_limits(max_duration_ms=limit)
        timed = solve(P)
        s.set_time_limits(0, 0)
        _untimed_matches_oracle(cfg, P, untimed, 16)
        is_u, only_b = _check_rule(cfg, P, None, None, timed, untimed)
        st = timed[2]
        assert np.all(st["solve_time_ms"][only_b] >= limit), "an instance stopped by the clock before its limit"
        assert is_u.any() and only_b.any(), (is_u.sum(), only_b.sum())
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. batch budget
def test_batch_budget_replays_and_ends_the_batch_early():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    B = 8192
    cfg, P = baseline_batch("cfg1", B)
    s = BatchSolver(cfg, max_batch=B)
    try:
        untimed = s.solve(P)
        ms_untimed = s.last_batch_ms
        s.set_time_limits(batch_budget_ms=ms_untimed / 4)
        assert s.kernel_name == "nmpc_solve_hyb_kernel<Timed<ShapeDefault>>"
        timed = s.solve(P)
        ms_timed = s.last_batch_ms
    finally:
        s.close()
    _untimed_matches_oracle(cfg, P, untimed, 32)
    is_u, only_b = _check_rule(cfg, P, None, None, timed, untimed)
    assert is_u.any() and only_b.any(), (is_u.sum(), only_b.sum())
    # a quarter of the budget: about 9 against 36 ms; the bound leaves room for the last iterations and the launch
    assert ms_timed < 0.75 * ms_untimed, (ms_timed, ms_untimed)


# ---------------------------------------------------------------------------------------------- 4. closed loop on a budget
def test_device_loop_under_a_batch_budget_replays_every_step():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    cfg = named_config("cfg1")
    route = harness.scene_route(cfg, 11)
    B = 1000
    i0, starts, _ = route_fleet(route, B, 17)
    s = BatchSolver(cfg, max_batch=B, batch_budget_ms=2.0)
    stopped = 0
    try:
        dev = DeviceRecedingHorizon(s, route, starts, None, idx0=i0)
        for k in range(4):
            _, U0, Y0 = dev.params()            # the warm start of this step (nmpc_loop_step: previous u and y, initial penalty)
            dev.step()
            Pk, Uk, Yk = dev.params()
            st = dev.read()[4]
            # (U): the untimed oracle solve from the same warm start; (B): the same with max_total_inner = T_i
            uU, yU, sU = oracle_for(cfg).solve_batch(Pk, u0=U0, y0=Y0, threads=THREADS)
            _check_rule(cfg, Pk, U0, Y0, (Uk, Yk, st), (uU, yU, sU))
            stopped += int(np.sum(st["exit_status"] == OUT_OF_TIME))
        dev.close()
    finally:
        s.close()
    assert stopped > 0, "a 2 ms budget stopped no instance of a cold-started fleet of 1000"


# ---------------------------------------------------------------------------------------------- 5. arguments and the shim
def test_bad_limits_are_refused_and_keep_the_limits_in_force():
    from mpc_trajectory_generator_amd.solver import BatchSolver, SolverError
    cfg = named_config("cfg1")
    s = BatchSolver(cfg, max_batch=8, max_duration_ms=5.0)
    try:
        timed = "nmpc_solve_hyb_kernel<Timed<ShapeDefault>>"
        assert s.kernel_name == timed
        for bad in ((-1.0, 0.0), (0.0, -1e-9), (math.nan, 0.0), (0.0, math.nan), (math.inf, 0.0), (0.0, -math.inf)):
            assert s.lib.nmpc_set_time_limits(s._h, *bad) == -2, bad
            with pytest.raises(SolverError):
                s.set_time_limits(*bad)
            assert s.kernel_name == timed and (s.max_duration_ms, s.batch_budget_ms) == (5.0, 0.0)
        # the limits in force still act: a limit far below one solve stops every instance of a cold batch
        P = baseline_batch("cfg1", 8)[1]
        s.set_time_limits(0, 0)
        s.set_time_limits(0.001, 0)
        assert s.lib.nmpc_set_time_limits(s._h, -5.0, 0.0) == -2
        _, _, st = s.solve(P)
        assert np.all(st["exit_status"] == OUT_OF_TIME)
    finally:
        s.close()
    with pytest.raises(SolverError):
        BatchSolver(cfg, max_batch=8, batch_budget_ms=-1.0)


def test_shim_max_duration():
    from mpc_trajectory_generator_amd.tcp_shim import OptimizerTcpManager
    cfg, P = baseline_batch("cfg1", 3, seed=2)
    plain, ref_time, tiny = (OptimizerTcpManager(config=cfg, max_batch=4), OptimizerTcpManager(config=cfg, max_batch=4, max_duration_micros=500_000),
                             OptimizerTcpManager(config=cfg, max_batch=4, max_duration_micros=1))
    for m in (plain, ref_time, tiny):
        m.start()
    try:
        assert ref_time._solver.kernel_name == "nmpc_solve_hyb_kernel<Timed<ShapeDefault>>"
        for p in P:      # consecutive calls: both managers warm-start from their own previous solution
            a, b = plain.call(p), ref_time.call(p)
            assert a.is_ok() and b.is_ok()
            ra, rb = a.get(), b.get()
            assert ra.solution == rb.solution and ra.lagrange_multipliers == rb.lagrange_multipliers
            for f in ("exit_status", "num_outer_iterations", "num_inner_iterations", "last_problem_norm_fpr", "f2_norm", "penalty", "cost"):
                assert getattr(ra, f) == getattr(rb, f), f
        r = tiny.call(P[0])
        assert r.is_ok(), "non-convergence is not an error"
        assert r.get().exit_status == "NotConvergedOutOfTime"
        assert r.get().solve_time_ms >= 0.001
    finally:
        for m in (plain, ref_time, tiny):
            m.kill()
