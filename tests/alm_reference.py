"""A plain reference for the ALM outer loop (a helper module of the tests, not a conftest).

Two parts, both written from the math and nothing else:

* ``plain_f`` / ``plain_f1_f2``: the cost f and the constraint maps F1, F2 of SURVEY.md App. A/B, vectorised over a
  batch, in ``np.longdouble`` (sin and cos included) and rounded to f64 at the end.  No prefix-sum order, no tree sums,
  no canonical sin/cos: none of the arithmetic the kernels and the oracle share.
* ``outer_step`` / ``reconstruct``: the literal ALM outer step of SURVEY.md App. C.3 with the choices of DESIGN.md
  section 9 (y / max(c, 1) shift, no penalty growth at nu = 0, the absolute DBL_EPSILON the exit and stall
  comparisons carry).  ``max_outer`` only enters the loop's end test, so a solve capped at m performs exactly the
  first m outer iterations of one with a higher cap: the runs capped at m - 1 and m give the state entering outer
  iteration m and what it produced, and that step is recomputed here from F1(u), F2(u) and compared.  PANOC is not
  reimplemented: the inner solution u is taken from the solver under test.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS_M = float(np.finfo(np.float64).eps)      # DBL_EPSILON: the absolute term of the exit and stall comparisons
Y_BOUND = 1e12                               # Y = [-1e12, 1e12]^n1
AMBIGUOUS_RTOL = 1e-9
Y_RTOL = 1e-12                               # y+ to 1e-12 * (|y| + c * max(|F1|, 1)), elementwise
Y_ROUND = 16 * EPS_M                         # ... and what the solver's rounding moves it by, for the branch decisions
F2_RTOL = 1e-12                              # f2_norm to 1e-12 relative, plus the rounding of the cancelling h terms:
F2_ABS = 64 * EPS_M                          # 64 DBL_EPSILON * sum_t (r^2 + dx^2 + dy^2) over the (nearly) active stages


# ------------------------------------------------------------------------------------------------ the cost layer
def _unpack(cfg, P):
    """P [B, n_p] -> the pieces of the parameter vector, as long doubles."""
    N, nobs, ndyn = cfg.N_hor, cfg.Nobs, cfg.Ndynobs
    P = np.asarray(P, dtype=np.float64).astype(LD)
    B = P.shape[0]
    c0 = 20 + N
    d0 = c0 + 3 * nobs
    r0 = d0 + 5 * ndyn * N
    assert P.shape[1] == r0 + 3 * N == cfg.n_p
    return dict(
        state=P[:, 0:3], last_u=P[:, 3:5], target=P[:, 5:8], w=P[:, 10:20], vref=P[:, 20:20 + N],
        circles=P[:, c0:d0].reshape(B, nobs, 3),
        ellipses=P[:, d0:r0].reshape(B, ndyn, N, 5),           # obstacle-major, stage-minor: (x, y, rx, ry, angle)
        ref=P[:, r0:].reshape(B, N, 3))


def _rollout(cfg, st, U):
    """Euler rollout: states x_0 .. x_N, each [B, N + 1]."""
    ts = LD(cfg.ts)
    v, w = U[:, 0::2], U[:, 1::2]
    B, N = v.shape
    th = np.empty((B, N + 1), dtype=LD)
    x = np.empty_like(th)
    y = np.empty_like(th)
    th[:, 0], x[:, 0], y[:, 0] = st["state"][:, 2], st["state"][:, 0], st["state"][:, 1]
    for t in range(N):
        x[:, t + 1] = x[:, t] + ts * v[:, t] * np.cos(th[:, t])
        y[:, t + 1] = y[:, t] + ts * v[:, t] * np.sin(th[:, t])
        th[:, t + 1] = th[:, t] + ts * w[:, t]
    return x, y, th


def _accelerations(cfg, st, U):
    """(v_t - v_{t-1}) / ts and (w_t - w_{t-1}) / ts, with (v_{-1}, w_{-1}) the last applied controls p[3:5]."""
    ts = LD(cfg.ts)
    v, w = U[:, 0::2], U[:, 1::2]
    av = np.diff(np.concatenate([st["last_u"][:, 0:1], v], axis=1), axis=1) / ts
    aw = np.diff(np.concatenate([st["last_u"][:, 1:2], w], axis=1), axis=1) / ts
    return av, aw


def _f1_f2(cfg, st, U):
    x, y, _ = _rollout(cfg, st, U)
    av, aw = _accelerations(cfg, st, U)
    F1 = np.concatenate([av, aw], axis=1)                                   # [v..., w...] like F1
    xn, yn = x[:, 1:], y[:, 1:]                                             # post-update positions, stage t -> x_{t+1}
    circ = st["circles"]                                                    # [B, nobs, 3]
    h = circ[:, :, 2:3] ** 2 - (xn[:, None, :] - circ[:, :, 0:1]) ** 2 - (yn[:, None, :] - circ[:, :, 1:2]) ** 2
    F2c = np.maximum(h, LD(0)).sum(axis=2)
    mag = LD(2) * circ[:, :, 2:3] ** 2 - h                                  # r^2 + dx^2 + dy^2
    S2c = np.where(h > -AMBIGUOUS_RTOL * mag, mag, LD(0)).sum(axis=2)
    e = st["ellipses"]                                                      # [B, ndyn, N, 5]
    dx, dy = xn[:, None, :] - e[..., 0], yn[:, None, :] - e[..., 1]
    ca, sa = np.cos(e[..., 4]), np.sin(e[..., 4])
    a = dx * ca + dy * sa
    b = dx * sa - dy * ca
    h = LD(1) - a * a / (e[..., 2] ** 2) - b * b / (e[..., 3] ** 2)
    F2e = np.maximum(h, LD(0)).sum(axis=2)
    mag = LD(2) - h                                                         # 1 + a^2/rx^2 + b^2/ry^2
    S2e = np.where(h > -AMBIGUOUS_RTOL * mag, mag, LD(0)).sum(axis=2)
    return F1, np.concatenate([F2c, F2e], axis=1), np.concatenate([S2c, S2e], axis=1)


def plain_f1_f2(cfg, P, U, scale=False):
    """F1 [B, n1] and F2 [B, n2] of a batch, computed in long double, rounded to f64.  scale=True adds S2 [B, n2]: per
    obstacle, the magnitude of the terms whose sum F2 is, over the stages where they (nearly) count -- what a rounding
    error in the solver's F2 is proportional to."""
    st = _unpack(cfg, P)
    F1, F2, S2 = _f1_f2(cfg, st, np.asarray(U, dtype=np.float64).astype(LD))
    out = F1.astype(np.float64), F2.astype(np.float64)
    return out + (S2.astype(np.float64),) if scale else out


def plain_f(cfg, P, U):
    """The cost f(u; p) [B], in long double, rounded to f64."""
    st = _unpack(cfg, P)
    U = np.asarray(U, dtype=np.float64).astype(LD)
    q, qv, qth, rv, rw, qN, qthN, qcte, pa, pw = (st["w"][:, k:k + 1] for k in range(10))
    v, w = U[:, 0::2], U[:, 1::2]
    x, y, th = _rollout(cfg, st, U)
    xf, yf, thf = (st["target"][:, k:k + 1] for k in range(3))
    f = (rv * v * v + rw * w * w + qv * (v - st["vref"]) ** 2).sum(axis=1)
    f += (q * ((x[:, :-1] - xf) ** 2 + (y[:, :-1] - yf) ** 2) + qth * (th[:, :-1] - thf) ** 2).sum(axis=1)
    # cross-track error of the post-update position: squared distance to the nearest of the N - 1 reference segments
    ref = st["ref"]
    A, D = ref[:, :-1, :2], ref[:, 1:, :2] - ref[:, :-1, :2]                  # segment i joins samples i and i + 1
    Pn = np.stack([x[:, 1:], y[:, 1:]], axis=2)                              # [B, N, 2]
    rel = Pn[:, :, None, :] - A[:, None, :, :]                               # [B, N, N - 1, 2]
    that = (rel * D[:, None]).sum(axis=3) / ((D * D).sum(axis=2)[:, None, :] + LD(1e-16))
    that = np.clip(that, LD(0), LD(1))
    err = rel - that[..., None] * D[:, None]
    f += (qcte * (err ** 2).sum(axis=3).min(axis=2)).sum(axis=1)
    f += (qN * ((x[:, -1:] - xf) ** 2 + (y[:, -1:] - yf) ** 2) + qthN * (th[:, -1:] - thf) ** 2)[:, 0]
    av, aw = _accelerations(cfg, st, U)
    f += (pa * av * av + pw * aw * aw).sum(axis=1)
    return f.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the outer loop
DEFAULT_OPTS = dict(tolerance=1e-4, initial_tolerance=1e-4, delta_tolerance=1e-4, initial_penalty=1.0, penalty_update=5.0,
                    tolerance_update=0.1, sufficient_decrease=0.1, max_inner=500, max_outer=10, max_total_inner=0,
                    inner_status=0)


def eps_schedule(opts, nu):
    """epsilon_nu: epsilon_0 = initial_tolerance, epsilon_{nu+1} = max(beta * epsilon_nu, epsilon)."""
    e = float(opts["initial_tolerance"])
    for _ in range(nu):
        e = max(float(opts["tolerance_update"]) * e, float(opts["tolerance"]))
    return e


def _le(lhs, rhs, err):
    """lhs <= rhs in three values: True / False, or None when the sides are within 1e-9 relative of each other or
    within ``err``, what rounding in the solver can move them by."""
    if abs(lhs - rhs) <= AMBIGUOUS_RTOL * max(abs(lhs), abs(rhs)) + err:
        return None
    return lhs <= rhs


def _and(*xs):
    if any(x is False for x in xs):
        return False
    return None if any(x is None for x in xs) else True


def outer_step(cfg, opts, nu, y, c, F1, F2, S2, dy_prev, f2_prev, dy_prev_err, f2_prev_err):
    """One literal outer step of one instance.  y: the multipliers entering the step (before Pi_Y), c the penalty in
    force, F1 / F2 at the inner solution (S2: F2's rounding scale, plain_f1_f2), (dy_prev, f2_prev) the previous step's Delta and phi2 (ignored at nu = 0).
    -> dict with y+, Delta, phi2, their rounding scales, and the branch decisions (True / False / None = ambiguous)."""
    N = cfg.N_hor
    lo = np.r_[np.full(N, cfg.lin_acc_min), np.full(N, -cfg.ang_acc_max)].astype(LD)
    hi = np.r_[np.full(N, cfg.lin_acc_max), np.full(N, cfg.ang_acc_max)].astype(LD)
    yc = np.clip(np.asarray(y, dtype=np.float64), -Y_BOUND, Y_BOUND)       # y <- Pi_Y(y)
    yl, F1l, cl = yc.astype(LD), np.asarray(F1, dtype=np.float64).astype(LD), LD(c)
    yplus = yl + cl * (F1l - np.clip(F1l + yl / max(cl, LD(1)), lo, hi))
    dy = float(np.sqrt(((yplus - yl) ** 2).sum()))
    f2 = float(np.sqrt((np.asarray(F2, dtype=np.float64).astype(LD) ** 2).sum()))
    scale = np.abs(yc) + c * np.maximum(np.abs(F1), 1.0)
    y_tol = Y_RTOL * scale
    # what rounding can move Delta by: a few ulps of |y| + c |F1| per component, nothing on a component with y = 0 whose
    # F1 lies inside C by more than its own rounding (y+ - y = c * (F1 - F1) = 0 exactly, in any arithmetic)
    inside = (yc == 0.0) & (F1l > lo + y_tol) & (F1l < hi - y_tol)
    dy_err = float(np.sqrt((np.where(inside, 0.0, Y_ROUND * scale) ** 2).sum()))
    f2_err = F2_RTOL * f2 + F2_ABS * float(np.sqrt((np.asarray(S2, dtype=np.float64) ** 2).sum()))
    delta, theta, rho = float(opts["delta_tolerance"]), float(opts["sufficient_decrease"]), float(opts["penalty_update"])
    eps_nu = eps_schedule(opts, nu)
    n2 = len(F2)
    crit1 = False if nu == 0 else _le(dy, c * delta + EPS_M, dy_err)
    crit2 = True if n2 == 0 else _le(f2, delta + EPS_M, f2_err)
    crit3 = eps_nu <= float(opts["tolerance"]) + EPS_M                     # exact: the schedule is recomputed as the solver does
    converged = _and(crit1, crit2, crit3)
    if nu == 0:
        stall = True
    else:
        stall = _and(_le(dy, theta * dy_prev + EPS_M, dy_err + theta * dy_prev_err),
                     _le(f2, theta * f2_prev + EPS_M, f2_err + theta * f2_prev_err))
    return dict(nu=nu, y_in=yc, c=c, yplus=yplus.astype(np.float64), y_tol=y_tol, dy=dy, dy_err=dy_err, f2=f2, f2_err=f2_err,
                eps_nu=eps_nu, crit1=crit1, crit2=crit2, crit3=crit3, converged=converged, stall=stall,
                c_next=c if stall else (c * rho if stall is False else None), clamped=bool(np.any(np.abs(y) > Y_BOUND)))


STATUS_COPY = ("exit_status", "num_outer_iterations", "num_inner_iterations", "num_cost_evals", "num_grad_evals",
               "last_problem_norm_fpr", "delta_y_norm_over_c", "f2_norm", "penalty", "cost")


def _same_bits(a, b, i, j):
    (u, y, st), (u2, y2, st2) = a, b
    return (np.array_equal(u[i], u2[j]) and np.array_equal(y[i], y2[j]) and
            all(np.array_equal(st[f][i], st2[f][j]) for f in STATUS_COPY))


def reconstruct(make_solve, cfg, P, u0=None, y0=None, c0=None, opts=None):
    """Run a solver with max_outer = 1 .. opts["max_outer"] and recompute every outer step with ``outer_step``.

    make_solve(opts) -> solve(P, u0, y0, c0) -> (u, y, status): e.g. an oracle's ``solve_batch`` or a ``BatchSolver``'s
    ``solve`` built with those options.  ``opts`` are the non-default options (the rest is DEFAULT_OPTS).
    -> (records, runs): one record per instance per outer step, and the solver outputs per cap.  Each record carries
    the literal step, what the solver reported, and the list of problems found (empty = the step obeys the rules)."""
    full = dict(DEFAULT_OPTS, **(opts or {}))
    B = len(P)
    n1 = cfg.n1
    y_start = np.zeros((B, n1)) if y0 is None else np.asarray(y0, dtype=np.float64)
    c_start = np.full(B, float(full["initial_penalty"])) if c0 is None else np.asarray(c0, dtype=np.float64)
    c_start = np.where(c_start > 0.0, c_start, float(full["initial_penalty"]))
    budget = int(full["max_total_inner"])
    runs = {}
    for m in range(1, int(full["max_outer"]) + 1):
        runs[m] = make_solve(dict(opts or {}, max_outer=m))(P, u0, y0, c0)
    records = []
    for b in range(B):
        y_in, c_in, inner_before = y_start[b], float(c_start[b]), 0
        dy_prev = f2_prev = dy_prev_err = f2_prev_err = 0.0
        for m in range(1, int(full["max_outer"]) + 1):
            nu = m - 1
            u, y, st = runs[m]
            F1, F2, S2 = plain_f1_f2(cfg, P[b:b + 1], u[b:b + 1], scale=True)
            step = outer_step(cfg, full, nu, y_in, c_in, F1[0], F2[0], S2[0], dy_prev, f2_prev, dy_prev_err, f2_prev_err)
            s = st[b]
            it = int(s["num_inner_iterations"]) - inner_before
            if budget > 0 and it >= budget - inner_before:
                inner = 2
            else:
                inner = 0 if it < int(full["max_inner"]) else 1
            rep_dy = float(s["delta_y_norm_over_c"]) * float(s["penalty"])
            problems = []
            if int(s["num_outer_iterations"]) != m:
                problems.append(f"num_outer_iterations {s['num_outer_iterations']} != {m}")
            if not np.all(np.abs(y[b] - step["yplus"]) <= step["y_tol"]):
                problems.append(f"y+ off by {np.max(np.abs(y[b] - step['yplus']) / step['y_tol']):.3g} tolerances")
            if abs(float(s["f2_norm"]) - step["f2"]) > step["f2_err"]:
                problems.append(f"f2_norm {s['f2_norm']!r} != |F2(u)| {step['f2']!r}")
            if abs(rep_dy - step["dy"]) > step["dy_err"] + 1e-12 * step["dy"]:
                problems.append(f"Delta {rep_dy!r} != {step['dy']!r}")
            ends = None                      # how the solve ends after this step, if it does: "converged" / "budget"
            if step["converged"] is not None:
                if step["converged"]:
                    want = 0 if int(full["inner_status"]) == 1 else inner
                    if int(s["exit_status"]) != want:
                        problems.append(f"converged: exit_status {s['exit_status']} != {want}")
                    if float(s["penalty"]) != c_in:
                        problems.append("converged: the penalty changed")
                    ends = "converged"
                elif int(s["exit_status"]) != 1:
                    problems.append(f"not converged at the cap: exit_status {s['exit_status']} != 1")
            if step["converged"] is False and step["stall"] is not None and float(s["penalty"]) != step["c_next"]:
                problems.append(f"penalty {s['penalty']!r} != {step['c_next']!r} (stall {step['stall']})")
            if step["converged"] is False and inner == 2:
                ends = "budget"
            records.append(dict(step, b=b, m=m, inner=inner, exit_status=int(s["exit_status"]),
                                penalty=float(s["penalty"]), ends=ends, problems=problems))
            if ends is None and step["converged"] is None:
                ends = "converged" if int(s["exit_status"]) != 1 else None        # ambiguous: follow the solver
            if ends is not None:
                # the solve is over: under every higher cap the same bits (a budget end: exit 2 instead of 1)
                for m2 in range(m + 1, int(full["max_outer"]) + 1):
                    u2, y2, st2 = runs[m2]
                    if ends == "converged" and not _same_bits(runs[m], runs[m2], b, b):
                        problems.append(f"converged at {m}, other bits under cap {m2}")
                    if ends == "budget":
                        if int(st2["exit_status"][b]) != 2 or int(st2["num_outer_iterations"][b]) != m:
                            problems.append(f"budget spent at {m}: cap {m2} gives exit {st2['exit_status'][b]} "
                                            f"after {st2['num_outer_iterations'][b]}")
                        elif not (np.array_equal(u2[b], u[b]) and np.array_equal(y2[b], y[b])):
                            problems.append(f"budget spent at {m}: other bits under cap {m2}")
                break
            y_in, c_in, inner_before = y[b], float(s["penalty"]), int(s["num_inner_iterations"])
            dy_prev, f2_prev, dy_prev_err, f2_prev_err = step["dy"], step["f2"], step["dy_err"], step["f2_err"]
    return records, runs


# ------------------------------------------------------------------------------------------------ the option sets
# Each changes only the named fields of nmpc_opts; everything else stays at its default.
SCHEDULE = dict(initial_tolerance=1e-2, tolerance_update=0.5)
OPTION_SETS = {
    "schedule": SCHEDULE,                                             # the epsilon_nu ladder: 1e-2, 5e-3, ... 1e-4 at nu = 7
    "ladder": dict(penalty_update=2.0, sufficient_decrease=0.5),      # + per-instance c0 < 1 and huge y0 (set_inputs)
    "loose": dict(delta_tolerance=1e-2),
    "tight": dict(tolerance=1e-6, delta_tolerance=1e-6, max_outer=12),
    "start": dict(initial_penalty=0.1, penalty_update=10.0, sufficient_decrease=0.01),
    "budget": dict(SCHEDULE, inner_status=1, max_total_inner=600),
}
FIRST_NU_CRIT3 = {"schedule": 7, "budget": 7}                         # the first nu at which epsilon_nu <= epsilon


def set_inputs(name, B, n1, seed):
    """-> (y0, c0) of an option set: None, None except for "ladder" (c0 in {0.25, 0.5, 1, 40}, y0 ~ N(0, 3) with
    entries of +-1e13 in every third instance, beyond Y)."""
    if name != "ladder":
        return None, None
    rng = np.random.default_rng(seed)
    c0 = np.resize([0.25, 0.5, 1.0, 40.0], B)
    y0 = rng.normal(0.0, 3.0, (B, n1))
    for b in range(0, B, 3):
        k = rng.choice(n1, 2, replace=False)
        y0[b, k] = rng.choice([-1e13, 1e13], 2)
    return y0, c0


def summary(records):
    """What a set of records exercised, and what it could not decide."""
    decisions = [r["converged"] for r in records] + [r["stall"] for r in records if r["nu"] > 0 and r["converged"] is False]
    return dict(
        steps=len(records), decisions=len(decisions), ambiguous=sum(d is None for d in decisions),
        problems=[(r["b"], r["m"], p) for r in records for p in r["problems"]],
        growth=sum(r["nu"] >= 1 and r["converged"] is False and r["stall"] is False for r in records),
        stall=sum(r["nu"] >= 1 and r["converged"] is False and r["stall"] is True for r in records),
        converged_nu=sorted({r["nu"] for r in records if r["ends"] == "converged"}),
        budget=sum(r["ends"] == "budget" for r in records),
        clamped=sum(r["clamped"] for r in records),
        small_c_with_y=sum(r["c"] < 1.0 and bool(np.any(r["y_in"] != 0.0)) for r in records))
