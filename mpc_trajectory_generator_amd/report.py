"""Run-time report of a trajectory run: counterpart of the reference's ``runtime_analysis`` and
``plot_solver_performance`` / ``plot_solver_hist`` (src/path_generator.py:190-195,479-568).

The reference prints a table of launch / front-end / MPC / solver times with mean, max and the number
of solver calls, optionally appends it to a file, and draws a histogram of per-step loop times.
Here the same quantities come back as text and as histogram arrays (plotting stays with the caller;
matplotlib is not a dependency of this package).
"""
from __future__ import annotations

import numpy as np


def runtime_analysis(time_dict: dict, solver_times, overhead_times=None, file_name: str = "") -> str:
    """Text block with the keys the reference reports (path_generator.py:479-533); appended to
    ``file_name`` when given, like the reference does."""
    st = np.asarray(solver_times, dtype=np.float64)
    lines = ["Runtime Analysis", "-" * 44]
    for key, label in (("opt_launch", "Launching optimizer"), ("prepare", "Prepare visibility graph"),
                       ("initial_guess", "Finding A* solution"), ("rough_ref", "Generating rough reference"),
                       ("mpc_time", "MPC loop"), ("solver_time", "  of which solver"), ("total_time", "Total")):
        if key in time_dict:
            lines.append(f"{label:<30}{float(time_dict[key]):>12.1f} ms")
    if st.size:
        lines += ["-" * 44, f"{'Solver calls':<30}{st.size:>12d}", f"{'Mean solver time':<30}{st.mean():>12.3f} ms",
                  f"{'Median solver time':<30}{np.median(st):>12.3f} ms", f"{'Max solver time':<30}{st.max():>12.3f} ms"]
    if overhead_times is not None and len(overhead_times):
        ov = np.asarray(overhead_times, dtype=np.float64)
        lines.append(f"{'Mean loop overhead':<30}{ov.mean():>12.3f} ms")
    text = "\n".join(lines) + "\n"
    if file_name:
        with open(file_name, "a") as fh:
            fh.write(text)
    return text


def loop_time_histogram(solver_times, overhead_times, bins: int = 30):
    """Histogram of per-step loop time = solver + overhead, what ``gen_runtime_plots.py:28-33`` plots.
    -> (counts, bin_edges)."""
    total = np.asarray(solver_times, dtype=np.float64) + np.asarray(overhead_times, dtype=np.float64)
    return np.histogram(total, bins=bins)


def batch_summary(status) -> dict:
    """Summary of a batched solve (status structured array): the numbers bench.py reports."""
    it = status["num_inner_iterations"].astype(np.float64)
    return {"solves": int(status.shape[0]), "converged_frac": float((status["exit_status"] == 0).mean()),
            "mean_inner_iters": float(it.mean()), "p50_inner_iters": float(np.median(it)),
            "p99_inner_iters": float(np.percentile(it, 99)), "max_inner_iters": int(it.max()),
            "mean_outer_iters": float(status["num_outer_iterations"].mean()),
            "exit_status_counts": {int(k): int(v) for k, v in zip(*np.unique(status["exit_status"], return_counts=True))}}


def _logged(loop):
    """-> (trajectory [rows, B, 3], controls, step_records, drive_summary, step_totals) of a loop that keeps a drive log: a
    ``DeviceRecedingHorizon`` or its host mirror ``FleetRecedingHorizon``, either with ``log=DriveLog()``."""
    if getattr(loop, "log", None) is None:
        raise ValueError("the loop keeps no drive log (log=DriveLog())")
    get = lambda name: (lambda v: v() if callable(v) else v)(getattr(loop, name))      # noqa: E731
    traj = loop.trajectory() if callable(getattr(loop, "trajectory", None)) else np.stack(loop.traj)
    return traj, get("controls"), get("step_records"), get("drive_summary"), get("step_totals")


def fleet_runs(loop):
    """What the reference's ``PathGenerator.run`` returns (src/path_generator.py:431-437), per robot of a logged loop: -> a list [B] of
    ``(xx, xy, uv, uomega, solver_times)``, cut at the robot's last driven row: ``rows`` controls, ``rows + 1`` poses and ``steps``
    solve times (ms), ``rows`` and ``steps`` the robot's summary's.  A robot that retired is cut where it stopped."""
    traj, ctrl, rec, summary, _ = _logged(loop)
    out = []
    for b in range(traj.shape[1]):
        rows, steps = int(summary["rows"][b]), int(summary["steps"][b])
        out.append((traj[:rows + 1, b, 0].tolist(), traj[:rows + 1, b, 1].tolist(), ctrl[:rows, b, 0].tolist(), ctrl[:rows, b, 1].tolist(),
                    rec["solve_time_ms"][:steps, b].tolist()))
    return out


def fleet_runtime_text(loop, file_name: str = "") -> str:
    """``runtime_analysis`` over the fleet of a logged loop, from its totals and summaries: the solver times are the steps' slowest solves
    (``solve_ms_max``: what a control period has to wait for), followed by the fleet's solves per exit status, its PANOC iterations and
    the largest acceleration any robot used."""
    from ._lib import EXIT_STATUS
    _, _, _, summary, tot = _logged(loop)
    ms = tot["solve_ms_max"][tot["solved"] > 0]
    text = runtime_analysis({"solver_time": float(ms.sum())}, ms)
    solves = int(tot["solved"].sum())
    lines = ["-" * 44, f"{'Robots':<30}{len(summary):>12d}", f"{'Steps':<30}{len(tot):>12d}", f"{'Solves':<30}{solves:>12d}"]
    for e, n in enumerate(tot["exits"].sum(axis=0).tolist()):
        if n:
            lines.append(f"{'  ' + EXIT_STATUS[e]:<30}{n:>12d}")
    lines.append(f"{'PANOC iterations':<30}{int(tot['inner_total'].sum()):>12d}")
    if len(tot):
        k = int(np.argmax(tot["inner_max"]))
        lines.append(f"{'  most in one solve':<30}{int(tot['inner_max'][k]):>12d}  (step {k + 1}, robot {int(tot['inner_max_robot'][k])})")
    if len(summary):
        lines += [f"{'Longest path':<30}{float(summary['length'].max()):>12.3f} m",
                  f"{'Largest |acceleration|':<30}{float(summary['acc_abs_max'].max()):>12.3f} m/s^2",
                  f"{'Largest |angular acc.|':<30}{float(summary['wacc_abs_max'].max()):>12.3f} rad/s^2"]
    more = "\n".join(lines) + "\n"
    if file_name:
        with open(file_name, "a") as fh:
            fh.write(more)
    return text + more


def ensemble_text(stats, group: int = 0) -> str:
    """One line per step for group ``group`` of an ensemble's records (``ensemble_stats()`` [steps, G] of a ``DeviceRecedingHorizon`` or
    its host mirror): the mean position, the semi-axes of the position's covariance ellipse (the square roots of the eigenvalues of
    [[xx, xy], [xy, yy]], the larger first), the standard deviation of the heading, the distance of the member furthest from the mean
    with its robot index, and the share of the members that have arrived."""
    st = np.asarray(stats)
    if st.ndim != 2 or not 0 <= group < st.shape[1]:
        raise ValueError(f"ensemble records of shape {st.shape} have no group {group}")
    lines = [f"Ensemble group {group}", f"{'step':>5}{'mean x':>10}{'mean y':>10}{'axis a':>10}{'axis b':>10}{'sd theta':>10}{'furthest':>10}{'robot':>7}{'arrived':>9}",
             "-" * 81]
    for k, r in enumerate(st[:, group]):
        n = int(r["n"])
        if n == 0:
            lines.append(f"{k + 1:>5}{'(no members)':>76}")
            continue
        xx, xy, yy, tt = (float(v) for v in r["cov"])
        half, det = (xx + yy) / 2, np.hypot((xx - yy) / 2, xy)
        a, b = np.sqrt(max(half + det, 0.0)), np.sqrt(max(half - det, 0.0))
        lines.append(f"{k + 1:>5}{float(r['mean'][0]):>10.4f}{float(r['mean'][1]):>10.4f}{a:>10.4f}{b:>10.4f}{np.sqrt(max(tt, 0.0)):>10.4f}"
                     f"{np.sqrt(max(float(r['far2']), 0.0)):>10.4f}{int(r['far_robot']):>7d}{int(r['arrived']) / n:>9.1%}")
    return "\n".join(lines) + "\n"


def tracking_summary(records) -> dict:
    """What a set of track-monitor records (``tracking()`` [n], ``_lib.TRACKING_DTYPE``) says as a whole, computed here on the host:
    the largest and the RMS cross-track error in metres (sums over all rows that had a closest segment: ``rows`` counts NaN poses too,
    which add nothing to the sums), the largest and the RMS heading error in radians (not wrapped, as the cost sees it), the share of
    rows off the route and of robots that ever were."""
    rec = np.asarray(records)
    rows = int(rec["rows"].sum())
    div = float(max(rows, 1))
    return {"robots": int(len(rec)), "rows": rows,
            "cte_max_m": float(np.sqrt(rec["cte2_max"].max(initial=0.0))), "cte_rms_m": float(np.sqrt(rec["cte2_sum"].sum() / div)),
            "dth_max_rad": float(rec["dth_max"].max(initial=0.0)), "dth_rms_rad": float(np.sqrt(rec["dth2_sum"].sum() / div)),
            "rows_off_frac": float(rec["off_rows"].sum() / div), "robots_off_frac": float((rec["off_rows"] > 0).mean()) if len(rec) else 0.0}


def tracking_text(records, group_of=None) -> str:
    """One line for the fleet and, with ``group_of`` [B], one per group (ascending group index) of a track monitor's records (``tracking()``
    [B] of a ``DeviceRecedingHorizon`` or its host mirror): the largest and the RMS cross-track error in metres, the share of rows off
    the route, the share of robots that ever were, and the largest heading error in radians (``tracking_summary``)."""
    rec = np.asarray(records)
    sets = [("fleet", np.ones(len(rec), dtype=bool))]
    if group_of is not None:
        g = np.asarray(group_of).reshape(-1)
        if len(g) != len(rec):
            raise ValueError(f"group_of of length {len(g)} for {len(rec)} records")
        sets += [(f"group {int(v)}", g == v) for v in np.unique(g)]
    lines = ["Route tracking", f"{'':<12}{'robots':>8}{'rows':>10}{'cte max m':>12}{'cte rms m':>12}{'rows off':>10}{'robots off':>12}{'dth max rad':>13}",
             "-" * 89]
    for name, sel in sets:
        s = tracking_summary(rec[sel])
        lines.append(f"{name:<12}{s['robots']:>8d}{s['rows']:>10d}{s['cte_max_m']:>12.4f}{s['cte_rms_m']:>12.4f}{s['rows_off_frac']:>10.1%}"
                     f"{s['robots_off_frac']:>12.1%}{s['dth_max_rad']:>13.4f}")
    return "\n".join(lines) + "\n"
