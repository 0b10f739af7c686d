"""The wall-clock limits (nmpc_set_time_limits) measured: one JSON line per measurement, to stdout and to profiles/<tag>/time_limits.jsonl.

  (a) overhead of the timed instantiation: the untimed kernel against the Timed<> kernel with an unreachable limit (1e6 ms), alternated
      A/B on one handle, the bench's batch (B = 8192, 32 planned routes) of cfg 1 and cfg 2; kernel ms from HIP events (last_batch_ms)
  (b) batch budget sweep {off, 30, 20, 10, 5, 2} ms on the same batches: kernel ms, converged / out-of-time / iteration-capped shares,
      and what stopping costs an instance: cost of its returned iterate against the untimed solve's (mean and max, over the instances
      the budget changed)
  (c) B = 1 through the reference-shaped handle (tcp_shim.OptimizerTcpManager(max_duration_micros=...)), cold calls of cfg 1: overshoot
      solve_time_ms - limit of the calls the limit stopped
usage: python scripts/time_limits.py [tag] [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpc_trajectory_generator_amd.solver import BatchSolver  # noqa: E402
from mpc_trajectory_generator_amd.tcp_shim import OptimizerTcpManager  # noqa: E402
from mpc_trajectory_generator_amd.workloads import baseline_batch  # noqa: E402

TAG = sys.argv[1] if len(sys.argv) > 1 else "time_limits"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
OUT = os.path.join("profiles", TAG)
os.makedirs(OUT, exist_ok=True)
sink = open(os.path.join(OUT, "time_limits.jsonl"), "a")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def shares(st):
    e = st["exit_status"]
    return {"converged": round(float(np.mean(e == 0)), 4), "out_of_time": round(float(np.mean(e == 2)), 4),
            "iteration_capped": round(float(np.mean(e == 1)), 4)}


for name in ("cfg1", "cfg2"):
    cfg, P = baseline_batch(name)
    s = BatchSolver(cfg, max_batch=len(P))
    u_ref, y_ref, st_ref = s.solve(P)                 # (warm-up, and the untimed solve (b) compares with)
    # (a) untimed | timed with an unreachable limit, alternated
    ms = {"untimed": [], "timed_unreachable": []}
    same = True
    for r in range(REPS):
        for leg in ("untimed", "timed_unreachable"):
            s.set_time_limits(0, 0) if leg == "untimed" else s.set_time_limits(1e6, 1e6)
            u, y, st = s.solve(P)
            ms[leg].append(s.last_batch_ms)
            same &= bool(np.array_equal(u, u_ref) and np.array_equal(y, y_ref))
    a, b = np.array(ms["untimed"]), np.array(ms["timed_unreachable"])
    emit({"part": "a", "cfg": name, "B": len(P), "reps": REPS, "untimed_ms": [round(x, 3) for x in a],
          "timed_ms": [round(x, 3) for x in b], "untimed_median": round(float(np.median(a)), 3),
          "timed_median": round(float(np.median(b)), 3), "overhead_pct": round(100 * (float(np.median(b)) / float(np.median(a)) - 1), 2),
          "same_bits": same})
    # (b) batch budget sweep
    for budget in (0.0, 30.0, 20.0, 10.0, 5.0, 2.0):
        s.set_time_limits(0, budget)
        kms = []
        for r in range(3):
            u, y, st = s.solve(P)
            kms.append(s.last_batch_ms)
        changed = ~(np.all(u == u_ref, axis=1) & (st["num_inner_iterations"] == st_ref["num_inner_iterations"]))
        dc = st["cost"][changed] - st_ref["cost"][changed]
        rel = dc / np.maximum(np.abs(st_ref["cost"][changed]), 1e-12)
        emit({"part": "b", "cfg": name, "B": len(P), "budget_ms": budget, "kernel_ms": [round(x, 3) for x in kms],
              **shares(st), "changed": int(changed.sum()),
              "cost_increase_mean": float(dc.mean()) if dc.size else 0.0, "cost_increase_max": float(dc.max()) if dc.size else 0.0,
              "cost_increase_rel_mean": float(rel.mean()) if rel.size else 0.0, "cost_increase_rel_max": float(rel.max()) if rel.size else 0.0,
              "inner_iterations_mean": float(st["num_inner_iterations"].mean()),
              "inner_iterations_untimed_mean": float(st_ref["num_inner_iterations"].mean())})
    s.close()

# (c) B = 1 through the shim, cold calls (zero guess and multipliers) of cfg 1's batch
cfg, P = baseline_batch("cfg1", B=48, seed=4)
for lim_us in (None, 500_000, 10_000, 5_000, 2_000, 1_000, 500):
    m = OptimizerTcpManager(config=cfg, max_batch=4, max_duration_micros=lim_us)
    m.start()
    t, status = [], []
    for p in P:
        g = m.call(p, initial_guess=[0.0] * cfg.n_u, initial_y=[0.0] * cfg.n1).get()
        t.append(g.solve_time_ms)
        status.append(g.exit_status)
    m.kill()
    t = np.array(t)
    rec = {"part": "c", "cfg": "cfg1", "calls": len(P), "max_duration_micros": lim_us, "solve_ms_median": round(float(np.median(t)), 4),
           "solve_ms_max": round(float(t.max()), 4), "out_of_time": int(sum(x == "NotConvergedOutOfTime" for x in status))}
    if lim_us is not None:
        stopped = np.array([x == "NotConvergedOutOfTime" for x in status])
        over = t[stopped] - lim_us / 1000.0
        rec.update({"overshoot_ms_median": round(float(np.median(over)), 4) if over.size else None,
                    "overshoot_ms_max": round(float(over.max()), 4) if over.size else None,
                    "overshoot_ms_min": round(float(over.min()), 4) if over.size else None})
    emit(rec)
