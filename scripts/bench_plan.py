#!/usr/bin/env python3
"""The batched planner (frontend.DevicePlanner) on B queries between collision-free points of a scene: planner
creation time, the planner kernels' time per batch (nmpc_planner_last_ms: the median of --repeat calls after a warm-up call), and in the
same run the host planner's `VisibilityPlanner.shortest_path` loop over the first --host-queries of the same queries, scaled to B.
--scene N: scene N of the reference; --scene grid: the synthetic 80-node scene (workloads.square_grid_planner).  --mirror: check the
device's answers against frontend.plan_batch_mirror, bit for bit.  Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mpc_trajectory_generator_amd import named_config                                            # noqa: E402
from mpc_trajectory_generator_amd.frontend import DevicePlanner, plan_batch_mirror, scene_planner   # noqa: E402
from mpc_trajectory_generator_amd.workloads import free_point_sampler, square_grid_planner       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="11")
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--host-queries", type=int, default=1024)
ap.add_argument("--mirror", action="store_true")
args = ap.parse_args()
cfg = named_config("cfg1")
pl = square_grid_planner(cfg) if args.scene == "grid" else scene_planner(cfg, int(args.scene))
sample = free_point_sampler(pl, np.random.Generator(np.random.PCG64(0)))
B = args.batch
q = np.array([[*sample(), *sample()] for _ in range(B)])
starts, goals = q[:, :2].copy(), q[:, 2:].copy()
t = time.perf_counter()
dp = DevicePlanner(pl, max_batch=B)
create_ms = 1e3 * (time.perf_counter() - t)
res = dp.plan(starts, goals)                       # warm-up
ms, wall = [], []
for _ in range(args.repeat):
    t = time.perf_counter()
    res = dp.plan(starts, goals)
    wall.append(1e3 * (time.perf_counter() - t))
    ms.append(dp.last_ms)
out = {"metric": "plan_ms", "value": statistics.median(ms), "unit": "ms", "scene": args.scene, "queries": B, "nodes": dp.V,
       "edges": len(dp.scene.edges), "plan_ms_all": ms, "plan_call_wall_ms_median": statistics.median(wall), "planner_creation_ms": create_ms,
       "reachable_frac": float((res.n_wp > 0).mean()), "mean_waypoints": float(res.n_wp[res.n_wp > 0].mean())}
if args.mirror:
    want = plan_batch_mirror(pl, starts, goals)
    out["equals_mirror"] = all(getattr(res, f).tobytes() == getattr(want, f).tobytes() for f in ("n_wp", "wp", "length", "vis"))
dp.close()
n = min(args.host_queries, B)
if n:
    t = time.perf_counter()
    for s, g in zip(starts[:n], goals[:n]):
        try:
            pl.shortest_path(s, g)
        except ValueError:
            pass
    host = 1e3 * (time.perf_counter() - t)
    out.update({"host_shortest_path_ms": host, "host_queries": n, "host_ms_scaled_to_batch": host * B / n})
print(json.dumps(out))
