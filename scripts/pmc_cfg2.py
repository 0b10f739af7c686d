import sys
import numpy as np
sys.path.insert(0, ".")
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch
cfg, P = baseline_batch("cfg2")
sol = BatchSolver(cfg, max_batch=8192)
for _ in range(2):
    u, y, st = sol.solve(P)
ev = (st["num_cost_evals"].astype(np.int64) + st["num_grad_evals"]).sum()
print("launches 2 passes/launch", int(st["reserved"].astype(np.int64).sum()), "evals/launch", int(ev), "iters", int(st["num_inner_iterations"].astype(np.int64).sum()), "ms", sol.last_batch_ms)
