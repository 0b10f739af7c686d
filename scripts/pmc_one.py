"""Two launches of the headline batch (for rocprofv3 --pmc runs); prints the pass / evaluation totals the
counter values are divided by."""
import sys
import numpy as np
sys.path.insert(0, ".")
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch
cfg, P = baseline_batch("cfg1")
sol = BatchSolver(cfg, max_batch=8192)
for _ in range(2):
    u, y, st = sol.solve(P)
print("launches 2 passes/launch", int(st["reserved"].astype(np.int64).sum()), "iters/launch", int(st["num_inner_iterations"].astype(np.int64).sum()),
      "evals/launch", int((st["num_cost_evals"].astype(np.int64) + st["num_grad_evals"]).sum()), "ms", sol.last_batch_ms)
