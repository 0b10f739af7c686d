"""One hard instance solved alone (a single wavefront on the chip), twice: the workload of lone-wave PMC runs."""
import sys
import numpy as np
sys.path.insert(0, ".")
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch
cfg, P = baseline_batch("cfg1")
sol = BatchSolver(cfg, max_batch=8192)
b = int(sys.argv[1]) if len(sys.argv) > 1 else 170
for _ in range(2):
    u, y, st = sol.solve(P[b:b + 1])
print("launches 2 passes/launch", int(st["reserved"][0]), "iters/launch", int(st["num_inner_iterations"][0]), "ms", sol.last_batch_ms)
