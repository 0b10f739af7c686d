"""Full batches of every BASELINE config, several seeds: two launches (the second on a permuted batch) must give the same bits, and a sample must equal the oracle's.
The long version of tests/test_gpu_fullbatch.py's permutation test -- what catches a scheduler-dependent miscompilation (csrc/Makefile).  usage: python scripts/determinism_check.py [seeds...]"""
import sys, numpy as np
sys.path.insert(0, ".")
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch, differing
from oracle import Oracle
seeds = [int(a) for a in sys.argv[1:]] or [1, 2, 3]
bad = 0
for name in ("cfg1", "cfg2", "cfg3", "cfg4"):
    cfg = named_config(name)
    sol = BatchSolver(cfg, max_batch=8192)
    for seed in seeds:
        P = baseline_batch(name, seed=seed)[1]
        res = sol.solve(P)
        perm = np.random.default_rng(seed).permutation(8192)
        same = not differing(res, sol.solve(P[perm]), perm)
        idx = np.random.default_rng(100 + seed).choice(8192, 48, replace=False)
        par = not differing(res, Oracle.for_config(cfg).solve_batch(P[idx], threads=16), idx)
        print(name, "seed", seed, sol.kernel_name, "permutation-invariant", same, "sample == oracle", par, "ms", round(sol.last_batch_ms, 1), flush=True)
        bad += (not same) + (not par)
    sol.close()
print("DETERMINISM_OK" if bad == 0 else f"FAILURES {bad}")
sys.exit(1 if bad else 0)
