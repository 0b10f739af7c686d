"""Do a kernel's results depend on what the registers / LDS held before it started?  The batch is solved after scrubbing every SIMD's
register file and every CU's LDS (tests/scrub/scrub.hip) with different patterns; a difference means an uninitialised read.  Each figure
is the number of outputs (u, y, the status fields of workloads.PARITY_FIELDS) that are not the same bits: 0 = none.
usage: [NMPC_LIB_PATH=...] python scripts/scrub_probe.py tag [cfgN ...]"""
import ctypes, json, os, sys
sys.path.insert(0, ".")
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch, differing

scrub = ctypes.CDLL(os.path.join("tests", "scrub", "libscrub.so"))
tag = sys.argv[1]
for name in (sys.argv[2:] or ["cfg2"]):
    cfg, P = baseline_batch(name)
    s = BatchSolver(cfg, max_batch=len(P))
    res = []
    for pat in (0x00000000, 0x7ff80000, 0xdeadbeef, 0x00000000):
        rc = scrub.nmpc_scrub(0, ctypes.c_uint(pat), 4096, 160 * 1024)
        assert rc == 0, rc
        res.append(s.solve(P))
    print(json.dumps({"lib": tag, "cfg": name, "kernel": s.kernel_name, "zero_vs_nan": len(differing(res[0], res[1])), "zero_vs_beef": len(differing(res[0], res[2])), "zero_vs_zero": len(differing(res[0], res[3]))}), flush=True)
    s.close()
