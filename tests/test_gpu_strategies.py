"""GPU: the two-stage kernel (BASELINE config 2, N_hor = 40; the kernel at the edge of the register file) built under FOUR machine-scheduler
strategies must give the same bits under each: oracle-exact on a sample, invariant under a permutation of the batch, and independent of what
the registers and the LDS held before the launch (tests/scrub).  Round 3 had builds of this kernel whose results changed from run to run and
filed them under "miscompilation"; the causes are in mpc_trajectory_generator_amd/codegen_check.py, whose checks every variant must pass too.
The solve is deterministic in the reference (src/mpc/mpc_generator.py:206-214: same p, same u*)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from conftest import oracle_for
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.workloads import baseline_batch, differing
B = 8192
cfg, P = baseline_batch(os.environ.get("PROBE_CFG", "cfg2"), B)
scrub = ctypes.CDLL(os.path.join("tests", "scrub", "libscrub.so"))
s = BatchSolver(cfg, max_batch=B)
assert scrub.nmpc_scrub(0, ctypes.c_uint(0), 4096, 160 * 1024) == 0
r0 = s.solve(P)
assert scrub.nmpc_scrub(0, ctypes.c_uint(0x7ff80000), 4096, 160 * 1024) == 0      # every register a NaN, every LDS word half of one
r1 = s.solve(P)
perm = np.random.default_rng(0).permutation(B)
assert scrub.nmpc_scrub(0, ctypes.c_uint(0xdeadbeef), 4096, 160 * 1024) == 0
r2 = s.solve(P[perm])
idx = np.random.default_rng(1).choice(B, 24, replace=False)
par = not differing(r0, oracle_for(cfg).solve_batch(P[idx], threads=16), idx)
print(json.dumps({"kernel": s.kernel_name, "scrub_independent": not differing(r0, r1), "permutation_invariant": not differing(r0, r2, perm), "sample_equals_oracle": par,
                  "checksum": float(r0[0].sum()), "ms": s.last_batch_ms}))
"""


def run_probe(lib, config="cfg2"):
    env = dict(os.environ, PROBE_CFG=config)
    if lib:
        env["NMPC_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, "-c", PROBE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


@pytest.mark.parametrize("strategy", ["iterative-ilp (shipped)", "default", "max-memory-clause", "max-ilp"])
def test_two_stage_kernel_same_bits_under_every_scheduler(strategy):
    from mpc_trajectory_generator_amd import _lib
    if strategy.startswith("iterative-ilp"):
        _lib.load_library()            # (builds the library, and with it build_info.json, if this checkout has none yet)
        check, lib = _lib.build_info().get("codegen_check", {}), None
    else:
        check, lib = _lib.build_variant(strategy), _lib.variant_path(strategy)
    assert check.get("ok"), f"code-generation check failed for {strategy}: {check}"
    res = run_probe(lib)
    assert res["kernel"] == "nmpc_solve_hyb2_kernel<ShapeN40>"
    assert res["sample_equals_oracle"], res
    assert res["permutation_invariant"], res
    assert res["scrub_independent"], res


@pytest.mark.parametrize("strategy", ["default", "max-memory-clause", "max-ilp"])
def test_headline_kernel_has_tested_fallback_strategies(strategy):
    """The shipped build needs an LLVM-internal scheduler option (iterative-ilp) and a code-generation gate; a toolchain that drops the
    option or trips the gate must not leave the project without a library.  The HEADLINE kernel (BASELINE config 1) built under the three
    other strategies passes the gate and gives the same bits -- oracle-exact on a sample, permutation-invariant, scrub-independent --
    only slower (`make SCHED=...` builds it)."""
    from mpc_trajectory_generator_amd import _lib
    check = _lib.build_variant(strategy)
    assert check.get("ok"), f"code-generation check failed for {strategy}: {check}"
    res = run_probe(_lib.variant_path(strategy), "cfg1")
    assert res["kernel"] == "nmpc_solve_hyb_kernel<ShapeDefault>"
    assert res["sample_equals_oracle"] and res["permutation_invariant"] and res["scrub_independent"], res


@pytest.mark.parametrize("config", ["cfg1", "cfg2"])
def test_full_scan_build_gives_the_same_bits(config):
    """-DNMPC_WIN=0 (a documented setting of the kernels: the cross-track search always as the full scan) keeps the obstacle certificate, and with
    it the helper-side guard of what a helper lane has learnt about an owner's tables: that guard must not depend on the window being compiled in
    (advisor, round 5).  Same bits as the oracle on a sample, permutation-invariant, scrub-independent -- and a small batch in the team mode (every
    instance with three helpers from its first iteration) equals the oracle instance for instance."""
    from mpc_trajectory_generator_amd import _lib
    check = _lib.build_variant("win0")
    assert check.get("ok"), f"code-generation check failed for the -DNMPC_WIN=0 build: {check}"
    res = run_probe(_lib.variant_path("win0"), config)
    assert res["sample_equals_oracle"] and res["permutation_invariant"] and res["scrub_independent"], res
    small = r"""
import json, sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from conftest import oracle_for
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.solver import BatchSolver
from mpc_trajectory_generator_amd.harness import synthetic_batch
from mpc_trajectory_generator_amd.workloads import differing
cfg = named_config(sys.argv[1])
P = synthetic_batch(cfg, 11, 40, 4711)
s = BatchSolver(cfg, max_batch=64)
ok = True
for rep in range(3):
    ok = ok and not differing(s.solve(P), oracle_for(cfg).solve_batch(P, threads=16))
print(json.dumps({"ok": ok}))
"""
    r = subprocess.run([sys.executable, "-c", small, config], cwd=ROOT, env=dict(os.environ, NMPC_LIB_PATH=_lib.variant_path("win0")),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().split("\n")[-1])["ok"]


def test_headline_kernels_do_not_read_what_they_did_not_write():
    """The shipped library, all four BASELINE configurations: the results do not depend on the register / LDS content left by earlier waves."""
    r = subprocess.run([sys.executable, "scripts/scrub_probe.py", "shipped", "cfg1", "cfg3", "cfg4"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [json.loads(l) for l in r.stdout.strip().split("\n") if l.startswith("{")]
    assert len(rows) == 3
    for row in rows:
        assert row["zero_vs_nan"] == 0 and row["zero_vs_beef"] == 0 and row["zero_vs_zero"] == 0, row
