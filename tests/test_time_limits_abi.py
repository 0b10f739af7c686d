"""CPU: the wall-clock limits' interface (nmpc_set_time_limits, include/nmpc_solver.h) is declared, exported and reachable from
Python, without a GPU: the library entry point, BatchSolver's and OptimizerTcpManager's keywords.  What the limits do is
tests/test_gpu_time_limits.py."""
import inspect
import os
import re

import pytest

from conftest import ROOT
from mpc_trajectory_generator_amd import _lib, named_config


def test_library_exports_set_time_limits():
    lib = _lib.load_library()
    assert hasattr(lib, "nmpc_set_time_limits")
    assert "nmpc_set_time_limits" in _lib.SYMBOLS
    # a NULL handle is an argument error, before anything touches a device
    assert lib.nmpc_set_time_limits(None, 1.0, 2.0) == -3


def test_header_declares_set_time_limits():
    header = open(os.path.join(ROOT, "include", "nmpc_solver.h")).read()
    decl = re.search(r"int\s+nmpc_set_time_limits\s*\(([^)]*)\)\s*;", header)
    assert decl, "nmpc_set_time_limits is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["nmpc_handle *h", "double max_duration_ms", "double batch_budget_ms"]
    # additive: the ABI version and the option / status structs stay as they are
    assert re.search(r"#define NMPC_ABI_VERSION 3\b", header)


def test_batch_solver_accepts_time_limit_keywords():
    from mpc_trajectory_generator_amd.solver import BatchSolver
    sig = inspect.signature(BatchSolver.__init__)
    for k in ("max_duration_ms", "batch_budget_ms"):
        assert k in sig.parameters and sig.parameters[k].default == 0.0, k
    assert list(inspect.signature(BatchSolver.set_time_limits).parameters) == ["self", "max_duration_ms", "batch_budget_ms"]
    # the limits are not solver options: they never reach nmpc_opts
    assert not any(f in ("max_duration_ms", "batch_budget_ms") for f, _ in _lib.NmpcOpts._fields_)


def test_tcp_manager_accepts_max_duration_micros():
    from mpc_trajectory_generator_amd.tcp_shim import OptimizerTcpManager
    cfg = named_config("cfg1")
    assert inspect.signature(OptimizerTcpManager.__init__).parameters["max_duration_micros"].default is None
    m = OptimizerTcpManager(config=cfg, max_duration_micros=500_000)      # the reference's MAX_SOVLER_TIME (no device touched before start())
    assert m._max_duration_ms == 500.0
    assert OptimizerTcpManager(config=cfg)._max_duration_ms == 0.0
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError):
            OptimizerTcpManager(config=cfg, max_duration_micros=bad)
