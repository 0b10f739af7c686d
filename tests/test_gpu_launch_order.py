"""GPU: the launch order (csrc/nmpc_order.h) against its literal rule (tests/launch_order_reference.py), integer
for integer: there is no tolerance anywhere.  The order is read through the experiments build's ``BatchSolver.launch_order()`` and
``BatchSolver.order_of()``; the product library exports neither (tests/test_abi.py).

* levels from the inputs (``nmpc_classify_kernel``): the workload batches of every configuration and four run-time shapes, a leading
  block of each overwritten by the crafted instances of tests/test_launch_order_literal.py -- every level, every comparison of the
  rule from both sides.  The solves behind them are cut to one PANOC iteration: the order kernels run whatever the solve takes.
* the order (``nmpc_order_kernel``) is the stable partition of those levels, and of level vectors handed in through ``order_of`` at
  the sizes around the block's 1024 threads and their multiples, where chunks of one, two, eight and twenty instances meet empty ones.
* levels from the previous pass counts (``nmpc_classify_prev_kernel``) at every power of two of a uint32.
* no order where none is used, and the closed loop's hint: a retiring fleet of 2208 robots stepped beside its mirror, whose levels
  must be those of the very robots each gathered row holds.

tests/test_launch_order_literal.py holds the fixtures to the rule on the CPU; each test here prints its wall time."""
import time

import numpy as np
import pytest

from conftest import oracle_for
from launch_order_reference import LEVELS, level_from_passes, stable_partition
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.workloads import step_differing
from test_large_fleet_mirror import mirror_of
from test_launch_order_literal import (HINT_WAVES, SHAPES, hint_case, levels_of, reach_hint, shape_workload, with_crafted, workload)

pytestmark = pytest.mark.gpu

TRIVIAL = dict(max_inner=1, max_outer=1)       # the solve is not the subject
INPUT_CASES = [(name, B) for name in ("cfg1", "cfg3", "cfg4") for B in (2600, 8192)] + [("cfg2", 2100)] + [(s, 2100) for s in SHAPES]
ORDER_SIZES = [1, 2, 1023, 1024, 1025, 2047, 2048, 8191, 8192, 20000]
MAX_ORDER = 20000

_BATCHES = {}


def reference_batch(key):
    """-> (cfg, P, names of the crafted block, the literal rule's levels), at the largest size the key is checked at; computed once.
    (The generator draws instance after instance, so the first 2600 rows are the batch of 2600.)"""
    if key not in _BATCHES:
        B = max(b for k, b in INPUT_CASES if k == key)
        cfg, P = workload(key, B) if isinstance(key, str) else shape_workload(key, B)
        P, names = with_crafted(cfg, P)
        _BATCHES[key] = (cfg, P, names, levels_of(cfg, P))
    return _BATCHES[key]


def new_solver(cfg, max_batch, **opts):
    from mpc_trajectory_generator_amd.solver import BatchSolver
    return BatchSolver(cfg, max_batch=max_batch, experiments=True, **opts)


def assert_partition(cls, order, what=""):
    B = len(cls)
    assert len(order) == B and sorted(order.tolist()) == list(range(B)), f"{what}: not a permutation of 0..{B - 1}"
    want = stable_partition(cls.tolist())
    if order.tolist() != want:
        at = int(np.nonzero(order != np.array(want))[0][0])
        raise AssertionError(f"{what}: position {at} holds {order[at]} (level {cls[order[at]]}), the stable partition {want[at]} (level {cls[want[at]]})")


@pytest.mark.parametrize("key,B", INPUT_CASES, ids=[f"{k if isinstance(k, str) else 'n%d-o%d-d%d' % k}-b{b}" for k, b in INPUT_CASES])
def test_levels_from_inputs_equal_the_literal_rule(key, B):
    t0 = time.perf_counter()
    cfg, P, names, levels = reference_batch(key)
    P, levels = P[:B], levels[:B]
    t1 = time.perf_counter()
    s = new_solver(cfg, B, **TRIVIAL)
    try:
        s.solve(P)
        n, from_prev, cls, order = s.launch_order()
    finally:
        s.close()
    assert (n, from_prev) == (B, 0)
    wrong = np.nonzero(cls != levels)[0]
    assert not len(wrong), (f"{len(wrong)} instances, the first: " +
                            ", ".join(f"{b} ({names[b] if b < len(names) else 'workload'}): level {cls[b]}, the rule {levels[b]}" for b in wrong[:8]))
    assert_partition(cls, order, "the launch's order")
    counts = np.bincount(levels, minlength=LEVELS)
    assert (counts > 0).sum() >= (LEVELS if cfg.Nobs else 4)        # (the crafted block alone reaches them)
    print(f"levels {counts.tolist()}, reference {t1 - t0:.1f} s, all {time.perf_counter() - t0:.1f} s")


@pytest.fixture(scope="module")
def order_solver():
    s = new_solver(named_config("cfg1"), MAX_ORDER, **TRIVIAL)
    yield s
    s.close()


def passes_of(levels):
    """pass counts that give the levels: 0 -> level 0, 16 << l -> level l"""
    levels = np.asarray(levels, dtype=np.uint32)
    return np.where(levels == 0, 0, np.uint32(16) << levels).astype(np.uint32)


def level_vectors(B):
    rng = np.random.default_rng(B)
    lone = np.zeros(B, dtype=int)
    lone[B - 1] = 12
    return {"one level": np.full(B, 7), "cycling": np.arange(B) % LEVELS, "ascending": np.arange(B) * LEVELS // B,
            "descending": (LEVELS - 1) - np.arange(B) * LEVELS // B, "a lone 12 at the end": lone, "random": rng.integers(0, LEVELS, B)}


@pytest.mark.parametrize("B", ORDER_SIZES)
def test_order_is_the_stable_partition(order_solver, B):
    t0 = time.perf_counter()
    for what, levels in level_vectors(B).items():
        cls, order = order_solver.order_of(passes_of(levels))
        assert np.array_equal(cls, levels), f"{what}: the levels handed in came out differently"
        assert_partition(cls, order, f"B = {B}, {what}")
    print(f"B = {B}: {time.perf_counter() - t0:.2f} s")


def test_levels_from_passes_at_every_power_of_two(order_solver):
    t0 = time.perf_counter()
    n = [0, 31, 32, 63, 64] + [v for k in range(1, 32) for v in (2 ** k - 1, 2 ** k)] + [2 ** 31 + 1, 2 ** 32 - 1]
    cls, order = order_solver.order_of(np.array(n, dtype=np.uint32))
    want = [level_from_passes(v) for v in n]
    assert cls.tolist() == want, [(v, int(c), w) for v, c, w in zip(n, cls, want) if c != w]
    assert_partition(cls, order)
    assert set(want) == set(range(LEVELS))
    print(f"{time.perf_counter() - t0:.2f} s")


def test_order_readers_need_the_experiments_build():
    from mpc_trajectory_generator_amd.solver import BatchSolver, SolverError
    s = BatchSolver(named_config("cfg1"), max_batch=8, **TRIVIAL)
    try:
        with pytest.raises(SolverError):
            s.launch_order()
        with pytest.raises(SolverError):
            s.order_of([1, 2, 3])
        assert not hasattr(s.lib, "nmpc_debug_launch_order") and not hasattr(s.lib, "nmpc_debug_order_of")
    finally:
        s.close()


def test_no_order_where_none_is_used(monkeypatch):
    t0 = time.perf_counter()
    cfg, P, _, levels = reference_batch("cfg1")
    s = new_solver(cfg, 2600, **TRIVIAL)
    try:
        s.solve(P[:2600])
        n, from_prev, cls, order = s.launch_order()
        assert (n, from_prev) == (2600, 0) and np.array_equal(cls, levels[:2600])
        s.solve(P[:64])                                        # within the resident waves: fetched in index order
        n, from_prev, cls, order = s.launch_order()
        assert (n, from_prev, len(cls), len(order)) == (0, 0, 0, 0)
    finally:
        s.close()
    monkeypatch.setenv("NMPC_ORDER", "0")
    s = new_solver(cfg, 2600, **TRIVIAL)
    try:
        s.solve(P[:2600])
        assert s.launch_order()[:2] == (0, 0)
    finally:
        s.close()
    print(f"{time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("from_prev", [True, False], ids=["hint", "NMPC_LOOP_ORDER_PREV=0"])
def test_closed_loop_orders_by_the_gathered_robots_previous_passes(monkeypatch, from_prev):
    """Before each step the statuses and the active list are read, after it the launch's order: from the second step on the level of
    gathered row i must be that of robot act[i]'s previous pass count -- which it is only if the gather carries the status row along
    -- and the order its stable partition.  Step 0, and every step with the knob off, goes by the inputs.  The mirror is stepped
    beside the hinted loop and must agree bit for bit, as everywhere."""
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    t0 = time.perf_counter()
    monkeypatch.setenv("NMPC_WAVES_PER_CU", "4")               # 1024 resident waves: more robots than that stay active as they retire
    if not from_prev:
        monkeypatch.setenv("NMPC_LOOP_ORDER_PREV", "0")
    c = hint_case()
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o) if from_prev else None
    solver, dev = new_solver(c.cfg, c.B, **c.opts), None
    reached, driven = [], []
    try:
        dev = DeviceRecedingHorizon(solver, c.routes, c.starts, c.dyn, max_steps=c.steps, idx0=c.idx0, route_of=c.route_of, **c.kw)
        for k in range(c.steps):
            act = np.nonzero(dev.active()[1] < 0)[0]
            passes = dev.read()[4]["reserved"]
            if host is not None:
                bad, Pd, _ = step_differing(dev, host, o.warm_solve(threads=16))
                assert not bad, f"step {k}: {bad}"
            else:
                dev.step()
                Pd = dev.params()[0]
            n, prev, cls, order = solver.launch_order()
            assert n == len(act), f"step {k}: the launch ordered {n} instances, the step drove {len(act)}"
            driven.append(n)
            if from_prev and k >= 1:
                assert prev == 1, f"step {k}: the levels did not come from the statuses"
                want = np.array([level_from_passes(v) for v in passes[act]])
                reached.append(reach_hint(act, want, c.B))
            else:
                assert prev == 0, f"step {k}: the levels came from the statuses"
                want = levels_of(c.cfg, Pd[act])
            wrong = np.nonzero(cls != want)[0]
            assert not len(wrong), f"step {k}: rows {wrong[:8]} (robots {act[wrong[:8]]}): levels {cls[wrong[:8]]}, the rule {want[wrong[:8]]}"
            assert_partition(cls, order, f"step {k}")
            assert n > HINT_WAVES
    finally:
        if dev is not None:
            dev.close()
        solver.close()
    assert len(set(driven)) >= 3, f"robots driven per step {driven}: fewer than two steps at which somebody retired"
    if from_prev:
        assert sum(reached) >= 2, f"conditions reached at steps 1.. {reached}"
    print(f"robots driven per step {driven}, conditions reached {reached}, {time.perf_counter() - t0:.1f} s")
