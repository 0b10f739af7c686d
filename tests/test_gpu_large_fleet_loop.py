"""GPU: the later stages of the on-device loop (csrc/nmpc_loop.h) on fleets of over a thousand robots and a crowd of 16 384 obstacles,
against the ``FleetRecedingHorizon`` mirror driven by the oracle and given the kernels' sin / cos.  After EVERY step the loop's arrays
(``step_differing``) and every product of every stage that is on -- the grid, the drive log (but the two fields a clock gives), the
plant's controls and poses, the ensemble's records, the walls, both monitors' records, the crowd's table, choices and records -- must be
the mirror's bits, and the trajectory at the end; there is no tolerance anywhere.  tests/test_large_fleet_mirror.py builds the fleets,
holds the mirror to the literal rules at these sizes, and owns the ``reach_*`` predicates called here on the mirror of every case: a
fleet that stops exercising its path fails, it does not pass emptily.

What each case makes a kernel do that no smaller case does:

* grid peers at B = 1100 and 2100: ``block_chunk`` hands a thread of ``nmpc_loop_peer_grid_kernel`` two and three robots and leaves
  the threads behind them empty; 53 x 52 cells (1 m) give the scan's ``block_chunk(cells + 1)`` three entries per thread (as the
  160 robots of tests/test_gpu_peers_grid_loop.py::test_more_than_a_wave do, one robot per thread), 128 x 128 (0.25 m) seventeen,
  and the ``cell_off`` zeroing loop further strides; at 0.25 m ``grid_axis`` takes the clamp branch, so ``h`` and every
  ``cellof`` with it (the grid kernel's and the window of ``nmpc_loop_peers_grid_kernel``) are the device's division.
* the drive log at B = 1100 and 2100: the stride loop of ``nmpc_loop_log_totals_kernel`` runs twice and three times, all sixteen
  waves feed the LDS combine, and thread 1 meets the step's ``inner_max`` in two strides (robots 1 and 1025).
* the retiring fleet: ``nmpc_loop_log_kernel``, ``nmpc_loop_measure_kernel`` and ``nmpc_loop_plant_kernel`` over five workgroups with
  ``n < B``, the compaction's chunks of two with retired and active robots side by side, ``arrived`` from ``retired_at``.
* the ensemble: groups of 550 (three strides of 256), of 733 and 367, of 1100 (five strides), and an empty one.
* the crowd: 256 obstacles per lane of ``nmpc_loop_crowd_kernel`` and ``nmpc_loop_crowd_monitor_kernel``, 1.6 M table entries per
  step of ``nmpc_loop_crowd_advance_kernel``; and 1000 obstacles at rows of 200 doubles.
* everything at once: every stage enqueued in one step, at 1100 robots.

Each test prints its wall time."""
import time

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd.workloads import (clearance_differing, ensemble_differing, log_differing, map_clearance_differing,
                                                    plant_differing, step_differing, trajectory_differing, walls_differing)
from test_gpu_crowd_loop import crowd_differing
from test_gpu_peers_grid_loop import _grid_differing
from test_gpu_peers_loop import _filled
from test_large_fleet_mirror import (CROWDS, ENSEMBLES, GRID_CASES, crowd_case, ensemble_case, everything_case, fill_counts, grid_case,
                                     log_case, mirror_of, reach_crowd, reach_ensemble, reach_everything, reach_fills, reach_grid, reach_log,
                                     reach_retiring, retiring_case)

pytestmark = pytest.mark.gpu


class Pair:
    """A case's device loop and its mirror, on a solver of their own; ``step()`` steps both and names everything that differs."""

    def __init__(self, c):
        from mpc_trajectory_generator_amd.solver import BatchSolver
        from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
        self.c, self.o = c, oracle_for(c.cfg, **c.opts)
        self.solver, self.dev = BatchSolver(c.cfg, max_batch=c.B, **c.opts), None
        try:
            self.dev = DeviceRecedingHorizon(self.solver, c.routes, c.starts, c.dyn, max_steps=c.steps, idx0=c.idx0, route_of=c.route_of, **c.kw)
            self.host = mirror_of(c, self.o)
        except Exception:
            self.close()
            raise

    def step(self):
        """-> (the names that differ, the device's parameter vectors)"""
        dev, host = self.dev, self.host
        bad, Pd, _ = step_differing(dev, host, self.o.warm_solve(threads=16))
        kw = self.c.kw
        if kw.get("peers") is not None and kw["peers"].cell is not None:
            bad += [f"grid {n}" for n in _grid_differing(dev, host.grid)]
        if kw.get("log") is not None:
            bad += log_differing(dev, host)
        if kw.get("plant") is not None:
            bad += plant_differing(dev, host)
        if kw.get("ensemble") is not None:
            bad += ensemble_differing(dev, host)
        if kw.get("walls") is not None:
            bad += walls_differing(dev, host)
        if kw.get("monitor") is not None:
            bad += [f"clearance.{n}" for n in clearance_differing(dev, host)]
        if kw.get("map_monitor") is not None:
            bad += [f"map_clearance.{n}" for n in map_clearance_differing(dev, host)]
        if kw.get("crowd") is not None:
            bad += crowd_differing(dev, host)
        return bad, Pd

    def close(self):
        if self.dev is not None:               # before its solver: a loop must not outlive the handle it was made on
            self.dev.close()
            self.dev = None
        self.solver.close()


_T0 = [0.0]


def _start():
    _T0[0] = time.perf_counter()


def _run(c, each=None):
    """Step a case's pair ``c.steps`` times, everything compared after every step and the trajectory at the end; ``each(host, Pd,
    drove)`` after every step (``drove``: the active robots as the step found them) -> (the mirror, the seconds since the module's
    last ``_start()``: building the case counts)."""
    pair = Pair(c)
    try:
        host = pair.host
        for k in range(c.steps):
            drove = np.ones(c.B, dtype=bool) if host.active is None else host.active.copy()
            bad, Pd = pair.step()
            assert not bad, f"step {k}: {bad}"
            if each is not None:
                each(host, Pd, drove)
        assert not trajectory_differing(pair.dev, host, c.steps)
    finally:
        pair.close()
    return host, time.perf_counter() - _T0[0]


@pytest.mark.parametrize("which", list(GRID_CASES))
def test_grid_peers_with_several_robots_and_cells_per_thread(which):
    _start()
    c = grid_case(which)
    counts, dims = [], []

    def each(host, Pd, drove):
        dims.append(reach_grid(c, host.grid))
        counts.append(fill_counts(host))
        assert np.array_equal(_filled(c.cfg, Pd, 0, host.peers.slots), host.peer_index >= 0)

    _, seconds = _run(c, each)
    reach_fills(counts)
    print(f"{which}: grids {dims}, fill counts {[n.tolist() for n in counts]}, {seconds:.1f} s")


@pytest.mark.parametrize("B", [1100, 2100])
def test_log_totals_over_several_strides(B):
    _start()
    c = log_case(B)
    host, seconds = _run(c, lambda host, Pd, drove: reach_log(host))
    tot = host.step_totals
    print(f"B = {B}: exits per step {tot['exits'].tolist()}, inner_max {tot['inner_max'].tolist()} at {tot['inner_max_robot'].tolist()}, {seconds:.1f} s")


def test_retiring_fleet_with_log_plant_and_ensemble():
    _start()
    c = retiring_case()
    seen = []

    def each(host, Pd, drove):
        reach_retiring(host, drove)
        seen.append(int(drove.sum()))

    host, seconds = _run(c, each)
    assert len(set(seen)) >= 3, "fewer than two steps at which somebody retired"
    print(f"robots driven per step {seen}, arrived {host.ensemble_stats()['arrived'].tolist()}, {seconds:.1f} s")


@pytest.mark.parametrize("which", list(ENSEMBLES))
def test_ensemble_groups_beyond_a_stride_and_beyond_1024(which):
    _start()
    c = ensemble_case(which)
    host, seconds = _run(c)
    st = host.ensemble_stats()
    reach_ensemble(which, st)
    print(f"{which}: n {st['n'][-1].tolist()}, furthest {st['far_robot'][-1].tolist()}, {seconds:.1f} s")


@pytest.mark.parametrize("which", CROWDS)
def test_crowd_with_many_obstacles_per_lane(which):
    """``d16384`` is also the setter's boundary: the most obstacles it takes (one more is refused:
    tests/test_gpu_crowd_loop.py::test_crowd_arguments_validated)."""
    _start()
    c = crowd_case(which)
    seen = []
    host, seconds = _run(c, lambda host, Pd, drove: seen.append(host.crowd_seen.copy()))
    reach_crowd(which, seen, host)
    print(f"{which}: largest chosen index {int(np.max(seen))}, observer's obstacles {host.crowd_clearance()['obstacle'].tolist()[:8]}, {seconds:.1f} s")


def test_everything_at_once():
    """Plant, crowd, grid peers, walls, retirement, both monitors, log and ensemble in one loop of 1100 robots."""
    _start()
    c = everything_case()
    seen = []

    def each(host, Pd, drove):
        seen.append((host.crowd_seen[:, 0] >= 0, host.peer_index[:, 0] >= 0, (host.wall_edge >= 0).any(axis=1)))
        assert np.array_equal(_filled(c.cfg, Pd, 2, 1)[:, 0][drove], (host.peer_index[:, 0] >= 0)[drove])      # slot 0 scripted, 1 the crowd's

    host, seconds = _run(c, each)
    reach_everything(host, seen)
    print(f"active after the steps {host.n_active}, grid {host.grid.nx} x {host.grid.ny}, {seconds:.1f} s")
