"""CPU: the fleets of tests/test_gpu_large_fleet_loop.py -- over a thousand robots, sixteen thousand obstacles -- and, on the host mirror
alone, the proof that each of them contains what it is there for (the ``reach_*`` predicates, which the GPU module calls again on the
mirror it compares the device with): a grid of more than 2048 cells and a capped one, chunks of two and three robots, every fill count
of the peer slots, an ``inner_max`` tied between a robot and the one 1024 places behind it, mixed exits, ``0 < n_active < B`` over more
than two workgroups, groups of 550 and of 1100 members, chosen obstacles beyond index 8192.

The literal rules of the smaller suites are held at these sizes where that is cheap: the ensemble's tree at n = 1100 and 2049, the
ensemble's records against ``literal_stats``, the log's totals against a loop over robots, and ``peer_grid``'s candidates against all
pairs on the capped grid at B = 1100.

The oracle solves.  Where the subject is the parameter vector (peers, crowd, everything at once) it is given ``max_total_inner`` = 40,
which makes a step of 1100 robots cost tenths of a second; the log cases get 1000, so that exits 0, 1 and 2 all occur."""
import types

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import frontend, named_config
from mpc_trajectory_generator_amd.trajectory import (CROWD_MAX, PEER_GRID_CAP, Crowd, DriveLog, Ensemble, FleetRecedingHorizon, MapMonitor,
                                                     Monitor, Peers, ensemble_sum)
from mpc_trajectory_generator_amd.workloads import (ensemble_differing, fleet_ellipses, move_near_goal, placed_fleet, staggered_fleet,
                                                    tiled_fleet)
from test_crowd_mirror import filled, narrow_range, scattered
from test_ensemble_mirror import bits, literal_stats, literal_sum, tree_values
from test_loop_shapes_mirror import mixed_chunks
from test_peers_grid_mirror import all_pairs
from test_plant_mirror import plant_of
from test_walls_mirror import scene_map, walls_of

SEED = 43                    # frontend.random_fleet(cfg, 11, 4, B, SEED): the fleet of test_gpu_peers_grid_loop.test_more_than_a_wave, larger
RX, RY = 0.37, 0.53          # radii no scripted, padding or crowd ellipse has
CHEAP = {"max_total_inner": 40}        # the solve is not the subject
LOG_BUDGET = 1000
THREADS = 1024               # of the single-workgroup kernels (peer grid, log totals, compaction)
STEPS = 3


def case(cfg, fleet, opts, steps=STEPS, dyn=None, **kw):
    """A fleet, the solver options (``BatchSolver`` and the oracle take the same names) and the loop's stages ``kw``, as both
    ``FleetRecedingHorizon`` and ``DeviceRecedingHorizon`` take them."""
    routes, route_of, starts, idx0 = fleet
    return types.SimpleNamespace(cfg=cfg, routes=routes, route_of=route_of, starts=starts, idx0=idx0, dyn=dyn, opts=opts, steps=steps,
                                 kw=kw, B=len(starts))


def mirror_of(c, o):
    return FleetRecedingHorizon(c.routes, c.route_of, c.starts, c.dyn, sincos=o.sincos_array, idx0=c.idx0, **c.kw)


def big_fleet(B, name="cfg1"):
    cfg = named_config(name)
    return cfg, frontend.random_fleet(cfg, 11, 4, B, seed=SEED)


# ---- grid peers ----
GRID_CASES = {"b1100-cell1": (1100, 1.0), "b1100-cell025": (1100, 0.25), "b2100-cell025": (2100, 0.25)}
GRID_SLOTS = 3


def second_neighbour_range(starts):
    """The median over robots of the distance to the second nearest robot at the start: where a bisection on the range for "half of
    the robots find two peers" ends.  At step 0 everybody is predicted to stand still, so about half of the fleet has two peers or
    more and half has fewer: all of 0 .. 3 filled slots occur."""
    d = np.linalg.norm(starts[:, None, :2] - starts[None, :, :2], axis=2)
    d[np.eye(len(starts), dtype=bool)] = np.inf
    return float(np.median(np.sort(d, axis=1)[:, 1]))


def grid_case(which):
    B, cell = GRID_CASES[which]
    cfg, fleet = big_fleet(B)
    peers = Peers(slots=GRID_SLOTS, rx=RX, ry=RY, range=second_neighbour_range(fleet[2]), cell=cell)      # one group of everybody
    return case(cfg, fleet, CHEAP, peers=peers)


def reach_grid(c, grid):
    """What a step's grid (the mirror's) makes ``nmpc_loop_peer_grid_kernel`` do."""
    B, cell = c.B, c.kw["peers"].cell
    assert -(-B // THREADS) >= 2, "one robot per thread"
    assert grid.filed == B
    cells = grid.nx * grid.ny
    if cell == 1.0:
        assert cells + 1 > 2 * THREADS and max(grid.nx, grid.ny) < PEER_GRID_CAP and (grid.h == cell).all(), (grid.nx, grid.ny)
    else:
        assert grid.nx == grid.ny == PEER_GRID_CAP and (grid.h > cell).all(), (grid.nx, grid.ny, grid.h)
    assert -(-(cells + 1) // THREADS) >= 3                     # the scan's chunks, and the zeroing loop's strides
    return grid.nx, grid.ny


def fill_counts(host):
    """-> [M + 1]: how many robots have 0 .. M peers at the step just taken"""
    return np.bincount((host.peer_index >= 0).sum(axis=1), minlength=host.peers.slots + 1)


def reach_fills(counts):
    total = np.sum(counts, axis=0)
    assert (total > 0).all(), f"fill counts {total.tolist()}: a number of filled slots never occurs"


@pytest.mark.parametrize("which", list(GRID_CASES))
def test_grid_fleets_reach_chunks_the_cap_and_every_fill_count(which):
    c = grid_case(which)
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    counts, dims = [], []
    for k in range(c.steps):
        _, st = host.step(o.warm_solve(threads=8))
        dims.append(reach_grid(c, host.grid))
        counts.append(fill_counts(host))
        assert (st["exit_status"] == 2).all()                  # the budget of 40 ends every solve
    print(which, "range", c.kw["peers"].range, "grids", dims, "fill counts", [n.tolist() for n in counts])
    reach_fills(counts)


def test_capped_grid_candidates_hold_every_peer_at_1100():
    """On the capped grid of the 0.25 m case, after a step (so that the predictions move): every j with D(b, j) < range^2 by the
    all-pairs expression is among b's candidates, and the grid prunes."""
    c = grid_case("b1100-cell025")
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    host.step(o.warm_solve(threads=8))
    pred = host.predict()                                      # what the second step's grid is built from
    host.step(o.warm_solve(threads=8))
    grid, rng_ = host.grid, c.kw["peers"].range
    assert grid.nx == grid.ny == PEER_GRID_CAP and not np.array_equal(pred[:, 0], pred[:, -1])
    want = all_pairs(pred, rng_)
    n_cand = []
    for b in range(c.B):
        cand = grid.candidates(b)
        missed = set(np.nonzero(want[b])[0].tolist()) - set(cand.tolist())
        assert not missed, f"robot {b} misses {sorted(missed)}"
        n_cand.append(len(cand))
    assert want.any() and np.mean(n_cand) < c.B / 4
    assert sorted(grid.cell_mem.tolist()) == list(range(c.B))


# ---- the ensemble's tree and rule ----
@pytest.mark.parametrize("n", [1100, 2049])
def test_tree_equals_its_literal_rule_beyond_four_strides(n):
    """n = 1100: five strides, the fifth of 76 slots; n = 2049: nine, the ninth of one slot."""
    v = tree_values(n)
    assert -(-n // 256) >= 5
    assert bits(ensemble_sum(v)) == bits(literal_sum(v))
    cols = np.stack([v, -v, v * 3.0], axis=1)
    assert [bits(x) for x in ensemble_sum(cols)] == [bits(literal_sum(cols[:, k])) for k in range(3)]


ENSEMBLES = {"two-of-550-and-an-empty": lambda B: Ensemble(np.arange(B) % 2, groups=3), "one-of-1100": lambda B: Ensemble()}


def ensemble_case(which):
    """1100 robots under the plant of all channels, so that the members differ."""
    cfg, fleet = big_fleet(1100)
    return case(cfg, fleet, CHEAP, plant=plant_of("all"), ensemble=ENSEMBLES[which](1100))


def reach_ensemble(which, st):
    """``st``: the records so far [steps, G]"""
    if which == "one-of-1100":
        assert st.shape[1] == 1 and (st["n"] == 1100).all() and 1100 > 4 * 256
    else:
        assert st.shape[1] == 3 and (st["n"] == [550, 550, 0]).all() and (st["far_robot"][:, 2] == -1).all()
        assert (st["far_robot"][:, :2] % 2 == np.arange(2)).all()
    members = st["n"] > 0
    assert (st["cov"][members][:, [0, 2, 3]] > 0).all()


@pytest.mark.parametrize("which", list(ENSEMBLES))
def test_large_groups_equal_the_literal_rule(which):
    c = ensemble_case(which)
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    g, G = c.kw["ensemble"].checked(c.B)
    for k in range(c.steps):
        host.step(o.warm_solve(threads=8))
        bad = ensemble_differing(host.ensemble_stats()[-1], literal_stats(host, g, G))
        assert not bad, f"step {k}: {bad}"
    reach_ensemble(which, host.ensemble_stats())


# ---- the drive log ----
PROBE = 64                   # robots of the fleet driven beforehand to find who goes where
TIE_AT = 1                   # where the robot that exhausts its budget at every step is put; another one THREADS places behind it


def log_case(B):
    """The fleet of ``big_fleet`` without peers, the solves given 1000 inner iterations, three robots moved: one that converges at
    every step to place 0, one that exhausts the budget at every step to place ``TIE_AT`` and another such to ``TIE_AT + THREADS`` --
    the totals kernel's thread ``TIE_AT`` meets the same ``inner_max`` in its first and in its second stride, and robot 0 does not
    have it.  They are found by driving the fleet's first ``PROBE`` robots alone (the robots do not depend on each other)."""
    cfg, fleet = big_fleet(B)
    opts = {"max_total_inner": LOG_BUDGET}
    o = oracle_for(cfg, **opts)
    routes, route_of, starts, idx0 = fleet
    probe = FleetRecedingHorizon(routes, route_of[:PROBE], starts[:PROBE], None, sincos=o.sincos_array, idx0=idx0[:PROBE])
    inner = np.stack([probe.step(o.warm_solve(threads=8))[1]["num_inner_iterations"] for _ in range(STEPS)])
    spent, never = np.nonzero((inner == LOG_BUDGET).all(axis=0))[0], np.nonzero((inner < LOG_BUDGET).all(axis=0))[0]
    assert len(spent) >= 2 and len(never) >= 1, "the probe holds no robot that converges at every step, or fewer than two that never do"
    fleet = placed_fleet(*fleet, {0: int(never[0]), TIE_AT: int(spent[0]), TIE_AT + THREADS: int(spent[1])})
    return case(cfg, fleet, opts, steps=STEPS if B <= 1100 else 2, log=DriveLog())      # (2100 robots: two steps, a step's oracle takes seconds)


def literal_totals(st, drove):
    """A step's totals robot by robot: a strictly larger count is the only way to take the record over."""
    solved, exits, inner_max, who, total = 0, [0] * 5, 0, 0, 0
    for b in range(len(drove)):
        if not drove[b]:
            continue
        e, inner = int(st["exit_status"][b]), int(st["num_inner_iterations"][b])
        if solved == 0 or inner > inner_max:
            inner_max, who = inner, b
        solved += 1
        exits[e] += 1
        total += inner
    return solved, exits, inner_max, who, total


def totals_differing(tot, st, drove):
    """The last record of ``tot`` against ``literal_totals``: the names that differ"""
    solved, exits, inner_max, who, total = literal_totals(st, drove)
    t = tot[-1]
    pairs = (("solved", solved), ("inner_max", inner_max), ("inner_max_robot", who), ("inner_total", total))
    return [n for n, v in pairs if int(t[n]) != v] + (["exits"] if t["exits"].tolist() != exits else [])


def reach_log(host):
    """The step just taken, on a fleet nobody retires from: see ``log_case``."""
    tot, rec = host.step_totals[-1], host.step_records[-1]
    assert tot["solved"] == host.B and host.B > THREADS
    assert (tot["exits"] > 0).sum() >= 2, f"exits {tot['exits'].tolist()}: one exit status only"
    top = np.nonzero(rec["num_inner_iterations"] == tot["inner_max"])[0]
    assert len(top) >= 2 and top[0] == tot["inner_max_robot"] and top[0] != 0, top[:4]
    assert (top >= top[0] + THREADS).any() and top[0] + THREADS in top, "no second candidate in the same thread's later stride"


@pytest.mark.parametrize("B", [1100, 2100])
def test_log_fleet_ties_its_inner_max_across_strides_and_totals_equal_the_literal_loop(B):
    c = log_case(B)
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    for k in range(c.steps):
        _, st = host.step(o.warm_solve(threads=8))
        bad = totals_differing(host.step_totals, st, np.ones(B, dtype=bool))
        assert not bad, f"step {k}: {bad}"
        reach_log(host)
    tot = host.step_totals
    print(f"B = {B}: exits per step {tot['exits'].tolist()}, inner_max {tot['inner_max'].tolist()} at {tot['inner_max_robot'].tolist()}")
    assert (tot["exits"].sum(axis=0)[[0, 2]] > 0).all() and (B > 1100 or tot["exits"][:, 1].sum() > 0)      # three steps: all of 0, 1, 2


# ---- a retiring fleet with log, plant and ensemble ----
RETIRING_STEPS = 4
RETIRING_GROUPS = np.arange(1100) % 3 % 2      # 733 and 367 interleaved members (b % 2 would put every copy of the robots that start
                                               # two samples before their goals, b % 16 in 0, 4, 8, 12, into group 0), and an empty group


def retiring_case():
    """The staggered fleet tiled to 1100 under the plant of all channels: robot b draws the disturbances of id b, so the copies of a
    robot part and retire at different steps -- from the first step on some are retired and over a thousand are not."""
    cfg = named_config("cfg1")
    fleet = tiled_fleet(*staggered_fleet(cfg), 1100 / 16)
    return case(cfg, fleet, {"max_total_inner": LOG_BUDGET}, steps=RETIRING_STEPS, retire=True, log=DriveLog(), plant=plant_of("all"),
                ensemble=Ensemble(RETIRING_GROUPS, groups=3))


def reach_retiring(host, drove):
    """The step just taken, ``drove`` = the active robots as it found them."""
    n, B = int(drove.sum()), host.B
    if host.steps > 1:
        assert 2 * 256 < n < B, f"{n} robots driven: not some retired among more than two workgroups of active ones"
        assert mixed_chunks(drove) > 0
    rec, ctrl, s = host.step_records[-1], host.controls[-host.cfg.num_steps_taken:], host.cfg.num_steps_taken
    assert (rec["exit_status"][~drove] == -1).all() and (rec["exit_status"][drove] >= 0).all()
    assert not ctrl[:, ~drove].any() and not np.signbit(ctrl[:, ~drove]).any() and len(ctrl) == s
    st = host.ensemble_stats()[-1]
    assert (st["n"] == [733, 367, 0]).all() and st["arrived"].sum() == (host.retired_at >= 0).sum()
    assert (0 < st["arrived"][:2]).all() and (st["arrived"][:2] < st["n"][:2]).all()


def test_retiring_fleet_keeps_retired_rows_and_counts_arrivals():
    c = retiring_case()
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    g, G = c.kw["ensemble"].checked(c.B)
    seen = []
    for k in range(c.steps):
        drove = host.active.copy()
        _, st = host.step(o.warm_solve(threads=8))
        reach_retiring(host, drove)
        assert not totals_differing(host.step_totals, st, drove), f"step {k}"
        assert not ensemble_differing(host.ensemble_stats()[-1], literal_stats(host, g, G)), f"step {k}"
        seen.append(int(drove.sum()))
    print("robots driven per step", seen, "exits", host.step_totals["exits"].tolist())
    assert len(set(seen)) >= 3, "fewer than two steps at which somebody retired"


# ---- the crowd ----
CROWDS = ["d16384", "d1000-n40"]


def crowd_case(which):
    """``d16384``: cfg4, eight robots and the most obstacles the setter takes, 256 per lane, three slots, a range that excludes nobody.
    ``d1000-n40``: the N = 40 configuration, 24 robots, 1000 obstacles (15 or 16 per lane), a range that leaves slots unfilled."""
    if which == "d16384":
        cfg = named_config("cfg4")
        fleet = frontend.random_fleet(cfg, 11, 3, 8, seed=41)
        obs, sinus = scattered(cfg, CROWD_MAX)
        return case(cfg, fleet, CHEAP, crowd=Crowd(obs, 3, 1e3, sinus=sinus, watch=True))
    cfg = named_config("cfg2")
    fleet = frontend.random_fleet(cfg, 11, 3, 24, seed=41)
    obs, sinus = scattered(cfg, 1000)
    r = 1.5 * narrow_range(lambda r: FleetRecedingHorizon(*fleet[:3], None, idx0=fleet[3], crowd=Crowd(obs, 3, r, sinus=sinus)))
    return case(cfg, fleet, CHEAP, crowd=Crowd(obs, 3, r, sinus=sinus, watch=True))


def reach_crowd(which, seen, host):
    """``seen``: the chosen obstacles of every step [steps, B, M]"""
    seen = np.asarray(seen)
    if which == "d16384":
        assert len(host.crowd_table()) == CROWD_MAX == 256 * 64
        assert filled(seen).all() and (seen >= CROWD_MAX // 2).any(), "no chosen obstacle from the upper half of the table"
    else:
        assert host.cfg.N_hor == 40 and len(host.crowd_table()) == 1000
        assert filled(seen).any() and not filled(seen).all(), "the range must leave filled and unfilled slots"
        assert (seen >= 64).any()
    rec = host.crowd_clearance()
    assert (rec["obstacle"] >= 64).any() and (rec["row"] >= 1).all()


@pytest.mark.parametrize("which", CROWDS)
def test_crowd_fleets_reach_deep_into_a_lanes_list(which):
    c = crowd_case(which)
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    seen = []
    for k in range(c.steps):
        host.step(o.warm_solve(threads=8))
        seen.append(host.crowd_seen.copy())
    reach_crowd(which, seen, host)
    print(which, "largest chosen index", int(np.max(seen)), "observer's obstacles", host.crowd_clearance()["obstacle"].tolist()[:8])


def test_the_most_obstacles_are_taken_and_one_more_is_not():
    obs, sinus = scattered(named_config("cfg4"), 8)
    most = tuple(np.resize(a, (CROWD_MAX,) + a.shape[1:]) for a in obs)
    Crowd(most, 1, 5.0).checked(8, 0, 3)
    with pytest.raises(ValueError):
        Crowd(tuple(np.resize(a, (CROWD_MAX + 1,) + a.shape[1:]) for a in obs), 1, 5.0).checked(8, 0, 3)


# ---- everything at once ----
NEAR_GOAL = (1, 1, 2, 2, 3, 3)


def everything_case():
    """cfg4, 1100 robots, one scripted ellipse each; a measuring plant, a watched crowd of 200 (one slot), grid peers (one slot, one
    group of everybody), three wall slots on the 104-edge map, retirement, both monitors (the clearance monitor over one group of
    1100: its mirror takes tenths of a second), the log and the ensemble."""
    cfg, (routes, route_of, starts, idx0) = big_fleet(1100, "cfg4")
    starts, idx0 = move_near_goal(routes, route_of, starts, idx0, NEAR_GOAL)
    dyn = fleet_ellipses(routes, route_of, idx0, 1, 9)
    obs, sinus = scattered(cfg, 200)
    return case(cfg, (routes, route_of, starts, idx0), CHEAP, dyn=dyn, plant=plant_of("all"),
                crowd=Crowd(obs, 1, 3.0, sinus=sinus, watch=True),
                peers=Peers(slots=1, rx=RX, ry=RY, range=second_neighbour_range(starts), cell=1.0),
                walls=walls_of(cfg, pieces=4, spacing=1.0), retire=True, monitor=Monitor(), map_monitor=MapMonitor(*scene_map(cfg, 4)),
                log=DriveLog(), ensemble=Ensemble(np.arange(1100) % 2, groups=3))


def reach_everything(host, seen):
    """After the last step; ``seen`` = per step (crowd slots filled [B], peer slots filled [B], wall slots filled [B])."""
    crowd, peer, wall = (np.stack(x) for x in zip(*seen))
    assert len(host._wall_edges) == 104 and host.K == 1 and host.B == 1100
    for what, got in (("crowd", crowd), ("peer", peer), ("wall", wall)):
        assert got.any() and not got.all(), f"the {what} slots are all filled or all empty"
    assert (host.grid.nx * host.grid.ny + 1) > 2 * THREADS and host.grid.filed == host.B
    assert not np.array_equal(host.measured(), host.state)
    rec = host.clearance
    assert np.isfinite(rec["circle"]).all() and np.isfinite(rec["ellipse"]).all() and (rec["peer"] >= 0).all()
    assert np.isfinite(host.map_clearance["wall2"]).all() and (host.crowd_clearance()["obstacle"] >= 0).all()
    assert (host.step_totals["solved"] > 2 * 256).all() and host.step_totals["solved"][-1] < host.B, "nobody retired before the last step"
    st = host.ensemble_stats()
    assert (st["n"] == [550, 550, 0]).all()


def everything_step(host, solve):
    host.step(solve)
    return (host.crowd_seen[:, 0] >= 0, host.peer_index[:, 0] >= 0, (host.wall_edge >= 0).any(axis=1))


def test_everything_at_once_fills_some_slots_of_every_kind():
    c = everything_case()
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    seen = [everything_step(host, o.warm_solve(threads=8)) for _ in range(c.steps)]
    reach_everything(host, seen)
    print("active after the steps", host.n_active, "retired at", host.retired_at[host.retired_at >= 0].tolist(),
          "grid", host.grid.nx, host.grid.ny, "filled (crowd, peer, wall)", [int(np.stack(x).sum()) for x in zip(*seen)])


def test_placed_fleet_swaps_robots_into_place():
    cfg, fleet = big_fleet(12)
    routes, route_of, starts, idx0 = placed_fleet(*fleet, {0: 5, 1: 0, 7: 1})
    order = [5, 0, 2, 3, 4, 1, 6, 7, 8, 9, 10, 11]
    order[7], order[5] = 1, 7                                  # robot 1 stood at place 5 after the first swap
    assert np.array_equal(starts, fleet[2][order]) and np.array_equal(route_of, fleet[1][order]) and np.array_equal(idx0, fleet[3][order])
    assert routes == list(fleet[0]) and sorted(order) == list(range(12))
