"""CPU: the host mirrors of the on-device loop at the shapes tests/test_gpu_loop_shapes.py drives the kernels at -- several steps taken
per solve (3, 5, 11, 20 of N_hor = 20, 7 of 33), routes of five samples and of one, braking tables of 8 and 45 entries, 150 vertices
with duplicates, no vertices, no obstacle slots, a peers group larger than three candidates per lane, a NaN pose -- and at the three sets of
vehicle constants of tests/vehicle_sets.py (``fast-``, ``slow-``, ``fwd-``): another ts, base speed, circle radius, ellipse padding and
braking tables of 5 and 27 entries.

The device tests compare against ``VectorizedRecedingHorizon`` / ``FleetRecedingHorizon``; here those are held, bit for bit, to
``BatchedRecedingHorizon``, whose robots run the one literal per-robot step that tests/test_harness.py ties to the reference's recorded
goldens (the oracle with cheap caps solves: the assembly is what is tested), and the peers to the literal rule of
tests/test_peers_mirror.py.  Every case also asserts, on the mirror alone, that the edge it is there for was reached (``REACH``):
that is what makes the device comparison of the same case run the kernel lines named in the GPU module.

``CASES`` and ``REACH`` are shared with the GPU module, so both run exactly the same fleets."""
import types

import numpy as np
import pytest

from conftest import oracle_for
from mpc_trajectory_generator_amd import frontend, harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.trajectory import BatchedRecedingHorizon, FleetRecedingHorizon, Peers, VectorizedRecedingHorizon
from mpc_trajectory_generator_amd.workloads import fleet_ellipses, handmade_route, route_fleet, staggered_fleet, stale_idx0, tiled_fleet
from test_peers_mirror import _run as run_peers_against_literal_rule
from vehicle_sets import VEHICLE_SETS, vehicle_config

RX, RY = 0.37, 0.53          # radii no scripted or padding ellipse has (tests/test_gpu_peers_loop.py)


def _standing(route, i0, seed, off=0.05):
    """-> starts [B, 3]: on the samples ``i0`` of the route, off them by up to ``off`` m per axis (and 0.1 rad)."""
    rng = np.random.default_rng(seed)
    ref = np.stack([route.x_ref, route.y_ref, route.theta_ref], axis=1)[np.asarray(i0)]
    return ref + np.stack([rng.uniform(-off, off, len(i0)), rng.uniform(-off, off, len(i0)), rng.uniform(-0.1, 0.1, len(i0))], axis=1)


def _case(cfg, route, starts, idx0, K=0, sinus=False, steps=4, reach=None, seed=3, until_done=False):
    idx0 = np.asarray(idx0, dtype=np.int32)
    dyn = fleet_ellipses([route], np.zeros(len(idx0), dtype=np.int32), idx0, K, seed)
    return types.SimpleNamespace(cfg=cfg, route=route, starts=np.asarray(starts, dtype=np.float64), idx0=idx0, K=K, dyn=dyn,
                                 sinus=sinus, steps=steps, reach=reach, until_done=until_done)


# ---- steps taken per solve ----
def _steps_taken(s, K=2, sinus=False, steps=4, **shape):
    cfg = load_config(num_steps_taken=s, **shape)
    route = harness.scene_route(cfg, 11)
    i0, starts, _ = route_fleet(route, 12, 20 + s)
    return _case(cfg, route, starts, i0, K, sinus, steps)


def _stale():
    """s = 11: the window is 66 samples wide.  Every robot's search starts 54 samples behind where it stands, so the closest sample
    lies at window offset 54 + 11 = 65 (a robot standing on sample 100 with idx0 = 46: the window is [35, 101))."""
    cfg = load_config(num_steps_taken=11)
    route = harness.scene_route(cfg, 11)
    assert len(route.x_ref) == 216
    i0 = np.array([100, 60, 54, 30, 0, 150, 180, 200, 120, 75, 90, 210])
    c = _case(cfg, route, _standing(route, i0, 4), stale_idx0(i0, 54), K=2, steps=3, reach="stale")
    assert c.idx0[0] == 46
    return c


# ---- route tables ----
def _short(waypoints, n_ref, i0, vertices=()):
    cfg = named_config("cfg1")
    route = handmade_route(cfg, waypoints, vertices)
    assert len(route.x_ref) == n_ref
    i0 = np.asarray(i0)
    starts = _standing(route, i0, 6, off=0.3)
    starts[0] = [route.x_ref[i0[0]], route.y_ref[i0[0]], route.theta_ref[i0[0]]]          # one robot on the route itself
    return _case(cfg, route, starts, i0, steps=5, reach="short")


def _braking(vel_red_steps):
    """Scene 1, robots 2, 5, 12 and 40 samples before the end, on the route and up to 0.3 m off it."""
    cfg = load_config(vel_red_steps=vel_red_steps)
    route = harness.scene_route(cfg, 1)
    i0 = len(route.x_ref) - np.array([2, 5, 12, 40, 2, 5, 12, 40])
    starts = _standing(route, i0, 8, off=0.3)
    starts[:4] = np.stack([route.x_ref, route.y_ref, route.theta_ref], axis=1)[i0[:4]]
    return _case(cfg, route, starts, i0, steps=8, reach=f"brake{vel_red_steps}", until_done=True)


def _many_vertices(Nobs):
    """Scene 11's waypoints with 150 circle centres: 80 beside the route, about 0.9 m off every third sample from its start on, then
    the first 70 of them once more -- vertex j < 70 has an exact duplicate 80 positions later."""
    cfg = load_config(Nobs=Nobs)
    plain = harness.scene_route(cfg, 11)
    rng = np.random.default_rng(12)
    at = np.minimum(len(plain.x_ref) - 1, 3 * np.arange(80))
    pts = np.stack([np.array(plain.x_ref)[at] + 0.9 + rng.uniform(-0.1, 0.1, 80), np.array(plain.y_ref)[at] + rng.uniform(-0.1, 0.1, 80)], axis=1)
    vertices = np.concatenate([pts, pts[:70]])
    route = handmade_route(cfg, harness.SCENES[11]["waypoints"], vertices)
    assert len(route.vertices) == 150 and route.x_ref == plain.x_ref
    i0 = np.array([0, 3, 8, 14, 20, 25, 40, 80, 120, 150, 170, 185])
    return _case(cfg, route, _standing(route, i0, 9), i0, K=1, steps=3, reach="dupvert")


def _scene1(waypoints_only=False, **shape):
    cfg = load_config(**shape)
    route = handmade_route(cfg, harness.SCENES[1]["waypoints"]) if waypoints_only else harness.scene_route(cfg, 1)
    i0, starts, _ = route_fleet(route, 12, 15)
    return _case(cfg, route, starts, i0, K=min(1, cfg.Ndynobs), steps=3)


def _nan_pose():
    """One robot of 12 with a NaN x; Nobs = 3 against scene 11's six vertices, so that both arg-min searches see it."""
    cfg = load_config(Nobs=3)
    route = harness.scene_route(cfg, 11)
    i0, starts, _ = route_fleet(route, 12, 19)
    starts[NAN_ROBOT, 0] = np.nan
    assert i0[NAN_ROBOT] > 1
    return _case(cfg, route, starts, i0, steps=3)


# ---- vehicle constants other than the default (tests/vehicle_sets.py) ----
def _set_steps_taken(name, scene, s, K, sinus=False, steps=4):
    cfg = vehicle_config(name, num_steps_taken=s)
    route = harness.scene_route(cfg, scene)
    i0, starts, _ = route_fleet(route, 12, 20 + s)
    return _case(cfg, route, starts, i0, K, sinus, steps)


def _set_braking(name):
    """``_braking`` at a set's constants, for a fixed number of steps."""
    cfg = vehicle_config(name)
    route = harness.scene_route(cfg, 1)
    i0 = len(route.x_ref) - np.array([2, 5, 12, 40, 2, 5, 12, 40])
    starts = _standing(route, i0, 8, off=0.3)
    starts[:4] = np.stack([route.x_ref, route.y_ref, route.theta_ref], axis=1)[i0[:4]]
    return _case(cfg, route, starts, i0, steps=8, reach=f"{name}-brake", until_done=False)


NAN_ROBOT = 5

CASES = {
    "s3": lambda: _steps_taken(3),
    "s11-stale": _stale,
    "s20": lambda: _steps_taken(20, steps=3),
    "n33-s7": lambda: _steps_taken(7, steps=3, N_hor=33),
    "s5-sinus": lambda: _steps_taken(5, K=3, sinus=True),
    "route5": lambda: _short([(2.0, 2.0), (3.5, 2.0)], 5, [0, 1, 2, 3, 4, 0, 2, 4], vertices=[(2.7, 3.0)]),
    "route1": lambda: _short([(2.0, 2.0), (2.2, 2.0)], 1, [0] * 6),
    "brake7": lambda: _braking(7),
    "brake45": lambda: _braking(45),
    "verts150-nobs10": lambda: _many_vertices(10),
    "verts150-nobs64": lambda: _many_vertices(64),
    "no-vertices": lambda: _scene1(waypoints_only=True),
    "nobs0-ndyn0": lambda: _scene1(Nobs=0, Ndynobs=0),
    "fast-s1": lambda: _set_steps_taken("fast", 11, 1, K=2),
    "slow-s3-sinus": lambda: _set_steps_taken("slow", 11, 3, K=3, sinus=True),
    "fwd-s2": lambda: _set_steps_taken("fwd", 1, 2, K=1),
    "slow-brake5": lambda: _set_braking("slow"),
    "fwd-brake27": lambda: _set_braking("fwd"),
}


# ---- what a case must have reached, on the mirror: trace = per step (state before, idx before, idx after) ----
def _reach_stale(c, trace):
    s = c.cfg.num_steps_taken
    off = max(int((idx - np.maximum(0, before - s)).max()) for _, before, idx in trace)
    assert off >= 64, f"largest window offset {off}: no lane took a second sample of the window"
    assert int((trace[0][2] - np.maximum(0, trace[0][1] - s))[0]) == 65            # the robot on sample 100, started at 46


def _reach_dupvert(c, trace):
    vert = np.array(c.route.vertices)
    hit = 0
    for state, _, _ in trace:
        for b in range(len(state)):
            lb = harness.closest_index(state[b, :2], vert)                           # the literal rule: the first minimum
            twins = np.nonzero((vert == vert[lb]).all(axis=1))[0]
            assert lb == twins[0], "the literal rule chose a higher duplicate"
            hit += bool(lb < c.cfg.Nobs and twins[-1] >= lb + 64)                    # (lb < Nobs: the window [lb, Nobs) shows it in p)
    assert hit, "no robot's closest vertex is one with a duplicate 64 or more positions later and inside the circle slots"


def _reach_short(c, trace):
    N, n = c.cfg.N_hor, len(c.route.x_ref)
    assert n < N and all((idx + N >= n).all() for _, _, idx in trace)
    assert any((n - idx - 1 == 0).any() for _, _, idx in trace), "nbase == 0 never taken"


def _reach_brake(n_brake):
    def reach(c, trace):
        r, N, n = c.route, c.cfg.N_hor, len(c.route.x_ref)
        assert len(r.brake_velocities) == len(r.brake_distances) == n_brake
        nbase = np.stack([np.minimum(n - idx - 1, N) for _, _, idx in trace])
        braking = np.stack([(idx + N) >= n - r.brake_distances[0] / r.base_speed for _, _, idx in trace])
        assert (braking & (nbase == 0)).any(), "nobody inside the last sample: the table filter never ran"
        assert (braking & (nbase > 0) & (nbase < N)).any(), "no horizon with base speeds followed by the table"
        if n_brake < N:
            assert (braking & (nbase > 0) & (N - nbase > n_brake)).any(), "no horizon reaches past the table's end"
    return reach


def _reach_set_brake(n_brake):
    """The table length the route reports, and a horizon that holds base speeds followed by entries of the table."""
    def reach(c, trace):
        r, N, n = c.route, c.cfg.N_hor, len(c.route.x_ref)
        assert len(r.brake_velocities) == len(r.brake_distances) == n_brake
        assert r.base_speed == c.cfg.lin_vel_max * c.cfg.throttle_ratio and r.radius == c.cfg.vehicle_width / 2 + c.cfg.vehicle_margin
        nbase = np.stack([np.minimum(n - idx - 1, N) for _, _, idx in trace])
        braking = np.stack([(idx + N) >= n - r.brake_distances[0] / r.base_speed for _, _, idx in trace])
        assert (braking & (nbase > 0) & (nbase < N)).any(), "no horizon with base speeds followed by the table"
        if n_brake < N:
            assert (braking & (nbase > 0) & (N - nbase > n_brake)).any(), "no horizon reaches past the table's end"
        else:
            assert (braking & (nbase > 0) & (N - nbase < n_brake)).any(), "no horizon that the table outlasts"
    return reach


REACH = {"slow-brake": _reach_set_brake(5), "fwd-brake": _reach_set_brake(27), "stale": _reach_stale, "dupvert": _reach_dupvert, "short": _reach_short, "brake7": _reach_brake(8), "brake45": _reach_brake(45)}


def traced_step(host, solve, trace):
    """One step of a single-route mirror, recorded for the REACH checks."""
    state, before = host.state.copy(), np.array(host.idx).copy()
    out = host.step(solve)
    trace.append((state, before, np.array(host.idx).copy()))
    return out


def _lists(dyn, B):
    """The six arrays of ``dyn`` as the per-robot obstacle lists ``BatchedRecedingHorizon`` takes."""
    if dyn is None:
        return [[] for _ in range(B)]
    p1, p2, freq, rx, ry, ang = dyn
    return [[[list(p1[b, k]), list(p2[b, k]), freq[b, k], rx[b, k], ry[b, k], ang[b, k]] for k in range(p1.shape[1])] for b in range(B)]


def _mirror_against_loop(c, nan_robot=None):
    o = oracle_for(c.cfg, max_inner=40, max_outer=2)               # cheap solves: the assembly is what is tested
    B = len(c.starts)
    loop = BatchedRecedingHorizon(c.route, c.starts, _lists(c.dyn, B), sinus_object=c.sinus, idx0=c.idx0)
    vec = VectorizedRecedingHorizon(c.route, c.starts, c.dyn, sinus_object=c.sinus, idx0=c.idx0)
    solve, trace = o.warm_solve(threads=4), []
    for k in range(c.steps):
        Pl, _ = loop.step(solve)
        Pv, _ = traced_step(vec, solve, trace)
        assert np.array_equal(Pl, Pv, equal_nan=nan_robot is not None), (k, np.argwhere(Pl != Pv)[:5])
        assert np.array_equal(vec.idx, loop.idx), k
        if nan_robot is not None:
            assert np.isnan(Pv[nan_robot, 0]) and not np.isnan(np.delete(Pv, nan_robot, axis=0)).any()
        assert np.array_equal(vec.state, np.array([s[-3:] for s in loop.states]), equal_nan=nan_robot is not None), k
    return vec, trace


@pytest.mark.parametrize("which", list(CASES))
def test_mirror_equals_the_per_robot_loop(which):
    c = CASES[which]()
    _, trace = _mirror_against_loop(c)
    if c.reach:
        REACH[c.reach](c, trace)


def test_shapes_are_the_ones_asked_for():
    """What each case is there for, read off its configuration and route."""
    c = {k: f() for k, f in CASES.items()}
    assert [c[k].cfg.num_steps_taken for k in ("s3", "s11-stale", "s20", "n33-s7", "s5-sinus")] == [3, 11, 20, 7, 5]
    assert c["n33-s7"].cfg.N_hor == 33 and c["s20"].cfg.N_hor == 20 and c["s5-sinus"].sinus and c["s5-sinus"].K == 3
    assert all(c[k].K == 2 for k in ("s3", "s11-stale", "s20", "n33-s7"))
    assert len(c["route5"].route.x_ref) == 5 and len(c["route1"].route.x_ref) == 1
    for k in ("route5", "route1"):
        d = np.hypot(c[k].starts[:, 0] - np.array(c[k].route.x_ref)[c[k].idx0], c[k].starts[:, 1] - np.array(c[k].route.y_ref)[c[k].idx0])
        assert d[0] == 0 and 0.05 < d.max() <= 0.3 * np.sqrt(2)
    assert len(c["brake7"].route.brake_velocities) == 8 and len(c["brake45"].route.brake_velocities) == 45
    assert len(c["verts150-nobs10"].route.vertices) == 150 and c["verts150-nobs64"].cfg.Nobs == 64
    assert len(c["no-vertices"].route.vertices) == 0 and c["no-vertices"].cfg.Nobs == 10
    assert (c["nobs0-ndyn0"].cfg.Nobs, c["nobs0-ndyn0"].cfg.Ndynobs, len(c["nobs0-ndyn0"].route.vertices)) == (0, 0, 3)
    assert all(len(v.starts) <= 32 and 3 <= v.steps <= 8 for v in c.values())
    sets = {"fast-s1": ("fast", 1, 2, False), "slow-s3-sinus": ("slow", 3, 3, True), "fwd-s2": ("fwd", 2, 1, False),
            "slow-brake5": ("slow", 1, 0, False), "fwd-brake27": ("fwd", 1, 0, False)}
    for k, (name, s, K, sinus) in sets.items():
        assert all(c[k].cfg[key] == v for key, v in VEHICLE_SETS[name].items()), k
        assert (c[k].cfg.num_steps_taken, c[k].K, c[k].sinus) == (s, K, sinus) and len(c[k].starts) <= 12 and 3 <= c[k].steps <= 8, k
        assert c[k].route.base_speed == c[k].cfg.lin_vel_max * c[k].cfg.throttle_ratio
    assert [c[k].cfg.ts for k in sets] == [0.1, 0.35, 0.05, 0.35, 0.05]
    assert c["fwd-s2"].route.radius == 0.55 and c["fast-s1"].route.radius == c["slow-s3-sinus"].route.radius == 0.5
    assert len(c["slow-brake5"].route.brake_velocities) == 5 and len(c["fwd-brake27"].route.brake_velocities) == 27
    assert len(c["fast-s1"].route.brake_velocities) == 20 and not c["slow-brake5"].until_done and c["slow-brake5"].steps == 8


def test_nan_pose_mirror_picks_the_first_sample_like_the_per_robot_loop():
    c = _nan_pose()
    vec, trace = _mirror_against_loop(c, nan_robot=NAN_ROBOT)
    s = c.cfg.num_steps_taken
    for _, before, idx in trace:
        assert idx[NAN_ROBOT] == max(0, before[NAN_ROBOT] - s)      # np.argmin over NaNs: the window's first sample
    assert trace[0][2][NAN_ROBOT] > 0 and not vec.done[NAN_ROBOT]


# ---- peers ----
def large_group_fleet():
    """-> (cfg, routes, route_of, starts, idx0, peers): 300 robots on four planned routes of scene 11, one group of 272 and one of 28,
    three slots, a range that excludes nobody: a lane of the 272 sees 4 or 5 members, its list keeps 3."""
    cfg = named_config("cfg1")
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 4, 300, seed=47)
    group_of = np.where(np.arange(300) % 75 < 68, 5, 9).astype(np.int32)
    assert (group_of == 5).sum() == 272 and (group_of == 9).sum() == 28
    return cfg, routes, route_of, starts, i0, Peers(slots=3, rx=RX, ry=RY, range=1e3, group_of=group_of)


def reach_overflow(host):
    """Some robot's chosen peer sits at position 192 or later of its group's member list, in another lane's stride than the robot
    itself: that lane had met three candidates before it, so its list of three was full and the chosen one displaced an entry."""
    g = np.asarray(host.peers.group_of)
    pos = np.empty(host.B, dtype=np.int64)                          # position inside the own group's member list (ascending index)
    for v in np.unique(g):
        mem = np.nonzero(g == v)[0]
        pos[mem] = np.arange(len(mem))
    chosen = host.peer_index
    ok = chosen >= 0
    p = np.where(ok, pos[np.where(ok, chosen, 0)], -1)
    assert (ok & (p >= 192) & (p % 64 != pos[:, None] % 64)).any(), "no chosen peer had to displace an entry of a full lane list"


def test_large_group_mirror_chooses_by_distance_then_index():
    """The mirror's choice among 271 candidates against the rule written out per robot on the mirror's own predictions (which
    tests/test_peers_mirror.py holds to the literal Euler steps): the first three in (D, j) order."""
    cfg, routes, route_of, starts, i0, peers = large_group_fleet()
    o = oracle_for(cfg, max_inner=40, max_outer=2)
    host = FleetRecedingHorizon(routes, route_of, starts, None, sincos=o.sincos_array, idx0=i0, peers=peers)
    g = peers.group_of
    for k in range(2):
        pred = host.predict()
        host.step(o.warm_solve(threads=4))
        for b in range(host.B):
            cand = []
            for j in np.nonzero(g == g[b])[0]:
                if j != b:
                    d = (pred[b, :, 0] - pred[j, :, 0]) * (pred[b, :, 0] - pred[j, :, 0]) + (pred[b, :, 1] - pred[j, :, 1]) * (pred[b, :, 1] - pred[j, :, 1])
                    cand.append((float(d.min()), int(j)))
            assert host.peer_index[b].tolist() == [j for _, j in sorted(cand)[:3]], (k, b)
        reach_overflow(host)


def peers_s3_fleet():
    """-> (cfg, routes, route_of, starts, idx0, K, peers): three steps taken per solve at N_hor = 20, so the shifted plan holds its last
    control for the last three stages of the prediction."""
    cfg = load_config(num_steps_taken=3)
    routes, route_of, starts, i0 = frontend.random_fleet(cfg, 11, 3, 24, seed=41)
    return cfg, routes, route_of, starts, i0, 1, Peers(slots=2, rx=RX, ry=RY, range=1e3, group_of=None)


def test_peers_mirror_at_three_steps_taken_equals_the_literal_rule():
    cfg, routes, route_of, starts, i0, K, peers = peers_s3_fleet()
    assert cfg.num_steps_taken == 3 and cfg.N_hor == 20
    chosen = run_peers_against_literal_rule(cfg, routes, route_of[:9], starts[:9], i0[:9], K, None, peers.slots, peers.range, 3)
    assert min(len(c) for step in chosen for c in step) == peers.slots


# ---- compaction beyond one robot per thread: what the tiling puts into a thread's chunk ----
def mixed_chunks(active, nt=1024):
    """-> how many threads of the compaction (thread t holds the robots [t * chunk, (t + 1) * chunk), chunk = ceil(B / nt)) hold
    active and retired robots side by side."""
    B = len(active)
    chunk = -(-B // nt)
    pad = np.concatenate([active.astype(int), np.full((-B) % chunk, -1)]).reshape(-1, chunk)
    return int((((pad == 1).any(axis=1)) & ((pad == 0).any(axis=1))).sum())


@pytest.mark.parametrize("B,chunk,threads,last", [(1025, 2, 513, 1), (2050, 3, 684, 1)])
def test_tiled_staggered_fleet_mixes_retired_and_active_in_a_chunk(B, chunk, threads, last):
    cfg = named_config("cfg1")
    base = staggered_fleet(cfg)
    routes, route_of, starts, i0 = tiled_fleet(*base, B / 16)
    assert len(starts) == B and -(-B // 1024) == chunk and -(-B // chunk) == threads and B - (threads - 1) * chunk == last
    rows = np.arange(B) % 16
    o = oracle_for(cfg)
    host = FleetRecedingHorizon(*base[:3], None, idx0=base[3], retire=True)
    seen = []
    while len(set(host.retired_at[host.retired_at >= 0].tolist())) < 2 and host.steps < 20:
        host.step(o.warm_solve())
        n = int(host.active[rows].sum())
        if 0 < n < B:
            seen.append(mixed_chunks(host.active[rows]))
    assert len(set(host.retired_at[host.retired_at >= 0].tolist())) >= 2
    assert seen and min(seen) > 0, "a step with retired robots had no thread holding both kinds"
    assert mixed_chunks(np.array([1, 1, 0, 0, 1, 0], dtype=bool), nt=3) == 1 and mixed_chunks(np.ones(5, dtype=bool), nt=2) == 0
