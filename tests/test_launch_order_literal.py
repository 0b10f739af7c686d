"""CPU: the fixtures of tests/test_gpu_launch_order.py, held to the literal rule of tests/launch_order_reference.py (DESIGN.md section
5.5) so that the GPU tests cannot pass without exercising anything.

* ``crafted(cfg)``: hand-made parameter vectors that reach every level 0..12, show each flag as alone as the rule lets it be (a graze
  is hard too, an early graze is a graze) and all six together, and sit on both sides of every comparison of the rule.  Each states
  what it claims (``want``), and the reference must agree here, on the CPU: a boundary case that slipped to the wrong side of its
  edge fails this file, it does not weaken the GPU one.
* the workload batches (``workload``, ``shape_workload``) spread over the levels, and nothing in them hinges on rounding: away from
  the thresholds the flags are the same in ``np.longdouble``.
* the rule is useful: on cfg1 the oracle's pass counts of the instances at level >= 8 exceed those at level 0.
* ``hint_case()`` / ``reach_hint``: the retiring fleet of the closed loop's hint and the conditions its checked steps must reach.
"""
import math

import numpy as np
import pytest

from conftest import oracle_for
from launch_order_reference import (FLAGS, LEVELS, NZ, flag_margins, level_from_inputs, level_from_passes, level_of, offsets,
                                    stable_partition)
from mpc_trajectory_generator_amd import named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.harness import synthetic_batch
from mpc_trajectory_generator_amd.workloads import staggered_fleet, tiled_fleet
from test_large_fleet_mirror import LOG_BUDGET, case, mirror_of
from test_plant_mirror import plant_of

SEED = 12345
WORKLOADS = {"cfg1": {}, "cfg2": {}, "cfg3": dict(synthetic_circles=True), "cfg4": dict(random_dyn=True)}
SHAPES = [(2, 0, 0), (5, 1, 3), (17, 4, 1), (33, 10, 3)]        # run-time shapes: (N, Nobs, Ndynobs)
AWAY = 1e-9                    # relative distance of a compared pair above which the number type must not matter


def workload(name, B):
    cfg = named_config(name)
    return cfg, synthetic_batch(cfg, 11, B, SEED, **WORKLOADS[name])


def shape_workload(shape, B):
    N, nobs, ndyn = shape
    cfg = load_config(N_hor=N, Nobs=nobs, Ndynobs=ndyn)
    return cfg, synthetic_batch(cfg, 11, B, SEED, random_dyn=ndyn > 0)


# ------------------------------------------------------------------------------------------------ crafted instances
SPACING = 8.0                  # m between reference samples: an obstacle placed at one sample is far from every other
FAR = -1000.0                  # where the ellipses nobody asked for stand


class Craft:
    """One hand-made parameter vector: the reference runs up the line x = ``xs``, sample t at y = 8 t, heading 0; the last applied
    speed and every reference speed are 0.5; every circle slot is empty (r = 0 at the origin: with xs = 0, ON sample 0); every
    ellipse is a 0.5 m disc far away.  Level 0 until something is put in."""

    def __init__(self, cfg, xs=0.0):
        self.cfg, self.N = cfg, cfg.N_hor
        _, self.c0, self.e0, self.r0 = offsets(cfg)
        p = np.zeros(cfg.n_p)
        p[3], p[4] = 0.5, 0.125
        p[10:20] = cfg.weights()
        p[NZ:NZ + self.N] = 0.5
        for k in range(cfg.Ndynobs):
            for t in range(self.N):
                p[self.e0 + (k * self.N + t) * 5:][:5] = (FAR, FAR, 0.5, 0.5, 0.0)
        for t in range(self.N):
            p[self.r0 + 3 * t:][:3] = (xs, SPACING * t, 0.0)
        self.p = p
        self.xs = xs

    def sample(self, t):
        return self.p[self.r0 + 3 * t], self.p[self.r0 + 3 * t + 1]

    def move(self, t, x, y):
        self.p[self.r0 + 3 * t:][:2] = (x, y)
        return self

    def heading(self, t, th):
        self.p[self.r0 + 3 * t + 2] = th
        return self

    def circle(self, cx, cy, r, k=None):
        """in slot k (the last one unless given)"""
        k = self.cfg.Nobs - 1 if k is None else k
        self.p[self.c0 + 3 * k:][:3] = (cx, cy, r)
        return self

    def ellipse(self, t, x, y, rx, ry, k=None):
        """obstacle k (the last one unless given) at stage t"""
        k = self.cfg.Ndynobs - 1 if k is None else k
        self.p[self.e0 + (k * self.N + t) * 5:][:5] = (x, y, rx, ry, 0.3)
        return self

    def speeds(self, first_ref, last_applied=0.5):
        self.p[NZ], self.p[3] = first_ref, last_applied
        return self

    def finish(self):
        self.p[0:3] = self.p[self.r0:self.r0 + 3]              # the robot stands on its first sample
        self.p[5:8] = self.p[self.r0 + 3 * (self.N - 1):][:3]
        return self.p


def _ladder(cfg):
    """name -> Craft for the levels the shape can reach, one ingredient more per step (see the module docstring)"""
    N, out = cfg.N_hor, {}

    def build(what):
        c = Craft(cfg)
        last = N - 1
        if "goal" in what:
            c.move(last, *c.sample(last - 1))
        x, y = c.sample(last)
        if "hard" in what:         # 0.5 m from the last sample, r = 0.25: inside 0.85, outside 0.3
            c.circle(x + 0.5, y, 0.25) if cfg.Nobs else c.ellipse(last, x + 0.5, y, 0.25, 0.25)
        if "graze" in what:        # on the last sample, r = 0.1: the samples 8 m away see nothing
            c.circle(x, y, 0.1) if cfg.Nobs else c.ellipse(last, x, y, 0.1, 0.1)
        if "early" in what:        # on sample 0
            c.circle(*c.sample(0), 0.1)
        if "bend" in what:
            c.heading(last, 0.1)
        if "gap" in what:
            c.speeds(2.0)
        return c

    steps = [()]
    tops = (["hard", "graze"] if cfg.Nobs or cfg.Ndynobs else []) + (["early"] if cfg.Nobs else [])
    for top in tops:
        steps += [(top,), (top, "bend"), (top, "bend", "gap"), (top, "bend", "gap", "goal")]
    if not tops:
        steps += [("bend",), ("bend", "gap"), ("bend", "gap", "goal")]
    steps += [("bend",), ("gap",), ("goal",)]
    for s in steps:
        want = {f: f in s for f in FLAGS}
        want["graze"] = want["graze"] or "early" in s
        want["hard"] = want["hard"] or want["graze"]
        out["ladder-" + ("+".join(s) or "nothing")] = (build(s), dict(want, level=level_of(want)))
    return out


def crafted(cfg):
    """-> [(name, p [n_p], want)]: ``want`` = the flags (and sometimes the level) the case claims; a flag it does not name is left to
    the rule.  What a shape has no room for (circles with Nobs = 0, ellipses with Ndynobs = 0) is left out."""
    N, last = cfg.N_hor, cfg.N_hor - 1
    cases = dict(_ladder(cfg))
    up, down = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    if cfg.Nobs:
        r = 0.25
        for what, by, flag in (("clearance", 0.6, "hard"), ("graze", 0.05, "graze")):
            lim = r + by               # the kernel's own sum; the sample stands at x = lim, the circle at x = 0 on the sample's y: dy = 0
            for side, xs, inside in (("on", lim, False), ("ulp-inside", down(lim), True), ("ulp-outside", up(lim), False)):
                c = Craft(cfg, xs)
                cases[f"circle-{what}-{side}"] = (c.circle(0.0, c.sample(last)[1], r), {flag: inside, "early": False})
        # a graze at the stages around the middle of the horizon: early is 2 t < N
        for t in sorted({t for t in ((N - 1) // 2, N // 2, (N + 1) // 2, N // 2 - 1) if 0 <= t < N}):
            c = Craft(cfg)
            cases[f"graze-at-stage-{t}-of-{N}"] = (c.circle(*c.sample(t), 0.1), {"graze": True, "early": 2 * t < N, "hard": True})
        # empty and negative slots on the path
        c = Craft(cfg)
        cases["circle-r-zero-on-the-path"] = (c.circle(*c.sample(0), 0.0), {"level": 0})
        c = Craft(cfg)
        cases["circle-r-negative-on-the-path"] = (c.circle(*c.sample(0), -1.0), {"level": 0})
        c = Craft(cfg)
        cases["circle-first-slot"] = (c.circle(*c.sample(0), 0.1, k=0), {"level": 9})
        c = Craft(cfg)
        cases["circle-at-infinity"] = (c.circle(math.inf, c.sample(0)[1], 0.25), {"level": 0})
    # headings
    for name, th, bent in (("plus-pi", math.pi, True), ("minus-pi", -math.pi, True), ("plus-almost-two-pi", 2 * math.pi - 1e-3, False),
                           ("minus-almost-two-pi", -(2 * math.pi - 1e-3), False), ("just-below-bend", down(0.05), False),
                           ("exactly-bend", 0.05, False), ("just-above-bend", up(0.05), True)):
        c = Craft(cfg)
        for t in range(1, N):              # one step, then straight on
            c.heading(t, th)
        cases[f"heading-{name}"] = (c, {"bend": bent, "level": int(bent)})
    if N >= 3:                             # there and back: two steps of 0.03 bend by 0.06
        cases["heading-two-small-steps"] = (Craft(cfg).heading(1, 0.03), {"bend": True})
    # speed gap
    for name, first, gap in (("exactly-one", 1.5, False), ("ulp-above-one", up(1.5), True), ("exactly-minus-one", -0.5, False),
                             ("ulp-below-minus-one", -0.5 - 2.0 ** -52, True)):       # (-1 - 2^-52: the next double below -1)
        cases[f"gap-{name}"] = (Craft(cfg).speeds(first), {"gap": gap, "level": int(gap)})
    # the goal
    c = Craft(cfg)
    for t in range(max(1, N - 3), N):
        c.move(t, *c.sample(t - 1))
    cases["goal-padded-tail"] = (c, {"goal": True, "level": 1})
    cases["goal-last-two-differ-in-y"] = (Craft(cfg), {"goal": False})
    c = Craft(cfg)
    cases["goal-last-two-differ-in-x"] = (c.move(last, c.xs + 1.0, c.sample(last - 1)[1]), {"goal": False})
    if cfg.Ndynobs:
        # rx >> ry (and ry >> rx): hard out to the larger radius + 0.6 = 3.6, graze within the smaller + 0.05 = 0.25
        for name, rx, ry in (("wide", 3.0, 0.2), ("tall", 0.2, 3.0)):
            for d, hard, graze in ((3.7, False, False), (3.5, True, False), (0.3, True, False), (0.2, True, True)):
                c = Craft(cfg)
                x, y = c.sample(last)
                cases[f"ellipse-{name}-at-{d}"] = (c.ellipse(last, x + d, y, rx, ry), {"hard": hard, "graze": graze, "early": False})
        c = Craft(cfg)
        cases["ellipse-on-sample-0-is-never-early"] = (c.ellipse(0, *c.sample(0), 0.5, 0.5, k=0), {"level": 5})
        c = Craft(cfg)
        cases["ellipse-of-another-stage"] = (c.ellipse(last, *c.sample(0), 0.5, 0.5), {"level": 0})
    # a NaN reference sample: every comparison with it is false
    c = Craft(cfg)
    cases["nan-sample"] = (c.move(min(1, last), math.nan, c.sample(min(1, last))[1]), {"hard": False, "graze": False, "bend": False, "gap": False})
    return [(name, c.finish().copy(), want) for name, (c, want) in cases.items()]


def with_crafted(cfg, P):
    """-> (P with its leading block overwritten by ``crafted(cfg)``, the names of the block)"""
    block = crafted(cfg)
    P = P.copy()
    assert len(block) < len(P) // 2
    P[:len(block)] = np.stack([p for _, p, _ in block])
    return P, [n for n, _, _ in block]


def levels_of(cfg, P):
    """the literal rule over a batch -> int [B]"""
    return np.array([level_from_inputs(cfg, p)[0] for p in P])


ALL_CONFIGS = [pytest.param(lambda n=n: named_config(n), id=n) for n in WORKLOADS] + \
              [pytest.param(lambda s=s: load_config(N_hor=s[0], Nobs=s[1], Ndynobs=s[2]), id="n%d-o%d-d%d" % s) for s in SHAPES]


@pytest.mark.parametrize("make", ALL_CONFIGS)
def test_crafted_cases_sit_where_they_claim(make):
    cfg = make()
    seen, names = set(), set()
    for name, p, want in crafted(cfg):
        level, flags = level_from_inputs(cfg, p)
        got = dict(flags, level=level)
        assert {k: got[k] for k in want} == want, (name, got)
        assert level == level_of(flags)
        seen.add(level)
        names.add(name)
    top = 12 if cfg.Nobs else 8 if cfg.Ndynobs else 3
    assert seen >= set(range(top + 1)), sorted(seen)
    if cfg.Nobs:
        assert len(seen) == LEVELS
        level, flags = level_from_inputs(cfg, dict((n, p) for n, p, _ in crafted(cfg))["ladder-early+bend+gap+goal"])
        assert level == 12 and all(flags.values())
    # each flag as alone as the rule lets it be
    by_name = {n: level_from_inputs(cfg, p)[1] for n, p, _ in crafted(cfg)}
    for alone in ("bend", "gap", "goal") + (("hard",) if cfg.Nobs or cfg.Ndynobs else ()):
        assert [f for f, v in by_name[f"ladder-{alone}"].items() if v] == [alone]
    if cfg.Nobs:
        assert {"circle-clearance-on", "circle-clearance-ulp-inside", "circle-graze-on", "circle-graze-ulp-inside"} <= names
        stages = [int(n.split("-")[3]) for n in names if n.startswith("graze-at-stage-")]
        assert {2 * t - cfg.N_hor for t in stages} >= ({-1, 1} if cfg.N_hor % 2 else {0})


def test_the_on_the_edge_circles_are_on_the_edge():
    """The clearance and graze boundary cases compare two equal doubles: d2 == lim^2 exactly, which strict < calls outside."""
    cfg = named_config("cfg1")
    _, c0, _, r0 = offsets(cfg)
    for name, p, _ in crafted(cfg):
        if name in ("circle-clearance-on", "circle-graze-on"):
            k, t = cfg.Nobs - 1, cfg.N_hor - 1
            dx, dy = p[r0 + 3 * t] - p[c0 + 3 * k], p[r0 + 3 * t + 1] - p[c0 + 3 * k + 1]
            lim = p[c0 + 3 * k + 2] + (0.6 if "clearance" in name else 0.05)
            assert dy == 0.0 and dx * dx + dy * dy == lim * lim


def test_stable_partition_is_the_stable_sort_by_falling_level():
    rng = np.random.default_rng(7)
    for B in (1, 2, 13, 1025, 5000):
        for levels in (rng.integers(0, LEVELS, B), np.zeros(B, dtype=int), np.arange(B) % LEVELS, np.sort(rng.integers(0, LEVELS, B))):
            levels = levels.tolist()
            assert stable_partition(levels) == sorted(range(B), key=lambda i: -levels[i])


def test_level_from_passes_is_the_top_bit():
    assert [level_from_passes(n) for n in (0, 1, 31, 32, 63, 64, 127, 128)] == [0, 0, 0, 1, 1, 2, 2, 3]
    for k in range(5, 32):
        assert level_from_passes(2 ** k) == min(k - 4, 12) and level_from_passes(2 ** k - 1) == min(max(k - 5, 0), 12)
        assert level_from_passes(16 << min(k - 4, 12)) == min(k - 4, 12)
    assert level_from_passes(2 ** 31 + 1) == level_from_passes(2 ** 32 - 1) == 12


# ------------------------------------------------------------------------------------------------ the workload batches
B_WORKLOAD = 512
_LEVELS = {}


def workload_levels(name):
    if name not in _LEVELS:
        cfg, P = workload(name, B_WORKLOAD)
        _LEVELS[name] = (cfg, P, levels_of(cfg, P))
    return _LEVELS[name]


@pytest.mark.parametrize("name,least", [("cfg1", 10), ("cfg2", 10), ("cfg4", 10), ("cfg3", 3)])
def test_workload_batches_spread_over_the_levels(name, least):
    _, _, levels = workload_levels(name)
    counts = np.bincount(levels, minlength=LEVELS)
    print(name, "instances per level", counts.tolist())
    assert (counts > 0).sum() >= least


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_flags_do_not_hinge_on_rounding(name):
    """Away from every threshold (each compared pair more than 1e-9 apart, relatively) np.longdouble gives the same flags; under 1 %
    of a workload batch is nearer than that, and the crafted boundary cases are, by design."""
    cfg, P, levels = workload_levels(name)
    near = 0
    for p, level in zip(P, levels):
        flags, margin = flag_margins(cfg, p)
        if margin > AWAY:
            assert level_of(flags) == level and flags == level_from_inputs(cfg, p)[1]
        else:
            near += 1
    assert near < 0.01 * len(P), near
    skipped = [n for n, p, _ in crafted(cfg) if flag_margins(cfg, p)[1] <= AWAY]
    assert any(n.endswith("-on") for n in skipped) and "gap-exactly-one" in skipped
    for n, p, _ in crafted(cfg):
        if n not in skipped:
            assert flag_margins(cfg, p)[0] == level_from_inputs(cfg, p)[1], n


def test_levels_predict_the_oracles_pass_counts():
    """Measured against the oracle, not the kernels: on cfg1 the instances the rule puts at level >= 8 take more evaluation passes
    (``reserved``) on average than those at level 0.  Only the ordering is asserted (DESIGN.md section 5.5 has the means)."""
    cfg, P, levels = workload_levels("cfg1")
    passes = oracle_for(cfg).solve_batch(P, threads=8)[2]["reserved"].astype(float)
    means = [passes[levels == k].mean() if (levels == k).any() else float("nan") for k in range(LEVELS)]
    print("mean passes per level", [round(m) if m == m else None for m in means], "correlation", np.corrcoef(levels, passes)[0, 1])
    assert (levels >= 8).any() and (levels == 0).any()
    assert passes[levels >= 8].mean() > passes[levels == 0].mean()


# ------------------------------------------------------------------------------------------------ the closed loop's hint
HINT_COPIES = 2208 / 16        # the staggered fleet of 16, tiled
HINT_STEPS = 4
HINT_WAVES = 1024              # resident waves with NMPC_WAVES_PER_CU=4 on the 256 CUs of an MI355X: what n has to stay above


def hint_case():
    """The retiring fleet of ``test_large_fleet_mirror.retiring_case`` without its observers, tiled to 2208 robots: under the plant of
    all channels the copies of a robot part and retire at different steps, from the first step on, all over the fleet -- so from the
    second step on the active rows are not the robots' indices."""
    cfg = named_config("cfg1")
    fleet = tiled_fleet(*staggered_fleet(cfg), HINT_COPIES)
    return case(cfg, fleet, {"max_total_inner": LOG_BUDGET}, steps=HINT_STEPS, retire=True, plant=plant_of("all"))


def reach_hint(act, levels, B):
    """One checked step k >= 1: ``act`` = the robots it drove, ascending; ``levels`` = their levels from the previous pass counts.
    -> whether the step shows what the test is there for (some retired robot below an active one, two levels or more, n > 1024)."""
    retired = np.setdiff1d(np.arange(B), act)
    return bool(len(retired) and len(act) and retired.min() < act.max() and len(set(levels)) >= 2 and len(act) > HINT_WAVES)


def test_hint_fleet_reaches_its_conditions():
    """On the mirror alone (the oracle's pass counts): at least two checked steps at which the rows are not the indices, the levels
    differ and more than 1024 robots are driven."""
    c = hint_case()
    assert c.B >= 2100
    o = oracle_for(c.cfg, **c.opts)
    host = mirror_of(c, o)
    reached, driven, passes = [], [], None
    for k in range(c.steps):
        act = np.nonzero(host.active)[0]
        driven.append(len(act))
        if k >= 1:
            reached.append(reach_hint(act, [level_from_passes(n) for n in passes[act]], c.B))
        _, st = host.step(o.warm_solve(threads=8))
        passes = st["reserved"].copy()                 # of all B robots, a retired one's from its last step
    print("robots driven", driven, "conditions reached at steps 1..", reached)
    assert sum(reached) >= 2, reached
