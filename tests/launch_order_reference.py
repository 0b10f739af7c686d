"""The launch order's rule, literally (a helper module of the tests, not a conftest): DESIGN.md section 5.5 restated one instance at
a time in scalar Python, the way ``panoc_reference.py`` and ``alm_reference.py`` restate theirs.  No loop of the kernels is transcribed:
the functions follow the words of the rule.

The library is compiled with ``-ffp-contract=off`` and the classification is unfused f64 -- products, sums, ``rint``, ``fabs``,
``fmax``, ``fmin`` and strict comparisons -- so Python's floats give the device's integers and nothing here has a tolerance.

* ``level_from_inputs(cfg, p)``: the hardness level 0..12 of one parameter vector and the six flags it is made of.
* ``level_from_passes(n)``: the level of an instance whose previous solve took ``n`` evaluation passes.
* ``stable_partition(levels)``: the order instances are handed out in.
* ``flag_margins(cfg, p, F)``: the flags once more in the number type ``F`` (``np.longdouble``), with the smallest relative distance
  of any compared pair: how far the instance is from the nearest threshold.
"""
from __future__ import annotations

import math

import numpy as np

NZ = 20                        # p[0:20]: state, last controls, target, weights; then N speeds, circles, ellipses, reference samples
CLEARANCE = 0.6                # m: a reference sample this close to an obstacle's edge makes the instance hard
GRAZE = 0.05                   # m: ... this close, it grazes
BEND = 0.05                    # rad of summed |heading change| of the reference samples
SPEED_GAP = 1.0                # m/s between the last applied speed and the first reference speed
LEVELS = 13
TWO_PI, INV_TWO_PI = 6.283185307179586, 0.15915494309189535      # the two constants of the kernel's wrap
FLAGS = ("graze", "early", "hard", "bend", "gap", "goal")


def offsets(cfg):
    """-> (speeds, circles, ellipses, reference samples): where each block of p starts"""
    N = cfg.N_hor
    circles = NZ + N
    ellipses = circles + 3 * cfg.Nobs
    refs = ellipses + 5 * cfg.Ndynobs * N
    assert refs + 3 * N == cfg.n_p
    return NZ, circles, ellipses, refs


def _rint(x):
    """round to the nearest integer, ties to even; NaN and infinities stay"""
    if x != x or x in (math.inf, -math.inf):
        return x
    return type(x)(np.rint(x)) if isinstance(x, np.floating) else float(round(x))


def _fmax(a, b):               # C's fmax / fmin: a NaN operand loses
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _distance(a, b):
    """relative distance of a compared pair (inf where a NaN or an infinity decides the comparison whatever the rounding)"""
    if not (math.isfinite(a) and math.isfinite(b)):
        return math.inf
    m = max(abs(a), abs(b))
    return math.inf if m == 0 else float(abs(a - b) / m)


def _flags(cfg, p, F):
    """-> (flags, margin).  Every operation is one rounded operation of the type F, in the order the rule's words give."""
    N, nobs, ndyn = cfg.N_hor, cfg.Nobs, cfg.Ndynobs
    _, c0, e0, r0 = offsets(cfg)
    p = [F(v) for v in p]
    clearance, graze_by, two_pi, inv_two_pi = F(CLEARANCE), F(GRAZE), F(TWO_PI), F(INV_TWO_PI)
    margin = [math.inf]

    def less(a, b):
        margin[0] = min(margin[0], _distance(a, b))
        return bool(a < b)

    graze = early = hard = False
    bend = F(0.0)
    circles = []                               # (centre, the two squared limits) of the slots that hold a circle
    for k in range(nobs):
        cx, cy, r = p[c0 + 3 * k], p[c0 + 3 * k + 1], p[c0 + 3 * k + 2]
        if r > 0:                              # an empty slot (r = 0), a negative or a NaN radius: skipped
            far, near = r + clearance, r + graze_by
            circles.append((cx, cy, far * far, near * near))
    for t in range(N):
        x, y = p[r0 + 3 * t], p[r0 + 3 * t + 1]
        if t >= 1:
            d = p[r0 + 3 * t + 2] - p[r0 + 3 * (t - 1) + 2]
            d = d - two_pi * _rint(d * inv_two_pi)
            bend = bend + abs(d)
        for cx, cy, far2, near2 in circles:
            dx, dy = x - cx, y - cy
            d2 = dx * dx + dy * dy
            if less(d2, far2):
                hard = True
            if less(d2, near2):
                graze = True
                if 2 * t < N:
                    early = True
        for k in range(ndyn):
            e = e0 + (k * N + t) * 5
            dx, dy = x - p[e], y - p[e + 1]
            d2 = dx * dx + dy * dy
            far, near = _fmax(p[e + 2], p[e + 3]) + clearance, _fmin(p[e + 2], p[e + 3]) + graze_by
            if less(d2, far * far):
                hard = True
            if less(d2, near * near):
                graze = True                   # (an ellipse never sets early)
    bent = less(F(BEND), bend)
    gap = less(F(SPEED_GAP), abs(p[NZ] - p[3]))
    last, before = r0 + 3 * (N - 1), r0 + 3 * (N - 2)
    goal = bool(p[last] == p[before] and p[last + 1] == p[before + 1])       # inputs compared as they are: no rounding to be near
    return dict(graze=graze, early=early, hard=hard, bend=bent, gap=gap, goal=goal), margin[0]


def level_of(flags):
    return 4 * flags["graze"] + 4 * flags["early"] + flags["hard"] + flags["bend"] + flags["gap"] + flags["goal"]


def level_from_inputs(cfg, p):
    """-> (level, flags) of one parameter vector p [n_p]"""
    flags, _ = _flags(cfg, [float(v) for v in p], float)
    return level_of(flags), flags


def flag_margins(cfg, p, F=np.longdouble):
    """-> (flags computed in F, the smallest relative distance of any pair the rule compares)"""
    return _flags(cfg, np.asarray(p, dtype=np.float64), F)


def level_from_passes(n):
    """0 below 32 passes, else floor(log2 n) - 4, at most 12; n: any uint32 value"""
    n = int(n)
    assert 0 <= n < 1 << 32
    if n < 32:
        return 0
    return min(n.bit_length() - 1 - 4, LEVELS - 1)


def stable_partition(levels):
    """-> the indices, those of the highest level first, ascending within a level"""
    out = []
    for lvl in range(LEVELS - 1, -1, -1):
        for i, v in enumerate(levels):
            if v == lvl:
                out.append(i)
    return out
