"""CPU: the launch geometry of a batch solve (csrc/nmpc_launch.h: what solve_launch launches by and nmpc_launch_geometry reports),
compiled for the host in a stand-alone program (tests/launch_geometry_main.cpp) under -fsanitize=undefined,address and printed for every
batch size 0 .. 3 grid_cap + 2, grid_cap in {4, 8, 1024, 2048}, both kernel families, ordering on and off, the pools' knobs on and off and
the forced owner counts of the experiments build.  Every line must be ``entry_cases.literal_geometry``, the rule as DESIGN.md section 5.5
and the header state it, and with automatic owners the invariants of a launch in which no wave and no workgroup is without work hold."""
import os
import subprocess

import pytest

from conftest import ROOT
from entry_cases import literal_geometry

CAPS = (4, 8, 1024, 2048)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_geometry") / "launch_geometry")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpc_trajectory_generator_amd", "csrc"), os.path.join(ROOT, "tests", "launch_geometry_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + [str(c) for c in CAPS], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        left, right = line.split(" : ")
        out.append((tuple(int(w) for w in left.split()), tuple(int(w) for w in right.split())))
    return out


def test_header_includes_no_hip_header():
    text = open(os.path.join(ROOT, "mpc_trajectory_generator_amd", "csrc", "nmpc_launch.h")).read()
    assert "#include" not in text


def test_every_case_is_printed(lines):
    keys = [k for k, _ in lines]
    assert len(set(keys)) == len(keys) == sum(3 * c + 3 for c in CAPS) * 2 * 2 * 8
    for cap in CAPS:
        for P in (20, 40):
            for order in (0, 1):
                assert {k[6] for k in keys if k[:3] == (cap, P, order) and k[3:6] == (500, 1, 0)} == set(range(3 * cap + 3))


def test_geometry_equals_the_literal_rule(lines):
    bad = [(k, got) for k, got in lines if got != literal_geometry(B=k[6], grid_cap=k[0], P=k[1], use_order=k[2], park_min=k[3],
                                                                   sched_mode=k[4], forced=k[5])]
    assert not bad, bad[:5]


def test_invariants_of_the_automatic_geometry(lines):
    seen_owners, seen_flags = set(), set()
    for (cap, P, order, park_min, sched, forced, B), (grid, owners, wgs, ordered, pools, pool_cap) in lines:
        if forced:
            continue
        where = (cap, P, order, park_min, sched, B)
        assert 1 <= owners <= 4, where
        assert wgs <= cap // 4, where
        assert wgs * owners >= grid, where
        assert wgs * owners - grid < owners, where            # no workgroup without an owner that has work
        assert grid == min(B, cap), where
        assert (ordered, pools) == (0, 0) or B > cap, where
        assert ordered in (0, 1) and pools in (0, 1), where
        assert ordered == int(B > cap and order == 1), where
        assert pool_cap == B, where
        seen_owners.add(owners)
        seen_flags.add((ordered, pools))
    assert seen_owners == {1, 2, 3, 4} and seen_flags == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_boundaries_by_hand(lines):
    """the sizes at which a regime begins, for 2048 resident waves (256 CUs x 8, the headline kernel): G = 512 workgroups"""
    got = {k[6]: v for k, v in lines if k[:6] == (2048, 20, 1, 500, 1, 0)}
    assert got[1] == (1, 1, 1, 0, 0, 1)
    assert got[512] == (512, 1, 512, 0, 0, 512)
    assert got[513] == (513, 2, 257, 0, 0, 513)               # 257 workgroups x 2 owners: one wave owns nothing
    assert got[1024] == (1024, 2, 512, 0, 0, 1024)
    assert got[1025] == (1025, 3, 342, 0, 0, 1025)
    assert got[1536] == (1536, 3, 512, 0, 0, 1536)
    assert got[1537] == (1537, 4, 385, 0, 0, 1537)
    assert got[2048] == (2048, 4, 512, 0, 0, 2048)
    assert got[2049] == (2048, 4, 512, 1, 1, 2049)
    assert got[6146] == (2048, 4, 512, 1, 1, 6146)
