"""CPU: the one build recipe of the HIP library and its variants (_lib.LIBRARIES, _lib._build) and the code-generation gate's compile commands
(codegen_check.gate_commands): the gate compiles with exactly the flags csrc/Makefile builds with, and the build's freshness rule and failure
policy hold.  The recipe tests stub make and the gate: no hipcc, no GPU."""
import json
import os
import shutil
import subprocess
import types

import pytest

from conftest import ROOT
from mpc_trajectory_generator_amd import _lib, codegen_check as cc

CSRC = os.path.join(ROOT, "mpc_trajectory_generator_amd", "csrc")


def _make(*args):
    return subprocess.run(["make", "-s", "-C", CSRC, *args], capture_output=True, text=True, check=True).stdout.split()


@pytest.mark.parametrize("name", list(_lib.LIBRARIES))
def test_gate_compiles_with_the_flags_of_the_build(name, monkeypatch):
    make_vars = [f"{k}={v}" for k, v in _lib.LIBRARIES[name].items()]
    flags = _make("print-flags", *make_vars)
    assert flags[0] == "--offload-arch=gfx950"
    # print-flags is what the build itself compiles with
    assert _make("-n", "-B", "OUT=x.so", *make_vars) == [cc.HIPCC] + flags + ["-shared", "-o", "x.so", "nmpc_kernels.hip"]
    # and the gate's two compilations are that + its own flags
    seen, real = [], cc.gate_commands

    def spy(*args):
        seen.append(real(*args))
        return [["false"], ["false"]]
    monkeypatch.setattr(cc, "gate_commands", spy)
    res = cc.verify(_lib.LIBRARIES[name])
    assert res["ok"] is False and "error" in res                      # (the stubbed compilations fail)
    (sched, regalloc), = seen
    src = os.path.join(cc.CSRC, "nmpc_kernels.hip")
    dev = [cc.HIPCC] + flags + ["-S", "--cuda-device-only"]
    assert sched[:-2] == dev + ["-mllvm", "-print-before=machine-scheduler", "-mllvm", "-print-after=machine-scheduler", "-o"]
    assert regalloc[:-2] == dev + ["-mllvm", "-print-after=virtregrewriter", "-o"]
    assert sched[-1] == regalloc[-1] == src and sched[-2].endswith("x.s")
    # the verdict's `flags` (bench.py quotes the product's): the tail of that list, the scheduler flags in force + the entry's defines
    in_force = _lib.STRATEGIES.get(name, ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"])
    assert res["flags"] == in_force + _lib.LIBRARIES[name].get("EXTRA", "").split() and flags[len(flags) - len(res["flags"]):] == res["flags"]


@pytest.fixture
def tree(tmp_path, monkeypatch):
    """a copy of the kernel sources with the build's outputs redirected into it, make and the gate stubbed: -> .calls (make command lines),
    .refuse (names whose gate fails)"""
    csrc = tmp_path / "pkg" / "csrc"
    csrc.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    *kernels, header = _lib._sources()                               # (csrc/*, include/nmpc_solver.h)
    for s in kernels:
        shutil.copy(s, csrc)
    shutil.copy(header, tmp_path / "include")
    monkeypatch.setattr(_lib, "_CSRC", str(csrc))
    monkeypatch.setattr(_lib, "LIB_PATH", str(csrc / "libnmpc_hip.so"))
    monkeypatch.setattr(_lib, "BUILD_INFO", str(csrc / "build_info.json"))
    monkeypatch.setattr(_lib, "_lib_experiments", None)
    t = types.SimpleNamespace(csrc=str(csrc), calls=[], refuse=set())

    def make(cmd, **kw):
        t.calls.append(cmd)
        out = next(a[4:] for a in cmd if a.startswith("OUT="))
        with open(os.path.join(cmd[2], out), "w") as fh:
            fh.write(" ".join(cmd))
        return types.SimpleNamespace(returncode=0, stdout="", stderr="")

    def verify(make_vars=None, src=None):
        name = next(n for n, v in _lib.LIBRARIES.items() if v == (make_vars or {}))
        return {"ok": name not in t.refuse, "flags": ["-mllvm", name], "details": [] if name not in t.refuse else ["wrong code"],
                "resources": {"kernel": {"vgpr_total": 1}}}

    monkeypatch.setattr(_lib, "subprocess", types.SimpleNamespace(run=make))
    monkeypatch.setattr(cc, "verify", verify)
    return t


def _leftovers(d):
    return [f for f in os.listdir(d) if ".tmp" in f]


def test_refused_variant_leaves_no_library_and_does_not_raise(tree):
    path = _lib.variant_path("max-ilp")
    os.makedirs(os.path.dirname(path))
    with open(path, "w") as fh:
        fh.write("an older build")
    tree.refuse.add("max-ilp")
    check = _lib.build_variant("max-ilp")
    assert check["ok"] is False and check["details"] == ["wrong code"]
    assert not os.path.exists(path) and not _leftovers(os.path.dirname(path))
    with open(path[:-3] + ".json") as fh:
        assert json.load(fh)["codegen_check"] == check                # the verdict is written
    assert _lib.build_variant("max-ilp") == check and len(tree.calls) == 1      # and stands until the content changes


def test_refused_experiments_build_is_an_error_that_quotes_the_verdict(tree):
    tree.refuse.add(_lib.EXPERIMENTS)
    with pytest.raises(RuntimeError, match="REFUSED.*wrong code"):
        _lib.load_library(experiments=True)


def test_refused_product_raises_and_keeps_the_library_in_place(tree):
    with open(_lib.LIB_PATH, "w") as fh:
        fh.write("the library in place")
    with open(_lib.BUILD_INFO, "w") as fh:
        fh.write('{"source_hash": "describes the library in place"}')
    tree.refuse.add(_lib.PRODUCT)
    with pytest.raises(RuntimeError, match="REFUSED"):
        _lib.build_library()
    with open(_lib.LIB_PATH) as fh:
        assert fh.read() == "the library in place"
    with open(_lib.BUILD_INFO) as fh:
        assert fh.read() == '{"source_hash": "describes the library in place"}'
    with open(_lib.BUILD_INFO + ".refused") as fh:
        assert json.load(fh)["codegen_check"]["ok"] is False
    assert not _leftovers(tree.csrc)


def test_a_library_is_rebuilt_only_when_its_content_changes(tree):
    assert _lib.build_library() == _lib.LIB_PATH
    assert _lib.build_variant("win0")["ok"]
    assert len(tree.calls) == 2 and tree.calls[0][-1].startswith("OUT=") and tree.calls[1][-1] == "EXTRA=-DNMPC_WIN=0 -DNMPC_WIN2=0"
    with open(_lib.BUILD_INFO) as fh:
        info = json.load(fh)
    assert set(info) == {"source_hash", "flags", "codegen_check", "resources", "build_key"} and info["source_hash"] == _lib.source_hash()
    assert info["flags"] == ["-mllvm", _lib.PRODUCT] and "resources" not in info["codegen_check"]
    makefile = os.path.join(tree.csrc, "Makefile")
    os.utime(makefile, (2e9, 2e9))                                    # a newer time stamp is not a change
    _lib.build_library()
    _lib.build_variant("win0")
    assert len(tree.calls) == 2
    with open(makefile, "a") as fh:                                   # a changed Makefile is
        fh.write("\n# edited\n")
    _lib.build_library()
    _lib.build_variant("win0")
    assert len(tree.calls) == 4
    _lib.build_variant("win0", force=True)
    assert len(tree.calls) == 5 and not _leftovers(tree.csrc) and not _leftovers(os.path.dirname(_lib.variant_path("win0")))
