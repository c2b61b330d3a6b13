"""CPU: the k-NN pyramid's grid builders through the host emulator (tests/hipemu), the cases of tests/pyramid_build_cases.py.

* the default build against the oracle, bit for bit (from 48 clouds on: grid_build_pyramid, one launch with one workgroup per
  cloud; below: the launch chain);
* the cases the one-workgroup builder serves again through a second emulator library whose knn.hip is compiled with
  ``-DML3D_GRID_PYRAMID_FUSED=0`` (the launch chain everywhere), in a child interpreter: both builds must return identical
  neighbour and interpolation arrays AND identical grids -- the GridSeg records, the cell-start words a search reads, the set of
  points of every cell;
* the path choice at the batch bound, read off the emulator's launch trace.

What the emulator's cooperative fibers cannot show (a missing wait between two phases, a stale cache line) is the business of
tests/test_gpu_pyramid_build.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import pyramid_build_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

CASES = list(PC.EMULATED)
FUSED = list(PC.FUSED)


@pytest.fixture(scope="module")
def fused():
    """{case: emulated_grids(case)} of the default build, filled as the tests ask."""
    return {}


def _fused(cache, name):
    if name not in cache:
        cache[name] = PC.emulated_grids(name)
    return cache[name]


@pytest.mark.parametrize("name", CASES)
def test_pyramid_through_the_default_build_matches_the_oracle(fused, name):
    g = _fused(fused, name)
    nl = len(PC.CASES[name][1])
    PC.check(name, [g["nbr%d" % l] for l in range(nl)], [g["itp%d" % l] for l in range(nl)], [g["order%d" % l] for l in range(nl)])


def _chain_library():
    """The emulator library with knn.hip rebuilt for the launch chain (every other object is the default build's)."""
    base = subprocess.check_output([os.path.join(HERE, "hipemu", "build_emu.sh")]).decode().strip().splitlines()[-1]
    build = os.path.dirname(base)
    cxx = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    obj = os.path.join(build, "knn_pyramid_chain_variant.o")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fPIC", "-DML3D_TEST_HOOKS", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unused-value", "-Wno-deprecated-declarations", "-DML3D_GRID_PYRAMID_FUSED=0",
                           "-I" + os.path.join(HERE, "hipemu", "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "open3d-ml_amd", "csrc"), "-x", "c++", "-c",
                           os.path.join(ROOT, "open3d-ml_amd", "csrc", "knn.hip"), "-o", obj])
    others = [os.path.join(build, f) for f in sorted(os.listdir(build))
              if f.endswith(".o") and f not in ("knn.hip.o", os.path.basename(obj))]
    so = os.path.join(build, "libml3d_emu_pyramid_chain.so")
    subprocess.check_call([cxx, "-shared", "-rdynamic", "-o", so + ".tmp.%d" % os.getpid(), obj] + others + ["-lpthread"])
    os.replace(so + ".tmp.%d" % os.getpid(), so)
    return so


_CHILD = r"""
import os, sys
for p in (%(root)r, os.path.join(%(root)r, "open3d-ml_amd"), %(here)r):
    sys.path.insert(0, p)
import numpy as np
import pyramid_build_cases as PC
for name in %(cases)r:
    np.savez(os.path.join(%(out)r, name + ".npz"), **PC.emulated_grids(name))
print("chain ok")
"""


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """Directory of <case>.npz: emulated_grids of every case through the launch-chain build (one child interpreter: another library)."""
    emu.lib()
    out = str(tmp_path_factory.mktemp("pyramid_chain"))
    so = _chain_library()
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "here": HERE, "cases": FUSED, "out": out}],
                       capture_output=True, text=True, timeout=1500, cwd="/tmp", env=dict(os.environ, ML3D_EMU_LIB=so, HIPEMU_TRACE="1"))
    assert r.returncode == 0 and "chain ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    # the child really took the chain: it launched the chain's kernels and never the one-workgroup builder
    assert "grid_hist" in r.stderr and "grid_pyramid_cloud" not in r.stderr, r.stderr[-2000:]
    return out


def test_path_choice_follows_the_cloud_size():
    """The default build's launches (HIPEMU_TRACE, a child interpreter): one grid_pyramid_cloud launch and no chain kernel at 48
    clouds, the chain and no grid_pyramid_cloud launch at 47 (and at one)."""
    emu.lib()
    for name, want_fused in (("one_cloud_fused", True), ("below_min_batch", False), ("one_cloud", False)):
        code = _CHILD % {"root": ROOT, "here": HERE, "cases": [], "out": ""} + "PC.emulated_grids(%r)\n" % name
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd="/tmp",
                           env=dict(os.environ, HIPEMU_TRACE="1"))
        assert r.returncode == 0, r.stderr[-4000:]
        assert (r.stderr.count("grid_pyramid_cloud") == 1) == want_fused and ("grid_hist" in r.stderr) != want_fused, (name, r.stderr[-2000:])


@pytest.mark.parametrize("name", FUSED)
def test_both_builders_give_identical_results_and_identical_grids(fused, chain, name):
    a = _fused(fused, name)
    with np.load(os.path.join(chain, name + ".npz")) as b:
        assert sorted(a) == sorted(b.files)
        for key in sorted(a):
            if key.startswith("order"):
                continue                    # arrival order inside a cell: free in both builders
            assert np.array_equal(a[key], b[key]), (name, key)
