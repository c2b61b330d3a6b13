"""CPU: ``ops.vote_confusion`` / ``ops.score_confusion`` executed against the HOST EMULATION of the HIP sources (tests/hipemu), like
tests/test_emulated_vote_project.py: each case runs in its own interpreter because tests/emu_runtime.py monkeypatches the package's
device gates.  The bodies live in tests/eval_cases.py (shared with the GPU suite and with tests/test_eval_cases_can_fail.py)."""
import os
import subprocess
import sys

import pytest

import emu
import eval_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_runtime
emu_runtime.install("ml3d")
import eval_cases as V
'''


@pytest.mark.parametrize("case", sorted(V.CASES))
def test_confusion_case(case):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + 'V.CASES[%r]("cpu")\nprint("ok")\n' % case],
                       capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def _merge_library():
    """The emulator library with knn.hip rebuilt with ``-DML3D_CONFUSION_WAVE_MERGE=1`` (every other object is the default build's).
    Its object lives in a directory of its own: other variant builds link every object of the build directory."""
    base = subprocess.check_output([os.path.join(ROOT, "tests", "hipemu", "build_emu.sh")]).decode().strip().splitlines()[-1]
    build = os.path.dirname(base)
    own = os.path.join(build, "confusion_merge")
    os.makedirs(own, exist_ok=True)
    cxx = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    obj = os.path.join(own, "knn_merge.o")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fPIC", "-DML3D_TEST_HOOKS", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unused-value", "-Wno-deprecated-declarations", "-DML3D_CONFUSION_WAVE_MERGE=1",
                           "-I" + os.path.join(ROOT, "tests", "hipemu", "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "open3d-ml_amd", "csrc"), "-x", "c++", "-c",
                           os.path.join(ROOT, "open3d-ml_amd", "csrc", "knn.hip"), "-o", obj])
    others = [os.path.join(build, f) for f in sorted(os.listdir(build))
              if (f.endswith(".hip.o") and f != "knn.hip.o") or f == "hipemu.cpp.o"]
    so = os.path.join(own, "libml3d_emu_confusion_merge.so")
    subprocess.check_call([cxx, "-shared", "-rdynamic", "-o", so + ".tmp.%d" % os.getpid(), obj] + others + ["-lpthread"])
    os.replace(so + ".tmp.%d" % os.getpid(), so)
    return so


@pytest.fixture(scope="module")
def merge_library():
    emu.lib()
    return _merge_library()


@pytest.mark.parametrize("case", sorted(V.DATA_CASES))
def test_confusion_case_with_the_wave_merge_build(merge_library, case):
    """The A/B form that is off by default (a wave merges its equal cells by ballot before the add) passes the same cases."""
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + 'V.CASES[%r]("cpu")\nprint("ok")\n' % case],
                       capture_output=True, text=True, timeout=900, cwd="/tmp", env=dict(os.environ, ML3D_EMU_LIB=merge_library))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
