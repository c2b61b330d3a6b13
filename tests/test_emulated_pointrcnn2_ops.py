"""CPU: ``ml3d_roi_pool`` of csrc/pointrcnn.hip through the HOST EMULATION (tests/hipemu), reached like
tests/test_emulated_pointrcnn_ops.py: each case runs in its own interpreter with tests/emu_runtime.py installed, so the product's own
wrapper (``ml3d.ops.roi_pool``) drives the emulated kernel.  The bodies are those of tests/prcnn2_cases.py, the same ones
tests/test_gpu_pointrcnn2_ops.py runs on the MI355X: ``pool_idx`` / ``empty`` for EQUALITY with the restatement of
tests/prcnn2_ref.py, the leading columns against the float64 formula within max(1e-5, 4 e32), the feature columns bit for bit."""
import os
import subprocess
import sys

import pytest

import emu
import prcnn2_cases as C      # (the shape tables only: the bodies run in the subprocess)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import emu_runtime
emu_runtime.install("ml3d")
import prcnn2_cases as C
'''


def _case(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp")
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("n", C.POOL_N)
def test_roi_pool_equals_the_restatement(n):
    out = _case("C.check_pool('cpu', %d)" % n)
    assert out.count("max_abs_delta") == len(C.pool_cases(n))


def test_roi_pool_refusals():
    _case("C.check_pool_refusals('cpu')")
