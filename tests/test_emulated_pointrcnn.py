"""CPU: the ``PointRCNN`` class (stage 1) through the HOST EMULATION, reached like tests/test_emulated_pointnet2.py.  The small
golden of tools/gen_golden_pointrcnn.py (the REAL reference on PyTorch-CPU): state layout and strict load, cls / reg within
max(1e-4, 4.4e-6 scale), the proposals against the golden and against the restatement on the product's own heads, on both
``ML3D_PRCNN_OPS`` paths; the mode and ``.train()`` refusals.  (The KITTI configuration's 2 x 16 384 points are left to the GPU.)"""
import os
import subprocess
import sys

import pytest

import emu
import prcnn_cases as C

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
import prcnn_cases as C
'''


def _case(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp")
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_small_model_against_the_reference_golden_on_both_paths():
    out = _case("C.check_model('cpu', %r)" % C.MODEL_GOLDENS[0])
    assert out.count("max_abs_delta") == 8


def test_rpn_mode_keys_and_the_refusals():
    _case("C.check_model_modes('cpu')")
