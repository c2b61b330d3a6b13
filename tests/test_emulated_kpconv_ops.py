"""CPU: every dispatch arm of csrc/kpconv.hip through the HOST EMULATION (tests/hipemu), reached like
tests/test_emulated_pointnet2.py: each group of cases runs in its own interpreter with tests/emu_runtime.py installed, so the
product's own wrappers (``ml3d.ops.kpconv``) drive the emulated kernels.  The bodies and tables are those of tests/kp_cases.py, the
same ones tests/test_gpu_kpconv_ops.py runs on the MI355X: floats against the float64 formulas of tests/kp_ref.py within
max(1e-5, 4 e32), repeated calls / rows alone / all-shadow rows / pools for equality.  This run is where the bodies themselves get
debugged.  No case is left to the GPU: both long walks (8221 queries on kp_agg_mfma, 16 517 on kp_agg_gemm32) run here too."""
import os
import subprocess
import sys

import pytest

import emu
import kp_cases as C      # (the tables only: the bodies run in the subprocess)

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
import kp_cases as C
'''


def _case(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp")
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def _comparisons(cases):
    """Lines with measured figures a group prints: one per float case, three per H = 0 case (its three activations), three for
    nq = 0 (its shapes), two per adjoint case (dx, then the inner-product identity)."""
    per = dict(weighted=1, rigid=1, deformable=1, adjoint=2, h0=3, nq0=len(C.H0_SHAPES), pool=0)
    return sum(per[c["body"]] for c in cases)


@pytest.mark.parametrize("group", C.GROUPS)
def test_group_on_the_emulator(group):
    cases = C.cases_of(group)
    out = _case("for c in C.cases_of(%r):\n    C.run_case('cpu', c)" % group)
    assert out.count("max_abs_delta") == _comparisons(cases), out[-3000:]
    assert out.count(" arm=") >= len(cases) - sum(c["body"] in ("adjoint", "nq0", "h0") for c in cases)


def test_deformable_refusals():
    _case("C.check_deformable_refusals('cpu')")
