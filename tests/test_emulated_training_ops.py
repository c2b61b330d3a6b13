"""CPU: every dispatch arm of csrc/train.hip and the four differentiable entry points of csrc/randla.hip through the HOST EMULATION
(tests/hipemu), reached like tests/test_emulated_kpconv_ops.py: each group of cases runs in its own interpreter with
tests/emu_runtime.py installed, so the product's own wrappers (``ml3d.ops.train``, ``ml3d.ops.randla``) and the C entry points drive
the emulated kernels.  The bodies and tables are those of tests/train_cases.py, the same ones tests/test_gpu_training_ops.py runs on
the MI355X: floats against the float64 formulas of tests/train_ref.py within max(1e-5, 4 e32); gather / max forwards, repeated calls
of everything without float atomics and the sentinel padding for equality.  No case is left to the GPU: the three-level partial
sum (2050 points at d = 18), the 160 MB cap of the private partials (1282 points at d = 256, the one slow case) and the grids past
the caps of ``tr_blocks`` run here too."""
import os
import subprocess
import sys

import pytest

import emu
import train_cases as C      # (the tables only: the bodies run in the subprocess)

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
import train_cases as C
'''


def _case(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp")
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("group", C.GROUPS)
def test_group_on_the_emulator(group):
    cases = C.cases_of(group)
    out = _case("for c in C.cases_of(%r):\n    C.run_case('cpu', c)" % group)
    assert out.count("max_abs_delta") == sum(C.comparisons(c) for c in cases), out[-3000:]
    assert out.count(" arm=") == len(cases)


@pytest.mark.parametrize("family", C.REFUSAL_FAMILIES)
def test_refusals(family):
    _case("C.check_refusals('cpu', %r)" % family)
