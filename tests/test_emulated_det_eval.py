"""CPU: ``ops.det_match`` and ``ml3d.metrics`` executed against the HOST EMULATION of the HIP sources (tests/hipemu), like
tests/test_emulated_eval.py: each case runs in its own interpreter because tests/emu_runtime.py monkeypatches the package's device
gates.  The bodies live in tests/det_cases.py (shared with the GPU suite and with tests/test_det_cases_can_fail.py)."""
import os
import subprocess
import sys

import pytest

import emu
import det_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_runtime
emu_runtime.install("ml3d")
import det_cases as V
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + '\nprint("ok")\n'],
                       capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("case", sorted(V.CASES))
def test_det_match_case(case):
    _run('V.CASES[%r]("cpu")' % case)


@pytest.mark.parametrize("route", ["device", "host"])
def test_map_and_objdetmetric_reproduce_the_reference(route):
    """``mAP`` / ``precision_3d`` / ``ObjdetMetric`` on the frames of tests/golden/eval_objdet.npz: the reference's arrays."""
    _run('V.check_golden_model("cpu", %r)' % route)
