"""CPU: ``ops.vote_project`` / ``ml3d_vote_project`` executed against the HOST EMULATION of the HIP sources (tests/hipemu), like
tests/test_emulated_multicloud.py: each case runs in its own interpreter because tests/emu_runtime.py monkeypatches the package's
device gates.  The bodies live in tests/finish_cases.py (shared with the GPU suite and with tests/test_finish_cases_can_fail.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import emu
import finish_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_runtime
emu_runtime.install("ml3d")
import finish_cases as F
'''


@pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")
@pytest.mark.parametrize("case", sorted(F.CASES))
def test_vote_project_case(case):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + 'F.CASES[%r]("cpu")\nprint("ok")\n' % case],
                       capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call (the hipcc-built library, no GPU)."""
    import __graft_entry__ as ge
    from ml3d import _abi
    ge.build()
    L = _abi.get()
    INVALID = -1
    p = C.c_void_p(256)                      # a non-null "device pointer": never followed, every call below returns before a launch

    def call(votes=p, n_sub=100, classes=19, proj=p, n_full=10, labels=p, scores=p):
        return L.ml3d_vote_project(votes, n_sub, classes, proj, n_full, labels, scores, None)
    assert call(n_full=0) == 0 and call(n_full=0, n_sub=0) == 0 and call(n_full=0, scores=None) == 0      # nothing to do: no launch
    assert call(votes=None) == INVALID and call(proj=None) == INVALID and call(labels=None) == INVALID
    assert call(classes=0) == INVALID and call(classes=257) == INVALID and call(classes=-1) == INVALID
    assert call(classes=257, n_full=0) == INVALID
    assert call(n_sub=0) == INVALID and call(n_sub=-1) == INVALID and call(n_full=-1) == INVALID
    assert call(n_full=1 << 31) == INVALID and call(n_sub=1 << 31) == INVALID and call(n_sub=1 << 40, n_full=1 << 40) == INVALID
