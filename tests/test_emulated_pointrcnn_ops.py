"""CPU: csrc/pointrcnn.hip through the HOST EMULATION (tests/hipemu), reached like tests/test_emulated_pointnet2.py: each case runs
in its own interpreter with tests/emu_runtime.py installed, so the product's own wrappers (``ml3d.ops.pointrcnn``) drive the
emulated kernels.  The bodies are those of tests/prcnn_cases.py, the same ones tests/test_gpu_pointrcnn_ops.py runs on the MI355X:
the decode against the float64 formula within max(1e-5, 4 e32), the proposals for EQUALITY with the restatement of
tests/prcnn_ref.py.  This run is where the bodies themselves get debugged."""
import os
import subprocess
import sys

import pytest

import emu
import prcnn_cases as C      # (the shape tables only: the bodies run in the subprocess)

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


@pytest.mark.parametrize("bins", C.DECODE_BINS, ids=["H%d" % b[2] for b in C.DECODE_BINS])
def test_decode_all_flags_and_widths_against_float64(bins):
    out = _case("for n in C.DECODE_N:\n    C.check_decode('cpu', n, %r)" % (bins,))
    assert out.count("max_abs_delta") == len(C.DECODE_N) * 16


def test_decode_refuses_a_wrong_channel_count():
    _case("C.check_decode_refusals('cpu')")


@pytest.mark.parametrize("n", C.PROP_N)
def test_proposals_equal_the_restatement(n):
    _case("for pre, post in C.PROP_PRE_POST:\n    C.check_proposals('cpu', %d, pre, post)" % n)


@pytest.mark.parametrize("n", (65, 700))
def test_proposals_zone_and_suppression_arms(n):
    _case("for kind in C.PROP_KINDS:\n    for pre, post in ((10, 4), (9000, 100)):\n"
          "        C.check_proposals('cpu', %d, pre, post, kind, batches=(3,))" % n)


def test_proposals_refusals():
    _case("C.check_proposal_refusals('cpu')")
