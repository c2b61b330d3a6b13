"""CPU: csrc/pointnet2.hip through the HOST EMULATION (tests/hipemu), reached like tests/test_emulated_pointtransformer.py: each
case runs in its own interpreter with tests/emu_runtime.py installed, so the product's own wrappers (``ml3d.ops.pointnet2``)
drive the emulated kernels.  The bodies are those of tests/pn2_cases.py, the same ones tests/test_gpu_pointnet2.py runs on the
MI355X: index results equal to the numpy restatements of tests/pn2_ref.py, floats against the float64 formula within
max(1e-5, 4 e32).  This run is where the bodies themselves get debugged."""
import os
import subprocess
import sys

import pytest

import emu
import pn2_cases as C      # (the shape tables only: the bodies run in the subprocess)

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
import pn2_cases as C
'''


def _case(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp")
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("n", C.BALL_N)
def test_ball_query_both_scales_in_one_scan_equal_the_contract(n):
    _case("for m in C.BALL_M:\n    C.check_ball_query('cpu', %d, m)" % n)


def test_ball_query_truncation_padding_no_hit_and_early_fill():
    _case("C.check_ball_query_properties('cpu')")


def test_ball_query_boundary_duplicates_batch_and_refusals():
    _case("C.check_ball_query_boundary_and_duplicates('cpu')\nC.check_ball_query_batch('cpu')\nC.check_ball_query_refusals('cpu')")


@pytest.mark.parametrize("ns", C.SA_NSAMPLE)
@pytest.mark.parametrize("cf,widths", C.SA_CASES, ids=["-".join(map(str, w)) for _, w in C.SA_CASES])
def test_set_abstraction_against_float64(cf, widths, ns):
    out = _case("for m in C.SA_M:\n    C.check_sa('cpu', %d, %r, %d, m)" % (cf, tuple(widths), ns))
    assert out.count("max_abs_delta") == len(C.SA_M)


def test_set_abstraction_refusals():
    _case("C.check_sa_refusals('cpu')")


def test_small_module_forward_against_the_reference_golden():
    """(the KITTI backbone's 2 x 16 384 points are left to the GPU)"""
    out = _case("C.check_module('cpu', %r)" % C.MODULE_GOLDENS[0])
    assert out.count("max_abs_delta") == 3


def test_three_nn_order_ties_and_refusal():
    _case("C.check_three_nn('cpu')")


@pytest.mark.parametrize("c", C.INTERP_C)
def test_interpolate_against_float64(c):
    out = _case("C.check_interpolate('cpu', %d)" % c)
    assert out.count("max_abs_delta") == 2
