"""CPU: PointRCNN stage 2 (RoI pooling, the RCNN network, ``inference_end``) through the HOST EMULATION (tests/hipemu), each case in
its own interpreter with tests/emu_runtime.py installed -- the model bodies of tests/prcnn2_cases.py, the same ones
tests/test_gpu_pointrcnn2.py runs on the MI355X, against tests/golden/pointrcnn_rcnn_small.npz (tools/gen_golden_pointrcnn2.py: the
REAL reference's ``RCNN.forward`` on PyTorch-CPU, its wheel op stood in for by the restatement of tests/prcnn2_ref.py)."""
import os
import subprocess
import sys

import pytest

import emu

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


def test_pooling_equals_the_golden_on_its_rois_and_the_restatement_on_the_models_own():
    _case("C.check_model_pooling('cpu')")


def test_network_on_the_goldens_rows_on_both_paths():
    _case("C.check_model_network('cpu')")


def test_rcnn_forward_is_its_two_halves_and_chunks_do_not_change_a_bit():
    _case("C.check_model_plumbing('cpu')")


def test_inference_end_reproduces_the_goldens_detections():
    _case("C.check_model_inference_end('cpu')")


def test_forward_still_refuses_and_names_the_new_method():
    _case("C.check_model_refusals('cpu')")
