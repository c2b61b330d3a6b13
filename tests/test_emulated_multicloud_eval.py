"""CPU: ``inference_many(evaluate=True)`` of RandLA-Net and KPFCNN (ground-truth scoring of every finished cloud, on the device by
``ops.vote_confusion`` or on the host) executed against the HOST EMULATION of the HIP sources like
tests/test_emulated_multicloud_finish.py, one interpreter per case.  The bodies live in tests/eval_cases.py (shared with
tests/test_gpu_multicloud_eval.py); clouds and models are those of ``finish_cases.randla_setup`` / ``kpconv_setup``."""
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
import finish_cases as F
import eval_cases as V
import kpconv_multicloud_cases as K
randla = lambda: F.randla_setup("cpu")
kpconv = lambda: F.kpconv_setup("cpu", K.EMU_CFG)
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=1500,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("finish", ["device", "host"])
def test_randlanet_evaluate(finish):
    _run('make, clouds, seeds = randla()\nV.check_model_evaluate(make(), clouds, seeds, %r)\nprint("ok")\n' % finish)


@pytest.mark.parametrize("finish", ["device", "host"])
def test_kpfcnn_evaluate(finish):
    _run('make, clouds, seeds = kpconv()\nV.check_model_evaluate(make(), clouds, seeds, %r)\nprint("ok")\n' % finish)


def test_a_label_of_the_wrong_length_raises_before_any_patch_runs():
    _run(r'''
make, clouds, seeds = randla()
V.check_wrong_length_label(make(), clouds, seeds)
make, clouds, seeds = kpconv()
V.check_wrong_length_label(make(), clouds, seeds)
print("ok")
''')
