"""CPU: the device finish of the multi-cloud loops (``inference_many(finish="device")``: ``ops.vote_project``, copies on a copy
stream, results handed over by ``CloudSlots.poll`` / ``drain``) and of the single-cloud loops, executed against the HOST EMULATION of
the HIP sources like tests/test_emulated_multicloud.py, one interpreter per case.  The bodies live in tests/finish_cases.py (shared
with tests/test_gpu_multicloud_finish.py); the clouds and models are those of tests/multicloud_cases.py and
tests/kpconv_multicloud_cases.py; KPFCNN runs on four sparse tiles (``finish_cases.kpconv_setup``), here at a quarter of the widths
(``EMU_CFG``: the emulator takes seconds per full-width forward)."""
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


@pytest.mark.parametrize("in_flight", [1, 2])
def test_randlanet_device_finish_equals_host_finish(in_flight):
    """4 clouds, max_in_flight 1 and 2: a cloud retires while another is active, and every admission rebuilds the buffers while
    the retire's copies may still be on their way."""
    _run('make, clouds, seeds = randla()\nF.check_finish_device_equals_host(make(), clouds, seeds, %d)\nprint("ok")\n' % in_flight)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_kpfcnn_device_finish_equals_host_finish(in_flight):
    _run('make, clouds, seeds = kpconv()\nF.check_finish_device_equals_host(make(), clouds, seeds, %d)\nprint("ok")\n' % in_flight)


def test_single_cloud_loops_finish_like_the_host_formula():
    _run(r'''
make, clouds, seeds = randla()
F.check_single_cloud_finish(make(seed=seeds[2]), clouds[2])
make, clouds, seeds = kpconv()
np.random.seed(seeds[2])
F.check_single_cloud_finish(make(), clouds[2])
print("ok")
''')


def test_a_bad_finish_value_raises_and_a_state_without_device_indices_uploads_them():
    _run(r'''
make, clouds, seeds = randla()
F.check_bad_finish(make(), clouds, seeds)
make, clouds, seeds = kpconv()
F.check_bad_finish(make(), clouds, seeds)
F.check_pickled_tree_takes_one_upload("cpu")
print("ok")
''')
