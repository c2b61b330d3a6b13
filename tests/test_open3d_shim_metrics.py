"""CPU (skipped without a reference checkout): beside a checkout the ``open3d`` shim rebinds ``mAP`` -- in the checkout's
``ml3d.metrics`` and in ``ml3d.torch.pipelines.object_detection`` -- to this repository's function, and
``ML3D_AMD_KEEP_REFERENCE_METRICS=1`` leaves both alone.  No other name of the two modules changes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d-ml_amd")
REF = os.environ.get("ML3D_REFERENCE_ROOT", "/root/reference")

_BODY = r'''
import os, sys, types
import torch.utils as _tu
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
sys.modules["torch.utils.tensorboard"] = _tb
_tu.tensorboard = _tb
import open3d.ml.torch
import ml3d.metrics as M
import ml3d.metrics.mAP          # (the package attribute stays whatever the shim made it)
import ml3d.torch.pipelines.object_detection as OD
ref = os.path.abspath(%(ref)r)
assert os.path.abspath(M.__file__).startswith(ref)
mod = sys.modules["ml3d.metrics.mAP"]
assert os.path.abspath(mod.__file__).startswith(ref)
native = %(native)r
want = "ml3d_amd.metrics.mAP" if native else "ml3d.metrics.mAP"
assert M.mAP.__module__ == want and OD.mAP.__module__ == want, (M.mAP.__module__, OD.mAP.__module__)
assert M.mAP is OD.mAP
# nothing else moved: the checkout's own functions are still the checkout's
assert M.precision_3d.__module__ == "ml3d.metrics.mAP" and mod.mAP.__module__ == "ml3d.metrics.mAP"
assert mod.precision_3d is M.precision_3d and mod.filter_data.__module__ == "ml3d.metrics.mAP"
assert OD.ObjectDetection.__module__ == "ml3d.torch.pipelines.object_detection"
print("SHIM OK")
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ml3d")), reason="needs the reference checkout (absent on the GPU box)")
@pytest.mark.parametrize("keep", [False, True])
def test_map_is_rebound_beside_a_checkout_unless_opted_out(keep):
    env = dict(os.environ, OPEN3D_ML_ROOT=REF, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests", "stubs")]))
    env.pop("ML3D_AMD_KEEP_REFERENCE_METRICS", None)
    if keep:
        env["ML3D_AMD_KEEP_REFERENCE_METRICS"] = "1"
    r = subprocess.run([sys.executable, "-c", _BODY % {"ref": REF, "native": not keep}], env=env, cwd="/tmp", capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SHIM OK" in r.stdout
