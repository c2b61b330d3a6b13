"""CPU, no kernel: the host side of PointRCNN stage 1 -- the two entry points are declared and bound, the wrappers check their
arguments before any call and refuse CPU tensors with the project's message, the class is importable and refuses a CPU device, and
the ``open3d`` shim leaves the reference's own ``PointRCNN`` in the registry (the native class cannot run the default mode yet)."""
import os
import re

import pytest
import torch

from ml3d import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    assert "#define ML3D_ABI_VERSION 13" in header
    for sym in ("ml3d_bin_decode", "ml3d_rpn_proposals"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _abi.SYMBOLS
    assert "_workspace_bytes" not in "".join(s for s in _abi.SYMBOLS if "rpn" in s or "bin_decode" in s)

    class Fn:
        pass

    class Lib:
        def __getattr__(self, name):
            f = Fn()
            object.__setattr__(self, name, f)
            return f

    lib = _abi.bind(Lib())
    assert len(lib.ml3d_bin_decode.argtypes) == 17 and len(lib.ml3d_rpn_proposals.argtypes) == 19


def test_cpu_tensors_are_refused_with_the_no_fallback_message():
    from ml3d import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bin_decode(torch.zeros((4, 3)), torch.zeros((4, 76)), (1.5, 1.6, 3.9), 3.0, 0.5, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rpn_proposals(torch.zeros((1, 8)), torch.zeros((1, 8, 7)), 10, 4, 0.8)


def test_argument_checks_raise_before_the_call(monkeypatch):
    from ml3d import ops
    from ml3d.ops import _gates, pointrcnn
    monkeypatch.setattr(_gates, "_need_gpu", lambda *t: None)
    monkeypatch.setattr(_abi, "get", lambda: None)             # (a call into the library would be an AttributeError)
    roi, reg = torch.zeros((4, 3)), torch.zeros((4, 76))
    for bad in (lambda: ops.bin_decode(roi[:, :2], reg, (1.5, 1.6, 3.9), 3.0, 0.5, 12),
                lambda: ops.bin_decode(roi, reg[:, :75], (1.5, 1.6, 3.9), 3.0, 0.5, 12),
                lambda: ops.bin_decode(roi, reg[:3], (1.5, 1.6, 3.9), 3.0, 0.5, 12),
                lambda: ops.bin_decode(roi, reg, (1.5, 1.6), 3.0, 0.5, 12),
                lambda: ops.bin_decode(roi, reg, (1.5, 1.6, 3.9), 3.0, 0.0, 12),
                lambda: ops.bin_decode(roi, reg.double(), (1.5, 1.6, 3.9), 3.0, 0.5, 12),
                lambda: ops.rpn_proposals(torch.zeros((1, 8)), torch.zeros((1, 9, 7)), 10, 4, 0.8),
                lambda: ops.rpn_proposals(torch.zeros((1, 8)), torch.zeros((1, 8, 7)), 70000, 4, 0.8),
                lambda: ops.rpn_proposals(torch.zeros((1, 8)), torch.zeros((1, 8, 7)), 10, -1, 0.8),
                lambda: ops.rpn_proposals(torch.zeros((1, 8)), torch.zeros((1, 8, 7)), 10, 4, 0.8, out=(torch.zeros((1, 4, 7)),) * 3)):
        with pytest.raises(RuntimeError):
            bad()
    assert pointrcnn.reg_channels(3.0, 0.5, 12) == 76 and pointrcnn.reg_channels(1.5, 0.5, 9, True, True, 0.5, 0.25) == 53


def test_the_class_is_exported_and_needs_a_gpu():
    from ml3d.torch.models import PointRCNN
    import ml3d.torch.models as M
    assert "PointRCNN" in M.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PointRCNN(device="cpu", mode="RPN")


def test_the_shim_keeps_the_reference_class_in_the_registry():
    src = open(os.path.join(ROOT, "open3d-ml_amd", "open3d", "ml", "torch", "__init__.py")).read()
    registered = src[src.index("for cls in ("):src.index("MODEL._register_module(cls")]
    assert "PointRCNN" not in registered
    assert "native.RandLANet" in registered


_REGISTRY = r'''
import os, sys, types
try:
    import torch.utils.tensorboard
except Exception:
    import torch.utils as _tu
    _tb = types.ModuleType("torch.utils.tensorboard")
    _tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = _tb
    _tu.tensorboard = _tb
import open3d.ml as _ml3d
import open3d.ml.torch as ml3d
import ml3d as ref_pkg
assert os.path.abspath(ref_pkg.__file__).startswith(%(ref)r), ref_pkg.__file__
Model = _ml3d.utils.get_module("model", "PointRCNN", "torch")
assert Model.__module__ == "ml3d.torch.models.point_rcnn", Model.__module__          # the checkout's own class
assert ml3d.models.PointRCNN is Model
import ml3d_amd.torch.models as native
assert native.PointRCNN is not Model and native.PointRCNN.__module__.startswith("ml3d_amd.")
assert _ml3d.utils.get_module("model", "PVCNN", "torch").__module__.startswith("ml3d_amd.")
print("REGISTRY OK")
'''

REF = os.environ.get("ML3D_REFERENCE_ROOT", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "ml3d")), reason="needs the reference checkout (absent on the GPU box)")
def test_the_registry_resolves_pointrcnn_to_the_reference_class():
    import subprocess
    import sys
    pkg = os.path.join(ROOT, "open3d-ml_amd")
    env = dict(os.environ, OPEN3D_ML_ROOT=REF, PYTHONPATH=os.pathsep.join([pkg, os.path.join(ROOT, "tests", "stubs")]))
    r = subprocess.run([sys.executable, "-c", _REGISTRY % {"ref": os.path.abspath(REF)}], env=env, cwd="/tmp", capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "REGISTRY OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
