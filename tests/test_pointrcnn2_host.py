"""CPU, no kernel: the host side of ``ml3d_roi_pool`` (PointRCNN stage 2, the pooling) -- the entry point is declared and bound
with the ABI still 13 and without a workspace-size function, the wrapper refuses CPU tensors with the project's message and checks
its arguments before any call, and the ``open3d`` shim's own ``roi_pool`` stays inert (the native op is ``ml3d.ops.roi_pool``)."""
import os
import re

import pytest
import torch

from ml3d import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    assert "#define ML3D_ABI_VERSION 13" in header
    assert re.search(r"\bint ml3d_roi_pool\(", header) and "ml3d_roi_pool" in _abi.SYMBOLS
    assert not [s for s in _abi.SYMBOLS if "roi_pool" in s and "_workspace_bytes" in s]
    assert "UNPINNED against the open3d wheel" in header[header.index("ml3d_roi_pool produces"):]

    class Fn:
        pass

    class Lib:
        def __getattr__(self, name):
            f = Fn()
            object.__setattr__(self, name, f)
            return f

    lib = _abi.bind(Lib())
    assert len(lib.ml3d_roi_pool.argtypes) == 16
    declared = header[header.index("int ml3d_roi_pool("):]
    assert declared[:declared.index(");")].count(",") == 15


def test_the_op_is_exported_and_refuses_cpu_tensors():
    from ml3d import ops
    from ml3d.ops import pointrcnn
    assert ops.roi_pool is pointrcnn.roi_pool and "roi_pool" in pointrcnn.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.roi_pool(torch.zeros((1, 8, 3)), torch.zeros((8, 4)), torch.zeros((1, 8)), torch.zeros((1, 2, 7)), 16)


def test_argument_checks_raise_before_the_call(monkeypatch):
    from ml3d import ops
    from ml3d.ops import _gates
    monkeypatch.setattr(_gates, "_need_gpu", lambda *t: None)
    monkeypatch.setattr(_abi, "get", lambda: None)             # (a call into the library would be an AttributeError)
    xyz, feat, sc, rois = torch.zeros((2, 8, 3)), torch.zeros((16, 4)), torch.zeros((2, 8)), torch.zeros((2, 3, 7))
    for bad in (lambda: ops.roi_pool(xyz, feat, sc, rois, 0),
                lambda: ops.roi_pool(xyz, feat, sc, rois, -4),
                lambda: ops.roi_pool(xyz, feat[:1].expand(16, 4), sc, rois, 8),
                lambda: ops.roi_pool(xyz, feat.t().contiguous().t(), sc, rois, 8),
                lambda: ops.roi_pool(xyz, feat[:15], sc, rois, 8),
                lambda: ops.roi_pool(xyz[..., :2], feat, sc, rois, 8),
                lambda: ops.roi_pool(xyz, feat, sc[:1], rois, 8),
                lambda: ops.roi_pool(xyz, feat, sc, rois[..., :6], 8),
                lambda: ops.roi_pool(xyz, feat, sc, rois[:1], 8),
                lambda: ops.roi_pool(xyz.double(), feat, sc, rois, 8),
                lambda: ops.roi_pool(xyz, feat, sc, rois, 2 ** 29),
                lambda: ops.roi_pool(xyz, feat, sc, rois, 8, out=(torch.zeros((6, 8, 9)),) * 3)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            bad()
    with pytest.raises(ValueError, match="cuda device"):         # well-formed arguments pass every check and reach the device scope
        ops.roi_pool(xyz, feat, sc, rois, 8)


def test_the_shim_keeps_its_own_roi_pool_inert():
    src = open(os.path.join(ROOT, "open3d-ml_amd", "open3d", "ml", "torch", "__init__.py")).read()
    registered = src[src.index("for cls in ("):src.index("MODEL._register_module(cls")]
    assert "PointRCNN" not in registered
    shim_ops = open(os.path.join(ROOT, "open3d-ml_amd", "open3d", "ml", "torch", "ops.py")).read()
    inert = shim_ops[shim_ops.index("for _n in ("):shim_ops.index("globals()[_n] = _out_of_scope(_n)")]
    assert '"roi_pool"' in inert and "def roi_pool" not in shim_ops
