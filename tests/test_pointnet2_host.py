"""CPU: the host side of the PointNet++ backbone -- ABI list and version, argument validation before any HIP call, the
no-CPU-fallback refusals, the configurations ``Pointnet2MSG`` does not take, and the ``open3d`` shim, whose ``ball_query`` /
``three_nn`` / ``three_interpolate`` / ``roi_pool`` stay inert (the native class calls ``ml3d.ops`` directly).  The case that needs
a model instance runs against the host emulator in its own interpreter, like tests/test_pointtransformer_host.py."""
import os
import re
import subprocess
import sys

import pytest
import torch

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ml3d_ball_query", "ml3d_pn2_sa_fused_supported", "ml3d_pn2_sa_mlp_max", "ml3d_pn2_group_rows", "ml3d_pn2_interpolate")
SHIM_INERT = ("ball_query", "three_nn", "three_interpolate", "roi_pool")
SA2 = dict(npoints=[8, 4], radius=[[0.5], [1.0]], nsample=[[16], [16]], mlps=[[[16, 16, 32]], [[32, 32, 64]]])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    from ml3d import _abi
    ge.build()
    return _abi.get()


def test_abi_lists_the_new_symbols_at_version_13(built):
    from ml3d import _abi
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    assert _abi.ABI_VERSION == 13 and re.search(r"#define ML3D_ABI_VERSION 13\b", header) and built.ml3d_abi_version() == 13
    for s in NEW_SYMBOLS:
        assert s in _abi.SYMBOLS and re.search(r"\b%s\(" % s, header) and hasattr(built, s), s


def test_arguments_are_validated_before_any_hip_call(built):
    """(no GPU here: an entry that launched anything would not return these codes)"""
    import ctypes as C
    import numpy as np
    r, k = np.float32([0.5]), np.int32([16])
    one = (C.c_void_p * 1)(C.c_void_p(64))
    bq = lambda scales, n, r_, k_: built.ml3d_ball_query(64, 64, 1, n, 4, scales, r_.ctypes.data, k_.ctypes.data, one, None)   # noqa: E731
    assert bq(0, 10, r, k) == -1 and bq(5, 10, r, k) == -1 and bq(1, 0, r, k) == -1
    assert bq(1, 10, np.float32([-1.0]), k) == -1 and bq(1, 10, r, np.int32([0])) == -1 and bq(1, 1 << 31, r, k) == -1
    assert built.ml3d_ball_query(64, 64, 0, 10, 4, 1, r.ctypes.data, k.ctypes.data, one, None) == 0          # an empty batch
    sa = lambda ns, c1, c2, c3, ldy=256: built.ml3d_pn2_sa_mlp_max(64, ldy, 64, 64, 64, 1, 10, 4, ns, c1, c2, c3, 64, 64, 64, 64, 64, 64, None, 512, None)   # noqa: E731
    assert sa(16, 16, 16, 32, ldy=8) == -1 and sa(16, 16, 16, 32) == -1                                      # ldy < c1; out == NULL
    assert sa(8, 16, 16, 32) == -4 and sa(64, 16, 16, 32) == -4 and sa(16, 130, 16, 32) == -4 and sa(16, 16, 16, 48) == -4
    assert sa(32, 128, 196, 256) == -4 and sa(16, 256, 256, 512) == -4 and sa(32, 15, 16, 32) == -4
    for ns in (16, 32):                                       # levels 1 and 2 of the KITTI backbone run on the fused kernel
        for w in ((16, 16, 32), (32, 32, 64), (64, 64, 128), (64, 96, 128)):
            assert built.ml3d_pn2_sa_fused_supported(ns, *w) == 1, (ns, w)
        for w in ((128, 196, 256), (256, 256, 512), (256, 384, 512)):
            assert built.ml3d_pn2_sa_fused_supported(ns, *w) == 0, (ns, w)
    assert built.ml3d_pn2_group_rows(64, 8, 64, 64, 64, 1, 10, 4, 16, 16, 64, 64, 64, 16, None) == -1         # ldy < c1
    assert built.ml3d_pn2_group_rows(64, 16, 64, 64, 64, 1, 0, 4, 16, 16, 64, 64, 64, 16, None) == -1         # centres without points
    assert built.ml3d_pn2_group_rows(None, 0, None, 64, 64, 1, 10, 4, 16, 16, 64, 64, 64, 16, None) == -1     # no points
    ip = lambda mk, d2, w, c=8: built.ml3d_pn2_interpolate(64, 8, 1, mk, 64, d2, w, 10, c, 64, 8, None)       # noqa: E731
    assert ip(2, 64, None) == -1 and ip(5, None, None) == -1 and ip(5, 64, 64) == -1 and ip(5, 64, None, c=9) == -1


def test_cpu_tensors_are_refused():
    from ml3d import ops
    from ml3d.torch.modules import Pointnet2MSG
    xyz, ctr = torch.zeros(1, 64, 3), torch.zeros(1, 4, 3)
    idx, w = torch.zeros(1, 64, 3, dtype=torch.int32), torch.zeros(1, 64, 3)
    for call in (lambda: ops.ball_query(xyz, ctr, 0.5, 16), lambda: ops.ball_query(xyz, ctr, [0.5, 1.0], [16, 32]),
                 lambda: ops.three_nn(xyz, ctr), lambda: ops.three_interpolate(torch.zeros(1, 8, 4), idx, w),
                 lambda: ops.pn2_interpolate(torch.zeros(4, 8), 1, idx[0], w[0]), lambda: Pointnet2MSG(3, True, SA2, [], device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_unsupported_configurations_are_refused():
    """(refused while the configuration is read, before any parameter is placed on a device)"""
    from ml3d.torch.modules import Pointnet2MSG
    bad = (dict(SA2, npoints=[8, -1]), dict(SA2, npoints=[8, None]), dict(SA2, radius=[0.5, 1.0], nsample=[16, 16]),
           dict(SA2, mlps=[[[16, 32]], [[32, 32, 64]]]), dict(SA2, radius=[[0.1] * 5, [1.0]], nsample=[[4] * 5, [16]],
                                                              mlps=[[[16, 16, 32]] * 5, [[32, 32, 64]]]))
    for cfg in bad:
        with pytest.raises(NotImplementedError, match="unsupported|supported"):
            Pointnet2MSG(3, True, cfg, [])
    for kw in (dict(use_xyz=False), dict(pool_method="avg_pool"), dict(instance_norm=torch.nn.InstanceNorm2d)):
        with pytest.raises(NotImplementedError, match="unsupported"):
            Pointnet2MSG(**dict(dict(in_channels=3, use_xyz=True, SA_config=SA2, fp_mlps=[]), **kw))
    with pytest.raises(ValueError):
        Pointnet2MSG(-1, True, SA2, [])


def test_shim_names_remain_inert():
    import open3d.ml.torch as mlt
    for name in SHIM_INERT:
        with pytest.raises(NotImplementedError, match="outside this repository's scope"):
            getattr(mlt.ops, name)()


@pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")
def test_model_instance_is_inference_only_and_checks_its_input():
    emu.lib()
    body = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import emu_runtime
emu_runtime.install("ml3d")
from ml3d.torch.modules import Pointnet2MSG
m = Pointnet2MSG(3, True, %(sa)r, [[16, 16], [32, 32]], device="cpu")
assert not m.training and m.eval() is m
try:
    m.train()
    raise SystemExit(".train() accepted")
except NotImplementedError as e:
    assert "inference only" in str(e)
for shape in ((1, 64, 5), (64, 6)):
    try:
        m(torch.zeros(shape))
        raise SystemExit("a pointcloud of shape %%s was accepted" %% (shape,))
    except ValueError as e:
        assert "[B, N, 6]" in str(e)
try:
    m(torch.zeros(1, 6, 6))
    raise SystemExit("6 points for 8 samples accepted")
except ValueError as e:
    assert "samples 8 of 6" in str(e)
xyz, feat = m(torch.rand(2, 64, 6))
assert tuple(xyz.shape) == (2, 64, 3) and tuple(feat.shape) == (2, 16, 64) and bool(torch.isfinite(feat).all())
''' % dict(root=ROOT, sa=SA2)
    r = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
