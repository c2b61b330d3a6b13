"""CPU: the host side of the PointTransformer extension -- ABI list and version, the no-CPU-fallback refusals, the batcher, the
model's argument checks, the ``open3d`` shim's op list and the data path (``transform`` / ``inference_end``) against numpy
restatements.  Cases that need a model instance run against the host emulator in their own interpreter
(tests/emu_runtime.py), like tests/test_emulated_api.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ml3d_fps_workspace_bytes", "ml3d_furthest_point_sampling", "ml3d_pt_attention", "ml3d_pt_transition_down",
               "ml3d_pt_interpolate")
STILL_INERT = ("reduce_subarrays_sum", "roi_pool", "three_nn", "three_interpolate", "three_interpolate_grad", "ball_query",
               "trilinear_devoxelize_forward", "trilinear_devoxelize_backward", "continuous_conv", "sparse_conv",
               "sparse_conv_transpose", "invert_neighbors_list", "build_spatial_hash_table")

_PRELUDE = r'''
import os, sys, json
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import emu_runtime
emu_runtime.install("ml3d")
import pt_ref
from ml3d.torch.models import PointTransformer
from ml3d.torch.dataloaders import PointTransformerBatch
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=900,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


needs_emu = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")


def test_abi_lists_the_new_symbols_at_version_13():
    from ml3d import _abi
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    assert _abi.ABI_VERSION == 13 and re.search(r"#define ML3D_ABI_VERSION 13\b", header)
    for s in NEW_SYMBOLS:
        assert s in _abi.SYMBOLS and re.search(r"\b%s\(" % s, header), s


def test_cpu_tensors_are_refused():
    from ml3d import ops
    p = torch.zeros(64, 3)
    i = torch.zeros(64, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.furthest_point_sampling(p, [0, 64], [0, 16])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pt_attention(torch.zeros(64, 96), p, i, {k: torch.zeros(1) for k in ops.pointtransformer.ATTENTION_KEYS})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pt_transition_down(torch.zeros(64, 32), p, i[:16, 0].contiguous(), i[:16], torch.zeros(32, 64), torch.zeros(3, 64),
                               torch.zeros(64), torch.zeros(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pt_interpolate(torch.zeros(64, 32), torch.zeros(16, 32), i[:, :3].contiguous(), torch.zeros(64, 3))
    if not torch.cuda.is_available():
        from ml3d.torch.models import PointTransformer
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            PointTransformer(device="cpu")


def test_batch_class_and_batcher_dispatch():
    from ml3d.torch.dataloaders import ConcatBatcher, PointTransformerBatch
    rng = np.random.default_rng(0)
    items = [{"data": dict(point=torch.from_numpy(rng.random((n, 3), dtype=np.float32)),
                           feat=torch.from_numpy(rng.random((n, 3), dtype=np.float32)),
                           label=torch.from_numpy(rng.integers(0, 13, n)))} for n in (5000, 4100, 4096)]
    b = ConcatBatcher("cpu", model="PointTransformer").collate_fn(items)
    assert set(b) == {"data", "attr"} and isinstance(b["data"], PointTransformerBatch)
    b = b["data"]
    assert b.point.shape == (13196, 3) and b.feat.shape == (13196, 3) and b.label.shape == (13196,)
    assert b.point.dtype == torch.float32 and b.label.dtype == torch.int64 and b.row_splits.dtype == torch.int64
    assert b.row_splits.tolist() == [0, 5000, 9100, 13196] and b.row_splits_host.tolist() == [0, 5000, 9100, 13196]
    assert torch.equal(b.point[5000:9100], items[1]["data"]["point"]) and b.to("cpu") is b
    with pytest.raises(Exception, match="outside the hot path"):
        ConcatBatcher("cpu", model="PVCNN").collate_fn(items)


def test_shim_op_list():
    import open3d.ml.torch as mlt
    for name in STILL_INERT:
        with pytest.raises(NotImplementedError, match="outside this repository's scope"):
            getattr(mlt.ops, name)()
    fps = mlt.ops.furthest_point_sampling
    assert fps.__module__ == "open3d.ml.torch.ops" and fps.__doc__ and "canonical order" in fps.__doc__
    try:                                      # live: with a GPU it samples, without one it fails loudly -- never "inert"
        out = fps(torch.from_numpy(np.random.default_rng(0).random((2, 64, 3), dtype=np.float32)), torch.tensor(16))
        assert out.shape == (2, 16) and out.dtype == torch.int32 and int(out.max()) < 64 and out[:, 0].tolist() == [0, 0]
    except NotImplementedError:
        raise
    except RuntimeError as e:
        assert not torch.cuda.is_available() and re.search("no CPU implementation|no GPU|MI355X", str(e))


@needs_emu
def test_model_argument_checks():
    _run(r'''
m = PointTransformer(blocks=[1, 1, 1, 1, 1], device="cpu")
assert not m.training
def batch(sizes):
    pts, feat, rs = pt_ref.make_batch_arrays(range(len(sizes)), sizes)
    return PointTransformerBatch([{"data": dict(point=pts[rs[i]:rs[i + 1]], feat=feat[rs[i]:rs[i + 1]],
                                                label=np.zeros(sizes[i], np.int64))} for i in range(len(sizes))])
try:
    m(batch([4096, 4095]))
    raise SystemExit("a 4095-point item was accepted")
except ValueError as e:
    assert "item 1" in str(e) and "4095" in str(e) and "4096" in str(e), e
m.train()
try:
    m(batch([4096]))
    raise SystemExit("a training forward was accepted")
except NotImplementedError as e:
    assert "inference only" in str(e)
m.eval()
out = m(batch([4096]))
assert out.shape == (4096, 13) and bool(torch.isfinite(out).all())
# the pack is built once and dropped by whatever changes the parameters
pk = m.packed_params()
assert m.packed_params() is pk
m.load_state_dict(m.state_dict())
assert m._packed is None
''')


@needs_emu
def test_data_path_against_numpy():
    _run(r'''
m = PointTransformer(blocks=[1, 1, 1, 1, 1], num_classes=5, voxel_size=0.25, max_voxels=300, device="cpu")
rng = np.random.default_rng(5)
raw = (pt_ref.room(9, 6000) + np.float32([10, -3, 2])).astype(np.float32)
colour = (rng.random((6000, 3)) * 255).astype(np.float32)
data = dict(point=raw, feat=colour, label=rng.integers(0, 5, 6000).astype(np.int32))
pre = m.preprocess(dict(data), {"split": "test"})
sub = pre["point"]
assert sub.dtype == np.float32 and 300 < len(sub) < 6000 and pre["feat"].shape == (len(sub), 3) and pre["label"].shape == (len(sub),)
assert sub.min() >= -1e-3                                  # the cloud's minimum corner was moved to the origin first
shifted = raw - raw.min(0)
d = ((shifted[:, None, :].astype(np.float64) - sub[None, :, :].astype(np.float64)) ** 2).sum(2)
near = d.argmin(1)
assert pre["proj_inds"].dtype == np.int32 and pre["proj_inds"].shape == (6000,)
assert np.allclose(d[np.arange(6000), pre["proj_inds"]], d[np.arange(6000), near], rtol=1e-5, atol=1e-9)
# transform, test split: centre on the bounding-box middle, feat / 255, no crop
t = m.transform(dict(pre), {"split": "test"})
want = sub - (sub.min(0) + sub.max(0)) / 2.0
assert t["point"].dtype == torch.float32 and np.allclose(t["point"].numpy(), want, atol=1e-6)
assert np.allclose(t["feat"].numpy(), pre["feat"] / 255.0, atol=1e-7) and t["label"].dtype == torch.int64
assert np.array_equal(t["proj_inds"], pre["proj_inds"])
# validation split: the max_voxels nearest points of the middle point
v = m.transform(dict(pre), {"split": "validation"})
keep = np.argsort(np.sum(np.square(sub - sub[len(sub) // 2]), 1))[:300]
assert v["point"].shape == (300, 3) and np.array_equal(v["label"].numpy(), pre["label"][keep])
cp = sub[keep]
assert np.allclose(v["point"].numpy(), cp - (cp.min(0) + cp.max(0)) / 2.0, atol=1e-6)
try:
    m.transform(dict(pre), {"split": "training"})
    raise SystemExit("training transform accepted")
except NotImplementedError:
    pass
# inference_begin / inference_preprocess / inference_end: one label and one score row per ORIGINAL point
m.inference_begin(dict(data))
inp = m.inference_preprocess()
n_sub = inp["point"].shape[0]
logits = torch.from_numpy(rng.standard_normal((n_sub, 5)).astype(np.float32))
res = m.inference_end(None, logits)
e = np.exp(logits.numpy() - logits.numpy().max(1, keepdims=True))
probs = (e / e.sum(1, keepdims=True))[inp["proj_inds"]]
assert res["predict_labels"].shape == (6000,) and res["predict_scores"].shape == (6000, 5)
assert np.array_equal(res["predict_labels"], probs.argmax(1)) and np.allclose(res["predict_scores"], probs, atol=1e-6)
assert np.allclose(m.update_probs(None, logits, None), e / e.sum(1, keepdims=True), atol=1e-6)
b = m.make_batch(inp)
assert b.point.shape == (n_sub, 3) and b.row_splits.tolist() == [0, n_sub]
''')
