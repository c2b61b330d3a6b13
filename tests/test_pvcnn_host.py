"""CPU: the host side of the PVCNN extension -- ABI bookkeeping, the "no CPU fallback" gates, the state-dict layout against
the one recorded from the reference (tests/golden/pvcnn_small.npz), the data path against numpy restatements and
``DefaultBatcher``'s collation of PVCNN items.  (The kernels run in tests/test_emulated_pvcnn.py and tests/test_gpu_pvcnn.py.)"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu
import pvcnn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ml3d_pvcnn_voxel_coords", "ml3d_avg_voxelize_workspace_bytes", "ml3d_avg_voxelize", "ml3d_conv3d_ndhwc_bf16x3",
               "ml3d_trilinear_devoxelize", "ml3d_segment_max_rows_workspace_bytes", "ml3d_segment_max_rows")

_PRELUDE = r'''
import os, sys, json
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import emu_runtime
emu_runtime.install("ml3d")
import pt_ref, pvcnn_ref
from ml3d.torch.models import PVCNN
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=900,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


needs_emu = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")


def test_abi_lists_the_new_symbols_at_the_unchanged_version():
    from ml3d import _abi
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    ver = int(re.search(r"#define\s+ML3D_ABI_VERSION\s+(\d+)", header).group(1))
    assert _abi.ABI_VERSION == ver == 13          # new symbols only: no signature or struct changed
    for s in NEW_SYMBOLS:
        assert s in _abi.SYMBOLS and re.search(r"\b%s\(" % s, header), s


def test_cpu_tensors_are_refused():
    from ml3d import ops
    z = torch.zeros
    idx = z(64, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pvcnn_voxel_coords(z(2, 3, 32), [4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.avg_voxelize(z(64, 32), idx, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv3d_ndhwc(z(2, 4, 4, 4, 32), z(16, dtype=torch.uint8), z(32), 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trilinear_devoxelize(z(2, 4, 4, 4, 32), z(64, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_max_rows(z(64, 32), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_rows_bf16x3(z(64, 32), z(16, dtype=torch.uint8), 32)
    if not torch.cuda.is_available():
        from ml3d.torch.models import PVCNN
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            PVCNN(device="cpu")


@pytest.mark.parametrize("name", ["pvcnn_small", "pvcnn_s3dis"])
def test_state_dict_layout_equals_the_reference(golden_dir, name):
    """The layout recorded from the reference's module, its restatement in pvcnn_ref and the native class (constructed on the
    meta device: parameters only) agree key for key and shape for shape."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    keys = [str(k) for k in g["state_keys"]]
    shapes = [tuple(json.loads(str(s))) for s in g["state_shapes"]]
    assert list(zip(keys, shapes)) == pvcnn_ref.state_shapes(mcfg)
    from ml3d import _abi
    from ml3d.torch.models import pvcnn as native
    gate = _abi.require_gpu
    _abi.require_gpu = lambda device, what: torch.device(device)
    try:
        m = native.PVCNN(**mcfg, device="meta")
    finally:
        _abi.require_gpu = gate
    sd = m.state_dict()
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    want = dict(pvcnn_small=336 * 2, pvcnn_s3dis=1344)[name]
    assert m.concat_channels == want and m.cfg.batcher == "DefaultBatcher"


def test_default_batcher_collates_pvcnn_items():
    from ml3d.torch.dataloaders import DefaultBatcher
    point, feat = pvcnn_ref.make_inputs([1, 2, 3], 500, lattice=False)
    items = [dict(point=torch.from_numpy(point[i]), feat=torch.from_numpy(feat[i]), label=torch.zeros(500, dtype=torch.int32))
             for i in range(3)]
    b = DefaultBatcher().collate_fn(items)
    assert b["point"].shape == (3, 3, 500) and b["feat"].shape == (3, 9, 500) and b["label"].shape == (3, 500)
    assert torch.equal(b["point"][1], items[1]["point"]) and torch.equal(b["feat"][2], items[2]["feat"])
    b = DefaultBatcher().collate_fn([{"data": it, "attr": {"split": "test"}} for it in items])
    assert b["data"]["point"].shape == (3, 3, 500) and b["data"]["feat"].shape == (3, 9, 500)


@needs_emu
def test_data_path_against_numpy():
    _run(r'''
m = PVCNN(num_classes=5, num_points=700, width_multiplier=0.5, voxel_resolution_multiplier=0.25, seed=11, device="cpu")
assert not m.training and m.cfg.num_points == 700
rng = np.random.default_rng(5)
raw = (pt_ref.room(9, 1000) + np.float32([10, -3, 2])).astype(np.float32)
colour = (rng.random((1000, 3)) * 255).astype(np.float32)
data = dict(point=raw, feat=colour, label=rng.integers(0, 5, 1000).astype(np.int32))
pre = m.preprocess(dict(data), {"split": "test"})
assert pre["point"].shape == (3, 700) and pre["feat"].shape == (9, 700) and pre["label"].shape == (700,)
assert pre["point"].dtype == np.float32 and pre["feat"].dtype == np.float32
# the same draw from a generator of the same seed: num_points rows WITHOUT replacement (the cloud is larger)
choices = np.random.default_rng(11).choice(1000, 700, replace=False)
shifted = raw - raw.min(0)
assert len(set(choices.tolist())) == 700 and np.array_equal(pre["point"], shifted[choices].T)
want = np.concatenate([shifted, colour / 255.0, shifted / shifted.max(0)], 1)[choices].T
assert np.allclose(pre["feat"], want, atol=1e-7) and np.array_equal(pre["label"], data["label"][choices])
assert pre["feat"][6:].max() == 1.0 and pre["feat"][:3].min() == 0.0
# a cloud smaller than num_points is drawn WITH replacement; a missing label is zeros, a missing feat the raw points
small = m.preprocess(dict(point=raw[:300], feat=None, label=None), {"split": "test"})
assert small["point"].shape == (3, 700) and small["feat"].shape == (9, 700) and not small["label"].any()
try:
    m.preprocess(dict(data), {"split": "training"})
    raise SystemExit("the training augmentation was accepted")
except NotImplementedError:
    pass
t = m.transform(dict(pre), {"split": "test"})
assert all(torch.is_tensor(t[k]) for k in ("point", "feat", "label")) and np.array_equal(t["point"].numpy(), pre["point"])
# inference_begin / _preprocess / _end: one label and one score row per input point of the sampled cloud
m.inference_begin(dict(data))
inp = m.inference_preprocess()
assert inp["point"].shape == (3, 700) and inp["batch_lengths"] == [3]
b = m.make_batch(inp)
assert b["point"].shape == (1, 3, 700) and b["feat"].shape == (1, 9, 700)
logits = m(b)
assert logits.shape == (1, 700, 5) and bool(torch.isfinite(logits).all())
res = m.inference_end(inp, logits)
lg = logits.reshape(-1, 5).numpy()
e = np.exp(lg - lg.max(1, keepdims=True))
probs = e / e.sum(1, keepdims=True)
assert res["predict_labels"].shape == (700,) and res["predict_scores"].shape == (700, 5)
assert np.array_equal(res["predict_labels"], probs.argmax(1)) and np.allclose(res["predict_scores"], probs, atol=1e-6)
assert np.allclose(m.update_probs(None, logits, None), probs, atol=1e-6)
# the pack is built once and dropped by whatever changes the parameters
pk = m.packed_params()
assert m.packed_params() is pk
m.load_state_dict(m.state_dict())
assert m._packed is None
try:
    PVCNN(width_multiplier=0.3, device="cpu")
    raise SystemExit("a width that is no multiple of 32 was accepted")
except NotImplementedError as e:
    assert "multiple of 32" in str(e)
''')
