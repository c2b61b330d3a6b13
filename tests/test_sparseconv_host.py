"""CPU: the host side of the SparseConvUnet extension -- ABI bookkeeping, the "no CPU fallback" gates, ``ConcatBatcher``'s
dispatch to ``SparseConvUnetBatch``, the dictionary-lookup rulebooks of tests/scn_ref.py against a brute-force O(M^2)
construction, the data path against numpy restatements under a seeded generator, and the state-dict layout against the one
recorded from the reference.  (The kernels run in tests/test_emulated_sparseconv.py and tests/test_gpu_sparseconv.py.)"""
import json
import os
import re

import numpy as np
import pytest
import torch

import pt_ref
import scn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ml3d_scn_build_workspace_bytes", "ml3d_scn_build", "ml3d_sparse_conv_bf16x3", "ml3d_scn_bn_relu")


def _host_model(**cfg):
    """The native class on the meta / cpu device: parameters and host methods only (the device gate is lifted for the test)."""
    from ml3d import _abi
    from ml3d.torch.models import sparseconvunet as native
    gate = _abi.require_gpu
    _abi.require_gpu = lambda device, what: torch.device(device)
    try:
        return native.SparseConvUnet(**cfg)
    finally:
        _abi.require_gpu = gate


def test_abi_lists_the_new_symbols_at_the_unchanged_version():
    from ml3d import _abi
    header = open(os.path.join(ROOT, "include", "ml3d_hip.h")).read()
    ver = int(re.search(r"#define\s+ML3D_ABI_VERSION\s+(\d+)", header).group(1))
    assert _abi.ABI_VERSION == ver == 13          # new symbols only: no signature or struct changed
    for s in NEW_SYMBOLS:
        assert s in _abi.SYMBOLS and re.search(r"\b%s\(" % s, header), s
    assert "UNPINNED" in header


def test_cpu_tensors_are_refused():
    from ml3d import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scn_build(z(64, 3), z(64, 3), [0, 64])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sparse_conv(z(64, 32), z(64, 27, dtype=torch.int32), z(16, dtype=torch.uint8), 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scn_bn_relu(z(64, 32), z(32), z(32))
    if not torch.cuda.is_available():
        from ml3d.torch.models import SparseConvUnet
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SparseConvUnet(device="cpu")


def test_batch_class_and_batcher_dispatch():
    from ml3d.torch.dataloaders import ConcatBatcher, SparseConvUnetBatch
    rng = np.random.default_rng(0)
    items = [{"data": dict(point=torch.from_numpy(rng.random((n, 3), dtype=np.float32)),
                           feat=torch.from_numpy(rng.random((n, 3), dtype=np.float32)),
                           label=torch.from_numpy(rng.integers(0, 20, n).astype(np.int32)))} for n in (500, 410, 96)]
    b = ConcatBatcher("cpu", model="SparseConvUnet").collate_fn(items)
    assert set(b) == {"data", "attr"} and isinstance(b["data"], SparseConvUnetBatch)
    b = b["data"]
    assert b.batch_lengths == [500, 410, 96] and len(b.point) == len(b.feat) == len(b.label) == 3
    assert all(torch.equal(b.point[i], items[i]["data"]["point"]) and torch.equal(b.feat[i], items[i]["data"]["feat"]) and
               torch.equal(b.label[i], items[i]["data"]["label"]) for i in range(3))
    assert b.to("cpu") is b
    parts = SparseConvUnetBatch.scatter(b, 2)
    assert [p.batch_lengths for p in parts] == [[500, 410], [96]] and torch.equal(parts[1].point[0], b.point[2])
    assert [p.batch_lengths for p in SparseConvUnetBatch.scatter(b, 8)] == [[500], [410], [96]]


def test_rulebooks_agree_with_a_brute_force_construction():
    rng = np.random.default_rng(3)
    c = np.unique(np.concatenate([rng.integers(0, 2, (260, 1)), rng.integers(40, 47, (260, 3))], 1), axis=0)[:200]
    pts = (c[:, 1:] + 0.5).astype(np.float32)
    order = np.argsort(c[:, 0], kind="stable")
    pts, item = pts[order], c[order, 0]
    rs = np.asarray([0, int((item == 0).sum()), len(pts)], np.int64)
    ref = scn_ref.build(pts, np.zeros((len(pts), 3), np.float32), rs, levels=3)
    assert ref["counts"][0] == 200 and np.array_equal(ref["coords"][0], c[np.lexsort(c.T[::-1])])
    for l in range(3):
        assert np.array_equal(ref["nbr27"][l], scn_ref.brute_force_nbr27(ref["coords"][l])), l
        assert (ref["nbr27"][l][:, 13] == np.arange(ref["counts"][l])).all()
    for l in range(2):
        parent, child8 = scn_ref.brute_force_children(ref["coords"][l], ref["coords"][l + 1])
        assert np.array_equal(parent, ref["parent"][l]) and np.array_equal(child8, ref["child8"][l + 1]), l
        rows = np.arange(ref["counts"][l])
        assert (ref["up8"][l][rows, ref["ptap"][l]] == parent).all() and ((ref["up8"][l] >= 0).sum(1) == 1).all()
    # the stand-in layers see the same neighbourhoods, per item
    one = pts[:rs[1]]
    rule = scn_ref._rule(torch.from_numpy(one), torch.from_numpy(one), "sub")
    assert np.array_equal(rule, ref["nbr27"][0][:rs[1]])


def test_data_path_against_numpy():
    m = _host_model(multiplier=16, voxel_size=0.04, seed=11, device="cpu")
    assert not m.training and m.cfg.grid_size == 4096 and m.cfg.batcher == "ConcatBatcher"
    rng = np.random.default_rng(5)
    raw = (pt_ref.room(9, 1000) + np.float32([10, -3, 2])).astype(np.float32)
    colour = rng.random((1000, 3)).astype(np.float32)
    data = dict(point=raw, feat=colour, label=rng.integers(0, 20, 1000).astype(np.int32))
    pre = m.preprocess(dict(data), {"split": "test"})
    # the same two draws from a generator of the same seed
    g = np.random.default_rng(11)
    p = raw * np.float32(1. / 0.04)
    lo, hi = p.min(0), p.max(0)
    off = -lo + np.clip(4096 - hi + lo - 0.001, 0, None) * g.random(3) + np.clip(4096 - hi + lo + 0.001, None, 0) * g.random(3)
    p = p + off
    keep = (p.min(1) >= 0) * (p.max(1) < 4096)
    want = (p[keep].astype(np.int32) + 0.5).astype(np.float32)
    assert keep.all() and np.array_equal(pre["point"], want) and pre["point"].dtype == np.float32
    assert np.array_equal(pre["feat"], colour) and np.array_equal(pre["label"], data["label"])
    with pytest.raises(Exception, match="feature"):
        m.preprocess(dict(point=raw, label=None), {"split": "test"})
    with pytest.raises(NotImplementedError):
        m.preprocess(dict(data), {"split": "training"})
    m.inference_begin(dict(data))
    inp = m.inference_preprocess()
    assert inp["batch_lengths"] == [1000] and isinstance(inp["point"], torch.Tensor) and inp["label"].dtype == torch.int32
    logits = torch.from_numpy(rng.normal(size=(1000, 20)).astype(np.float32))
    res = m.inference_end(inp, logits)
    e = np.exp(logits.numpy() - logits.numpy().max(1, keepdims=True))
    assert np.allclose(res["predict_scores"], e / e.sum(1, keepdims=True), atol=1e-6)
    assert np.array_equal(res["predict_labels"], logits.numpy().argmax(1))
    probs, labels = m.update_probs(inp, logits, None, None)
    assert np.array_equal(labels, res["predict_labels"]) and probs.shape == (1000, 20)
    m.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(dict(point=[inp["point"]], feat=[inp["feat"]]))


@pytest.mark.parametrize("name", ["sparseconvunet_small", "sparseconvunet_scannet"])
def test_state_dict_layout_equals_the_reference(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    keys = [str(k) for k in g["state_keys"]]
    shapes = [tuple(json.loads(str(s))) for s in g["state_shapes"]]
    assert list(zip(keys, shapes)) == scn_ref.state_shapes(mcfg)
    m = _host_model(**mcfg, device="meta")
    sd = m.state_dict()
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    assert sum(k.endswith(".net.offset") for k in keys) == sum(k.endswith(".net.kernel") for k in keys)
    assert m.residual == bool(mcfg["residual_blocks"]) and m.planes[-1] == 7 * int(mcfg["multiplier"])
    # a reference-shaped checkpoint loads unchanged, and loading drops the folded parameters
    m2 = _host_model(**mcfg, device="cpu")
    m2._packed = object()
    m2.load_state_dict(scn_ref.make_state_dict(mcfg, 1))
    assert m2._packed is None
