"""GPU: the PointTransformer extension on the MI355X -- furthest point sampling EXACT against the numpy restatement of its
contract (tests/pt_ref.py) on clouds whose float32 sequences contain exact ties, both goldens of the REAL reference forward
(tools/gen_golden_pointtransformer.py: FPS indices and k-NN checksums exact, logits within the project's rule
``max(1e-4, 4.4e-6 * logit_scale)``), the fused path against the torch formulation (``ML3D_PT_OPS=torch``), a forward without
device->host synchronisation, and the data path.  The measured deviations are appended to the per-YAML parity record of
tests/test_gpu_configs.py (its ``record``, same file, same format).

Measured on an MI355X: max |dlogit| 4.29e-6 (small, logit scale 8.64) and 6.2e-6 (s3dis, logit scale 9.18) against the
reference, label agreement 1.0 on both; fused against torch formulation 8.11e-6 on 4 x 40 960 points."""
import json
import os

import numpy as np
import pytest
import torch

import pt_ref
import synth_data
from test_gpu_configs import record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def tol_for(scale, base=1e-4):
    """The project's rule (tests/test_gpu_configs.py:25-31), unchanged."""
    return max(base, 4.4e-6 * float(scale))


def _batch(pts, feat, rs):
    from ml3d.torch.dataloaders import PointTransformerBatch
    items = [{"data": dict(point=pts[rs[i]:rs[i + 1]], feat=feat[rs[i]:rs[i + 1]], label=np.zeros(rs[i + 1] - rs[i], np.int64))}
             for i in range(len(rs) - 1)]
    return PointTransformerBatch(items).to(DEV)


def _model(mcfg, seed):
    from ml3d.torch.models import PointTransformer
    m = PointTransformer(**mcfg, device=DEV)
    m.load_state_dict(pt_ref.make_state_dict(mcfg, seed))
    return m.eval()


@pytest.fixture(autouse=True)
def _fused_by_default(monkeypatch):
    monkeypatch.delenv("ML3D_PT_OPS", raising=False)


def test_fps_exact_including_float32_ties():
    from ml3d import ops
    clouds = [synth_data.toronto3d_sphere(0, 50000), synth_data.toronto3d_sphere(1, 24000), pt_ref.room(7, 50000)]
    refs, n_ties = [], 0
    for c in clouds:
        r, ties = pt_ref.fps_item(c, len(c) // 4, return_ties=True)
        refs.append(r)
        n_ties += len(ties)
    assert n_ties >= 4                       # picks 1 124 / 3 586 of the first sphere, 4 069 / 5 701 of the second
    for c, r in zip(clouds, refs):
        out = ops.furthest_point_sampling(torch.from_numpy(c).to(DEV), [0, len(c)], [0, len(c) // 4])
        assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), r), int(np.argmax(out.cpu().numpy() != r))
    rs = np.concatenate(([0], np.cumsum([len(c) for c in clouds])))
    nrs = np.concatenate(([0], np.cumsum([len(c) // 4 for c in clouds])))
    out = ops.furthest_point_sampling(torch.from_numpy(np.concatenate(clouds)).to(DEV), torch.from_numpy(rs).to(DEV),
                                      torch.from_numpy(nrs).to(DEV)).cpu().numpy()
    assert np.array_equal(out, np.concatenate([r + np.int32(o) for r, o in zip(refs, rs[:-1])]))
    # an item longer than the register-resident classes (65 536 points): the workspace form, same order
    big = pt_ref.room(8, 70000)
    out = ops.furthest_point_sampling(torch.from_numpy(big).to(DEV), [0, 70000], [0, 3000]).cpu().numpy()
    assert np.array_equal(out, pt_ref.fps_item(big, 3000))


@pytest.mark.parametrize("name", ["pointtransformer_small", "pointtransformer_s3dis"])
def test_golden_of_the_reference_forward(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    m = _model(mcfg, int(g["weights_seed"]))
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g["state_shapes"]]
    pts, feat, rs = pt_ref.make_batch_arrays(g["cloud_seeds"], g["sizes"])
    assert abs(pts.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    out = m(_batch(pts, feat, rs))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    used = m.last_indices
    for l in range(4):
        assert np.array_equal(used["fps"][l].cpu().numpy(), g["fps%d" % (l + 1)]), l
        assert pt_ref.knn_checksum(used["knn_down"][l].cpu().numpy()) == int(g["knn_down%d" % (l + 1)]), l
        assert pt_ref.knn_checksum(used["knn_up"][l].cpu().numpy()) == int(g["knn_up%d" % l]), l
    for l in range(5):
        assert pt_ref.knn_checksum(used["knn_self"][l].cpu().numpy()) == int(g["knn_self%d" % l]), l
    stride, tol = int(g["logit_stride"]), tol_for(g["logit_scale"])
    err = float(np.abs(out[::stride] - g["logits"]).max())
    labels = out.argmax(1)
    bad = np.nonzero(labels != g["labels"])[0]
    srt = np.sort(out[bad], axis=1)
    margins = [float(x) for x in (srt[:, -1] - srt[:, -2])]
    agree = float(1.0 - len(bad) / out.shape[0])
    print("%s: max|dlogit| = %.3g (tol %.3g, logit scale %.2f), label agreement %.6f, flipped margins %s" %
          (name, err, tol, float(g["logit_scale"]), agree, margins[:10]))
    record(name, family="pointtransformer", max_abs_delta=err, tol=tol, logit_scale=float(g["logit_scale"]),
           ref_abs_max=float(np.abs(g["logits"]).max()), label_agreement=agree, flipped_margins=margins[:50],
           points=int(out.shape[0]))
    assert out.shape == (len(pts), int(mcfg["num_classes"])) and err <= tol
    assert all(x <= 2 * tol for x in margins), margins[:10]      # a differing label only where OUR top two are that close


def test_fused_path_against_the_torch_formulation(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, "pointtransformer_s3dis.npz"))
    mcfg = json.loads(str(g["model_json"]))
    m = _model(mcfg, int(g["weights_seed"]))
    pts, feat, rs = pt_ref.make_batch_arrays([31, 32, 33, 34], [40960] * 4)
    b = _batch(pts, feat, rs)
    fused = m(b).cpu().numpy()
    fused_idx = [t.cpu().numpy() for t in m.last_indices["fps"]]
    monkeypatch.setenv("ML3D_PT_OPS", "torch")
    plain = m(b).cpu().numpy()
    assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(fused_idx, m.last_indices["fps"]))
    scale = float(np.abs(plain).max())
    err = float(np.abs(fused - plain).max())
    agree = float((fused.argmax(1) == plain.argmax(1)).mean())
    print("fused vs torch on 4 x 40 960 points: max|dlogit| = %.3g (tol %.3g, logit scale %.2f), label agreement %.6f" %
          (err, tol_for(scale), scale, agree))
    record("pointtransformer_fused_vs_torch", family="pointtransformer", max_abs_delta=err, tol=tol_for(scale), logit_scale=scale,
           ref_abs_max=scale, label_agreement=agree, flipped_margins=[], points=int(fused.shape[0]))
    assert fused.shape == (163840, 13) and err <= tol_for(scale)


def test_forward_makes_no_device_to_host_synchronisation(golden_dir):
    g = np.load(os.path.join(golden_dir, "pointtransformer_small.npz"))
    m = _model(json.loads(str(g["model_json"])), int(g["weights_seed"]))
    b = _batch(*pt_ref.make_batch_arrays(g["cloud_seeds"], g["sizes"]))
    first = m(b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = m(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(first, second)


def test_data_path_returns_one_label_per_original_point():
    from oracle import ops as oops
    from ml3d.torch.models import PointTransformer
    m = PointTransformer(blocks=[2, 2, 2, 2, 2], in_channels=6, num_classes=13, voxel_size=0.04, device=DEV)
    m.load_state_dict(pt_ref.make_state_dict(m.cfg, 2026))
    m.eval()
    n = 120000
    raw = (pt_ref.room(41, n) + np.float32([12.0, -7.0, 1.5])).astype(np.float32)
    data = dict(point=raw, feat=(pt_ref.colours(41, n) * 255).astype(np.float32), label=np.zeros(n, np.int32))
    m.inference_begin(dict(data))
    inp = m.inference_preprocess()
    sub = m.preprocess(dict(data), {"split": "test"})["point"]
    assert 4096 <= len(sub) < n and inp["point"].shape == (len(sub), 3)
    want = oops.knn_search(sub, raw - raw.min(0), 1, brute=True).reshape(-1)
    assert inp["proj_inds"].dtype == np.int32 and np.array_equal(inp["proj_inds"], want)
    logits = m(m.make_batch(inp))
    res = m.inference_end(inp, logits)
    lg = logits.cpu().numpy().astype(np.float32)
    e = np.exp(lg - lg.max(1, keepdims=True))
    probs = (e / e.sum(1, keepdims=True))[want]
    assert res["predict_labels"].shape == (n,) and res["predict_scores"].shape == (n, 13)
    assert np.array_equal(res["predict_labels"], probs.argmax(1))
    assert np.allclose(res["predict_scores"], probs, atol=1e-6)
