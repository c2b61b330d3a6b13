"""GPU: the PVCNN extension on the MI355X -- the voxel coordinates EXACT against the numpy restatement of their contract
(tests/pvcnn_ref.py), the scatter-mean, 3 x 3 x 3 convolution, trilinear gather and column maximum against direct formulas,
both goldens of the REAL reference forward (tools/gen_golden_pvcnn.py: ``stats`` bit-exact, voxel indices / checksums exact,
logits within the project's rule ``max(1e-4, 4.4e-6 * logit_scale)``), the native path against the torch formulation
(``ML3D_PVCNN_OPS=torch``) on real-valued rooms, a forward without device->host synchronisation, and the data path.  The
measured deviations are appended to the per-YAML parity record of tests/test_gpu_configs.py (its ``record``).

Tolerance of the op tests, 1e-5: the convolution sums at most 27 * 64 = 1 728 products of order 1 / sqrt(1 728) with float32
accumulation (the bf16x3 split is float32-equivalent), expected error ~ sqrt(1 728) * 6e-8 = 2.5e-6 at outputs of order 1; the
other ops add at most eight or a handful of terms."""
import json
import os

import numpy as np
import pytest
import torch

import pt_ref
import pvcnn_ref
from test_gpu_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tol_for(scale, base=1e-4):
    """The project's rule (tests/test_gpu_configs.py:25-31), unchanged."""
    return max(base, 4.4e-6 * float(scale))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _model(mcfg, seed):
    from ml3d.torch.models import PVCNN
    m = PVCNN(**mcfg, device=DEV)
    m.load_state_dict(pvcnn_ref.make_state_dict(mcfg, seed))
    return m.eval()


@pytest.fixture(autouse=True)
def _native_by_default(monkeypatch):
    monkeypatch.delenv("ML3D_PVCNN_OPS", raising=False)


def test_voxel_coords_exact():
    from ml3d import ops
    half = np.float32([[64, 0, 0], [8, 24, 16], [0, 40, -8], [-56, 0, 8], [16, -16, 16]])
    clouds = [(np.stack([pvcnn_ref.lattice_room(s, 40960).T for s in (1, 2)]), [64, 32]),
              (np.stack([pvcnn_ref.real_room(s, 5000).T + np.float32([[12.25], [-7.5], [1.5]]) for s in (3, 4, 5)]), [5, 12, 6]),
              (np.concatenate([half, -half]).T[None], [8]),                       # v exactly integral / k + 0.5 / at the maximum norm
              (np.tile(np.float32([[1.5], [-2.0], [0.25]]), (1, 200))[None], [5, 6])]      # all points coincident
    for coords, res in clouds:
        stats, vox = ops.pvcnn_voxel_coords(dev(coords), res)
        rstats, rvox = pvcnn_ref.voxel_coords(coords, res)
        assert np.array_equal(stats.cpu().numpy(), rstats)
        for r in res:
            assert np.array_equal(vox[r][0].cpu().numpy(), rvox[r][0]), r
            assert vox[r][1].dtype == torch.int32 and np.array_equal(vox[r][1].cpu().numpy(), rvox[r][1]), r
    assert np.array_equal(vox[5][1].cpu().numpy(), np.full(200, 62, np.int32))             # 2.5 -> cell 2 on every axis
    stats, vox = ops.pvcnn_voxel_coords(dev(clouds[2][0]), [8])
    assert vox[8][0].cpu().numpy()[1].tolist() == [4.5, 5.5, 5.0] and int(vox[8][1][1]) == (4 * 8 + 6) * 8 + 5


def _conv_case(rng, cin, cout):
    w5 = torch.from_numpy(rng.uniform(-1, 1, (cout, cin, 3, 3, 3)) * 2.0 / np.sqrt(27 * cin))
    cb = torch.from_numpy(rng.uniform(-1, 1, cout) / np.sqrt(27 * cin))
    gamma = torch.from_numpy(rng.uniform(0.6, 1.5, cout) * np.where(rng.random(cout) < 0.2, -1, 1))
    beta, mean, var = (torch.from_numpy(a) for a in (rng.normal(0, 0.2, cout), rng.normal(0, 0.2, cout), rng.uniform(0.5, 1.5, cout)))
    return w5, cb, gamma, beta, mean, var


def _conv_reference(x64, w5, cb, gamma, beta, mean, var):
    """float64 conv3d + BatchNorm3d(eps = 1e-4, running statistics) + LeakyReLU(0.1) on the CPU, channels-last result."""
    v = lambda t: t.view(1, -1, 1, 1, 1)      # noqa: E731
    y = torch.nn.functional.conv3d(x64, w5, cb, padding=1)
    y = (y - v(mean)) / torch.sqrt(v(var) + 1e-4) * v(gamma) + v(beta)
    return torch.nn.functional.leaky_relu(y, 0.1).permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("r,cin,cout", [(6, 9, 32), (12, 32, 32), (5, 32, 64)])
def test_ops_against_the_direct_formulas(r, cin, cout):
    from ml3d import ops
    B, N = 2, 1000
    rng = np.random.default_rng(100 * r + cin)
    coords = np.stack([pvcnn_ref.real_room(s, N).T for s in (6, 7)])
    _, vox = ops.pvcnn_voxel_coords(dev(coords), [r])
    v, idx = vox[r]
    cp = (cin + 31) // 32 * 32
    wide = dev(rng.standard_normal((B * N, cin + 8)))
    feat = wide[:, 4:4 + cin]                                   # a column slice of a wider buffer
    grid = ops.avg_voxelize(feat, idx, B, r, out_channels=cp)
    assert torch.equal(grid, ops.avg_voxelize(feat, idx, B, r, out_channels=cp))           # deterministic: the same bits
    ref = pvcnn_ref.avg_voxelize(feat.cpu().numpy(), idx.cpu().numpy(), B, r, out_channels=cp)
    e_vox = float(np.abs(grid.cpu().numpy() - ref).max())
    w5, cb, gamma, beta, mean, var = _conv_case(rng, cin, cout)
    scale = gamma / torch.sqrt(var + 1e-4)
    w, bias, _ = ops.pack_conv3d_weights(w5.to(DEV), scale.to(DEV), (beta - mean * scale).to(DEV), cb.to(DEV))
    out = ops.conv3d_ndhwc(grid, ops.pack_bf16x3(w), bias, cout, act=1, slope=0.1)
    y = _conv_reference(grid[..., :cin].cpu().double().permute(0, 4, 1, 2, 3), w5, cb, gamma, beta, mean, var)
    e_conv = float((out.cpu().double() - y).abs().max())
    buf = dev(rng.standard_normal((B * N, cout + 16)))
    sl = buf[:, 8:8 + cout]
    keep = buf.clone()
    ref = pvcnn_ref.devoxelize(out.cpu().numpy(), v.cpu().numpy(), addend=sl.cpu().numpy())
    ops.trilinear_devoxelize(out, v, addend=sl, out=sl)          # in place, into the slice
    e_dev = float(np.abs(sl.cpu().numpy() - ref).max())
    assert torch.equal(buf[:, :8], keep[:, :8]) and torch.equal(buf[:, 8 + cout:], keep[:, 8 + cout:])
    print("r=%d %d -> %d: avg_voxelize %.3g, conv3d %.3g (|ref| <= %.3g), devoxelize %.3g" %
          (r, cin, cout, e_vox, e_conv, float(y.abs().max()), e_dev))
    assert e_vox <= 1e-5 and e_conv <= 1e-5 and e_dev <= 1e-5
    # points on cell corners and at r - 1: the value IS the corner's
    cv = dev([[0, 0, 0], [r - 1, r - 1, r - 1], [1, 2, r - 1], [r - 1, 0, 3], [2, 2, 2], [0, r - 1, 0], [3, 1, 0], [1, 1, 1]])
    got = ops.trilinear_devoxelize(out, cv)
    for i, (a, b_, c) in enumerate(cv.long().tolist()):
        assert torch.equal(got[i], out[i // 4, a, b_, c]), i
    assert torch.equal(ops.segment_max_rows(sl, B), sl.reshape(B, N, cout).max(1)[0])


def test_conv3d_at_resolution_64_against_float64():
    """r = 64, 64 -> 64, B = 1: 2 048 row tiles, every border case of the 27-tap mask at the model's largest grid."""
    from ml3d import ops
    rng = np.random.default_rng(64)
    x = dev(rng.standard_normal((1, 64, 64, 64, 64)) * (rng.random((1, 64, 64, 64, 1)) < 0.15))      # mostly empty, like a real grid
    w5, cb, gamma, beta, mean, var = _conv_case(rng, 64, 64)
    scale = gamma / torch.sqrt(var + 1e-4)
    w, bias, _ = ops.pack_conv3d_weights(w5.to(DEV), scale.to(DEV), (beta - mean * scale).to(DEV), cb.to(DEV))
    out = ops.conv3d_ndhwc(x, ops.pack_bf16x3(w), bias, 64, act=1, slope=0.1)
    y = _conv_reference(x.cpu().double().permute(0, 4, 1, 2, 3), w5, cb, gamma, beta, mean, var)
    err = float((out.cpu().double() - y).abs().max())
    print("conv3d r=64 64 -> 64: max|d| = %.3g at |ref| <= %.3g" % (err, float(y.abs().max())))
    assert err <= 1e-5


@pytest.mark.parametrize("name", ["pvcnn_small", "pvcnn_s3dis"])
def test_golden_of_the_reference_forward(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    m = _model(mcfg, int(g["weights_seed"]))
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g["state_shapes"]]
    point, feat = pvcnn_ref.make_inputs(g["cloud_seeds"], int(g["n"]))
    assert abs(point.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    B, N = point.shape[0], point.shape[2]
    out = m(dict(point=torch.from_numpy(point), feat=torch.from_numpy(feat)))
    torch.cuda.synchronize()
    assert out.shape == (B, N, int(mcfg["num_classes"]))
    out = out.reshape(B * N, -1).cpu().numpy()
    assert np.array_equal(m.last_voxels["stats"].cpu().numpy(), g["stats"])
    for r in g["resolutions"]:
        idx = m.last_voxels["vox"][int(r)].cpu().numpy()
        want = g["vox%d" % r]
        assert np.array_equal(idx, want) if want.ndim else pvcnn_ref.vox_checksum(idx) == int(want), r
    stride, tol = int(g["logit_stride"]), tol_for(g["logit_scale"])
    err = float(np.abs(out[::stride] - g["logits"]).max())
    labels = out.argmax(1)
    bad = np.nonzero(labels != g["labels"])[0]
    srt = np.sort(out[bad], axis=1)
    margins = [float(x) for x in (srt[:, -1] - srt[:, -2])]
    agree = float(1.0 - len(bad) / out.shape[0])
    print("%s: max|dlogit| = %.3g (tol %.3g, logit scale %.2f), label agreement %.6f, flipped margins %s" %
          (name, err, tol, float(g["logit_scale"]), agree, margins[:10]))
    record(name, family="pvcnn", max_abs_delta=err, tol=tol, logit_scale=float(g["logit_scale"]),
           ref_abs_max=float(np.abs(g["logits"]).max()), label_agreement=agree, flipped_margins=margins[:50],
           points=int(out.shape[0]))
    assert err <= tol
    assert all(x <= 2 * tol for x in margins), margins[:10]      # a differing label only where OUR top two are that close


def test_native_path_against_the_torch_formulation(golden_dir, monkeypatch):
    """Real-valued rooms of 2 x 40 960 points; both paths share the native voxel coordinates, so no voxel can flip."""
    g = np.load(os.path.join(golden_dir, "pvcnn_s3dis.npz"))
    mcfg = json.loads(str(g["model_json"]))
    m = _model(mcfg, int(g["weights_seed"]))
    point, feat = pvcnn_ref.make_inputs([31, 32], 40960, lattice=False)
    inp = dict(point=torch.from_numpy(point), feat=torch.from_numpy(feat))
    native = m(inp).reshape(-1, 13).cpu().numpy()
    vox = {r: t.cpu().numpy() for r, t in m.last_voxels["vox"].items()}
    monkeypatch.setenv("ML3D_PVCNN_OPS", "torch")
    plain = m(inp).reshape(-1, 13).cpu().numpy()
    assert all(np.array_equal(vox[r], t.cpu().numpy()) for r, t in m.last_voxels["vox"].items())
    scale = float(np.abs(plain).max())
    err = float(np.abs(native - plain).max())
    agree = float((native.argmax(1) == plain.argmax(1)).mean())
    print("native vs torch on 2 x 40 960 points: max|dlogit| = %.3g (tol %.3g, logit scale %.2f), label agreement %.6f" %
          (err, tol_for(scale), scale, agree))
    record("pvcnn_native_vs_torch", family="pvcnn", max_abs_delta=err, tol=tol_for(scale), logit_scale=scale,
           ref_abs_max=scale, label_agreement=agree, flipped_margins=[], points=int(native.shape[0]))
    assert native.shape == (81920, 13) and err <= tol_for(scale)


def test_forward_makes_no_device_to_host_synchronisation(golden_dir):
    g = np.load(os.path.join(golden_dir, "pvcnn_small.npz"))
    m = _model(json.loads(str(g["model_json"])), int(g["weights_seed"]))
    point, feat = pvcnn_ref.make_inputs(g["cloud_seeds"], int(g["n"]))
    inp = dict(point=torch.from_numpy(point).to(DEV), feat=torch.from_numpy(feat).to(DEV))
    first = m(inp)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = m(inp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(first, second)


def test_data_path_returns_one_label_per_input_point():
    from ml3d.torch.models import PVCNN
    mcfg = dict(num_classes=13, num_points=4096, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    m = PVCNN(**mcfg, seed=3, device=DEV)
    m.load_state_dict(pvcnn_ref.make_state_dict(mcfg, 2026))
    m.eval()
    n = 20000
    raw = (pt_ref.room(41, n) + np.float32([12.0, -7.0, 1.5])).astype(np.float32)
    data = dict(point=raw, feat=(pt_ref.colours(41, n) * 255).astype(np.float32), label=np.zeros(n, np.int32))
    m.inference_begin(dict(data))
    inp = m.inference_preprocess()
    assert inp["point"].shape == (3, 4096) and inp["feat"].shape == (9, 4096)
    logits = m(m.make_batch(inp))
    assert logits.shape == (1, 4096, 13)
    res = m.inference_end(inp, logits)
    lg = logits.reshape(-1, 13).cpu().numpy()
    e = np.exp(lg - lg.max(1, keepdims=True))
    probs = e / e.sum(1, keepdims=True)
    assert res["predict_labels"].shape == (4096,) and res["predict_scores"].shape == (4096, 13)
    assert np.array_equal(res["predict_labels"], probs.argmax(1)) and np.allclose(res["predict_scores"], probs, atol=1e-6)
