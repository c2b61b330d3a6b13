"""GPU parity: PointPillars inference forward (batched HIP voxelize -> fused pillar gather + PFN + scatter ->
f32-MFMA SECOND / SECONDFPN / heads) vs the CPU oracle and the reference-generated golden vectors
(tests/golden/pointpillars_*.npz, produced by the REAL reference module).  Tolerance 1e-4 on the head maps."""
import os

import numpy as np
import pytest
import torch

import synth_data
from oracle import pointpillars_ref as P

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _model(cfg, sd):
    from ml3d.torch.models.point_pillars import PointPillars
    m = PointPillars(device="cuda:0", **cfg)
    m.load_state_dict(sd)
    return m.eval()


def _clouds(cfg, frames):
    return [P.crop_for_cfg(synth_data.kitti_sweep(int(f)), cfg) for f in frames]


@pytest.mark.parametrize("name,cfg_name", [("pointpillars_small", "SMALL_CFG"), ("pointpillars_kitti", "KITTI_CFG")])
def test_forward_matches_reference_golden(golden_dir, name, cfg_name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = getattr(P, cfg_name)
    sd = P.make_state_dict(cfg, int(g["weights_seed"]))
    clouds = _clouds(cfg, g["frame_ids"])
    assert [len(c) for c in clouds] == list(g["n_points"])
    m = _model(cfg, sd)
    dev = torch.device("cuda:0")
    pts = [torch.from_numpy(c).to(dev) for c in clouds]
    # reference API: voxelize() -> (voxels, num_points, coors)
    voxels, num_points, coors = m.voxelize(pts)
    assert len(coors) == int(g["n_pillars"]) and int(num_points.sum()) == int(g["num_points_sum"])
    assert int((coors.cpu().long() * torch.tensor([1000003, 10007, 101, 1])).sum()) == int(g["coors_checksum"])
    assert np.array_equal(coors[:256].cpu().numpy().astype(np.int32), g["coors_head"])

    class In:
        point = pts
    outs = m(In())
    torch.cuda.synchronize()
    s = int(g["stride"])
    for nm, t in zip(("cls", "reg", "dir"), outs):
        a = t.cpu().numpy()
        assert list(a.shape) == list(g[nm + "_shape"])
        assert np.abs(a[:, :, ::s, ::s] - g[nm]).max() <= TOL
        assert abs(a.astype(np.float64).sum() - float(g[nm + "_sum"])) <= 1e-5 * float(g[nm + "_abssum"]) + 1e-3


def test_forward_matches_oracle_two_samples_kitti_widths():
    cfg = P.KITTI_CFG
    sd = P.make_state_dict(cfg, 11)
    clouds = _clouds(cfg, [3, 4])
    (rc, rr, rd), aux = P.forward(sd, cfg, [torch.from_numpy(c) for c in clouds])
    m = _model(cfg, sd)
    outs = m([torch.from_numpy(c).cuda() for c in clouds])
    for a, b in zip(outs, (rc, rr, rd)):
        assert a.shape == b.shape and (a.cpu() - b).abs().max().item() <= TOL
    # dense-voxel API parity (reference PointPillarsVoxelization.forward) on one sample
    v, c, n = m.voxel_layer(torch.from_numpy(clouds[0]).cuda())
    rv, rc2, rn = P.voxelization(torch.from_numpy(clouds[0]), cfg)
    assert torch.equal(v.cpu(), rv) and torch.equal(c.cpu(), rc2) and torch.equal(n.cpu(), rn)


def test_waymo_stride_pattern_and_three_channel_points():
    cfg = dict(P.SMALL_CFG)
    cfg["backbone"] = dict(in_channels=64, out_channels=[64, 128, 256], layer_nums=[1, 1, 1], layer_strides=[1, 2, 2])
    cfg["neck"] = dict(in_channels=[64, 128, 256], out_channels=[128, 128, 128], upsample_strides=[1, 2, 4],
                       use_conv_for_no_stride=False)
    cfg["head"] = dict(P.SMALL_CFG["head"], in_channels=384, feat_channels=384)
    sd = P.make_state_dict(cfg, 12)
    clouds = _clouds(cfg, [8])
    ref, _ = P.forward(sd, cfg, [torch.from_numpy(c) for c in clouds])
    outs = _model(cfg, sd)([torch.from_numpy(c).cuda() for c in clouds])
    for a, b in zip(outs, ref):
        assert (a.cpu() - b).abs().max().item() <= TOL


def test_get_bboxes_decode_and_hip_nms_match_reference_golden(golden_dir):
    """Anchor3DHead.get_bboxes on the reference's own head maps (full maps are stored for the small config)."""
    g = np.load(os.path.join(golden_dir, "pointpillars_small.npz"))
    cfg = P.SMALL_CFG
    m = _model(cfg, P.make_state_dict(cfg, int(g["weights_seed"])))
    dev = torch.device("cuda:0")
    cls, reg, dr = (torch.from_numpy(g[k]).to(dev) for k in ("cls", "reg", "dir"))
    boxes, scores, labels = m.bbox_head.get_bboxes(cls, reg, dr)
    for i in range(cls.shape[0]):
        assert np.array_equal(labels[i].cpu().numpy(), g["labels%d" % i])
        assert np.abs(scores[i].cpu().numpy() - g["scores%d" % i]).max() <= 1e-6
        assert np.abs(boxes[i].cpu().numpy() - g["boxes%d" % i]).max() <= 1e-4


def test_bench_configuration_16_sweeps_matches_the_oracle_on_sweeps_0_and_15():
    """The configuration bench.py --workload pointpillars times: 16 KITTI-shaped sweeps per forward.  Only at this size do the
    SECOND convolutions take the 128 x 128 register-blocked tiles everywhere (>= 256 workgroups on the 62 x 54 and 31 x 27
    maps) and the canvas / neck offsets pass 2^31 bytes.  The head maps of the first and the last sweep of the batch against
    the oracle's forward of those two sweeps (<= 1e-4), and their detections (decode + rotated NMS) against the oracle's
    ``get_bboxes`` on the oracle's maps."""
    cfg = P.KITTI_CFG
    sd = P.make_state_dict(cfg, 2024)
    clouds = _clouds(cfg, range(16))                                   # the bench's sweeps (rank 0)
    m = _model(cfg, sd)
    outs = m([torch.from_numpy(c).cuda() for c in clouds])
    torch.cuda.synchronize()
    pick = [0, 15]
    ref, _ = P.forward(sd, cfg, [torch.from_numpy(clouds[i]) for i in pick])
    for a, b in zip(outs, ref):
        assert a.shape[0] == 16 and a.shape[1:] == b.shape[1:]
        assert (a[pick].cpu() - b).abs().max().item() <= TOL
    boxes, scores, labels = m.bbox_head.get_bboxes(*outs)          # the whole batch decodes (what the bench step ends with)
    assert len(boxes) == 16 and all(b.shape[1] == 7 and b.shape[0] == s.shape[0] == l.shape[0]
                                    for b, s, l in zip(boxes, scores, labels))
    # decode + NMS on IDENTICAL inputs (the oracle's maps: a 1e-4 difference of the maps may swap the 100th / 101st candidate)
    gb, gs, gl = m.bbox_head.get_bboxes(*[t.cuda() for t in ref])
    for j in range(len(pick)):
        rb, rs, rl = P.get_bboxes_single(cfg, ref[0][j], ref[1][j], ref[2][j])
        assert np.array_equal(gl[j].cpu().numpy(), rl.numpy()), j
        assert np.abs(gs[j].cpu().numpy() - rs.numpy()).max() <= 1e-5
        assert (np.abs(gb[j].cpu().numpy() - rb.numpy()) / np.maximum(1.0, np.abs(rb.numpy()))).max() <= 1e-4


def test_two_lane_stream_returns_the_single_lane_detections():
    """``ml3d.engine.PointPillarsStream`` as bench.py runs it (2 lanes: the 16 sweeps of a step dealt to two independent
    pipelines whose kernels overlap on the GPU) against one lane: every sweep's labels identical, scores and boxes to 1e-5
    (the forward of a sweep does not depend on which other sweeps share its launch), in the order the sweeps were submitted."""
    from ml3d.engine import PointPillarsStream
    cfg = P.KITTI_CFG
    m = _model(cfg, P.make_state_dict(cfg, 2024))
    steps = [_clouds(cfg, range(16 * s, 16 * s + 16)) for s in range(3)]
    hosts = [[torch.from_numpy(c).pin_memory() for c in st] for st in steps]
    runs = []
    for lanes, threaded in ((1, False), (2, False), (2, True)):          # (2 lanes on one host thread / one thread per lane: round 5)
        pipe = PointPillarsStream(m, "cuda", lanes=lanes, threaded=threaded)
        got = [pipe.submit(h) for h in hosts] + [pipe.flush()]
        assert got[0] is None and pipe.flush() is None
        runs.append(got[1:])
    for other in runs[1:]:
        for one, two in zip(runs[0], other):
            assert len(one[0]) == len(two[0]) == 16
            for i in range(16):
                assert torch.equal(one[2][i], two[2][i]) and len(one[2][i]) > 0, i
                assert (one[1][i] - two[1][i]).abs().max().item() <= 1e-5
                assert (one[0][i] - two[0][i]).abs().max().item() <= 1e-4


# ---- SECOND's convolutions on the bf16 matrix pipe (three-way bf16 split, gemm_tile_bf3) ----------------------------------------
@pytest.mark.parametrize("cin,cout,stride,hw", [(64, 64, 1, (248, 216)), (64, 128, 2, (248, 216)), (128, 256, 2, (124, 108)),
                                                (256, 256, 1, (62, 54)), (32, 20, 1, (17, 9))])
def test_bf16x3_convolution_is_float32_equivalent(cin, cout, stride, hw):
    """The layer shapes of pointpillars_kitti.yml (2 sweeps) + a ragged one: |out - float64| of the bf16x3 kernel is of the order of the
    f32 MFMA kernel's own rounding (max over the map <= 4x + 2e-6; measured 0.9x .. 2.5x, profiles/r05_bf16x3_conv.log) and far inside the 1e-4 bar."""
    from ml3d import ops
    g = torch.Generator().manual_seed(cin + cout)
    dev = torch.device("cuda:0")
    x = torch.randn((2,) + hw + (cin,), generator=g).relu_().to(dev)
    w = (torch.randn((9 * cin, cout), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
    b = (torch.randn((cout,), generator=g) * 0.1).to(dev)
    pk = ops.pack_bf16x3(w)
    assert pk is not None and pk.dtype == torch.uint8
    o32 = ops.conv2d_nhwc(x, w, b, 3, 3, stride, 1, act=2)
    obf = ops.conv2d_nhwc(x, w, b, 3, 3, stride, 1, act=2, packed=pk)
    w4 = w.double().view(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous()
    ref = torch.relu(torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w4, b.double(), stride=stride, padding=1)).permute(0, 2, 3, 1)
    e32, ebf = float((o32.double() - ref).abs().max()), float((obf.double() - ref).abs().max())
    assert ebf <= 4 * e32 + 2e-6 and ebf <= 2e-5, (ebf, e32)
    assert e32 <= 2e-5, e32
    assert ops.pack_bf16x3(torch.zeros((9 * 48, 64), device=dev)) is None          # K = 432 is not a multiple of 32: f32 kernel


def test_both_convolution_paths_give_the_same_detections(monkeypatch):
    """ML3D_PP_CONV=f32 (f32 MFMA) and the default (bf16x3) on the same sweeps: head maps within 5e-5, the same detections."""
    cfg = P.KITTI_CFG
    sd = P.make_state_dict(cfg, 2024)
    clouds = [torch.from_numpy(c).cuda() for c in _clouds(cfg, [0, 5, 9])]
    res = {}
    for path in ("f32", "bf16x3"):
        monkeypatch.setenv("ML3D_PP_CONV", path)
        m = _model(cfg, sd)
        P_ = m.packed_params(m.device)
        assert all((c['packed'] is not None) == (path == "bf16x3") for blk in P_['blocks'] for c in blk)
        assert all((d['packed'] is not None) == (path == "bf16x3") for d in P_['deblocks'])
        assert (P_['head_packed'] is not None) == (path == "bf16x3")
        outs = m(clouds)
        res[path] = (outs, m.bbox_head.get_bboxes(*outs))
    for a, b in zip(res["f32"][0], res["bf16x3"][0]):
        # two float32-equivalent pipes that sum in different orders (the f32 path alone moves by 1.6e-5 when the batch size changes
        # its tile shapes: gpurun_out r5zb / tools/r05_calls/diag_two_lane.py); each is held to 1e-4 against the reference elsewhere
        d = (a - b).abs().max().item()
        assert d <= 5e-5, d
    # detections: the maps differ by a few 1e-5, so a candidate at the nms_pre cut or a pair at the IoU threshold may fall on the other
    # side -- every f32 detection must have a bf16x3 twin (same label, score within 1e-4, box within 2e-4 relative) except at most 1 % of them
    # (measured, tools/r05_calls/diag_two_pipes.py on 6 sweeps: identical labels and counts, scores within 2e-6, boxes within 3e-5 relative)
    for i in range(len(clouds)):
        bf, sf, lf = (res["f32"][1][k][i].cpu() for k in range(3))
        bb, sb, lb = (res["bf16x3"][1][k][i].cpu() for k in range(3))
        assert abs(len(lf) - len(lb)) <= max(1, len(lf) // 100), (len(lf), len(lb))
        unmatched = 0
        for j in range(len(lf)):
            same = (lb == lf[j]).nonzero().flatten()
            rel = (bb[same] - bf[j]).abs() / bf[j].abs().clamp(min=1.0)          # (random-init heads: exp(d) sizes of hundreds of metres)
            ok = len(same) > 0 and bool(((rel.amax(1) <= 2e-4) & ((sb[same] - sf[j]).abs() <= 1e-4)).any())
            unmatched += 0 if ok else 1
        assert unmatched <= max(1, len(lf) // 100), (i, unmatched, len(lf))
    monkeypatch.setenv("ML3D_PP_CONV", "fp8")
    with pytest.raises(ValueError):
        _model(cfg, sd).packed_params(torch.device("cuda:0"))


def _act64(x, act, slope):
    return {0: x, 1: np.where(x > 0, x, x * slope), 2: np.maximum(x, 0.0)}[act]


@pytest.mark.parametrize("path", ["f32", "bf16x3", "f32-split", "bf16x3-split"])
def test_every_epilogue_mode_at_every_store_site(path):
    """The GPU twin of tests/test_emulated_pillars.py::test_every_epilogue_mode_at_every_store_site (same shapes, data, float64
    reference and 1e-5 bound): plain, bias + leaky ReLU, bias + ReLU, residual, globally gathered residual with one index out of
    range and the stride-2 pixel shuffle through gemm_tile (f32, K = 64), tile2_epilogue (bf16x3, K = 64) and gemm_reduce (K = 512)."""
    from ml3d import _abi, ops
    lib = _abi.get()
    bf3, split = path.startswith("bf16x3"), path.endswith("split")
    k = 512 if split else 64
    rng = np.random.default_rng(k)
    m, n, mc, slope = 130, 36, 40, 0.2
    a = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)       # unit-variance sums at either K
    b = rng.standard_normal(n).astype(np.float32)
    r = rng.standard_normal((m, n)).astype(np.float32)
    rcoarse = rng.standard_normal((mc, n)).astype(np.float32)
    g = rng.integers(0, mc, (m, 3)).astype(np.int32)
    g[77, 0] = mc                                                          # ONE row outside [0, mc): adds nothing
    wsb = int((lib.ml3d_linear_bf16x3_workspace_bytes if bf3 else lib.ml3d_linear_workspace_bytes)(m, n, k))
    assert (wsb - 512 >= 2 * 4 * m * n) if split else (wsb == 512)         # K = 512 really is cut: partials of >= 2 slices
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()
    da, dw = dev(a), dev(w)
    packed = ops.pack_bf16x3(dw) if bf3 else None

    def run(bias, act, res, gather):
        if bf3:
            out = ops.linear_bf16x3(da, packed, n, dev(bias), act=act, slope=slope, residual=dev(res), residual_gather=dev(gather))
            assert out is not None
        else:
            out = ops.linear(da, dw, dev(bias), residual=dev(res), act=act, slope=slope, residual_gather=dev(gather))
        return out.cpu().numpy()

    prod = a.astype(np.float64) @ w.astype(np.float64)
    gathered = np.where((g[:, :1] >= 0) & (g[:, :1] < mc), rcoarse[np.clip(g[:, 0], 0, mc - 1)], 0.0)
    for name, bias, act, res, gather, ref in [("plain", None, 0, None, None, prod),
                                              ("bias + leaky", b, 1, None, None, prod + b),
                                              ("bias + relu", b, 2, None, None, prod + b),
                                              ("residual", b, 1, r, None, prod + b + r),
                                              ("gathered residual", b, 1, rcoarse, g, prod + b + gathered)]:
        err = np.abs(run(bias, act, res, gather) - _act64(ref, act, slope)).max()
        print("%s, %s: max|d| = %.3g" % (path, name, err))
        assert err <= 1e-5, (path, name, err)

    if path == "bf16x3-split":
        return                                   # (the bf16x3 deconvolution takes no workspace: never cut along K)
    h, wd, s, cout, ld, off = 10, 13, 2, 9, 16, 4
    if not bf3:
        dwsb = int(lib.ml3d_conv2d_workspace_bytes(1, h, wd, k, n, 1, 1))
        assert (dwsb - 512 >= 2 * 4 * m * n) if split else (dwsb == 512)
    big = torch.full((1, h * s, wd * s, ld), -1.0, dtype=torch.float32, device="cuda:0")
    ops.deconv2d_nhwc(da.view(1, h, wd, k), dw, dev(b[:cout].copy()), s, cout, act=2, out=big, out_channel_offset=off, packed=packed)
    big = big.cpu().numpy()
    ref = np.maximum(prod.reshape(h, wd, s, s, cout) + b[:cout], 0.0).transpose(0, 2, 1, 3, 4).reshape(1, h * s, wd * s, cout)
    err = np.abs(big[..., off:off + cout] - ref).max()
    print("%s, pixel shuffle: max|d| = %.3g" % (path, err))
    assert err <= 1e-5, (path, "pixel shuffle", err)
    assert (big[..., :off] == -1).all() and (big[..., off + cout:] == -1).all()
