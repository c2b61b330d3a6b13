"""Shared bodies of the PointNet++ op tests: tests/test_emulated_pointnet2.py runs them on CPU tensors against the host emulation
of csrc/pointnet2.hip, tests/test_gpu_pointnet2.py on the MI355X, tests/test_pn2_cases_can_fail.py against deliberately wrong
stand-ins (every body takes the implementation under test as ``impl``; None = the product's ``ml3d.ops``).

Index results (ball query, three nearest neighbours) are compared for EQUALITY with the numpy restatements of tests/pn2_ref.py.
Float results are judged by ``pt_cases.judge``: against the direct formula in FLOAT64, within max(1e-5, 4 e32), e32 the error of
the same formula in float32 at the case's own inputs.  Slice writes, row independence and determinism are compared bit for bit."""
import numpy as np
import torch

import pn2_ref
import pt_ref
from pt_cases import _dbl, _print, f32, judge, refused, same_bits

BALL_N = (5, 67, 130, 1000)
BALL_M = (1, 8, 67)
BALL_SCALES = ((0.8, 1.15), (16, 32))                 # (radii, nsample) of the two-scale call: at n = 1000 about half the balls overflow
SA_CASES = ((0, (16, 16, 32)), (3, (32, 32, 64)), (96, (64, 96, 128)), (64, (128, 196, 256)))      # (feature channels, widths); the last one unfused
SA_NSAMPLE = (16, 32)
SA_M = (5, 67)
SA_RADIUS = {16: 1.4, 32: 2.0}                         # on 300 points of the room: hit counts on both sides of nsample
INTERP_C = (13, 128, 512)


def _ops(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- ball query ---------------------------------------------------------------------------------------------------------------------
def ball_cloud(n, m, seed=0):
    """A 6 x 5 x 3 m room with n points; m centres: the first far outside the room (no hit at any radius used here), the others
    on points of the cloud spread over its whole index range, every third one moved 0.3 m off its point."""
    rng = np.random.default_rng([n, m, seed])
    pts = pt_ref.room(n + 7 * seed, n)
    pick = np.linspace(0, n - 1, m).astype(np.int64)
    ctr = pts[pick].copy()
    ctr[::3] += np.float32(0.3)
    ctr[0] = np.float32([100.0, 100.0, 100.0])
    return pts, ctr.astype(np.float32), rng


def run_ball_query(dev, impl, xyz, new_xyz, radius, nsample):
    out = _ops(impl).ball_query(_t(xyz, dev), _t(new_xyz, dev), radius, nsample)
    outs = out if isinstance(out, (list, tuple)) else [out]
    for o, k in zip(outs, nsample if isinstance(nsample, (list, tuple)) else [nsample]):
        assert o.dtype == torch.int32 and tuple(o.shape) == (xyz.shape[0], new_xyz.shape[1], k)
    res = [o.cpu().numpy() for o in outs]
    return res if isinstance(out, (list, tuple)) else res[0]


def _ball_equal(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def check_ball_query(dev, n, m, impl=None):
    """Both scales in one call against the restatement, each scale alone equal to its half of the joint call, the call twice."""
    pts, ctr, _ = ball_cloud(n, m)
    xyz, new_xyz = pts[None], ctr[None]
    radii, ns = list(BALL_SCALES[0]), list(BALL_SCALES[1])
    got = run_ball_query(dev, impl, xyz, new_xyz, radii, ns)
    for s in range(2):
        _ball_equal(got[s], pn2_ref.ball_query(xyz, new_xyz, radii[s], ns[s]), ("joint", n, m, s))
        _ball_equal(run_ball_query(dev, impl, xyz, new_xyz, radii[s], ns[s]), got[s], ("alone", n, m, s))
        assert not got[s][0, 0].any(), "the centre outside the room has no hit: all zeros"
    again = run_ball_query(dev, impl, xyz, new_xyz, radii, ns)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    if n < 16:
        assert ns[0] > n                                     # more slots than points: every ball is padded
    # a tiny radius: a centre ON a point finds that point alone, every other centre nothing
    tiny = run_ball_query(dev, impl, xyz, new_xyz, 1e-4, 16)
    _ball_equal(tiny, pn2_ref.ball_query(xyz, new_xyz, 1e-4, 16), ("tiny", n, m))
    assert int(pn2_ref.hit_counts(xyz, new_xyz, 1e-4).max()) <= 1


def check_ball_query_properties(dev, impl=None):
    """n = 1000, m = 67: the case holds what the contract distinguishes (asserted on the restatement's hit counts), so a kernel
    that passes has been through each: truncation with hits spread over several 64-point steps, padding, no hit, one scale
    full while the other scans on."""
    n, m = 1000, 67
    pts, ctr, _ = ball_cloud(n, m)
    xyz, new_xyz = pts[None], ctr[None]
    radii, ns = list(BALL_SCALES[0]), list(BALL_SCALES[1])
    cnt = [pn2_ref.hit_counts(xyz, new_xyz, r)[0] for r in radii]
    want = [pn2_ref.ball_query(xyz, new_xyz, radii[s], ns[s]) for s in range(2)]
    for s in range(2):
        full = cnt[s] > ns[s]
        assert full.sum() >= 5 and ((cnt[s] > 0) & (cnt[s] < ns[s])).sum() >= 5 and (cnt[s] == 0).sum() >= 1, (s, cnt[s])
        steps = [len(np.unique(want[s][0, i] // 64)) for i in np.flatnonzero(full)]
        assert max(steps) >= 3, "the kept hits of some truncated ball come from at least 3 steps of 64 points"
    # the wide scale takes its 32nd hit at a later point than the narrow one its 16th, or the reverse
    both = np.flatnonzero((cnt[0] > ns[0]) & (cnt[1] > ns[1]))
    last = np.array([[want[s][0, i].max() // 64 for s in range(2)] for i in both])
    assert (last[:, 0] > last[:, 1]).any() and (last[:, 0] < last[:, 1]).any(), "either scale fills first somewhere"
    got = run_ball_query(dev, impl, xyz, new_xyz, radii, ns)
    for s in range(2):
        _ball_equal(got[s], want[s], ("properties", s))


def check_ball_query_boundary_and_duplicates(dev, impl=None):
    """r = 0.5 and a point at offset (0.5, 0, 0): d2 == r * r exactly, NOT a hit; the point one ulp nearer is.  Duplicate points:
    each copy is a hit of its own, in index order."""
    ctr = np.zeros((1, 1, 3), np.float32)
    near = np.nextafter(np.float32(0.5), np.float32(0))
    pts = np.float32([[[3, 0, 0], [0.5, 0, 0], [near, 0, 0], [0, 0.5, 0], [0, 0, -0.5], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [0.5, 0, 0]]])
    assert pn2_ref.dist2(ctr[0], pts[0])[0, 1] == np.float32(0.25)
    got = run_ball_query(dev, impl, pts, ctr, 0.5, 6)
    want = np.int32([[[2, 5, 6, 2, 2, 2]]])
    assert np.array_equal(pn2_ref.ball_query(pts, ctr, 0.5, 6), want)
    _ball_equal(got, want, "boundary")
    rng = np.random.default_rng(3)
    base = pt_ref.room(3, 90)
    dup = np.concatenate([base, base[rng.integers(0, 90, 60)], base[:40]])[None]       # 190 points, 100 of them copies
    c = dup[:, [0, 17, 95, 150, 189]].copy()
    for r, k in ((0.6, 16), (1e-4, 8)):
        _ball_equal(run_ball_query(dev, impl, dup, c, r, k), pn2_ref.ball_query(dup, c, r, k), ("duplicates", r))
    assert pn2_ref.hit_counts(dup, c, 1e-4).min() >= 2


def check_ball_query_batch(dev, impl=None):
    """B = 3: every item equals its single-item run (item-local indices)."""
    items = [ball_cloud(130, 8, seed) for seed in (1, 2, 3)]
    xyz, new_xyz = np.stack([i[0] for i in items]), np.stack([i[1] for i in items])
    radii, ns = list(BALL_SCALES[0]), list(BALL_SCALES[1])
    got = run_ball_query(dev, impl, xyz, new_xyz, radii, ns)
    for s in range(2):
        _ball_equal(got[s], pn2_ref.ball_query(xyz, new_xyz, radii[s], ns[s]), ("batch", s))
        for b in range(3):
            alone = run_ball_query(dev, impl, xyz[b:b + 1], new_xyz[b:b + 1], radii, ns)[s]
            _ball_equal(got[s][b:b + 1], alone, ("batch item", b, s))
        assert int(got[s].max()) < 130


def check_ball_query_refusals(dev):
    from ml3d import ops
    xyz, c = torch.zeros((1, 10, 3), device=dev), torch.zeros((1, 2, 3), device=dev)
    refused(lambda: ops.ball_query(xyz, c, [0.1] * 5, [4] * 5), "5 scales")
    refused(lambda: ops.ball_query(xyz, c, 0.1, 0), "nsample = 0")
    refused(lambda: ops.ball_query(xyz, c, -1.0, 4), "negative radius")
    refused(lambda: ops.ball_query(xyz[:, :0].contiguous(), c, 0.1, 4), "no points")


# ---- set abstraction ----------------------------------------------------------------------------------------------------------------
def sa_inputs(cf, widths, ns, m, seed=0):
    """B = 2 items of n = 300 points, item 0 centred on the origin, item 1 moved to (30, -20, 5) (a lidar frame's coordinates:
    W p - W c would cancel there), ``cf`` feature channels, m centres per item (cloud points; the index row of centre 0 is all
    zeros, as ball_query writes it for a centre without a hit; centre 1 keeps a single neighbour in every slot: all padding).
    Weights at the magnitudes of tests/pt_cases.py, about a quarter of every layer's BatchNorm scales negative."""
    rng = np.random.default_rng([cf, widths[0], widths[2], ns, m, seed])
    b, n = 2, 300
    xyz = np.stack([pt_ref.room(11 + i, n) for i in range(b)])
    xyz = (xyz - (xyz.min(1, keepdims=True) + xyz.max(1, keepdims=True)) / np.float32(2)).astype(np.float32)
    xyz[1] += np.float32([30.0, -20.0, 5.0])
    ctr = np.stack([x[rng.choice(n, m, replace=False)] for x in xyz])
    idx = pn2_ref.ball_query(xyz, ctr, SA_RADIUS[ns], ns)
    idx[:, 0, :] = 0
    if m > 1:
        idx[:, 1, :] = idx[:, 1, :1]
    hits = pn2_ref.hit_counts(xyz, ctr, SA_RADIUS[ns])[:, 2:]
    # full balls (every slot another neighbour: the LAST slot matters) and padded ones
    assert (hits >= ns).any() and (m < 60 or (((hits > 0) & (hits < ns)).any() and (hits >= ns).sum() >= 10)), hits
    feat = None if cf == 0 else f32(np.abs(rng.standard_normal((b, n, cf))))
    layers, cin = [], 3 + cf
    for cout in widths:
        w = rng.uniform(-1, 1, (cin, cout)) * 1.6 / np.sqrt(cin)
        sc = rng.uniform(0.6, 1.5, cout) * np.where(rng.random(cout) < 0.25, -1, 1)
        sc[cout // 3] = -abs(sc[cout // 3])
        layers.append((f32(w), f32(sc), f32(rng.normal(0, 0.2, cout))))
        cin = cout
    return f32(xyz), feat, f32(ctr), torch.from_numpy(idx), layers


def sa_refs(xyz, feat, ctr, idx, layers):
    return pn2_ref.sa_formula(*_dbl((xyz, feat, ctr)), idx, _dbl(layers)), pn2_ref.sa_formula(xyz, feat, ctr, idx, layers)


def sa_pack(ops, xyz, feat, layers, ns, dev):
    """What the model class does once per scale: fold the BatchNorm scales into the weights, split off the position rows; and once
    per forward: y = f Wf per source point (None without features)."""
    (w1, s1, t1), (w2, s2, t2), (w3, s3, t3) = layers
    w1 = w1 * s1
    params = ops.pack_sa_weights(w1[:3].to(dev), t1.to(dev), (w2 * s2).to(dev), t2.to(dev), (w3 * s3).to(dev), t3.to(dev), ns)
    y = None if feat is None else (feat.reshape(-1, feat.shape[2]) @ w1[3:]).contiguous().to(dev)
    return params, y


def run_sa(dev, impl, xyz, feat, ctr, idx, layers, out=None):
    ops = _ops(impl)
    params, y = sa_pack(ops, xyz, feat, layers, int(idx.shape[2]), dev)
    return ops.pn2_sa_mlp_max(y, xyz.to(dev), ctr.to(dev), idx.to(dev), params, out=out)


def poison(dev, nbytes=1 << 24):
    """NaN into memory the allocator hands out next (intermediate buffers and workspaces of the call that follows)."""
    blocks = [torch.full((nbytes // 4 // 4,), float("nan"), dtype=torch.float32, device=dev) for _ in range(4)]
    del blocks


def check_sa(dev, cf, widths, ns, m, impl=None, report=_print):
    xyz, feat, ctr, idx, layers = sa_inputs(cf, widths, ns, m)
    if impl is None:
        from ml3d import ops
        assert ops.sa_fused(ns, *widths) == (max(widths) <= 128), "the dispatch rule: fused up to width 128"
    r64, r32 = sa_refs(xyz, feat, ctr, idx, layers)
    b, c3 = int(xyz.shape[0]), widths[2]
    name = "sa cf=%d widths=%s ns=%d m=%d" % (cf, "-".join(map(str, widths)), ns, m)
    poison(dev)
    got = run_sa(dev, impl, xyz, feat, ctr, idx, layers).cpu()
    judge(report, name, got, r64.reshape(b * m, c3), r32.reshape(b * m, c3))
    assert float(r64.max()) > 0
    # a column slice of a wider buffer: the other columns keep their sentinel
    wide = torch.full((b * m, c3 + 11), -7.0, dtype=torch.float32, device=dev)
    poison(dev)
    run_sa(dev, impl, xyz, feat, ctr, idx, layers, out=wide[:, 4:4 + c3])
    wide = wide.cpu()
    assert same_bits(wide[:, 4:4 + c3].contiguous(), got), "slice write"
    assert bool((wide[:, :4] == -7.0).all()) and bool((wide[:, 4 + c3:] == -7.0).all()), "columns outside the slice were written"
    # every centre alone: the same bits (first, second, last -- at odd m the last tile of two centres is half empty)
    for i in sorted(set((0, min(1, m - 1), m // 2, m - 1))):
        alone = run_sa(dev, impl, xyz, feat, ctr[:, i:i + 1].contiguous(), idx[:, i:i + 1].contiguous(), layers).cpu()
        assert same_bits(alone, got.view(b, m, c3)[:, i].contiguous()), (name, "row alone", i)


def check_sa_refusals(dev):
    """The fused entry refuses what the dispatch rule sends elsewhere (before any launch: the output keeps its fill), and the
    wrapper refuses inconsistent shapes."""
    from ml3d import _abi, ops
    from ml3d.ops import _gates
    L = _abi.get()
    for ns, c1, c2, c3, want in ((8, 16, 16, 32, -4), (16, 130, 16, 32, -4), (16, 16, 16, 48, -4), (32, 64, 196, 128, -4),
                                 (16, 16, 16, 32, -1)):
        out = torch.full((4, 256), -7.0, dtype=torch.float32, device=dev)
        z = torch.zeros((64, 256), dtype=torch.float32, device=dev)
        idx = torch.zeros((1, 4, 64), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = L.ml3d_pn2_sa_mlp_max(z.data_ptr(), 256 if want == -4 else 8, z.data_ptr(), z.data_ptr(), idx.data_ptr(), 1, 64, 4, ns,
                                       c1, c2, c3, *[z.data_ptr()] * 6, out.data_ptr(), 256, _gates._stream())
        assert rc == want and bool((out.cpu() == -7.0).all()), (ns, c1, c2, c3, rc)
    xyz, feat, ctr, idx, layers = sa_inputs(3, (32, 32, 64), 16, 5)
    params, y = sa_pack(ops, xyz, feat, layers, 16, dev)
    refused(lambda: ops.pn2_sa_mlp_max(y, xyz.to(dev), ctr.to(dev), idx[:, :, :8].contiguous().to(dev), params), "nsample mismatch", "expected")
    refused(lambda: ops.pn2_sa_mlp_max(y, xyz[:, :299].contiguous().to(dev), ctr.to(dev), idx.to(dev), params), "row count mismatch", "expected")


# ---- the module against the reference's forward -------------------------------------------------------------------------------------
MODULE_GOLDENS = ("pointnet2_small", "pointnet2_kitti")


def check_module(dev, name, report=_print):
    """tests/golden/<name>.npz (tools/gen_golden_pointnet2.py: the REAL reference ``Pointnet2MSG`` on PyTorch-CPU): the state-dict
    layout, every FPS / ball-query / 3-NN index array for equality, the features within max(1e-4, 4.4e-6 scale) -- the project's
    rule for whole forwards -- on the HIP kernels AND on the torch formulation (``ML3D_PN2_OPS=torch``), and the two against each
    other under the same bound."""
    import json
    import os
    from ml3d.torch.modules import Pointnet2MSG
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    model = Pointnet2MSG(**mcfg, device=dev)
    sd = model.state_dict()
    keys, shapes = [str(k) for k in g["state_keys"]], [json.loads(str(s)) for s in g["state_shapes"]]
    assert list(sd) == keys and [list(v.shape) for v in sd.values()] == shapes
    model.load_state_dict(pn2_ref.make_state_dict(keys, shapes, int(g["weights_seed"])))
    pc = pn2_ref.make_pointcloud(g["cloud_seeds"], int(g["n"]), int(mcfg["in_channels"]), float(g["cloud_scale"]), g["cloud_offset"])
    assert abs(pc.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    scale, stride = float(g["feature_scale"]), int(g["row_stride"])
    tol = max(1e-4, 4.4e-6 * scale)
    outs = {}
    for mode in ("hip", "torch"):
        os.environ["ML3D_PN2_OPS"] = mode
        try:
            xyz, feat = model(_t(pc, dev))
        finally:
            del os.environ["ML3D_PN2_OPS"]
        assert same_bits(xyz, torch.from_numpy(pc[..., :3]).contiguous())
        used = model.last_indices
        for l, (fps, balls) in enumerate(zip(used["fps"], used["ball"])):
            assert np.array_equal(fps.cpu().numpy(), g["fps%d" % l].astype(np.int32)), (mode, "fps", l)
            for s, idx in enumerate(balls):
                assert np.array_equal(idx.cpu().numpy(), g["ball%d_%d" % (l, s)].astype(np.int32)), (mode, "ball", l, s)
        for j, idx in enumerate(used["nn3"]):
            assert np.array_equal(idx.cpu().numpy(), g["nn3_%d" % j].astype(np.int32)), (mode, "nn3", j)
        outs[mode] = feat.cpu()
        got = outs[mode][:, :, ::stride].numpy()
        err = float(np.abs(got - g["features"]).max())
        report(name="%s %s" % (name, mode), max_abs_delta=err, tol=tol, feature_scale=scale)
        assert got.shape == g["features"].shape and bool(np.isfinite(got).all()) and err <= tol, (name, mode, err, tol)
    err = float((outs["hip"] - outs["torch"]).abs().max())
    report(name="%s hip vs torch" % name, max_abs_delta=err, tol=tol, feature_scale=scale)
    assert err <= tol, (name, err, tol)


# ---- three nearest neighbours, interpolation ----------------------------------------------------------------------------------------
def interp_inputs(c, seed=0):
    """B = 2, n = 133 queries (no multiple of 64), M = 40 known points of the same room; query 5 of each item coincides with a
    known point."""
    rng = np.random.default_rng([c, seed])
    b, n, mk = 2, 133, 40
    q = np.stack([pt_ref.room(21 + i, n) for i in range(b)])
    known = np.stack([x[rng.choice(n, mk, replace=False)] for x in q])
    q[:, 5] = known[:, 7]
    return q, known, f32(np.abs(rng.standard_normal((b, mk, c))))


def check_three_nn(dev, impl=None):
    """Equality with the restatement -- indices AND squared distances (the same three products and two sums); duplicated known
    points: the tie goes to the lowest index; fewer than 3 known points are refused."""
    ops = _ops(impl)
    q, known, _ = interp_inputs(13)
    known[:, 30] = known[:, 2]
    known[:, 31] = known[:, 2]                                 # three copies of one point: (2, 30, 31) in that order wherever it is nearest
    q[:, 9] = known[:, 2]
    d2, idx = ops.three_nn(_t(q, dev), _t(known, dev))
    want_d, want_i = pn2_ref.three_nn(q, known)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(d2.cpu().numpy(), want_d)
    rows = np.flatnonzero(want_i[0, :, 0] == 2)
    assert len(rows) and (want_i[0, rows] == [2, 30, 31]).all() and (want_d[0, rows, 0] == want_d[0, rows, 2]).all()
    assert want_d[0, 5, 0] == 0.0
    refused(lambda: ops.three_nn(_t(q, dev), _t(known[:, :2], dev)), "2 known points")


def check_interpolate(dev, c, impl=None, report=_print):
    ops = _ops(impl)
    q, known, feat = interp_inputs(c)
    b, n, mk = q.shape[0], q.shape[1], known.shape[1]
    want_d, want_i = pn2_ref.three_nn(q, known)
    d2, idx = torch.from_numpy(want_d), torch.from_numpy(want_i)
    r64, r32 = pn2_ref.fp_interpolate_formula(feat.double(), idx, d2.double()), pn2_ref.fp_interpolate_formula(feat, idx, d2)
    args = (feat.reshape(b * mk, c).to(dev), b, idx.reshape(b * n, 3).to(dev), d2.reshape(b * n, 3).to(dev))
    got = ops.pn2_interpolate(*args).cpu()
    judge(report, "interpolate c=%d" % c, got, r64.reshape(b * n, c), r32.reshape(b * n, c))
    # the query ON a known point takes that point's features (weight 1 up to the 1e-8 guard)
    for i in range(b):
        assert int(idx[i, 5, 0]) == 7 and float((got.view(b, n, c)[i, 5] - feat[i, 7]).abs().max()) <= 1e-5
    # into a column slice, from a column slice
    wide = torch.full((b * n, c + 9), -7.0, dtype=torch.float32, device=dev)
    src = torch.full((b * mk, c + 5), 3.0, dtype=torch.float32, device=dev)
    src[:, 2:2 + c] = args[0]
    ops.pn2_interpolate(src[:, 2:2 + c], *args[1:], out=wide[:, 6:6 + c])
    wide = wide.cpu()
    assert same_bits(wide[:, 6:6 + c].contiguous(), got)
    assert bool((wide[:, :6] == -7.0).all()) and bool((wide[:, 6 + c:] == -7.0).all())
    # the public form in the reference's layout, with the reference's own weights
    rec = 1.0 / (torch.sqrt(d2) + 1e-8)
    w = rec / rec.sum(2, keepdim=True)
    pub = ops.three_interpolate(feat.transpose(1, 2).contiguous().to(dev), idx.to(dev), w.to(dev)).cpu()
    assert tuple(pub.shape) == (b, c, n)
    judge(report, "three_interpolate c=%d" % c, pub.transpose(1, 2).reshape(b * n, c), r64.reshape(b * n, c), r32.reshape(b * n, c))
    refused(lambda: ops.pn2_interpolate(args[0][:2 * b].contiguous(), b, args[2], args[3]), "2 known points per item")
