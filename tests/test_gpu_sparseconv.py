"""GPU: the SparseConvUnet extension on the MI355X -- the voxel pyramid and every rulebook of ``ml3d_scn_build`` EXACT against
the dictionary-lookup restatement of the contract (tests/scn_ref.py), the rulebook convolution against the float64 direct
formula, both goldens of the REAL reference forward (tools/gen_golden_sparseconvunet.py; logits within the project's rule
``max(1e-4, 4.4e-6 * logit_scale)``), the native path against the torch formulation (``ML3D_SCN_OPS=torch``) on a real-valued
room, at most ONE device -> host synchronisation per forward, and the data path.  The measured deviations are appended to the
per-YAML parity record of tests/test_gpu_configs.py (its ``record``).

Tolerance of the op tests, 1e-5 at outputs of order 1 (the derivation of tests/test_gpu_pvcnn.py restated for these shapes):
a convolution sums at most 27 * 224 = 6 048 products with float32 accumulation (the bf16x3 split is float32-equivalent: its own
error is O(2^-25) per product); with products of order 1 / sqrt(6 048) the expected accumulation error is
sqrt(6 048) * 6e-8 = 4.7e-6 at outputs of order 1.  The cases here sum at most 27 * 96 = 2 592 products (3.1e-6)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import scn_ref
from test_gpu_configs import flips, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_TOL = 1e-5


def tol_for(scale, base=1e-4):
    """The project's rule (tests/test_gpu_configs.py:25-31), unchanged."""
    return max(base, 4.4e-6 * float(scale))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _model(mcfg, seed, gain=scn_ref.WEIGHT_GAIN):
    from ml3d.torch.models import SparseConvUnet
    m = SparseConvUnet(**mcfg, device=DEV)
    m.load_state_dict(scn_ref.make_state_dict(mcfg, seed, gain=gain))
    return m.eval()


@pytest.fixture(autouse=True)
def _native_by_default(monkeypatch):
    monkeypatch.delenv("ML3D_SCN_OPS", raising=False)


@pytest.fixture(scope="module")
def edge():
    """The edge batch, its reference pyramid (computed once, shared, never modified) and the native one."""
    from ml3d import ops
    pts, feat, rs = scn_ref.edge_batch()
    ref = scn_ref.build(pts, feat, rs)
    pyr = ops.scn_build(dev(pts), dev(feat), rs)
    return pts, feat, rs, ref, pyr


def _check_pyramid(pyr, ref):
    levels = len(ref["coords"])
    assert pyr.read_counts() == ref["counts"].tolist()
    assert np.array_equal(pyr.index_map.cpu().numpy(), ref["index_map"])
    assert np.array_equal(pyr.feat0[:, :3].cpu().numpy(), ref["feat0"])           # 2^-6 lattice: the float32 sums are exact
    assert not pyr.feat0[:, 3:].any()
    for l in range(levels):
        assert np.array_equal(pyr.coords(l).cpu().numpy(), ref["coords"][l]), l
        assert np.array_equal(pyr.nbr27(l).cpu().numpy(), ref["nbr27"][l]), l
        if l >= 1:
            assert np.array_equal(pyr.child8(l).cpu().numpy(), ref["child8"][l]), l
        if l + 1 < levels:
            assert np.array_equal(pyr.parent(l).cpu().numpy(), ref["parent"][l]), l
            assert np.array_equal(pyr.ptap(l).cpu().numpy(), ref["ptap"][l]), l
            assert np.array_equal(pyr.up8(l).cpu().numpy(), ref["up8"][l]), l


def test_rulebooks_exact_on_the_edge_batch(edge):
    pts, feat, rs, ref, pyr = edge
    c0 = ref["coords"][0]
    counts = ref["counts"].tolist()
    # what the batch must contain (see scn_ref.edge_batch)
    for item in (0, 1):
        have = {tuple(r[1:]) for r in c0[c0[:, 0] == item].tolist()}
        assert {(0, 0, 0), (4095, 4095, 4095), (2000, 17, 3001), (1000, 1000, 1000), (1001, 1001, 1001)} <= have
        assert all((500 + a, 600 + b, 700 + c) in have for a in range(3) for b in range(3) for c in range(3))
    iso = np.nonzero((c0[:, 1:] == (2000, 17, 3001)).all(1))[0]
    assert all((ref["nbr27"][0][i] >= 0).sum() == 1 for i in iso)                                   # isolated: only itself
    assert ((ref["nbr27"][0] >= 0).sum(1) == 27).any()                                               # a full block's centre
    assert np.bincount(ref["index_map"]).max() >= 50                                                 # >= 50 duplicate points
    assert len({tuple(r[1:]) for r in c0[c0[:, 0] == 0].tolist()} & {tuple(r[1:]) for r in c0[c0[:, 0] == 1].tolist()}) >= 40
    assert all(c % 128 for c in counts) and min(counts) < 128 < max(counts)
    _check_pyramid(pyr, ref)


def test_rulebooks_exact_down_to_a_single_row():
    """(A two-item batch has two rows at least at every level -- the item is part of a voxel's identity -- so the single-row
    deepest level comes from a one-item cloud.)"""
    from ml3d import ops
    pts, feat, rs = scn_ref.deep_cloud()
    ref = scn_ref.build(pts, feat, rs)
    assert ref["counts"][-1] == 1
    _check_pyramid(ops.scn_build(dev(pts), dev(feat), rs), ref)


CONV_CASES = [(32, 32, 27), (96, 64, 27), (64, 96, 8), (16, 48, 27)]


@pytest.mark.parametrize("cin,cout,taps", CONV_CASES)
def test_sparse_conv_against_the_direct_formula(edge, cin, cout, taps):
    from ml3d import ops
    _, _, _, ref, pyr = edge
    rng = np.random.default_rng(cin * 1000 + cout)
    if taps == 27:
        rule_ref, rule, rows_in = ref["nbr27"][0], pyr.nbr27(0), int(ref["counts"][0])
    else:
        rule_ref, rule, rows_in = ref["child8"][1], pyr.child8(1), int(ref["counts"][0])
    x = rng.uniform(-1, 1, (rows_in, cin)).astype(np.float32)
    # (order-1 outputs: a row meets ~ a fifth of the taps)
    w = (rng.uniform(-1, 1, (taps, cin, cout)) * np.sqrt(3.0 / (0.25 * taps * cin))).astype(np.float32)
    wt, _, cp, _ = ops.pack_sparse_weights(dev(w))
    xp = torch.zeros((rows_in, cp), device=DEV)
    xp[:, :cin] = dev(x)
    packed = ops.pack_bf16x3(wt)
    out = ops.sparse_conv(xp, rule.contiguous(), packed, cout, cp=cp)
    want = scn_ref.conv_direct(x, rule_ref, w)
    err = float(np.abs(out.cpu().numpy() - want).max())
    print("sparse_conv %d -> %d, T = %d: max |d| = %.3g at max |out| = %.3g" % (cin, cout, taps, err, np.abs(want).max()))
    assert 0.5 < np.abs(want).max() < 8 and err <= OP_TOL * max(1.0, np.abs(want).max())
    again = ops.sparse_conv(xp, rule.contiguous(), packed, cout, cp=cp)
    assert torch.equal(out, again)


def test_transposed_conv_and_the_residual_second_block_epilogue(edge):
    from ml3d import ops
    _, _, _, ref, pyr = edge
    rng = np.random.default_rng(5)
    m0, m1 = int(ref["counts"][0]), int(ref["counts"][1])
    # transposed 2 x 2 x 2, 64 -> 32, written into the right half of a [M0, 64] join buffer
    y = rng.uniform(-1, 1, (m1, 64)).astype(np.float32)
    w = (rng.uniform(-1, 1, (8, 64, 32)) * np.sqrt(3.0 / 64)).astype(np.float32)
    wt, _, cp, _ = ops.pack_sparse_weights(dev(w))
    join = torch.full((m0, 64), 7.0, device=DEV)
    ops.sparse_conv(dev(y), pyr.up8(0).contiguous(), ops.pack_bf16x3(wt), 32, cp=cp, out=join[:, 32:])
    want = np.stack([y[ref["parent"][0][i]].astype(np.float64) @ w[ref["ptap"][0][i]].astype(np.float64) for i in range(m0)])
    # (two float64 evaluations of the same formula: equal up to the summation order of the 64 products)
    assert np.abs(scn_ref.conv_direct(y, ref["up8"][0], w) - want).max() <= 1e-12
    got = join.cpu().numpy()
    assert (got[:, :32] == 7.0).all() and np.abs(got[:, 32:] - want).max() <= OP_TOL * max(1.0, np.abs(want).max())
    # 3 x 3 x 3, 32 -> 32 + bias + identity residual + ReLU; then 3 x 3 x 3, 32 -> 32 with a dense second block [M0, 64] x [64, 32]
    x = rng.uniform(-1, 1, (m0, 32)).astype(np.float32)
    x2 = rng.uniform(-1, 1, (m0, 64)).astype(np.float32)
    res = rng.uniform(-1, 1, (m0, 32)).astype(np.float32)
    bias = rng.uniform(-1, 1, 32).astype(np.float32)
    w3 = (rng.uniform(-1, 1, (27, 32, 32)) * np.sqrt(3.0 / (0.25 * 27 * 32))).astype(np.float32)
    w2 = (rng.uniform(-1, 1, (64, 32)) * np.sqrt(3.0 / 64)).astype(np.float32)
    rule = pyr.nbr27(0).contiguous()
    wt, _, cp, _ = ops.pack_sparse_weights(dev(w3))
    out = ops.sparse_conv(dev(x), rule, ops.pack_bf16x3(wt), 32, cp=cp, bias=dev(bias), residual=dev(res), act=2)
    want = scn_ref.conv_direct(x, ref["nbr27"][0], w3, bias=bias, residual=res, relu=True)
    assert np.abs(out.cpu().numpy() - want).max() <= OP_TOL * max(1.0, np.abs(want).max())
    wt, _, cp, k2 = ops.pack_sparse_weights(dev(w3), extra=dev(w2))
    packed = ops.pack_bf16x3(wt)
    out = ops.sparse_conv(dev(x), rule, packed, 32, cp=cp, a2=dev(x2), k2=k2)
    want = scn_ref.conv_direct(x, ref["nbr27"][0], w3, x2=x2, w2=w2)
    assert k2 == 64 and np.abs(out.cpu().numpy() - want).max() <= OP_TOL * max(1.0, np.abs(want).max())
    assert torch.equal(out, ops.sparse_conv(dev(x), rule, packed, 32, cp=cp, a2=dev(x2), k2=k2))


def test_bn_relu_rows():
    from ml3d import ops
    rng = np.random.default_rng(2)
    x, s, t = rng.normal(size=(333, 48)).astype(np.float32), rng.normal(size=48).astype(np.float32), rng.normal(size=48).astype(np.float32)
    buf = torch.zeros((333, 64), device=DEV)
    ops.scn_bn_relu(dev(x), dev(s), dev(t), out=buf[:, :48])
    assert np.array_equal(buf[:, :48].cpu().numpy(), np.maximum(x * s + t, 0)) and not buf[:, 48:].any()


def _golden_forward(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    mcfg = json.loads(str(g["model_json"]))
    m = _model(mcfg, int(g["weights_seed"]), float(g["weight_gain"]))
    pts, fts = scn_ref.golden_inputs(g["clouds"], float(g["room_voxel_size"]))
    assert abs(np.concatenate(pts).astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    return g, mcfg, m, dict(point=[dev(p) for p in pts], feat=[dev(f) for f in fts], batch_lengths=[len(p) for p in pts])


@pytest.mark.parametrize("name", ["sparseconvunet_small", "sparseconvunet_scannet"])
def test_golden_of_the_reference_forward(golden_dir, name):
    g, mcfg, m, inp = _golden_forward(golden_dir, name)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g["state_shapes"]]
    out = m(inp)
    torch.cuda.synchronize()
    assert m.last_pyramid.read_counts() == g["level_counts"].tolist()
    out = out.cpu().numpy()
    n = sum(inp["batch_lengths"])
    assert out.shape == (n, int(mcfg["num_classes"]))
    stride, scale = int(g["logit_stride"]), float(g["logit_scale"])
    tol = tol_for(scale)
    err = float(np.abs(out[::stride] - g["logits"]).max())
    agree, flipped = flips(out, g["labels"].astype(np.int64))
    record(name, yaml=name, model="SparseConvUnet", tolerance=tol, max_abs_delta=err, ref_abs_max=scale, label_agreement=agree,
           flipped_margins=[float(v) for v in flipped], points=n)
    print("%s: max |d logit| = %.3g (tolerance %.3g, logit scale %.2f), label agreement %.6f" % (name, err, tol, scale, agree))
    assert err <= tol
    # (margins are stored as float16, rounded to nearest: 1e-3 relative covers the rounding)
    sure = g["margins"].astype(np.float64) * (1 - 1e-3) > 2 * tol
    assert np.array_equal(out.argmax(1)[sure], g["labels"].astype(np.int64)[sure])


def test_native_against_the_torch_formulation_on_a_real_valued_room(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, "sparseconvunet_small.npz"))
    for mcfg in (json.loads(str(g["model_json"])),
                 dict(json.loads(str(g["model_json"])), residual_blocks=True, conv_block_reps=1, multiplier=32)):
        m = _model(mcfg, int(g["weights_seed"]), 1.6)
        p, f = scn_ref.room(91, 6000, voxel_size=0.1, lattice=False)
        inp = dict(point=[dev(p)], feat=[dev(f)])
        native = m(inp)
        monkeypatch.setenv("ML3D_SCN_OPS", "torch")
        other = m(inp)
        monkeypatch.delenv("ML3D_SCN_OPS")
        scale = float(other.abs().max())
        err = float((native - other).abs().max())
        print("native against torch ops (residual_blocks=%s): max |d| = %.3g at logit scale %.2f" % (mcfg["residual_blocks"], err, scale))
        assert native.shape == (6000, 20) and scale > 0.1 and err <= tol_for(scale)
        assert torch.equal(native, m(inp))                      # the same input gives the same bits


def test_forward_makes_at_most_one_device_to_host_synchronisation(golden_dir):
    g, mcfg, m, inp = _golden_forward(golden_dir, "sparseconvunet_small")
    first = m(inp)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            second = m(inp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) <= 1, [str(w.message) for w in syncs]
    assert torch.equal(first, second)


def test_data_path_returns_one_label_per_input_point():
    mcfg = dict(name="SparseConvUnet", multiplier=16, voxel_size=0.05, conv_block_reps=1, residual_blocks=True, num_classes=20,
                seed=3)
    m = _model(mcfg, 9, 1.6)
    import pt_ref
    n = 5000
    cloud = dict(point=pt_ref.room(33, n), feat=pt_ref.colours(33, n).astype(np.float32) * 2 - 1, label=np.zeros(n, np.int32))
    m.inference_begin(cloud)
    data = m.inference_preprocess()
    assert data["batch_lengths"] == [n] and data["point"].shape == (n, 3)
    assert torch.equal(data["point"], torch.floor(data["point"]) + 0.5) and 0 <= float(data["point"].min()) and float(data["point"].max()) < 4096
    batch = m.make_batch(data)
    out = m(batch)
    res = m.inference_end(batch, out)
    assert res["predict_labels"].shape == (n,) and res["predict_scores"].shape == (n, 20)
    assert np.allclose(res["predict_scores"].sum(1), 1.0, atol=1e-5)
    assert np.array_equal(res["predict_labels"], out.argmax(1).cpu().numpy())
