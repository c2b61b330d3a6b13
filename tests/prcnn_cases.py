"""Shared bodies of the PointRCNN stage-1 tests: tests/test_emulated_pointrcnn_ops.py / test_emulated_pointrcnn.py run them on
CPU tensors against the host emulation of csrc/pointrcnn.hip, tests/test_gpu_pointrcnn_ops.py / test_gpu_pointrcnn.py on the
MI355X, tests/test_prcnn_cases_can_fail.py against deliberately wrong stand-ins (every op body takes the implementation under
test as ``impl``; None = the product's ``ml3d.ops``).

Decode: floats judged by ``pt_cases.judge`` against the float64 formula of tests/prcnn_ref.py within max(1e-5, 4 e32); on the
float64 side every argmax is either an EXACT tie (integers) or decided by at least 1e-3, and no heading lies within 1e-4 of a
wrap.  Proposals: compared for EQUALITY with the restatement -- order, indices, box bits.  Model: tests/golden/pointrcnn_rpn_*.npz
(tools/gen_golden_pointrcnn.py: the REAL reference on PyTorch-CPU)."""
import itertools
import json
import os

import numpy as np
import torch

import prcnn_ref
from pt_cases import _print, judge, refused, same_bits

ANCHOR = (1.52563191462, 1.62856739989, 3.88311640418)
DECODE_N = (1, 63, 64, 65, 257)
DECODE_BINS = ((3.0, 0.5, 12), (1.5, 0.5, 9))              # (loc_scope, loc_bin_size, num_head_bin)
Y_BINS = (0.5, 0.25)
FLAGS = tuple(itertools.product((False, True), repeat=3))  # (get_xz_fine, get_y_by_bin, get_ry_fine)

PROP_N = (1, 64, 65, 700, 5000)
PROP_PRE_POST = ((10, 4), (3, 1), (9000, 100))
PROP_KINDS = ("far_empty", "near_empty", "both_empty", "all_suppressed", "none_suppressed", "tied")
PROP_THRES = 0.5


def _ops(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- decode -------------------------------------------------------------------------------------------------------------------------
def decode_inputs(n, bins, flags, width):
    """reg [n, C]: per segment a designated winner; rows 0, 3, 6, ... hold an EXACT integer tie between the winner and a LATER bin,
    the others win by 0.01 .. 3.  Heading winners run down from the last bin (row 0 lies past the ``ry > pi`` wrap), residuals keep
    0.05 away from 0, so no heading comes near a multiple of pi."""
    scope, bin_size, H = bins
    xz, yb, ryf = flags
    rng = np.random.default_rng([n, H, int(xz), int(yb), int(ryf), width])
    L, Y = int(scope / bin_size) * 2, int(Y_BINS[0] / Y_BINS[1]) * 2
    C = prcnn_ref.reg_channels(scope, bin_size, H, xz, yb, *Y_BINS)
    reg = rng.normal(0, 1.5, (n, C)).astype(np.float32)
    segs = [(0, L), (L, L)]
    off = 4 * L if xz else 2 * L
    if yb:
        segs.append((off, Y))
        off += 2 * Y
    else:
        off += 1
    segs.append((off, H))
    ry_res = off + H
    for lo, w in segs:
        for i in range(n):
            win = (w - 1 - i) % w if lo == off else int(rng.integers(0, w))
            top = float(np.ceil(reg[i, lo:lo + w].max())) + 1.0
            if i % 3 == 0:
                win = min(win, w - 2)                               # (a later bin must exist to tie with)
                reg[i, lo + win] = top
                reg[i, lo + int(rng.integers(win + 1, w))] = top
            else:
                reg[i, lo + win] = np.float32(top - 1.0 + rng.uniform(0.01, 3.0))
    sign = np.where(rng.random((n, H)) < 0.5, -1.0, 1.0)
    reg[:, ry_res:ry_res + H] = (sign * rng.uniform(0.05, 0.95, (n, H))).astype(np.float32)
    roi = np.concatenate((rng.uniform(-30, 30, (n, 3)), np.abs(rng.normal(2, 0.5, (n, 3))), rng.uniform(-3.1, 3.1, (n, 1))), 1).astype(np.float32)
    return np.ascontiguousarray(roi[:, :width]), reg


def run_decode(dev, impl, roi, reg, bins, flags):
    scope, bin_size, H = bins
    xz, yb, ryf = flags
    reg = reg if torch.is_tensor(reg) else _t(reg, dev)
    return _ops(impl).bin_decode(_t(roi, dev), reg, ANCHOR, scope, bin_size, H, xz, yb, Y_BINS[0], Y_BINS[1], ryf)


def check_decode(dev, n, bins, impl=None, report=_print):
    """All 8 flag combinations x both roi widths at one (n, bin set): against float64; a strided ``pred_reg`` gives the same bits."""
    scope, bin_size, H = bins
    sides = set()
    for flags, width in itertools.product(FLAGS, (3, 7)):
        roi, reg = decode_inputs(n, bins, flags, width)
        kw = dict(get_xz_fine=flags[0], get_y_by_bin=flags[1], loc_y_scope=Y_BINS[0], loc_y_bin_size=Y_BINS[1], get_ry_fine=flags[2])
        detail = {}
        r64 = prcnn_ref.decode(roi, reg, ANCHOR, scope, bin_size, H, dtype=np.float64, detail=detail, **kw)
        r32 = prcnn_ref.decode(roi, reg, ANCHOR, scope, bin_size, H, dtype=np.float32, **kw)
        m = detail["margin"]
        assert bool(((m == 0) | (m >= 1e-3)).all()), "every argmax an exact tie or decided by 1e-3"
        assert (m[::3] == 0).all(), "the tie rows"
        if detail["ry_raw"] is not None:
            assert prcnn_ref.wrap_distance(detail["ry_raw"]).min() >= 1e-4, "no heading within 1e-4 of a wrap"
            wrapped = np.mod(detail["ry_raw"], 2 * np.pi) > np.pi
            sides |= set(wrapped.tolist())
            assert wrapped[0], "row 0 lies past the wrap"
        name = "decode n=%d bins=%s flags=%s width=%d" % (n, bins, "".join(str(int(f)) for f in flags), width)
        got = run_decode(dev, impl, roi, reg, bins, flags).cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 7)
        judge(report, name, got, torch.from_numpy(r64), torch.from_numpy(r32))
        wide = torch.full((n, reg.shape[1] + 9), 55.0, dtype=torch.float32)
        wide[:, 4:4 + reg.shape[1]] = torch.from_numpy(reg)
        again = run_decode(dev, impl, roi, wide.to(dev)[:, 4:4 + reg.shape[1]], bins, flags).cpu()
        assert same_bits(again, got), (name, "strided pred_reg")
    assert n < 63 or sides == {True, False}, "rows on both sides of the wrap"


def check_decode_refusals(dev):
    """A channel count the flags do not imply is refused: by the wrapper, and by the entry point itself (ML3D_E_INVALID, before any
    launch: the output keeps its fill)."""
    from ml3d import _abi, ops
    from ml3d.ops import _gates
    roi, reg = decode_inputs(5, DECODE_BINS[0], (True, False, False), 3)
    refused(lambda: run_decode(dev, None, roi, reg[:, :-1], DECODE_BINS[0], (True, False, False)), "C - 1 columns")
    refused(lambda: run_decode(dev, None, roi, reg, DECODE_BINS[0], (False, False, False)), "C of another flag set")
    refused(lambda: run_decode(dev, None, roi, reg, DECODE_BINS[1], (True, False, False)), "C of another bin set")
    refused(lambda: ops.bin_decode(_t(roi, dev)[:, :2].contiguous(), _t(reg, dev), ANCHOR, 3.0, 0.5, 12), "roi width 2")
    out = torch.full((5, 7), -7.0, dtype=torch.float32, device=dev)
    anchor = np.asarray(ANCHOR, np.float32)
    r, g = _t(roi, dev), _t(reg, dev)
    with torch.cuda.device(dev):
        rc = _abi.get().ml3d_bin_decode(r.data_ptr(), 3, g.data_ptr(), reg.shape[1], reg.shape[1] - 1, 5, anchor.ctypes.data, 3.0, 0.5, 12,
                                        0.5, 0.25, 1, 0, 0, out.data_ptr(), _gates._stream())
    assert rc == -1 and bool((out.cpu() == -7.0).all()), rc


# ---- proposals ----------------------------------------------------------------------------------------------------------------------
def proposal_inputs(b, n, kind, seed=0):
    """scores [b, n] (integers: a permutation -- tie-free -- or, kind "tied", drawn with repeats), boxes [b, n, 7]: car-sized boxes
    on a 20 m wide strip, depth by ``kind``.  "both": depths over both zones, and rows 0 / 1 / 2 of every item at EXACTLY z = 0, 40
    and 80 with the three highest scores."""
    rng = np.random.default_rng([b, n, PROP_KINDS.index(kind) if kind in PROP_KINDS else 99, seed])
    z_range = dict(both=(2.0, 78.0), far_empty=(2.0, 39.5), near_empty=(40.5, 79.5), both_empty=(80.5, 120.0)).get(kind, (2.0, 78.0))
    boxes = np.zeros((b, n, 7), np.float32)
    boxes[..., 0] = rng.uniform(-10, 10, (b, n))
    boxes[..., 1] = rng.uniform(0.5, 2.0, (b, n))
    boxes[..., 2] = rng.uniform(*z_range, (b, n))
    boxes[..., 3:6] = np.asarray(ANCHOR, np.float32) * rng.uniform(0.8, 1.25, (b, n, 3)).astype(np.float32)
    boxes[..., 6] = rng.uniform(-np.pi, np.pi, (b, n))
    if kind == "both_empty":
        boxes[:, ::2, 2] *= -1
    if kind == "all_suppressed":                              # one box per zone, copied: only each zone's first candidate survives
        far = boxes[..., 2] > 40
        boxes[:] = np.where(far[..., None], np.float32([1, 1, 60, 1.5, 1.6, 3.9, 0.3]), np.float32([1, 1, 20, 1.5, 1.6, 3.9, 0.3]))
    if kind == "none_suppressed":                             # 8 m apart in x: no two boxes touch
        boxes[..., 0] = np.arange(n, dtype=np.float32)[None] * 8
    scores = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.float32) - np.float32(n // 2)
    if kind == "tied":
        scores = rng.integers(0, max(n // 8, 2), (b, n)).astype(np.float32)
    if kind == "both" and n >= 3:
        boxes[:, 0, 2], boxes[:, 1, 2], boxes[:, 2, 2] = 0.0, 40.0, 80.0
        top = scores.max(1) + 1
        for i in range(3):
            scores[:, i] = top + 3 - i
    return scores, boxes


def run_proposals(dev, impl, scores, boxes, pre, post, nan_scratch=False):
    """Outputs pre-filled with a sentinel; ``nan_scratch``: the product's scratch arrays arrive filled with 0xFF bytes (NaN)."""
    ops = _ops(impl)
    b = scores.shape[0]
    out = (torch.full((b, post, 7), -7.0, dtype=torch.float32, device=dev), torch.full((b, post), -7.0, dtype=torch.float32, device=dev),
           torch.full((b, post), -9, dtype=torch.int32, device=dev))
    if nan_scratch:
        from ml3d.ops import pointrcnn as mod
        plain = mod._scratch

        def filled(*a):
            ts = plain(*a)
            for t in ts:
                t.view(torch.uint8).fill_(255)
            return ts

        mod._scratch = filled
        try:
            res = ops.rpn_proposals(_t(scores, dev), _t(boxes, dev), pre, post, PROP_THRES, out=out)
        finally:
            mod._scratch = plain
    else:
        res = ops.rpn_proposals(_t(scores, dev), _t(boxes, dev), pre, post, PROP_THRES, out=out)
    return tuple(r.cpu().numpy() for r in res)


def _equal(got, want, what):
    for g, w, part in zip(got, want, ("rois", "roi_scores", "roi_index")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part, g.shape, g.dtype)
        same = np.array_equal(g.view(np.int32), w.view(np.int32))
        assert same, (what, part, np.argwhere(g.view(np.int32) != w.view(np.int32))[:4].tolist())


def check_proposals(dev, n, pre, post, kind="both", batches=(1, 3), impl=None):
    """Equality with the restatement at every batch size, every item equal to its single-item run, scratch full of NaN bytes."""
    for b in batches:
        scores, boxes = proposal_inputs(b, n, kind)
        want = prcnn_ref.proposals(scores, boxes, pre, post, PROP_THRES)
        z = boxes[..., 2]
        near, far = (z > 0) & (z <= 40), (z > 40) & (z <= 80)
        filled = (want[2] >= 0).sum(1)
        if kind == "both" and n >= 64:
            assert near.any(1).all() and far.any(1).all()
            assert (z[:, :3] == np.float32([0, 40, 80])).all()
        if kind == "far_empty":
            assert near.any() and not far.any()
            assert n <= int(pre * 0.7) or (filled > min(int(post * 0.7), int(pre * 0.7))).all() or post - int(post * 0.7) == 0, "the fallback arm adds rows"
        if kind == "near_empty":
            assert far.any() and not near.any() and (filled <= post - int(post * 0.7)).all()
        if kind == "both_empty":
            assert not near.any() and not far.any() and (filled == 0).all()
        if kind == "all_suppressed":
            assert (filled <= 2).all() and (filled >= 1).all()
        if kind == "none_suppressed":
            assert (filled == np.minimum(post, np.minimum(near.sum(1), int(post * 0.7)) + np.minimum(far.sum(1), post - int(post * 0.7)))).all() or pre < post
        if kind == "tied":
            assert len(np.unique(scores)) < scores.size
        if kind in ("all_suppressed", "both_empty", "near_empty"):
            assert (filled < post).all(), "fewer survivors than nms_post: zero rows and -1 indices over the sentinel"
        got = run_proposals(dev, impl, scores, boxes, pre, post, nan_scratch=impl is None)
        _equal(got, want, (n, pre, post, kind, b))
        if b > 1:
            alone = run_proposals(dev, impl, scores[1:2], boxes[1:2], pre, post)
            _equal(alone, tuple(w[1:2] for w in want), (n, pre, post, kind, "item 1 alone"))


def check_proposal_refusals(dev):
    from ml3d import ops
    s, bx = torch.zeros((2, 10), device=dev), torch.zeros((2, 10, 7), device=dev)
    refused(lambda: ops.rpn_proposals(s, bx[:, :9].contiguous(), 10, 4, 0.8), "row count mismatch")
    refused(lambda: ops.rpn_proposals(s, bx[..., :6].contiguous(), 10, 4, 0.8), "6 box columns")
    refused(lambda: ops.rpn_proposals(s, bx, 70000, 4, 0.8), "nms_pre past the NMS limit")
    refused(lambda: ops.rpn_proposals(s, bx, 10, -1, 0.8), "negative nms_post")
    refused(lambda: ops.rpn_proposals(s.double(), bx, 10, 4, 0.8), "float64 scores")


# ---- the model against the reference's stage 1 ---------------------------------------------------------------------------------------
MODEL_GOLDENS = ("pointrcnn_rpn_small", "pointrcnn_rpn_kitti")


def load_golden(name):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return g, json.loads(str(g["model_json"]))


def build_model(dev, g, mcfg):
    from ml3d.torch.models import PointRCNN
    model = PointRCNN(**mcfg, device=dev)
    sd = model.state_dict()
    keys, shapes = [str(k) for k in g["state_keys"]], [json.loads(str(s)) for s in g["state_shapes"]]
    assert list(sd) == keys and [list(v.shape) for v in sd.values()] == shapes, "the reference's state_dict layout"
    model.load_state_dict(prcnn_ref.make_state_dict(keys, shapes, int(g["weights_seed"])), strict=True)
    return model


def check_model(dev, name, report=_print):
    """State layout and strict load; cls / reg within max(1e-4, 4.4e-6 scale) of the golden on both ``ML3D_PRCNN_OPS`` paths; the
    small case's proposals against the golden directly (same ``roi_index`` order, boxes within 4 x that tolerance: the largest
    coefficient of a box coordinate in ``reg`` is the anchor length 3.88 < 4, xyz passes through exactly); for both cases the rois
    equal to the restatement applied to the product's OWN cls / reg / xyz (order and index exact, boxes within 1e-5)."""
    g, mcfg = load_golden(name)
    model = build_model(dev, g, mcfg)
    head = mcfg["rpn"]["head"]
    pts = prcnn_ref.make_points(g["cloud_seeds"], int(g["n"]), int(mcfg["rpn"]["backbone"]["in_channels"]), float(g["cloud_scale"]),
                                g["cloud_offsets"])
    assert abs(pts.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    scale, stride = float(g["scale"]), int(g["row_stride"])
    tol = max(1e-4, 4.4e-6 * scale)
    for mode in ("hip", "torch"):
        os.environ["ML3D_PRCNN_OPS"] = mode
        try:
            r = model.proposals(_t(pts, dev))
        finally:
            del os.environ["ML3D_PRCNN_OPS"]
        r = {k: v.cpu().numpy() for k, v in r.items()}
        assert np.array_equal(r["xyz"], pts[..., :3])
        for part in ("cls", "reg"):
            got = r[part][:, ::stride]
            err = float(np.abs(got - g[part]).max())
            report(name="%s %s %s" % (name, mode, part), max_abs_delta=err, tol=tol, scale=scale)
            assert got.shape == g[part].shape and bool(np.isfinite(got).all()) and err <= tol, (name, mode, part, err, tol)
        post = r["rois"].shape[1]
        assert r["rois"].shape == g["rois"].shape and r["roi_index"].dtype == np.int32 and r["roi_scores"].shape == (len(pts), post)
        if name == MODEL_GOLDENS[0]:
            assert np.array_equal(r["roi_index"], g["roi_index"]), (name, mode, "roi order against the golden")
            err = float(np.abs(r["rois"] - g["rois"]).max())
            report(name="%s %s rois" % (name, mode), max_abs_delta=err, tol=4 * tol)
            assert err <= 4 * tol and float(np.abs(r["roi_scores"] - g["roi_scores"]).max()) <= tol, (name, mode, err)
        want = prcnn_ref.rpn_stage(r["cls"], r["reg"], r["xyz"], head)
        assert np.array_equal(r["roi_index"], want[2]), (name, mode, "roi order against the restatement on the product's own heads")
        err = float(np.abs(r["rois"] - want[0]).max())
        report(name="%s %s rois vs restatement" % (name, mode), max_abs_delta=err, tol=1e-5)
        assert err <= 1e-5 and np.array_equal(r["roi_scores"], want[1]), (name, mode, err)
        pad = r["roi_index"] < 0
        assert not r["rois"][pad].any() and not r["roi_scores"][pad].any()


def check_model_modes(dev):
    """``mode="RPN"`` returns exactly the reference's three keys; ``mode="RCNN"`` forward and ``.train()`` are refused."""
    g, mcfg = load_golden(MODEL_GOLDENS[0])
    model = build_model(dev, g, mcfg)
    pts = prcnn_ref.make_points(g["cloud_seeds"], int(g["n"]), int(mcfg["rpn"]["backbone"]["in_channels"]), float(g["cloud_scale"]),
                                g["cloud_offsets"])

    class Batch:
        point = [_t(p, dev) for p in pts]

    out = model(Batch())
    assert sorted(out) == ["cls", "reg", "rois"]
    assert tuple(out["cls"].shape) == (2, int(g["n"]), 1) and out["reg"].shape[:2] == out["cls"].shape[:2] and out["rois"].shape[2] == 7
    both = model.proposals(_t(pts, dev))
    assert same_bits(out["rois"], both["rois"])
    alone = model.proposals(_t(pts[:1], dev))                    # a single cloud: the same proposals as inside the batch
    assert torch.equal(alone["roi_index"], both["roi_index"][:1]) and float((alone["rois"] - both["rois"][:1]).abs().max()) <= 1e-4
    for fn in (model.train, lambda: model.train(True)):
        try:
            fn()
        except NotImplementedError as e:
            assert "inference only" in str(e)
        else:
            raise AssertionError(".train() was accepted")
    assert model.eval() is model and not model.training
    rcnn = build_model(dev, g, dict(mcfg, mode="RCNN"))
    try:
        rcnn(Batch())
    except NotImplementedError as e:
        assert "RoI stage" in str(e) and "proposals()" in str(e)
    else:
        raise AssertionError("mode='RCNN' forward ran")
    assert "rois" in rcnn.proposals(_t(pts, dev))
