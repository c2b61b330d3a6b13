"""CPU restatements of the PointRCNN stage-1 contracts of include/ml3d_hip.h ("PointRCNN stage 1") in numpy, operation for
operation: ``decode`` = the reference's ``decode_bbox_target`` (point_rcnn.py:1153-1272) in float64 or float32 (one rounding per
operation, the reference's order), ``proposals`` = ``ProposalLayer.forward`` with ``post_process=True`` + ``distance_based_proposal``
(:1020-1150) with the repository's CPU oracle for ``nms``.  tools/gen_golden_pointrcnn.py ASSERTS that these, fed the reference's
own cls / reg / xyz, reproduce the reference's rois bit for bit and in order; they then judge the product where the reference does
not exist.  The ``wrong`` switches are the deliberately wrong forms of tests/test_prcnn_cases_can_fail.py.  Also the pseudo-trained
weights of the model goldens."""
import numpy as np

import pn2_ref

WRONG_DECODE = ("last_max", "z_res_from_x", "no_wrap")
CLS_GAIN = 3.0
WRONG_PROPOSALS = ("fallback_from_0", "zone_ge_0", "cut_before_nms", "no_padding")


def reg_channels(loc_scope, loc_bin_size, num_head_bin, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5, loc_y_bin_size=0.25):
    per_loc = int(loc_scope / loc_bin_size) * 2
    return per_loc * (4 if get_xz_fine else 2) + (int(loc_y_scope / loc_y_bin_size) * 4 if get_y_by_bin else 1) + num_head_bin * 2 + 3


def _argmax(a, wrong):
    if "last_max" in wrong:
        return a.shape[1] - 1 - np.argmax(a[:, ::-1], 1)
    return np.argmax(a, 1)                                       # the first maximum


def decode(roi, pred_reg, anchor_size, loc_scope, loc_bin_size, num_head_bin, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
           loc_y_bin_size=0.25, get_ry_fine=False, dtype=np.float32, wrong=(), detail=None):
    """-> [n, 7] in ``dtype``.  float32: every python scalar becomes a float32 scalar first, as torch does for a float32 tensor.
    ``detail`` (a dict) receives the argmax margins and the heading before the wrap, for the robustness assertions."""
    T = dtype
    roi, reg, anchor = np.asarray(roi, T), np.asarray(pred_reg, T), np.asarray(anchor_size, T)
    L = int(loc_scope / loc_bin_size) * 2
    Y = int(loc_y_scope / loc_y_bin_size) * 2
    H = int(num_head_bin)
    assert reg.shape[1] == reg_channels(loc_scope, loc_bin_size, H, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size)
    rows = np.arange(len(reg))
    margins = []

    def amax(lo, width):
        seg = reg[:, lo:lo + width]
        if width > 1:
            top = np.sort(seg.astype(np.float64), 1)
            margins.append(top[:, -1] - top[:, -2])
        return _argmax(seg, wrong)

    x_bin, z_bin = amax(0, L), amax(L, L)
    pos_x = x_bin.astype(T) * T(loc_bin_size) + T(loc_bin_size / 2) - T(loc_scope)
    pos_z = z_bin.astype(T) * T(loc_bin_size) + T(loc_bin_size / 2) - T(loc_scope)
    off = 2 * L
    if get_xz_fine:
        pos_x = pos_x + reg[rows, 2 * L + x_bin] * T(loc_bin_size)
        pos_z = pos_z + reg[rows, (2 * L if "z_res_from_x" in wrong else 3 * L) + z_bin] * T(loc_bin_size)
        off = 4 * L
    if get_y_by_bin:
        y_bin = amax(off, Y)
        y_res = reg[rows, off + Y + y_bin] * T(loc_y_bin_size)
        pos_y = y_bin.astype(T) * T(loc_y_bin_size) + T(loc_y_bin_size / 2) - T(loc_y_scope) + y_res
        pos_y = pos_y + roi[:, 1]
        off += 2 * Y
    else:
        pos_y = roi[:, 1] + reg[:, off]
        off += 1
    ry_bin = amax(off, H)
    ry_norm = reg[rows, off + H + ry_bin]
    if get_ry_fine:
        apc = (np.pi / 2) / H
        ry = (ry_bin.astype(T) * T(apc) + T(apc / 2)) + ry_norm * T(apc / 2) - T(np.pi / 4)
        raw = None
    else:
        apc = (2 * np.pi) / H
        raw = ry_bin.astype(T) * T(apc) + ry_norm * T(apc / 2)
        ry = np.mod(raw, T(2 * np.pi))
        if "no_wrap" not in wrong:
            ry = np.where(ry > T(np.pi), ry - T(2 * np.pi), ry)
    hwl = reg[:, off + 2 * H:off + 2 * H + 3] * anchor + anchor
    if roi.shape[1] == 7:
        ang = -roi[:, 6]
        ca, sa = np.cos(ang).astype(T), np.sin(ang).astype(T)
        pos_x, pos_z = pos_x * ca - pos_z * sa, pos_x * sa + pos_z * ca
        ry = ry + roi[:, 6]
    if detail is not None:
        detail["margin"] = np.min(np.stack(margins), 0) if margins else np.full(len(reg), np.inf)
        detail["ry_raw"] = None if raw is None else raw.astype(np.float64)
    out = np.stack((pos_x + roi[:, 0], pos_y, pos_z + roi[:, 2], hwl[:, 0], hwl[:, 1], hwl[:, 2], ry), 1)
    return np.ascontiguousarray(out, T)


def wrap_distance(ry_raw):
    """float64 heading before ``% 2 pi``: its distance from the nearest place where the wrap decides (a multiple of 2 pi for the
    remainder, pi + a multiple of 2 pi for ``ry > pi``) = the distance from a multiple of pi."""
    r = np.mod(np.asarray(ry_raw, np.float64), np.pi)
    return np.minimum(r, np.pi - r)


def bev_of(boxes):
    """xywhr_to_xyxyr(boxes[:, [0, 2, 3, 5, 6]]) (objdet_helper.py:69-87) in float32."""
    b = np.asarray(boxes, np.float32)
    half_w, half_h = b[:, 3] / np.float32(2), b[:, 5] / np.float32(2)
    return np.ascontiguousarray(np.stack((b[:, 0] - half_w, b[:, 2] - half_h, b[:, 0] + half_w, b[:, 2] + half_h, b[:, 6]), 1), np.float32)


def _oracle_nms(bev, scores, thr):
    from oracle import ops as oops
    return oops.nms(bev, scores, thr)


def zone_candidates(scores, boxes, nms_pre, wrong=(), with_next=False):
    """One item -> (order, [near candidate positions, far candidate positions]) as positions INTO the score order; ``with_next``:
    also, per zone, the position that would have been taken next (or None)."""
    order = np.argsort(-np.asarray(scores, np.float32), kind="stable")
    dist = np.asarray(boxes, np.float32)[order, 2]
    lo0 = (dist >= 0) if "zone_ge_0" in wrong else (dist > 0)
    first = lo0 & (dist <= 40.0)
    second = (dist > 40.0) & (dist <= 80.0)
    pre = [int(nms_pre * 0.7), nms_pre - int(nms_pre * 0.7)]
    near = np.flatnonzero(first)
    if second.any():
        far, lo = np.flatnonzero(second), 0
    else:
        far, lo = near, (0 if "fallback_from_0" in wrong else pre[0])
    zones = [near[:pre[0]], far[lo:lo + pre[1]]]
    if not with_next:
        return order, zones
    return order, zones, [near[pre[0]] if len(near) > pre[0] else None, far[lo + pre[1]] if len(far) > lo + pre[1] else None]


def proposals(scores, boxes, nms_pre, nms_post, nms_thres, nms=None, wrong=(), out=None):
    """``scores`` [B, N], ``boxes`` [B, N, 7] (decoded, y NOT yet moved) -> (rois [B, nms_post, 7], roi_scores [B, nms_post],
    roi_index int32 [B, nms_post]).  An empty near zone contributes no rows (the reference asserts there)."""
    nms = nms or _oracle_nms
    scores, boxes = np.asarray(scores, np.float32), np.array(boxes, np.float32, copy=True)
    boxes[..., 1] += boxes[..., 3] / np.float32(2)
    b = scores.shape[0]
    if out is None or "no_padding" not in wrong:
        rois, roi_scores = np.zeros((b, nms_post, 7), np.float32), np.zeros((b, nms_post), np.float32)
        roi_index = np.full((b, nms_post), -1, np.int32)
    else:
        rois, roi_scores, roi_index = (np.array(o, copy=True) for o in out)
    post = [int(nms_post * 0.7), nms_post - int(nms_post * 0.7)]
    for k in range(b):
        order, zones = zone_candidates(scores[k], boxes[k], nms_pre, wrong)
        at = 0
        for z, pos in enumerate(zones):
            if "cut_before_nms" in wrong:
                pos = pos[:post[z]]
            if len(pos) == 0:
                continue
            src = order[pos]
            keep = np.asarray(nms(bev_of(boxes[k][src]), scores[k][src], nms_thres), np.int64)[:post[z]]
            m = len(keep)
            rois[k, at:at + m], roi_scores[k, at:at + m], roi_index[k, at:at + m] = boxes[k][src[keep]], scores[k][src[keep]], src[keep]
            at += m
    return rois, roi_scores, roi_index


def rpn_stage(cls, reg, xyz, head, nms=None):
    """The restated stage 1 behind the heads: cls [B, N, 1], reg [B, N, C], xyz [B, N, 3] and the ``rpn.head`` settings (eval: the
    ``_val`` settings when given) -> (rois, roi_scores, roi_index, decoded boxes [B, N, 7])."""
    b, n = cls.shape[:2]
    boxes = decode(np.asarray(xyz, np.float32).reshape(b * n, 3), np.asarray(reg, np.float32).reshape(b * n, -1), head["mean_size"],
                   head.get("loc_scope", 3.0), head.get("loc_bin_size", 0.5), head.get("num_head_bin", 12), head.get("loc_xz_fine", True),
                   head.get("get_y_by_bin", False), head.get("loc_y_scope", 0.5), head.get("loc_y_bin_size", 0.25),
                   head.get("get_ry_fine", False)).reshape(b, n, 7)
    post = head.get("nms_post_val") if head.get("nms_post_val") is not None else head.get("nms_post", 512)
    thr = head.get("nms_thres_val") if head.get("nms_thres_val") is not None else head.get("nms_thres", 0.85)
    return proposals(np.asarray(cls, np.float32)[:, :, 0], boxes, head.get("nms_pre", 9000), post, thr, nms) + (boxes,)


# ---- inputs of the model goldens (tools/gen_golden_pointrcnn.py writes with them, the tests rebuild them) -----------------------------
def make_state_dict(keys, shapes, seed):
    """Pseudo-trained parameters for the reference's WHOLE layout: the backbone's (``rpn.backbone.*``) by ``pn2_ref.make_state_dict``
    (same seed), everything else in the same style -- conv weights (3-d Conv1d, 4-d Conv2d) uniform in +-2.45 / sqrt(fan_in),
    BatchNorm scales in +-[0.6, 1.5] (a fifth negative), biases / shifts N(0, 0.2), running means N(0, 0.1), variances in [0.5, 1.5].
    The LAST convolution of the RPN's classification head takes ``CLS_GAIN`` times that weight range: with the plain range a
    cloud's scores crowd within about one unit (a narrow head behind interpolated features), with it they spread over several, as
    a trained network's do."""
    import torch
    bb = [(k, s) for k, s in zip(keys, shapes) if k.startswith("rpn.backbone.")]
    sd_bb = pn2_ref.make_state_dict([k[len("rpn.backbone."):] for k, _ in bb], [s for _, s in bb], seed)
    rng = np.random.default_rng([int(seed), 0x5243])
    cls_last = {k for k in keys if k.startswith("rpn.cls_blocks.") and k.endswith(".weight") and k[:-6] + "bias" in keys and
                k[:-6] + "running_mean" not in keys}
    sd = {}
    for k, shape in zip(keys, shapes):
        shape = tuple(int(v) for v in shape)
        if k.startswith("rpn.backbone."):
            sd[k] = sd_bb[k[len("rpn.backbone."):]]
            continue
        if k.endswith("num_batches_tracked"):
            v = np.asarray(1, np.int64)
        elif k.endswith("running_mean"):
            v = rng.normal(0, 0.1, shape)
        elif k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("bias"):
            v = rng.normal(0, 0.2, shape)
        elif len(shape) >= 3:
            v = rng.uniform(-1, 1, shape) * 2.45 / np.sqrt(shape[1]) * (CLS_GAIN if k in cls_last else 1.0)
        else:
            v = rng.uniform(0.6, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1, 1)
        sd[k] = torch.from_numpy(np.asarray(v, np.int64 if k.endswith("num_batches_tracked") else np.float32))
    return sd


def make_points(seeds, n, in_channels, scale, offsets):
    """[B, n, 3 + in_channels] float32: per item a room of tests/pt_ref.py scaled and moved by its OWN offset (the z offset decides
    the zones), features uniform in [0, 1) -- ``pn2_ref.make_pointcloud`` with an offset per item."""
    return np.concatenate([pn2_ref.make_pointcloud([s], n, in_channels, scale, o) for s, o in zip(seeds, offsets)])
