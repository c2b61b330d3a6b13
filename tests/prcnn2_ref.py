"""CPU restatement of the ``ml3d_roi_pool`` contract of include/ml3d_hip.h ("PointRCNN stage 2, the pooling") in numpy, operation
for operation: ``roipool3d_gpu`` (roipool3d_utils.py:24: ``enlarge_box3d`` + the open3d wheel's ``roi_pool``), the two extra
per-point columns and the canonical transform of ``RCNN.forward`` (point_rcnn.py:848-887), in float64 or float32 (one rounding
per operation).  The wheel is not available to this project: for its op THIS FILE is the oracle, with the semantics of the
PointRCNN ``roipool3d`` kernel the wheel's op was taken from.  The ``wrong`` switches are the deliberately wrong forms of
tests/test_prcnn2_cases_can_fail.py."""
import numpy as np

WRONG_POOL = ("open_faces", "zero_fill", "cy_plus", "rot_sign", "transform_enlarged", "no_prefilter", "empty_unflagged",
              "empty_depth")
PREFILTER = 10.0


def enlarge(rois, extra_width, T=np.float32):
    """``enlarge_box3d``: [..., 7] -> a copy with h, w, l + 2 * extra_width and y + extra_width."""
    big = np.array(rois, T, copy=True)
    big[..., 3:6] = big[..., 3:6] + T(2.0 * extra_width)
    big[..., 1] = big[..., 1] + T(extra_width)
    return big


def box_terms(pts, box, T=np.float32, wrong=()):
    """One ENLARGED box against pts [n, 3] -> the five decision quantities, each ``value - bound`` style pairs:
    (|dx|, |dy|, |dz|, xr, zr) and the bounds (10, h / 2, 10, l / 2, w / 2)."""
    pts, box = np.asarray(pts, T), np.asarray(box, T)
    x, y, z, h, w, l, ry = (box[i] for i in range(7))
    half = h / T(2)
    cy = y + half if "cy_plus" in wrong else y - half
    dx, dy, dz = pts[:, 0] - x, pts[:, 1] - cy, pts[:, 2] - z
    ca, sa = T(np.cos(ry)), T(np.sin(ry))
    xr = dx * ca + dz * (-sa)
    zr = dx * sa + dz * ca
    return (np.abs(dx), np.abs(dy), np.abs(dz), xr, zr), (T(PREFILTER), half, T(PREFILTER), l / T(2), w / T(2))


def in_box(pts, box, T=np.float32, wrong=()):
    (adx, ady, adz, xr, zr), (pre, hh, _, hl, hw) = box_terms(pts, box, T, wrong)
    with np.errstate(invalid="ignore"):
        rejected = ady > hh
        if "no_prefilter" not in wrong:
            rejected = rejected | (adx > pre) | (adz > pre)
        if "open_faces" in wrong:
            inside = (xr > -hl) & (xr < hl) & (zr > -hw) & (zr < hw)
        else:
            inside = (xr >= -hl) & (xr <= hl) & (zr >= -hw) & (zr <= hw)
    return inside & ~rejected


def margins(pts, box):
    """float64 distance of every point from every place where ``in_box`` decides: the prefilter, the y range, the four faces."""
    (adx, ady, adz, xr, zr), (pre, hh, _, hl, hw) = box_terms(pts, box, np.float64)
    return np.minimum.reduce((np.abs(adx - pre), np.abs(ady - hh), np.abs(adz - pre), np.abs(np.abs(xr) - hl), np.abs(np.abs(zr) - hw)))


def decisive_margins(pts, box):
    """float64: how far every point is from CHANGING SIDES of ``in_box`` -- an inside point leaves through its nearest bound, an
    outside point enters only when every test it fails turns, so its largest violation counts."""
    (adx, ady, adz, xr, zr), (pre, hh, _, hl, hw) = box_terms(pts, box, np.float64)
    slack = np.stack((pre - adx, hh - ady, pre - adz, hl - np.abs(xr), hw - np.abs(zr)))
    return np.where((slack >= 0).all(0), slack.min(0), (-slack).max(0))


def wheel_roi_pool(xyz, boxes, feat, num_points):
    """The open3d wheel's ``roi_pool(pts [B, N, 3], boxes [B, M, 7] ALREADY enlarged, feat [B, N, C], S)`` in float32 ->
    (pooled [B, M, S, 3 + C] = xyz | feat of the pooled points, zero rows for an empty box; empty int32 [B, M])."""
    xyz, boxes, feat = np.asarray(xyz, np.float32), np.asarray(boxes, np.float32), np.asarray(feat, np.float32)
    B, M, S = boxes.shape[0], boxes.shape[1], int(num_points)
    pooled = np.zeros((B, M, S, 3 + feat.shape[2]), np.float32)
    empty = np.zeros((B, M), np.int32)
    for b in range(B):
        for m in range(M):
            hits = np.flatnonzero(in_box(xyz[b], boxes[b, m]))[:S]
            if len(hits) == 0:
                empty[b, m] = 1
                continue
            idx = hits[np.arange(S) % len(hits)]
            pooled[b, m] = np.concatenate((xyz[b][idx], feat[b][idx]), 1)
    return pooled, empty


def roi_pool(xyz, feat, scores, rois, num_points, score_thres, extra_width, dtype=np.float32, wrong=(), out=None):
    """xyz [B, N, 3], feat [B * N, C], scores [B, N], rois [B, M, 7] -> (pts_input [B * M, S, 5 + C] in ``dtype``, pool_idx int32
    [B, M, S], empty int32 [B, M], cnt int64 [B, M]: ALL the inside points of a roi, not cut at S).  The decisions (in the box,
    above the threshold) are taken in ``dtype`` as well: the tests' inputs keep every one of them 1e-3 away from its bound."""
    T = dtype
    xyz, scores, rois = np.asarray(xyz, T), np.asarray(scores, T), np.asarray(rois, T)
    feat = np.asarray(feat, np.float32)
    B, N = scores.shape
    M, S, C = rois.shape[1], int(num_points), feat.shape[1]
    big = enlarge(rois, extra_width, T)
    pts_input = np.zeros((B * M, S, 5 + C), T)
    pool_idx = np.full((B, M, S), -1, np.int32)
    empty = np.zeros((B, M), np.int32)
    count = np.zeros((B, M), np.int64)
    for b in range(B):
        for m in range(M):
            hits = np.flatnonzero(in_box(xyz[b], big[b, m], T, wrong))
            count[b, m] = len(hits)
            row = pts_input[b * M + m]
            box = big[b, m] if "transform_enlarged" in wrong else rois[b, m]
            if len(hits) == 0:
                if "empty_unflagged" not in wrong:
                    empty[b, m] = 1
                p = np.zeros((S, 3), T)
                if "empty_depth" in wrong:
                    row[:, 4] = T(-0.5)
            else:
                first = hits[:S]
                idx = first[np.arange(S) % len(first)]
                if "zero_fill" in wrong:
                    idx = np.concatenate((first, np.zeros(S - len(first), np.int64)))
                pool_idx[b, m] = idx
                p = xyz[b][idx]
                with np.errstate(over="ignore", invalid="ignore"):
                    sig = T(1) / (T(1) + np.exp(-scores[b][idx]))
                    row[:, 3] = (sig > T(score_thres)).astype(T)
                    row[:, 4] = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) / T(70) - T(0.5)
                row[:, 5:] = feat[b * N + idx]
            d = p - box[:3]
            ca, sa = T(np.cos(box[6])), T(np.sin(box[6]))
            if "rot_sign" in wrong:
                sa = -sa
            row[:, 0] = d[:, 0] * ca - d[:, 2] * sa
            row[:, 1] = d[:, 1]
            row[:, 2] = d[:, 0] * sa + d[:, 2] * ca
    return pts_input, pool_idx, empty, count
