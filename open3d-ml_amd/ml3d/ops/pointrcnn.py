"""PointRCNN ops on the HIP kernels of csrc/pointrcnn.hip (contracts: include/ml3d_hip.h, "PointRCNN stage 1" / "stage 2"):
``bin_decode`` restates the reference's ``decode_bbox_target`` (point_rcnn.py:1153-1272), ``rpn_proposals`` its
``ProposalLayer.forward`` with ``post_process=True`` (:1020-1150) for a whole batch, without a read-back; ``roi_pool`` produces
the ``pts_input`` rows of ``RCNN.forward`` (:848-887): the wheel's RoI pooling, the two extra columns and the canonical transform."""
import numpy as np
import torch

from .. import _abi
from . import _gates
from .gemm import _rows


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def reg_channels(loc_scope, loc_bin_size, num_head_bin, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
                 loc_y_bin_size=0.25):
    """The column count of ``pred_reg`` the flags imply, computed as the reference does (point_rcnn.py:652-658, 809-815)."""
    per_loc = int(loc_scope / loc_bin_size) * 2
    y = int(loc_y_scope / loc_y_bin_size) * 2 * 2 if get_y_by_bin else 1
    return per_loc * (4 if get_xz_fine else 2) + y + int(num_head_bin) * 2 + 3


def bin_decode(roi, pred_reg, anchor_size, loc_scope, loc_bin_size, num_head_bin, get_xz_fine=True, get_y_by_bin=False,
               loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False):
    """``decode_bbox_target(roi_box3d, pred_reg, ...)``: ``roi`` [n, 3 or 7], ``pred_reg`` [n, C] (may be a column slice),
    ``anchor_size`` three numbers -> boxes [n, 7] = (x, y, z, h, w, l, ry).  C must be the count the flags imply."""
    _need_gpu(roi, pred_reg)
    lib = _abi.get()
    if roi.dim() != 2 or roi.shape[1] not in (3, 7) or roi.dtype != torch.float32 or not roi.is_contiguous():
        raise RuntimeError("bin_decode: invalid argument: roi must be contiguous float32 [n, 3] or [n, 7]")
    ld = _rows("bin_decode", pred_reg)
    n, c = int(roi.shape[0]), int(pred_reg.shape[1])
    if pred_reg.shape[0] != n:
        raise RuntimeError("bin_decode: invalid argument: roi has %d rows, pred_reg %d" % (n, pred_reg.shape[0]))
    anchor = np.ascontiguousarray(torch.as_tensor(anchor_size).detach().cpu().numpy().reshape(-1), np.float32)
    if anchor.size != 3:
        raise RuntimeError("bin_decode: invalid argument: anchor_size must hold 3 numbers")
    if not (loc_scope > 0 and loc_bin_size > 0 and int(num_head_bin) >= 1) or (get_y_by_bin and not (loc_y_scope > 0 and loc_y_bin_size > 0)):
        raise RuntimeError("bin_decode: invalid argument: scopes, bin sizes and num_head_bin must be positive")
    want = reg_channels(loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size)
    if c != want:
        raise RuntimeError("bin_decode: invalid argument: pred_reg has %d columns, the flags imply %d" % (c, want))
    out = torch.empty((n, 7), dtype=torch.float32, device=roi.device)
    with torch.cuda.device(roi.device):
        rc = lib.ml3d_bin_decode(roi.data_ptr(), int(roi.shape[1]), pred_reg.data_ptr(), ld, c, n, anchor.ctypes.data, float(loc_scope),
                                 float(loc_bin_size), int(num_head_bin), float(loc_y_scope), float(loc_y_bin_size), int(bool(get_xz_fine)),
                                 int(bool(get_y_by_bin)), int(bool(get_ry_fine)), out.data_ptr(), _stream())
    _abi.check(rc, "ml3d_bin_decode")
    return out


def _scratch(b, n, pre, dev):
    """The caller-owned scratch of ``ml3d_rpn_proposals`` (include/ml3d_hip.h), typed, UNINITIALISED on purpose."""
    total, p = b * n, b * pre
    keys = torch.empty((2 * total + 1,), dtype=torch.int64, device=dev)
    vals = torch.empty((2 * total + 1,), dtype=torch.int32, device=dev)
    hist = torch.empty((257 * ((total + 1023) // 1024) + 4,), dtype=torch.int32, device=dev)
    lists = torch.empty((2 * p + 2 * b + 1,), dtype=torch.int32, device=dev)
    nms_boxes = torch.empty((6 * p + 1,), dtype=torch.float32, device=dev)
    nms_keep = torch.empty((p + 2 * b + 1,), dtype=torch.int64, device=dev)
    ws = _gates._ws(int(_abi.get().ml3d_nms_workspace_bytes(pre)), dev)
    return keys, vals, hist, lists, nms_boxes, nms_keep, ws


def rpn_proposals(scores, boxes, nms_pre, nms_post, nms_thres, out=None):
    """``ProposalLayer.forward`` behind the decode: ``scores`` [B, N], ``boxes`` [B, N, 7] (left untouched) -> (rois
    [B, nms_post, 7] zero padded, roi_scores [B, nms_post] zero padded, roi_index int32 [B, nms_post]: the item-local source
    point of each roi, -1 in the padding).  ``out``: the three tensors to write into."""
    _need_gpu(scores, boxes, *(out or ()))
    lib = _abi.get()
    if scores.dim() != 2 or boxes.dim() != 3 or boxes.shape[2] != 7 or tuple(boxes.shape[:2]) != tuple(scores.shape):
        raise RuntimeError("rpn_proposals: invalid argument: scores [B, N] and boxes [B, N, 7] expected")
    for t in (scores, boxes):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("rpn_proposals: invalid argument: float32 contiguous tensors required")
    b, n, pre, post = int(scores.shape[0]), int(scores.shape[1]), int(nms_pre), int(nms_post)
    if pre < 0 or post < 0 or pre > 65536 or b > 65536 or b * n >= 2 ** 31:
        raise RuntimeError("rpn_proposals: invalid argument: 0 <= nms_pre <= 65536, nms_post >= 0, B <= 65536 and B * N < 2^31 required")
    dev = scores.device
    if out is None:
        out = (torch.empty((b, post, 7), dtype=torch.float32, device=dev), torch.empty((b, post), dtype=torch.float32, device=dev),
               torch.empty((b, post), dtype=torch.int32, device=dev))
    rois, roi_scores, roi_index = out
    if tuple(rois.shape) != (b, post, 7) or tuple(roi_scores.shape) != (b, post) or tuple(roi_index.shape) != (b, post) or \
            rois.dtype != torch.float32 or roi_scores.dtype != torch.float32 or roi_index.dtype != torch.int32 or \
            not (rois.is_contiguous() and roi_scores.is_contiguous() and roi_index.is_contiguous()):
        raise RuntimeError("rpn_proposals: invalid argument: out = (f32 [B, nms_post, 7], f32 [B, nms_post], int32 [B, nms_post]) contiguous")
    keys, vals, hist, lists, nms_boxes, nms_keep, ws = _scratch(b, n, pre, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_rpn_proposals(scores.data_ptr(), boxes.data_ptr(), b, n, pre, post, float(nms_thres), rois.data_ptr(),
                                    roi_scores.data_ptr(), roi_index.data_ptr(), keys.data_ptr(), vals.data_ptr(), hist.data_ptr(),
                                    lists.data_ptr(), nms_boxes.data_ptr(), nms_keep.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    _abi.check(rc, "ml3d_rpn_proposals")
    return rois, roi_scores, roi_index


def roi_pool(xyz, feat, scores, rois, num_points=512, score_thres=0.3, extra_width=1.0, out=None):
    """``xyz`` [B, N, 3], ``feat`` rows [B * N, C] (may be a column slice of a wider buffer), ``scores`` [B, N] raw, ``rois``
    [B, M, 7] -> (pts_input [B * M, num_points, 5 + C], pool_idx int32 [B, M, num_points] item-local or -1, empty int32 [B, M]).
    ``out``: the three tensors to write into."""
    _need_gpu(xyz, feat, scores, rois, *(out or ()))
    lib = _abi.get()
    if xyz.dim() != 3 or xyz.shape[2] != 3 or scores.dim() != 2 or tuple(scores.shape) != tuple(xyz.shape[:2]) or rois.dim() != 3 or \
            rois.shape[2] != 7 or rois.shape[0] != xyz.shape[0]:
        raise RuntimeError("roi_pool: invalid argument: xyz [B, N, 3], scores [B, N] and rois [B, M, 7] expected")
    for t in (xyz, scores, rois):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("roi_pool: invalid argument: float32 contiguous tensors required")
    b, n, m, s = int(xyz.shape[0]), int(xyz.shape[1]), int(rois.shape[1]), int(num_points)
    if feat.dim() != 2 or feat.dtype != torch.float32 or feat.shape[0] != b * n or (feat.shape[1] > 1 and feat.stride(1) != 1):
        raise RuntimeError("roi_pool: invalid argument: feat must be float32 rows [B * N, C] with unit column stride")
    c = int(feat.shape[1])
    ld = int(feat.stride(0)) if b * n > 1 else max(int(feat.stride(0)), c)
    if s < 1 or ld < c:
        raise RuntimeError("roi_pool: invalid argument: num_points >= 1 and a row stride >= C required")
    if b * n >= 2 ** 31 or b * m * s >= 2 ** 31:
        raise RuntimeError("roi_pool: invalid argument: B * N < 2^31 and B * M * num_points < 2^31 required")
    dev = xyz.device
    if out is None:
        out = (torch.empty((b * m, s, 5 + c), dtype=torch.float32, device=dev), torch.empty((b, m, s), dtype=torch.int32, device=dev),
               torch.empty((b, m), dtype=torch.int32, device=dev))
    pts_input, pool_idx, empty = out
    if tuple(pts_input.shape) != (b * m, s, 5 + c) or tuple(pool_idx.shape) != (b, m, s) or tuple(empty.shape) != (b, m) or \
            pts_input.dtype != torch.float32 or pool_idx.dtype != torch.int32 or empty.dtype != torch.int32 or \
            not (pts_input.is_contiguous() and pool_idx.is_contiguous() and empty.is_contiguous()):
        raise RuntimeError("roi_pool: invalid argument: out = (f32 [B * M, S, 5 + C], int32 [B, M, S], int32 [B, M]) contiguous")
    with torch.cuda.device(dev):
        rc = lib.ml3d_roi_pool(xyz.data_ptr(), feat.data_ptr(), ld, c, scores.data_ptr(), rois.data_ptr(), b, n, m, s,
                               float(score_thres), float(extra_width), pts_input.data_ptr(), pool_idx.data_ptr(), empty.data_ptr(),
                               _stream())
    _abi.check(rc, "ml3d_roi_pool")
    return pts_input, pool_idx, empty


__all__ = ["bin_decode", "rpn_proposals", "reg_channels", "roi_pool"]
