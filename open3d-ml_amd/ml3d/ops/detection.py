"""PointPillars front end, BEV convolutions, box decode + NMS, box IoU."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from . import _gates
from ._gates import KnnResult, RadiusResult, VoxelizeResult, _splits, _splits_of_lengths
from .gemm import pack_bf16x3, linear_bf16x3   # noqa: F401  (re-exported: their first callers were the BEV convolutions)


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def _ws(nbytes, device):
    return _gates._ws(nbytes, device)

def pillar_features(points, vox, in_channels, max_num_points, vx, vy, x_offset, y_offset, nx, ny, layers, batch):
    """Fused dense-gather + PillarFeatureNet + PointPillarsScatter (point_pillars.py:359-382, 512-555, 577-616).
    ``vox``: VoxelizeResult of the whole batch; ``layers``: [(wt [cin, units], bias [units]), ...] BN-folded.
    Returns the NHWC canvas [batch, ny, nx, units_last]."""
    lib = _abi.get()
    _need_gpu(points, vox.voxel_coords)
    dev = points.device
    if points.dtype != torch.float32 or points.dim() != 2 or points.stride(1) != 1:
        raise RuntimeError("pillar_features: points must be float32 [N, C] rows")
    stride = points.stride(0) if points.shape[0] > 1 else points.shape[1]
    M = vox.voxel_coords.shape[0]
    nl = len(layers)
    units = (C.c_int32 * nl)(*[int(w.shape[1]) for w, _ in layers])
    cc = int(layers[-1][0].shape[1])
    canvas = torch.empty((int(batch), int(ny), int(nx), cc), dtype=torch.float32, device=dev)
    wsb = lib.ml3d_pillar_features_workspace_bytes(M, int(max_num_points), nl, units)
    ws = _ws(wsb, dev)
    tw = _abi.ptr_table([w.data_ptr() for w, _ in layers])
    tb = _abi.ptr_table([b.data_ptr() for _, b in layers])
    with torch.cuda.device(dev):
        rc = lib.ml3d_pillar_features(points.data_ptr(), stride, int(in_channels), vox.voxel_coords.data_ptr(),
                                      vox.voxel_point_indices.data_ptr(), vox.voxel_point_row_splits.data_ptr(),
                                      vox.voxel_batch_splits.data_ptr(), int(batch), M, int(max_num_points), float(vx),
                                      float(vy), float(x_offset), float(y_offset), int(nx), int(ny), nl, units, tw, tb,
                                      canvas.data_ptr(), cc, ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_pillar_features")
    return canvas


def conv2d_nhwc(x, weights, bias, kh, kw, stride, pad, act=2, slope=0.0, out=None, out_channel_offset=0, packed=None):
    """Conv2d + folded BN + activation on NHWC maps (SECOND, point_pillars.py:640-682).  `packed` = pack_bf16x3(weights) runs the
    same product on the bf16 matrix pipe (three-way split, float32-equivalent); `weights` still gives the shape."""
    lib = _abi.get()
    _need_gpu(x, weights, bias)
    B, H, W, Cin = x.shape
    cout = weights.shape[1]
    OH, OW = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty((B, OH, OW, cout), dtype=torch.float32, device=x.device)
    ld = out.shape[3]
    if packed is not None:
        with torch.cuda.device(x.device):
            rc = lib.ml3d_conv2d_nhwc_bf16x3(x.data_ptr(), B, H, W, Cin, packed.data_ptr(),
                                             None if bias is None else bias.data_ptr(), kh, kw, stride, pad, act, slope, cout,
                                             out.data_ptr() + 4 * out_channel_offset, ld, _stream())
        if rc != _abi.E_UNSUPPORTED:
            _abi.check(rc, "ml3d_conv2d_nhwc_bf16x3")
            return out
    wsb = lib.ml3d_conv2d_workspace_bytes(B, OH, OW, Cin, cout, kh, kw)
    ws = _ws(wsb, x.device)
    with torch.cuda.device(x.device):
        rc = lib.ml3d_conv2d_nhwc(x.data_ptr(), B, H, W, Cin, weights.data_ptr(), None if bias is None else bias.data_ptr(),
                                  kh, kw, stride, pad, act, slope, cout, out.data_ptr() + 4 * out_channel_offset, ld,
                                  ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_conv2d_nhwc")
    return out


def deconv2d_nhwc(x, weights, bias, stride, cout, act=2, slope=0.0, out=None, out_channel_offset=0, packed=None):
    """ConvTranspose2d(kernel == stride) + folded BN + activation (SECONDFPN, point_pillars.py:712-717, 749).  `packed` =
    pack_bf16x3(weights): the same GEMM on the bf16 matrix pipe."""
    lib = _abi.get()
    _need_gpu(x, weights, bias)
    B, H, W, Cin = x.shape
    if out is None:
        out = torch.empty((B, H * stride, W * stride, cout), dtype=torch.float32, device=x.device)
    ld = out.shape[3]
    if packed is not None:
        with torch.cuda.device(x.device):
            rc = lib.ml3d_deconv2d_nhwc_bf16x3(x.data_ptr(), B, H, W, Cin, packed.data_ptr(), None if bias is None else bias.data_ptr(),
                                               stride, act, slope, cout, out.data_ptr() + 4 * out_channel_offset, ld, _stream())
        if rc != _abi.E_UNSUPPORTED:
            _abi.check(rc, "ml3d_deconv2d_nhwc_bf16x3")
            return out
    wsb = lib.ml3d_conv2d_workspace_bytes(B, H, W, Cin, stride * stride * cout, 1, 1)
    ws = _ws(wsb, x.device)
    with torch.cuda.device(x.device):
        rc = lib.ml3d_deconv2d_nhwc(x.data_ptr(), B, H, W, Cin, weights.data_ptr(),
                                    None if bias is None else bias.data_ptr(), stride, act, slope, cout,
                                    out.data_ptr() + 4 * out_channel_offset, ld, ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_deconv2d_nhwc")
    return out


def nhwc_to_nchw(x, channel_offset, channels):
    lib = _abi.get()
    _need_gpu(x)
    B, H, W, ld = x.shape
    out = torch.empty((B, channels, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.ml3d_nhwc_to_nchw(x.data_ptr(), ld, int(channel_offset), int(channels), B, H * W, out.data_ptr(), _stream())
    _abi.check(rc, "ml3d_nhwc_to_nchw")
    return out


def nms(boxes, scores, nms_overlap_thresh):
    """``open3d.ml.torch.ops.nms`` (ml3d/torch/utils/objdet_helper.py:346): rotated-BEV NMS on boxes
    [N, 5] = (x0, y0, x1, y1, r); returns the kept indices (int64) in descending-score order."""
    lib = _abi.get()
    _need_gpu(boxes, scores)
    boxes = boxes.detach().contiguous().float()
    scores = scores.detach().contiguous().float()
    n = boxes.shape[0]
    dev = boxes.device
    if boxes.dim() != 2 or boxes.shape[1] != 5 or scores.numel() != n:
        raise RuntimeError("nms: boxes must be [N, 5] and scores [N]")
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    wsb = lib.ml3d_nms_workspace_bytes(n)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_nms(boxes.data_ptr(), scores.data_ptr(), n, float(nms_overlap_thresh), keep.data_ptr(),
                          count.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_nms")
    return keep[:int(count.item())]


def topk_rows(values, k, with_values=False):
    """The ``nms_pre`` top-k of ``Anchor3DHead.get_bboxes_single`` (``max_scores.topk(self.nms_pre)``, point_pillars.py:985-992)
    for all rows at once: ``values`` float32 [rows, n] (or [n]) -> int64 indices [rows, k] (or [k]) of the k largest of every
    row in descending value, equal values by ascending index, NaN first -- a HIP radix select (``ml3d_topk_rows``), no
    ``torch.topk``.  ``with_values=True`` also returns the values."""
    lib = _abi.get()
    _need_gpu(values)
    v = values.detach()
    flat = v.dim() == 1
    if flat:
        v = v.unsqueeze(0)
    if v.dim() != 2:
        raise RuntimeError("topk_rows: values must be [rows, n] or [n]")
    v = v.contiguous().float()
    rows, n = v.shape
    k = int(k)
    if k < 0 or k > n:
        raise RuntimeError("topk_rows: k = %d outside [0, %d]" % (k, n))
    dev = v.device
    idx = torch.empty((rows, k), dtype=torch.int64, device=dev)
    val = torch.empty((rows, k), dtype=torch.float32, device=dev) if with_values else None
    if rows * k > 0:
        wsb = lib.ml3d_topk_rows_workspace_bytes(rows, n, k)
        if wsb == 0:
            raise RuntimeError("topk_rows: k = %d is beyond the kernel's 4096 candidates per row" % k)
        ws = _ws(wsb, dev)
        with torch.cuda.device(dev):
            rc = lib.ml3d_topk_rows(v.data_ptr(), rows, n, k, idx.data_ptr(), val.data_ptr() if with_values else None,
                                    ws.data_ptr(), wsb, _stream())
        _abi.check(rc, "ml3d_topk_rows")
    if flat:
        idx, val = idx[0], (val[0] if with_values else None)
    return (idx, val) if with_values else idx


def _head_map(t):
    """[B, ch, H, W] float32 head map in any layout whose (H, W) plane has ONE pixel stride (NCHW tensors, channel slices of
    an NHWC tensor viewed as NCHW) -> (tensor, (batch, channel, pixel) element strides); anything else is made contiguous."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() != 4:
        raise RuntimeError("pointpillars_boxes: head maps must be [B, channels, H, W]")
    if t.shape[2] > 1 and t.stride(2) != t.shape[3] * t.stride(3):
        t = t.contiguous()
    return t, (t.stride(0), t.stride(1), t.stride(3))


def pointpillars_boxes(cls_scores, bbox_preds, dir_preds, anchors, nms_pre, score_thr, iou_thr, dir_offset=0.0):
    """``Anchor3DHead.get_bboxes`` for the whole batch with no host read-back inside (point_pillars.py:945-1025): head maps
    [B, A*C | A*7 | A*2, H, W] (the reference's NCHW tensors, or NCHW VIEWS of a fused NHWC head tensor -- no copy either
    way), ``anchors`` [H*W*A, 7] -> (rows [B, C*k, 9], total [B] int32): ``rows[b, :total[b]]`` = (x, y, z, w, l, h, yaw,
    score, label) of sample b's detections, class-major in NMS order."""
    lib = _abi.get()
    _need_gpu(cls_scores, bbox_preds, dir_preds, anchors)
    (cls_scores, s_cls), (bbox_preds, s_reg), (dir_preds, s_dir) = (_head_map(t) for t in (cls_scores, bbox_preds, dir_preds))
    anchors = anchors.contiguous().float()
    B, AC, H, W = cls_scores.shape
    A = dir_preds.shape[1] // 2
    C_ = AC // A
    if bbox_preds.shape[1] != A * 7 or anchors.shape[0] != H * W * A or anchors.shape[1] != 7:
        raise RuntimeError("pointpillars_boxes: head maps / anchors do not agree on the anchor count")
    dev = cls_scores.device
    n_anchor = H * W * A
    strides = (C.c_int64 * 9)(*[int(v) for v in s_cls + s_reg + s_dir])
    with torch.cuda.device(dev):
        if n_anchor > int(nms_pre):
            smax = torch.empty((B, n_anchor), dtype=torch.float32, device=dev)
            rc = lib.ml3d_pp_anchor_scores(cls_scores.data_ptr(), strides, B, A, C_, H * W, smax.data_ptr(), _stream())
            _abi.check(rc, "ml3d_pp_anchor_scores")
            cand = topk_rows(smax, int(nms_pre))
        else:
            cand = torch.arange(n_anchor, dtype=torch.int64, device=dev).repeat(B, 1).contiguous()
        k = cand.shape[1]
        rows = torch.empty((B, C_ * k, 9), dtype=torch.float32, device=dev)
        total = torch.empty(B, dtype=torch.int32, device=dev)
        wsb = lib.ml3d_pp_boxes_workspace_bytes(B, k, C_)
        if wsb == 0:
            raise RuntimeError("pointpillars_boxes: nms_pre = %d candidates per sample is beyond the batched kernel (4096)" % k)
        ws = _ws(wsb, dev)
        rc = lib.ml3d_pp_boxes(cls_scores.data_ptr(), bbox_preds.data_ptr(), dir_preds.data_ptr(), strides, anchors.data_ptr(),
                               cand.data_ptr(), B, k, A, C_, H * W, float(score_thr), float(iou_thr), float(dir_offset),
                               rows.data_ptr(), total.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_pp_boxes")
    return rows, total


def _iou(fn_name, boxes_a, boxes_b, cols):
    lib = _abi.get()
    _need_gpu(boxes_a, boxes_b)
    a = boxes_a.contiguous().float()
    b = boxes_b.contiguous().float()
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != cols or b.shape[1] != cols:
        raise RuntimeError("%s: boxes must be float32 [N, %d] / [M, %d]" % (fn_name, cols, cols))
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = getattr(lib, fn_name)(a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], out.data_ptr(), _stream())
    _abi.check(rc, fn_name)
    return out


def iou_bev(boxes_a, boxes_b):
    """``open3d.ml.contrib.iou_bev_*`` (ml3d/metrics/mAP.py:85): rotated bird's-eye-view IoU of every pair;
    boxes [N, 5] / [M, 5] = (x, z, w, l, yaw) -> float32 [N, M]."""
    return _iou("ml3d_iou_bev", boxes_a, boxes_b, 5)


def iou_3d(boxes_a, boxes_b):
    """``open3d.ml.contrib.iou_3d_*`` (ml3d/metrics/mAP.py:87): 3-D IoU of every pair; boxes [N, 7] / [M, 7] =
    (x, y, z, w, h, l, yaw) with y the bottom face (camera frame, y down) -> float32 [N, M]."""
    return _iou("ml3d_iou_3d", boxes_a, boxes_b, 7)


def det_pair_starts(pred_start, tgt_start):
    """int64 [F + 1]: frame f's IoU block starts at ``sum(P_g * T_g for g < f)`` of a ``pair_iou`` plane (host arrays in and out)."""
    ps, ts = np.asarray(pred_start, np.int64), np.asarray(tgt_start, np.int64)
    out = np.zeros(ps.size, np.int64)
    np.cumsum(np.diff(ps) * np.diff(ts), out=out[1:])
    return out


def det_match(pred_box, pred_cls, pred_dmask, pred_start, tgt_box, tgt_lab, tgt_dmask, tgt_start, min_overlap, similar,
              num_difficulties, metrics=3, out_flags=None, out_fn=None, return_iou=False, pair_start=None, num_pairs=None,
              pair_iou=None):
    """``precision_3d`` (ml3d/metrics/mAP.py:38-135) for every frame of a split in ONE call of ``ml3d_det_match`` (two launches,
    no read-back): device tensors ``pred_box`` float32 [NP, 7], ``pred_cls`` int32 [NP] (index into ``classes``, -1 = dropped),
    ``pred_dmask`` int32 [NP] (bit j: passes difficulty j), the same for the targets (``tgt_lab``: vocabulary ids),
    ``min_overlap`` float32 [C], ``similar`` int32 [C].  ``pred_start`` / ``tgt_start`` are the int64 [F + 1] row splits: HOST
    arrays, from which the block offsets are computed and uploaded here -- or device tensors together with ``pair_start`` (device,
    ``det_pair_starts``) and ``num_pairs``, for a caller that uploaded everything at once.
    Returns (``flags`` uint8 [2, D, NP]: bit 0 tp, bit 1 fp, plane 0 BEV / 1 3-D, a plane ``metrics`` (1 | 2 | 3) does not name
    untouched; ``fn`` int64 [2, C, D], ADDED to when handed in) and, with ``return_iou=True``, ``pair_iou`` float32
    [2, num_pairs]: frame f's P_f x T_f block row-major at its offset, only the pairs whose classes relate written
    (``pair_iou=``: the caller's buffer, float32 [2, capacity]; a capacity below ``num_pairs`` is refused: "workspace too small")."""
    lib = _abi.get()
    _need_gpu(pred_box, pred_cls, pred_dmask, tgt_box, tgt_lab, tgt_dmask, min_overlap, similar)
    dev = pred_box.device
    D, C_ = int(num_difficulties), int(min_overlap.numel())
    NP, NT = int(pred_cls.numel()), int(tgt_lab.numel())

    def bad(why):
        raise RuntimeError("det_match: invalid argument: " + why)
    for t, dt, shape, name in ((pred_box, torch.float32, (NP, 7), "pred_box"), (tgt_box, torch.float32, (NT, 7), "tgt_box"),
                               (pred_cls, torch.int32, (NP,), "pred_cls"), (tgt_lab, torch.int32, (NT,), "tgt_lab"),
                               (pred_dmask, torch.int32, (NP,), "pred_dmask"), (tgt_dmask, torch.int32, (NT,), "tgt_dmask"),
                               (min_overlap, torch.float32, (C_,), "min_overlap"), (similar, torch.int32, (C_,), "similar")):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            bad("%s must be a contiguous %s tensor of shape %s" % (name, dt, list(shape)))
    if not 1 <= D <= 32 or C_ < 1 or int(metrics) not in (1, 2, 3):
        bad("1..32 difficulties, at least one class and metrics 1, 2 or 3 expected")
    if pair_start is None:
        ps = np.ascontiguousarray(pred_start.cpu().numpy() if isinstance(pred_start, torch.Tensor) else pred_start, dtype=np.int64)
        ts = np.ascontiguousarray(tgt_start.cpu().numpy() if isinstance(tgt_start, torch.Tensor) else tgt_start, dtype=np.int64)
        if ps.ndim != 1 or ps.shape != ts.shape or ps.size < 1 or ps[0] != 0 or ts[0] != 0 or ps[-1] != NP or ts[-1] != NT or \
                (np.diff(ps) < 0).any() or (np.diff(ts) < 0).any():
            bad("pred_start / tgt_start must be row splits [F + 1] of the predictions / targets")
        starts = np.stack([ps, ts, det_pair_starts(ps, ts)])
        num_pairs = int(starts[2, -1])
        pred_start, tgt_start, pair_start = torch.from_numpy(starts).to(dev)
    else:
        _need_gpu(pred_start, tgt_start, pair_start)
        for t in (pred_start, tgt_start, pair_start):
            if t.dtype != torch.int64 or t.dim() != 1 or t.shape != pred_start.shape or not t.is_contiguous() or t.numel() < 1:
                bad("the three row splits must be contiguous int64 [F + 1]")
        if num_pairs is None:
            bad("num_pairs goes with pair_start")
    F = int(pred_start.numel()) - 1
    if out_flags is None:
        out_flags = torch.zeros((2, D, NP), dtype=torch.uint8, device=dev)
    elif out_flags.dtype != torch.uint8 or tuple(out_flags.shape) != (2, D, NP) or not out_flags.is_contiguous():
        bad("out_flags must be contiguous uint8 [2, D, NP]")
    if out_fn is None:
        out_fn = torch.zeros((2, C_, D), dtype=torch.int64, device=dev)
    elif out_fn.dtype != torch.int64 or tuple(out_fn.shape) != (2, C_, D) or not out_fn.is_contiguous():
        bad("out_fn must be contiguous int64 [2, C, D]")
    if pair_iou is None:
        pair_iou = torch.empty((2, int(num_pairs)), dtype=torch.float32, device=dev)
    elif pair_iou.dtype != torch.float32 or pair_iou.dim() != 2 or pair_iou.shape[0] != 2 or not pair_iou.is_contiguous():
        bad("pair_iou must be contiguous float32 [2, capacity]")
    with torch.cuda.device(dev):
        rc = lib.ml3d_det_match(pred_box.data_ptr(), pred_cls.data_ptr(), pred_dmask.data_ptr(), pred_start.data_ptr(),
                                tgt_box.data_ptr(), tgt_lab.data_ptr(), tgt_dmask.data_ptr(), tgt_start.data_ptr(),
                                pair_start.data_ptr(), F, NP, NT, int(num_pairs), min_overlap.data_ptr(), similar.data_ptr(), C_, D,
                                int(metrics), out_flags.data_ptr(), out_fn.data_ptr(), pair_iou.data_ptr(), int(pair_iou.shape[1]), _stream())
    _abi.check(rc, "ml3d_det_match")
    return (out_flags, out_fn, pair_iou) if return_iou else (out_flags, out_fn)
