"""PointRCNN (ml3d/torch/models/point_rcnn.py of the reference; Shi et al., CVPR 2019), MI355X-native STAGE 1: everything from
the point cloud to the region proposals -- the reference's ``mode="RPN"`` forward.  The module tree holds the parameters of the
WHOLE model under the reference's names (``state_dict()`` keys and shapes are the reference's, a reference checkpoint loads with
``strict=True``); ``rcnn.*`` is parameter containers only: RoI pooling and the RCNN stage are NOT built, ``mode="RCNN"`` forward
raises and points to ``proposals()``, the hand-off the second stage will start from.

Stage 1 on the device: the ``Pointnet2MSG`` backbone (ml3d/torch/modules/pointnet.py), the two heads with their BatchNorms folded
once in float64 on the shared GEMM over rows [B * N, 128] (the first layers of both heads as ONE product, their weights side by
side; Dropout is the identity in eval), ``ml3d_bin_decode`` for all B * N rows and ``ml3d_rpn_proposals`` for the whole batch
(include/ml3d_hip.h, "PointRCNN stage 1") -- no ``torch.cat`` / ``torch.sort`` and no Python loop over items or zones.

``ML3D_PRCNN_OPS=torch`` (A/B switch, read per forward): the same stage behind the SAME backbone output written with torch ops on
the GPU (matmul, ``argmax``, ``gather``, ``sort``, boolean masks, the native ``nms`` per zone, as the reference's Python loop
does) -- the baseline the kernels are measured against and an independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _abi
from ... import ops
from ...ops import pointnet2 as pn2_ops
from ...ops import pointrcnn as prcnn_ops
from ..modules.pointnet import Pointnet2MSG

_HEAD_DEFAULTS = dict(nms_pre=9000, nms_post=512, nms_thres=0.85, nms_post_val=None, nms_thres_val=None, mean_size=[1.0],
                      loc_xz_fine=True, loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_y_by_bin=False, get_ry_fine=False,
                      loc_y_scope=0.5, loc_y_bin_size=0.25, post_process=True)


class _ProposalLayer(nn.Module):
    """The settings of ``ProposalLayer`` (point_rcnn.py:984-1018); no parameters."""

    def __init__(self, **head):
        super().__init__()
        unknown = set(head) - set(_HEAD_DEFAULTS)
        if unknown:
            raise TypeError("ProposalLayer: unexpected arguments %s" % sorted(unknown))
        for k, v in _HEAD_DEFAULTS.items():
            setattr(self, k, head.get(k, v))
        self.mean_size = [float(v) for v in self.mean_size]


def _head(in_ch, out_ch, last, db_ratio):
    """``cls_blocks`` / ``reg_blocks`` of the RPN (point_rcnn.py:637-671): Conv1d at 0, 4, ...; BatchNorm1d at 1, 5, ..."""
    widths = [in_ch, *out_ch[:-1]]
    layers = []
    for i in range(len(out_ch)):
        layers += [nn.Conv1d(widths[i], out_ch[i], 1, bias=False), nn.BatchNorm1d(out_ch[i]), nn.ReLU(inplace=True), nn.Dropout(db_ratio)]
    layers.append(nn.Conv1d(out_ch[-1], last, 1, bias=True))
    return nn.Sequential(*layers)


def _cnn(widths, conv):
    """``gen_CNN(widths, conv=conv)`` (torch_utils.py:26): conv with bias at 0, 2, 4, ..."""
    layers = []
    for ci, co in zip(widths[:-1], widths[1:]):
        layers += [conv(ci, co, 1, bias=True), nn.ReLU(inplace=True)]
    return nn.Sequential(*layers)


class _RPN(nn.Module):

    def __init__(self, device, backbone={}, cls_in_ch=128, cls_out_ch=[128], reg_in_ch=128, reg_out_ch=[128], db_ratio=0.5, head={},
                 focal_loss={}, loss_weight=[1.0, 1.0], **kwargs):
        super().__init__()
        self.backbone = Pointnet2MSG(**backbone, device=device)
        self.proposal_layer = _ProposalLayer(**head)
        pl = self.proposal_layer
        self.cls_blocks = _head(cls_in_ch, list(cls_out_ch), 1, db_ratio)
        per_loc_bin_num = int(pl.loc_scope / pl.loc_bin_size) * 2
        reg_channel = per_loc_bin_num * (4 if pl.loc_xz_fine else 2) + pl.num_head_bin * 2 + 3 + 1
        self.reg_channel = reg_channel
        self.reg_blocks = _head(reg_in_ch, list(reg_out_ch), reg_channel, db_ratio)


class _SAParams(nn.Module):
    """Parameter container of ``PointnetSAModule(..., bias=True)`` (pointnet.py:214-246): ``mlps.0`` = conv with bias + ReLU."""

    def __init__(self, widths):
        super().__init__()
        self.mlps = nn.ModuleList([_cnn(widths, nn.Conv2d)])


class _RCNN(nn.Module):
    """Parameter containers of the reference's ``RCNN`` (point_rcnn.py:773-826) under its names and shapes.  No forward."""

    def __init__(self, num_classes, in_channels=128,
                 SA_config={"npoints": [128, 32, -1], "radius": [0.2, 0.4, 100], "nsample": [64, 64, 64],
                            "mlps": [[128, 128, 128], [128, 128, 256], [256, 256, 512]]},
                 cls_out_ch=[256, 256], reg_out_ch=[256, 256], db_ratio=0.5, use_xyz=True, xyz_up_layer=[128, 128], head={},
                 target_head={}, loss={}):
        super().__init__()
        self.rcnn_input_channel = 5
        self.proposal_layer = _ProposalLayer(**head)
        pl = self.proposal_layer
        self.SA_modules = nn.ModuleList()
        for i in range(len(SA_config["npoints"])):
            widths = [in_channels + (3 if use_xyz else 0)] + [int(c) for c in SA_config["mlps"][i]]
            self.SA_modules.append(_SAParams(widths))
            in_channels = widths[-1]
        self.xyz_up_layer = _cnn([self.rcnn_input_channel] + list(xyz_up_layer), nn.Conv2d)
        c_out = xyz_up_layer[-1]
        self.merge_down_layer = _cnn([c_out * 2, c_out], nn.Conv2d)
        cls_channel = 1 if num_classes == 2 else num_classes
        self.cls_blocks = _cnn([in_channels, *cls_out_ch], nn.Conv1d)
        self.cls_blocks.append(nn.Conv1d(cls_out_ch[-1], cls_channel, 1, bias=True))
        per_loc_bin_num = int(pl.loc_scope / pl.loc_bin_size) * 2
        loc_y_bin_num = int(pl.loc_y_scope / pl.loc_y_bin_size) * 2
        reg_channel = per_loc_bin_num * 4 + pl.num_head_bin * 2 + 3 + (1 if not pl.get_y_by_bin else loc_y_bin_num * 2)
        self.reg_blocks = _cnn([in_channels, *reg_out_ch], nn.Conv1d)
        self.reg_blocks.append(nn.Conv1d(reg_out_ch[-1], reg_channel, 1, bias=True))


def _fold_head(seq):
    """-> [(weights_t [in, out] f32, shift [out] f32, act)]: each Conv1d + BatchNorm1d folded in float64, the last Conv1d with its bias."""
    out = []
    mods = list(seq)
    for i in range(0, len(mods) - 1, 4):
        conv, bn = mods[i], mods[i + 1]
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
        w = conv.weight.detach().double()[:, :, 0] * scale[:, None]
        out.append((w.t().float().contiguous(), shift.float().contiguous(), 2))
    last = mods[-1]
    out.append((last.weight.detach().double()[:, :, 0].t().float().contiguous(), last.bias.detach().float().contiguous(), 0))
    return out


class PointRCNN(nn.Module):
    """``PointRCNN(name, device, classes, score_thres, npoints, rpn, rcnn, mode)`` of the reference, stage 1 on the MI355X."""

    def __init__(self, name="PointRCNN", device="cuda", classes=['Car'], score_thres=0.3, npoints=16384, rpn={}, rcnn={}, mode="RCNN",
                 **kwargs):
        super().__init__()
        assert mode == "RPN" or mode == "RCNN"
        self.name = name
        self.mode = mode
        self.device = torch.device(device) if isinstance(device, str) else device
        _abi.require_gpu(self.device, "PointRCNN")
        self.npoints = npoints
        self.classes = list(classes)
        self.name2lbl = {n: i for i, n in enumerate(self.classes)}
        self.lbl2name = {i: n for i, n in enumerate(self.classes)}
        self.score_thres = score_thres
        self.rpn = _RPN(device=self.device, **rpn)
        self.rcnn = _RCNN(num_classes=len(self.classes), **rcnn)
        self._packed = None
        self.to(self.device)
        self.eval()

    # ---- folded parameters ------------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        r = super().load_state_dict(*a, **k)
        self.rpn.backbone._packed = None
        self.rpn.backbone.packed_params()
        self.packed_params()
        return r

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("PointRCNN (MI355X build): inference only; .train() is unsupported")
        return super().train(False)

    def packed_params(self):
        """Fold the heads' BatchNorms (float64) ONCE: the first layers of both heads side by side when both have one."""
        if self._packed is not None:
            return self._packed
        with torch.no_grad():
            cls, reg = _fold_head(self.rpn.cls_blocks), _fold_head(self.rpn.reg_blocks)
            P = dict(cls=cls, reg=reg, first=None)
            if len(cls) > 1 and len(reg) > 1 and cls[0][0].shape[0] == reg[0][0].shape[0]:
                P["first"] = (torch.cat((cls[0][0], reg[0][0]), 1).contiguous(), torch.cat((cls[0][1], reg[0][1])).contiguous(),
                              int(cls[0][0].shape[1]))
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._packed = P
        return P

    # ---- stage 1 --------------------------------------------------------------------------------------------------------------
    def _heads(self, rows, hip):
        """rows [B * N, C] -> (cls [B * N, 1], reg [B * N, reg_channel])."""
        P = self.packed_params()

        def lin(a, w, b, act):
            return pn2_ops._linear_rows(a, w, b, act) if hip else _torch_linear(a, w, b, act)

        outs = []
        if P["first"] is not None:
            w, b, split = P["first"]
            h = lin(rows, w, b, 2)
            starts = ((h[:, :split], P["cls"][1:]), (h[:, split:], P["reg"][1:]))
        else:
            starts = ((rows, P["cls"]), (rows, P["reg"]))
        for x, layers in starts:
            for w, b, act in layers:
                x = lin(x, w, b, act)
            outs.append(x)
        return outs

    def _points(self, points):
        if hasattr(points, "point"):
            points = torch.stack(list(points.point))
        if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] < 3:
            raise ValueError("PointRCNN: points [B, N, 3+] or an object with a .point list expected")
        ops._gates._need_gpu(points)
        return points.float().contiguous()

    def proposals(self, points):
        """``points`` [B, N, 3+] (or a batch object with a ``.point`` list) -> dict: ``rois`` [B, nms_post, 7] zero padded,
        ``roi_scores`` [B, nms_post], ``roi_index`` int32 [B, nms_post] (source point, -1 in the padding), ``cls`` [B, N, 1],
        ``reg`` [B, N, C], ``xyz`` [B, N, 3], ``features`` [B, 128, N] -- the hand-off to the second stage."""
        if self.training:
            raise NotImplementedError("PointRCNN (MI355X build): inference only; call .eval()")
        hip = os.environ.get("ML3D_PRCNN_OPS", "hip").strip().lower() != "torch"
        points = self._points(points)
        with torch.no_grad():
            xyz, features = self.rpn.backbone(points)
        return self.proposals_from_features(xyz, features, hip)

    def proposals_from_features(self, xyz, features, hip=True):
        """Everything behind the backbone: ``xyz`` [B, N, 3], ``features`` [B, C, N] (as ``rpn.backbone`` returns them) -> the dict of
        ``proposals()``."""
        pl = self.rpn.proposal_layer
        nms_post = pl.nms_post if pl.nms_post_val is None else pl.nms_post_val
        nms_thres = pl.nms_thres if pl.nms_thres_val is None else pl.nms_thres_val
        if not pl.post_process:
            raise NotImplementedError("PointRCNN (MI355X build): post_process=False is unsupported")
        with torch.no_grad():
            b, c, n = (int(v) for v in features.shape)
            rows = features.transpose(1, 2).contiguous().view(b * n, c)
            cls, reg = self._heads(rows, hip)
            args = (pl.mean_size, pl.loc_scope, pl.loc_bin_size, pl.num_head_bin, pl.loc_xz_fine, pl.get_y_by_bin, pl.loc_y_scope,
                    pl.loc_y_bin_size, pl.get_ry_fine)
            if hip:
                boxes = prcnn_ops.bin_decode(xyz.view(b * n, 3), reg, *args).view(b, n, 7)
                rois, roi_scores, roi_index = prcnn_ops.rpn_proposals(cls.view(b, n), boxes, pl.nms_pre, nms_post, nms_thres)
            else:
                boxes = _torch_decode(xyz.view(b * n, 3), reg, *args).view(b, n, 7)
                rois, roi_scores, roi_index = _torch_proposals(cls.view(b, n), boxes, pl.nms_pre, nms_post, nms_thres)
        return dict(rois=rois, roi_scores=roi_scores, roi_index=roi_index, cls=cls.view(b, n, 1), reg=reg.view(b, n, -1), xyz=xyz,
                    features=features)

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError("PointRCNN (MI355X build): inference only; call .eval()")
        if self.mode != "RPN":
            raise NotImplementedError("PointRCNN (MI355X build): the RoI stage (RoI pooling and the RCNN network) is not built; "
                                      "mode='RPN' returns the first stage's outputs and proposals() its hand-off to the second")
        r = self.proposals(inputs)
        return {"rois": r["rois"], "cls": r["cls"], "reg": r["reg"]}


# ---- the torch formulation (ML3D_PRCNN_OPS=torch) ------------------------------------------------------------------------------
def _torch_linear(a, w, b, act):
    x = a @ w + b
    return torch.relu(x) if act == 2 else x


def _torch_decode(roi, pred_reg, anchor_size, loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin, loc_y_scope,
                  loc_y_bin_size, get_ry_fine):
    """``decode_bbox_target`` (point_rcnn.py:1153-1272) with torch ops."""
    anchor = torch.tensor(anchor_size, dtype=torch.float32, device=roi.device)
    L = int(loc_scope / loc_bin_size) * 2
    Y = int(loc_y_scope / loc_y_bin_size) * 2

    def pick(lo, width, idx):
        return torch.gather(pred_reg[:, lo:lo + width], 1, idx.unsqueeze(1)).squeeze(1)

    x_bin, z_bin = torch.argmax(pred_reg[:, :L], 1), torch.argmax(pred_reg[:, L:2 * L], 1)
    pos_x = x_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
    pos_z = z_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
    off = 2 * L
    if get_xz_fine:
        pos_x = pos_x + pick(2 * L, L, x_bin) * loc_bin_size
        pos_z = pos_z + pick(3 * L, L, z_bin) * loc_bin_size
        off = 4 * L
    if get_y_by_bin:
        y_bin = torch.argmax(pred_reg[:, off:off + Y], 1)
        y_res = pick(off + Y, Y, y_bin) * loc_y_bin_size
        pos_y = y_bin.float() * loc_y_bin_size + loc_y_bin_size / 2 - loc_y_scope + y_res
        pos_y = pos_y + roi[:, 1]
        off += 2 * Y
    else:
        pos_y = roi[:, 1] + pred_reg[:, off]
        off += 1
    H = num_head_bin
    ry_bin = torch.argmax(pred_reg[:, off:off + H], 1)
    ry_norm = pick(off + H, H, ry_bin)
    if get_ry_fine:
        apc = (np.pi / 2) / H
        ry = (ry_bin.float() * apc + apc / 2) + ry_norm * (apc / 2) - np.pi / 4
    else:
        apc = (2 * np.pi) / H
        ry = (ry_bin.float() * apc + ry_norm * (apc / 2)) % (2 * np.pi)
        ry = torch.where(ry > np.pi, ry - 2 * np.pi, ry)
    hwl = pred_reg[:, off + 2 * H:off + 2 * H + 3] * anchor + anchor
    if roi.shape[1] == 7:
        ca, sa = torch.cos(-roi[:, 6]), torch.sin(-roi[:, 6])
        pos_x, pos_z = pos_x * ca - pos_z * sa, pos_x * sa + pos_z * ca
        ry = ry + roi[:, 6]
    return torch.stack((pos_x + roi[:, 0], pos_y, pos_z + roi[:, 2], hwl[:, 0], hwl[:, 1], hwl[:, 2], ry), 1)


def _torch_proposals(scores, boxes, nms_pre, nms_post, nms_thres):
    """``ProposalLayer.forward`` + ``distance_based_proposal`` (point_rcnn.py:1045-1150) as the reference writes them: a sort, and
    per item and zone boolean masks and one call of the native ``nms``.  (Stable sort: equal scores by ascending index.)"""
    b, n = scores.shape
    boxes = boxes.clone()
    boxes[..., 1] += boxes[..., 3] / 2
    order = torch.sort(scores, dim=1, descending=True, stable=True)[1]
    rois = scores.new_zeros((b, nms_post, 7))
    roi_scores = scores.new_zeros((b, nms_post))
    roi_index = torch.full((b, nms_post), -1, dtype=torch.int32, device=scores.device)
    pre = [int(nms_pre * 0.7), nms_pre - int(nms_pre * 0.7)]
    post = [int(nms_post * 0.7), nms_post - int(nms_post * 0.7)]
    bounds = [0.0, 40.0, 80.0]
    for k in range(b):
        so, po = scores[k][order[k]], boxes[k][order[k]]
        dist = po[:, 2]
        first = (dist > bounds[0]) & (dist <= bounds[1])
        at = 0
        for i in (1, 2):
            mask = (dist > bounds[i - 1]) & (dist <= bounds[i])
            if bool(mask.any()):
                idx = torch.nonzero(mask)[:, 0][:pre[i - 1]]
            elif i == 2:
                idx = torch.nonzero(first)[:, 0][pre[0]:][:pre[1]]
            else:
                continue
            if idx.numel() == 0:
                continue
            cur = po[idx]
            half_w, half_h = cur[:, 3] / 2, cur[:, 5] / 2
            bev = torch.stack((cur[:, 0] - half_w, cur[:, 2] - half_h, cur[:, 0] + half_w, cur[:, 2] + half_h, cur[:, 6]), 1)
            keep = ops.nms(bev.contiguous(), so[idx].contiguous(), nms_thres)[:post[i - 1]]
            m = int(keep.numel())
            rois[k, at:at + m] = cur[keep]
            roi_scores[k, at:at + m] = so[idx][keep]
            roi_index[k, at:at + m] = order[k][idx][keep].int()
            at += m
    return rois, roi_scores, roi_index
