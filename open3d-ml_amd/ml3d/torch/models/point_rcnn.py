"""PointRCNN (ml3d/torch/models/point_rcnn.py of the reference; Shi et al., CVPR 2019), MI355X-native STAGE 1: everything from
the point cloud to the region proposals -- the reference's ``mode="RPN"`` forward -- and STAGE 2 behind ``proposals()``: RoI
pooling, the RCNN network and ``inference_end``.  The module tree holds the parameters of the WHOLE model under the reference's
names (``state_dict()`` keys and shapes are the reference's, a reference checkpoint loads with ``strict=True``).  ``forward`` with
``mode="RCNN"`` still raises (the class is not registered over the reference's); stage 2 is reached through ``rcnn_forward`` /
``rcnn_from_proposals`` / ``rcnn_network`` / ``inference_end``.

Stage 1 on the device: the ``Pointnet2MSG`` backbone (ml3d/torch/modules/pointnet.py), the two heads with their BatchNorms folded
once in float64 on the shared GEMM over rows [B * N, 128] (the first layers of both heads as ONE product, their weights side by
side; Dropout is the identity in eval), ``ml3d_bin_decode`` for all B * N rows and ``ml3d_rpn_proposals`` for the whole batch
(include/ml3d_hip.h, "PointRCNN stage 1") -- no ``torch.cat`` / ``torch.sort`` and no Python loop over items or zones.

Stage 2 on the device: ``ml3d_roi_pool`` writes the ``pts_input`` rows [B * M, S, 5 + C] in one launch (pooling on the enlarged
boxes, the two extra columns, the canonical transform); the network runs on rows in CHUNKS of rois (they are independent):
``xyz_up_layer`` and ``merge_down_layer`` on the shared GEMM (the merge as [xyz_feature | rpn_feature] W with the second block read
in place from ``pts_input``: no concat), the ``PointnetSAModule`` levels through ``modules.pointnet.sa_level`` on R clouds of S
points (FPS, ``ml3d_ball_query``, ``pn2_sa_mlp_max``), the last level as ``sa_group_all``, both heads on the [R, c] rows of all
chunks together; ``inference_end`` decodes with ``ml3d_bin_decode`` (roi width 7), runs ``ml3d_nms`` per item and reads back once.

``ML3D_PRCNN_OPS=torch`` (A/B switch, read per forward): the same stages behind the SAME backbone output (stage 2: the SAME
``pts_input`` and the same FPS / ball-query ops) written with torch ops on the GPU (matmul, ``argmax``, ``gather``, ``sort``,
boolean masks, the native ``nms`` per zone, as the reference's Python loop does) -- the baseline the kernels are measured against
and an independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _abi
from ... import ops
from ...ops import pointnet2 as pn2_ops
from ...ops import pointrcnn as prcnn_ops
from ..modules.pointnet import Pointnet2MSG, sa_group_all, sa_level

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
    """The reference's ``RCNN`` (point_rcnn.py:743-916) under its names and shapes; ``network`` is its forward behind
    ``pts_input`` (:889-910), on rows.  No BatchNorm in this half: every conv has a bias and a ReLU, the last of a head is plain."""

    def __init__(self, num_classes, in_channels=128,
                 SA_config={"npoints": [128, 32, -1], "radius": [0.2, 0.4, 100], "nsample": [64, 64, 64],
                            "mlps": [[128, 128, 128], [128, 128, 256], [256, 256, 512]]},
                 cls_out_ch=[256, 256], reg_out_ch=[256, 256], db_ratio=0.5, use_xyz=True, xyz_up_layer=[128, 128], head={},
                 target_head={}, loss={}):
        super().__init__()
        self.rcnn_input_channel = 5
        self.pool_extra_width = float(target_head.get("pool_extra_width", 1.0))
        self.num_points = int(target_head.get("num_points", 512))
        levels = len(SA_config["npoints"])
        self.npoints = [None if int(v) == -1 else int(v) for v in SA_config["npoints"]]
        self.radius = [float(v) for v in SA_config["radius"]]
        self.nsample = [int(v) for v in SA_config["nsample"]]
        # (stage 1 runs with any of these; the RCNN network refuses them when it packs its weights)
        self._stage2_ok = bool(use_xyz) and levels >= 1 and self.npoints[-1] is None and None not in self.npoints[:-1] and \
            all(len(spec) == 3 for spec in SA_config["mlps"])
        self._packed = None
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
        self.cls_channel, self.reg_channel = cls_channel, reg_channel

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def packed_params(self):
        """Transposed float32 weights for the row GEMM and the set-abstraction kernels, ONCE."""
        if self._packed is not None:
            return self._packed
        if not self._stage2_ok:
            raise NotImplementedError("PointRCNN (MI355X build): the RCNN stage needs use_xyz, three-layer SA MLPs and npoints -1 "
                                      "(GroupAll) at the last level only")

        def convs(seq):
            mods = [m for m in seq if isinstance(m, (nn.Conv1d, nn.Conv2d))]
            return [(m.weight.detach().reshape(m.weight.shape[0], -1).t().float().contiguous(), m.bias.detach().float().contiguous(),
                     0 if (m is mods[-1] and isinstance(m, nn.Conv1d)) else 2) for m in mods]

        with torch.no_grad():
            P = dict(up=convs(self.xyz_up_layer), merge=convs(self.merge_down_layer)[0], cls=convs(self.cls_blocks),
                     reg=convs(self.reg_blocks), sa=[])
            entering = self.num_points
            for i, sa in enumerate(self.SA_modules):
                (w1, b1, _), (w2, b2, _), (w3, b3, _) = raw = convs(sa.mlps[0])            # w1 [3 + c, c1]: position rows first
                nsample = entering if self.npoints[i] is None else self.nsample[i]
                one = dict(hip=pn2_ops.pack_sa_weights(w1[:3].contiguous(), b1, w2, b2, w3, b3, nsample),
                           raw=[(w, torch.ones_like(b), b) for w, b, _ in raw], c1=int(w1.shape[1]), c3=int(w3.shape[1]))
                P["sa"].append(dict(scales=[one], w1=w1[3:].contiguous()))
                entering = self.npoints[i]
        self._packed = P
        return P

    def _up_merge(self, pts, hip):
        """pts [R, S, 5 + C] contiguous -> (xyz [R, S, 3], rows [R * S, c] behind ``xyz_up_layer`` and ``merge_down_layer``)."""
        P = self.packed_params()
        r, s, width = (int(v) for v in pts.shape)
        if s != self.num_points:
            raise ValueError("PointRCNN: pts_input holds %d points per roi, the RCNN stage is built for %d" % (s, self.num_points))
        rows = pts.view(r * s, width)
        x = rows[:, :self.rcnn_input_channel]
        for w, b, act in P["up"]:
            x = pn2_ops._linear_rows(x, w, b, act) if hip else _torch_linear(x, w, b, act)
        w, b, act = P["merge"]
        if hip:                                                  # [xyz_feature | rpn_feature] W, the second block read in place
            return pts[..., :3].contiguous(), pn2_ops._linear_rows(x, w, b, act, a2=rows[:, self.rcnn_input_channel:])
        return pts[..., :3].contiguous(), _torch_linear(torch.cat((x, rows[:, self.rcnn_input_channel:]), 1), w, b, act)

    def _level(self, i, xyz, feat, hip):
        """Level i of ``SA_modules`` -> (new_xyz or None, rows, fps or None, ball-query indices or None)."""
        p = self.packed_params()["sa"][i]
        if self.npoints[i] is None:
            return None, sa_group_all(xyz, feat, p, hip), None, None
        xyz, feat, fps, idx = sa_level(xyz, feat, self.npoints[i], [self.radius[i]], [self.nsample[i]], p, hip, "PointRCNN")
        return xyz, feat, fps, idx[0]

    def _sa_stack(self, pts, hip):
        """pts [R, S, 5 + C] contiguous -> (rows [R, c] behind the GroupAll level, fps per level, ball-query indices per level)."""
        xyz, feat = self._up_merge(pts, hip)
        fps, ball = [], []
        for i in range(len(self.SA_modules)):
            xyz, feat, f, idx = self._level(i, xyz, feat, hip)
            if f is not None:
                fps.append(f)
                ball.append(idx)
        return feat, fps, ball

    def _heads(self, rows, hip):
        out = {}
        for name in ("cls", "reg"):
            x = rows
            for w, b, act in self.packed_params()[name]:
                x = pn2_ops._linear_rows(x, w, b, act) if hip else _torch_linear(x, w, b, act)
            out[name] = x
        return out

    def network(self, pts_input, hip=True, chunk=64):
        """``RCNN.forward`` behind ``pts_input`` [R, S, 5 + C]: -> dict(cls [R, cls_channel], reg [R, reg_channel], fps / ball: the
        per-level index arrays).  Rois are independent: the levels run in chunks of ``chunk`` rois (the grouped intermediates of
        512 rois x 128 centres x 64 samples x 128 floats are 2 GB each), the heads on all rows together."""
        if pts_input.dim() != 3 or pts_input.dtype != torch.float32 or not pts_input.is_contiguous() or pts_input.shape[2] <= 5:
            raise ValueError("PointRCNN: pts_input float32 contiguous [R, S, 5 + C] expected")
        r, chunk = int(pts_input.shape[0]), max(int(chunk), 1)
        if r < 1:
            raise ValueError("PointRCNN: pts_input holds no roi")
        with torch.no_grad():
            parts = [self._sa_stack(pts_input[lo:lo + chunk], hip) for lo in range(0, r, chunk)]
            rows = torch.cat([p[0] for p in parts]) if len(parts) != 1 else parts[0][0]
            out = self._heads(rows, hip)
            levels = len(parts[0][1]) if parts else 0
            out["fps"] = [torch.cat([p[1][l] for p in parts]) for l in range(levels)]
            out["ball"] = [torch.cat([p[2][l] for p in parts]) for l in range(levels)]
        return out


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
        self.rcnn._packed = None
        if self.rcnn._stage2_ok:
            self.rcnn.packed_params()
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
                    features=features, feature_rows=rows)

    # ---- stage 2 --------------------------------------------------------------------------------------------------------------
    def _stage2_checks(self):
        if self.training:
            raise NotImplementedError("PointRCNN (MI355X build): inference only; call .eval()")
        if self.rcnn.cls_channel != 1:
            raise NotImplementedError("PointRCNN (MI355X build): the RCNN stage supports one score column (cls_channel == 1) only")
        if self.rcnn.proposal_layer.post_process:
            raise NotImplementedError("PointRCNN (MI355X build): rcnn.head.post_process=True is unsupported")
        return os.environ.get("ML3D_PRCNN_OPS", "hip").strip().lower() != "torch"

    def rcnn_network(self, pts_input, chunk=64):
        """The RCNN network alone on given rows ``pts_input`` [R, S, 5 + C] -> dict(cls [R, 1], reg [R, C_reg], fps, ball)."""
        hip = self._stage2_checks()
        ops._gates._need_gpu(pts_input)
        return self.rcnn.network(pts_input, hip, chunk)

    def rcnn_from_proposals(self, r, chunk=64):
        """``r`` = the dict of ``proposals()`` -> the reference's RCNN-mode output ``rois`` [B, M, 7], ``cls`` [B * M, 1], ``reg``
        [B * M, C_reg], and ``pts_input`` [B * M, S, 5 + C], ``pool_idx`` int32 [B, M, S], ``empty`` int32 [B, M], ``fps`` / ``ball``
        (the RCNN levels' index arrays)."""
        hip = self._stage2_checks()
        xyz, rois = r["xyz"], r["rois"]
        b, n = int(xyz.shape[0]), int(xyz.shape[1])
        with torch.no_grad():
            rows = r.get("feature_rows")
            if rows is None:
                rows = r["features"].transpose(1, 2).contiguous().view(b * n, -1)
            scores = r["cls"].reshape(b, n)
            pool = prcnn_ops.roi_pool if hip else _torch_roi_pool
            pts_input, pool_idx, empty = pool(xyz, rows, scores, rois, self.rcnn.num_points, self.score_thres, self.rcnn.pool_extra_width)
        net = self.rcnn.network(pts_input, hip, chunk)
        return dict(rois=rois, cls=net["cls"], reg=net["reg"], pts_input=pts_input, pool_idx=pool_idx, empty=empty, fps=net["fps"],
                    ball=net["ball"])

    def rcnn_forward(self, points, chunk=64):
        """``rcnn_from_proposals(proposals(points))``: both stages."""
        self._stage2_checks()
        return self.rcnn_from_proposals(self.proposals(points), chunk)

    def rcnn_boxes(self, results):
        """The device half of ``inference_end``: ``rcnn.proposal_layer`` with ``post_process=False`` (point_rcnn.py:1020-1077) and the
        scoring -> (boxes [B, M, 7] decoded, scores [B, M] = sigmoid(cls), keep int64 [B, M]: per item the NMS survivors in
        descending score, count int64 [B]).  Nothing is read back."""
        hip = self._stage2_checks()
        pl = self.rcnn.proposal_layer
        rois = results["rois"]
        b, m = int(rois.shape[0]), int(rois.shape[1])
        nms_thres = pl.nms_thres if pl.nms_thres_val is None else pl.nms_thres_val
        args = (pl.mean_size, pl.loc_scope, pl.loc_bin_size, pl.num_head_bin, pl.loc_xz_fine, pl.get_y_by_bin, pl.loc_y_scope,
                pl.loc_y_bin_size, pl.get_ry_fine)
        with torch.no_grad():
            raw = results["cls"].reshape(b, m).contiguous()
            reg = results["reg"].reshape(b * m, -1)
            flat = rois.reshape(b * m, 7).contiguous()
            boxes = (prcnn_ops.bin_decode(flat, reg, *args) if hip else _torch_decode(flat, reg, *args)).view(b, m, 7)
            half_w, half_h = boxes[..., 3] / 2, boxes[..., 5] / 2           # xywhr_to_xyxyr of columns [0, 2, 3, 5, 6]
            bev = torch.stack((boxes[..., 0] - half_w, boxes[..., 2] - half_h, boxes[..., 0] + half_w, boxes[..., 2] + half_h,
                               boxes[..., 6]), 2).contiguous()
            keep = torch.zeros((b, m), dtype=torch.int64, device=rois.device)
            count = torch.zeros((b,), dtype=torch.int64, device=rois.device)
            lib = _abi.get()
            wsb = int(lib.ml3d_nms_workspace_bytes(m))
            ws = ops._gates._ws(wsb, rois.device)
            with torch.cuda.device(rois.device):
                for k in range(b if m else 0):
                    rc = lib.ml3d_nms(bev[k].data_ptr(), raw[k].data_ptr(), m, float(nms_thres), keep[k].data_ptr(), count[k:].data_ptr(),
                                      ws.data_ptr(), wsb, ops._gates._stream())
                    _abi.check(rc, "ml3d_nms")
            return boxes, torch.sigmoid(raw), keep, count

    def inference_end(self, results, inputs):
        """point_rcnn.py:375-427 on the output of ``rcnn_forward``: decode, per-item rotated NMS on the raw scores, sigmoid, keep
        ``score > score_thres``, one box object per detection (``dim = box[[4, 3, 5]]``, camera -> world, ``z += dim[1] / 2``).  With
        an Open3D-ML checkout on the path the objects are its ``BEVBox3D``, stand-alone ``DetectedBox`` records (point_pillars.py).
        ONE read-back, at the end.  A missing calibration is the identity."""
        if self.mode == "RPN":
            return [[]]
        try:
            from ml3d.datasets.utils import BEVBox3D as Box       # the reference's class when a checkout is importable
        except Exception:
            from .point_pillars import DetectedBox as Box
        boxes, scores, keep, count = self.rcnn_boxes(results)
        b, m = int(boxes.shape[0]), int(boxes.shape[1])
        host = torch.cat((boxes.reshape(-1).double(), scores.reshape(-1).double(), keep.reshape(-1).double(), count.double())).cpu().numpy()
        boxes = host[:b * m * 7].astype(np.float32).reshape(b, m, 7)
        scores = host[b * m * 7:b * m * 8].astype(np.float32).reshape(b, m)
        keep, count = host[b * m * 8:b * m * 9].astype(np.int64).reshape(b, m), host[b * m * 9:].astype(np.int64)
        calibs = list(getattr(inputs, "calib", None) or [])
        name = self.lbl2name.get(0, "ignore")
        detections = []
        for i in range(b):
            calib = (calibs[i] if i < len(calibs) else None) or {}
            world_cam, cam_img = calib.get("world_cam", None), calib.get("cam_img", None)
            kept = keep[i, :count[i]]
            kept = kept[scores[i, kept] > np.float32(self.score_thres)]
            found = []
            for j in kept:
                box = boxes[i, j]
                dim = box[[4, 3, 5]]
                pos = _cam2world(box[:3], world_cam)
                pos = pos + [0, 0, dim[1] / 2]
                found.append(Box(pos, dim, box[6], name, scores[i, j], world_cam, cam_img))
            detections.append(found)
        return detections

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError("PointRCNN (MI355X build): inference only; call .eval()")
        if self.mode != "RPN":
            raise NotImplementedError("PointRCNN (MI355X build): forward does not run the RoI stage (RoI pooling and the RCNN network): "
                                      "call rcnn_forward(points), or rcnn_from_proposals(proposals()) behind proposals(), then "
                                      "inference_end; mode='RPN' returns the first stage's outputs")
        r = self.proposals(inputs)
        return {"rois": r["rois"], "cls": r["cls"], "reg": r["reg"]}


# ---- the torch formulation (ML3D_PRCNN_OPS=torch) ------------------------------------------------------------------------------
def _torch_linear(a, w, b, act):
    x = a @ w + b
    return torch.relu(x) if act == 2 else x


def _cam2world(pos, world_cam):
    """``DataProcessing.cam2world`` (dataprocessing.py:176-217) for one point."""
    if world_cam is None:
        return np.asarray(pos, np.float64)
    world_cam = np.asarray(world_cam)
    rot = np.linalg.inv(world_cam[:3, :3])
    cam_world = np.concatenate([np.concatenate([rot, world_cam[3:, :3] @ -rot], 0), [[0], [0], [0], [1]]], 1)
    return np.matmul(np.hstack((np.asarray(pos).reshape(1, 3), np.ones((1, 1), np.float32))), cam_world)[..., :3].flatten()


def _torch_roi_pool(xyz, feat, scores, rois, num_points, score_thres, extra_width):
    """The contract of ``ml3d_roi_pool`` (include/ml3d_hip.h) with torch ops, per item a [M, N] mask: the op-level cross-check."""
    b, n, m, s = int(xyz.shape[0]), int(xyz.shape[1]), int(rois.shape[1]), int(num_points)
    c = int(feat.shape[1])
    dev = xyz.device
    big = rois.clone()
    big[..., 3:6] += extra_width * 2
    big[..., 1] += extra_width
    pts_input = torch.zeros((b * m, s, 5 + c), dtype=torch.float32, device=dev)
    pool_idx = torch.full((b, m, s), -1, dtype=torch.int32, device=dev)
    seg = (torch.sigmoid(scores) > score_thres).float()
    depth = torch.norm(xyz, p=2, dim=2) / 70.0 - 0.5
    slot = torch.arange(s, device=dev)[None]
    for k in range(b):
        p, q = xyz[k][None], big[k][:, None]                                    # [1, N, 3], [M, 1, 7]
        half = q[..., 3] / 2
        dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - (q[..., 1] - half), p[..., 2] - q[..., 2]
        ca, sa = torch.cos(q[..., 6]), torch.sin(q[..., 6])
        xr, zr = dx * ca + dz * (-sa), dx * sa + dz * ca
        inside = ~((dx.abs() > 10.0) | (dy.abs() > half) | (dz.abs() > 10.0)) & (xr >= -q[..., 5] / 2) & (xr <= q[..., 5] / 2) & \
            (zr >= -q[..., 4] / 2) & (zr <= q[..., 4] / 2)
        cnt = inside.sum(1)
        order = torch.sort((~inside).to(torch.uint8), dim=1, stable=True)[1]     # the hits first, in ascending point index
        idx = torch.gather(order, 1, slot % torch.clamp(cnt, 1, s)[:, None])
        some = (cnt > 0)[:, None]
        pool_idx[k] = torch.where(some, idx, torch.full_like(idx, -1)).int()
        src = torch.where(some, idx, torch.zeros_like(idx))
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        pk = torch.where(some[..., None], xyz[k][src], zero)                      # [M, S, 3]; an empty roi pools the origin
        d = pk - rois[k][:, None, :3]
        ca, sa = torch.cos(rois[k][:, None, 6]), torch.sin(rois[k][:, None, 6])
        out = pts_input[k * m:(k + 1) * m]
        out[..., 0], out[..., 1], out[..., 2] = d[..., 0] * ca - d[..., 2] * sa, d[..., 1], d[..., 0] * sa + d[..., 2] * ca
        out[..., 3], out[..., 4] = torch.where(some, seg[k][src], zero), torch.where(some, depth[k][src], zero)
        out[..., 5:] = torch.where(some[..., None], feat[k * n:(k + 1) * n][src], zero)
    return pts_input, pool_idx, (pool_idx[..., 0] < 0).int()


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
