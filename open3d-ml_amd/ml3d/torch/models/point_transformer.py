"""PointTransformer (ml3d/torch/models/point_transformer.py of the reference; Zhao et al., ICCV 2021), MI355X-native
INFERENCE: the module tree only holds the parameters under the reference's names (``state_dict()`` keys and shapes are the
reference's, a reference checkpoint loads unchanged); the forward folds every BatchNorm once and runs on the HIP ops --
``ml3d_knn_search`` (one search per level and use: 13 where the reference makes 44 for the S3DIS config),
``ml3d_furthest_point_sampling``, ``ml3d_linear``, ``ml3d_pt_attention``, ``ml3d_pt_transition_down``,
``ml3d_pt_interpolate``.  An extension beyond SURVEY.md's scope table.

``ML3D_PT_OPS=torch`` (A/B switch, read per forward): the same forward written with torch ops on the GPU
(``index_select``, matmul, ``softmax``) on the SAME native k-NN / FPS indices -- the baseline the fused kernels are measured
against and an independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _abi
from ... import ops
from ...ops import pointtransformer as pt_ops
from . import _datapath
from .kpconv import _Cfg

PLANES = (32, 64, 128, 256, 512)
STRIDE = (1, 4, 4, 4, 4)
NSAMPLE = (8, 16, 16, 16, 16)
SHARE_PLANES = 8
MIN_COARSE_POINTS = 16


def min_item_points():
    """Fewest points an item may have: 16 (the coarsest level's nsample) must survive four stride-4 samplings."""
    n = MIN_COARSE_POINTS
    for s in STRIDE[1:]:
        n *= s
    return n


# ---- parameter containers under the reference's names (point_transformer.py:377-413, 470-494, 539-566, 603-627) ---------------
class _Transformer(nn.Module):

    def __init__(self, planes):
        super().__init__()
        s = planes // SHARE_PLANES
        self.linear_q = nn.Linear(planes, planes)
        self.linear_k = nn.Linear(planes, planes)
        self.linear_v = nn.Linear(planes, planes)
        self.linear_p = nn.Sequential(nn.Linear(3, 3), nn.BatchNorm1d(3), nn.ReLU(inplace=True), nn.Linear(3, planes))
        self.linear_w = nn.Sequential(nn.BatchNorm1d(planes), nn.ReLU(inplace=True), nn.Linear(planes, s), nn.BatchNorm1d(s),
                                      nn.ReLU(inplace=True), nn.Linear(s, s))
        self.softmax = nn.Softmax(dim=1)


class _TransitionDown(nn.Module):

    def __init__(self, in_planes, out_planes, stride, nsample):
        super().__init__()
        self.stride, self.nsample = stride, nsample
        if stride != 1:
            self.linear = nn.Linear(3 + in_planes, out_planes, bias=False)
            self.pool = nn.MaxPool1d(nsample)
        else:
            self.linear = nn.Linear(in_planes, out_planes, bias=False)
        self.bn = nn.BatchNorm1d(out_planes)
        self.relu = nn.ReLU(inplace=True)


class _TransitionUp(nn.Module):

    def __init__(self, in_planes, out_planes=None):
        super().__init__()
        self.is_head = out_planes is None
        if out_planes is None:
            self.linear1 = nn.Sequential(nn.Linear(2 * in_planes, in_planes), nn.BatchNorm1d(in_planes), nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(nn.Linear(in_planes, in_planes), nn.ReLU(inplace=True))
        else:
            self.linear1 = nn.Sequential(nn.Linear(out_planes, out_planes), nn.BatchNorm1d(out_planes), nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(nn.Linear(in_planes, out_planes), nn.BatchNorm1d(out_planes), nn.ReLU(inplace=True))


class _Bottleneck(nn.Module):

    def __init__(self, planes):
        super().__init__()
        self.linear1 = nn.Linear(planes, planes, bias=False)
        self.bn1 = nn.BatchNorm1d(planes)
        self.transformer2 = _Transformer(planes)
        self.bn2 = nn.BatchNorm1d(planes)
        self.linear3 = nn.Linear(planes, planes, bias=False)
        self.bn3 = nn.BatchNorm1d(planes)
        self.relu = nn.ReLU(inplace=True)


# ---- BatchNorm folding (float64 on the host side of the arithmetic, float32 results) -----------------------------------------
def _bn(bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def _f(t):
    return t.float().contiguous()


def _fold_linear(lin, bn=None):
    """-> (weights_t [in, out], bias [out] or None) of Linear (+ BatchNorm) for ``ops.linear``."""
    w = lin.weight.detach().double()
    b = None if lin.bias is None else lin.bias.detach().double()
    if bn is not None:
        s, t = _bn(bn)
        w = w * s[:, None]
        b = t if b is None else b * s + t
    return _f(w.t()), None if b is None else _f(b)


def _pack_bottleneck(blk):
    tr = blk.transformer2
    c = tr.linear_q.weight.shape[0]
    s = c // SHARE_PLANES
    R = pt_ops.attention_hidden_rows(c)
    p = dict()
    p["w1t"], p["b1"] = _fold_linear(blk.linear1, blk.bn1)
    wq, bq = _fold_linear(tr.linear_q)
    wk, bk = _fold_linear(tr.linear_k)
    wv, bv = _fold_linear(tr.linear_v)
    p["wqkv_t"], p["bqkv"] = torch.cat((wq, wk, wv), 1).contiguous(), torch.cat((bq, bk, bv)).contiguous()
    sp, tp = _bn(tr.linear_p[1])
    a = dict()
    a["p_w1"] = _f(tr.linear_p[0].weight.detach().double() * sp[:, None])
    a["p_b1"] = _f(tr.linear_p[0].bias.detach().double() * sp + tp)
    a["p_w2t"] = _f(tr.linear_p[3].weight.detach().t())
    a["p_b2"] = _f(tr.linear_p[3].bias.detach())
    s0, t0 = _bn(tr.linear_w[0])
    a["w_scale0"], a["w_shift0"] = _f(s0), _f(t0)
    s1, t1 = _bn(tr.linear_w[3])
    w1 = torch.zeros((R, c), dtype=torch.float64, device=s1.device)
    b1 = torch.zeros((R,), dtype=torch.float64, device=s1.device)
    w1[:s] = tr.linear_w[2].weight.detach().double() * s1[:, None]
    b1[:s] = tr.linear_w[2].bias.detach().double() * s1 + t1
    a["w_w1"], a["w_b1"] = _f(w1), _f(b1)
    a["w_w2"], a["w_b2"] = _f(tr.linear_w[5].weight.detach()), _f(tr.linear_w[5].bias.detach())
    p["attn"] = a
    s2, t2 = _bn(blk.bn2)
    p["ep"] = (_f(s2), _f(t2))
    p["w3t"], p["b3"] = _fold_linear(blk.linear3, blk.bn3)
    return p


# ---- the torch formulation of the three fused ops (ML3D_PT_OPS=torch) ---------------------------------------------------------
def _torch_linear(a, wt, bias=None, residual=None, act=0):
    y = a @ wt
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual
    return torch.relu(y) if act == 2 else y


def _torch_attention(qkv, points, idx, a, ep):
    n, ns = idx.shape
    c = qkv.shape[1] // 3
    s = c // SHARE_PLANES
    flat = idx.reshape(-1).long()
    q, kv = qkv[:, :c], qkv.index_select(0, flat)
    k, v = kv[:, c:2 * c].view(n, ns, c), kv[:, 2 * c:].view(n, ns, c)
    d = points.index_select(0, flat).view(n, ns, 3) - points[:, None, :]
    h = torch.relu(d @ a["p_w1"].t() + a["p_b1"])
    r = h @ a["p_w2t"] + a["p_b2"]
    u = torch.relu((k - q[:, None, :] + r) * a["w_scale0"] + a["w_shift0"])
    g = torch.relu(u @ a["w_w1"][:s].t() + a["w_b1"][:s])
    w = torch.softmax(g @ a["w_w2"].t() + a["w_b2"], dim=1)
    out = ((v + r).view(n, ns, SHARE_PLANES, s) * w[:, :, None, :]).sum(1).view(n, c)
    return out if ep is None else torch.relu(out * ep[0] + ep[1])


def _torch_transition_down(feat, points, sample_idx, idx, w_f_t, w_x, scale, shift):
    m, ns = idx.shape
    flat = idx.reshape(-1).long()
    d = points.index_select(0, flat).view(m, ns, 3) - points.index_select(0, sample_idx.long())[:, None, :]
    x = torch.cat((d, feat.index_select(0, flat).view(m, ns, -1)), 2)
    y = torch.relu((x @ torch.cat((w_x, w_f_t), 0)) * scale + shift)
    return y.max(1)[0]


def _torch_interpolate(a, b, idx, d2):
    rec = 1.0 / (d2 + 1e-8)
    w = rec / rec.sum(1, keepdim=True)
    new = torch.zeros_like(a)
    for t in range(idx.shape[1]):
        new += b.index_select(0, idx[:, t].long()) * w[:, t:t + 1]
    return a + new


class PointTransformer(nn.Module):
    """Semantic segmentation with PointTransformer, inference on the MI355X (constructor arguments, state_dict layout and
    data-path methods of the reference's class; ``.train()`` + forward is not implemented yet)."""

    def __init__(self, name="PointTransformer", blocks=[2, 2, 2, 2, 2], in_channels=6, num_classes=13, voxel_size=0.04,
                 max_voxels=80000, batcher='ConcatBatcher', augment=None, device='cuda', **kwargs):
        super().__init__()
        blocks = [int(b) for b in blocks]
        if len(blocks) != 5 or min(blocks) < 1:
            raise ValueError("PointTransformer: blocks must list five positive block counts")
        self.cfg = _Cfg(name=name, blocks=blocks, in_channels=in_channels, num_classes=num_classes, voxel_size=voxel_size,
                        max_voxels=max_voxels, batcher=batcher, augment=augment, **kwargs)
        self.name = name
        self.device = torch.device(device) if isinstance(device, str) else device
        _abi.require_gpu(self.device, "PointTransformer")
        self.in_channels = in_channels
        in_planes = in_channels
        self.encoders = nn.ModuleList()
        for i in range(5):
            layers = [_TransitionDown(in_planes, PLANES[i], STRIDE[i], NSAMPLE[i])]
            in_planes = PLANES[i]
            layers += [_Bottleneck(in_planes) for _ in range(1, blocks[i])]
            self.encoders.append(nn.Sequential(*layers))
        self.decoders = nn.ModuleList()
        for i in range(4, -1, -1):
            layers = [_TransitionUp(in_planes, None if i == 4 else PLANES[i])]
            in_planes = PLANES[i]
            layers += [_Bottleneck(in_planes)]          # (the reference builds its decoders with two layers each)
            self.decoders.append(nn.Sequential(*layers))
        self.cls = nn.Sequential(nn.Linear(PLANES[0], PLANES[0]), nn.BatchNorm1d(PLANES[0]), nn.ReLU(inplace=True),
                                 nn.Linear(PLANES[0], num_classes))
        self._packed = None
        self.inference_input = None
        self.last_indices = None
        self.to(self.device)
        self.eval()

    # ---- folded parameters ------------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def train(self, mode=True):
        self._packed = None
        return super().train(mode)

    def invalidate_packed(self):
        self._packed = None

    def packed_params(self):
        """Fold every BatchNorm and lay the weights out for the kernels, ONCE; the device is synchronised before the pack is
        published, so a forward on any stream may read it."""
        if self._packed is not None:
            return self._packed
        with torch.no_grad():
            P = dict(enc=[], dec=[])
            for i, enc in enumerate(self.encoders):
                td = enc[0]
                s, t = _bn(td.bn)
                e = dict()
                if td.stride == 1:
                    e["wt"], e["b"] = _fold_linear(td.linear, td.bn)
                else:
                    w = td.linear.weight.detach()
                    e["w_x"], e["w_f_t"] = _f(w[:, :3].t()), _f(w[:, 3:].t())
                    e["scale"], e["shift"] = _f(s), _f(t)
                e["blocks"] = [_pack_bottleneck(b) for b in list(enc)[1:]]
                P["enc"].append(e)
            for dec in self.decoders:
                tu = dec[0]
                d = dict()
                if tu.is_head:
                    d["w1t"], d["b1"] = _fold_linear(tu.linear1[0], tu.linear1[1])
                    d["w2t"], d["b2"] = _fold_linear(tu.linear2[0])
                else:
                    d["w1t"], d["b1"] = _fold_linear(tu.linear1[0], tu.linear1[1])
                    d["w2t"], d["b2"] = _fold_linear(tu.linear2[0], tu.linear2[1])
                d["blocks"] = [_pack_bottleneck(b) for b in list(dec)[1:]]
                P["dec"].append(d)
            P["cls1"] = _fold_linear(self.cls[0], self.cls[1])
            P["cls2"] = _fold_linear(self.cls[3])
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._packed = P
        return P

    # ---- forward ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _host_row_splits(batch):
        host = getattr(batch, "row_splits_host", None)
        if host is None:
            rs = batch.row_splits
            host = rs.detach().cpu().numpy() if torch.is_tensor(rs) else rs      # (a device tensor costs one read-back)
        return np.ascontiguousarray(host, dtype=np.int64).reshape(-1)

    def _bottleneck(self, p, x, points, idx, hip):
        if hip:
            y = ops.linear(x, p["w1t"], p["b1"], act=2)
            qkv = ops.linear(y, p["wqkv_t"], p["bqkv"])
            y = pt_ops.pt_attention(qkv, points, idx, p["attn"], epilogue=p["ep"])
            return ops.linear(y, p["w3t"], p["b3"], residual=x, act=2)
        y = _torch_linear(x, p["w1t"], p["b1"], act=2)
        qkv = _torch_linear(y, p["wqkv_t"], p["bqkv"])
        y = _torch_attention(qkv, points, idx, p["attn"], p["ep"])
        return _torch_linear(y, p["w3t"], p["b3"], residual=x, act=2)

    def forward(self, batch):
        """batch: ``point`` [n, 3], ``feat`` [n, in_channels - 3], ``row_splits`` int64 [b + 1] (and, to avoid a read-back,
        ``row_splits_host``: ``PointTransformerBatch`` carries it) -> logits [n, num_classes]."""
        if self.training:
            raise NotImplementedError("PointTransformer (MI355X build): inference only; call .eval() (training is a follow-up)")
        hip = os.environ.get("ML3D_PT_OPS", "hip").strip().lower() != "torch"
        lin = ops.linear if hip else _torch_linear
        P = self.packed_params()
        dev = self.device
        rs_host = [self._host_row_splits(batch)]
        lens = np.diff(rs_host[0])
        for b, n_b in enumerate(lens):
            if n_b < min_item_points():
                raise ValueError("PointTransformer: batch item %d has %d points; every item needs at least %d (16 on the "
                                 "coarsest of the five levels)" % (b, n_b, min_item_points()))
        for s in STRIDE[1:]:
            lens = lens // s
            rs_host.append(np.concatenate(([0], np.cumsum(lens))).astype(np.int64))
        rs_dev = [torch.from_numpy(r).to(dev, non_blocking=True) for r in rs_host]
        p0 = batch.point.to(dev).float().contiguous()
        x = p0 if self.in_channels == 3 else torch.cat((p0, batch.feat.to(dev).float()), 1).contiguous()
        if p0.shape[0] != rs_host[0][-1] or x.shape[1] != self.in_channels:
            raise ValueError("PointTransformer: point / feat / row_splits do not fit together")

        def knn(l_pts, l_q, k, dist=False):
            r = ops.knn_search(points[l_pts], points[l_q], k, rs_dev[l_pts], rs_dev[l_q], return_distances=dist)
            return (r.neighbors_index, r.neighbors_distance) if dist else r.neighbors_index

        # ---- encoder: level l = 0 .. 4 with PLANES[l] channels ------------------------------------------------------------
        points, feats, self_idx = [p0], [], []
        used = dict(fps=[], knn_self=self_idx, knn_down=[], knn_up=[])      # the indices of this forward, for inspection
        for l in range(5):
            e = P["enc"][l]
            if l == 0:
                x = lin(x, e["wt"], e["b"], act=2)
            else:
                fps = pt_ops.furthest_point_sampling(points[l - 1], rs_dev[l - 1], rs_dev[l], rs_host[l - 1], rs_host[l])
                used["fps"].append(fps)
                points.append(points[l - 1].index_select(0, fps.long()))
                r = ops.knn_search(points[l - 1], points[l], NSAMPLE[l], rs_dev[l - 1], rs_dev[l])
                used["knn_down"].append(r.neighbors_index)
                down = pt_ops.pt_transition_down if hip else _torch_transition_down
                x = down(x, points[l - 1], fps, r.neighbors_index, e["w_f_t"], e["w_x"], e["scale"], e["shift"])
                if hip:
                    x = x[1]
            self_idx.append(knn(l, l, NSAMPLE[l]))
            for blk in e["blocks"]:
                x = self._bottleneck(blk, x, points[l], self_idx[l], hip)
            feats.append(x)
        # ---- decoder --------------------------------------------------------------------------------------------------------
        d = P["dec"][0]
        x = feats[4]
        glob = torch.cat([x[int(s):int(e)].sum(0, keepdim=True) / float(e - s) for s, e in zip(rs_host[4][:-1], rs_host[4][1:])], 0)
        glob = lin(glob.contiguous(), d["w2t"], d["b2"], act=2)
        rep = torch.cat([glob[b:b + 1].expand(int(e - s), -1) for b, (s, e) in enumerate(zip(rs_host[4][:-1], rs_host[4][1:]))], 0)
        x = lin(torch.cat((x, rep), 1).contiguous(), d["w1t"], d["b1"], act=2)
        for blk in d["blocks"]:
            x = self._bottleneck(blk, x, points[4], self_idx[4], hip)
        for l in range(3, -1, -1):
            d = P["dec"][4 - l]
            a = lin(feats[l], d["w1t"], d["b1"], act=2)
            bsrc = lin(x, d["w2t"], d["b2"], act=2)
            idx3, d3 = knn(l + 1, l, 3, dist=True)
            used["knn_up"].insert(0, idx3)
            x = pt_ops.pt_interpolate(a, bsrc, idx3, d3) if hip else _torch_interpolate(a, bsrc, idx3, d3)
            for blk in d["blocks"]:
                x = self._bottleneck(blk, x, points[l], self_idx[l], hip)
        self.last_indices = used
        x = lin(x, P["cls1"][0], P["cls1"][1], act=2)
        return lin(x, P["cls2"][0], P["cls2"][1])

    # ---- data path (point_transformer.py:198-337) -----------------------------------------------------------------------------
    def preprocess(self, data, attr):
        """Grid subsampling on the native op after moving the cloud's minimum corner to the origin; for the test split
        ``proj_inds`` (nearest sub-cloud point of every ORIGINAL point) from a k = 1 ``ml3d_knn_search``."""
        cfg = self.cfg
        points = np.array(data['point'][:, 0:3], dtype=np.float32)
        if cfg.voxel_size:
            points = points - np.min(points, 0)
            return _datapath.preprocess_segmentation(dict(data, point=points), attr, cfg.voxel_size, self.device)
        labels = np.zeros((points.shape[0],), np.int32) if data.get('label') is None else \
            np.array(data['label'], dtype=np.int32).reshape((-1,))
        feat = None if data.get('feat') is None else np.array(data['feat'], dtype=np.float32)
        out = dict(point=points, feat=feat, label=labels, search_tree=_datapath.GpuSearchTree(points, self.device))
        if attr['split'] in ("test", "testing"):
            out['proj_inds'] = np.arange(points.shape[0], dtype=np.int32)
        return out

    def transform(self, data, attr):
        """Test / validation transform: the ``max_voxels`` crop around the middle point (validation only), centring on the
        bounding-box middle, ``feat / 255``.  (Training augmentation belongs to the training follow-up.)"""
        cfg = self.cfg
        if attr['split'] in ('training', 'train'):
            raise NotImplementedError("PointTransformer (MI355X build): the training transform is a follow-up")
        points, feat, labels = np.array(data['point'], np.float32), data['feat'], data['label']
        if attr['split'] not in ('test', 'testing') and cfg.max_voxels and labels.shape[0] > cfg.max_voxels:
            init_idx = labels.shape[0] // 2
            crop_idx = np.argsort(np.sum(np.square(points - points[init_idx]), 1))[:cfg.max_voxels]
            points, labels = points[crop_idx], labels[crop_idx]
            feat = None if feat is None else feat[crop_idx]
        points_min, points_max = np.min(points, 0), np.max(points, 0)
        points -= (points_min + points_max) / 2.0
        out = dict(data)
        out['point'] = torch.from_numpy(points).to(torch.float32)
        if feat is not None:
            out['feat'] = torch.from_numpy(np.asarray(feat)).to(torch.float32) / 255.0
        out['label'] = torch.from_numpy(np.asarray(labels)).to(torch.int64)
        return out

    def update_probs(self, inputs, results, test_probs):
        result = results.reshape(-1, self.cfg.num_classes)
        probs = torch.nn.functional.softmax(result, dim=-1).cpu().data.numpy()
        sampler = getattr(self, "trans_point_sampler", None)
        if sampler is not None:
            sampler(patchwise=False)
        return probs

    def inference_begin(self, data):
        data = self.preprocess(data, {'split': 'test'})
        self.inference_input = self.transform(data, {'split': 'test'})

    def inference_preprocess(self):
        return self.inference_input

    def make_batch(self, transformed):
        from ..dataloaders import PointTransformerBatch
        return PointTransformerBatch([{'data': transformed}]).to(self.device)

    def inference_end(self, inputs, results):
        results = torch.reshape(results, (-1, self.cfg.num_classes))
        probs = torch.softmax(results, dim=-1).cpu().data.numpy()
        probs = np.reshape(probs, [-1, self.cfg.num_classes])[self.inference_input['proj_inds']]
        return {'predict_labels': np.argmax(probs, 1), 'predict_scores': probs}
