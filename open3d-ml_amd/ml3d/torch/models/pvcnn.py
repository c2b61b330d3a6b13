"""PVCNN (ml3d/torch/models/pvcnn.py of the reference; Liu et al., NeurIPS 2019), MI355X-native INFERENCE: the module tree
only holds the parameters under the reference's names (``state_dict()`` keys and shapes are the reference's, a reference
checkpoint loads unchanged); the forward folds every BatchNorm once and runs on rows [B * N, C] with the HIP ops --
``ml3d_pvcnn_voxel_coords`` (ONE normalisation per forward where the reference repeats it per PVConv), ``ml3d_avg_voxelize``,
``ml3d_conv3d_ndhwc_bf16x3``, ``ml3d_trilinear_devoxelize``, ``ml3d_segment_max_rows`` and the bf16x3 Linears.  Every block
writes its fused feature into its column slice of one [B * N, concat] buffer (no ``torch.cat``); the classifier's first layer
is split by linearity, so the per-cloud feature enters as a [B, 512] product through the gathered residual of
``ml3d_linear_bf16x3_gathered`` and nothing [B, 128, N] is ever repeated.  An extension beyond SURVEY.md's scope table.

``ML3D_PVCNN_OPS=torch`` (A/B switch, read per forward): the same forward written with torch ops on the GPU (``index_add_``,
``F.conv3d``, gathers, matmul) on the SAME native voxel coordinates -- the baseline the kernels are measured against and an
independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _abi
from ... import ops
from ...ops import pvcnn as pv_ops
from .kpconv import _Cfg

BLOCKS = ((64, 1, 32), (64, 2, 16), (128, 1, 16), (1024, 1, None))      # (out_channels, num_blocks, voxel_resolution)
CLOUD = (256, 128)
CLASSIFIER = (512, 256)


# ---- parameter containers under the reference's names (pvcnn.py:352-355, 455-486, 504-557) ------------------------------------
class SharedMLP(nn.Module):

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.layers = nn.Sequential(nn.Conv1d(in_channels, out_channels, 1), nn.BatchNorm1d(out_channels), nn.ReLU(True))


class PVConv(nn.Module):

    def __init__(self, in_channels, out_channels, resolution):
        super().__init__()
        self.in_channels, self.out_channels, self.resolution = in_channels, out_channels, int(resolution)
        self.voxel_layers = nn.Sequential(
            nn.Conv3d(in_channels, out_channels, 3, stride=1, padding=1), nn.BatchNorm3d(out_channels, eps=1e-4),
            nn.LeakyReLU(0.1, True),
            nn.Conv3d(out_channels, out_channels, 3, stride=1, padding=1), nn.BatchNorm3d(out_channels, eps=1e-4),
            nn.LeakyReLU(0.1, True))
        self.point_features = SharedMLP(in_channels, out_channels)


def _linear_bn_relu(in_channels, out_channels):
    return nn.Sequential(nn.Linear(in_channels, out_channels), nn.BatchNorm1d(out_channels), nn.ReLU(True))


# ---- BatchNorm folding (float64 on the host side of the arithmetic, float32 results) -----------------------------------------
def _bn(bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def _fold(weight, bias, bn=None, pad_to=None):
    """Conv1d [out, in, 1] / Linear [out, in] (+ BatchNorm) -> (weights_t [in or pad_to, out] float32, bias [out] float32)."""
    w = weight.detach().double().reshape(weight.shape[0], -1)
    b = bias.detach().double()
    if bn is not None:
        s, t = _bn(bn)
        w, b = w * s[:, None], b * s + t
    wt = w.t()
    if pad_to is not None and pad_to > wt.shape[0]:
        wt = torch.cat((wt, torch.zeros((pad_to - wt.shape[0], wt.shape[1]), dtype=wt.dtype, device=wt.device)), 0)
    return wt.float().contiguous(), b.float().contiguous()


# ---- the torch formulation of the ops (ML3D_PVCNN_OPS=torch) --------------------------------------------------------------------
def _torch_avg_voxelize(feat, vox, batch, r, cg):
    n, c = feat.shape[0] // batch, feat.shape[1]
    flat = (vox.long() + torch.div(torch.arange(batch * n, device=feat.device), n, rounding_mode='floor') * (r ** 3))
    grid = torch.zeros((batch * r ** 3, cg), dtype=torch.float32, device=feat.device)
    grid[:, :c].index_add_(0, flat, feat)
    cnt = torch.zeros((batch * r ** 3,), dtype=torch.float32, device=feat.device)
    cnt.index_add_(0, flat, torch.ones_like(flat, dtype=torch.float32))
    return (grid / cnt.clamp(min=1)[:, None]).view(batch, r, r, r, cg)


def _torch_conv3d(x, w, bias, cout):
    """x [B, r, r, r, cin] channels-last, w [27 cin, cout] as the kernel takes it."""
    cin = x.shape[4]
    w5 = w.view(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    y = F.leaky_relu(F.conv3d(x.permute(0, 4, 1, 2, 3), w5, bias, stride=1, padding=1), 0.1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _torch_devoxelize(grid, v, addend, out):
    B, r, c = grid.shape[0], grid.shape[1], grid.shape[4]
    n = v.shape[0] // B
    lo = torch.floor(v)
    f = v - lo
    lo_i = lo.long().clamp(0, r - 1)
    hi_i = (lo_i + (f > 0).long()).clamp(max=r - 1)
    base = torch.div(torch.arange(B * n, device=v.device), n, rounding_mode='floor') * (r ** 3)
    g = grid.reshape(B * r ** 3, c)
    acc = torch.zeros((v.shape[0], c), dtype=torch.float32, device=v.device)
    for k in range(8):
        ix = hi_i[:, 0] if k & 4 else lo_i[:, 0]
        iy = hi_i[:, 1] if k & 2 else lo_i[:, 1]
        iz = hi_i[:, 2] if k & 1 else lo_i[:, 2]
        w = (f[:, 0] if k & 4 else 1 - f[:, 0]) * (f[:, 1] if k & 2 else 1 - f[:, 1]) * (f[:, 2] if k & 1 else 1 - f[:, 2])
        acc += g.index_select(0, base + (ix * r + iy) * r + iz) * w[:, None]
    out.copy_(acc if addend is None else acc + addend)
    return out


def _torch_linear(a, wt, bias, act, out=None, residual=None):
    y = a @ wt
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual
    y = torch.relu(y) if act == 2 else y
    if out is None:
        return y
    out.copy_(y)
    return out


class PVCNN(nn.Module):
    """Semantic segmentation with Point-Voxel convolutions, inference on the MI355X (constructor arguments, state_dict layout
    and data-path methods of the reference's class; ``.train()`` + forward is not implemented)."""

    def __init__(self, name='PVCNN', device="cuda", num_classes=13, num_points=40960, extra_feature_channels=6,
                 width_multiplier=1, voxel_resolution_multiplier=1, batcher='DefaultBatcher', augment=None, **kwargs):
        super().__init__()
        self.cfg = _Cfg(name=name, num_classes=num_classes, num_points=num_points, extra_feature_channels=extra_feature_channels,
                        width_multiplier=width_multiplier, voxel_resolution_multiplier=voxel_resolution_multiplier,
                        batcher=batcher, augment=augment, **kwargs)
        self.name = name
        self.device = torch.device(device) if isinstance(device, str) else device
        _abi.require_gpu(self.device, "PVCNN")
        self.rng = np.random.default_rng(kwargs.get('seed', None))
        self.in_channels = extra_feature_channels + 3
        r, vr = width_multiplier, voxel_resolution_multiplier
        layers, cin, concat = [], self.in_channels, 0
        for oc, num, res in BLOCKS:
            oc = int(r * oc)
            for _ in range(num):
                layers.append(SharedMLP(cin, oc) if res is None else PVConv(cin, oc, int(vr * res)))
                cin = oc
                concat += oc
        self.point_features = nn.ModuleList(layers)
        self.concat_channels = concat
        cloud, c = [], cin
        for oc in CLOUD:
            cloud.append(_linear_bn_relu(c, int(r * oc)))
            c = int(r * oc)
        self.cloud_features = nn.Sequential(*cloud)
        self.cloud_channels = c
        c1, c2 = int(r * CLASSIFIER[0]), int(r * CLASSIFIER[1])
        self.classifier = nn.Sequential(SharedMLP(concat + c, c1), nn.Dropout(0.3), SharedMLP(c1, c2), nn.Dropout(0.3),
                                        nn.Conv1d(c2, num_classes, 1))
        widths = [m.layers[0].out_channels if isinstance(m, SharedMLP) else m.out_channels for m in self.point_features]
        if any(w % 32 for w in widths + [concat, c1, c2]) or any(m.resolution < 1 or m.resolution > 64 for m in self.point_features
                                                               if isinstance(m, PVConv)):
            raise NotImplementedError("PVCNN (MI355X build): every layer width must be a multiple of 32 and every voxel resolution "
                                      "in [1, 64] (got widths %s)" % (widths + [c1, c2],))
        self._packed = None
        self.inference_input = None
        self.last_voxels = None
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

    @staticmethod
    def _pack_linear(weight, bias, bn=None, pad_to=None):
        wt, b = _fold(weight, bias, bn, pad_to)
        return dict(wt=wt, b=b, n=int(wt.shape[1]), packed=ops.pack_bf16x3(wt))

    def packed_params(self):
        """Fold every BatchNorm (BatchNorm3d with its eps of 1e-4, the others 1e-5; float64) and split the weights into their
        bf16x3 planes, ONCE and eagerly; the device is synchronised before the pack is published, so a forward on any stream may
        read it."""
        if self._packed is not None:
            return self._packed
        with torch.no_grad():
            P = dict(blocks=[])
            cin = self.in_channels
            for m in self.point_features:
                if isinstance(m, PVConv):
                    vl = m.voxel_layers
                    e = dict(kind="pvconv", r=m.resolution, cout=m.out_channels, cin_pad=pv_ops.pad32(cin))
                    for tag, conv, bn in (("c1", vl[0], vl[1]), ("c2", vl[3], vl[4])):
                        s, t = _bn(bn)
                        w, b, _ = pv_ops.pack_conv3d_weights(conv.weight, s, t, conv.bias)
                        e[tag] = dict(w=w, b=b, packed=ops.pack_bf16x3(w))
                    pt = m.point_features.layers
                    e["pt"] = self._pack_linear(pt[0].weight, pt[0].bias, pt[1], pad_to=pv_ops.pad32(cin))
                    cin = m.out_channels
                else:
                    e = dict(kind="mlp", cout=m.layers[0].out_channels)
                    e["pt"] = self._pack_linear(m.layers[0].weight, m.layers[0].bias, m.layers[1])
                    cin = e["cout"]
                P["blocks"].append(e)
            P["cloud"] = [_fold(seq[0].weight, seq[0].bias, seq[1]) for seq in self.cloud_features]
            c0 = self.classifier[0].layers
            wt, b = _fold(c0[0].weight, c0[0].bias, c0[1])
            main = wt[:self.concat_channels].contiguous()
            P["cls1"] = dict(wt=main, b=b, n=int(wt.shape[1]), packed=ops.pack_bf16x3(main))
            P["cls1_cloud"] = wt[self.concat_channels:].contiguous()          # [cloud channels, c1]: the per-item half
            c2 = self.classifier[2].layers
            P["cls2"] = self._pack_linear(c2[0].weight, c2[0].bias, c2[1])
            P["cls3"] = self._pack_linear(self.classifier[4].weight, self.classifier[4].bias)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._packed = P
        return P

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, inputs):
        """inputs: ``point`` (B, 3, N) float32, ``feat`` (B, extra_feature_channels + 3, N) float32 -> logits (B, N, num_classes)."""
        if self.training:
            raise NotImplementedError("PVCNN (MI355X build): inference only; call .eval() (training is out of scope)")
        hip = os.environ.get("ML3D_PVCNN_OPS", "hip").strip().lower() != "torch"
        P = self.packed_params()
        dev = self.device
        coords = inputs['point'].to(dev, non_blocking=True).float().contiguous()
        feat = inputs['feat'].to(dev, non_blocking=True).float()
        if coords.dim() != 3 or coords.shape[1] != 3 or feat.dim() != 3 or feat.shape[1] != self.in_channels or \
                feat.shape[0] != coords.shape[0] or feat.shape[2] != coords.shape[2]:
            raise ValueError("PVCNN: point (B, 3, N) and feat (B, %d, N) expected" % self.in_channels)
        B, _, N = coords.shape
        rows = B * N

        def lin(a, p, act, out=None, residual=None, gather=None):
            if hip:
                return pv_ops.linear_rows_bf16x3(a, p["packed"], p["n"], p["b"], act=act, out=out, residual=residual,
                                                 residual_gather=gather)
            if gather is not None:
                residual = residual.index_select(0, gather.long())
            return _torch_linear(a, p["wt"], p["b"], act, out=out, residual=residual)

        # the voxel coordinates of every resolution, once (native in both modes: a flipped voxel is no rounding difference)
        res = sorted(set(e["r"] for e in P["blocks"] if e["kind"] == "pvconv"))
        stats, vox = pv_ops.pvcnn_voxel_coords(coords, res)
        self.last_voxels = dict(stats=stats, vox={r: vox[r][1].view(B, N) for r in res})

        x = torch.zeros((rows, pv_ops.pad32(self.in_channels)), dtype=torch.float32, device=dev)
        x[:, :self.in_channels] = feat.transpose(1, 2).reshape(rows, self.in_channels)
        cat = torch.empty((rows, self.concat_channels), dtype=torch.float32, device=dev)
        off = 0
        for e in P["blocks"]:
            out = cat[:, off:off + e["cout"]]
            if e["kind"] == "pvconv":
                v, idx = vox[e["r"]]
                if hip:
                    g = pv_ops.avg_voxelize(x, idx, B, e["r"], out_channels=e["cin_pad"])
                    g = pv_ops.conv3d_ndhwc(g, e["c1"]["packed"], e["c1"]["b"], e["cout"])
                    g = pv_ops.conv3d_ndhwc(g, e["c2"]["packed"], e["c2"]["b"], e["cout"])
                    lin(x, e["pt"], 2, out=out)
                    pv_ops.trilinear_devoxelize(g, v, addend=out, out=out)
                else:
                    g = _torch_avg_voxelize(x, idx, B, e["r"], e["cin_pad"])
                    g = _torch_conv3d(g, e["c1"]["w"], e["c1"]["b"], e["cout"])
                    g = _torch_conv3d(g, e["c2"]["w"], e["c2"]["b"], e["cout"])
                    _torch_devoxelize(g, v, lin(x, e["pt"], 2), out)
            else:
                lin(x, e["pt"], 2, out=out)
            x = out
            off += e["cout"]
        # ---- the per-cloud feature (B rows) and its half of the classifier's first layer ---------------------------------------
        glob = pv_ops.segment_max_rows(x, B) if hip else x.reshape(B, N, -1).max(1)[0]
        for wt, b in P["cloud"]:
            glob = ops.linear(glob.contiguous(), wt, b, act=2) if hip else _torch_linear(glob, wt, b, 2)
        item_half = ops.linear(glob, P["cls1_cloud"]) if hip else glob @ P["cls1_cloud"]
        item = torch.div(torch.arange(rows, dtype=torch.int32, device=dev), N, rounding_mode='floor')
        h = lin(cat, P["cls1"], 2, residual=item_half, gather=item)
        h = lin(h, P["cls2"], 2)                  # (Dropout is the identity in eval mode)
        return lin(h, P["cls3"], 0).view(B, N, -1)

    # ---- data path (pvcnn.py:162-282) -----------------------------------------------------------------------------------------
    def preprocess(self, data, attr):
        """pvcnn.py:162-230: min-shifted points, ``feat`` = [x, y, z, colour / 255, x / max x, y / max y, z / max z], ``num_points``
        rows drawn by the model's generator (with replacement only when the cloud is smaller); point / feat come out (3, N) /
        (9, N).  The training augmentation is out of scope."""
        if attr['split'] in ('training', 'train'):
            raise NotImplementedError("PVCNN (MI355X build): the training augmentation is out of scope")
        info = torch.utils.data.get_worker_info()
        if info:
            rng = np.random.default_rng(np.random.SeedSequence(info.seed + info.id).spawn(1)[0])
        else:
            rng = self.rng
        points = np.array(data['point'], dtype=np.float32)
        if 'label' not in data or data['label'] is None:
            labels = np.zeros((points.shape[0],), dtype=np.int32)
        else:
            labels = np.array(data['label'], dtype=np.int32).reshape((-1,))
        feat = points.copy() if data.get('feat') is None else np.array(data['feat'], dtype=np.float32)
        points -= np.min(points, 0)
        feat = feat / 255.0
        norm = points / np.max(points, 0)
        feat = np.concatenate([points, feat, norm], axis=-1)
        choices = rng.choice(points.shape[0], self.cfg.num_points, replace=(points.shape[0] < self.cfg.num_points))
        return dict(point=points[choices].transpose(), feat=feat[choices].transpose(), label=labels[choices])

    def transform(self, data, attr):
        data['point'] = torch.from_numpy(np.ascontiguousarray(data['point']))
        data['feat'] = torch.from_numpy(np.ascontiguousarray(data['feat']))
        data['label'] = torch.from_numpy(np.ascontiguousarray(data['label']))
        return data

    def update_probs(self, inputs, results, test_probs):
        result = results.reshape(-1, self.cfg.num_classes)
        probs = torch.nn.functional.softmax(result, dim=-1).cpu().data.numpy()
        sampler = getattr(self, "trans_point_sampler", None)
        if sampler is not None:
            sampler(patchwise=False)
        return probs

    def inference_begin(self, data):
        data = self.preprocess(data, {'split': 'test'})
        data['batch_lengths'] = [data['point'].shape[0]]
        self.inference_input = self.transform(data, {})

    def inference_preprocess(self):
        return self.inference_input

    def make_batch(self, transformed):
        from ..dataloaders import DefaultBatcher
        return DefaultBatcher().collate_fn([{k: transformed[k] for k in ('point', 'feat', 'label')}])

    def inference_end(self, inputs, results):
        results = torch.reshape(results, (-1, self.cfg.num_classes))
        probs = torch.softmax(results, dim=-1).cpu().data.numpy()
        probs = np.reshape(probs, [-1, self.cfg.num_classes])
        return {'predict_labels': np.argmax(probs, 1), 'predict_scores': probs}
