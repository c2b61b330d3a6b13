"""PointNet++ multi-scale-grouping backbone (``Pointnet2MSG`` of the reference's ml3d/torch/modules/pointnet.py; Qi et al.,
NeurIPS 2017), MI355X-native INFERENCE: the module tree only holds the parameters under the reference's names (``state_dict()``
keys and shapes are the reference's); the forward folds every BatchNorm once and runs on the HIP ops -- per set-abstraction
level ``ml3d_furthest_point_sampling``, ONE ``ml3d_ball_query`` for all scales, ONE ``ml3d_linear`` with the feature rows of
the first-layer matrices of all scales side by side (once per SOURCE point; the three position rows act on the exact p_j - c_i
inside the kernel), and per scale ``ml3d_pn2_sa_mlp_max`` (or, for the wide scales, its unfused route) into its column slice of
the level's output; per feature-propagation level the exact 3-NN, ``ml3d_pn2_interpolate`` and ``ml3d_linear``.

``ML3D_PN2_OPS=torch`` (A/B switch, read per forward): the same forward written with torch ops on the GPU (``gather``, matmul,
``max``), grouping BEFORE the first convolution as the reference does, on the SAME native FPS / ball-query / 3-NN indices -- the
baseline the fused kernels are measured against and an independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _abi
from ... import ops
from ...ops import pointnet2 as pn2_ops


def _cnn(widths):
    """``gen_CNN(widths, conv=nn.Conv2d, batch_norm=nn.BatchNorm2d, bias=False)`` (torch_utils.py:26): conv at 0, 3, 6 ..."""
    layers = []
    for ci, co in zip(widths[:-1], widths[1:]):
        layers += [nn.Conv2d(ci, co, 1, bias=False), nn.BatchNorm2d(co), nn.ReLU(inplace=True)]
    return nn.Sequential(*layers)


class _SAModule(nn.Module):
    """Parameter container of ``PointnetSAModuleMSG`` (pointnet.py:163-211)."""

    def __init__(self, npoint, radii, nsamples, mlps):
        super().__init__()
        self.npoint, self.radii, self.nsamples = int(npoint), [float(r) for r in radii], [int(k) for k in nsamples]
        self.mlps = nn.ModuleList(_cnn(spec) for spec in mlps)


class _FPModule(nn.Module):
    """Parameter container of ``PointnetFPModule`` (pointnet.py:252-264)."""

    def __init__(self, mlp):
        super().__init__()
        self.mlp = _cnn(mlp)


def _fold(conv, bn):
    """-> (weights_t [in, out] float64, scale [out], shift [out]) of Conv2d(1x1, no bias) + BatchNorm2d (eval)."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return conv.weight.detach().double()[:, :, 0, 0].t(), scale, shift


def _f(t):
    return t.float().contiguous()


def _layers(seq):
    return [_fold(seq[i], seq[i + 1]) for i in range(0, len(seq), 3)]


class Pointnet2MSG(nn.Module):
    """``Pointnet2MSG(in_channels, use_xyz, SA_config, fp_mlps)`` of the reference, inference on the MI355X.  Supported: the
    ``SA_config`` form whose radius / nsample / mlps entries are lists per level (1 - 4 scales, three-layer MLPs), positive
    ``npoints``, ``use_xyz=True``, ``in_channels >= 0``."""

    def __init__(self, in_channels=6, use_xyz=True,
                 SA_config={"npoints": [128, 32], "radius": [[0.2], [0.4]], "nsample": [[64], [64]],
                            "mlps": [[[128, 128, 128]], [[128, 128, 256]]]},
                 fp_mlps=[], pool_method="max_pool", instance_norm=None, device="cuda"):
        super().__init__()
        self.device = torch.device(device) if isinstance(device, str) else device
        _abi.require_gpu(self.device, "Pointnet2MSG")
        if not use_xyz:
            raise NotImplementedError("Pointnet2MSG (MI355X build): use_xyz=False is unsupported")
        if pool_method != "max_pool" or instance_norm is not None:
            raise NotImplementedError("Pointnet2MSG (MI355X build): avg_pool / instance norm are unsupported")
        in_channels = int(in_channels)
        if in_channels < 0:
            raise ValueError("Pointnet2MSG: in_channels must be >= 0")
        levels = len(SA_config["npoints"])
        if not (len(SA_config["radius"]) == len(SA_config["nsample"]) == len(SA_config["mlps"]) == levels):
            raise ValueError("Pointnet2MSG: SA_config lists differ in length")
        self.in_channels = in_channels
        self.SA_modules = nn.ModuleList()
        skip = [in_channels]
        cin = in_channels
        for i in range(levels):
            npoint, radii, nsamples, mlps = (SA_config[k][i] for k in ("npoints", "radius", "nsample", "mlps"))
            if npoint is None or int(npoint) <= 0:
                raise NotImplementedError("Pointnet2MSG (MI355X build): GroupAll levels (npoints <= 0 or None) are unsupported")
            if not all(isinstance(v, (list, tuple)) for v in (radii, nsamples, mlps)) or not len(radii) == len(nsamples) == len(mlps):
                raise NotImplementedError("Pointnet2MSG (MI355X build): radius / nsample / mlps must be lists per level of equal "
                                          "length; the scalar form is unsupported")
            if not 1 <= len(radii) <= 4 or any(len(spec) != 3 for spec in mlps):
                raise NotImplementedError("Pointnet2MSG (MI355X build): 1 - 4 scales per level with three-layer MLPs are supported")
            self.SA_modules.append(_SAModule(npoint, radii, nsamples, [[cin + 3] + [int(c) for c in spec] for spec in mlps]))
            cin = sum(int(spec[-1]) for spec in mlps)
            skip.append(cin)
        self.FP_modules = nn.ModuleList()
        for i in range(len(fp_mlps)):
            pre = fp_mlps[i + 1][-1] if i + 1 < len(fp_mlps) else cin
            self.FP_modules.append(_FPModule([int(pre) + skip[i]] + [int(c) for c in fp_mlps[i]]))
        if len(fp_mlps) > levels:
            raise ValueError("Pointnet2MSG: more feature-propagation levels than set-abstraction levels")
        self._packed = None
        self.last_indices = None
        self.to(self.device)
        self.eval()

    # ---- folded parameters ------------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        r = super().load_state_dict(*a, **k)
        self.packed_params()
        return r

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("Pointnet2MSG (MI355X build): inference only; .train() is unsupported")
        return super().train(False)

    def packed_params(self):
        """Fold every BatchNorm and lay the weights out for the kernels, ONCE."""
        if self._packed is not None:
            return self._packed
        with torch.no_grad():
            P = dict(sa=[], fp=[])
            for sa in self.SA_modules:
                scales, w1_all = [], []
                for s, seq in enumerate(sa.mlps):
                    (w1, s1, t1), (w2, s2, t2), (w3, s3, t3) = raw = _layers(seq)
                    w1 = w1 * s1                                                  # [3 + c, c1]: position rows first
                    w1_all.append(w1[3:])
                    scales.append(dict(hip=pn2_ops.pack_sa_weights(_f(w1[:3]), _f(t1), _f(w2 * s2), _f(t2), _f(w3 * s3), _f(t3),
                                                                   sa.nsamples[s]),
                                       raw=[(_f(w), _f(sc), _f(sh)) for w, sc, sh in raw], c1=int(w1.shape[1]), c3=int(w3.shape[1])))
                P["sa"].append(dict(scales=scales, w1=_f(torch.cat(w1_all, 1))))
            for fp in self.FP_modules:
                raw = _layers(fp.mlp)
                P["fp"].append(dict(hip=[(_f(w * sc), _f(sh)) for w, sc, sh in raw], raw=[(_f(w), _f(sc), _f(sh)) for w, sc, sh in raw]))
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._packed = P
        return P

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def _sa_level(self, sa, p, xyz, feat, hip):
        """xyz [B, n, 3], feat [B * n, c] or None -> (new_xyz [B, m, 3], new_feat [B * m, sum c3], fps, ball-query indices)."""
        return sa_level(xyz, feat, sa.npoint, sa.radii, sa.nsamples, p, hip, "Pointnet2MSG")

    def _fp_level(self, p, unknown, known, skip, known_feat, hip):
        b = int(unknown.shape[0])
        d2, idx = pn2_ops.three_nn(unknown, known)
        idx2, d22 = idx.view(-1, 3), d2.view(-1, 3)
        if hip:
            x = pn2_ops.pn2_interpolate(known_feat, b, idx2, d22)
            for l, (w, sh) in enumerate(p["hip"]):
                x = ops.linear(x, w, sh, a2=skip if l == 0 else None, act=2)
        else:
            x = _torch_interpolate(known_feat, b, idx2, d22)
            if skip is not None:
                x = torch.cat((x, skip), 1)
            for w, sc, sh in p["raw"]:
                x = torch.relu((x @ w) * sc + sh)
        return x, idx

    def forward(self, pointcloud):
        """pointcloud [B, N, 3 + in_channels] -> (xyz [B, N, 3], features [B, C_out, N]), as the reference returns them."""
        if self.training:
            raise NotImplementedError("Pointnet2MSG (MI355X build): inference only; call .eval()")
        hip = os.environ.get("ML3D_PN2_OPS", "hip").strip().lower() != "torch"
        ops._gates._need_gpu(pointcloud)
        if pointcloud.dim() != 3 or pointcloud.shape[2] != 3 + self.in_channels or pointcloud.dtype != torch.float32:
            raise ValueError("Pointnet2MSG: float32 pointcloud [B, N, %d] expected" % (3 + self.in_channels))
        P = self.packed_params()
        b, n0 = int(pointcloud.shape[0]), int(pointcloud.shape[1])
        with torch.no_grad():
            l_xyz = [pointcloud[..., :3].contiguous()]
            l_feat = [pointcloud[..., 3:].contiguous().view(b * n0, self.in_channels) if self.in_channels else None]
            used = dict(fps=[], ball=[], nn3=[None] * len(self.FP_modules))
            for sa, p in zip(self.SA_modules, P["sa"]):
                new_xyz, feat, fps, idx = self._sa_level(sa, p, l_xyz[-1], l_feat[-1], hip)
                l_xyz.append(new_xyz)
                l_feat.append(feat)
                used["fps"].append(fps)
                used["ball"].append(idx)
            for i in range(-1, -(len(self.FP_modules) + 1), -1):
                l_feat[i - 1], used["nn3"][i] = self._fp_level(P["fp"][i], l_xyz[i - 1], l_xyz[i], l_feat[i - 1], l_feat[i], hip)
            self.last_indices = used
            out = l_feat[0]
            features = None if out is None else out.view(b, n0, -1).transpose(1, 2).contiguous()
        return l_xyz[0], features


# ---- one set-abstraction level on rows (Pointnet2MSG and the RCNN stage of PointRCNN) -------------------------------------------
def sa_level(xyz, feat, npoint, radii, nsamples, p, hip, who="sa_level"):
    """xyz [B, n, 3], feat [B * n, c] or None, ``p`` = dict(scales=[dict(hip=pack_sa_weights(...), raw=[(w, scale, shift)] * 3, c1,
    c3)], w1=[c, sum c1]) -> (new_xyz [B, m, 3], new_feat [B * m, sum c3], fps int32 [B, m] item-local, ball-query indices)."""
    b, n, m = int(xyz.shape[0]), int(xyz.shape[1]), npoint
    if m > n:
        raise ValueError("%s: a level samples %d of %d points" % (who, m, n))
    rows = xyz.view(b * n, 3)
    rs, nrs = np.arange(b + 1, dtype=np.int64) * n, np.arange(b + 1, dtype=np.int64) * m
    fps = ops.furthest_point_sampling(rows, rs, nrs, rs, nrs)              # GLOBAL rows
    new_xyz = rows.index_select(0, fps.long()).view(b, m, 3)
    idx = pn2_ops.ball_query(xyz, new_xyz, radii, nsamples)
    out = _sa_scales(xyz, feat, new_xyz, idx, p, hip)
    local = fps.view(b, m) - torch.arange(b, dtype=torch.int32, device=fps.device)[:, None] * n
    return new_xyz, out, local, idx


def _sa_scales(xyz, feat, new_xyz, idx, p, hip):
    b, m = int(new_xyz.shape[0]), int(new_xyz.shape[1])
    out = torch.empty((b * m, sum(s["c3"] for s in p["scales"])), dtype=torch.float32, device=xyz.device)
    y = ops.linear(feat, p["w1"]) if hip and feat is not None else None      # the feature rows of every scale's first layer
    o1 = o3 = 0
    for s, sc in enumerate(p["scales"]):
        if hip:
            pn2_ops.pn2_sa_mlp_max(None if y is None else y[:, o1:o1 + sc["c1"]], xyz, new_xyz, idx[s], sc["hip"],
                                   out=out[:, o3:o3 + sc["c3"]])
        else:
            out[:, o3:o3 + sc["c3"]] = _torch_sa(xyz, feat, new_xyz, idx[s], sc["raw"])
        o1, o3 = o1 + sc["c1"], o3 + sc["c3"]
    return out


def sa_group_all(xyz, feat, p, hip):
    """The reference's ``GroupAll`` level (pointnet2_utils.py:281; ``npoint=None``): every point of a cloud, RAW xyz (no centre is
    subtracted), one output row per cloud -- the set-abstraction body with a centre at the origin and the index list 0 .. n - 1.
    xyz [B, n, 3], feat [B * n, c] -> [B, c3]."""
    b, n = int(xyz.shape[0]), int(xyz.shape[1])
    centres = torch.zeros((b, 1, 3), dtype=torch.float32, device=xyz.device)
    idx = torch.arange(n, dtype=torch.int32, device=xyz.device).expand(b, 1, n).contiguous()
    return _sa_scales(xyz, feat, centres, [idx], p, hip)


# ---- the torch formulation (ML3D_PN2_OPS=torch) --------------------------------------------------------------------------------
def _torch_sa(xyz, feat, centres, idx, layers):
    """QueryAndGroup + the three conv / BatchNorm / ReLU + max_pool2d of one scale (pointnet2_utils.py:252-271, pointnet.py:139-157)
    on rows: -> [B * m, c3]."""
    b, m, ns = idx.shape
    n = xyz.shape[1]
    rows = (idx.long() + torch.arange(b, device=idx.device)[:, None, None] * n).reshape(-1)
    g = xyz.reshape(b * n, 3).index_select(0, rows).view(b, m, ns, 3) - centres[:, :, None, :]
    if feat is not None:
        g = torch.cat((g, feat.index_select(0, rows).view(b, m, ns, -1)), 3)
    for w, sc, sh in layers:
        g = torch.relu((g @ w) * sc + sh)
    return g.max(2)[0].reshape(b * m, -1)


def _torch_interpolate(known, batch, idx, d2):
    n, mk = idx.shape[0] // batch, known.shape[0] // batch
    rec = 1.0 / (torch.sqrt(d2) + 1e-8)
    w = rec / rec.sum(1, keepdim=True)
    rows = idx.long() + (torch.arange(batch, device=idx.device) * mk).repeat_interleave(n)[:, None]
    out = 0
    for t in range(3):
        out = out + known.index_select(0, rows[:, t]) * w[:, t:t + 1]
    return out
