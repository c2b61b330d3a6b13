"""SparseConvUnet (ml3d/torch/models/sparseconvnet.py of the reference; Graham et al., CVPR 2018), MI355X-native INFERENCE:
the module tree only holds the parameters under the reference's names (``state_dict()`` keys and shapes are the reference's
with the wheel's ``SparseConv`` layers as ``kernel`` + ``offset``, a reference checkpoint loads unchanged); the forward builds
the voxel pyramid and every rulebook with ONE ``ml3d_scn_build`` (one read-back: the vector of level sizes), folds the
BatchNorms once and runs every convolution -- submanifold 3 x 3 x 3, strided 2 x 2 x 2, transposed 2 x 2 x 2 and the final
Linear gathered through ``index_map`` -- on ``ml3d_sparse_conv_bf16x3``.  The contract of the wheel's layers is UNPINNED
(include/ml3d_hip.h).  An extension beyond SURVEY.md's scope table.

Fusions.  Plain blocks (``residual_blocks=False``): the raw output of a convolution is only ever consumed through BatchNorm +
ReLU, so the consumer's BatchNorm is folded into the producer (scaled weight columns, shift as bias, ReLU epilogue); the one
value with TWO consumers (the skip: the strided convolution's BatchNorm and the left half of the BatchNorm behind JoinFeat) is
stored raw and activated by two ``ml3d_scn_bn_relu`` passes, the second straight into the left column slice of the join
buffer; the transposed convolution writes the right slice (no ``torch.cat``).  Residual blocks: the raw input is needed by the
shortcut, so BatchNorm1 + ReLU is one rows pass, BatchNorm2 + ReLU is folded into the first convolution, and the shortcut is
the residual epilogue of the second (identity) or a second dense column block of the same GEMM (``NetworkInNetwork``'s Linear).

``ML3D_SCN_OPS=torch`` (A/B switch, read per forward): the same forward written with torch ops on the GPU (``index_select``,
masked matmul) on the SAME native rulebooks and the same folded weights -- the baseline the kernel is measured against
and an independent second implementation for the cross-check test."""
import os

import numpy as np
import torch
import torch.nn as nn

from ... import _abi
from ... import ops
from ...ops import sparseconv as sc_ops
from .kpconv import _Cfg

LEVELS = 7
BN_EPS = 1e-4


# ---- parameter containers under the reference's names -------------------------------------------------------------------------
class _SparseKernel(nn.Module):
    """The wheel's SparseConv / SparseConvTranspose as a parameter holder: ``kernel`` [k, k, k, Cin, Cout], ``offset`` [3]."""

    def __init__(self, in_channels, filters, k, offset):
        super().__init__()
        self.kernel = nn.Parameter(torch.empty(k, k, k, in_channels, filters).uniform_(-1, 1) / float(np.sqrt(k ** 3 * in_channels)))
        self.register_buffer("offset", torch.full((3,), float(offset)))


class _Conv(nn.Module):
    """SubmanifoldSparseConv (k = 3, offset 0), Convolution / DeConvolution (k = 2, offset -0.5)."""

    def __init__(self, kind, in_channels, filters):
        super().__init__()
        self.kind = kind
        self.net = _SparseKernel(in_channels, filters, 3 if kind == "sub" else 2, 0.0 if kind == "sub" else -0.5)


class BatchNormBlock(nn.Module):

    def __init__(self, m):
        super().__init__()
        self.bn = nn.BatchNorm1d(m, eps=BN_EPS, momentum=0.01)


class LinearBlock(nn.Module):

    def __init__(self, a, b):
        super().__init__()
        self.linear = nn.Linear(a, b)


class NetworkInNetwork(nn.Module):

    def __init__(self, a, b):
        super().__init__()
        self.linear = nn.Identity() if a == b else nn.Linear(a, b, bias=False)


class ResidualBlock(nn.Module):

    def __init__(self, a, b):
        super().__init__()
        self.lin = NetworkInNetwork(a, b)
        self.batch_norm1 = BatchNormBlock(a)
        self.sub_sparse_conv1 = _Conv("sub", a, b)
        self.batch_norm2 = BatchNormBlock(b)
        self.sub_sparse_conv2 = _Conv("sub", b, b)


class _Marker(nn.Module):
    """ReLUBlock / ConcatFeat / JoinFeat: no parameters, they only keep the reference's positions in ``unet.net``."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind


class UNet(nn.Module):

    def __init__(self, reps, planes, residual):
        super().__init__()
        layers = []

        def block(a, b):
            if residual:
                layers.append(ResidualBlock(a, b))
            else:
                layers.extend([BatchNormBlock(a), _Marker("relu"), _Conv("sub", a, b)])

        def level(p):
            for _ in range(reps):
                block(p[0], p[0])
            if len(p) > 1:
                layers.extend([_Marker("concat"), BatchNormBlock(p[0]), _Marker("relu"), _Conv("down", p[0], p[1])])
                level(p[1:])
                layers.extend([BatchNormBlock(p[1]), _Marker("relu"), _Conv("up", p[1], p[0]), _Marker("join")])
                for i in range(reps):
                    block(p[0] * (2 if i == 0 else 1), p[0])

        level(list(planes))
        self.net = nn.ModuleList(layers)


def _bn(block):
    bn = block.bn
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


class SparseConvUnet(nn.Module):
    """Semantic segmentation with submanifold sparse convolutions, inference on the MI355X (constructor arguments, state_dict
    layout and data-path methods of the reference's class; ``.train()`` + forward is not implemented)."""

    def __init__(self, name="SparseConvUnet", device="cuda", multiplier=16, voxel_size=0.05, conv_block_reps=1,
                 residual_blocks=False, in_channels=3, num_classes=20, grid_size=4096, batcher='ConcatBatcher', augment=None,
                 **kwargs):
        super().__init__()
        self.cfg = _Cfg(name=name, multiplier=multiplier, voxel_size=voxel_size, conv_block_reps=conv_block_reps,
                        residual_blocks=residual_blocks, in_channels=in_channels, num_classes=num_classes, grid_size=grid_size,
                        batcher=batcher, augment=augment, **kwargs)
        self.name = name
        self.device = torch.device(device) if isinstance(device, str) else device
        _abi.require_gpu(self.device, "SparseConvUnet")
        if int(conv_block_reps) < 1 or int(in_channels) != 3 or int(multiplier) % 16 or not 1 <= int(grid_size) <= 4096:
            raise NotImplementedError("SparseConvUnet (MI355X build): conv_block_reps >= 1, in_channels == 3 (InputLayer averages "
                                      "three columns), multiplier a multiple of 16 and grid_size <= 4096 required")
        self.rng = np.random.default_rng(kwargs.get('seed', None))
        self.multiplier, self.reps, self.residual = int(multiplier), int(conv_block_reps), bool(residual_blocks)
        m = self.multiplier
        self.planes = [m * (i + 1) for i in range(LEVELS)]
        self.sub_sparse_conv = _Conv("sub", in_channels, m)
        self.unet = UNet(self.reps, self.planes, self.residual)
        self.batch_norm = BatchNormBlock(m)
        self.linear = LinearBlock(m, num_classes)
        self._packed = None
        self.inference_input = None
        self.last_pyramid = None
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
    def _pack(kernel, post=None, extra=None, cp=None):
        """-> dict(w [K, n] float32, b, packed, n, cp, k2, act): ``post`` = the BatchNormBlock folded in behind (then ReLU)."""
        scale, shift = (None, None) if post is None else _bn(post)
        w, b, cp, k2 = sc_ops.pack_sparse_weights(kernel, cp=cp, scale=scale, shift=shift, extra=extra)
        return dict(w=w, b=b, packed=ops.pack_bf16x3(w), n=int(w.shape[1]), cp=cp, k2=k2, act=2 if post is not None else 0,
                    taps=int(w.shape[0] - k2) // cp)

    @staticmethod
    def _pack_bn(block, sl=None):
        s, t = _bn(block)
        if sl is not None:
            s, t = s[sl], t[sl]
        return s.float().contiguous(), t.float().contiguous()

    def packed_params(self):
        """Fold every BatchNorm (eps 1e-4, float64) and split the weights into their bf16x3 planes, ONCE and eagerly; the
        device is synchronised before the pack is published, so a forward on any stream may read it."""
        if self._packed is not None:
            return self._packed
        net = list(self.unet.net)
        with torch.no_grad():
            P = dict()
            if self.residual:
                tree = self._residual_tree(net)
                P["stem"] = self._pack(self.sub_sparse_conv.net.kernel)
                P["bn_out"] = self._pack_bn(self.batch_norm)
            else:
                tree, first_bn = self._plain_tree(net)
                P["stem"] = self._pack(self.sub_sparse_conv.net.kernel, post=first_bn)
            P["tree"] = tree
            lw = self.linear.linear.weight.detach().t()                     # [m, classes]
            P["head"] = self._pack(lw.reshape(1, lw.shape[0], lw.shape[1]))
            P["head"]["b"] = self.linear.linear.bias.detach().float().contiguous()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._packed = P
        return P

    def _residual_tree(self, net):
        """``residual_blocks=True``: every block wants its input raw (the shortcut), so nothing is folded across a block
        boundary; inside a block BatchNorm2 + ReLU is folded into the first convolution."""
        pos = [0]

        def take():
            m = net[pos[0]]
            pos[0] += 1
            return m

        def blocks():
            out = []
            for _ in range(self.reps):
                mod = take()
                lin = mod.lin.linear
                extra = None if isinstance(lin, nn.Identity) else lin.weight.detach().t()
                out.append(dict(bn1=self._pack_bn(mod.batch_norm1),
                                c1=self._pack(mod.sub_sparse_conv1.net.kernel, post=mod.batch_norm2),
                                c2=self._pack(mod.sub_sparse_conv2.net.kernel, extra=extra), identity=extra is None))
            return out

        def level(l):
            e = dict(pre=blocks())
            if l < LEVELS - 1:
                _, bn_d, _, down = take(), take(), take(), take()
                e.update(bn_d=self._pack_bn(bn_d), down=self._pack(down.net.kernel), sub=level(l + 1))
                bn_u, _, up, _ = take(), take(), take(), take()
                e.update(bn_u=self._pack_bn(bn_u), up=self._pack(up.net.kernel), post=blocks())
            return e

        return level(0)

    def _plain_tree(self, net):
        """``residual_blocks=False``: every convolution knows the BatchNorm of its single consumer, so the tree is packed in
        two steps -- collect (BatchNorm, convolution) in order, then fold each convolution with the BatchNorm that follows it."""
        pos = [0]

        def take():
            m = net[pos[0]]
            pos[0] += 1
            return m

        def blocks():
            out = []
            for _ in range(self.reps):
                bn, _, conv = take(), take(), take()
                out.append(dict(bn=bn, kernel=conv.net.kernel))
            return out

        def level(l):
            e = dict(pre=blocks())
            if l < LEVELS - 1:
                _, bn_d, _, down = take(), take(), take(), take()
                e.update(bn_d_mod=bn_d, down_kernel=down.net.kernel, sub=level(l + 1))
                bn_u, _, up, _ = take(), take(), take(), take()
                e.update(bn_u_mod=bn_u, up_kernel=up.net.kernel, post=blocks())
            return e

        tree = level(0)

        def fold(e, l, post_out):
            """post_out: the BatchNormBlock behind this level's last convolution."""
            deepest = "sub" not in e
            seq = e["pre"]
            for i, blk in enumerate(seq):
                nxt = seq[i + 1]["bn"] if i + 1 < len(seq) else (post_out if deepest else None)
                blk["c"] = self._pack(blk["kernel"], post=nxt)
            if deepest:
                return
            a = self.planes[l]
            e["bn_d"] = self._pack_bn(e["bn_d_mod"])
            e["down"] = self._pack(e["down_kernel"], post=e["sub"]["pre"][0]["bn"])
            fold(e["sub"], l + 1, e["bn_u_mod"])
            bn_j = e["post"][0]["bn"]
            s, t = _bn(bn_j)
            w, b, cp, _ = sc_ops.pack_sparse_weights(e["up_kernel"], scale=s[a:], shift=t[a:])
            e["up"] = dict(w=w, b=b, packed=ops.pack_bf16x3(w), n=int(w.shape[1]), cp=cp, k2=0, act=2, taps=8)
            e["bn_jl"] = (s[:a].float().contiguous(), t[:a].float().contiguous())
            seq = e["post"]
            for i, blk in enumerate(seq):
                nxt = seq[i + 1]["bn"] if i + 1 < len(seq) else post_out
                blk["c"] = self._pack(blk["kernel"], post=nxt)

        fold(tree, 0, self.batch_norm)
        return tree, tree["pre"][0]["bn"]

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, inputs):
        """inputs: ``point`` / ``feat`` lists of [n_i, 3] float32 tensors (voxel centres, colours), ``batch_lengths`` -> logits
        [sum n_i, num_classes] in input point order."""
        if self.training:
            raise NotImplementedError("SparseConvUnet (MI355X build): inference only; call .eval() (training is out of scope)")
        hip = os.environ.get("ML3D_SCN_OPS", "hip").strip().lower() != "torch"
        P = self.packed_params()
        dev = self.device
        get = (lambda k: inputs[k]) if isinstance(inputs, dict) else (lambda k: getattr(inputs, k))
        pts, fts = list(get("point")), list(get("feat"))
        if len(pts) == 0 or len(pts) != len(fts) or any(p.dim() != 2 or p.shape[1] != 3 or f.shape != p.shape for p, f in zip(pts, fts)):
            raise ValueError("SparseConvUnet: lists of point [n, 3] and feat [n, 3] expected")
        splits = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in pts])]).astype(np.int64)
        points = torch.cat([p.to(dev, non_blocking=True).float() for p in pts], 0).contiguous()
        feat = torch.cat([f.to(dev, non_blocking=True).float() for f in fts], 0).contiguous()
        pyr = sc_ops.scn_build(points, feat, splits, levels=LEVELS, grid_size=int(self.cfg.grid_size), feat_pitch=32)
        pyr.read_counts()                       # the forward's one device -> host read
        self.last_pyramid = pyr
        planes = self.planes

        def buf(rows, c):
            # (a pitch that is no multiple of 32 is padded with ZERO columns: the padded weight rows are zero, the data must be finite)
            cp = sc_ops.pad32(c)
            t = torch.empty((rows, cp), dtype=torch.float32, device=dev) if cp == c else \
                torch.zeros((rows, cp), dtype=torch.float32, device=dev)
            return t

        def conv(x, rule, p, out=None, residual=None, a2=None):
            """x [rows, >= p.cp] -> [M, p.n] in a (padded) buffer of its own unless ``out`` is given."""
            m = int(rule.shape[0])
            if out is None:
                out = buf(m, p["n"])[:, :p["n"]]
            if hip:
                return sc_ops.sparse_conv(x, rule, p["packed"], p["n"], cp=p["cp"], bias=p["b"], residual=residual, a2=a2,
                                          k2=p["k2"], act=p["act"], out=out)
            return _torch_conv(x, rule, p, out, residual, a2)

        def bnrelu(x, st, out=None):
            if out is None:
                out = buf(int(x.shape[0]), int(x.shape[1]))[:, :x.shape[1]]
            if hip:
                return sc_ops.scn_bn_relu(x, st[0], st[1], out=out)
            out.copy_(torch.relu(x * st[0] + st[1]))
            return out

        def wide(x):
            """The padded buffer behind a column slice that starts at column 0 (what a convolution reads as its input rows)."""
            return x if x.shape[1] % 32 == 0 else x.as_strided((x.shape[0], sc_ops.pad32(x.shape[1])), x.stride(), x.storage_offset())

        def res_block(x, e, rule, out=None):
            xa = bnrelu(x, e["bn1"])
            h = conv(wide(xa), rule, e["c1"])
            if e["identity"]:
                return conv(wide(h), rule, e["c2"], out=out, residual=x)
            return conv(wide(h), rule, e["c2"], out=out, a2=wide(x))

        def run(l, x, e):
            """Residual: x raw -> raw.  Plain: x activated for the level's first block -> activated for the caller's consumer."""
            rule = pyr.nbr27(l)
            deepest = "sub" not in e
            a = planes[l]
            join = None if deepest else buf(pyr.rows(l), 2 * a)
            for i, blk in enumerate(e["pre"]):
                last = i + 1 == len(e["pre"])
                if self.residual:
                    x = res_block(x, blk, rule, out=join[:, :a] if (last and not deepest) else None)
                else:
                    x = conv(wide(x), rule, blk["c"])
            if deepest:
                return x
            if self.residual:
                xd = bnrelu(x, e["bn_d"])
            else:
                xd = bnrelu(x, e["bn_d"])
                bnrelu(x, e["bn_jl"], out=join[:, :a])
            y = conv(wide(xd), pyr.child8(l + 1), e["down"])
            y = run(l + 1, y, e["sub"])
            if self.residual:
                y = bnrelu(y, e["bn_u"])
            conv(wide(y), pyr.up8(l), e["up"], out=join[:, a:2 * a])
            x = join
            for blk in e["post"]:
                x = res_block(x, blk, rule) if self.residual else conv(wide(x), rule, blk["c"])
            return x

        x = conv(pyr.feat0, pyr.nbr27(0), P["stem"])
        x = run(0, x, P["tree"])
        if self.residual:
            x = bnrelu(x, P["bn_out"])
        # Linear + OutputLayer: the rows are gathered through index_map inside the GEMM's loader
        return conv(wide(x), pyr.index_map.view(-1, 1), P["head"])

    # ---- data path (sparseconvnet.py:95-191) ------------------------------------------------------------------------------------
    def preprocess(self, data, attr):
        """sparseconvnet.py:95-152: points scaled by 1 / voxel_size, placed in the grid by the model's generator (two draws of
        three), points outside the grid dropped, positions moved to voxel centres.  The training augmentation is out of scope."""
        if attr['split'] in ('training', 'train'):
            raise NotImplementedError("SparseConvUnet (MI355X build): the training augmentation is out of scope")
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
        if 'feat' not in data or data['feat'] is None:
            raise Exception("SparseConvnet doesn't work without feature values.")
        feat = np.array(data['feat'], dtype=np.float32)
        points *= 1. / self.cfg.voxel_size
        lo, hi = points.min(0), points.max(0)
        grid_size = self.cfg.grid_size
        offset = -lo + np.clip(grid_size - hi + lo - 0.001, 0, None) * rng.random(3) + \
            np.clip(grid_size - hi + lo + 0.001, None, 0) * rng.random(3)
        points += offset
        keep = (points.min(1) >= 0) * (points.max(1) < 4096)
        points, feat, labels = points[keep], feat[keep], labels[keep]
        points = (points.astype(np.int32) + 0.5).astype(np.float32)
        return dict(point=points, feat=feat, label=labels)

    def transform(self, data, attr):
        data['point'] = torch.from_numpy(data['point'])
        data['feat'] = torch.from_numpy(data['feat'])
        data['label'] = torch.from_numpy(data['label'])
        return data

    def update_probs(self, inputs, results, test_probs, test_labels):
        result = results.reshape(-1, self.cfg.num_classes)
        probs = torch.nn.functional.softmax(result, dim=-1).cpu().data.numpy()
        labels = np.argmax(probs, 1)
        sampler = getattr(self, "trans_point_sampler", None)
        if sampler is not None:
            sampler(patchwise=False)
        return probs, labels

    def inference_begin(self, data):
        data = self.preprocess(data, {'split': 'test'})
        data['batch_lengths'] = [data['point'].shape[0]]
        self.inference_input = self.transform(data, {})

    def inference_preprocess(self):
        return self.inference_input

    def make_batch(self, transformed):
        from ..dataloaders import ConcatBatcher
        return ConcatBatcher(self.device, model="SparseConvUnet").collate_fn(
            [{'data': {k: transformed[k] for k in ('point', 'feat', 'label')}}])['data']

    def inference_end(self, inputs, results):
        results = torch.reshape(results, (-1, self.cfg.num_classes))
        probs = torch.softmax(results, dim=-1).cpu().data.numpy()
        probs = np.reshape(probs, [-1, self.cfg.num_classes])
        return {'predict_labels': np.argmax(probs, 1), 'predict_scores': probs}


# ---- the torch formulation (ML3D_SCN_OPS=torch) --------------------------------------------------------------------------------
def _torch_conv(x, rule, p, out, residual, a2):
    """The rulebook convolution with index_select / masked matmul on the folded float32 weights ``p['w']``."""
    cp, n, taps = p["cp"], p["n"], p["taps"]
    w = p["w"]
    m = int(rule.shape[0])
    acc = torch.zeros((m, n), dtype=torch.float32, device=x.device)
    r = rule.long()
    for t in range(taps):
        # (no read-back: absent neighbours gather row 0 and are multiplied away by the mask)
        ok = (r[:, t] >= 0)
        g = x[:, :cp].index_select(0, r[:, t].clamp(min=0)) * ok[:, None].to(torch.float32)
        acc += g @ w[t * cp:(t + 1) * cp]
    if a2 is not None:
        acc += a2[:, :p["k2"]] @ w[taps * cp:]
    if p["b"] is not None:
        acc += p["b"]
    if residual is not None:
        acc += residual
    out.copy_(torch.relu(acc) if p["act"] == 2 else acc)
    return out
