"""Numpy / torch-CPU restatement of the SparseConvUnet contract of include/ml3d_hip.h ("SparseConvUnet inference"), written
independently of the kernels: key order, rulebooks by DICTIONARY lookup, stand-ins for the four entry points the reference
takes from the ``open3d`` wheel (``SparseConv``, ``SparseConvTranspose``, ``voxelize``, ``reduce_subarrays_sum``) that work on
arbitrary positions, the ``state_dict`` layout, seeded pseudo-trained weights and seeded synthetic rooms.  The contract is
UNPINNED against the wheel (it is not available to this project); tools/gen_golden_sparseconvunet.py runs the reference's
own module on top of these stand-ins."""
import numpy as np
import torch
import torch.nn as nn

import pt_ref

F32 = np.float32
WEIGHT_GAIN = 2.0
KERNEL_FILL = 0.2              # share of a kernel's taps that meet an occupied voxel in a room (surfaces): the effective fan-in
PLANES = 7                       # the U-Net's levels: m, 2m, ... 7m channels


# ---- keys and rulebooks --------------------------------------------------------------------------------------------------------
def int_coords(pos):
    """Voxel centres (int + 0.5, or any position inside the voxel) -> integer coordinates."""
    return np.floor(np.asarray(pos, np.float64)).astype(np.int64)


def level_coords(coords):
    """[M, 4] (item, x, y, z) -> the sorted distinct rows (ascending item, x, y, z)."""
    return np.unique(np.asarray(coords, np.int64).reshape(-1, 4), axis=0)


def table(coords):
    return {tuple(int(v) for v in c): i for i, c in enumerate(coords)}


def nbr27(coords, grid_size=4096):
    t = table(coords)
    out = np.full((len(coords), 27), -1, np.int32)
    for i, (b, x, y, z) in enumerate(coords.tolist()):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    out[i, (dz + 1) * 9 + (dy + 1) * 3 + dx + 1] = t.get((b, x + dx, y + dy, z + dz), -1)
    return out


def parity_tap(coords):
    return ((coords[:, 3] & 1) * 4 + (coords[:, 2] & 1) * 2 + (coords[:, 1] & 1)).astype(np.int32)


def coarsen(coords):
    """Level l -> (level l + 1 coordinates, parent [M_l], tap [M_l], child8 [M_{l+1}, 8], up8 [M_l, 8])."""
    half = coords.copy()
    half[:, 1:] >>= 1
    up = level_coords(half)
    t = table(up)
    parent = np.asarray([t[tuple(c)] for c in half.tolist()], np.int32).reshape(-1)
    tap = parity_tap(coords)
    child8 = np.full((len(up), 8), -1, np.int32)
    child8[parent, tap] = np.arange(len(coords), dtype=np.int32)
    up8 = np.full((len(coords), 8), -1, np.int32)
    up8[np.arange(len(coords)), tap] = parent
    return up, parent, tap, child8, up8


def build(points, feat, row_splits, levels=PLANES, grid_size=4096):
    """The whole pyramid of ``ml3d_scn_build``: points [N, 3] float32 (all items), feat [N, C], row_splits [B + 1] ->
    dict(counts, coords[l], nbr27[l], child8[l] (l >= 1), parent[l], ptap[l], up8[l] (l < levels - 1), index_map, feat0)."""
    points = np.asarray(points, F32)
    feat = np.asarray(feat, F32)
    n = points.shape[0]
    c = int_coords(points)
    item = np.zeros(n, np.int64)
    for b in range(len(row_splits) - 1):
        item[row_splits[b]:row_splits[b + 1]] = b
    ok = ((c >= 0) & (c < grid_size)).all(1)
    full = np.concatenate([item[:, None], c], 1)
    lv = level_coords(full[ok])
    t = table(lv)
    index_map = np.asarray([t[tuple(r)] if o else -1 for r, o in zip(full.tolist(), ok.tolist())], np.int32).reshape(-1)
    feat0 = np.zeros((len(lv), feat.shape[1]), F32)
    cnt = np.zeros(len(lv), np.int64)
    for i in range(n):                                   # ascending point order, float32 adds
        r = index_map[i]
        if r >= 0:
            feat0[r] = feat0[r] + feat[i]
            cnt[r] += 1
    feat0 = feat0 / cnt.astype(F32)[:, None]
    out = dict(coords=[], nbr27=[], child8=[None], parent=[], ptap=[], up8=[], index_map=index_map, feat0=feat0)
    for l in range(levels):
        out["coords"].append(lv.astype(np.int32))
        out["nbr27"].append(nbr27(lv, grid_size))
        if l + 1 < levels:
            lv, parent, tap, child8, up8 = coarsen(lv)
            out["parent"].append(parent)
            out["ptap"].append(tap)
            out["up8"].append(up8)
            out["child8"].append(child8)
    out["counts"] = np.asarray([len(c) for c in out["coords"]], np.int32)
    return out


def brute_force_nbr27(coords):
    """O(M^2): every pair of rows compared."""
    c = np.asarray(coords, np.int64)
    out = np.full((len(c), 27), -1, np.int32)
    d = c[None, :, :] - c[:, None, :]                     # d[i, j] = c[j] - c[i]
    near = (d[:, :, 0] == 0) & (np.abs(d[:, :, 1:]).max(2) <= 1)
    for i, j in zip(*np.nonzero(near)):
        dx, dy, dz = d[i, j, 1:]
        out[i, (dz + 1) * 9 + (dy + 1) * 3 + dx + 1] = j
    return out


def brute_force_children(fine, coarse):
    f, c = np.asarray(fine, np.int64), np.asarray(coarse, np.int64)
    child8 = np.full((len(c), 8), -1, np.int32)
    parent = np.full(len(f), -1, np.int32)
    for i in range(len(f)):
        for j in range(len(c)):
            if f[i, 0] == c[j, 0] and (f[i, 1:] >> 1 == c[j, 1:]).all():
                parent[i] = j
                child8[j, (f[i, 3] & 1) * 4 + (f[i, 2] & 1) * 2 + (f[i, 1] & 1)] = i
    return parent, child8


# ---- direct formulas (float64) ----------------------------------------------------------------------------------------------------
def conv_direct(x, rule, w, x2=None, w2=None, bias=None, residual=None, relu=False):
    """out[r] = sum_t x[rule[r, t]] @ w[t] (+ x2 @ w2 + bias + residual), float64.  w [T, Cin, Cout]."""
    x = np.asarray(x, np.float64)
    out = np.zeros((rule.shape[0], w.shape[2]), np.float64)
    for t in range(rule.shape[1]):
        m = rule[:, t] >= 0
        out[m] += x[rule[m, t]] @ np.asarray(w[t], np.float64)
    if x2 is not None:
        out += np.asarray(x2, np.float64) @ np.asarray(w2, np.float64)
    if bias is not None:
        out += np.asarray(bias, np.float64)
    if residual is not None:
        out += np.asarray(residual, np.float64)
    return np.maximum(out, 0) if relu else out


# ---- stand-ins for the wheel's entry points (per cloud, arbitrary positions) ----------------------------------------------------
_RULES = {}


def _rule(in_pos, out_pos, kind):
    ip, op = int_coords(in_pos.numpy()), int_coords(out_pos.numpy())
    key = (kind, ip.tobytes(), op.tobytes())
    if key in _RULES:
        return _RULES[key]
    if len(_RULES) > 64:
        _RULES.clear()
    t = {tuple(c): i for i, c in enumerate(ip.tolist())}
    if kind == "sub":             # 3 x 3 x 3, offset 0
        rule = np.full((len(op), 27), -1, np.int64)
        for i, (x, y, z) in enumerate(op.tolist()):
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        rule[i, (dz + 1) * 9 + (dy + 1) * 3 + dx + 1] = t.get((x + dx, y + dy, z + dz), -1)
    elif kind == "down":          # 2 x 2 x 2, offset -0.5: the output sits on the even corner of its 8 children
        rule = np.full((len(op), 8), -1, np.int64)
        for i, (x, y, z) in enumerate(op.tolist()):
            for pz in (0, 1):
                for py in (0, 1):
                    for px in (0, 1):
                        rule[i, pz * 4 + py * 2 + px] = t.get((x + px, y + py, z + pz), -1)
    else:                         # transposed 2 x 2 x 2: the input sits on the even corner of the output's block
        rule = np.full((len(op), 8), -1, np.int64)
        for i, (x, y, z) in enumerate(op.tolist()):
            rule[i, (z & 1) * 4 + (y & 1) * 2 + (x & 1)] = t.get((x - (x & 1), y - (y & 1), z - (z & 1)), -1)
    _RULES[key] = rule
    return rule


class _SparseBase(nn.Module):
    KIND3, KIND2 = "sub", "down"

    def __init__(self, in_channels, filters, kernel_size, use_bias=False, offset=None, normalize=False, **kwargs):
        super().__init__()
        assert not use_bias and not normalize and list(kernel_size) in ([3, 3, 3], [2, 2, 2])
        self.kernel_size = list(kernel_size)
        self.kernel = nn.Parameter(torch.zeros(*kernel_size, in_channels, filters))
        self.register_buffer("offset", torch.zeros(3) if offset is None else offset.clone().float())

    def forward(self, feat, in_pos, out_pos, voxel_size=1.0):
        assert float(voxel_size) == 1.0
        rule = _rule(in_pos, out_pos, self.KIND3 if self.kernel_size[0] == 3 else self.KIND2)
        w = self.kernel.reshape(-1, self.kernel.shape[3], self.kernel.shape[4])        # [kz, ky, kx] -> t, x fastest
        out = torch.zeros((rule.shape[0], w.shape[2]), dtype=feat.dtype)
        for t in range(rule.shape[1]):
            m = torch.from_numpy(rule[:, t] >= 0)
            if bool(m.any()):
                out[m] += feat[torch.from_numpy(rule[:, t])[m]] @ w[t]
        return out


class SparseConv(_SparseBase):
    pass


class SparseConvTranspose(_SparseBase):
    KIND2 = "up"


class _Voxels:
    pass


def voxelize(points, row_splits, voxel_size, points_range_min, points_range_max):
    """Voxels in ascending (x, y, z) order, the points of a voxel in ascending index order."""
    c = int_coords(points.numpy())
    uniq, inv = np.unique(c, axis=0, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind="stable")
    v = _Voxels()
    v.voxel_point_indices = torch.from_numpy(order.astype(np.int64))
    v.voxel_point_row_splits = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(inv.reshape(-1), minlength=len(uniq)))])
                                                .astype(np.int64))
    return v


def reduce_subarrays_sum(values, row_splits):
    v, rs = values.numpy(), row_splits.numpy()
    out = np.zeros(len(rs) - 1, v.dtype)
    for i in range(len(out)):                            # ascending order, float32 adds
        acc = v.dtype.type(0)
        for x in v[rs[i]:rs[i + 1]]:
            acc = acc + x
        out[i] = acc
    return torch.from_numpy(out)


# ---- the state-dict layout, restated from the architecture ----------------------------------------------------------------------
def unet_layout(planes, reps, residual):
    """The flat module list of the reference's ``UNet.get_UNet``: [(kind, a, b)]."""
    out = []

    def block(a, b):
        out.extend([("res", a, b)] if residual else [("bn", a, a), ("relu", 0, 0), ("sub", a, b)])

    def rec(p):
        for _ in range(reps):
            block(p[0], p[0])
        if len(p) > 1:
            out.extend([("concat", 0, 0), ("bn", p[0], p[0]), ("relu", 0, 0), ("down", p[0], p[1])])
            rec(p[1:])
            out.extend([("bn", p[1], p[1]), ("relu", 0, 0), ("up", p[1], p[0]), ("join", 0, 0)])
            for i in range(reps):
                block(p[0] * (2 if i == 0 else 1), p[0])

    rec(list(planes))
    return out


def state_shapes(cfg):
    m = int(cfg.get("multiplier", 16))
    reps = int(cfg.get("conv_block_reps", 1))
    residual = bool(cfg.get("residual_blocks", False))
    out = []

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out.append((p + ".bn." + k, (c,)))
        out.append((p + ".bn.num_batches_tracked", ()))

    def conv(p, k, a, b):
        out.append((p + ".net.kernel", (k, k, k, a, b)))
        out.append((p + ".net.offset", (3,)))

    conv("sub_sparse_conv", 3, int(cfg.get("in_channels", 3)), m)
    for i, (kind, a, b) in enumerate(unet_layout([m * (j + 1) for j in range(PLANES)], reps, residual)):
        p = "unet.net.%d" % i
        if kind == "bn":
            bn(p, a)
        elif kind == "sub":
            conv(p, 3, a, b)
        elif kind in ("down", "up"):
            conv(p, 2, a, b)
        elif kind == "res":
            if a != b:
                out.append((p + ".lin.linear.weight", (b, a)))
            bn(p + ".batch_norm1", a)
            conv(p + ".sub_sparse_conv1", 3, a, b)
            bn(p + ".batch_norm2", b)
            conv(p + ".sub_sparse_conv2", 3, b, b)
    bn("batch_norm", m)
    out.append(("linear.linear.weight", (int(cfg.get("num_classes", 20)), m)))
    out.append(("linear.linear.bias", (int(cfg.get("num_classes", 20)),)))
    return out


def make_state_dict(cfg, seed, shapes=None, gain=WEIGHT_GAIN):
    """Pseudo-trained weights (the manner of ``pvcnn_ref.make_state_dict``): kernels / Linear weights uniform in
    +-WEIGHT_GAIN / sqrt(fan_in), BatchNorm gamma in +-[0.6, 1.5], beta / running mean ~ N(0, 0.2^2), running variance in
    [0.5, 1.5]; the conv offsets are the reference's (0 for 3 x 3 x 3, -0.5 for 2 x 2 x 2).  Every entry draws from its own
    generator seeded by (seed, position).  ``gain`` scales the kernels and Linear weights (a golden stores its own: the deep
    residual configuration grows faster per layer than the plain one)."""
    shapes = state_shapes(cfg) if shapes is None else list(shapes)
    sd = {}
    for i, (key, shape) in enumerate(shapes):
        rng = np.random.default_rng([int(seed), i])
        shape = tuple(int(v) for v in shape)
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[key] = torch.zeros((), dtype=torch.int64)
            continue
        if leaf == "offset":
            prev = sd[key[:-len("offset")] + "kernel"]
            sd[key] = torch.full((3,), 0.0 if prev.shape[0] == 3 else -0.5)
            continue
        if leaf == "kernel":
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(KERNEL_FILL * shape[0] * shape[1] * shape[2] * shape[3]) * gain
        elif len(shape) == 2:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shape[1]) * gain
        elif key.startswith("linear.") and leaf == "bias":
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shapes[i - 1][1][1])
        elif leaf == "weight":
            v = rng.uniform(0.6, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1.0, 1.0)
        elif leaf == "running_var":
            v = rng.uniform(0.5, 1.5, shape)
        else:
            v = rng.normal(0.0, 0.2, shape)
        sd[key] = torch.from_numpy(np.asarray(v, F32))
    return sd


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def room(seed, n, voxel_size=0.05, lattice=True, origin=(100, 200, 50)):
    """A synthetic room as ``SparseConvUnet.preprocess`` hands it on: positions = voxel centres (int + 0.5) float32 [n, 3]
    somewhere inside the 4096 grid, colours [n, 3] in [-1, 1] -- on a 2^-6 lattice (every float32 sum of <= 2^17 of them is exact
    in any order) unless ``lattice`` is False."""
    p = pt_ref.room(seed, n).astype(np.float64)
    p = np.floor((p - p.min(0)) / voxel_size).astype(np.int64) + np.asarray(origin, np.int64)
    assert p.min() >= 0 and p.max() < 4096
    col = pt_ref.colours(seed, n).astype(np.float64) * 2.0 - 1.0
    if lattice:
        col = np.round(col * 64.0) / 64.0
    return (p + 0.5).astype(F32), col.astype(F32)


def golden_inputs(clouds, voxel_size):
    """The clouds of a golden: [(seed, n)] -> (list of points [n, 3], list of feat [n, 3]), item i placed 700 voxels further in x."""
    pts, fts = [], []
    for i, (seed, n) in enumerate(clouds):
        p, f = room(int(seed), int(n), voxel_size=float(voxel_size), origin=(100 + 700 * i, 200, 50))
        pts.append(p)
        fts.append(f)
    return pts, fts


def deep_cloud():
    """One item inside [0, 64)^3: its seventh level is a single row."""
    rng = np.random.default_rng(11)
    c = rng.integers(0, 64, (300, 3))
    return (c + 0.5).astype(F32), (np.round(rng.uniform(-1, 1, (300, 3)) * 64.0) / 64.0).astype(F32), np.asarray([0, 300], np.int64)


def edge_batch():
    """The two-item batch of the rulebook tests (see tests/test_gpu_sparseconv.py): -> (points [N, 3], feat [N, 3], row_splits)."""
    rng = np.random.default_rng(7)

    def item(extra):
        c = [(0, 0, 0), (4095, 4095, 4095), (2000, 17, 3001)]                               # corners, an isolated voxel
        c += [(500 + dx, 600 + dy, 700 + dz) for dx in range(3) for dy in range(3) for dz in range(3)]      # a full 3 x 3 x 3 block
        c += [(1000, 1000, 1000), (1001, 1000, 1000), (1001, 1001, 1001), (1002, 1000, 1000)]  # odd / even siblings + a cousin
        c += [(64, 64, 64)] * 57                                                             # >= 50 duplicate points
        blob = rng.integers(0, 14, (extra, 3)) + np.asarray([300, 310, 320])                 # a dense blob: many shared voxels
        c = np.concatenate([np.asarray(c, np.int64), blob])
        return c[rng.permutation(len(c))]

    a, b = item(260), item(110)
    b = np.concatenate([b, a[:40]])                      # the SAME coordinates in both items
    pts = np.concatenate([a, b]).astype(np.float64) + 0.5
    feat = np.round(rng.uniform(-1, 1, (len(pts), 3)) * 64.0) / 64.0
    return pts.astype(F32), feat.astype(F32), np.asarray([0, len(a), len(a) + len(b)], np.int64)
