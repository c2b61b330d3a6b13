"""Test helper for the PVCNN family: numpy restatements of the contracts of include/ml3d_hip.h ("PVCNN inference": voxel
coordinates, scatter-mean, trilinear gather), the state-dict layout restated from the architecture, pseudo-trained weights
generated from that layout alone (so the golden generator and the tests build the SAME weights without shipping them) and
seeded rooms -- on a 2^-6 m lattice for the goldens, real-valued for everything else."""
import math

import numpy as np

import pt_ref

BLOCKS = ((64, 1, 32), (64, 2, 16), (128, 1, 16), (1024, 1, None))
F32, F64 = np.float32, np.float64
# make_state_dict: Linear / convolution weights are uniform in +-WEIGHT_GAIN / sqrt(fan_in), i.e. of variance 4 / (3 fan_in): a ReLU
# halves a centred signal's second moment, so 2.0 roughly keeps it through PVCNN's ten-layer depth (1.6, PointTransformer's value,
# lets it decay to logits of about 1.5; 2.4 grows them to about 50)
WEIGHT_GAIN = 2.0


# ---- contract (a): the voxel coordinates ----------------------------------------------------------------------------------------
def fma32(a, b, c):
    """Correctly rounded float32 a * b + c for float32 arrays.  a * b is exact in float64; the float64 sum may round, so its
    exact error (TwoSum) decides the one case in which rounding twice differs from rounding once: the float64 sum lying
    exactly halfway between two float32 values."""
    a, b, c = (np.asarray(t, F32).astype(F64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    d = s - r.astype(F64)
    other = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
    tie = (d != 0) & (np.abs(s - other.astype(F64)) == np.abs(d)) & (e != 0)
    return np.where(tie & (np.sign(e) == np.sign(d)), other, r).astype(F32)


def voxel_stats(coords):
    """coords [3, n] float32 of ONE item -> float32 [4] = (mean x, y, z, scale): steps 1-4 of the contract."""
    x = np.ascontiguousarray(coords, F32)
    n = x.shape[1]
    mean = np.asarray([F32(math.fsum(float(v) for v in x[c])) for c in range(3)], F32) / F32(n)
    d = x - mean[:, None]
    norm = np.sqrt(fma32(d[2], d[2], fma32(d[1], d[1], d[0] * d[0])))
    scale = norm.max() * F32(2.0) + F32(1e-6)
    return np.asarray([mean[0], mean[1], mean[2], scale], F32)


def voxel_coords(coords, resolutions):
    """coords [B, 3, N] -> (stats [B, 4], {r: (v float32 [B * N, 3], flat index int32 [B * N])})."""
    coords = np.ascontiguousarray(coords, F32)
    B, _, N = coords.shape
    stats = np.stack([voxel_stats(coords[b]) for b in range(B)])
    out = {}
    for r in resolutions:
        v = np.empty((B, N, 3), F32)
        for b in range(B):
            d = coords[b] - stats[b, :3, None]
            t = (d / stats[b, 3] + F32(0.5)) * F32(r)
            v[b] = np.minimum(np.maximum(t, F32(0.0)), F32(r - 1)).T
        c = np.rint(v).astype(np.int32)
        out[int(r)] = (v.reshape(B * N, 3), ((c[..., 0] * r + c[..., 1]) * r + c[..., 2]).reshape(B * N).astype(np.int32))
    return stats, out


def vox_checksum(idx):
    """``pt_ref.knn_checksum`` on the [B, N] matrix of flat voxel indices."""
    return pt_ref.knn_checksum(np.asarray(idx))


# ---- contracts (b) and (d) ------------------------------------------------------------------------------------------------------
def avg_voxelize(feat, idx, batch, r, out_channels=None):
    """feat [B * N, C], idx [B * N] -> [B, r, r, r, out_channels or C]; float32 sums in ascending point order (np.add.at is
    unbuffered and visits the rows in order), divided by the count."""
    feat = np.asarray(feat, F32)
    n, c = feat.shape[0] // batch, feat.shape[1]
    cg = c if out_channels is None else out_channels
    flat = np.asarray(idx, np.int64) + np.repeat(np.arange(batch, dtype=np.int64), n) * r ** 3
    grid = np.zeros((batch * r ** 3, cg), F32)
    np.add.at(grid, (flat[:, None], np.arange(c)[None, :]), feat)
    cnt = np.bincount(flat, minlength=batch * r ** 3).astype(F32)
    return (grid / np.maximum(cnt, F32(1.0))[:, None]).reshape(batch, r, r, r, cg)


def devoxelize(grid, v, addend=None):
    """grid [B, r, r, r, C] channels-last, v [B * N, 3] -> [B * N, C] (+ addend)."""
    grid, v = np.asarray(grid, F32), np.asarray(v, F32)
    B, r, c = grid.shape[0], grid.shape[1], grid.shape[4]
    n = v.shape[0] // B
    lo = np.floor(v)
    f = v - lo
    lo_i = np.clip(lo.astype(np.int64), 0, r - 1)
    hi_i = np.minimum(lo_i + (f > 0), r - 1)
    base = np.repeat(np.arange(B, dtype=np.int64), n) * r ** 3
    g = grid.reshape(B * r ** 3, c)
    out = np.zeros((v.shape[0], c), F32)
    for k in range(8):
        pick = [(k >> (2 - a)) & 1 for a in range(3)]
        cell = [np.where(pick[a], hi_i[:, a], lo_i[:, a]) for a in range(3)]
        w = [f[:, a] if pick[a] else F32(1.0) - f[:, a] for a in range(3)]
        out += g[base + (cell[0] * r + cell[1]) * r + cell[2]] * ((w[0] * w[1]) * w[2])[:, None]
    return out if addend is None else out + np.asarray(addend, F32)


def torch_devoxelize_forward(resolution, is_training, coords, features):
    """Stand-in for ``open3d.ml.torch.ops.trilinear_devoxelize_forward`` (contract (d)) on torch-CPU tensors: coords
    [B, 3, N] in voxel units, features [B, C, R, R, R] -> (outs [B, C, N], None, None)."""
    import torch
    B, C = features.shape[:2]
    r, N = int(resolution), coords.shape[2]
    v = coords.transpose(1, 2)
    lo = torch.floor(v)
    f = v - lo
    lo_i = lo.long().clamp(0, r - 1)
    hi_i = (lo_i + (f > 0).long()).clamp(max=r - 1)
    g = features.reshape(B, C, r ** 3)
    out = torch.zeros((B, C, N), dtype=features.dtype)
    for k in range(8):
        pick = [(k >> (2 - a)) & 1 for a in range(3)]
        cell = [hi_i[..., a] if pick[a] else lo_i[..., a] for a in range(3)]
        w = [f[..., a] if pick[a] else 1 - f[..., a] for a in range(3)]
        flat = ((cell[0] * r + cell[1]) * r + cell[2])[:, None, :].expand(B, C, N)
        out += torch.gather(g, 2, flat) * ((w[0] * w[1]) * w[2])[:, None, :]
    return out, None, None


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def real_room(seed, n):
    """``pt_ref.room`` moved to the origin as ``PVCNN.preprocess`` does: real-valued float32 [n, 3]."""
    p = pt_ref.room(seed, n)
    return (p - p.min(0)).astype(F32)


def lattice_room(seed, n):
    """The same room on a 2^-6 m lattice, minimum corner at 0, extents <= 6 m: with n * 6 * 64 < 2^24 every float32 partial sum
    of a coordinate is exact in any order, so a float32 mean equals the contract's double-sum mean bit for bit."""
    p = np.round(pt_ref.room(seed, n).astype(F64) * 64.0) / 64.0
    p = np.minimum(p - p.min(0), 6.0).astype(F32)
    assert n * float(p.max()) * 64 < 2 ** 24
    return p


def make_inputs(seeds, n, lattice=True):
    """-> (point [B, 3, N], feat [B, 9, N]) float32 as ``PVCNN.preprocess`` lays them out: feat = [xyz | colour | xyz / max]."""
    pts, feats = [], []
    for s in seeds:
        p = lattice_room(s, n) if lattice else real_room(s, n)
        f = np.concatenate([p, pt_ref.colours(s, n), p / p.max(0)], 1).astype(F32)
        pts.append(p.T)
        feats.append(f.T)
    return np.ascontiguousarray(np.stack(pts)), np.ascontiguousarray(np.stack(feats))


# ---- the state-dict layout, restated from the architecture (pvcnn.py:85-134, 352-452, 455-486, 504-557) --------------------------
def widths(model_cfg):
    r = model_cfg.get("width_multiplier", 1)
    vr = model_cfg.get("voxel_resolution_multiplier", 1)
    out = []
    for oc, num, res in BLOCKS:
        out += [(int(r * oc), None if res is None else int(vr * res))] * num
    return out


def state_shapes(model_cfg):
    """Ordered [(key, shape)] of the reference module's ``state_dict()``."""
    out = []
    r = model_cfg.get("width_multiplier", 1)

    def conv(prefix, i, o, k):
        out.append((prefix + ".weight", (o, i) + k))
        out.append((prefix + ".bias", (o,)))

    def bn(prefix, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out.append((prefix + "." + k, (c,)))
        out.append((prefix + ".num_batches_tracked", ()))

    def shared(prefix, i, o):
        conv(prefix + ".layers.0", i, o, (1,))
        bn(prefix + ".layers.1", o)

    cin = int(model_cfg.get("extra_feature_channels", 6)) + 3
    concat = 0
    for j, (oc, res) in enumerate(widths(model_cfg)):
        p = "point_features.%d" % j
        if res is None:
            shared(p, cin, oc)
        else:
            conv(p + ".voxel_layers.0", cin, oc, (3, 3, 3))
            bn(p + ".voxel_layers.1", oc)
            conv(p + ".voxel_layers.3", oc, oc, (3, 3, 3))
            bn(p + ".voxel_layers.4", oc)
            shared(p + ".point_features", cin, oc)
        cin = oc
        concat += oc
    for j, oc in enumerate((256, 128)):
        oc = int(r * oc)
        conv("cloud_features.%d.0" % j, cin, oc, ())
        bn("cloud_features.%d.1" % j, oc)
        cin = oc
    c1, c2 = int(r * 512), int(r * 256)
    shared("classifier.0", concat + cin, c1)
    shared("classifier.2", c1, c2)
    conv("classifier.4", c2, int(model_cfg.get("num_classes", 13)), (1,))
    return out


def make_state_dict(model_cfg, seed, shapes=None):
    """Pseudo-trained weights in the manner of ``pt_ref.make_state_dict``: every Linear / convolution weight uniform in
    +-WEIGHT_GAIN / sqrt(fan_in), its bias in +-1 / sqrt(fan_in), BatchNorm gamma in +-[0.6, 1.5] (a fifth negative), beta and running
    mean ~ N(0, 0.2^2), running variance in [0.5, 1.5] -- non-trivial running statistics.  Every entry draws from its own
    generator seeded by (seed, position), so the values depend on the layout only."""
    import torch
    shapes = state_shapes(model_cfg) if shapes is None else list(shapes)
    sd, fan_in = {}, {}
    for i, (key, shape) in enumerate(shapes):
        rng = np.random.default_rng([int(seed), i])
        shape = tuple(int(v) for v in shape)
        stem, leaf = key.rsplit(".", 1)
        if leaf == "num_batches_tracked":
            sd[key] = torch.zeros((), dtype=torch.int64)
            continue
        if len(shape) >= 2:
            fan_in[stem] = int(np.prod(shape[1:]))
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in[stem]) * WEIGHT_GAIN
        elif leaf == "bias" and stem in fan_in:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in[stem])
        elif leaf == "weight":
            v = rng.uniform(0.6, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1.0, 1.0)
        elif leaf == "running_var":
            v = rng.uniform(0.5, 1.5, shape)
        else:
            v = rng.normal(0.0, 0.2, shape)
        sd[key] = torch.from_numpy(np.asarray(v, F32))
    return sd
