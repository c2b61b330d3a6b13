"""CPU restatements of the PointNet++ op contracts of include/ml3d_hip.h ("PointNet++ MSG backbone inference"), operation for
operation, in numpy -- the references of tests/pn2_cases.py and the stand-ins tools/gen_golden_pointnet2.py puts in place of the
reference's ``open3d.ml.torch.ops`` imports.  Furthest point sampling comes from tests/pt_ref.py.  The float formulas at the end
are direct torch restatements of the reference modules (grouping BEFORE the first convolution), evaluated in whatever dtype
their inputs have."""
import numpy as np

import pt_ref


def dist2(centres, points):
    """[m, 3] x [n, 3] -> float32 [m, n]: d = c - p, (dx * dx + dy * dy) + dz * dz, every operation rounded separately."""
    c, p = np.asarray(centres, np.float32), np.asarray(points, np.float32)
    dx = c[:, None, 0] - p[None, :, 0]
    dy = c[:, None, 1] - p[None, :, 1]
    dz = c[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def ball_query_item(points, centres, radius, nsample, strict=True, by_distance=False):
    """One item: int32 [m, nsample].  ``strict`` / ``by_distance`` exist for tests/test_pn2_cases_can_fail.py: the WRONG forms
    ``d2 <= r * r`` and hits in ascending distance."""
    r = np.float32(radius)
    r2 = r * r
    out = np.zeros((len(centres), int(nsample)), np.int32)
    for lo in range(0, len(centres), 256):                       # (in chunks of centres: the [m, n] matrix stays small)
        d2 = dist2(centres[lo:lo + 256], points)
        hit = (d2 < r2) if strict else (d2 <= r2)
        for i in range(len(d2)):
            h = np.flatnonzero(hit[i])
            if by_distance:
                h = h[np.argsort(d2[i, h], kind="stable")]
            if len(h):
                k = min(len(h), int(nsample))
                out[lo + i, :k] = h[:k]
                out[lo + i, k:] = h[0]
    return out


def ball_query(xyz, new_xyz, radius, nsample, **wrong):
    """[B, N, 3], [B, m, 3] -> int32 [B, m, nsample], item-local."""
    return np.stack([ball_query_item(p, c, radius, nsample, **wrong) for p, c in zip(np.asarray(xyz), np.asarray(new_xyz))])


def hit_counts(xyz, new_xyz, radius):
    r = np.float32(radius)
    return np.stack([(dist2(c, p) < r * r).sum(1) for p, c in zip(np.asarray(xyz), np.asarray(new_xyz))])


def three_nn(query, data):
    """[B, n, 3], [B, M >= 3, 3] -> (dist2 float32 [B, n, 3], idx int32 [B, n, 3]): ascending d2, ties to the lowest index."""
    q, d = np.asarray(query, np.float32), np.asarray(data, np.float32)
    assert d.shape[1] >= 3, "fewer than 3 known points"
    out_d, out_i = [], []
    for b in range(len(q)):
        di, ii = [], []
        for lo in range(0, q.shape[1], 512):
            d2 = dist2(q[b, lo:lo + 512], d[b])
            order = np.argsort(d2, axis=1, kind="stable")[:, :3]
            ii.append(order.astype(np.int32))
            di.append(np.take_along_axis(d2, order, 1))
        out_i.append(np.concatenate(ii))
        out_d.append(np.concatenate(di))
    return np.stack(out_d), np.stack(out_i)


def three_interpolate(features, idx, weight):
    """[B, C, M], [B, n, 3], [B, n, 3] -> [B, C, n] in the dtype of ``features``."""
    f, w = np.asarray(features), np.asarray(weight)
    out = np.zeros((f.shape[0], f.shape[1], idx.shape[1]), f.dtype)
    for b in range(f.shape[0]):
        for t in range(3):
            out[b] += f[b][:, np.asarray(idx)[b, :, t]] * w[b, :, t][None, :].astype(f.dtype)
    return out


def furthest_point_sampling(xyz, npoint):
    """[B, N, 3] -> int32 [B, npoint], item-local, the canonical order of tests/pt_ref.py."""
    return np.stack([pt_ref.fps_item(p, int(npoint)) for p in np.asarray(xyz, np.float32)])


def torch_ops():
    """The four ops with the signatures ``pointnet2_utils`` imports from ``open3d.ml.torch.ops``, on CPU torch tensors."""
    import torch

    def fps(xyz, npoint):
        return torch.from_numpy(furthest_point_sampling(xyz.detach().numpy(), npoint))

    def bq(xyz, new_xyz, radius, nsample):
        return torch.from_numpy(ball_query(xyz.detach().numpy(), new_xyz.detach().numpy(), radius, nsample))

    def nn3(query, data):
        d, i = three_nn(query.detach().numpy(), data.detach().numpy())
        return torch.from_numpy(d), torch.from_numpy(i)

    def interp(features, idx, weight):
        return torch.from_numpy(three_interpolate(features.detach().numpy(), idx.numpy(), weight.detach().numpy()))

    return dict(furthest_point_sampling=fps, ball_query=bq, three_nn=nn3, three_interpolate=interp)


# ---- inputs of the module goldens (tools/gen_golden_pointnet2.py writes with them, the tests rebuild them) --------------------------
def make_state_dict(keys, shapes, seed):
    """Pseudo-trained parameters for the reference's layout: conv weights uniform in +-2.45 / sqrt(fan_in) (variance 2 / fan_in:
    the ReLU layers keep the activations' magnitude from the first level to the last), BatchNorm scales in
    +-[0.6, 1.5] (a fifth negative), shifts N(0, 0.2), running means N(0, 0.1), running variances in [0.5, 1.5]."""
    import torch
    rng = np.random.default_rng([int(seed), 0x504E32])
    sd = {}
    for k, shape in zip(keys, shapes):
        shape = tuple(int(v) for v in shape)
        if k.endswith("num_batches_tracked"):
            v = np.asarray(1, np.int64)
        elif k.endswith("running_mean"):
            v = rng.normal(0, 0.1, shape)
        elif k.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("bias"):
            v = rng.normal(0, 0.2, shape)
        elif len(shape) == 4:
            v = rng.uniform(-1, 1, shape) * 2.45 / np.sqrt(shape[1])
        else:
            v = rng.uniform(0.6, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1, 1)
        sd[k] = torch.from_numpy(np.asarray(v, np.int64 if k.endswith("num_batches_tracked") else np.float32))
    return sd


def make_pointcloud(seeds, n, in_channels, scale, offset):
    """[B, n, 3 + in_channels] float32: per item a room of tests/pt_ref.py scaled and moved (a lidar frame's coordinates are
    tens of metres from the origin), features uniform in [0, 1)."""
    out = []
    for s in seeds:
        rng = np.random.default_rng([int(s), 0x434C44])
        p = pt_ref.room(int(s), n) * np.float32(scale) + np.asarray(offset, np.float32)
        out.append(np.concatenate((p, rng.random((n, in_channels), dtype=np.float32)), 1))
    return np.ascontiguousarray(np.stack(out), np.float32)


# ---- float formulas (torch, any dtype) -------------------------------------------------------------------------------------------
def sa_formula(xyz, feat, centres, idx, layers, drop_last=0):
    """One scale of PointnetSAModuleMSG: ``xyz`` [B, n, 3], ``feat`` [B, n, c] or None, ``centres`` [B, m, 3], ``idx`` [B, m, ns],
    ``layers`` = three (W [cin, cout], scale [cout], shift [cout]) -> [B, m, c3]: group, subtract the centre, conv + BN + ReLU
    three times, maximum over the neighbours (over all but the last ``drop_last``: a WRONG form for the can-fail test)."""
    import torch
    b, m, ns = idx.shape
    gather = idx.reshape(b, m * ns).long()
    g = torch.gather(xyz, 1, gather[..., None].expand(-1, -1, 3)).view(b, m, ns, 3) - centres[:, :, None, :]
    if feat is not None:
        g = torch.cat((g, torch.gather(feat, 1, gather[..., None].expand(-1, -1, feat.shape[2])).view(b, m, ns, -1)), 3)
    for w, scale, shift in layers:
        g = torch.relu((g @ w) * scale + shift)
    return g[:, :, :ns - drop_last].max(2)[0]


def fp_interpolate_formula(known, idx, d2):
    """``known`` [B, M, c], ``idx`` / ``d2`` [B, n, 3] -> [B, n, c]: the weights of PointnetFPModule and three_interpolate."""
    import torch
    rec = 1.0 / (torch.sqrt(d2) + 1e-8)
    w = rec / rec.sum(2, keepdim=True)
    out = 0
    for t in range(3):
        out = out + torch.gather(known, 1, idx[:, :, t].long()[..., None].expand(-1, -1, known.shape[2])) * w[:, :, t:t + 1]
    return out
