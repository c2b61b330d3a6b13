"""Test helper for the PointTransformer family: the numpy restatement of the furthest-point-sampling contract of
include/ml3d_hip.h, a seeded synthetic indoor cloud, pseudo-trained weights generated from the state-dict layout alone (so the
golden generator and the GPU tests build the SAME weights without shipping them) and direct formulas of the fused ops."""
import numpy as np

PLANES = (32, 64, 128, 256, 512)
INF = np.float32(np.inf)


# ---- furthest point sampling: the canonical order ---------------------------------------------------------------------------
def fps_item(points, m, return_ties=False):
    """points [n, 3] float32, m <= n picks -> item-local int32 [m].  First pick = point 0; after each pick every running
    minimum takes min(mind, d2) with d2 = (dx*dx + dy*dy) + dz*dz in separately rounded float32 operations; the next pick is
    the largest minimum, ties to the lowest index (np.argmax returns the first maximum).  ``return_ties``: also the list of
    pick numbers at which the two best candidates were exactly equal."""
    p = np.ascontiguousarray(points, np.float32)
    n = p.shape[0]
    assert 0 <= m <= n
    out = np.zeros(m, np.int32)
    ties = []
    if m == 0:
        return (out, ties) if return_ties else out
    mind = np.full(n, INF, np.float32)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    cur = 0
    for s in range(1, m):
        dx, dy, dz = x - x[cur], y - y[cur], z - z[cur]          # float32 arrays: every numpy operation rounds once
        d2 = (dx * dx + dy * dy) + dz * dz
        np.minimum(mind, d2, out=mind)
        cur = int(np.argmax(mind))
        if return_ties and n > 1:
            best = mind[cur]
            if best > 0 and int(np.count_nonzero(mind == best)) > 1:
                ties.append(s)
        out[s] = cur
    return (out, ties) if return_ties else out


def fps(points, row_splits, new_row_splits):
    """The batched op: GLOBAL int32 rows."""
    rs, nrs = np.asarray(row_splits, np.int64), np.asarray(new_row_splits, np.int64)
    out = np.zeros(int(nrs[-1]), np.int32)
    for b in range(len(rs) - 1):
        out[nrs[b]:nrs[b + 1]] = fps_item(points[rs[b]:rs[b + 1]], int(nrs[b + 1] - nrs[b])) + np.int32(rs[b])
    return out


def level_row_splits(row_splits, levels=5, stride=4):
    rs = [np.asarray(row_splits, np.int64)]
    lens = np.diff(rs[0])
    for _ in range(levels - 1):
        lens = lens // stride
        rs.append(np.concatenate(([0], np.cumsum(lens))).astype(np.int64))
    return rs


def knn_checksum(idx):
    """The formula of tests/test_gpu_configs.py:78 on an [n, k] index matrix."""
    nb = np.asarray(idx).astype(np.int64)
    return int((nb * (np.arange(nb.shape[1]) + 1)).sum())


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def room(seed, n):
    """The six planes of a 6 x 5 x 3 m room, area-weighted, with 5 mm Gaussian jitter; float32 [n, 3]."""
    rng = np.random.default_rng([int(seed), 0x524f4f4d])
    size = np.array([6.0, 5.0, 3.0])
    areas = np.array([size[1] * size[2], size[1] * size[2], size[0] * size[2], size[0] * size[2], size[0] * size[1],
                      size[0] * size[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = rng.random((n, 3)) * size
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = side * size[axis]
    p += rng.normal(0.0, 0.005, (n, 3))
    return p.astype(np.float32)


def colours(seed, n):
    """feat [n, 3] in [0, 1) (what ``transform`` hands the model after ``/ 255``)."""
    return np.random.default_rng([int(seed), 0x434f4c]).random((n, 3), dtype=np.float32)


def make_batch_arrays(seeds, sizes):
    """-> (points [N, 3] centred per item on its bounding-box middle like ``transform``, feat [N, 3], row_splits)."""
    pts, feat, rs = [], [], [0]
    for s, n in zip(seeds, sizes):
        p = room(s, n)
        p = p - ((p.min(0) + p.max(0)) / np.float32(2.0)).astype(np.float32)
        pts.append(p.astype(np.float32))
        feat.append(colours(s, n))
        rs.append(rs[-1] + n)
    return np.concatenate(pts), np.concatenate(feat), np.asarray(rs, np.int64)


# ---- the state-dict layout, restated from the architecture (point_transformer.py:58-87, 377-413, 470-494, 539-566, 603-627) ----
def state_shapes(model_cfg):
    """Ordered [(key, shape)] of the reference module's ``state_dict()`` for ``blocks`` / ``in_channels`` / ``num_classes``."""
    out = []

    def lin(prefix, i, o, bias=True):
        out.append((prefix + ".weight", (o, i)))
        if bias:
            out.append((prefix + ".bias", (o,)))

    def bn(prefix, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out.append((prefix + "." + k, (c,)))
        out.append((prefix + ".num_batches_tracked", ()))

    def bottleneck(prefix, c):
        s = c // 8
        lin(prefix + ".linear1", c, c, False)
        bn(prefix + ".bn1", c)
        t = prefix + ".transformer2"
        lin(t + ".linear_q", c, c)
        lin(t + ".linear_k", c, c)
        lin(t + ".linear_v", c, c)
        lin(t + ".linear_p.0", 3, 3)
        bn(t + ".linear_p.1", 3)
        lin(t + ".linear_p.3", 3, c)
        bn(t + ".linear_w.0", c)
        lin(t + ".linear_w.2", c, s)
        bn(t + ".linear_w.3", s)
        lin(t + ".linear_w.5", s, s)
        bn(prefix + ".bn2", c)
        lin(prefix + ".linear3", c, c, False)
        bn(prefix + ".bn3", c)

    blocks = list(model_cfg.get("blocks", [2, 2, 2, 2, 2]))
    cin = int(model_cfg.get("in_channels", 6))
    for i in range(5):
        lin("encoders.%d.0.linear" % i, cin if i == 0 else 3 + PLANES[i - 1], PLANES[i], False)
        bn("encoders.%d.0.bn" % i, PLANES[i])
        for j in range(1, blocks[i]):
            bottleneck("encoders.%d.%d" % (i, j), PLANES[i])
    for d, i in enumerate(range(4, -1, -1)):
        c = PLANES[i]
        if i == 4:
            lin("decoders.%d.0.linear1.0" % d, 2 * c, c)
            bn("decoders.%d.0.linear1.1" % d, c)
            lin("decoders.%d.0.linear2.0" % d, c, c)
        else:
            lin("decoders.%d.0.linear1.0" % d, c, c)
            bn("decoders.%d.0.linear1.1" % d, c)
            lin("decoders.%d.0.linear2.0" % d, PLANES[i + 1], c)
            bn("decoders.%d.0.linear2.1" % d, c)
        bottleneck("decoders.%d.1" % d, c)
    lin("cls.0", PLANES[0], PLANES[0])
    bn("cls.1", PLANES[0])
    lin("cls.3", PLANES[0], int(model_cfg.get("num_classes", 13)))
    return out


def make_state_dict(model_cfg, seed, shapes=None):
    """Pseudo-trained weights: torch's default Linear init (uniform in +-1/sqrt(fan_in)) with every Linear weight x 1.6,
    BatchNorm gamma in +-[0.6, 1.5] (a fifth negative), beta and running mean ~ N(0, 0.2^2), running variance in [0.5, 1.5].
    Every entry draws from its own generator seeded by (seed, position), so the values depend on the layout only."""
    import torch
    shapes = state_shapes(model_cfg) if shapes is None else list(shapes)
    sd, fan_in = {}, {}
    for i, (key, shape) in enumerate(shapes):
        rng = np.random.default_rng([int(seed), i])
        shape = tuple(int(v) for v in shape)
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[key] = torch.zeros((), dtype=torch.int64)
            continue
        if len(shape) == 2:
            fan_in[key[:-len(".weight")]] = shape[1]
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shape[1]) * 1.6
        elif leaf == "bias" and key[:-len(".bias")] in fan_in:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in[key[:-len(".bias")]])
        elif leaf == "weight":
            v = rng.uniform(0.6, 1.5, shape) * np.where(rng.random(shape) < 0.2, -1.0, 1.0)
        elif leaf == "running_var":
            v = rng.uniform(0.5, 1.5, shape)
        else:                                   # BatchNorm beta, running mean
            v = rng.normal(0.0, 0.2, shape)
        sd[key] = torch.from_numpy(np.asarray(v, np.float32))
    return sd


# ---- direct torch-CPU formulas of the fused ops (unfolded parameters are the caller's; these take the folded layout) ----------
def attention_formula(qkv, points, idx, a, ep=None, rows=None):
    """``rows`` = range(lo, hi): only those query rows (a large case is evaluated in chunks of rows)."""
    import torch
    lo, hi = (0, idx.shape[0]) if rows is None else (rows.start, rows.stop)
    idx = idx[lo:hi]
    n, ns = idx.shape
    c = qkv.shape[1] // 3
    s = c // 8
    flat = idx.reshape(-1).long()
    q, k, v = qkv[lo:hi, :c], qkv[flat][:, c:2 * c].view(n, ns, c), qkv[flat][:, 2 * c:].view(n, ns, c)
    d = points[flat].view(n, ns, 3) - points[lo:hi, None, :]
    h = torch.relu(d @ a["p_w1"].t() + a["p_b1"])
    r = h @ a["p_w2t"] + a["p_b2"]
    u = torch.relu((k - q[:, None, :] + r) * a["w_scale0"] + a["w_shift0"])
    g = torch.relu(u @ a["w_w1"][:s].t() + a["w_b1"][:s])
    w = torch.softmax(g @ a["w_w2"].t() + a["w_b2"], dim=1)
    out = torch.zeros(n, c, dtype=qkv.dtype)
    vr = v + r
    for ch in range(c):
        out[:, ch] = (vr[:, :, ch] * w[:, :, ch % s]).sum(1)
    return out if ep is None else torch.relu(out * ep[0] + ep[1])


def transition_down_formula(feat, points, sample_idx, idx, w_f_t, w_x, scale, shift, rows=None):
    """``rows`` = range(lo, hi): only those sampled rows."""
    import torch
    lo, hi = (0, idx.shape[0]) if rows is None else (rows.start, rows.stop)
    idx, sample_idx = idx[lo:hi], sample_idx[lo:hi]
    m, ns = idx.shape
    flat = idx.reshape(-1).long()
    d = points[flat].view(m, ns, 3) - points[sample_idx.long()][:, None, :]
    x = torch.cat((d, feat[flat].view(m, ns, -1)), 2) @ torch.cat((w_x, w_f_t), 0)
    return torch.relu(x * scale + shift).max(1)[0]


def interpolate_formula(a, b, idx, d2):
    """``a`` = None: the interpolation alone."""
    import torch
    rec = 1.0 / (d2 + 1e-8)
    w = rec / rec.sum(1, keepdim=True)
    out = torch.zeros(idx.shape[0], b.shape[1], dtype=b.dtype) if a is None else a.clone()
    for t in range(idx.shape[1]):
        out = out + b[idx[:, t].long()] * w[:, t:t + 1]
    return out


def random_attention_params(c, seed, hidden_rows):
    import torch
    rng = np.random.default_rng(seed)
    s = c // 8

    def t(*shape, scale=1.0):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))
    a = dict(p_w1=t(3, 3), p_b1=t(3, scale=0.2), p_w2t=t(3, c, scale=0.6), p_b2=t(c, scale=0.2),
             w_scale0=torch.from_numpy((rng.uniform(0.6, 1.5, c) * np.where(rng.random(c) < 0.2, -1, 1)).astype(np.float32)),
             w_shift0=t(c, scale=0.2), w_w2=t(s, s, scale=1.0 / np.sqrt(s)), w_b2=t(s, scale=0.2))
    w1 = torch.zeros(hidden_rows, c)
    b1 = torch.zeros(hidden_rows)
    w1[:s] = t(s, c, scale=1.6 / np.sqrt(c))
    b1[:s] = t(s, scale=0.2)
    a["w_w1"], a["w_b1"] = w1, b1
    return a
