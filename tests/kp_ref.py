"""The KPConv operations as plain formulas -- the reference of tests/kp_cases.py.  Torch, in the dtype of the float inputs: the
bodies evaluate every formula twice, in float64 (THE reference) and in float32 (``e32``, the formula's own rounding at the case's
inputs).  Restated from ``KPConv.forward`` of the reference models (kpconv.py:1005-1159), not copied: one gather per operand,
the shadow neighbour as a mask instead of a padded row.

An index outside [0, Ns) is the shadow neighbour (include/ml3d_hip.h: ``>= Ns = shadow``): zero features, position irrelevant.
Everything works in chunks of query rows: the [rows, H, 15] distances and the [rows, H, cin] gather of a chunk stay far below a
gigabyte of float64 at the largest case of the tables."""
import numpy as np
import torch

K_POINTS = 15
INFLUENCES = {0: "constant", 1: "linear", 2: "gaussian"}
CHUNK_FLOATS = 1 << 24        # float64 elements of the largest intermediate of a chunk: 128 MB


def influence_weight(d2, extent, influence, gaussian_factor=2.0):
    """constant: 1; linear: clamp(1 - sqrt(d2) / extent, 0); gaussian: exp(-d2 / (2 (0.3 extent)^2 + 1e-9))."""
    influence = INFLUENCES.get(influence, influence)
    if influence == "constant":
        return torch.ones_like(d2)
    if influence == "linear":
        return torch.clamp(1 - torch.sqrt(d2) / extent, min=0)
    if influence == "gaussian":
        return torch.exp(-d2 / (gaussian_factor * (0.3 * extent) ** 2 + 1e-9))
    raise ValueError(influence)


def real(inds, ns):
    return (inds >= 0) & (inds < ns)


def _chunks(nq, per_row):
    rows = max(1, int(CHUNK_FLOATS // max(1, per_row)))
    return [slice(lo, min(nq, lo + rows)) for lo in range(0, nq, rows)]


def influences(q, s, inds, kp, extent, influence, offsets=None, **kw):
    """-> w [nq, 15, h]: the influence of neighbour h of query q on kernel point k (``kp[k] + offsets[q, k]`` when the kernel is
    deformed), zero for a shadow neighbour."""
    ok = real(inds, s.shape[0])
    safe = torch.where(ok, inds, torch.zeros_like(inds)).long()
    rel = s[safe] - q[:, None, :]                                            # [nq, h, 3]
    pts = kp[None] if offsets is None else kp[None] + offsets                # [1 | nq, 15, 3]
    d2 = ((rel[:, None, :, :] - pts[:, :, None, :]) ** 2).sum(3)             # [nq, 15, h]
    return influence_weight(d2, extent, influence, **kw) * ok[:, None, :].to(d2.dtype)


def weighted(q, s, inds, x, kp, extent, influence, offsets=None, modulations=None, **kw):
    """-> wf [nq, 15, cin] = sum_h w[q, k, h] x[inds[q, h]] (times ``modulations`` [nq, 15] where given)."""
    nq, h = inds.shape
    cin = x.shape[1]
    out = torch.zeros((nq, K_POINTS, cin), dtype=x.dtype)
    if h == 0:
        return out
    safe = torch.where(real(inds, s.shape[0]), inds, torch.zeros_like(inds)).long()
    for r in _chunks(nq, h * max(cin, 3 * K_POINTS)):
        w = influences(q[r], s, inds[r], kp, extent, influence, None if offsets is None else offsets[r], **kw)
        out[r] = torch.matmul(w, x[safe[r]])                                 # the shadow's row is multiplied by a zero weight
    if modulations is not None:
        out = out * modulations[:, :, None]
    return out


def activation(y, act, slope):
    if act == 1:
        return torch.where(y > 0, y, y * slope)
    if act == 2:
        return torch.clamp(y, min=0)
    return y


def contract(wf, weights, bias=None, act=0, slope=0.1):
    """wf [nq, 15, cin] . W [15 cin, cout] + bias, then the activation: 0 none, 1 leaky with ``slope``, 2 ReLU."""
    y = wf.flatten(1) @ weights
    if bias is not None:
        y = y + bias
    return activation(y, act, slope)


def conv(q, s, inds, x, kp, extent, influence, weights, bias=None, act=0, slope=0.1, **kw):
    return contract(weighted(q, s, inds, x, kp, extent, influence, **kw), weights, bias, act, slope)


def deformable(q, s, inds, x, kp, extent, weights, bias, offset_weights, offset_bias, act=1, slope=0.1):
    """The deformable convolution (linear influence): the inner rigid convolution cin -> 45 (| 60) gives every query the offsets of
    its kernel points in units of the extent (and, in the last 15 columns, modulation logits: 2 sigmoid)."""
    off = conv(q, s, inds, x, kp, extent, "linear", offset_weights, offset_bias)
    offsets = off[:, :3 * K_POINTS].reshape(-1, K_POINTS, 3) * extent
    mod = 2 * torch.sigmoid(off[:, 3 * K_POINTS:]) if off.shape[1] > 3 * K_POINTS else None
    return conv(q, s, inds, x, kp, extent, "linear", weights, bias, act, slope, offsets=offsets, modulations=mod), off


def adjoint(q, s, inds, dwf, kp, extent, influence):
    """dx [ns, cin]: dx[inds[q, h]] += sum_k w[q, k, h] dwf[q, k, :] over the real neighbours (dwf [nq, 15, cin])."""
    nq, h = inds.shape
    ns, cin = s.shape[0], dwf.shape[2]
    dx = torch.zeros((ns, cin), dtype=dwf.dtype)
    if h == 0:
        return dx
    safe = torch.where(real(inds, ns), inds, torch.zeros_like(inds)).long()
    for r in _chunks(nq, h * max(cin, 3 * K_POINTS)):
        w = influences(q[r], s, inds[r], kp, extent, influence)                   # [rows, 15, h], zero on shadows
        dx.index_add_(0, safe[r].reshape(-1), torch.matmul(w.transpose(1, 2), dwf[r]).reshape(-1, cin))
    return dx


# ---- pools, numpy (compared bit for bit) ----------------------------------------------------------------------------------------------
def _padded(x, inds):
    ns = x.shape[0]
    xp = np.concatenate([x, np.zeros_like(x[:1])], 0)
    return xp, np.where((inds >= 0) & (inds < ns), inds, ns).astype(np.int64)


def max_pool(x, inds):
    """The maximum over ALL listed neighbours, a shadow counting as a row of zeros."""
    xp, idx = _padded(x, inds)
    return xp[idx].max(1)


def closest_pool(x, inds):
    """The row of the first listed neighbour (zeros where that is the shadow)."""
    xp, idx = _padded(x, inds)
    return xp[idx[:, 0]]
