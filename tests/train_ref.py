"""The training ops of csrc/train.hip (and the four differentiable entry points at the end of csrc/randla.hip) as plain formulas --
the reference of tests/train_cases.py.  Every formula takes the ``dtype`` it is evaluated in: the bodies call each one twice, in
float64 (THE reference) and in float32 (``e32``, the formula's own rounding at the case's inputs).  Forward AND backward are written
out from the formulations the HIP comments cite (SharedMLP / BatchNormBlock: randlanet.py:503-518, kpconv.py:1238-1249; the gathers and
pools: randlanet.py:329-350, kpconv.py:821-858; the attentive pooling: randlanet.py:596-605, 617, 631-637; the deformed KPConv:
kpconv.py:1011-1066, 1105-1137; the regulariser: kpconv.py:2167-2206, 1058-1074; random_sample: randlanet.py:300-327) -- no autograd:
tests/test_train_cases_can_fail.py checks the written-out gradients against torch's autograd once, where that is defined.

The DISCRETE rules are index arithmetic, never ``torch.max``'s backward (whose tie rule is unspecified):
  * the gradient of a maximum goes to the FIRST maximal neighbour in list order (``numpy.argmax``: first occurrence),
  * the fitting term's gradient to the FIRST minimum (``numpy.argmin``: first occurrence),
  * an index outside [0, n) is the shadow: it reads the zero row (the regulariser: a support at 1e6) and takes no gradient,
  * ``clamp``'s gradient mask is inclusive at 0, LeakyReLU's mask is ``y > 0`` on the layer's OUTPUT."""
import numpy as np
import torch

K_POINTS = 15
FAR = 1.0e6


def real(idx, n):
    return (idx >= 0) & (idx < n)


def _safe(idx, n):
    return torch.where(real(idx, n), idx, torch.zeros_like(idx)).long()


# ---- gemm_tn ---------------------------------------------------------------------------------------------------------------------------
def gemm_tn(a, b, dtype):
    """-> (a^T b [k, n], the column sums of a [k])."""
    a, b = a.to(dtype), b.to(dtype)
    return a.t() @ b, a.sum(0)


# ---- BatchNorm on the batch statistics (+ LeakyReLU) -------------------------------------------------------------------------------------
def leaky(v, slope):
    return v if slope is None else torch.where(v > 0, v, v * slope)


def bn_forward(x, gamma, beta, eps, slope, dtype, unbiased=False):
    """x [rows, c] -> (y, pre-activation v, mean, BIASED variance, 1 / sqrt(var + eps))."""
    x = x.to(dtype)
    rows = x.shape[0]
    mean = x.sum(0) / rows
    var = ((x - mean) ** 2).sum(0) / (rows - 1 if unbiased else rows)
    invstd = 1.0 / torch.sqrt(var + eps)
    v = (x - mean) * invstd
    if gamma is not None:
        v = v * gamma.to(dtype)
    if beta is not None:
        v = v + beta.to(dtype)
    return leaky(v, slope), v, mean, var, invstd


def bn_backward(x, gy, gamma, beta, eps, slope, dtype, mask_from_input=False, drop_xhat_term=False):
    """-> (gx, ggamma, gbeta): g' = gy * (y > 0 ? 1 : slope) on the OUTPUT y, xhat = (x - mean) invstd,
    ggamma = sum g' xhat, gbeta = sum g', gx = gamma invstd (g' - mean(g') - xhat mean(g' xhat))."""
    y, _, mean, _, invstd = bn_forward(x, gamma, beta, eps, slope, dtype)
    x, gy = x.to(dtype), gy.to(dtype)
    rows = x.shape[0]
    xhat = (x - mean) * invstd
    gp = gy
    if slope is not None:
        gp = torch.where((x if mask_from_input else y) > 0, gy, gy * slope)
    gbeta, ggamma = gp.sum(0), (gp * xhat).sum(0)
    inner = gp - gbeta / rows
    if not drop_xhat_term:
        inner = inner - xhat * (ggamma / rows)
    gx = invstd * inner
    if gamma is not None:
        gx = gx * gamma.to(dtype)
    return gx, ggamma, gbeta


def running_update(rm, rv, mean, var, rows, momentum, dtype):
    """torch's update: the running mean takes the batch mean, the running variance the UNBIASED one (factor rows / (rows - 1))."""
    return (rm.to(dtype) * (1 - momentum) + mean.to(dtype) * momentum,
            rv.to(dtype) * (1 - momentum) + var.to(dtype) * (momentum * rows / (rows - 1)))


# ---- row gathers and their adjoints ----------------------------------------------------------------------------------------------------
def gather_rows(x, idx, shadow_is_row0=False):
    """x [n, c], idx [m] -> x[idx] with zeros for a shadow (exact in every dtype)."""
    n = x.shape[0]
    ok = real(idx, n)
    if n == 0:
        return torch.zeros((idx.shape[0], x.shape[1]), dtype=x.dtype)
    out = x[_safe(idx, n)]
    return out if shadow_is_row0 else torch.where(ok[:, None], out, torch.zeros_like(out))


def scatter_add_rows(g, n_src, idx, dtype, store=False, shadow_is_row0=False):
    """g [m, c], idx [m] -> gx [n_src, c]: gx[idx[r]] += g[r] over the real rows."""
    g = g.to(dtype)
    gx = torch.zeros((n_src, g.shape[1]), dtype=dtype)
    if n_src == 0 or idx.shape[0] == 0:
        return gx
    ok = real(idx, n_src) | shadow_is_row0
    rows = _safe(idx, n_src)[ok]
    if store:
        gx[rows] = g[ok]                                   # (the last writer wins)
    else:
        gx.index_add_(0, rows, g[ok])
    return gx


def _padded_values(x, inds):
    """[nq, H, c]: the listed rows, zeros for a shadow."""
    n = x.shape[0]
    if n == 0:
        return torch.zeros(tuple(inds.shape) + (x.shape[1],), dtype=x.dtype)
    rows = x[_safe(inds, n)]
    return torch.where(real(inds, n)[:, :, None], rows, torch.zeros_like(rows))


def max_pool(x, inds):
    """The maximum over ALL listed neighbours, a shadow counting as a row of zeros (exact)."""
    return _padded_values(x, inds).max(1)[0]


def max_winners(x, inds, last=False):
    """-> (column of the winner [nq, c], the padded values [nq, H, c]): the FIRST maximal neighbour in list order (``last``: the wrong rule)."""
    vals = _padded_values(x, inds).numpy()
    if last:
        arg = vals.shape[1] - 1 - np.argmax(vals[:, ::-1], axis=1)
    else:
        arg = np.argmax(vals, axis=1)                      # (numpy: the first occurrence of the maximum)
    return torch.from_numpy(arg), torch.from_numpy(vals)


def max_pool_adjoint(x, inds, g, dtype, last=False, shadow_to_real=False, store=False):
    """-> gx [n, c]: the gradient of (q, ch) goes to the first maximal neighbour of the row; a winning shadow drops it
    (``shadow_to_real``, the wrong rule: to the first REAL neighbour that holds the same value)."""
    n, c = x.shape
    nq, H = inds.shape
    g = g.to(dtype)
    gx = torch.zeros((n, c), dtype=dtype)
    if n == 0 or nq == 0 or H == 0:
        return gx
    arg, vals = max_winners(x, inds, last)
    ok = real(inds, n)
    if shadow_to_real:                                     # (the wrong rule, element by element where a shadow wins)
        won = torch.gather(ok, 1, arg)
        for q, ch in torch.nonzero(~won).tolist():
            same = [j for j in range(H) if ok[q, j] and vals[q, j, ch] == vals[q, arg[q, ch], ch]]
            if same:
                arg[q, ch] = same[0]
    rows = torch.gather(inds, 1, arg).long()               # [nq, c]: the winner's index
    keep = torch.gather(ok, 1, arg)
    chs = torch.arange(c)[None].expand(nq, -1)
    gx.index_put_((rows[keep], chs[keep]), g[keep], accumulate=not store)
    return gx


# ---- the attention stage of LocalFeatureAggregation ---------------------------------------------------------------------------------------
def attention_x(f, enc, idx, dtype, shadow_is_row0=False):
    """x [B, N, K, c1 + c2] = [ f[b, idx[b, p, k]] (zeros for a shadow) | enc ]."""
    B, n, _ = f.shape
    f, enc = f.to(dtype), enc.to(dtype)
    ok = real(idx, n)
    rows = f[torch.arange(B)[:, None, None], _safe(idx, n)]
    if not shadow_is_row0:
        rows = rows * ok[..., None].to(dtype)
    return torch.cat([rows, enc], -1)


def attention_forward(f, enc, idx, w, bias, dtype, **kw):
    """-> (out [B, N, d], p [B, N, K, d], x): s = x W^T + bias, p = softmax over K, out = sum_k p x."""
    x = attention_x(f, enc, idx, dtype, **kw)
    s = x @ w.to(dtype).t()
    if bias is not None:
        s = s + bias.to(dtype)
    s = s - s.max(2, keepdim=True)[0]
    p = torch.exp(s)
    p = p / p.sum(2, keepdim=True)
    return (p * x).sum(2), p, x


def attention_backward(f, enc, idx, w, bias, g, dtype, no_minus_out=False, shadow_is_row0=False, store=False):
    """-> (gf, genc, gw, gbias): gs = g p (x - out), gx = gs W + g p, gW = gs^T x, gbias = sum gs; the f half of gx is scattered
    through idx (a shadow takes nothing), the enc half is the gradient of enc."""
    B, n, c1 = f.shape
    out, p, x = attention_forward(f, enc, idx, w, bias, dtype, shadow_is_row0=shadow_is_row0)
    d = x.shape[-1]
    pg = p * g.to(dtype)[:, :, None, :]
    gs = pg * (x if no_minus_out else x - out[:, :, None, :])
    gx = gs @ w.to(dtype) + pg
    gw = gs.reshape(-1, d).t() @ x.reshape(-1, d)
    gb = gs.reshape(-1, d).sum(0)
    gf = torch.zeros((B, n, c1), dtype=dtype)
    for b in range(B):
        gf[b] = scatter_add_rows(gx[b, :, :, :c1].reshape(-1, c1), n, idx[b].reshape(-1), dtype, store=store, shadow_is_row0=shadow_is_row0)
    return gf, gx[..., c1:].contiguous(), gw, gb


# ---- the deformed KPConv aggregation -----------------------------------------------------------------------------------------------------
def deformed_geometry(q, s, inds, dkp, extent, dtype):
    """-> (diff [nq, K, H, 3] = (s[inds] - q) - dkp, dist [nq, K, H], wpre = 1 - dist / extent, real [nq, 1, H])."""
    q, s, dkp = q.to(dtype), s.to(dtype), dkp.to(dtype)
    ns = s.shape[0]
    nb = (s[_safe(inds, ns)] if ns else torch.zeros(inds.shape + (3,), dtype=dtype)) - q[:, None, :]
    diff = nb[:, None, :, :] - dkp[:, :, None, :]
    dist = torch.sqrt((diff ** 2).sum(3))
    return diff, dist, 1 - dist / extent, real(inds, ns)[:, None, :]


def deformed_forward(q, s, inds, x, dkp, extent, dtype):
    """-> wf [nq, K, cin] = sum_h max(0, 1 - |s[inds[q, h]] - q - dkp[q, k]| / extent) x[inds[q, h]] over the real neighbours."""
    nq, h = inds.shape
    ns, cin = x.shape
    if h == 0 or ns == 0:
        return torch.zeros((nq, dkp.shape[1], cin), dtype=dtype)
    _, _, wpre, ok = deformed_geometry(q, s, inds, dkp, extent, dtype)
    w = torch.clamp(wpre, min=0) * ok.to(dtype)
    return torch.matmul(w, x.to(dtype)[_safe(inds, ns)])


def deformed_backward(q, s, inds, x, dkp, extent, dwf, dtype, without=(), ignore_clamp=False, store=False):
    """-> (dx [ns, cin], gkp [nq, K, 3]).  dx[inds[q, h]] += sum_k w dwf[q, k];  with t[q, k, h] = sum_c dwf[q, k, c] x[inds[q, h], c],
    gkp[q, k] = sum_h t (s[inds] - q - dkp) / (dist extent) where 1 - dist / extent >= 0 (clamp's mask, inclusive).  ``without``:
    (q, h, k) terms left out of gkp -- at dist == 0 the formula is 0 / 0."""
    nq, h = inds.shape
    ns, cin = x.shape
    K = dkp.shape[1]
    dx, gkp = torch.zeros((ns, cin), dtype=dtype), torch.zeros((nq, K, 3), dtype=dtype)
    if h == 0 or ns == 0 or nq == 0:
        return dx, gkp
    diff, dist, wpre, ok = deformed_geometry(q, s, inds, dkp, extent, dtype)
    okf = ok.to(dtype)
    w = torch.clamp(wpre, min=0) * okf
    dwf = dwf.to(dtype).reshape(nq, K, cin)
    contrib = torch.matmul(w.transpose(1, 2), dwf)                                  # [nq, h, cin]
    dx = scatter_add_rows(contrib.reshape(-1, cin), ns, inds.reshape(-1), dtype, store=store)
    t = torch.matmul(dwf, x.to(dtype)[_safe(inds, ns)].transpose(1, 2))              # [nq, K, h]
    mask = okf if ignore_clamp else (wpre >= 0).to(dtype) * okf
    coef = t * mask / (extent * dist)
    for qi, hi, ki in without:
        coef[qi, ki, hi] = 0
    return dx, (coef[..., None] * diff).sum(2)


# ---- the offset regulariser ----------------------------------------------------------------------------------------------------------------
def regulariser(q, s, inds, dkp, extent, repulse, dtype):
    """-> dict(fit, rep: the two L1 terms (means over (q, k)); min_d2 [nq, K]; gfit, grep [nq, K, 3]: the gradients of the two SUMS over
    (q, k); d2 [nq, H, K]; active [nq, K, K]: the pairs whose repulsion is on).  A shadow neighbour sits at 1e6; the fitting gradient
    goes to the first minimum; the other points of the repulsive term are detached."""
    q, s, dkp = q.to(dtype), s.to(dtype), dkp.to(dtype)
    nq, K = dkp.shape[:2]
    ns, H = s.shape[0], inds.shape[1]
    far = torch.cat([s, torch.full((1, 3), FAR, dtype=dtype)], 0)
    idx = torch.where(real(inds, ns), inds, torch.full_like(inds, ns)).long()
    diff = (far[idx] - q[:, None, :])[:, :, None, :] - dkp[:, None, :, :]               # [nq, H, K, 3]
    d2 = (diff ** 2).sum(3)
    if H:
        arg = torch.from_numpy(np.argmin(d2.numpy(), axis=1))                        # (numpy: the first occurrence of the minimum)
        min_d2 = torch.gather(d2, 1, arg[:, None, :])[:, 0]
        best = torch.gather(diff, 1, arg[:, None, :, None].expand(-1, -1, -1, 3))[:, 0]
    else:
        min_d2, best = torch.zeros((nq, K), dtype=dtype), torch.zeros((nq, K, 3), dtype=dtype)
    gfit = -2 * best / extent ** 2
    locs = dkp / extent
    dl = locs[:, None, :, :] - locs[:, :, None, :]                                    # [nq, k, j, 3] = l_j - l_k
    dist = torch.sqrt((dl ** 2).sum(3))
    off = ~torch.eye(K, dtype=torch.bool)[None]
    c = torch.clamp(dist - repulse, max=0) * off.to(dtype)
    active = (c < 0) & (dist > 0)
    wgt = torch.where(active, 2 * c / torch.where(dist > 0, dist, torch.ones_like(dist)), torch.zeros_like(c))
    grep = -(wgt[..., None] * dl).sum(2) / extent
    denom = float(max(nq * K, 1))
    return dict(fit=min_d2.sum() / extent ** 2 / denom, rep=(c ** 2).sum() / denom, min_d2=min_d2, gfit=gfit, grep=grep, d2=d2,
                active=active, pairs=off.expand(nq, -1, -1))


# ---- RandLA-Net's differentiable ops --------------------------------------------------------------------------------------------------------
def gather_max(feat, idx, n_out):
    """feat [B, n_in, c], idx [B, n_in, K] (in range) -> [B, n_out, c]: the max over the listed neighbours of the first n_out rows (exact)."""
    B = feat.shape[0]
    return feat[torch.arange(B)[:, None, None], idx[:, :n_out].long()].max(2)[0]


def gather_max_adjoint(feat, idx, n_out, g, dtype, last=False, store=False):
    B, n_in, c = feat.shape
    gf = torch.zeros((B, n_in, c), dtype=dtype)
    for b in range(B):
        gf[b] = max_pool_adjoint(feat[b], idx[b, :n_out], g[b], dtype, last=last, store=store)
    return gf


def attentive_pool(scores, x, dtype):
    """scores, x [rows, K, c] -> (out [rows, c], p)."""
    s, x = scores.to(dtype), x.to(dtype)
    s = s - s.max(1, keepdim=True)[0]
    p = torch.exp(s)
    p = p / p.sum(1, keepdim=True)
    return (p * x).sum(1), p


def attentive_pool_backward(scores, x, g, dtype, no_minus_out=False):
    """-> (gscores = p (x - out) g, gx = p g)."""
    out, p = attentive_pool(scores, x, dtype)
    pg = p * g.to(dtype)[:, None, :]
    xd = x.to(dtype)
    return pg * (xd if no_minus_out else xd - out[:, None, :]), pg
