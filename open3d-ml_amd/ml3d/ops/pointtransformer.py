"""PointTransformer inference ops (an extension beyond SURVEY.md's scope table): furthest point sampling, the fused vector
self-attention layer, TransitionDown's gather / max and TransitionUp's 3-NN interpolation on the HIP kernels of
csrc/ptransformer.hip (contracts: include/ml3d_hip.h, "PointTransformer inference")."""
import numpy as np
import torch

from .. import _abi
from . import _gates
from .kpconv import linear


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def _f32(name, *tensors):
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("%s: float32 contiguous tensors required" % name)


def _i32(name, *tensors):
    for t in tensors:
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("%s: contiguous int32 index tensors required" % name)


def _host_splits(rs):
    if torch.is_tensor(rs):
        rs = rs.detach().cpu().numpy()      # (a device tensor costs one read-back here: pass host splits to avoid it)
    return np.ascontiguousarray(rs, dtype=np.int64).reshape(-1)


def furthest_point_sampling(points, row_splits, new_row_splits, row_splits_host=None, new_row_splits_host=None):
    """``furthest_point_sample_v2(point, row_splits, new_row_splits)`` (point_transformer.py:518): int32 GLOBAL rows, per
    item the canonical order of ``ml3d_furthest_point_sampling`` (first point first, float32 distances without fma, ties to
    the lowest index).  ``row_splits`` / ``new_row_splits``: int64 [batch + 1], tensors on any device or sequences; the
    ``*_host`` arguments (numpy / sequences with the same values) spare the read-back of device tensors."""
    _need_gpu(points)
    lib = _abi.get()
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("furthest_point_sampling: points must be [n, 3]")
    _f32("furthest_point_sampling", points)
    dev = points.device
    rsh = _host_splits(row_splits if row_splits_host is None else row_splits_host)
    nrsh = _host_splits(new_row_splits if new_row_splits_host is None else new_row_splits_host)
    if rsh.shape != nrsh.shape or rsh.size < 1:
        raise RuntimeError("furthest_point_sampling: row_splits and new_row_splits must have the same length")
    batch, n = rsh.size - 1, int(points.shape[0])
    rs = row_splits.to(device=dev, dtype=torch.int64).contiguous() if torch.is_tensor(row_splits) else \
        torch.from_numpy(rsh).to(dev)
    nrs = new_row_splits.to(device=dev, dtype=torch.int64).contiguous() if torch.is_tensor(new_row_splits) else \
        torch.from_numpy(nrsh).to(dev)
    out = torch.empty((int(nrsh[-1]),), dtype=torch.int32, device=dev)
    longest = int(np.max(np.diff(rsh))) if batch else 0
    wsb = lib.ml3d_fps_workspace_bytes(n, batch) if longest > 65536 else 0
    ws = _gates._ws(wsb, dev) if wsb else None
    with torch.cuda.device(dev):
        rc = lib.ml3d_furthest_point_sampling(points.data_ptr(), rs.data_ptr(), nrs.data_ptr(), rsh.ctypes.data,
                                              nrsh.ctypes.data, batch, n, out.data_ptr(),
                                              None if ws is None else ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_furthest_point_sampling")
    return out


ATTENTION_KEYS = ("p_w1", "p_b1", "p_w2t", "p_b2", "w_scale0", "w_shift0", "w_w1", "w_b1", "w_w2", "w_b2")


def attention_hidden_rows(c):
    """Rows of the padded ``w_w1`` / ``w_b1`` that ``ml3d_pt_attention`` reads for width ``c``."""
    return 16 if c <= 128 else (32 if c <= 256 else 64)


def pt_attention(qkv, points, neighbor_idx, params, epilogue=None):
    """``Transformer.forward`` (point_transformer.py:416-467) on ``qkv`` [n, 3c] = [q | k | v].  ``params``: dict with
    ``ATTENTION_KEYS`` (folded, laid out as include/ml3d_hip.h describes; ``w_w1`` / ``w_b1`` padded to
    ``attention_hidden_rows(c)`` rows); ``epilogue`` = (scale, shift) [c]: ``relu(out * scale + shift)`` fused in."""
    ts = [params[k] for k in ATTENTION_KEYS]
    ep = (None, None) if epilogue is None else tuple(epilogue)
    _need_gpu(qkv, points, neighbor_idx, *ts, *ep)
    lib = _abi.get()
    _f32("pt_attention", qkv, points, *ts, *ep)
    _i32("pt_attention", neighbor_idx)
    n, c3 = qkv.shape
    c, ns = c3 // 3, int(neighbor_idx.shape[1])
    if c3 != 3 * c or neighbor_idx.shape[0] != n or points.shape[0] != n:
        raise RuntimeError("pt_attention: qkv [n, 3c], points [n, 3] and neighbor_idx [n, nsample] expected")
    R = attention_hidden_rows(c)
    want = dict(p_w1=(3, 3), p_b1=(3,), p_w2t=(3, c), p_b2=(c,), w_scale0=(c,), w_shift0=(c,), w_w1=(R, c), w_b1=(R,),
                w_w2=(c // 8, c // 8), w_b2=(c // 8,))
    for k in ATTENTION_KEYS:
        if tuple(params[k].shape) != want[k]:
            raise RuntimeError("pt_attention: %s has shape %s, expected %s" % (k, tuple(params[k].shape), want[k]))
    out = torch.empty((n, c), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = lib.ml3d_pt_attention(qkv.data_ptr(), points.data_ptr(), neighbor_idx.data_ptr(), n, c, ns,
                                   *[t.data_ptr() for t in ts], *[None if t is None else t.data_ptr() for t in ep],
                                   out.data_ptr(), _stream())
    _abi.check(rc, "ml3d_pt_attention")
    return out


def pt_transition_down(feat, points, sample_idx, neighbor_idx, w_f_t, w_x, scale, shift):
    """``TransitionDown.forward`` with stride != 1 after the sampling (point_transformer.py:520-533): ``feat`` [n, c] of the
    source level, ``sample_idx`` int32 [m] (the FPS rows), ``neighbor_idx`` int32 [m, nsample]; the Linear (3 + c -> c', no
    bias) arrives split: ``w_f_t`` [c, c'] (feature columns, transposed), ``w_x`` [3, c'] (position columns, transposed);
    ``scale`` / ``shift`` the folded BatchNorm.  Returns (new_points [m, 3], new_feat [m, c'])."""
    _need_gpu(feat, points, sample_idx, neighbor_idx, w_f_t, w_x, scale, shift)
    lib = _abi.get()
    _f32("pt_transition_down", feat, points, w_f_t, w_x, scale, shift)
    _i32("pt_transition_down", sample_idx, neighbor_idx)
    m, ns, cout = int(sample_idx.shape[0]), int(neighbor_idx.shape[1]), int(w_f_t.shape[1])
    if neighbor_idx.shape[0] != m or tuple(w_x.shape) != (3, cout) or feat.shape[0] != points.shape[0]:
        raise RuntimeError("pt_transition_down: inconsistent shapes")
    y = linear(feat, w_f_t)      # once per SOURCE point (16x fewer products than per neighbour)
    out = torch.empty((m, cout), dtype=torch.float32, device=feat.device)
    new_points = torch.empty((m, 3), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        rc = lib.ml3d_pt_transition_down(y.data_ptr(), points.data_ptr(), points.shape[0], sample_idx.data_ptr(),
                                         neighbor_idx.data_ptr(), m, ns, cout, w_x.data_ptr(), scale.data_ptr(),
                                         shift.data_ptr(), out.data_ptr(), new_points.data_ptr(), _stream())
    _abi.check(rc, "ml3d_pt_transition_down")
    return new_points, out


def pt_interpolate(a, b, idx, dist2):
    """``a + interpolation(...)`` of ``TransitionUp.forward`` (point_transformer.py:597, 737-776): ``a`` [n, c] or None,
    ``b`` [n_src, c], ``idx`` / ``dist2`` [n, k] as ``knn_search(..., return_distances=True)`` returns them."""
    _need_gpu(a, b, idx, dist2)
    lib = _abi.get()
    _f32("pt_interpolate", a, b, dist2)
    _i32("pt_interpolate", idx)
    n, k = idx.shape
    c = int(b.shape[1])
    if tuple(dist2.shape) != (n, k) or (a is not None and tuple(a.shape) != (n, c)):
        raise RuntimeError("pt_interpolate: inconsistent shapes")
    out = torch.empty((n, c), dtype=torch.float32, device=b.device)
    with torch.cuda.device(b.device):
        rc = lib.ml3d_pt_interpolate(None if a is None else a.data_ptr(), b.data_ptr(), b.shape[0], idx.data_ptr(),
                                     dist2.data_ptr(), n, k, c, out.data_ptr(), _stream())
    _abi.check(rc, "ml3d_pt_interpolate")
    return out
