"""PointNet++ multi-scale-grouping ops on the HIP kernels of csrc/pointnet2.hip (contracts: include/ml3d_hip.h, "PointNet++
MSG backbone inference"): ball query for all scales of a level in one scan, the exact three nearest neighbours, three-point
interpolation, and the set-abstraction body (grouped MLP + maximum).  The public three take the reference's shapes
(``pointnet2_utils.py``); the ``pn2_*`` entries are the row-major forms the ``Pointnet2MSG`` class runs on."""
import numpy as np
import torch

from .. import _abi
from . import _gates
from .gemm import _rows
from .search import knn_search


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def _f32c(name, *tensors):
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("%s: float32 contiguous tensors required" % name)


def _i32c(name, *tensors):
    for t in tensors:
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("%s: contiguous int32 index tensors required" % name)


def ball_query(xyz, new_xyz, radius, nsample):
    """``ball_query(xyz, new_xyz, radius, nsample)`` (pointnet2_utils.py:212): ``xyz`` [B, N, 3], ``new_xyz`` [B, m, 3] ->
    int32 [B, m, nsample], item-local, the first ``nsample`` points with d2 < r * r in ascending index, padded with the first
    hit (all zeros without one).  Multi-scale form: ``radius`` and ``nsample`` sequences of 1 - 4 entries -> one tensor per
    scale from ONE scan of the points."""
    _need_gpu(xyz, new_xyz)
    lib = _abi.get()
    many = isinstance(radius, (list, tuple))
    radii = [float(r) for r in (radius if many else [radius])]
    ns = [int(k) for k in (nsample if many else [nsample])]
    if isinstance(nsample, (list, tuple)) != many or len(radii) != len(ns):
        raise RuntimeError("ball_query: radius and nsample must both be scalars or sequences of the same length")
    if xyz.dim() != 3 or new_xyz.dim() != 3 or xyz.shape[2] != 3 or new_xyz.shape[2] != 3 or xyz.shape[0] != new_xyz.shape[0]:
        raise RuntimeError("ball_query: xyz [B, N, 3] and new_xyz [B, m, 3] expected")
    _f32c("ball_query", xyz, new_xyz)
    b, n, m = int(xyz.shape[0]), int(xyz.shape[1]), int(new_xyz.shape[1])
    outs = [torch.empty((b, m, k), dtype=torch.int32, device=xyz.device) for k in (max(k, 0) for k in ns)]
    r_host, k_host = np.asarray(radii, np.float32), np.asarray(ns, np.int32)
    ptrs = _abi.ptr_table([o.data_ptr() for o in outs])
    with torch.cuda.device(xyz.device):
        rc = lib.ml3d_ball_query(xyz.data_ptr(), new_xyz.data_ptr(), b, n, m, len(ns), r_host.ctypes.data, k_host.ctypes.data,
                                 ptrs, _stream())
    _abi.check(rc, "ml3d_ball_query")
    return outs if many else outs[0]


def three_nn(query, data):
    """``three_nn(query_pts, data_pts)`` (pointnet2_utils.py:129): ``query`` [B, n, 3], ``data`` [B, M, 3] -> (dist2 [B, n, 3]
    SQUARED distances, idx int32 [B, n, 3] item-local), ascending d2, ties to the lowest index (the exact k-NN's order).
    Fewer than 3 data points per item are refused."""
    _need_gpu(query, data)
    if query.dim() != 3 or data.dim() != 3 or query.shape[2] != 3 or data.shape[2] != 3 or query.shape[0] != data.shape[0]:
        raise RuntimeError("three_nn: query [B, n, 3] and data [B, M, 3] expected")
    _f32c("three_nn", query, data)
    b, n, mk = int(query.shape[0]), int(query.shape[1]), int(data.shape[1])
    if mk < 3:
        raise RuntimeError("three_nn: invalid argument: %d data points per item, 3 neighbours need at least 3" % mk)
    dev = query.device
    prs = torch.arange(0, (b + 1) * mk, mk, dtype=torch.int64, device=dev)
    qrs = torch.arange(0, (b + 1) * n, n, dtype=torch.int64, device=dev)
    r = knn_search(data.reshape(b * mk, 3), query.reshape(b * n, 3), 3, prs, qrs, return_distances=True, index_local=True)
    return r.neighbors_distance.view(b, n, 3), r.neighbors_index.view(b, n, 3)


def pn2_interpolate(known, batch, idx, dist2=None, weight=None, out=None):
    """``PointnetFPModule.forward`` before its MLP (pointnet.py:278-284) on rows: ``known`` [B * M, c] (may be a column slice),
    ``idx`` int32 / ``dist2`` f32 [B * n, 3] as ``three_nn`` gives them (or the caller's own ``weight`` instead of ``dist2``) ->
    ``out`` [B * n, c], which may be a column slice of the concat buffer the MLP reads."""
    _need_gpu(known, idx, dist2, weight, out)
    lib = _abi.get()
    ldk = _rows("pn2_interpolate", known)
    w = dist2 if weight is None else weight
    if (dist2 is None) == (weight is None) or idx.dim() != 2 or idx.shape[1] != 3 or tuple(w.shape) != tuple(idx.shape):
        raise RuntimeError("pn2_interpolate: idx [rows, 3] and one of dist2 / weight [rows, 3] expected")
    _i32c("pn2_interpolate", idx)
    _f32c("pn2_interpolate", w)
    rows, c, batch = int(idx.shape[0]), int(known.shape[1]), int(batch)
    if batch < 1 or rows % batch or known.shape[0] % batch:
        raise RuntimeError("pn2_interpolate: rows must be a multiple of the batch size")
    if out is None:
        out = torch.empty((rows, c), dtype=torch.float32, device=known.device)
    ldo = _rows("pn2_interpolate", out, c)
    if out.shape[0] != rows:
        raise RuntimeError("pn2_interpolate: out has %d rows, %d expected" % (out.shape[0], rows))
    with torch.cuda.device(known.device):
        rc = lib.ml3d_pn2_interpolate(known.data_ptr(), ldk, batch, known.shape[0] // batch, idx.data_ptr(),
                                      None if dist2 is None else dist2.data_ptr(), None if weight is None else weight.data_ptr(),
                                      rows // batch, c, out.data_ptr(), ldo, _stream())
    _abi.check(rc, "ml3d_pn2_interpolate")
    return out


def three_interpolate(features, idx, weight):
    """``three_interpolate(features, idx, weight)`` (pointnet2_utils.py:162): ``features`` [B, C, M], ``idx`` int32 / ``weight``
    [B, n, 3] -> [B, C, n]."""
    _need_gpu(features, idx, weight)
    if features.dim() != 3 or idx.dim() != 3 or idx.shape[2] != 3 or idx.shape != weight.shape or idx.shape[0] != features.shape[0]:
        raise RuntimeError("three_interpolate: features [B, C, M], idx and weight [B, n, 3] expected")
    b, c, mk = (int(v) for v in features.shape)
    n = int(idx.shape[1])
    rows = features.transpose(1, 2).contiguous().view(b * mk, c)
    out = pn2_interpolate(rows, b, idx.reshape(b * n, 3), weight=weight.reshape(b * n, 3))
    return out.view(b, n, c).transpose(1, 2).contiguous()


SA_KEYS = ("w_x", "b1", "w2", "b2", "w3", "b3")


def sa_fused(nsample, c1, c2, c3):
    """The dispatch rule of ``pn2_sa_mlp_max``, from shape alone: nsample 16 or 32 and every width at most 128 (c1 even, c3 a
    multiple of 32, c2 after padding to a multiple of 32) run as ONE kernel; everything else goes the unfused route."""
    return bool(_abi.get().ml3d_pn2_sa_fused_supported(int(nsample), int(c1), int(c2), int(c3)))


def pack_sa_weights(w_x, b1, w2, b2, w3, b3, nsample):
    """The parameters of one scale as ``pn2_sa_mlp_max`` takes them: ``w_x`` [3, c1] (the position rows of the first layer),
    ``w2`` [c1, c2], ``w3`` [c2, c3] (transposed, the folded BatchNorm scale multiplied into the columns) and the shifts
    ``b1`` / ``b2`` / ``b3``.  On the fused route the middle width is zero-padded to a multiple of 32."""
    c1, c2, c3 = int(w2.shape[0]), int(w2.shape[1]), int(w3.shape[1])
    if tuple(w_x.shape) != (3, c1) or tuple(w3.shape) != (c2, c3) or (b1.numel(), b2.numel(), b3.numel()) != (c1, c2, c3):
        raise RuntimeError("pack_sa_weights: inconsistent shapes")
    p = dict(w_x=w_x, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3)
    p = {k: v.detach().float().contiguous() for k, v in p.items()}
    fused = sa_fused(nsample, c1, c2, c3)
    if fused and c2 % 32:
        c2p = (c2 + 31) // 32 * 32
        p["w2"] = torch.nn.functional.pad(p["w2"], (0, c2p - c2)).contiguous()
        p["b2"] = torch.nn.functional.pad(p["b2"], (0, c2p - c2)).contiguous()
        p["w3"] = torch.nn.functional.pad(p["w3"], (0, 0, 0, c2p - c2)).contiguous()
    p.update(fused=fused, widths=(c1, c2, c3), nsample=int(nsample))
    return p


def _linear_rows(a, w, bias, act, out=None, a2=None):
    """``ml3d_linear`` on rows that may be column slices -> act([a | a2] w + bias) into ``out`` (may be a column slice)."""
    lib = _abi.get()
    m, k, n = int(a.shape[0]), int(a.shape[1]), int(w.shape[1])
    lda = _rows("pn2 linear", a)
    lda2, k2 = (0, 0) if a2 is None else (_rows("pn2 linear", a2), int(a2.shape[1]))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    ldc = _rows("pn2 linear", out, n)
    if w.shape[0] != k + k2 or not w.is_contiguous() or out.shape[0] != m or (a2 is not None and a2.shape[0] != m):
        raise RuntimeError("pn2 linear: inconsistent shapes")
    wsb = lib.ml3d_linear_workspace_bytes(m, n, k + k2)
    ws = _gates._ws(wsb, a.device)
    with torch.cuda.device(a.device):
        rc = lib.ml3d_linear(a.data_ptr(), lda, k, None, 0, m, None if a2 is None else a2.data_ptr(), lda2, k2, w.data_ptr(),
                             None if bias is None else bias.data_ptr(), None, 0, None, 0, 0, int(act), 0.0, out.data_ptr(), ldc, m, n,
                             ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_linear")
    return out


def pn2_sa_mlp_max(y, xyz, centres, idx, params, out=None):
    """One scale of ``PointnetSAModuleMSG`` after the first-layer feature product: ``y`` [B * n, c1] = f Wf per SOURCE point (may
    be a column slice of the product for all scales; None for a level without features), ``xyz`` [B, n, 3], ``centres``
    [B, m, 3], ``idx`` int32 [B, m, nsample] (``ball_query``), ``params`` = ``pack_sa_weights(...)`` -> ``out`` [B * m, c3],
    which may be a column slice of the level's output."""
    ts = [params[k] for k in SA_KEYS]
    _need_gpu(y, xyz, centres, idx, out, *ts)
    lib = _abi.get()
    c1, c2, c3 = params["widths"]
    ldy = 0 if y is None else _rows("pn2_sa_mlp_max", y, c1)
    _f32c("pn2_sa_mlp_max", xyz, centres)
    _i32c("pn2_sa_mlp_max", idx)
    if xyz.dim() != 3 or xyz.shape[2] != 3 or centres.dim() != 3 or centres.shape[2] != 3 or centres.shape[0] != xyz.shape[0] or \
            idx.dim() != 3 or idx.shape[:2] != centres.shape[:2] or idx.shape[2] != params["nsample"] or \
            (y is not None and y.shape[0] != xyz.shape[0] * xyz.shape[1]):
        raise RuntimeError("pn2_sa_mlp_max: y [B * n, c1], xyz [B, n, 3], centres [B, m, 3] and idx [B, m, nsample] expected")
    b, m, ns = (int(v) for v in idx.shape)
    dev = xyz.device
    if out is None:
        out = torch.empty((b * m, c3), dtype=torch.float32, device=dev)
    ldo = _rows("pn2_sa_mlp_max", out, c3)
    if out.shape[0] != b * m:
        raise RuntimeError("pn2_sa_mlp_max: out has %d rows, %d expected" % (out.shape[0], b * m))
    lead = (None if y is None else y.data_ptr(), ldy, xyz.data_ptr(), centres.data_ptr(), idx.data_ptr(), b, int(xyz.shape[1]), m, ns)
    with torch.cuda.device(dev):
        if params["fused"]:
            rc = lib.ml3d_pn2_sa_mlp_max(*lead, c1, c2, c3, *[t.data_ptr() for t in ts], out.data_ptr(), ldo, _stream())
            _abi.check(rc, "ml3d_pn2_sa_mlp_max")
            return out
        h1 = torch.empty((b * m * ns, c1), dtype=torch.float32, device=dev)
        rc = lib.ml3d_pn2_group_rows(*lead, c1, params["w_x"].data_ptr(), params["b1"].data_ptr(), h1.data_ptr(), c1, _stream())
        _abi.check(rc, "ml3d_pn2_group_rows")
        h3 = _linear_rows(_linear_rows(h1, params["w2"], params["b2"], 2), params["w3"], params["b3"], 2)
        wsb = int(lib.ml3d_segment_max_rows_workspace_bytes(b * m, ns, c3))
        ws = _gates._ws(wsb, dev)
        rc = lib.ml3d_segment_max_rows(h3.data_ptr(), c3, b * m, ns, c3, out.data_ptr(), ldo, ws.data_ptr(), wsb, _stream())
        _abi.check(rc, "ml3d_segment_max_rows")
    return out


__all__ = ["ball_query", "three_nn", "three_interpolate", "pn2_interpolate", "pn2_sa_mlp_max", "pack_sa_weights", "sa_fused", "SA_KEYS"]
