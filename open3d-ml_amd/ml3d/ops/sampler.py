"""Patch sampler query, label argmax and the float16 vote update."""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from . import _gates
from ._gates import KnnResult, RadiusResult, VoxelizeResult, _splits, _splits_of_lengths


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def _ws(nbytes, device):
    return _gates._ws(nbytes, device)

def nearest_to_center(points, center, k, return_distances=False):
    """The ``k`` points nearest to ``center`` — the ``search_tree.query(center_point, k=num_points)`` of
    SemSegSpatiallyRegularSampler (ml3d/datasets/samplers/semseg_spatially_regular.py:90-91) in the order of the
    reference's sklearn ``KDTree``: ascending FLOAT64 reduced distance (ties: ascending index).  int32 indices [k]
    and, on request, the float64 reduced distances."""
    lib = _abi.get()
    _need_gpu(points)
    points = points.contiguous().float()
    n = points.shape[0]
    dev = points.device
    c = torch.as_tensor(center, dtype=torch.float32).detach().cpu().reshape(-1).contiguous()
    if c.numel() != 3 or not (0 <= int(k) <= n):
        raise RuntimeError("nearest_to_center: center must have 3 elements and 0 <= k <= n_points")
    idx = torch.empty(int(k), dtype=torch.int32, device=dev)
    d2 = torch.empty(int(k), dtype=torch.float64, device=dev) if return_distances else None
    wsb = lib.ml3d_nearest_to_center_workspace_bytes(n)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_nearest_to_center(points.data_ptr(), n, c.data_ptr(), int(k), idx.data_ptr(),
                                        None if d2 is None else d2.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_nearest_to_center")
    return (idx, d2) if return_distances else idx


def device_patch(points, possibility, center_index, perm, k, recenter_dims=(), extra=None, feat_bias=0.0, feat_scale=1.0, out=None):
    """One step of the spatially regular patch loop (semseg_spatially_regular.py:64-111 + randlanet.py:185-212) with nothing
    read back: ``points`` float32 [n, 3], ``possibility`` float64 [n] (bumped IN PLACE), ``center_index`` a 1-element DEVICE
    index tensor (the argmin of the possibilities), ``perm`` the host-drawn shuffle of 0..k-1 as a device int32 tensor,
    ``extra`` optional float32 [n, c] per-point features.  Returns (patch points [k, 3] recentred on ``recenter_dims``,
    features [k, 3 + c], selected cloud indices int32 [k]) -- the arithmetic and its ORDER are numpy's (float32 squared
    distances left to right, sequential float32 column sums for the mean): the patch feeds an exact neighbour search.
    ``out``: optional preallocated (points [k, 3] float32, features [k, 3 + c] float32, indices [k] int32) to write into."""
    lib = _abi.get()
    _need_gpu(points, possibility, center_index, perm)
    dev = points.device
    n = points.shape[0]
    k = int(k)
    if points.dtype != torch.float32 or not points.is_contiguous() or possibility.dtype != torch.float64 or \
            not possibility.is_contiguous() or possibility.numel() != n or perm.dtype != torch.int32 or perm.numel() != k or k > n:
        raise RuntimeError("device_patch: float32 [n, 3] points, float64 [n] possibilities, int32 [k] permutation, k <= n")
    center = points[center_index.reshape(1)].reshape(3).contiguous()          # (a device gather: the centre is never on the host)
    cand = torch.empty(k, dtype=torch.int32, device=dev)
    wsb = lib.ml3d_nearest_to_center_workspace_bytes(n)
    ws = _ws(wsb, dev)
    n_extra = 0 if extra is None else int(extra.shape[1])
    if out is None:
        pts = torch.empty((k, 3), dtype=torch.float32, device=dev)
        sel = torch.empty(k, dtype=torch.int32, device=dev)
        feats = torch.empty((k, 3 + n_extra), dtype=torch.float32, device=dev)
    else:
        pts, feats, sel = out
        if tuple(pts.shape) != (k, 3) or tuple(feats.shape) != (k, 3 + n_extra) or sel.numel() != k or pts.dtype != torch.float32 or \
                feats.dtype != torch.float32 or sel.dtype != torch.int32 or not (pts.is_contiguous() and feats.is_contiguous() and sel.is_contiguous()):
            raise RuntimeError("device_patch: out = (float32 [k, 3], float32 [k, 3 + c], int32 [k]), contiguous")
    scratch = torch.empty(4 * k + 64, dtype=torch.uint8, device=dev)
    ex = None
    mask = 0
    for d in recenter_dims:
        mask |= 1 << int(d)
    with torch.cuda.device(dev):
        rc = lib.ml3d_nearest_to_center_dev(points.data_ptr(), n, center.data_ptr(), k, cand.data_ptr(), None, ws.data_ptr(), wsb,
                                            _stream())
        _abi.check(rc, "ml3d_nearest_to_center_dev")
        rc = lib.ml3d_patch_crop(points.data_ptr(), n, cand.data_ptr(), perm.data_ptr(), center.data_ptr(), k, pts.data_ptr(),
                                 sel.data_ptr(), possibility.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream())
        _abi.check(rc, "ml3d_patch_crop")
        if n_extra:
            ex = extra[sel.long()].contiguous()
        rc = lib.ml3d_patch_recenter(pts.data_ptr(), k, mask, None if ex is None else ex.data_ptr(), n_extra, float(feat_bias),
                                     float(feat_scale), feats.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream())
        _abi.check(rc, "ml3d_patch_recenter")
    return pts, feats, sel


def _host_splits(cloud_row_splits, active, what):
    """The two HOST arrays of the multi-cloud entries: int64 row splits [C + 1] and the int32 list of active slots."""
    splits = np.ascontiguousarray(cloud_row_splits.cpu().numpy() if isinstance(cloud_row_splits, torch.Tensor) else cloud_row_splits,
                                  dtype=np.int64).reshape(-1)
    n_clouds = splits.size - 1
    act = np.arange(n_clouds, dtype=np.int32) if active is None else \
        np.ascontiguousarray(active.cpu().numpy() if isinstance(active, torch.Tensor) else active, dtype=np.int32).reshape(-1)
    if n_clouds < 1 or act.size < 1 or splits[0] != 0 or np.any(np.diff(splits) < 0) or act.min() < 0 or act.max() >= n_clouds or \
            np.any(np.diff(act) <= 0):
        raise RuntimeError(what + ": cloud_row_splits must be monotone from 0, active a strictly ascending list of its slots")
    return splits, act


def _check_cloud_set(what, splits, act, min_len, points=None, possibility=None, center_index=None, extra=None, recenter_dims=()):
    """What the multi-cloud entries take of a concatenated cloud set, checked against its host ``splits`` / ``act``: those given of
    ``points`` float32 [N, 3], ``possibility`` float64 [N], ``center_index`` int32 [C] and the optional per-point ``extra`` float32
    [N, c], and at least ``min_len`` points in every active cloud.  Returns (c, the bit mask of ``recenter_dims``)."""
    n, n_clouds = int(splits[-1]), splits.size - 1
    bad = bool(np.any(np.diff(splits)[act] < min_len))
    if points is not None:
        bad |= points.dtype != torch.float32 or not points.is_contiguous() or tuple(points.shape) != (n, 3)
    if possibility is not None:
        bad |= possibility.dtype != torch.float64 or not possibility.is_contiguous() or possibility.dim() != 1 or possibility.numel() != n
    if center_index is not None:
        bad |= center_index.dtype != torch.int32 or center_index.numel() != n_clouds or not center_index.is_contiguous()
    if bad:
        raise RuntimeError("%s: contiguous float32 [N, 3] points, float64 [N] possibilities and int32 [C] centre indices, "
                           "N == cloud_row_splits[-1], at least %d points in every active cloud" % (what, min_len))
    n_extra = 0
    if extra is not None:
        if extra.dtype != torch.float32 or not extra.is_contiguous() or extra.dim() != 2 or extra.shape[0] != n:
            raise RuntimeError(what + ": extra must be a contiguous float32 [N, c] tensor")
        _need_gpu(extra)
        n_extra = int(extra.shape[1])
    mask = 0
    for d in recenter_dims:
        mask |= 1 << int(d)
    return n_extra, mask


def possibility_argmin(possibility, cloud_row_splits, active=None, out=None):
    """Per cloud of a concatenated float64 ``possibility`` [N] (clouds delimited by the HOST ``cloud_row_splits`` [C + 1]): the
    FIRST index of its minimum (cloud-local, ``torch.argmin`` order) and the minimum -- (int32 [C], float64 [C]) device tensors,
    written for the slots of the HOST list ``active`` only (default: all; other entries of ``out`` are left as they are).
    Deterministic, two launches, nothing read back: the minima are the multi-cloud loop's one read-back per round."""
    lib = _abi.get()
    _need_gpu(possibility)
    splits, act = _host_splits(cloud_row_splits, active, "possibility_argmin")
    n_clouds = splits.size - 1
    dev = possibility.device
    _check_cloud_set("possibility_argmin", splits, act, 1, possibility=possibility)
    if out is None:
        idx = torch.empty(n_clouds, dtype=torch.int32, device=dev)
        mins = torch.empty(n_clouds, dtype=torch.float64, device=dev)
    else:
        idx, mins = out
        if idx.dtype != torch.int32 or mins.dtype != torch.float64 or idx.numel() != n_clouds or mins.numel() != n_clouds or \
                not (idx.is_contiguous() and mins.is_contiguous()):
            raise RuntimeError("possibility_argmin: out = (int32 [C], float64 [C]), contiguous")
    m = int(np.diff(splits)[act].sum())
    wsb = lib.ml3d_possibility_argmin_workspace_bytes(m, act.size)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_possibility_argmin(possibility.data_ptr(), splits.ctypes.data, n_clouds, act.ctypes.data, act.size,
                                         idx.data_ptr(), mins.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_possibility_argmin")
    return idx, mins


def device_patch_batch(points, possibility, cloud_row_splits, active, center_index, perm, k, recenter_dims=(), extra=None,
                       feat_bias=0.0, feat_scale=1.0, out=None):
    """One ROUND of the spatially regular patch loop for the A active clouds of a concatenated set (``device_patch`` for several
    clouds in lock step): ``points`` float32 [N, 3], ``possibility`` float64 [N] (bumped IN PLACE), HOST ``cloud_row_splits``
    [C + 1] and HOST ``active`` slot list (None: all), ``center_index`` DEVICE int32 [C] (``possibility_argmin``), ``perm`` DEVICE
    int32 [A, k] (row a: the a-th active cloud's own host-drawn shuffle of 0..k-1), ``extra`` optional float32 [N, c].
    Returns (points [A, k, 3] recentred on ``recenter_dims``, features [A, k, 3 + c], cloud-local indices int32 [A, k], rows of
    the concatenated arrays int32 [A, k]); every item is bit for bit what ``device_patch`` gives on its cloud alone.
    ``out``: the four tensors preallocated."""
    lib = _abi.get()
    _need_gpu(points, possibility, center_index, perm)
    splits, act = _host_splits(cloud_row_splits, active, "device_patch_batch")
    n_clouds, A, k = splits.size - 1, int(act.size), int(k)
    dev = points.device
    if perm.dtype != torch.int32 or tuple(perm.shape) != (A, k) or not perm.is_contiguous() or k < 1:
        raise RuntimeError("device_patch_batch: contiguous int32 [A, k] permutations, k >= 1")
    n_extra, mask = _check_cloud_set("device_patch_batch", splits, act, k, points, possibility, center_index, extra, recenter_dims)
    if out is None:
        pts = torch.empty((A, k, 3), dtype=torch.float32, device=dev)
        feats = torch.empty((A, k, 3 + n_extra), dtype=torch.float32, device=dev)
        sel = torch.empty((A, k), dtype=torch.int32, device=dev)
        row = torch.empty((A, k), dtype=torch.int32, device=dev)
    else:
        pts, feats, sel, row = out
        if tuple(pts.shape) != (A, k, 3) or tuple(feats.shape) != (A, k, 3 + n_extra) or tuple(sel.shape) != (A, k) or \
                tuple(row.shape) != (A, k) or pts.dtype != torch.float32 or feats.dtype != torch.float32 or sel.dtype != torch.int32 or \
                row.dtype != torch.int32 or not (pts.is_contiguous() and feats.is_contiguous() and sel.is_contiguous() and row.is_contiguous()):
            raise RuntimeError("device_patch_batch: out = (float32 [A, k, 3], float32 [A, k, 3 + c], int32 [A, k], int32 [A, k]), contiguous")
    m = int(np.diff(splits)[act].sum())
    wsb = lib.ml3d_patch_batch_workspace_bytes(m, A, k)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_patch_batch(points.data_ptr(), possibility.data_ptr(), splits.ctypes.data, n_clouds, act.ctypes.data, A,
                                  center_index.data_ptr(), perm.data_ptr(), k, mask, None if extra is None else extra.data_ptr(),
                                  n_extra, float(feat_bias), float(feat_scale), pts.data_ptr(), feats.data_ptr(), sel.data_ptr(),
                                  row.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_patch_batch")
    return pts, feats, sel, row


def sphere_select(points, cloud_row_splits, active, center_index, radius, out=None):
    """The radius query of the sphere sampler (semseg_spatially_regular.py:86-87) for the active clouds of a concatenated set in ONE
    call: per active slot s the cloud-local indices of its points within ``radius`` of ``points[splits[s] + center_index[s]]``,
    ascending (d2, index) -- the row ``fixed_radius_search`` returns for that one query on that cloud alone.  ``points`` float32
    [N, 3], HOST ``cloud_row_splits`` [C + 1] and HOST ``active`` (None: all), ``center_index`` DEVICE int32 [C].  Returns
    (indices int32 [points of the active clouds]: the lists back to back in active order, counts DEVICE int32 [C]: written for the
    active slots only) -- nothing is read back; the counts are the caller's one read-back.  ``out``: the two preallocated."""
    lib = _abi.get()
    _need_gpu(points, center_index)
    splits, act = _host_splits(cloud_row_splits, active, "sphere_select")
    n_clouds = splits.size - 1
    dev = points.device
    m = int(np.diff(splits)[act].sum())
    if not float(radius) >= 0:
        raise RuntimeError("sphere_select: radius >= 0")
    _check_cloud_set("sphere_select", splits, act, 1, points, center_index=center_index)
    if out is None:
        idx = torch.empty(m, dtype=torch.int32, device=dev)
        cnt = torch.empty(n_clouds, dtype=torch.int32, device=dev)
    else:
        idx, cnt = out
        if idx.dtype != torch.int32 or cnt.dtype != torch.int32 or idx.numel() < m or cnt.numel() != n_clouds or \
                not (idx.is_contiguous() and cnt.is_contiguous()):
            raise RuntimeError("sphere_select: out = (int32 [>= points of the active clouds], int32 [C]), contiguous")
        _need_gpu(idx, cnt)
    wsb = lib.ml3d_sphere_select_workspace_bytes(m, act.size)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_sphere_select(points.data_ptr(), splits.ctypes.data, n_clouds, act.ctypes.data, act.size, center_index.data_ptr(),
                                    float(radius), idx.data_ptr(), idx.numel(), cnt.data_ptr(), ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_sphere_select")
    return idx, cnt


def device_sphere_batch(points, possibility, cloud_row_splits, active, center_index, cand, cand_offsets, counts, perm, keep=None,
                        keep_counts=None, zero_extra=None, recenter_dims=(0, 1, 2), extra=None, feat_bias=0.0, feat_scale=1.0,
                        linear=False):
    """One input sphere of each of the A active clouds (the body of the loop of kpconv.py:446-531 after the radius query), nothing
    read back: ``cand`` DEVICE int32 (lists of ``sphere_select``), HOST ``cand_offsets`` [A] / ``counts`` [A] (first entry and
    length n_a of item a's list), ``perm`` DEVICE int32 [sum n_a] (the host's shuffles of 0..n_a-1, concatenated), ``keep`` optional
    DEVICE int32 (the host's ``choice(n_a, m_a, replace=False)`` results of the items with HOST ``keep_counts[a]`` >= 0,
    concatenated; < 0: the item is not cut), HOST ``zero_extra`` [A] flags (the colour drop).  ``possibility`` float64 [N] is bumped
    IN PLACE over all n_a points; with ``linear`` the WHOLE cloud's rows of ``extra`` float32 [N, c] are rescaled IN PLACE
    ((extra - feat_bias) / feat_scale, once per call, like the reference on its cached features).  Returns (points [M, 3]
    recentred on ``recenter_dims``, columns [M, 3 + c], cloud-local indices int32 [M], rows of the concatenated arrays int32 [M],
    HOST output offsets int64 [A + 1]) -- item a's rows are [offsets[a], offsets[a + 1])."""
    lib = _abi.get()
    _need_gpu(points, possibility, center_index, cand, perm)
    splits, act = _host_splits(cloud_row_splits, active, "device_sphere_batch")
    n_clouds, A = splits.size - 1, int(act.size)
    dev = points.device
    offs = np.ascontiguousarray(cand_offsets, dtype=np.int64).reshape(-1)
    n_a = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    n_extra, mask = _check_cloud_set("device_sphere_batch", splits, act, 1, points, possibility, center_index, extra, recenter_dims)
    if cand.dtype != torch.int32 or not cand.is_contiguous() or perm.dtype != torch.int32 or not perm.is_contiguous() or offs.size != A or \
            n_a.size != A or np.any(n_a < 1) or np.any(n_a > np.diff(splits)[act]) or np.any(offs < 0) or \
            np.any(offs + n_a > cand.numel()) or perm.numel() != int(n_a.sum()):
        raise RuntimeError("device_sphere_batch: contiguous int32 candidates holding every item's list, 1 <= n_a <= the cloud's size, "
                           "int32 [sum n_a] shuffles")
    m_a = None
    out_n = n_a.astype(np.int64)
    if keep is not None:
        _need_gpu(keep)
        m_a = np.ascontiguousarray(keep_counts, dtype=np.int32).reshape(-1)
        if keep.dtype != torch.int32 or not keep.is_contiguous() or m_a.size != A or np.any(m_a == 0) or np.any(m_a > n_a) or \
                keep.numel() != int(m_a[m_a > 0].sum()):
            raise RuntimeError("device_sphere_batch: keep = int32 [sum of the m_a >= 1], 1 <= m_a <= n_a (or < 0: no cut)")
        out_n = np.where(m_a > 0, m_a, n_a).astype(np.int64)
    zero = np.zeros(A, np.int32) if zero_extra is None else np.ascontiguousarray(zero_extra).astype(np.int32).reshape(-1)
    if zero.size != A:
        raise RuntimeError("device_sphere_batch: one zero_extra flag per item")
    out_offsets = np.zeros(A + 1, np.int64)
    np.cumsum(out_n, out=out_offsets[1:])
    M = int(out_offsets[-1])
    pts = torch.empty((M, 3), dtype=torch.float32, device=dev)
    cols = torch.empty((M, 3 + n_extra), dtype=torch.float32, device=dev)
    sel = torch.empty(M, dtype=torch.int32, device=dev)
    row = torch.empty(M, dtype=torch.int32, device=dev)
    wsb = lib.ml3d_sphere_batch_workspace_bytes(A, int(n_a.sum()))
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_sphere_batch(points.data_ptr(), possibility.data_ptr(), splits.ctypes.data, n_clouds, act.ctypes.data, A,
                                   center_index.data_ptr(), cand.data_ptr(), offs.ctypes.data, n_a.ctypes.data, perm.data_ptr(),
                                   None if keep is None else keep.data_ptr(), None if m_a is None else m_a.ctypes.data, zero.ctypes.data,
                                   mask, None if extra is None else extra.data_ptr(), n_extra, float(feat_bias), float(feat_scale),
                                   1 if linear else 0, pts.data_ptr(), cols.data_ptr(), sel.data_ptr(), row.data_ptr(), ws.data_ptr(), wsb,
                                   _stream())
    _abi.check(rc, "ml3d_sphere_batch")
    return pts, cols, sel, row, out_offsets


def argmax_labels(scores, out=None):
    """uint8 labels [...] = argmax over the last axis of float32 ``scores`` [..., C <= 256] (first maximum, like
    torch.argmax) -- one pass over the scores instead of torch's generic reduction + dtype cast."""
    lib = _abi.get()
    _need_gpu(scores)
    if scores.dtype != torch.float32 or not scores.is_contiguous() or scores.shape[-1] > 256:
        raise RuntimeError("argmax_labels: contiguous float32 scores with at most 256 classes")
    n = scores.numel() // scores.shape[-1]
    if out is None:
        out = torch.empty(scores.shape[:-1], dtype=torch.uint8, device=scores.device)
    elif out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous():
        raise RuntimeError("argmax_labels: out must be a contiguous uint8 tensor with one entry per point")
    with torch.cuda.device(scores.device):
        rc = lib.ml3d_argmax_labels(scores.data_ptr(), n, int(scores.shape[-1]), out.data_ptr(), _stream())
    _abi.check(rc, "ml3d_argmax_labels")
    return out


def vote_update(test_probs, point_inds, logits, smooth=0.95):
    """In place: ``test_probs[inds] = smooth * test_probs[inds] + (1 - smooth) * softmax(logits)`` on the float16
    vote accumulator [N_cloud, classes] (ml3d/torch/models/randlanet.py:420-421, 457-462).
    ONE batch item per call: every wave does an unsynchronised read-modify-write of its point's row, so the indices of a
    call MUST be unique.  A patch padded with repeated points (cloud smaller than num_points) is de-duplicated by the caller,
    keeping each point's last occurrence = numpy's fancy-assignment result (``RandLANet.update_probs``).  Patches of a batch
    that share points are applied by calling
    this once per item, in order, on one stream -- what ``RandLANet.update_probs`` / ``KPFCNN.update_probs`` do and what
    the reference's sequential loop (randlanet.py:455-463) means."""
    lib = _abi.get()
    _need_gpu(test_probs, point_inds, logits)
    if test_probs.dtype != torch.float16 or not test_probs.is_contiguous() or test_probs.dim() != 2:
        raise RuntimeError("vote_update: test_probs must be a contiguous float16 [N, classes] tensor")
    C_ = test_probs.shape[1]
    lg = logits.reshape(-1, C_).contiguous().float()
    inds = point_inds.reshape(-1).to(torch.int32).contiguous()
    if inds.numel() != lg.shape[0]:
        raise RuntimeError("vote_update: one index per logits row")
    with torch.cuda.device(test_probs.device):
        rc = lib.ml3d_vote_update(lg.data_ptr(), inds.data_ptr(), lg.shape[0], C_, float(smooth), test_probs.data_ptr(),
                                  test_probs.shape[0], _stream())
    _abi.check(rc, "ml3d_vote_update")
    return test_probs


def vote_project(votes, proj_inds, out_labels=None, out_scores=None, scores=True):
    """The finish of a cloud on the device: the float16 vote accumulator ``votes`` [n_sub, C <= 256] taken through ``proj_inds``
    (int32 [n_full], every entry in [0, n_sub) -- the caller's duty, not checked) to the FULL cloud.  Returns
    ``(uint8 [n_full] = np.argmax(votes, 1)[proj_inds]`` -- first maximum, the first NaN wins -- ``, float16 [n_full, C] =
    votes[proj_inds]`` bit for bit, or None with ``scores=False``).  ``votes`` and ``out_scores`` may be row slices of larger
    contiguous buffers: nothing beyond 2-byte alignment is assumed.  One launch (``ml3d_vote_project``)."""
    lib = _abi.get()
    _need_gpu(votes, proj_inds)
    if votes.dtype != torch.float16 or votes.dim() != 2 or not votes.is_contiguous() or not (1 <= votes.shape[1] <= 256):
        raise RuntimeError("vote_project: votes must be a contiguous float16 [n_sub, classes] tensor with 1 <= classes <= 256")
    if proj_inds.dtype != torch.int32 or proj_inds.dim() != 1 or not proj_inds.is_contiguous():
        raise RuntimeError("vote_project: proj_inds must be a contiguous int32 [n_full] tensor")
    n_sub, C_ = int(votes.shape[0]), int(votes.shape[1])
    n_full = int(proj_inds.numel())
    if n_full and not n_sub:
        raise RuntimeError("vote_project: no votes to project")
    dev = votes.device
    if out_labels is None:
        out_labels = torch.empty(n_full, dtype=torch.uint8, device=dev)
    elif out_labels.dtype != torch.uint8 or out_labels.numel() != n_full or not out_labels.is_contiguous():
        raise RuntimeError("vote_project: out_labels must be a contiguous uint8 tensor with one entry per point")
    if not scores:
        out_scores = None
    elif out_scores is None:
        out_scores = torch.empty((n_full, C_), dtype=torch.float16, device=dev)
    elif out_scores.dtype != torch.float16 or tuple(out_scores.shape) != (n_full, C_) or not out_scores.is_contiguous():
        raise RuntimeError("vote_project: out_scores must be a contiguous float16 [n_full, classes] tensor")
    with torch.cuda.device(dev):
        rc = lib.ml3d_vote_project(votes.data_ptr(), n_sub, C_, proj_inds.data_ptr(), n_full, out_labels.data_ptr(),
                                   None if out_scores is None else out_scores.data_ptr(), _stream())
    _abi.check(rc, "ml3d_vote_project")
    return out_labels, out_scores


def label_lut(num_classes, ignored_label_inds):
    """HOST int32 table from a dataset's label VALUE to its row of the confusion matrix, -1 for an ignored value: the table
    ``valid_scores_and_labels`` builds (modules/losses.py:78-85 -- an identity over ``num_classes`` with a zero inserted at every
    ignored index >= 0, in LIST order) with every entry whose index is an ignored value set to -1 afterwards (the points the
    reference drops before it looks the others up).  Length ``num_classes`` + the number of ignored indices >= 0."""
    table = list(range(int(num_classes)))
    ign = [int(i) for i in ignored_label_inds]
    for i in ign:
        if i >= 0:
            table = table[:i] + [0] + table[i:]
    for i in ign:
        if 0 <= i < len(table):
            table[i] = -1
    return np.asarray(table, dtype=np.int32)


def _confusion_args(what, num_classes, n, gt_labels, lut, confusion, counts, dev):
    """The checks and allocations the two confusion ops share, before any device scope.  Returns (HOST lut or None, DEVICE lut or
    None, confusion int64 [C, C], counts int64 [3])."""
    C_ = int(num_classes)
    if gt_labels.dtype != torch.int32 or gt_labels.dim() != 1 or not gt_labels.is_contiguous() or gt_labels.numel() != n:
        raise RuntimeError("%s: invalid argument: gt_labels must be a contiguous int32 [n_full] tensor, one entry per point" % what)
    if n >= 2 ** 31:
        raise RuntimeError("%s: invalid argument: at most 2^31 - 1 points" % what)
    lut_host = lut_dev = None
    if isinstance(lut, torch.Tensor) and lut.device.type != "cpu":
        # a table already on the device (the multi-cloud loops upload theirs once) is NOT read back: its shape is checked here, its
        # values by whoever built it -- the kernel counts an entry >= classes in counts[2] and never writes outside the matrix
        if lut.dtype != torch.int32 or lut.dim() != 1 or lut.numel() < 1 or not lut.is_contiguous() or lut.device != dev:
            raise RuntimeError("%s: invalid argument: a device lut must be a non-empty contiguous int32 [lut_size] tensor on the "
                               "votes' device" % what)
        lut_dev = lut
    elif lut is not None:
        lut_host = np.ascontiguousarray(lut.detach().numpy() if isinstance(lut, torch.Tensor) else lut)
        if lut_host.ndim != 1 or lut_host.size < 1 or lut_host.dtype.kind not in "iu" or int(lut_host.max()) >= C_:
            raise RuntimeError("%s: invalid argument: lut must be a non-empty 1-d integer table with every entry < num_classes "
                               "(negative: ignored)" % what)
        lut_host = lut_host.astype(np.int32)
        lut_dev = torch.from_numpy(lut_host).to(dev)
    if confusion is None:
        confusion = torch.zeros((C_, C_), dtype=torch.int64, device=dev)
    elif confusion.dtype != torch.int64 or tuple(confusion.shape) != (C_, C_) or not confusion.is_contiguous():
        raise RuntimeError("%s: invalid argument: confusion must be a contiguous int64 [classes, classes] tensor" % what)
    if counts is None:
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (3,) or not counts.is_contiguous():
        raise RuntimeError("%s: invalid argument: counts must be a contiguous int64 [3] tensor" % what)
    _need_gpu(gt_labels, confusion, counts)
    if gt_labels.device != dev or confusion.device != dev or counts.device != dev:
        raise RuntimeError("%s: invalid argument: gt_labels, confusion and counts must be on the device of the votes / scores" % what)
    return lut_host, lut_dev, confusion, counts


def vote_confusion(votes, proj_inds, gt_labels, lut=None, confusion=None, counts=None, labels=False):
    """Ground-truth scoring of a finished cloud on the device: filter_valid_label + SemSegMetric.update of the reference's
    ``run_test`` (semantic_segmentation.py:250-257), one launch (``ml3d_vote_confusion``), integer atomics only, deterministic.

    * Prediction: ``pred = np.argmax(votes, 1)[proj_inds]`` -- ``vote_project``'s labels, by the same device function.
      ``proj_inds=None`` is the identity (n_full == n_sub).
    * Ground truth: ``g = gt_labels[i]`` (int32 [n_full], the dataset's label VALUES, on the votes' device).  ``lut[g] >= 0``:
      ``confusion[lut[g], pred] += 1`` and ``counts[0] += 1``.  ``lut[g] < 0`` (ignored): ``counts[1] += 1``.  ``g`` outside the
      table: ``counts[2] += 1``.
    * ``lut``: ``label_lut``'s table as a host array or CPU tensor (every entry < classes, checked), or an int32 tensor already on
      the votes' device, which is used as it is without a read-back of its values.  None: the identity over the classes.
    * ``confusion`` int64 [C, C] (row = truth, column = prediction) and ``counts`` int64 [3], on the votes' device: allocated
      zeroed when None, else ADDED to.
    * ``labels``: True, or the uint8 [n_full] tensor to write: ``pred`` for every point, ignored or not.

    Returns ``(confusion, counts)``, or ``(confusion, counts, labels)`` when labels were asked for."""
    lib = _abi.get()
    _need_gpu(votes, gt_labels)
    if votes.dtype != torch.float16 or votes.dim() != 2 or not votes.is_contiguous() or not (1 <= votes.shape[1] <= 256):
        raise RuntimeError("vote_confusion: invalid argument: votes must be a contiguous float16 [n_sub, classes] tensor with "
                           "1 <= classes <= 256")
    n_sub, C_ = int(votes.shape[0]), int(votes.shape[1])
    if proj_inds is None:
        n_full = n_sub
    else:
        _need_gpu(proj_inds)
        if proj_inds.dtype != torch.int32 or proj_inds.dim() != 1 or not proj_inds.is_contiguous():
            raise RuntimeError("vote_confusion: invalid argument: proj_inds must be a contiguous int32 [n_full] tensor (or None)")
        n_full = int(proj_inds.numel())
        if n_full and not n_sub:
            raise RuntimeError("vote_confusion: invalid argument: no votes to project")
        if proj_inds.device != votes.device:
            raise RuntimeError("vote_confusion: invalid argument: proj_inds must be on the votes' device")
    dev = votes.device
    _, lut_dev, confusion, counts = _confusion_args("vote_confusion", C_, n_full, gt_labels, lut, confusion, counts, dev)
    out_labels = None
    if isinstance(labels, torch.Tensor):
        out_labels = labels
        if out_labels.dtype != torch.uint8 or out_labels.numel() != n_full or not out_labels.is_contiguous():
            raise RuntimeError("vote_confusion: invalid argument: labels must be a contiguous uint8 tensor with one entry per point")
        _need_gpu(out_labels)
        if out_labels.device != dev:
            raise RuntimeError("vote_confusion: invalid argument: labels must be on the votes' device")
    elif labels:
        out_labels = torch.empty(n_full, dtype=torch.uint8, device=dev)
    if n_full == 0:                             # (an empty tensor's address is NULL, which the library reads as "no projection")
        return (confusion, counts) if out_labels is None else (confusion, counts, out_labels)
    with torch.cuda.device(dev):
        rc = lib.ml3d_vote_confusion(votes.data_ptr(), n_sub, C_, None if proj_inds is None else proj_inds.data_ptr(), n_full,
                                     gt_labels.data_ptr(), None if lut_dev is None else lut_dev.data_ptr(),
                                     0 if lut_dev is None else int(lut_dev.numel()), confusion.data_ptr(), counts.data_ptr(),
                                     None if out_labels is None else out_labels.data_ptr(), _stream())
    _abi.check(rc, "ml3d_vote_confusion")
    return (confusion, counts) if out_labels is None else (confusion, counts, out_labels)


def score_confusion(scores, gt_labels, lut=None, confusion=None, counts=None):
    """``vote_confusion`` for float32 ``scores`` [n, C <= 256] (rows may be a column slice of a wider contiguous matrix: row pitch
    ``scores.stride(0)`` >= C, unit column stride): ``pred = argmax`` by ``argmax_labels``' rule.  What ``SemSegMetric.update``
    does with device tensors.  Returns ``(confusion, counts)``."""
    lib = _abi.get()
    _need_gpu(scores, gt_labels)
    if scores.dtype != torch.float32 or scores.dim() != 2 or not (1 <= scores.shape[1] <= 256):
        raise RuntimeError("score_confusion: invalid argument: scores must be a float32 [n, classes] tensor with 1 <= classes <= 256")
    n, C_ = int(scores.shape[0]), int(scores.shape[1])
    ld = C_ if n <= 1 else int(scores.stride(0))
    if (C_ > 1 and scores.stride(1) != 1) or ld < C_:
        raise RuntimeError("score_confusion: invalid argument: scores rows must be contiguous (unit column stride, row pitch >= classes)")
    dev = scores.device
    _, lut_dev, confusion, counts = _confusion_args("score_confusion", C_, n, gt_labels, lut, confusion, counts, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_score_confusion(scores.data_ptr(), ld, n, C_, gt_labels.data_ptr(), None if lut_dev is None else lut_dev.data_ptr(),
                                      0 if lut_dev is None else int(lut_dev.numel()), confusion.data_ptr(), counts.data_ptr(), _stream())
    _abi.check(rc, "ml3d_score_confusion")
    return confusion, counts
