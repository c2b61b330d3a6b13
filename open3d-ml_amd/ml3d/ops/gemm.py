"""The shared GEMM's own entry points (csrc/gemm.hip, csrc/gemm_api.hip): weight packing for the bf16x3 kernels and the Linears
on the f32 and the bf16x3 path, plus the two small helpers every caller of them needs (``pad32``, ``_rows``).  The model-specific
ops modules import from here and re-export what they always exported."""
import torch

from .. import _abi
from . import _gates


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def _ws(nbytes, device):
    return _gates._ws(nbytes, device)


def pad32(c):
    """The next multiple of 32: the K granularity of the bf16x3 kernels."""
    return (int(c) + 31) // 32 * 32


def _rows(name, t, cols=None):
    """A float32 [rows, cols] tensor or column slice (unit column stride) -> its row stride."""
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (cols is not None and t.shape[1] != cols):
        raise RuntimeError("%s: float32 rows with unit column stride%s required" %
                           (name, "" if cols is None else " and %d columns" % cols))
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def pack_bf16x3(weights):
    """Split a [K, N] float weight matrix (K % 32 == 0) once into the three bf16 planes `conv2d_nhwc(..., packed=)` multiplies
    with on the bf16 matrix pipe (float32-equivalent result: include/ml3d_hip.h, ml3d_gemm_pack_bf16x3).  Returns a uint8
    tensor, or None when the matrix is not eligible (the caller keeps the f32 kernel)."""
    lib = _abi.get()
    _need_gpu(weights)
    K, N = int(weights.shape[0]), int(weights.shape[1])
    nbytes = int(lib.ml3d_gemm_pack_bf16x3_bytes(K, N))
    if nbytes == 0:
        return None
    w = weights.contiguous()
    packed = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        rc = lib.ml3d_gemm_pack_bf16x3(w.data_ptr(), K, N, packed.data_ptr(), nbytes, _stream())
    _abi.check(rc, "ml3d_gemm_pack_bf16x3")
    return packed


def linear(a, weights_t, bias=None, a2=None, gather=None, residual=None, act=0, slope=0.0, residual_gather=None):
    """act([gather(a) | a2] @ weights_t + bias + residual) — UnaryBlock / decoder step (kpconv.py:1288-1293,
    283-286).  gather: int32 [M, H] neighbour matrix whose FIRST column selects the row of ``a`` (closest_pool).
    residual_gather: int32 [M, H] neighbour matrix whose first column selects the ROW OF ``residual`` added to output row m
    (rows >= residual.shape[0], the shadow index, add nothing)."""
    lib = _abi.get()
    _need_gpu(a, weights_t, bias, a2, gather, residual)
    dev = a.device
    k1 = a.shape[1]
    k2 = 0 if a2 is None else a2.shape[1]
    n = weights_t.shape[1]
    if weights_t.shape[0] != k1 + k2:
        raise RuntimeError("linear: weight rows %d != input columns %d" % (weights_t.shape[0], k1 + k2))
    if gather is not None:
        if gather.dtype != torch.int32 or not gather.is_contiguous():
            raise RuntimeError("linear: gather must be contiguous int32")
        m, gstride = gather.shape[0], gather.shape[1] if gather.dim() == 2 else 1
    else:
        m, gstride = a.shape[0], 0
    for t in (a, weights_t, bias, a2, residual):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("linear: float32 contiguous tensors required")
    rg_stride = 0
    if residual_gather is not None:
        if residual is None or residual_gather.dtype != torch.int32 or not residual_gather.is_contiguous() or \
                residual_gather.shape[0] != m:
            raise RuntimeError("linear: residual_gather must be a contiguous int32 [M, H] matrix next to a residual")
        rg_stride = residual_gather.shape[1] if residual_gather.dim() == 2 else 1
    out = torch.empty((m, n), dtype=torch.float32, device=dev)
    wsb = lib.ml3d_linear_workspace_bytes(m, n, k1 + k2)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_linear(a.data_ptr(), k1, k1, None if gather is None else gather.data_ptr(), gstride, a.shape[0],
                             None if a2 is None else a2.data_ptr(), k2, k2, weights_t.data_ptr(),
                             None if bias is None else bias.data_ptr(),
                             None if residual is None else residual.data_ptr(), n,
                             None if residual_gather is None else residual_gather.data_ptr(), rg_stride,
                             0 if residual is None else residual.shape[0], int(act), float(slope),
                             out.data_ptr(), n, m, n, ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_linear")
    return out


def _linear_bf16x3(name, a, packed, n, bias, act, slope, a2, out, residual, residual_gather):
    """What ``linear_bf16x3`` and ``linear_rows_bf16x3`` share: row strides of every operand (column slices allowed), the
    packed-size check, the split-K workspace and the ABI call -> (rc, out).  ``residual_gather``: int32 [M] or [M, H] whose first
    column selects the row of ``residual``."""
    _need_gpu(a, packed, bias, a2, out, residual, residual_gather)
    lib = _abi.get()
    lda, m, k1, n = _rows(name, a), int(a.shape[0]), int(a.shape[1]), int(n)
    lda2, k2 = (0, 0) if a2 is None else (_rows(name, a2), int(a2.shape[1]))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    ldc = _rows(name, out, n)
    ldr = 0 if residual is None else _rows(name, residual, n)
    want = int(lib.ml3d_gemm_pack_bf16x3_bytes(k1 + k2, n))
    if out.shape[0] != m or (a2 is not None and a2.shape[0] != m) or want == 0 or packed.numel() != want:
        raise RuntimeError("%s: out / packed do not fit a [%d, %d] x [%d, %d] product" % (name, m, k1 + k2, k1 + k2, n))
    gathered = residual_gather is not None
    if gathered and (residual is None or residual_gather.dtype != torch.int32 or not residual_gather.is_contiguous() or
                     residual_gather.dim() not in (1, 2) or residual_gather.shape[0] != m):
        raise RuntimeError("%s: residual_gather must be contiguous int32 [M] or [M, H] next to a residual" % name)
    wsb = int(lib.ml3d_linear_bf16x3_workspace_bytes(m, n, k1 + k2))
    ws = _ws(wsb, a.device)
    lead = (a.data_ptr(), lda, k1, None if a2 is None else a2.data_ptr(), lda2, k2, m, packed.data_ptr(),
            None if bias is None else bias.data_ptr(), None if residual is None else residual.data_ptr(), ldr)
    tail = (n, int(act), float(slope), out.data_ptr(), ldc, ws.data_ptr(), wsb, _stream())
    with torch.cuda.device(a.device):
        if gathered:
            rg_stride = int(residual_gather.shape[1]) if residual_gather.dim() == 2 else 1
            rc = lib.ml3d_linear_bf16x3_gathered(*lead, residual_gather.data_ptr(), rg_stride, int(residual.shape[0]), *tail)
        else:
            rc = lib.ml3d_linear_bf16x3(*lead, *tail)
    return rc, out


def linear_bf16x3(a, packed, n, bias=None, act=0, slope=0.0, a2=None, residual=None, residual_gather=None):
    """act([a | a2] @ W + bias + residual) on the bf16 matrix pipe, `packed` = pack_bf16x3(W [K, n]) (float32-equivalent: pack_bf16x3).
    ``residual_gather``: int32 [M, H] neighbour matrix whose first column selects the ROW of ``residual`` added to output row m
    (rows >= residual.shape[0], the shadow index, add nothing) -- as ``ops.linear``.
    Returns None when the problem is not eligible (block widths % 32, alignment): the caller keeps ops.linear."""
    _need_gpu(a, bias, a2, residual, residual_gather)
    for t in (a, a2, residual):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("linear_bf16x3: float32 contiguous rows required")
    if (a.shape[1] % 32) or (a2 is not None and a2.shape[1] % 32):
        return None
    rc, out = _linear_bf16x3("linear_bf16x3", a, packed, n, bias, act, slope, a2, None, residual, residual_gather)
    if rc == _abi.E_UNSUPPORTED:
        return None
    _abi.check(rc, "ml3d_linear_bf16x3")
    return out


def linear_rows_bf16x3(a, packed, n, bias=None, act=0, slope=0.0, out=None, residual=None, residual_gather=None):
    """``ops.linear_bf16x3`` for rows that are column slices: ``a`` [M, K] (K % 32 == 0) and ``out`` [M, n] may be slices of wider
    buffers; ``residual`` [R, n] contiguous with ``residual_gather`` int32 [M] (row of ``residual`` added to output row m).  An
    ineligible problem is an error here (the model has no other path)."""
    if residual_gather is not None and (residual_gather.dim() != 1 or residual is None or not residual.is_contiguous()):
        raise RuntimeError("linear_rows_bf16x3: residual_gather must be contiguous int32 [M] next to a contiguous residual")
    rc, out = _linear_bf16x3("linear_rows_bf16x3", a, packed, n, bias, act, slope, None, out, residual, residual_gather)
    _abi.check(rc, "ml3d_linear_bf16x3")
    return out


__all__ = ["pack_bf16x3", "pad32", "linear", "linear_bf16x3", "linear_rows_bf16x3"]
