"""PVCNN inference ops (an extension beyond SURVEY.md's scope table): the exact voxel coordinates, the deterministic
scatter-mean onto a channels-last grid, the 3 x 3 x 3 convolution on the bf16x3 implicit-GEMM kernel, the trilinear gather and
the per-item column maximum on the HIP kernels of csrc/pvcnn.hip / csrc/gemm.hip (contracts: include/ml3d_hip.h, "PVCNN
inference").  Row arguments may be column slices of a wider buffer (unit column stride): their row stride is passed on."""
import numpy as np
import torch

from .. import _abi
from . import _gates
from .gemm import _rows, linear_rows_bf16x3, pack_bf16x3, pad32   # noqa: F401  (re-exported)


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


def pvcnn_voxel_coords(coords, resolutions):
    """The normalisation of ``Voxelization.forward`` (pvcnn.py:653-662) under the exact contract of
    ``ml3d_pvcnn_voxel_coords``: ``coords`` [B, 3, N] -> (stats [B, 4] = mean x, y, z and scale,
    {r: (v float32 [B * N, 3], flat voxel index int32 [B * N])}) for every r of ``resolutions``."""
    _need_gpu(coords)
    lib = _abi.get()
    if coords.dtype != torch.float32 or coords.dim() != 3 or coords.shape[1] != 3 or not coords.is_contiguous():
        raise RuntimeError("pvcnn_voxel_coords: coords must be contiguous float32 [B, 3, N]")
    res = sorted(set(int(r) for r in resolutions))
    B, _, N = coords.shape
    dev = coords.device
    stats = torch.empty((B, 4), dtype=torch.float32, device=dev)
    out = {r: (torch.empty((B * N, 3), dtype=torch.float32, device=dev), torch.empty((B * N,), dtype=torch.int32, device=dev))
           for r in res}
    rh = np.asarray(res, np.int32)
    vt = _abi.ptr_table([out[r][0].data_ptr() for r in res])
    it = _abi.ptr_table([out[r][1].data_ptr() for r in res])
    with torch.cuda.device(dev):
        rc = lib.ml3d_pvcnn_voxel_coords(coords.data_ptr(), B, N, rh.ctypes.data, len(res), stats.data_ptr(), vt, it, _stream())
    _abi.check(rc, "ml3d_pvcnn_voxel_coords")
    return stats, out


def avg_voxelize(feat, vox_index, batch, r, out_channels=None):
    """``avg_voxelize`` (pvcnn.py:579-619) on rows: ``feat`` [B * N, C] (may be a column slice), ``vox_index`` int32 [B * N] ->
    channels-last grid [B, r, r, r, out_channels or C]; columns past C and empty cells are zero.  Deterministic."""
    _need_gpu(feat, vox_index)
    lib = _abi.get()
    ldf = _rows("avg_voxelize", feat)
    if vox_index.dtype != torch.int32 or not vox_index.is_contiguous() or vox_index.numel() != feat.shape[0] or feat.shape[0] % batch:
        raise RuntimeError("avg_voxelize: vox_index must be contiguous int32 [B * N]")
    n, c = feat.shape[0] // batch, int(feat.shape[1])
    cg = c if out_channels is None else int(out_channels)
    grid = torch.empty((batch, r, r, r, cg), dtype=torch.float32, device=feat.device)
    wsb = int(lib.ml3d_avg_voxelize_workspace_bytes(batch, n))
    ws = _gates._ws(wsb, feat.device)
    with torch.cuda.device(feat.device):
        rc = lib.ml3d_avg_voxelize(feat.data_ptr(), ldf, c, vox_index.data_ptr(), batch, n, int(r), grid.data_ptr(), cg,
                                   ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_avg_voxelize")
    return grid


def pack_conv3d_weights(weight, scale=None, shift=None, bias=None):
    """The reference's ``Conv3d.weight`` [cout, cin, 3, 3, 3] (+ ``bias``, + a BatchNorm as float64 ``scale`` / ``shift``) ->
    (weights [27 * cin_pad, cout] float32 with cin padded to a multiple of 32 by zero rows, bias [cout], cin_pad)."""
    w = weight.detach().double()
    cout, cin = int(w.shape[0]), int(w.shape[1])
    b = torch.zeros(cout, dtype=torch.float64, device=w.device) if bias is None else bias.detach().double()
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1, 1)
        b = b * scale + shift
    cp = pad32(cin)
    m = torch.zeros((27, cp, cout), dtype=torch.float64, device=w.device)
    m[:, :cin] = w.permute(2, 3, 4, 1, 0).reshape(27, cin, cout)
    return m.reshape(27 * cp, cout).float().contiguous(), b.float().contiguous(), cp


def conv3d_ndhwc(x, packed, bias, cout, act=1, slope=0.1):
    """3 x 3 x 3 / stride 1 / pad 1 convolution + bias + activation on a channels-last volume [B, D, H, W, cin] (cin % 32 == 0);
    ``packed`` = ``pack_bf16x3`` of the [27 * cin, cout] weights of ``pack_conv3d_weights``.  float32-equivalent (bf16x3)."""
    _need_gpu(x, packed, bias)
    lib = _abi.get()
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous():
        raise RuntimeError("conv3d_ndhwc: contiguous float32 [B, D, H, W, C] volume required")
    B, D, H, W, cin = x.shape
    want = int(lib.ml3d_gemm_pack_bf16x3_bytes(27 * cin, int(cout)))
    if want == 0 or packed.numel() != want:
        raise RuntimeError("conv3d_ndhwc: packed weights do not fit cin = %d, cout = %d (cin must be a multiple of 32)" % (cin, cout))
    out = torch.empty((B, D, H, W, int(cout)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.ml3d_conv3d_ndhwc_bf16x3(x.data_ptr(), B, D, H, W, cin, packed.data_ptr(), None if bias is None else bias.data_ptr(),
                                          int(act), float(slope), int(cout), out.data_ptr(), int(cout), _stream())
    _abi.check(rc, "ml3d_conv3d_ndhwc_bf16x3")
    return out


def trilinear_devoxelize(grid, v, addend=None, out=None):
    """Contract (d) of ``ml3d_trilinear_devoxelize``: ``grid`` [B, r, r, r, C] channels-last, ``v`` [B * N, 3] -> [B * N, C]
    (+ ``addend``); ``out`` / ``addend`` may be column slices of a wider buffer, and the same slice."""
    _need_gpu(grid, v, addend, out)
    lib = _abi.get()
    if grid.dtype != torch.float32 or grid.dim() != 5 or not grid.is_contiguous() or grid.shape[1] != grid.shape[2] or \
            grid.shape[2] != grid.shape[3]:
        raise RuntimeError("trilinear_devoxelize: contiguous float32 [B, r, r, r, C] grid required")
    B, r, c = int(grid.shape[0]), int(grid.shape[1]), int(grid.shape[4])
    if v.dtype != torch.float32 or not v.is_contiguous() or v.dim() != 2 or v.shape[1] != 3 or v.shape[0] % B:
        raise RuntimeError("trilinear_devoxelize: v must be contiguous float32 [B * N, 3]")
    rows = int(v.shape[0])
    if out is None:
        out = torch.empty((rows, c), dtype=torch.float32, device=grid.device)
    ldc = _rows("trilinear_devoxelize", out, c)
    lda = 0 if addend is None else _rows("trilinear_devoxelize", addend, c)
    if out.shape[0] != rows or (addend is not None and addend.shape[0] != rows):
        raise RuntimeError("trilinear_devoxelize: out / addend need one row per point")
    with torch.cuda.device(grid.device):
        rc = lib.ml3d_trilinear_devoxelize(grid.data_ptr(), c, r, c, v.data_ptr(), B, rows // B,
                                           None if addend is None else addend.data_ptr(), lda, out.data_ptr(), ldc, _stream())
    _abi.check(rc, "ml3d_trilinear_devoxelize")
    return out


def segment_max_rows(x, batch):
    """``feat.max(dim=-1)`` (pvcnn.py:156) on rows: ``x`` [B * N, C] (may be a column slice) -> [B, C]."""
    _need_gpu(x)
    lib = _abi.get()
    ldx = _rows("segment_max_rows", x)
    if x.shape[0] % batch:
        raise RuntimeError("segment_max_rows: rows must be a multiple of the batch size")
    n, c = x.shape[0] // batch, int(x.shape[1])
    out = torch.empty((batch, c), dtype=torch.float32, device=x.device)
    wsb = int(lib.ml3d_segment_max_rows_workspace_bytes(batch, n, c))
    ws = _gates._ws(wsb, x.device)
    with torch.cuda.device(x.device):
        rc = lib.ml3d_segment_max_rows(x.data_ptr(), ldx, batch, n, c, out.data_ptr(), c, ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_segment_max_rows")
    return out


__all__ = ["pvcnn_voxel_coords", "avg_voxelize", "pack_conv3d_weights", "conv3d_ndhwc", "trilinear_devoxelize", "segment_max_rows",
           "linear_rows_bf16x3", "pack_bf16x3", "pad32"]
