"""SparseConvUnet inference ops (an extension beyond SURVEY.md's scope table): the voxel pyramid with its rulebooks built in one
call, the rulebook convolution on the bf16x3 implicit-GEMM kernel and the BatchNorm + ReLU rows pass, on the HIP kernels of
csrc/sparseconv.hip / csrc/gemm.hip (contract: include/ml3d_hip.h, "SparseConvUnet inference" -- UNPINNED against the open3d
wheel).  Row arguments may be column slices of a wider buffer (unit column stride): their row stride is passed on."""
import numpy as np
import torch

from .. import _abi
from . import _gates
from .gemm import _rows, pack_bf16x3, pad32   # noqa: F401  (re-exported)


def _stream():
    return _gates._stream()


def _need_gpu(*tensors):
    return _gates._need_gpu(*tensors)


class ScnPyramid:
    """What ``ml3d_scn_build`` wrote, every per-level array at the fixed stride of N rows.  ``read_counts()`` is the ONE
    device -> host read of a forward (the vector of level sizes); after it ``level(l)`` hands out the arrays cut to M_l rows."""

    def __init__(self, n, levels, counts, coords, nbr27, child8, parent, ptap, up8, index_map, feat0):
        self.n, self.levels = int(n), int(levels)
        self.counts_dev, self._coords, self._nbr27, self._child8 = counts, coords, nbr27, child8
        self._parent, self._ptap, self._up8 = parent, ptap, up8
        self.index_map, self._feat0 = index_map, feat0
        self.counts = None

    def read_counts(self):
        if self.counts is None:
            self.counts = [int(v) for v in self.counts_dev.cpu().tolist()]
        return self.counts

    def rows(self, l):
        return self.read_counts()[l]

    @property
    def feat0(self):
        return self._feat0[:self.rows(0)]

    def coords(self, l):
        return self._coords[l, :self.rows(l)]

    def nbr27(self, l):
        return self._nbr27[l, :self.rows(l)]

    def child8(self, l):
        """Level l >= 1: the level l - 1 rows of a row's children."""
        return self._child8[l, :self.rows(l)]

    def parent(self, l):
        return self._parent[l, :self.rows(l)]

    def ptap(self, l):
        return self._ptap[l, :self.rows(l)]

    def up8(self, l):
        return self._up8[l, :self.rows(l)]


def scn_build(points, feat, row_splits_host, levels=7, grid_size=4096, feat_pitch=32):
    """``ml3d_scn_build``: ``points`` [N, 3] float32 voxel centres of all items, ``feat`` [N, C <= 4], ``row_splits_host`` the
    host row splits [B + 1] -> ``ScnPyramid`` (level-0 mean features in a zero-padded [N, feat_pitch] buffer).  No host sync."""
    _need_gpu(points, feat)
    lib = _abi.get()
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise RuntimeError("scn_build: points must be contiguous float32 [N, 3]")
    ldf = _rows("scn_build", feat)
    n, c = int(points.shape[0]), int(feat.shape[1])
    rs = np.ascontiguousarray(np.asarray(row_splits_host, np.int64))
    if feat.shape[0] != n or n == 0 or rs.ndim != 1 or rs.size < 2 or rs[0] != 0 or rs[-1] != n or c > 4 or feat_pitch < c:
        raise RuntimeError("scn_build: feat [N, <= 4] and host row splits [0 .. N] expected")
    dev, L = points.device, int(levels)
    i32 = dict(dtype=torch.int32, device=dev)
    counts = torch.empty((L,), **i32)
    coords, nbr27 = torch.empty((L, n, 4), **i32), torch.empty((L, n, 27), **i32)
    child8, up8 = torch.empty((L, n, 8), **i32), torch.empty((L, n, 8), **i32)
    parent, ptap = torch.empty((L, n), **i32), torch.empty((L, n), **i32)
    index_map = torch.empty((n,), **i32)
    feat0 = torch.zeros((n, int(feat_pitch)), dtype=torch.float32, device=dev)
    wsb = int(lib.ml3d_scn_build_workspace_bytes(n, L))
    ws = _gates._ws(wsb, dev)
    with torch.cuda.device(dev):
        rc = lib.ml3d_scn_build(points.data_ptr(), feat.data_ptr(), ldf, c, n, rs.ctypes.data, int(rs.size - 1), L, int(grid_size),
                                counts.data_ptr(), coords.data_ptr(), nbr27.data_ptr(), child8.data_ptr(), parent.data_ptr(),
                                ptap.data_ptr(), up8.data_ptr(), index_map.data_ptr(), feat0.data_ptr(), int(feat_pitch),
                                ws.data_ptr(), wsb, _stream())
    _abi.check(rc, "ml3d_scn_build")
    return ScnPyramid(n, L, counts, coords, nbr27, child8, parent, ptap, up8, index_map, feat0)


def pack_sparse_weights(kernel, cp=None, scale=None, shift=None, extra=None):
    """A ``SparseConv`` / ``SparseConvTranspose`` kernel [kz, ky, kx, Cin, Cout] (or [T, Cin, Cout]) -> (weights
    [T * cp + k2, Cout] float32, bias [Cout] float32 or None, cp, k2): Cin padded to ``cp`` (default: the next multiple of 32)
    by zero rows, a following BatchNorm folded in as float64 ``scale`` / ``shift`` per output channel, and ``extra`` [C2, Cout]
    (a Linear riding in the same GEMM, padded to a multiple of 32 rows) appended."""
    w = kernel.detach().double()
    cin, cout = int(w.shape[-2]), int(w.shape[-1])
    w = w.reshape(-1, cin, cout)
    cp = pad32(cin) if cp is None else int(cp)
    m = torch.zeros((w.shape[0], cp, cout), dtype=torch.float64, device=w.device)
    m[:, :cin] = w
    m = m.reshape(-1, cout)
    k2 = 0
    if extra is not None:
        e = extra.detach().double()
        k2 = pad32(e.shape[0])
        ep = torch.zeros((k2, cout), dtype=torch.float64, device=w.device)
        ep[:e.shape[0]] = e
        m = torch.cat((m, ep), 0)
    bias = None
    if scale is not None:
        m = m * scale.view(1, -1)
        bias = shift.float().contiguous()
    return m.float().contiguous(), bias, cp, k2


def sparse_conv(x, rule, packed, n, cp=None, bias=None, residual=None, a2=None, k2=0, act=0, slope=0.0, out=None):
    """``ml3d_sparse_conv_bf16x3``: ``x`` [rows, >= cp] (may be a column slice), ``rule`` int32 [M, T] contiguous (-1: absent),
    ``packed`` = ``pack_bf16x3`` of the [T * cp + k2, n] weights -> [M, n] (``out`` / ``residual`` / ``a2`` may be column
    slices).  An ineligible problem is an error (the model has no other path)."""
    _need_gpu(x, rule, packed, bias, residual, a2, out)
    lib = _abi.get()
    ldi = _rows("sparse_conv", x)
    cp = int(x.shape[1]) if cp is None else int(cp)
    if rule.dtype != torch.int32 or rule.dim() != 2 or not rule.is_contiguous() or cp > x.shape[1]:
        raise RuntimeError("sparse_conv: contiguous int32 [M, T] rulebook and cp <= the input's columns required")
    m, t, n = int(rule.shape[0]), int(rule.shape[1]), int(n)
    lda2 = 0
    if a2 is not None:
        lda2 = _rows("sparse_conv", a2)
        k2 = int(k2) if k2 else int(a2.shape[1])
        if a2.shape[0] != m or k2 > a2.shape[1]:
            raise RuntimeError("sparse_conv: the dense block needs one row per output row")
    else:
        k2 = 0
    if packed.numel() == 0 or packed.numel() != int(lib.ml3d_gemm_pack_bf16x3_bytes(t * cp + k2, n)):
        raise RuntimeError("sparse_conv: packed weights do not fit [%d * %d + %d, %d]" % (t, cp, k2, n))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    ldc = _rows("sparse_conv", out, n)
    ldr = 0 if residual is None else _rows("sparse_conv", residual, n)
    if out.shape[0] != m or (residual is not None and residual.shape[0] != m):
        raise RuntimeError("sparse_conv: out / residual need one row per output row")
    with torch.cuda.device(x.device):
        rc = lib.ml3d_sparse_conv_bf16x3(x.data_ptr(), ldi, int(x.shape[0]), cp, rule.data_ptr(), t, m,
                                         None if a2 is None else a2.data_ptr(), lda2, k2, packed.data_ptr(), n,
                                         None if bias is None else bias.data_ptr(),
                                         None if residual is None else residual.data_ptr(), ldr, int(act), float(slope),
                                         out.data_ptr(), ldc, _stream())
    _abi.check(rc, "ml3d_sparse_conv_bf16x3")
    return out


def scn_bn_relu(x, scale, shift, out=None):
    """``ml3d_scn_bn_relu``: max(x * scale + shift, 0) on rows; ``x`` / ``out`` may be column slices."""
    _need_gpu(x, scale, shift, out)
    lib = _abi.get()
    ldi = _rows("scn_bn_relu", x)
    m, c = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty((m, c), dtype=torch.float32, device=x.device)
    ldo = _rows("scn_bn_relu", out, c)
    if scale.numel() != c or shift.numel() != c or out.shape[0] != m or scale.dtype != torch.float32 or shift.dtype != torch.float32:
        raise RuntimeError("scn_bn_relu: float32 scale / shift [C] and one output row per input row required")
    with torch.cuda.device(x.device):
        rc = lib.ml3d_scn_bn_relu(x.data_ptr(), ldi, m, c, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), ldo, _stream())
    _abi.check(rc, "ml3d_scn_bn_relu")
    return out


__all__ = ["ScnPyramid", "scn_build", "pack_sparse_weights", "sparse_conv", "scn_bn_relu", "pack_bf16x3", "pad32"]
