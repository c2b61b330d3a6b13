"""Shared bodies and shape tables of the TRAINING op tests (csrc/train.hip and the four differentiable entry points at the end of
csrc/randla.hip): tests/test_emulated_training_ops.py runs them on CPU tensors against the host emulation,
tests/test_gpu_training_ops.py on the MI355X, tests/test_train_cases_can_fail.py against deliberately wrong float64 stand-ins.  Every
body takes ``(dev, case, impl=None, report=_print)``; ``impl=None`` = ``Product``, which drives ``ml3d.ops`` and -- where the wrappers
cannot express a call (strided ``gemm_tn``, strided gathers, null ``gamma`` / ``beta`` gradients, a workspace full of NaN bytes) -- the
C entry points through ``ml3d._abi.get()`` with ``tensor.data_ptr()``.  ``Product`` fills every output buffer with ``SENTINEL`` first:
host-side zeroing and "untouched" padding are part of what is compared.

Floats are judged by ``pt_cases.judge``: against the formulas of tests/train_ref.py in FLOAT64, within max(1e-5, 4 e32), e32 the
distance of the same formulas in float32 from float64 at the case's own inputs.  Inputs are scaled by a power of two so that the
largest float64 output of a call lies in [0.5, 20] (``TARGET``): the 1e-5 floor then means the same everywhere.  Gather and max
forwards, repeated calls of everything without float atomics, and sentinel padding are compared for EQUALITY.

DISCONTINUITIES: float32 and float64 must take the same branch, or e32 means nothing.  Each body asserts on the float64 reference
that every LeakyReLU input is at least 1e-3 from 0, every deformed influence at least 1e-4 from the clamp, every minimum of the
regulariser 1e-3 ahead of the runner-up or tied EXACTLY; maxima are taken over small integers, whose ties are exact in both types.

DISPATCH: ``gemm_plan`` / ``reduce_blocks`` / ``tr_blocks`` / ``attn_plan`` / ``attn_check`` restate the host rules of train.hip next to
their constants; ``RULE_TEXT`` pins each to the source text; ``arms_table`` names, for every kernel of ``REQUIRED_ARMS``, the cases
that reach it.  tests/test_train_cases_can_fail.py asserts all three before anything runs."""
import os
import re

import numpy as np
import torch

import train_ref as R
from kp_cases import EXTENT, SHADOWS, TARGET, geometry, neighbour_rows
from pt_cases import _print, f32, judge, refused, same_bits

F64, F32 = torch.float64, torch.float32
SENTINEL = -77.25
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BIG = 2 ** 31 - 1

GEMM_KN = (1, 31, 32, 33, 64, 65, 97, 130)
GEMM_M = (0, 1, 2, 3, 127, 128, 129, 257, 1000)
GEMM_M_SHAPES = ((33, 65), (130, 97))
GEMM_BY_TILES = dict(m=65665, k=65, n=65)                 # 4 tiles: 512 slices by 2048 / tiles, 514 by rows
BN_C = (1, 5, 64, 96, 255, 256, 257, 340, 512, 1024)
BN_ROWS = (2, 3, 7, 255, 257, 1000)
BN_ROWS_C = (5, 96, 340)
BN_SLOPES = (None, 0.2, 0.0)
BN_CAP = dict(rows=87400, c=48)                           # 4 195 200 elements > 4096 * 1024
GATHER_C = (1, 3, 48, 130)
GATHER_H = (1, 5)
GATHER_CAP = dict(nq=1100000, c=3, h=2, n=4001)           # 3 300 000 elements > 8192 * 256
ATTN_SHAPES = ((1, 1), (3, 3), (8, 8), (6, 10), (9, 9), (32, 32), (40, 56), (64, 64), (100, 30), (128, 128), (160, 96), (96, 160))
ATTN_ROWS = ((1, 1), (2, 1), (1, 3), (2, 2), (1, 5), (1, 33), (2, 32), (1, 65))       # (B, N): B N = 1, 2, 3, 4, 5, 33, 64, 65
ATTN_ROWS_SHAPES = ((3, 3), (9, 9), (40, 56), (160, 96))   # one per backward class
ATTN_THREE_LEVELS = dict(b=1, n=2050, c1=9, c2=9)         # 1025 groups, 33 chunks
ATTN_MEMORY_CAP = dict(b=1, n=1282, c1=160, c2=96)        # 641 tiles on 640 groups: group 0 reloads its private partial
ATTN_MORE_TILES = dict(b=2, n=4099, c1=3, c2=3)           # 2050 tiles on 2048 groups (d <= 16)
DEFORM_CIN = (1, 8, 63, 64, 65, 128, 200)
DEFORM_H = (0, 1, 5, 37)
DEFORM_NQ = (0, 1, 3, 4, 5, 33)
REG_K = (1, 6, 15, 16)
REG_NQ = (1, 15, 16, 17, 33)
REG_H = (0, 1, 14)
GMAX_C = (1, 6, 130)
GMAX_N_IN = 9
APOOL_K = (1, 2, 16, 31, 32)
APOOL_C = (1, 5, 64)
APOOL_ROWS = (1, 11, 257)


def _pow2(largest, target=TARGET):
    return float(2.0 ** np.round(np.log2(target / largest))) if largest > 0 and np.isfinite(largest) else 1.0


def _amax(*ts):
    return max([float(t.abs().max()) for t in ts if t is not None and t.numel()] or [0.0])


def _in_range(*ts):
    m = _amax(*ts)
    assert 0.5 <= m <= 20, m


def _shadowed(rng, idx, n, share=0.3):
    """``share`` of the entries of ``idx`` replaced by a shadow, spelt -1, n or 2^31 - 1."""
    hole = np.array((-1, n, BIG), np.int64)[rng.integers(0, 3, idx.shape)]
    return np.where(rng.random(idx.shape) < share, hole, idx)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))


# ---- the product behind the bodies -------------------------------------------------------------------------------------------------------
class Product:
    """``ml3d.ops`` and the C entry points on ``dev``: CPU tensors in, CPU tensors out, every output buffer prefilled with SENTINEL."""

    def __init__(self, dev):
        from ml3d import _abi, ops
        from ml3d.ops import _gates
        self.dev, self.ops, self.abi, self.lib, self.gates = dev, ops, _abi, _abi.get(), _gates

    def _to(self, t):
        return None if t is None else t.detach().contiguous().to(self.dev, copy=True)     # (a copy: the bodies keep their inputs)

    def _buf(self, *shape):
        return torch.full(shape, SENTINEL, dtype=F32, device=self.dev)

    def _ws(self, nbytes, fill=0xFF):
        return torch.full((int(nbytes) + 16,), fill, dtype=torch.uint8, device=self.dev)

    @staticmethod
    def _p(t):
        return None if t is None or t.numel() == 0 else t.data_ptr()

    def _call(self, name, *args):
        with torch.cuda.device(self.dev):
            rc = getattr(self.lib, name)(*args, self.gates._stream())
        self.abi.check(rc, name)

    def gemm_tn(self, a, b, k, n, ldc, col_sums):
        """a [m, lda], b [m, ldb] (the first k / n columns count) -> (C [k, ldc], column sums of a [k] or None)."""
        a, b = self._to(a), self._to(b)
        c, s = self._buf(k, ldc), self._buf(k) if col_sums else None
        self._call("ml3d_gemm_tn", self._p(a), a.shape[1], self._p(b), b.shape[1], a.shape[0], k, n, c.data_ptr(), ldc, self._p(s))
        if a.shape[1] == k and b.shape[1] == n and ldc == n and a.shape[0]:       # the wrapper, where it can express the call
            c2 = self.ops.gemm_tn(a, b, with_col_sums=col_sums)
            assert tuple((c2[0] if col_sums else c2).shape) == (k, n)
        return c.cpu(), None if s is None else s.cpu()

    def bn_forward(self, x, gamma, beta, eps, slope, workspace_bytes=None, rows=None):
        x, gamma, beta = self._to(x), self._to(gamma), self._to(beta)
        r, c = x.shape
        y, mean, var, invstd = self._buf(r, c), self._buf(c), self._buf(c), self._buf(c)
        wsb = self.lib.ml3d_batchnorm_train_workspace_bytes(c)
        ws = self._ws(wsb)
        self._call("ml3d_batchnorm_train_forward", self._p(x), r if rows is None else rows, c, self._p(gamma), self._p(beta), eps,
                   0 if slope is None else 1, float(slope or 0.0), y.data_ptr(), mean.data_ptr(), var.data_ptr(), invstd.data_ptr(),
                   ws.data_ptr(), wsb if workspace_bytes is None else workspace_bytes)
        return y.cpu(), mean.cpu(), var.cpu(), invstd.cpu()

    def bn_backward(self, x, y, gy, gamma, beta, mean, invstd, eps, slope):
        """-> (gx, ggamma, gbeta); a null ``gamma`` / ``beta`` passes a NULL gradient pointer (its result is then None)."""
        x, y, gy, gamma, mean, invstd = (self._to(t) for t in (x, y, gy, gamma, mean, invstd))
        r, c = x.shape
        gx = self._buf(r, c)
        gg, gb = None if gamma is None else self._buf(c), None if beta is None else self._buf(c)
        wsb = self.lib.ml3d_batchnorm_train_workspace_bytes(c)
        ws = self._ws(wsb)
        self._call("ml3d_batchnorm_train_backward", x.data_ptr(), y.data_ptr(), gy.data_ptr(), r, c, self._p(gamma), mean.data_ptr(),
                   invstd.data_ptr(), 0 if slope is None else 1, float(slope or 0.0), gx.data_ptr(), self._p(gg), self._p(gb),
                   ws.data_ptr(), wsb)
        return gx.cpu(), None if gg is None else gg.cpu(), None if gb is None else gb.cpu()

    def bn_function(self, x, gamma, beta, rm, rv, momentum, eps, slope, gy):
        """``ops.BatchNormActFunction`` -> (y, gx, ggamma, gbeta, running mean, running variance)."""
        x = self._to(x).requires_grad_(True)
        gamma = None if gamma is None else self._to(gamma).requires_grad_(True)
        beta = None if beta is None else self._to(beta).requires_grad_(True)
        rm, rv = self._to(rm).clone(), self._to(rv).clone()
        y = self.ops.BatchNormActFunction.apply(x, gamma, beta, rm, rv, momentum, eps, slope)
        y.backward(self._to(gy))
        g = lambda t: None if t is None else t.grad.cpu()
        return y.detach().cpu(), g(x), g(gamma), g(beta), rm.cpu(), rv.cpu()

    def gather_rows(self, x, idx, stride, m):
        x, idx = self._to(x), self._to(idx)
        out = self._buf(m, x.shape[1])
        self._call("ml3d_gather_rows", self._p(x), x.shape[0], x.shape[1], self._p(idx), stride, m, self._p(out))
        if stride == 1 and m and x.shape[0]:
            assert same_bits(self.ops.GatherRowsFunction.apply(x, idx.reshape(-1)[:m].contiguous()), out), "GatherRowsFunction"
        return out.cpu()

    def scatter_add_rows(self, g, n_src, idx, stride, m):
        g, idx = self._to(g), self._to(idx)
        gx = self._buf(n_src, g.shape[1])
        self._call("ml3d_scatter_add_rows", self._p(g), n_src, g.shape[1], self._p(idx), stride, m, self._p(gx))
        return gx.cpu()

    def pool_forward(self, x, inds, mode):
        return self.ops.GatherPoolFunction.apply(self._to(x), self._to(inds), mode).cpu()

    def pool_backward(self, x, inds, mode, g):
        x, inds, g = self._to(x), self._to(inds), self._to(g)
        gx = self._buf(*x.shape)
        self._call("ml3d_gather_pool_backward", self._p(x), x.shape[0], x.shape[1], self._p(inds), inds.shape[0], inds.shape[1],
                   0 if mode == "max" else 1, self._p(g), self._p(gx))
        return gx.cpu()

    def attention_forward(self, f, enc, idx, w, bias):
        f, enc, idx, w, bias = (self._to(t) for t in (f, enc, idx, w, bias))
        B, n, c1 = f.shape
        c2 = enc.shape[3]
        out = self._buf(B, n, c1 + c2)
        wt = w.t().contiguous()
        self._call("ml3d_randla_attention_stage", f.data_ptr(), enc.data_ptr(), idx.data_ptr(), wt.data_ptr(), self._p(bias), B, n, 16, c1, c2,
                   out.data_ptr())
        return out.cpu()

    def attention_backward(self, f, enc, idx, w, bias, out, g, through_function=True):
        """-> (gf, genc, gw, gbias): the C entry with a workspace of NaN bytes; ``ops.AttentionStageFunction`` must give the same
        ``out``, ``genc`` and ``gw`` (the three are deterministic) bit for bit."""
        f, enc, idx, w, bias, out, g = (self._to(t) for t in (f, enc, idx, w, bias, out, g))
        B, n, c1 = f.shape
        c2 = enc.shape[3]
        d = c1 + c2
        gf, genc, gw, gb = self._buf(B, n, c1), self._buf(B, n, 16, c2), self._buf(d, d), None if bias is None else self._buf(d)
        wsb = self.lib.ml3d_randla_attention_stage_backward_workspace_bytes(B, n, c1, c2)
        ws = self._ws(wsb)
        wt = w.t().contiguous()
        self._call("ml3d_randla_attention_stage_backward", f.data_ptr(), enc.data_ptr(), idx.data_ptr(), w.data_ptr(), wt.data_ptr(),
                   self._p(bias), out.data_ptr(), g.data_ptr(), B, n, 16, c1, c2, gf.data_ptr(), genc.data_ptr(), gw.data_ptr(), self._p(gb),
                   ws.data_ptr(), wsb)
        if through_function:
            assert self.ops.attention_stage_supported(16, c1, c2, B * n)
            fr, er, wr = f.clone().requires_grad_(True), enc.clone().requires_grad_(True), w.clone().requires_grad_(True)
            br = None if bias is None else bias.clone().requires_grad_(True)
            o2 = self.ops.AttentionStageFunction.apply(fr, er, idx, wr, br)
            o2.backward(g)
            assert same_bits(o2, out) and same_bits(er.grad, genc) and same_bits(wr.grad, gw), "AttentionStageFunction"
            assert tuple(fr.grad.shape) == (B, n, c1) and (br is None or tuple(br.grad.shape) == (d,))
        return gf.cpu(), genc.cpu(), gw.cpu(), None if gb is None else gb.cpu()

    def deformed(self, x, dkp, q, s, inds, extent, dwf):
        """``ops.KPConvDeformedFunction`` -> (wf [nq, K cin], dx, gkp)."""
        x, dkp = self._to(x).requires_grad_(True), self._to(dkp).requires_grad_(True)
        wf = self.ops.KPConvDeformedFunction.apply(x, dkp, self._to(q), self._to(s), self._to(inds), extent)
        wf.backward(self._to(dwf).reshape(wf.shape))
        return wf.detach().cpu(), x.grad.cpu(), dkp.grad.cpu()

    def regulariser(self, dkp, q, s, inds, extent, repulse):
        """``ops.OffsetRegulariserFunction`` -> dict(fit, rep, min_d2, gfit, grep): the gradients of the two SUMS over (q, k)."""
        dkp = self._to(dkp).requires_grad_(True)
        terms, min_d2 = self.ops.OffsetRegulariserFunction.apply(dkp, self._to(q), self._to(s), self._to(inds), extent, repulse)
        denom = float(max(dkp.shape[0] * dkp.shape[1], 1))
        one = lambda i: torch.autograd.grad(terms, dkp, torch.tensor([denom * (i == 0), denom * (i == 1)], dtype=F32, device=self.dev),
                                            retain_graph=True)[0].cpu()
        return dict(fit=terms[0].detach().cpu(), rep=terms[1].detach().cpu(), min_d2=min_d2.cpu(), gfit=one(0), grep=one(1))

    def gather_max(self, feat, idx, n_out, g):
        """``ops.GatherMaxFunction`` -> (out, gfeat)."""
        feat = self._to(feat).requires_grad_(True)
        out = self.ops.GatherMaxFunction.apply(feat, self._to(idx), n_out)
        out.backward(self._to(g))
        return out.detach().cpu(), feat.grad.cpu()

    def attentive_pool(self, scores, x, g):
        """``ops.AttentivePoolFunction`` -> (out, gscores, gx)."""
        scores, x = self._to(scores).requires_grad_(True), self._to(x).requires_grad_(True)
        out = self.ops.AttentivePoolFunction.apply(scores, x)
        out.backward(self._to(g))
        return out.detach().cpu(), scores.grad.cpu(), x.grad.cpu()


def _impl(dev, impl):
    return Product(dev) if impl is None else impl


# ---- gemm_tn ---------------------------------------------------------------------------------------------------------------------------
def check_gemm(dev, m, k, n, strided=False, col_sums=True, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    rng = np.random.default_rng([m, k, n, int(strided)])
    lda, ldb, ldc = (k + 3, n + 1, n + 2) if strided else (k, n, n)
    a, b = f32(rng.standard_normal((m, lda))), f32(rng.standard_normal((m, ldb)))
    r64, s64 = R.gemm_tn(a[:, :k], b[:, :n], F64)
    a = a * _pow2(_amax(r64, s64))
    r64, s64 = R.gemm_tn(a[:, :k], b[:, :n], F64)
    r32, s32 = R.gemm_tn(a[:, :k], b[:, :n], F32)
    name = "gemm_tn m=%d k=%d n=%d%s%s" % (m, k, n, " strided" if strided else "", " sums" if col_sums else "")
    if product:
        report(name=name, arm="gemm_tn_k slices=%d rows_per_slice=%d" % gemm_plan(m, k, n)[:2] if m else "zeroed by the host")
    c, s = impl.gemm_tn(a, b, k, n, ldc, col_sums)
    assert tuple(c.shape) == (k, ldc) and bool((c[:, n:] == SENTINEL).all()), (name, "the padding columns of C")
    judge(report, name, c[:, :n].contiguous(), r64, r32)
    if col_sums:
        judge(report, name + " column sums", s, s64, s32)
    if m:
        _in_range(r64, s64)
    else:
        assert not bool(c[:, :n].any()) and (s is None or not bool(s.any())), (name, "m = 0 zeroes C and the sums")


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------
def bn_inputs(rows, c, slope, gamma, beta):
    """x [rows, c] (rows of a short batch well apart), gamma (a fifth negative), beta, gy; with an activation, every pre-activation
    value of the float64 formula at least 1e-3 from 0 (entries of x and beta are nudged until that holds)."""
    rng = np.random.default_rng([rows, c, int(gamma), int(beta), 0 if slope is None else 1 + int(slope * 10)])
    x = rng.standard_normal((rows, c)) * 2 + 1
    if rows <= 7:
        x = x * 0.3 + 1.5 * rng.permuted(np.tile(np.arange(rows)[:, None], (1, c)), axis=0)
    x = f32(x)
    gam = f32(rng.uniform(0.5, 1.5, c) * np.where(rng.random(c) < 0.2, -1, 1)) if gamma else None
    bet = f32(rng.normal(0, 0.5, c)) if beta else None
    for _ in range(40):
        if slope is None:
            break
        v = R.bn_forward(x, gam, bet, BN_EPS, slope, F64)[1]
        near = v.abs() < 1e-3
        if not bool(near.any()):
            break
        x = x + near.float() * f32(rng.choice((-0.05, 0.05), (rows, c)))
        if bet is not None and rows <= 3:                  # (two or three rows: xhat is the same whatever x is)
            bet = bet + near.any(0).float() * 0.01
    gy = f32(rng.standard_normal((rows, c)))
    return x, gam, bet, gy


def _bn_refs(x, gam, bet, gy, slope):
    out = []
    for t in (F64, F32):
        y, v, mean, var, invstd = R.bn_forward(x, gam, bet, BN_EPS, slope, t)
        out.append(dict(y=y, v=v, mean=mean, var=var, invstd=invstd, grads=R.bn_backward(x, gy, gam, bet, BN_EPS, slope, t)))
    return out


def check_bn(dev, rows, c, slope=0.2, gamma=True, beta=True, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    x, gam, bet, gy = bn_inputs(rows, c, slope, gamma, beta)
    r64, r32 = _bn_refs(x, gam, bet, gy, slope)
    gy = gy * _pow2(_amax(*r64["grads"]))
    r64, r32 = _bn_refs(x, gam, bet, gy, slope)
    if slope is not None:
        assert float(r64["v"].abs().min()) >= 1e-3, "a pre-activation value too close to 0"
        assert bool((r64["v"] > 0).any()) and bool((r64["v"] < 0).any())
    name = "bn rows=%d c=%d slope=%s gamma=%d beta=%d" % (rows, c, slope, gamma, beta)
    if product:
        report(name=name, arm="col_reduce_k<1|2> blocks=%d bn_apply_k blocks=%d" % (reduce_blocks(rows, c), tr_blocks(rows * c, 1024, BN_APPLY_CAP)))
    y, mean, var, invstd = impl.bn_forward(x, gam, bet, BN_EPS, slope)
    judge(report, name + " y", y, r64["y"], r32["y"])
    for key, got in (("mean", mean), ("var", var), ("invstd", invstd)):
        judge(report, name + " " + key, got, r64[key], r32[key])
    _in_range(r64["y"])
    gx, gg, gb = impl.bn_backward(x, y, gy, gam, bet, mean, invstd, BN_EPS, slope)
    judge(report, name + " gx", gx, r64["grads"][0], r32["grads"][0])
    assert (gg is None) == (gam is None) and (gb is None) == (bet is None)
    if gg is not None:
        judge(report, name + " ggamma", gg, r64["grads"][1], r32["grads"][1])
    if gb is not None:
        judge(report, name + " gbeta", gb, r64["grads"][2], r32["grads"][2])
    _in_range(*r64["grads"])


def check_bn_function(dev, rows, c, slope=0.2, gamma=True, beta=True, impl=None, report=_print):
    """Through ``ops.BatchNormActFunction``: the output, the three gradients and the running buffers (momentum, the UNBIASED variance)."""
    product = impl is None
    impl = _impl(dev, impl)
    x, gam, bet, gy = bn_inputs(rows, c, slope, gamma, beta)
    rng = np.random.default_rng([rows, c, 9])
    rm, rv = f32(rng.standard_normal(c)), f32(rng.random(c) + 0.5)
    r64, r32 = _bn_refs(x, gam, bet, gy, slope)
    gy = gy * _pow2(_amax(*r64["grads"]))
    r64, r32 = _bn_refs(x, gam, bet, gy, slope)
    name = "bn function rows=%d c=%d slope=%s gamma=%d beta=%d" % (rows, c, slope, gamma, beta)
    if product:
        report(name=name, arm="BatchNormActFunction col_reduce_k<1|2> blocks=%d" % reduce_blocks(rows, c))
    y, gx, gg, gb, rm2, rv2 = impl.bn_function(x, gam, bet, rm, rv, BN_MOMENTUM, BN_EPS, slope, gy)
    judge(report, name + " y", y, r64["y"], r32["y"])
    judge(report, name + " gx", gx, r64["grads"][0], r32["grads"][0])
    if gamma:
        judge(report, name + " ggamma", gg, r64["grads"][1], r32["grads"][1])
    if beta:
        judge(report, name + " gbeta", gb, r64["grads"][2], r32["grads"][2])
    run64 = R.running_update(rm, rv, r64["mean"], r64["var"], rows, BN_MOMENTUM, F64)
    run32 = R.running_update(rm, rv, r32["mean"], r32["var"], rows, BN_MOMENTUM, F32)
    judge(report, name + " running mean", rm2, run64[0], run32[0])
    judge(report, name + " running var", rv2, run64[1], run32[1])


# ---- gathers and their adjoints ----------------------------------------------------------------------------------------------------------
GATHER_N, GATHER_NQ = 37, 23
TIED, ZERO_ROW, NEGATIVE = (10, 11), 12, 6                # two identical rows; a row of zeros; the first NEGATIVE rows are all negative


def gather_inputs(c, h, nq=GATHER_NQ, n=GATHER_N):
    """Integer-valued features [n, c] (ties are exact) and inds [nq, h] of real, duplicate and shadow (n, n + 5, -1, 2^31 - 1) entries;
    with h >= 3: row 0 lists the two identical rows first, row 1 a shadow BEFORE the zero row, row 2 the zero row before a shadow
    (both among negative rows), row 3 negative rows and one shadow, row 4 shadows only."""
    rng = np.random.default_rng([c, h, nq, n])
    x = rng.integers(-4, 5, (n, c)).astype(np.float32)
    free = np.array([i for i in range(max(n, 1)) if i not in TIED + (ZERO_ROW,)])     # (the special rows are listed by rows 0 .. 2 only)
    inds = free[rng.integers(0, len(free), (nq, h))]
    if n >= GATHER_N:
        x[:NEGATIVE] = -np.abs(x[:NEGATIVE]) - 1
        x[TIED[1]] = x[TIED[0]] = np.abs(x[TIED[0]]) + 5
        x[ZERO_ROW] = 0
    inds = np.where(rng.random((nq, h)) < 0.3, np.array((n, n + 5, -1, BIG))[rng.integers(0, 4, (nq, h))], inds)
    if h >= 3 and nq >= 5 and n >= GATHER_N:
        neg = lambda: rng.integers(0, NEGATIVE, h)
        inds[0] = neg(); inds[0, :2] = (TIED[1], TIED[0])
        inds[1] = neg(); inds[1, :2] = (n, ZERO_ROW)
        inds[2] = neg(); inds[2, :2] = (ZERO_ROW, -1)
        inds[3] = neg(); inds[3, h - 1] = BIG
        inds[4] = (n, n + 5, -1, BIG)[0]
    if nq > 8 and h:
        inds[5] = inds[6]                                  # two rows with the same list: their gradients meet
    return torch.from_numpy(x), _i32(inds), rng


def check_gathers(dev, c, h, nq=GATHER_NQ, n=GATHER_N, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    x, inds, rng = gather_inputs(c, h, nq, n)
    name = "gathers c=%d h=%d nq=%d n=%d" % (c, h, nq, n)
    if product:
        report(name=name, arm="gather_rows_k / scatter_add_rows_k / max_pool_adjoint_k blocks=%d" % tr_blocks(nq * c, 256, ROWS_CAP))
    g = f32(rng.standard_normal((nq, c)))
    first = inds[:, 0].contiguous() if h else torch.full((nq,), BIG, dtype=torch.int32)
    # forward gathers: a vector of indices, then column 0 of the [nq, h] matrix by its stride (closest_pool's read)
    assert same_bits(impl.gather_rows(x, first, 1, nq), R.gather_rows(x, first)), (name, "gather_rows")
    if h:
        assert same_bits(impl.gather_rows(x, inds, h, nq), R.gather_rows(x, first)), (name, "gather_rows by stride")
    if h and nq and n:
        assert same_bits(impl.pool_forward(x, inds, "max"), R.max_pool(x, inds)), (name, "max_pool")
        assert same_bits(impl.pool_forward(x, inds, "closest"), R.gather_rows(x, first)), (name, "closest_pool")
    want64 = R.scatter_add_rows(g, n, first, F64)
    g = g * _pow2(_amax(want64))
    adj = lambda t, **kw: (R.scatter_add_rows(g, n, first, t, **kw), R.max_pool_adjoint(x, inds, g, t))
    (sc64, mx64), (sc32, mx32) = adj(F64), adj(F32)
    judge(report, name + " scatter_add", impl.scatter_add_rows(g, n, first, 1, nq), sc64, sc32)
    if h:
        judge(report, name + " scatter_add by stride", impl.scatter_add_rows(g, n, inds, h, nq), sc64, sc32)
    judge(report, name + " closest adjoint", impl.pool_backward(x, inds, "closest", g), sc64 if h else torch.zeros_like(sc64), sc32 if h else torch.zeros_like(sc32))
    got = impl.pool_backward(x, inds, "max", g)
    judge(report, name + " max adjoint", got, mx64, mx32)
    if h >= 3 and nq >= 5 and n >= GATHER_N:
        _in_range(sc64, mx64)
        arg, vals = R.max_winners(x, inds)
        assert bool((arg[0] == 0).all()) and bool((vals[0, 0] == vals[0, 1]).all()), "row 0: a tie of two real rows, the first wins"
        assert same_bits(got[TIED[1]], g[0]) and not bool(got[TIED[0]].any()) and bool(g[0].all()), (name, "the first of two tied rows")
        assert bool((arg[1] == 0).all()) and bool((arg[2] == 0).all()) and bool((vals[1].max(0)[0] == 0).all())
        assert bool((vals[3].max(0)[0] == 0).all()) and bool((vals[3, :h - 1] < 0).all()), "row 3: the shadow wins over negative rows"
        # the zero row wins row 2 only (row 1 lists a shadow before it): it holds row 2's gradient and nothing else
        assert same_bits(got[ZERO_ROW], g[2]), (name, "the zero row takes row 2's gradient and not row 1's")

# ---- the attention stage ----------------------------------------------------------------------------------------------------------------
def attention_inputs(b, n, c1, c2, bias):
    rng = np.random.default_rng([b, n, c1, c2, int(bias)])
    d = c1 + c2
    f, enc = f32(rng.standard_normal((b, n, c1))), f32(rng.standard_normal((b, n, 16, c2)))
    idx = _i32(_shadowed(rng, rng.integers(0, n, (b, n, 16)), n))
    w = f32(rng.standard_normal((d, d)) / np.sqrt(d))
    bs = f32(rng.normal(0, 0.5, d)) if bias else None
    g = f32(rng.standard_normal((b, n, d)))
    return f, enc, idx, w, bs, g


def check_attention(dev, b, n, c1, c2, bias=True, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    f, enc, idx, w, bs, g = attention_inputs(b, n, c1, c2, bias)
    d = c1 + c2
    k = _pow2(_amax(R.attention_forward(f, enc, idx, w, bs, F64)[0]))
    f, enc = f * k, enc * k
    o64, o32 = R.attention_forward(f, enc, idx, w, bs, F64)[0], R.attention_forward(f, enc, idx, w, bs, F32)[0]
    g = g * _pow2(_amax(*R.attention_backward(f, enc, idx, w, bs, g, F64)[:3]))
    g64, g32 = R.attention_backward(f, enc, idx, w, bs, g, F64), R.attention_backward(f, enc, idx, w, bs, g, F32)
    name = "attention B=%d N=%d c1=%d c2=%d bias=%d" % (b, n, c1, c2, bias)
    if product:
        report(name=name, arm="%s %s" % attn_arms(b * n, c1, c2))
        assert attn_check(b, n, 16, c1, c2) == 0
    share = float((~R.real(idx, n)).double().mean())
    assert b * n < 16 or 0.2 <= share <= 0.4, share
    out = impl.attention_forward(f, enc, idx, w, bs)
    judge(report, name + " out", out, o64, o32)
    assert same_bits(impl.attention_forward(f, enc, idx, w, bs), out), (name, "the forward twice")
    got = impl.attention_backward(f, enc, idx, w, bs, out, g)
    for key, a, r64_, r32_ in zip(("gf", "genc", "gw", "gbias"), got, g64, g32):
        if a is not None:
            judge(report, "%s %s" % (name, key), a, r64_, r32_)
    assert (got[3] is None) == (bs is None)
    # (genc and gw twice, bit for bit: ``Product.attention_backward`` runs the C entry, then the Function, and compares the two)
    _in_range(*g64[:3])
    assert 0.25 <= _amax(o64) <= 20
    for bi in range(b):                                   # a point nobody lists takes exactly nothing
        listed = set(idx[bi].reshape(-1).tolist())
        for p in range(n):
            if p not in listed:
                assert not bool(got[0][bi, p].any()), (name, "gf of an unlisted point", bi, p)


# ---- the deformed KPConv aggregation -----------------------------------------------------------------------------------------------------
ON_KP = (0, 3)                                            # (query, kernel point) placed exactly on the query's first listed support


def deform_inputs(cin, nq, h, on_kp=False):
    g = geometry(nq, h, seed=3)
    rng = g["rng"]
    q, s, inds = g["q"].clone(), g["s"], g["inds"]
    ns = s.shape[0]
    dkp = g["kp"][None] + f32(rng.normal(0, 0.02, (nq, R.K_POINTS, 3)))
    exact = []
    if on_kp:
        assert nq and h and g["kinds"][0] == "full"
        q[ON_KP[0]] = 0
        dkp[ON_KP[0], ON_KP[1]] = s[int(inds[0, 0])]
        exact = [(ON_KP[0], hh, ON_KP[1]) for hh in range(h) if int(inds[0, hh]) == int(inds[0, 0])]
    for _ in range(40):                                    # every influence of a real neighbour at least 1e-4 from the clamp
        if not (nq and h):
            break
        _, _, wpre, ok = R.deformed_geometry(q, s, inds, dkp, EXTENT, F64)
        near = (wpre.abs() < 1e-4) & ok
        if not bool(near.any()):
            break
        dkp = dkp + near.any(2)[..., None].float() * f32(rng.normal(0, 2e-3, (nq, R.K_POINTS, 3)))
        if on_kp:
            dkp[ON_KP[0], ON_KP[1]] = s[int(inds[0, 0])]
    x = f32(rng.standard_normal((ns, cin)))
    dwf = f32(rng.standard_normal((nq, R.K_POINTS, cin)))
    return g, q, s, inds, dkp, x, dwf, exact


def check_deformed(dev, cin, nq, h, on_kp=False, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    g, q, s, inds, dkp, x, dwf, exact = deform_inputs(cin, nq, h, on_kp)
    ns = s.shape[0]
    name = "deformed cin=%d nq=%d h=%d%s" % (cin, nq, h, " on a kernel point" if on_kp else "")
    if product:
        report(name=name, arm="kp_deformed_weighted_k / _bwd_k blocks=%d chunks=%d" % ((nq + 3) // 4, (cin + 63) // 64))
    fwd = lambda t: R.deformed_forward(q, s, inds, x, dkp, EXTENT, t)
    x = x * _pow2(_amax(fwd(F64)))
    bwd = lambda t: R.deformed_backward(q, s, inds, x, dkp, EXTENT, dwf, t, without=exact)
    dwf = dwf * _pow2(_amax(*bwd(F64)))
    wf64, wf32, (dx64, gk64), (dx32, gk32) = fwd(F64), fwd(F32), bwd(F64), bwd(F32)
    if nq and h:
        _, dist, wpre, ok = R.deformed_geometry(q, s, inds, dkp, EXTENT, F64)
        assert float(wpre.abs()[ok.expand_as(wpre)].min()) >= 1e-4, "an influence too close to the clamp"
        assert bool(((wpre > 0) & ok).any()) and bool(((wpre < 0) & ok).any()), "the clamp cuts some and keeps others"
        assert int(((dist == 0) & ok).sum()) == len(exact)
    wf, dx, gkp = impl.deformed(x, dkp, q, s, inds, EXTENT, dwf)
    judge(report, name + " wf", wf.view(nq, R.K_POINTS, cin), wf64, wf32)
    judge(report, name + " dx", dx, dx64, dx32)
    assert bool(torch.isfinite(gkp).all()), (name, "grad_kernel_points is finite everywhere")
    judge(report, name + " gkp", gkp, gk64, gk32)
    if nq and h:
        _in_range(wf64)
        _in_range(dx64, gk64)
    else:
        assert not bool(wf.any()) and not bool(dx.any()) and not bool(gkp.any()) and tuple(wf.shape) == (nq, R.K_POINTS * cin)
    if on_kp:
        whole = R.deformed_backward(q, s, inds, x, dkp, EXTENT, dwf, F64)[1]
        assert bool(torch.isnan(whole[ON_KP]).all()), "the whole float64 formula is 0 / 0 at dist == 0"
        assert bool(torch.isfinite(torch.cat([whole[:ON_KP[0]], whole[ON_KP[0] + 1:]])).all()) and exact
    wf2, _, gkp2 = impl.deformed(x, dkp, q, s, inds, EXTENT, dwf)
    assert same_bits(wf2, wf) and same_bits(gkp2, gkp), (name, "wf and gkp twice")
    for r, kind in enumerate(g["kinds"]):
        if kind == "all_shadow":
            assert not bool(wf[r].any()) and not bool(gkp[r].any()), (name, "all-shadow row", r)


# ---- the offset regulariser ----------------------------------------------------------------------------------------------------------------
REG_NS, REG_EXTENT, REG_REPULSE = 40, 0.6, 1.2


def reg_inputs(K, nq, h, shadow_rows):
    """The first draw (of 50 seeds) whose float64 minima are all 1e-3 ahead of the runner-up or tied exactly.  With h >= 2, kernel
    point 0 of query 0 sits at the origin between supports 0 = (1, 0, 0) and 1 = (-1, 0, 0), listed alternately: an exact tie."""
    for seed in range(50):
        rng = np.random.default_rng([K, nq, h, int(shadow_rows), seed])
        ball = lambda m, r: f32(rng.standard_normal((m, 3)) * r / np.sqrt(3))
        s, q = ball(REG_NS, 1.5), ball(nq, 0.15)
        dkp = ball(K, 0.5)[None] + ball(nq * K, 0.2).view(nq, K, 3)
        inds, kinds = neighbour_rows(rng, nq, REG_NS, h, np.arange(REG_NS))
        if not shadow_rows:
            for r, kind in enumerate(kinds):
                if kind == "all_shadow" and h:
                    inds[r] = rng.integers(0, REG_NS, h)
                    kinds[r] = "full"
        if h >= 2:
            s[0], s[1] = torch.tensor([1.0, 0, 0]), torch.tensor([-1.0, 0, 0])
            q[0], dkp[0, 0] = 0, 0
            inds[0] = np.arange(h) % 2
            kinds[0] = "tie"
        inds = _i32(inds)
        d2 = torch.sort(R.regulariser(q, s, inds, dkp, REG_EXTENT, REG_REPULSE, F64)["d2"], 1)[0]
        if h < 2 or bool(((d2[:, 1] - d2[:, 0] >= 1e-3) | (d2[:, 1] == d2[:, 0])).all()):
            return q, s, inds, dkp, kinds
    raise AssertionError("no draw with clear minima")


def check_regulariser(dev, K, nq, h, shadow_rows=False, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    q, s, inds, dkp, kinds = reg_inputs(K, nq, h, shadow_rows)
    r64, r32 = (R.regulariser(q, s, inds, dkp, REG_EXTENT, REG_REPULSE, t) for t in (F64, F32))
    name = "regulariser K=%d nq=%d h=%d shadow_rows=%d" % (K, nq, h, shadow_rows)
    if product:
        report(name=name, arm="kp_offset_reg_k blocks=%d" % ((nq + 15) // 16))
    dark = torch.tensor([kind == "all_shadow" and h > 0 for kind in kinds])
    lit = ~dark
    if K > 1:
        on, pairs = r64["active"], r64["pairs"]
        assert bool(on.any()) and bool((~on & pairs).any()), "the repulsion is on for some pairs and off for others"
    if h >= 2:
        assert float(r64["d2"][0, 0, 0]) == 1.0 and float(r64["d2"][0, 1, 0]) == 1.0 and r64["gfit"][0, 0].tolist()[0] < 0, "the tie"
    got = impl.regulariser(dkp, q, s, inds, REG_EXTENT, REG_REPULSE)
    judge(report, name + " fitting term", got["fit"], r64["fit"], r32["fit"])
    judge(report, name + " repulsive term", got["rep"], r64["rep"], r32["rep"])
    judge(report, name + " grep", got["grep"], r64["grep"], r32["grep"])
    for rows, what in ((lit, ""), (dark, " all-shadow rows")):
        if bool(rows.any()):
            judge(report, "%s min_d2%s" % (name, what), got["min_d2"][rows], r64["min_d2"][rows], r32["min_d2"][rows])
            judge(report, "%s gfit%s" % (name, what), got["gfit"][rows], r64["gfit"][rows], r32["gfit"][rows])
    if h:
        _in_range(r64["min_d2"][lit])
        assert not bool(dark.any()) or float(r64["min_d2"][dark].min()) > 1e11
    else:
        assert not bool(got["min_d2"].any()) and not bool(got["gfit"].any())
    again = impl.regulariser(dkp, q, s, inds, REG_EXTENT, REG_REPULSE)
    assert all(same_bits(again[key], got[key]) for key in ("fit", "rep", "min_d2", "gfit", "grep")), (name, "twice")


# ---- RandLA-Net's differentiable ops ---------------------------------------------------------------------------------------------------------
def check_gather_max(dev, c, n_out, n_in=GMAX_N_IN, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    rng = np.random.default_rng([c, n_out, n_in])
    feat = torch.from_numpy(rng.integers(-3, 4, (2, n_in, c)).astype(np.float32))
    idx = _i32(rng.integers(0, n_in, (2, n_in, 16)))
    feat[:, :2] = 5                                        # rows 0 and 1 hold the same maximum; kept point 0 lists row 1 FIRST, row 0 last
    idx[:, 0, 0], idx[:, 0, 1], idx[:, 0, 15] = 1, 0, 0
    g = f32(rng.standard_normal((2, n_out, c)))
    g = g * _pow2(_amax(R.gather_max_adjoint(feat, idx, n_out, g, F64)))
    name = "gather_max c=%d n_out=%d n_in=%d" % (c, n_out, n_in)
    if product:
        report(name=name, arm="gather_max / gather_max_adjoint blocks=%d" % ((2 * n_out * c + 255) // 256))
    out, gf = impl.gather_max(feat, idx, n_out, g)
    assert same_bits(out, R.gather_max(feat, idx, n_out)), (name, "forward")
    r64, r32 = R.gather_max_adjoint(feat, idx, n_out, g, F64), R.gather_max_adjoint(feat, idx, n_out, g, F32)
    judge(report, name + " adjoint", gf, r64, r32)
    if n_out:
        _in_range(r64)
        arg, vals = R.max_winners(feat[0], idx[0, :n_out])
        tied = (vals == vals.max(1, keepdim=True)[0]) & (idx[0, :n_out, :, None] != torch.gather(idx[0, :n_out].long(), 1, arg)[:, None, :])
        assert bool(tied.any()), "a maximum held by two different rows"
    else:
        assert not bool(gf.any())


def check_attentive_pool(dev, k, c, rows, impl=None, report=_print):
    product = impl is None
    impl = _impl(dev, impl)
    rng = np.random.default_rng([k, c, rows])
    scores, x = f32(rng.standard_normal((rows, k, c)) * 2), f32(rng.standard_normal((rows, k, c)))
    x = x * _pow2(_amax(R.attentive_pool(scores, x, F64)[0]))
    g = f32(rng.standard_normal((rows, c)))
    g = g * _pow2(_amax(*R.attentive_pool_backward(scores, x, g, F64)))
    name = "attentive_pool k=%d c=%d rows=%d" % (k, c, rows)
    if product:
        report(name=name, arm="attentive_pool_k<false|true> blocks=%d" % ((rows * c + 255) // 256))
    out, gs, gx = impl.attentive_pool(scores, x, g)
    judge(report, name + " out", out, R.attentive_pool(scores, x, F64)[0], R.attentive_pool(scores, x, F32)[0])
    b64, b32 = R.attentive_pool_backward(scores, x, g, F64), R.attentive_pool_backward(scores, x, g, F32)
    judge(report, name + " gscores", gs, b64[0], b32[0])
    judge(report, name + " gx", gx, b64[1], b32[1])
    _in_range(*b64)
    again = impl.attentive_pool(scores, x, g)
    assert all(same_bits(a, b) for a, b in zip(again, (out, gs, gx))), (name, "twice")


# ---- refusals (the product only) -----------------------------------------------------------------------------------------------------------
INVALID, WORKSPACE, UNSUPPORTED = "invalid argument (-1)", "workspace too small (-2)", "unsupported configuration (-4)"
ATTN_REFUSED = ((1, 5, 8, 8, 8), (1, 5, 16, 3, 2), (1, 5, 16, 130, 128), (1, 5, 16, 161, 95), (1, 5, 16, 200, 56), (1, 2 ** 27, 16, 8, 8),
                (2, 2 ** 26, 16, 8, 8))                   # (B, N, K, c1, c2)


def check_refusals(dev, family):
    p = Product(dev)
    z = lambda *shape: torch.zeros(shape, dtype=F32)
    if family == "gemm":
        refused(lambda: p.gemm_tn(z(4, 3), z(4, 5), 4, 5, 5, True), "lda < k", INVALID)
        refused(lambda: p.gemm_tn(z(4, 4), z(4, 5), 4, 5, 4, True), "ldc < n", INVALID)
        refused(lambda: p.gemm_tn(z(4, 4), z(4, 5), 0, 5, 5, True), "k = 0", INVALID)
        k = -1
        refused(lambda: p._call("ml3d_gemm_tn", z(4, 4).to(dev).data_ptr(), 4, z(4, 5).to(dev).data_ptr(), 5, 4, k, 5, z(4, 5).to(dev).data_ptr(), 5, None),
                "k < 0", INVALID)
    elif family == "bn":
        refused(lambda: p.bn_forward(z(4, 4), None, None, BN_EPS, None, rows=0), "rows = 0", INVALID)
        refused(lambda: p.bn_forward(z(4, 4), None, None, BN_EPS, None, rows=-3), "rows < 0", INVALID)
        refused(lambda: p.bn_forward(z(4, 4), None, None, BN_EPS, None, workspace_bytes=8 * 2 * 4 + 255), "a short workspace", WORKSPACE)
        try:
            p.bn_function(z(1, 4), None, None, z(4), z(4), BN_MOMENTUM, BN_EPS, None, z(1, 4))
        except ValueError as e:
            assert "more than 1 row" in str(e)
        else:
            raise AssertionError("one row was accepted")
    elif family == "gathers":
        refused(lambda: p.gather_rows(z(4, 4), _i32(np.zeros(4)), 0, 4), "index_stride = 0", INVALID)
        refused(lambda: p.scatter_add_rows(z(4, 4), 4, _i32(np.zeros(4)), 0, 4), "index_stride = 0", INVALID)
    elif family == "attention":
        from ml3d import ops
        small = lambda: (z(64), z(64), _i32(np.zeros(64)).to(dev), z(64))
        for b, n, k, c1, c2 in ATTN_REFUSED:
            assert attn_check(b, n, k, c1, c2) == -4 and not ops.attention_stage_supported(k, c1, c2, b * n), (b, n, k, c1, c2)
            f, enc, idx, w = (t.to(dev) for t in small())
            out = z(64).to(dev)
            refused(lambda: p._call("ml3d_randla_attention_stage", f.data_ptr(), enc.data_ptr(), idx.data_ptr(), w.data_ptr(), None, b, n, k,
                                    c1, c2, out.data_ptr()), "attention %s" % ((b, n, k, c1, c2),), UNSUPPORTED)
            refused(lambda: p._call("ml3d_randla_attention_stage_backward", f.data_ptr(), enc.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                    w.data_ptr(), None, out.data_ptr(), out.data_ptr(), b, n, k, c1, c2, out.data_ptr(), out.data_ptr(),
                                    out.data_ptr(), None, out.data_ptr(), 1 << 40), "attention backward %s" % ((b, n, k, c1, c2),), UNSUPPORTED)
        for c in CASES:
            if c["body"] == "attention":
                kw = c["kw"]
                assert attn_check(kw["b"], kw["n"], 16, kw["c1"], kw["c2"]) == 0 and ops.attention_stage_supported(16, kw["c1"], kw["c2"], kw["b"] * kw["n"])
        assert ops.attention_stage_supported(16, 160, 96, 2 ** 27 - 1) and attn_check(1, 2 ** 27 - 1, 16, 160, 96) == 0
        f, enc, idx, w, bs, g = (None if t is None else t.to(dev) for t in attention_inputs(1, 5, 8, 8, False))
        bufs = [torch.zeros(n, dtype=F32, device=dev) for n in (5 * 16, 5 * 8, 5 * 16 * 8, 256)]
        need = p.lib.ml3d_randla_attention_stage_backward_workspace_bytes(1, 5, 8, 8)
        assert need == attn_workspace_bytes(5, 16)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        refused(lambda: p._call("ml3d_randla_attention_stage_backward", f.data_ptr(), enc.data_ptr(), idx.data_ptr(), w.data_ptr(), w.data_ptr(),
                                None, bufs[0].data_ptr(), g.data_ptr(), 1, 5, 16, 8, 8, bufs[1].data_ptr(), bufs[2].data_ptr(),
                                bufs[3].data_ptr(), None, ws.data_ptr(), need - 1), "a short workspace", WORKSPACE)
    elif family == "deformed":
        _, q, s, inds, dkp, x, dwf, _ = deform_inputs(8, 5, 5)
        refused(lambda: p.deformed(x, dkp[:, :14].contiguous(), q, s, inds, EXTENT, dwf[:, :14]), "K = 14", UNSUPPORTED)
    elif family == "regulariser":
        q, s, inds, dkp, _ = reg_inputs(16, 5, 14, False)
        refused(lambda: p.regulariser(torch.cat([dkp, dkp[:, :1]], 1), q, s, inds, REG_EXTENT, REG_REPULSE), "K = 17", UNSUPPORTED)
    elif family == "attentive_pool":
        refused(lambda: p.attentive_pool(z(3, 33, 4), z(3, 33, 4), z(3, 4)), "k = 33", UNSUPPORTED)
    else:
        raise AssertionError(family)


REFUSAL_FAMILIES = ("gemm", "bn", "gathers", "attention", "deformed", "regulariser", "attentive_pool")


# ---- the host rules of train.hip, restated --------------------------------------------------------------------------------------------------
GEMM_WAVES, GEMM_SLICE_ROWS = 2048, 128                   # ml3d_gemm_tn: ~waves in flight; fewest rows of a slice
REDUCE_ELEMS, REDUCE_CAP = 8192, 2048                     # tr_reduce_blocks
BN_APPLY_PER, BN_APPLY_CAP = 1024, 4096                   # bn_apply_k / bn_backward_apply_k on tr_blocks
ROWS_PER, ROWS_CAP = 256, 8192                            # the gathers and their adjoints on tr_blocks
AS_K, AS_DMAX, AS_C1MAX = 16, 256, 160
ATTN_FWD_CAP, ATTN_BWD_CAP, ATTN_PARTIAL_BYTES, ATTN_CHUNK = 2048, 2048, 160 << 20, 32

RULE_TEXT = (
    "if (m < 0 || k <= 0 || n <= 0 || lda < k || ldb < n || ldc < n || !c) return ML3D_E_INVALID;",
    "if (ldc == n) zero_async(c, sizeof(float) * (size_t)k * (size_t)n, st);",
    "else for (int i = 0; i < k; ++i) zero_async(c + (int64_t)i * ldc, sizeof(float) * (size_t)n, st);",
    "int64_t slices = (2048 + ntiles - 1) / ntiles;", "const int64_t max_slices = (m + 127) / 128;",
    "if (slices > max_slices) slices = max_slices;", "int64_t rps = (m + slices - 1) / slices;", "rps = (rps + 1) & ~(int64_t)1;",
    "slices = (m + rps - 1) / rps;",
    "int64_t b = (rows * (int64_t)c + 8191) / 8192;", "if (b > rows) b = rows;", "if (b > 2048) b = 2048;",
    "hipLaunchKernelGGL(bn_apply_k, dim3(tr_blocks(total, 1024, 4096))", "hipLaunchKernelGGL(bn_backward_apply_k, dim3(tr_blocks(total, 1024, 4096))",
    "hipLaunchKernelGGL(gather_rows_k, dim3(tr_blocks(total, 256, 8192))", "hipLaunchKernelGGL(scatter_add_rows_k, dim3(tr_blocks(total, 256, 8192))",
    "hipLaunchKernelGGL(max_pool_adjoint_k, dim3(tr_blocks(total, 256, 8192))",
    "if (rows <= 0 || channels <= 0 || (act != 0 && act != 1)) return ML3D_E_INVALID;",
    "return channels > 0 ? sizeof(double) * 2 * (size_t)channels + 256 : 0;",
    "constexpr int AS_K = 16;", "constexpr int AS_DMAX = 256;", "constexpr int AS_C1MAX = 160;",
    "if (batch * n >= ((int64_t)1 << 31) / 16) return ML3D_E_UNSUPPORTED;",
    "if (k != AS_K || d > AS_DMAX || (d & 1) || (d > 128 && c1 > AS_C1MAX)) return ML3D_E_UNSUPPORTED;",
    "if (d <= 128) { const int64_t tiles = (npts + 3) / 4; hipLaunchKernelGGL((attn_stage_fwd_k<64>), dim3(tr_blocks(tiles, 1, 2048))",
    "const int64_t tiles = (npts + 1) / 2; hipLaunchKernelGGL((attn_stage_fwd_k<32>), dim3(tr_blocks(tiles, 1, 2048))",
    "*tiles = d <= 16 ? (npts + 3) / 4 : (npts + 1) / 2;", "int64_t g = *tiles < 2048 ? *tiles : 2048;",
    "const int64_t cap = ((int64_t)160 << 20) / ((int64_t)d * d * 4);", "if (g > cap) g = cap;",
    "return sizeof(float) * (size_t)(groups + (groups + 31) / 32) * (size_t)d * (size_t)d + 256;",
    "if (d <= 16) hipLaunchKernelGGL((attn_stage_bwd_k<16>)", "else if (d <= 64) hipLaunchKernelGGL((attn_stage_bwd_k<64>)",
    "else if (d <= 128) hipLaunchKernelGGL((attn_stage_bwd_k<128>)", "else hipLaunchKernelGGL((attn_stage_bwd_k<256>)",
    "const int chunks = (groups + 31) / 32;", "if (chunks == 1) {", "if (chunks <= 32) {",
    "if (num_kernel_points != DK) return ML3D_E_UNSUPPORTED;", "constexpr int DK = 15;",
    "return num_kernel_points > 16 ? ML3D_E_UNSUPPORTED : ML3D_E_INVALID;",
    "hipLaunchKernelGGL(kp_offset_reg_k, dim3((unsigned)((n_queries + 15) / 16))",
    "hipLaunchKernelGGL(kp_deformed_weighted_k, dim3((unsigned)((n_queries + 3) / 4))",
)
RANDLA_RULE_TEXT = ("constexpr int AP_KMAX = 32;", "if (k > AP_KMAX) return ML3D_E_UNSUPPORTED;",
                    "hipLaunchKernelGGL((attentive_pool_k<false>), dim3((unsigned)((total + 255) / 256))",
                    "hipLaunchKernelGGL((attentive_pool_k<true>), dim3((unsigned)((total + 255) / 256))",
                    "hipLaunchKernelGGL(gather_max_adjoint, dim3((unsigned)((total + 255) / 256))")


def _source(name):
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, os.pardir, "open3d-ml_amd", "csrc", name)) as f:
        return re.sub(r"\s+", "", f.read())


def assert_rules_are_the_sources():
    for name, rules in (("train.hip", RULE_TEXT), ("randla.hip", RANDLA_RULE_TEXT)):
        src = _source(name)
        for text in rules:
            assert re.sub(r"\s+", "", text) in src, "%s no longer says: %s" % (name, text)


def train_globals():
    """Every ``__global__`` of train.hip, by name (what REQUIRED_ARMS has to cover)."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, os.pardir, "open3d-ml_amd", "csrc", "train.hip")) as f:
        return re.findall(r"__global__ void(?:\s+__launch_bounds__\(\d+\))?(?:\s+ML3D_WAVES_PER_SIMD\(\d+\))?\s+(\w+)\(", f.read())


def gemm_plan(m, k, n):
    """-> (slices, rows per slice, tiles, what limits the slices) of ml3d_gemm_tn."""
    tiles = ((k + 63) // 64) * ((n + 63) // 64)
    by_tiles, by_rows = (GEMM_WAVES + tiles - 1) // tiles, (m + GEMM_SLICE_ROWS - 1) // GEMM_SLICE_ROWS
    slices = max(1, min(by_tiles, by_rows))
    rps = ((m + slices - 1) // slices + 1) & ~1
    return (m + rps - 1) // rps, rps, tiles, "tiles" if by_tiles < by_rows else "rows"


def reduce_blocks(rows, c):
    return max(1, min((rows * c + REDUCE_ELEMS - 1) // REDUCE_ELEMS, rows, REDUCE_CAP))


def tr_blocks(total, per, cap):
    return max(1, min((total + per - 1) // per, cap))


def attn_check(b, n, k, c1, c2):
    if b < 0 or n < 0 or c1 <= 0 or c2 <= 0:
        return -1
    d = c1 + c2
    if b * n >= (1 << 31) // 16:
        return -4
    return -4 if k != AS_K or d > AS_DMAX or d % 2 or (d > 128 and c1 > AS_C1MAX) else 0


def attn_plan(npts, d):
    """-> (forward tile height, backward class, tiles, groups, levels of the partial sum) of the two attention entries."""
    tiles = (npts + 3) // 4 if d <= 16 else (npts + 1) // 2
    groups = max(1, min(tiles, ATTN_BWD_CAP, ATTN_PARTIAL_BYTES // (d * d * 4)))
    chunks = (groups + ATTN_CHUNK - 1) // ATTN_CHUNK
    return 64 if d <= 128 else 32, 16 if d <= 16 else 64 if d <= 64 else 128 if d <= 128 else 256, tiles, groups, 1 if chunks == 1 else 2 if chunks <= 32 else 3


def attn_workspace_bytes(npts, d):
    groups = attn_plan(npts, d)[3]
    return 4 * (groups + (groups + 31) // 32) * d * d + 256


def attn_arms(npts, c1, c2):
    r, cls, tiles, groups, levels = attn_plan(npts, c1 + c2)
    return "attn_stage_fwd_k<%d>" % r, "attn_stage_bwd_k<%d> tiles=%d groups=%d levels=%d" % (cls, tiles, groups, levels)


# ---- the case tables -----------------------------------------------------------------------------------------------------------------------
CASES = []


def _case(group, body, **kw):
    CASES.append(dict(group=group, body=body, kw=kw, id=",".join("%s=%s" % (k, v) for k, v in kw.items())))


for _k in GEMM_KN:
    for _n in GEMM_KN:
        _case("gemm_kn", "gemm", m=129, k=_k, n=_n, col_sums=(_k + _n) % 2 == 0)
for _k, _n in GEMM_M_SHAPES:
    for _m in GEMM_M:
        _case("gemm_m", "gemm", m=_m, k=_k, n=_n)
        _case("gemm_m", "gemm", m=_m, k=_k, n=_n, strided=True, col_sums=_m % 2 == 1)
for _k, _n in ((1, 1), (32, 65), (97, 33)):
    _case("gemm_strided", "gemm", m=257, k=_k, n=_n, strided=True)
_case("gemm_by_tiles", "gemm", **GEMM_BY_TILES)
for _c in BN_C:
    _case("bn_c", "bn", rows=257, c=_c, slope=0.2)
    _case("bn_c", "bn", rows=3 if _c > 256 else 7, c=_c, slope=None)
for _c in BN_ROWS_C:
    for _r in BN_ROWS:
        _case("bn_rows", "bn", rows=_r, c=_c, slope=0.2)
for _r, _c in ((2, 512), (3, 1024), (2, 257)):
    _case("bn_rows", "bn", rows=_r, c=_c, slope=0.2)
for _s in BN_SLOPES:
    for _g in (False, True):
        for _b in (False, True):
            _case("bn_full", "bn", rows=255, c=96, slope=_s, gamma=_g, beta=_b)
            _case("bn_full", "bn", rows=7, c=340, slope=_s, gamma=_g, beta=_b)
for _s in BN_SLOPES:
    _case("bn_function", "bn_function", rows=257, c=96, slope=_s)
_case("bn_function", "bn_function", rows=2, c=340, slope=0.2)
_case("bn_function", "bn_function", rows=255, c=5, slope=0.2, gamma=False, beta=False)
_case("bn_cap", "bn", slope=0.2, **BN_CAP)
for _c in GATHER_C:
    for _h in GATHER_H:
        _case("gathers", "gathers", c=_c, h=_h)
_case("gathers", "gathers", c=3, h=5, nq=0)
_case("gathers", "gathers", c=3, h=5, n=0)
_case("gathers", "gathers", c=3, h=0)
_case("gathers_cap", "gathers", **GATHER_CAP)
for _i, (_c1, _c2) in enumerate(ATTN_SHAPES):
    _case("attn_shapes", "attention", b=2, n=17, c1=_c1, c2=_c2, bias=_i % 3 != 2)
for _c1, _c2 in ATTN_ROWS_SHAPES:
    for _i, (_b, _n) in enumerate(ATTN_ROWS):
        _case("attn_rows", "attention", b=_b, n=_n, c1=_c1, c2=_c2, bias=_i % 2 == 0)
_case("attn_levels", "attention", **ATTN_THREE_LEVELS)
_case("attn_levels", "attention", bias=False, **ATTN_MORE_TILES)
_case("attn_cap", "attention", **ATTN_MEMORY_CAP)
for _cin in DEFORM_CIN:
    _case("deformed", "deformed", cin=_cin, nq=33, h=37, on_kp=_cin in (8, 65))
for _h in DEFORM_H:
    _case("deformed", "deformed", cin=65, nq=5, h=_h)
for _nq in DEFORM_NQ:
    _case("deformed", "deformed", cin=8, nq=_nq, h=5, on_kp=_nq == 3)
for _K in REG_K:
    _case("regulariser", "regulariser", K=_K, nq=33, h=14)
    _case("regulariser", "regulariser", K=_K, nq=33, h=14, shadow_rows=True)
for _nq in REG_NQ:
    _case("regulariser", "regulariser", K=15, nq=_nq, h=14)
for _h in REG_H:
    _case("regulariser", "regulariser", K=15, nq=17, h=_h, shadow_rows=_h == 1)
    _case("regulariser", "regulariser", K=16, nq=16, h=_h)
for _c in GMAX_C:
    for _n_out in (0, 1, GMAX_N_IN - 1, GMAX_N_IN):
        _case("gather_max", "gather_max", c=_c, n_out=_n_out)
for _k in APOOL_K:
    for _c in APOOL_C:
        for _r in APOOL_ROWS:
            _case("attentive_pool", "attentive_pool", k=_k, c=_c, rows=_r)

BODIES = dict(gemm=check_gemm, bn=check_bn, bn_function=check_bn_function, gathers=check_gathers, attention=check_attention,
              deformed=check_deformed, regulariser=check_regulariser, gather_max=check_gather_max, attentive_pool=check_attentive_pool)
GROUPS = tuple(dict.fromkeys(c["group"] for c in CASES))


def cases_of(group):
    return [c for c in CASES if c["group"] == group]


def run_case(dev, case, impl=None, report=_print):
    return BODIES[case["body"]](dev, impl=impl, report=report, **case["kw"])


def comparisons(case):
    """The lines with measured figures a case prints (``judge`` calls)."""
    kw, body = case["kw"], case["body"]
    if body == "gemm":
        return 1 + bool(kw.get("col_sums", True))
    if body == "bn":
        return 5 + bool(kw.get("gamma", True)) + bool(kw.get("beta", True))
    if body == "bn_function":
        return 4 + bool(kw.get("gamma", True)) + bool(kw.get("beta", True))
    if body == "gathers":
        return 3 + bool(kw["h"])
    if body == "attention":
        return 4 + bool(kw.get("bias", True))
    if body == "deformed":
        return 3
    if body == "regulariser":
        return 5 + 2 * bool(kw.get("shadow_rows") and kw["h"] and "all_shadow" in reg_inputs(**_reg_kw(kw))[4])
    return dict(gather_max=1, attentive_pool=3)[body]


def _reg_kw(kw):
    return dict(K=kw["K"], nq=kw["nq"], h=kw["h"], shadow_rows=kw.get("shadow_rows", False))


def arms_of(case):
    """The kernels a case reaches on the product, by the restated rules (+ the named properties of the large cases)."""
    kw, body = case["kw"], case["body"]
    if body == "gemm":
        if not kw["m"]:
            return ["gemm_tn m = 0"]
        arms = ["gemm_tn_k"] + ["col_reduce_k<0>"] * bool(kw.get("col_sums", True))
        slices, rps, tiles, by = gemm_plan(kw["m"], kw["k"], kw["n"])
        arms += ["gemm_tn_k slices by tiles"] * (by == "tiles") + ["gemm_tn_k odd last row"] * (kw["m"] % 2 == 1 and slices >= 1)
        arms += ["gemm_tn_k several slices"] * (slices > 1) + ["gemm_tn per-row zeroing"] * bool(kw.get("strided"))
        return arms
    if body in ("bn", "bn_function"):
        total = kw["rows"] * kw["c"]
        arms = ["col_reduce_k<1>", "col_reduce_k<2>", "bn_finalize_k", "bn_apply_k", "bn_backward_apply_k"]
        arms += ["bn_apply_k past the 4096-workgroup cap"] * (total > BN_APPLY_CAP * BN_APPLY_PER)
        arms += ["bn_backward_apply_k fewer threads than channels"] * (tr_blocks(total, BN_APPLY_PER, BN_APPLY_CAP) * 256 < kw["c"])
        return arms
    if body == "gathers":
        nq, n, h = kw.get("nq", GATHER_NQ), kw.get("n", GATHER_N), kw["h"]
        arms = ["gather_rows_k"] * bool(nq) + ["scatter_add_rows_k"] * bool(nq and n) + ["max_pool_adjoint_k"] * bool(nq and n and h)
        return arms + ["gathers past the 8192-workgroup cap"] * (nq * kw["c"] > ROWS_CAP * ROWS_PER)
    if body == "attention":
        npts, d = kw["b"] * kw["n"], kw["c1"] + kw["c2"]
        r, cls, tiles, groups, levels = attn_plan(npts, d)
        arms = ["attn_stage_fwd_k<%d>" % r, "attn_stage_bwd_k<%d>" % cls, "sum_partials_k", "sum_partials_k %d level%s" % (levels, "s" * (levels > 1))]
        arms += ["attn_stage_bwd_k more tiles than groups"] * (tiles > groups)
        arms += ["attn_stage_bwd_k groups by the 160 MB cap"] * (groups < min(tiles, ATTN_BWD_CAP))
        return arms
    if body == "deformed":
        return ["kp_deformed_weighted_k", "kp_deformed_weighted_bwd_k"] * bool(kw["nq"])
    if body == "regulariser":
        return ["kp_offset_reg_k"]
    if body == "gather_max":
        return ["gather_max", "gather_max_adjoint"] * bool(kw["n_out"])
    return ["attentive_pool_k<false>", "attentive_pool_k<true>"]


REQUIRED_ARMS = ("gemm_tn_k", "col_reduce_k<0>", "col_reduce_k<1>", "col_reduce_k<2>", "bn_finalize_k", "bn_apply_k", "bn_backward_apply_k",
                 "gather_rows_k", "scatter_add_rows_k", "max_pool_adjoint_k", "attn_stage_fwd_k<64>", "attn_stage_fwd_k<32>",
                 "attn_stage_bwd_k<16>", "attn_stage_bwd_k<64>", "attn_stage_bwd_k<128>", "attn_stage_bwd_k<256>", "sum_partials_k",
                 "kp_deformed_weighted_k", "kp_deformed_weighted_bwd_k", "kp_offset_reg_k",
                 "gather_max", "gather_max_adjoint", "attentive_pool_k<false>", "attentive_pool_k<true>",
                 "gemm_tn m = 0", "gemm_tn_k slices by tiles", "gemm_tn_k odd last row", "gemm_tn_k several slices", "gemm_tn per-row zeroing",
                 "bn_apply_k past the 4096-workgroup cap", "bn_backward_apply_k fewer threads than channels",
                 "gathers past the 8192-workgroup cap", "sum_partials_k 1 level", "sum_partials_k 2 levels", "sum_partials_k 3 levels",
                 "attn_stage_bwd_k more tiles than groups", "attn_stage_bwd_k groups by the 160 MB cap")


def arms_table():
    """arm -> ids of the cases that reach it."""
    table = {}
    for c in CASES:
        for arm in arms_of(c):
            table.setdefault(arm, []).append("%s[%s]" % (c["group"], c["id"]))
    return table
