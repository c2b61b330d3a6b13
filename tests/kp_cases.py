"""Shared bodies and shape tables of the KPConv op tests (csrc/kpconv.hip through ``ml3d.ops``): tests/test_emulated_kpconv_ops.py
runs them on CPU tensors against the host emulation, tests/test_gpu_kpconv_ops.py on the MI355X, tests/test_kp_cases_can_fail.py
against deliberately wrong float64 stand-ins.  Every body takes ``(dev, ..., impl=None, report=_print)``; ``impl=None`` = the
product's ``ml3d.ops``.

Floats are judged by ``pt_cases.judge``: against the formulas of tests/kp_ref.py in FLOAT64, within max(1e-5, 4 e32), e32 the
distance of the same formulas in float32 from float64 at the case's own inputs.  Repeated calls, rows computed alone, all-shadow
rows and the pools are compared for EQUALITY.

GEOMETRY (``geometry``): no radius search -- supports uniform in a ball of radius 0.2 around the origin, support 0 AT the origin,
queries within 0.02 of it, the 15 kernel points of ``synthetic_kernel_points(0.2)``, extent 0.12: the linear influence is nonzero
for about a sixth of all (query, support, kernel point) triples and for every kernel point, so the clamp cuts some and keeps
others (asserted on the float64 reference in ``_assert_shares``).  The neighbour ROWS are written by ``neighbour_rows``: row r of
a case is of kind ``row_kinds(h)[r % len]`` -- full, shadows anywhere, all shadows, shadows last, last real entry in the last
column, duplicates, last real entry exactly at column 63 / 64 / 127 / 128 -- with the shadow spelt Ns, Ns + 5 or 2^31 - 1.  The
last real entry of every row is a support within 0.09 of the origin: it has weight on the central kernel point under every
influence, so a walk that ends one column early always loses something.

DISPATCH: ``weighted_arm`` / ``rigid_arm`` / ``pool_arm`` restate the host rules of kpconv.hip next to the constants they use;
``RULE_TEXT`` pins each restated rule to the line of the source it restates; ``arms_table`` names, for every kernel
instantiation of ``REQUIRED_ARMS``, the cases that reach it.  tests/test_kp_cases_can_fail.py asserts all three before anything runs."""
import os
import re

import numpy as np
import torch

import kp_ref as R
from oracle import kpconv_ref as K
from pt_cases import _print, f32, judge, refused, same_bits

KP_RADIUS, EXTENT, NS, SLOPE = 0.2, 0.12, 300, 0.1
SHADOWS = lambda ns: (ns, ns + 5, 2 ** 31 - 1)
TARGET = 4.0                                              # the reference's largest magnitude after scaling, inside [0.5, 20]

H_WIDTHS = (1, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 131, 260)
NQ_TAILS = (1, 3, 9, 31, 33, 255, 257)
AGG_CIN = (1, 2, 3, 4, 5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512)
AGG_H = (5, 33, 65, 131)
AGG_MISALIGNED_CIN = (16, 32, 64)
AGG_INFLUENCE_CIN = (3, 24, 64, 200, 16, 32, 128, 256)           # one per kernel family, then the other MFMA tile counts
AGG_WIDTH_CIN = (4, 24, 64)
AGG_TAIL_CIN = (4, 24, 16)
AGG_LONG = dict(nq=8221, cin=16, h=9)
ALONE_ROWS = (0, 7, 32)
FUSED_CIN, FUSED_COUT = (1, 2, 3, 4, 5), (32, 64, 96, 128)
FUSED_FULL = ((1, 32), (3, 96), (5, 128))                 # three influences x {no bias, bias} x act {0, 1, 2}
FUSED_H = (1, 4, 5, 8, 9, 33, 131)
FUSED_LEAVING = tuple((cin, cout) for cin in (1, 5) for cout in (16, 48, 160))
B32_NQ = (1, 15, 16, 17, 257)
B32_H = (1, 5, 64, 65, 128, 129, 260)
B32_LONG = dict(nq=16517, h=9)
GEMM_CIN, GEMM_COUT = (16, 24, 64, 128, 256, 512), (32, 40, 64)
H0_SHAPES = ((1, 32), (32, 32), (64, 40))
DEFORM_CASES = ((16, 33, False), (256, 33, False), (512, 33, True), (32, 5, False), (128, 129, True), (64, 260, False))   # (cin, h, modulated)
ADJ_CIN = (1, 5, 24, 64, 65, 130, 512)
ADJ_H = (1, 33, 131)
POOL_C = (1, 3, 4, 6, 8, 64, 130, 132)
POOL_H = (1, 3, 4, 5, 8, 9, 73)
POOL_MISALIGNED_C = (4, 64)


def _ops(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _ball(rng, n, radius):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius * rng.random((n, 1)) ** (1.0 / 3.0)).astype(np.float32)


def row_kinds(h):
    kinds = ["full", "shuffled", "all_shadow"]
    if h >= 2:
        kinds += ["shadows_last", "last_col", "dup"]
    return kinds + ["end@%d" % c for c in (63, 64, 127, 128) if c < h]


def neighbour_rows(rng, nq, ns, h, near):
    """-> (inds int32 [nq, h], kind of every row).  ``near``: the supports a row may END with (see the module docstring)."""
    kinds = row_kinds(h)
    shadows = np.array(SHADOWS(ns), np.int64)
    inds = np.empty((nq, h), np.int64)
    used = []
    for r in range(nq):
        kind = kinds[r % len(kinds)] if h else "all_shadow"
        used.append(kind)
        row = rng.integers(0, ns, h)
        hole = shadows[rng.integers(0, 3, h)]
        if kind == "all_shadow":
            row = hole
        elif kind == "shuffled":                           # about half the columns shadows, anywhere
            row = np.where(rng.random(h) < 0.5, hole, row)
            if h == 1:
                row = rng.integers(0, ns, h)
        elif kind == "shadows_last":
            n_real = int(rng.integers(1, h))
            row[n_real:] = hole[n_real:]
        elif kind == "last_col":                           # shadows before a real LAST column
            row = np.where(rng.random(h) < 0.5, hole, row)
            row[h - 1] = 0
        elif kind == "dup":                                # a third of the columns repeat one index, another third a second one
            row[rng.random(h) < 0.34] = row[0]
            row[rng.random(h) < 0.34] = row[h - 1]
        elif kind.startswith("end@"):
            c = int(kind[4:])
            row = np.where(rng.random(h) < 0.4, hole, row)
            row[c] = 0
            row[c + 1:] = hole[c + 1:]
        real = np.flatnonzero(row < ns)
        if len(real):
            row[real[-1]] = near[rng.integers(0, len(near))]
        inds[r] = row
    return inds.astype(np.int32), used


def geometry(nq, h, ns=NS, seed=0):
    """-> dict(q, s, inds, kp as float32 / int32 CPU tensors, kinds)."""
    rng = np.random.default_rng([nq, h, ns, seed])
    s = _ball(rng, ns, KP_RADIUS)
    s[0] = 0
    q = _ball(rng, nq, 0.02)
    near = np.flatnonzero(np.linalg.norm(s, axis=1) < 0.09)
    assert len(near) >= 5 and near[0] == 0
    inds, kinds = neighbour_rows(rng, nq, ns, h, near)
    return dict(q=torch.from_numpy(q), s=torch.from_numpy(s), inds=torch.from_numpy(inds).reshape(nq, h),
                kp=torch.from_numpy(K.synthetic_kernel_points(KP_RADIUS)), kinds=kinds, rng=rng)


def _assert_shares(g):
    """On the float64 reference: the linear influence of the case's queries (the first 256) is nonzero for 10 .. 50 % of all (query,
    support, kernel point) triples and for at least 5 % of every kernel point's -- over ALL supports, so that the statement holds
    for a case of one query and one column too -- and, where a case lists at least 200 real neighbours, over the listed ones."""
    q, s, kp = g["q"][:256].double(), g["s"].double(), g["kp"].double()
    every = torch.arange(s.shape[0], dtype=torch.int32)[None].expand(q.shape[0], -1)
    for inds in (every, g["inds"][:256]):
        ok = R.real(inds, s.shape[0])
        if int(ok.sum()) < 200:
            continue
        nz = (R.influences(q, s, inds, kp, EXTENT, "linear") > 0).double().sum((0, 2)) / float(ok.sum())
        assert 0.10 <= float(nz.mean()) <= 0.50 and float(nz.min()) >= 0.05, nz.tolist()


def _features(g, cin):
    return f32(g["rng"].standard_normal((g["s"].shape[0], cin)))


def _misaligned(x, dev):
    """A contiguous copy of ``x`` that starts 4 bytes into a larger buffer: not 16-byte aligned."""
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=dev)
    lead = 1 + (-(buf.data_ptr() // 4) % 4)                # the view starts 4 bytes past a 16-byte boundary
    v = buf[lead:lead + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _pow2_scale(largest):
    return float(2.0 ** np.round(np.log2(TARGET / largest))) if largest > 0 else 1.0


def _dev(g, dev):
    return g["q"].to(dev), g["s"].to(dev), g["inds"].to(dev)


def _dbl(g):
    return g["q"].double(), g["s"].double(), g["inds"]


# ---- aggregation alone: ops.kpconv_weighted ------------------------------------------------------------------------------------------
def check_weighted(dev, cin, nq, h, influence=1, misaligned=False, alone=(), impl=None, report=_print):
    ops = _ops(impl)
    g = geometry(nq, h)
    _assert_shares(g)
    x = _features(g, cin)
    kp = g["kp"]
    r64 = R.weighted(*_dbl(g), x.double(), kp.double(), EXTENT, influence)
    k = _pow2_scale(float(r64.abs().max()))
    x, r64 = x * k, r64 * k
    r32 = R.weighted(g["q"], g["s"], g["inds"], x, kp, EXTENT, influence)
    name = "weighted cin=%d nq=%d h=%d influence=%d%s" % (cin, nq, h, influence, " misaligned" if misaligned else "")
    if impl is None:
        arm = weighted_arm(cin, nq, h, NS, influence, aligned=not misaligned)
        report(name=name, arm=arm)
    xd = _misaligned(x, dev) if misaligned else x.to(dev)
    q, s, inds = _dev(g, dev)
    call = lambda rows=slice(None): ops.kpconv_weighted(q[rows].contiguous(), s, inds[rows].contiguous(), xd, kp.to(dev), EXTENT, influence)
    got = call().cpu().view(nq, R.K_POINTS, cin)
    judge(report, name, got, r64, r32)
    assert 0.5 <= float(r64.abs().max()) <= 20
    assert same_bits(call().cpu().view(nq, R.K_POINTS, cin), got), (name, "the call twice")
    for r, kind in enumerate(g["kinds"]):
        if kind == "all_shadow":
            assert not bool(got[r].any()), (name, "all-shadow row", r)
    for r in alone:                                        # a wave's result depends on its own row only
        assert same_bits(call(slice(r, r + 1)).cpu().view(1, R.K_POINTS, cin), got[r:r + 1].contiguous()), (name, "row alone", r)


# ---- ops.kpconv_rigid: fused first layer, the 32 -> 32 block, aggregation + GEMM -------------------------------------------------------
def _weights(g, cin, cout, wf64, bias):
    rng = g["rng"]
    w = f32(rng.standard_normal((R.K_POINTS * cin, cout)))
    y = wf64.flatten(1) @ w.double()
    w = w * (_pow2_scale(float(y.abs().max())) if y.numel() else 2.0 ** -6)
    b = f32(rng.normal(0, 0.5, cout)) if bias else None
    return w, b


def check_rigid(dev, cin, cout, nq, h, influence=1, bias=True, act=1, misaligned=False, packed=False, impl=None, report=_print):
    ops = _ops(impl)
    g = geometry(nq, h)
    if h:
        _assert_shares(g)
    x, kp = _features(g, cin), g["kp"]
    wf64 = R.weighted(*_dbl(g), x.double(), kp.double(), EXTENT, influence)
    w, b = _weights(g, cin, cout, wf64, bias)
    r64 = R.contract(wf64, w.double(), None if b is None else b.double(), act, SLOPE)
    r32 = R.conv(g["q"], g["s"], g["inds"], x, kp, EXTENT, influence, w, b, act, SLOPE)
    name = "rigid %d->%d nq=%d h=%d influence=%d bias=%d act=%d%s%s" % (cin, cout, nq, h, influence, bias, act,
                                                                       " misaligned" if misaligned else "", " bf16x3" if packed else "")
    if impl is None:
        report(name=name, arm=rigid_arm(cin, cout, nq, h, NS, influence, aligned=not misaligned))
    xd = _misaligned(x, dev) if misaligned else x.to(dev)
    q, s, inds = _dev(g, dev)
    wd, bd = w.to(dev), None if b is None else b.to(dev)
    pk = None
    if packed:
        pk = ops.pack_bf16x3(wd)
        assert pk is not None, "the weight matrix is eligible for the bf16x3 split"
    got = ops.kpconv_rigid(q, s, inds, xd, kp.to(dev), wd, bd, EXTENT, act=act, slope=SLOPE, influence=influence, packed=pk).cpu()
    judge(report, name, got, r64, r32)
    if nq and h:
        pre = R.contract(wf64, w.double())
        assert 0.5 <= float(pre.abs().max()) <= 20
    rest = R.activation(b if b is not None else torch.zeros(cout), act, SLOPE)
    for r, kind in enumerate(g["kinds"]):
        if kind == "all_shadow":
            assert torch.equal(got[r], rest), (name, "all-shadow row is not act(bias)", r)
    return got


def check_h0(dev, cin, cout, impl=None, report=_print):
    """inds [nq, 0]: every row exactly act(bias), wf all zeros."""
    ops = _ops(impl)
    for act, bias in ((1, True), (2, True), (0, False)):
        got = check_rigid(dev, cin, cout, 9, 0, bias=bias, act=act, impl=impl, report=report)
        assert tuple(got.shape) == (9, cout)
    g = geometry(9, 0)
    q, s, inds = _dev(g, dev)
    wf = ops.kpconv_weighted(q, s, inds, _features(g, cin).to(dev), g["kp"].to(dev), EXTENT, 1).cpu()
    assert tuple(wf.shape) == (9, R.K_POINTS * cin) and not bool(wf.any())


def check_nq0(dev, impl=None, report=_print):
    for cin, cout in H0_SHAPES:
        got = check_rigid(dev, cin, cout, 0, 5, impl=impl, report=report)
        assert tuple(got.shape) == (0, cout)
    ops = _ops(impl)
    g = geometry(0, 5)
    q, s, inds = _dev(g, dev)
    assert tuple(ops.kpconv_weighted(q, s, inds, _features(g, 16).to(dev), g["kp"].to(dev), EXTENT, 1).shape) == (0, R.K_POINTS * 16)


# ---- ops.kpconv_deformable -------------------------------------------------------------------------------------------------------------
def _deform_inputs(cin, h, modulated, nq=33, cout=32):
    g = geometry(nq, h, seed=1)
    x, kp = _features(g, cin), g["kp"]
    rng = g["rng"]
    od = 60 if modulated else 45
    wf64 = R.weighted(*_dbl(g), x.double(), kp.double(), EXTENT, 1)
    ow = f32(rng.standard_normal((R.K_POINTS * cin, od)))
    ow = ow * (0.125 * _pow2_scale(float((wf64.flatten(1) @ ow.double()).abs().max())))     # offsets up to half an extent
    ob = f32(rng.normal(0, 0.05, od))
    w, b = _weights(g, cin, cout, wf64, True)
    return g, x, kp, w, b, ow, ob


def check_deformable(dev, cin, h, modulated, impl=None, report=_print):
    ops = _ops(impl)
    g, x, kp, w, b, ow, ob = _deform_inputs(cin, h, modulated)
    _assert_shares(g)
    r64, off64 = R.deformable(*_dbl(g), x.double(), kp.double(), EXTENT, w.double(), b.double(), ow.double(), ob.double(), 1, SLOPE)
    r32, _ = R.deformable(g["q"], g["s"], g["inds"], x, kp, EXTENT, w, b, ow, ob, 1, SLOPE)
    name = "deformable cin=%d h=%d modulated=%d" % (cin, h, modulated)
    if impl is None:
        report(name=name, arm=weighted_arm(cin, 33, h, NS, 1, deformable=True))
    q, s, inds = _dev(g, dev)
    got = ops.kpconv_deformable(q, s, inds, x.to(dev), kp.to(dev), w.to(dev), b.to(dev), EXTENT, ow.to(dev), ob.to(dev), act=1,
                                slope=SLOPE).cpu()
    judge(report, name, got, r64, r32)
    assert 0.25 <= float(off64[:, :45].abs().max()) <= 1.0
    rigid = R.conv(*_dbl(g), x.double(), kp.double(), EXTENT, 1, w.double(), b.double(), 1, SLOPE)
    assert float((rigid - r64).abs().max()) > 0.05, "the offsets move the result"
    if modulated:
        plain = R.conv(*_dbl(g), x.double(), kp.double(), EXTENT, 1, w.double(), b.double(), 1, SLOPE,
                       offsets=off64[:, :45].reshape(-1, R.K_POINTS, 3) * EXTENT)
        assert float((plain - r64).abs().max()) > 0.05, "the modulations move the result"
    rest = R.activation(b, 1, SLOPE)
    for r, kind in enumerate(g["kinds"]):
        if kind == "all_shadow":
            assert torch.equal(got[r], rest), (name, "all-shadow row", r)


DEFORM_REFUSAL = "ml3d_kpconv_deformable failed: unsupported configuration (-4)"      # = _abi.check's text for ML3D_E_UNSUPPORTED


def check_deformable_refusals(dev):
    from ml3d import ops
    for cin, influence in ((64, 0), (64, 2), (24, 1)):
        g, x, kp, w, b, ow, ob = _deform_inputs(cin, 9, False)
        q, s, inds = _dev(g, dev)
        refused(lambda: ops.kpconv_deformable(q, s, inds, x.to(dev), kp.to(dev), w.to(dev), b.to(dev), EXTENT, ow.to(dev), ob.to(dev),
                                              influence=influence), "deformable cin=%d influence=%d" % (cin, influence), DEFORM_REFUSAL)


# ---- the adjoint: ops.kpconv_weighted_backward (atomics: no bit-for-bit claim) ---------------------------------------------------------
EVERYONES, NOBODYS = 1, 2                                  # support rows: a neighbour of every query / of none


def check_adjoint(dev, cin, h, influence=1, nq=33, impl=None, report=_print):
    """dx against float64; support row EVERYONES is listed in column 0 of every query (h >= 2; the heaviest collision of the atomic adds),
    support row NOBODYS by nobody (exactly zero); sum wf(x) . g against sum x . adj(g), both accumulated in float64 from the
    kernels' outputs: the two differ by at most tol_wf sum |g| + tol_dx sum |x| when either kernel keeps its own bound."""
    ops = _ops(impl)
    g = geometry(nq, h, seed=2)
    ns = g["s"].shape[0]
    inds = g["inds"].clone()
    inds[inds == NOBODYS] = NOBODYS + 1
    if h >= 2:
        inds[:, 0] = EVERYONES
    g["inds"] = inds
    _assert_shares(g)
    x, kp = _features(g, cin), g["kp"]
    dwf = f32(g["rng"].standard_normal((nq, R.K_POINTS, cin)))
    r64 = R.adjoint(*_dbl(g), dwf.double(), kp.double(), EXTENT, influence)
    k = _pow2_scale(float(r64.abs().max()))
    dwf, r64 = dwf * k, r64 * k
    r32 = R.adjoint(g["q"], g["s"], inds, dwf, kp, EXTENT, influence)
    name = "adjoint cin=%d nq=%d h=%d influence=%d" % (cin, nq, h, influence)
    q, s, indsd = _dev(g, dev)
    got = ops.kpconv_weighted_backward(q, s, indsd, dwf.reshape(nq, -1).contiguous().to(dev), cin, kp.to(dev), EXTENT, influence).cpu()
    judge(report, name, got, r64, r32)
    assert 0.5 <= float(r64.abs().max()) <= 20
    assert tuple(got.shape) == (ns, cin) and not bool(got[NOBODYS].any()) and not bool(r64[NOBODYS].any())
    wf64 = R.weighted(*_dbl(g), x.double(), kp.double(), EXTENT, influence)
    wf32 = R.weighted(g["q"], g["s"], inds, x, kp, EXTENT, influence)
    wf = ops.kpconv_weighted(q, s, indsd, x.to(dev), kp.to(dev), EXTENT, influence).cpu().view(nq, R.K_POINTS, cin)
    tol_wf = max(1e-5, 4.0 * float((wf32.double() - wf64).abs().max()))
    tol_dx = max(1e-5, 4.0 * float((r32.double() - r64).abs().max()))
    lhs, rhs = float((wf.double() * dwf.double()).sum()), float((x.double() * got.double()).sum())
    bound = tol_wf * float(dwf.double().abs().sum()) + tol_dx * float(x.double().abs().sum())
    report(name=name + " <wf(x), g> = <x, adj(g)>", max_abs_delta=abs(lhs - rhs), tol=bound, ref_abs_max=abs(float((wf64 * dwf.double()).sum())))
    assert np.isfinite(lhs) and np.isfinite(rhs) and abs(lhs - rhs) <= bound, (name, lhs, rhs, bound)


# ---- pools: ops.gather_pool, bit for bit ----------------------------------------------------------------------------------------------
def pool_inputs(c, h, seed=0):
    """ns = 300 rows of features, the first 12 all NEGATIVE; 41 queries: the rows of ``neighbour_rows`` from row 4 on, row 0 lists
    negative rows only (no shadow: the maximum is negative), row 1 the same with one shadow (the maximum is 0.0), row 2 shadows
    only, row 3 a shadow in column 0 before real columns."""
    rng = np.random.default_rng([c, h, seed, 7])
    ns, nq = NS, 41
    x = rng.standard_normal((ns, c)).astype(np.float32)
    x[:12] = -np.abs(x[:12]) - np.float32(0.01)
    inds, _ = neighbour_rows(rng, nq, ns, h, np.arange(12))
    inds[0] = rng.integers(0, 12, h)
    inds[1] = inds[0]
    inds[1, h // 2] = ns
    inds[2] = 2 ** 31 - 1
    inds[3] = rng.integers(0, ns, h)
    inds[3, 0] = ns + 5
    return x, inds


def check_pool(dev, c, h, misaligned=False, impl=None, report=_print):
    ops = _ops(impl)
    x, inds = pool_inputs(c, h)
    want = {"max": R.max_pool(x, inds), "closest": R.closest_pool(x, inds)}
    assert (want["max"][0] < 0).all() and (want["max"][1] == 0).all() and (want["max"][2] == 0).all() and (want["closest"][3] == 0).all()
    assert (want["closest"][0] < 0).all()
    xt = torch.from_numpy(x)
    xd = _misaligned(xt, dev) if misaligned else xt.to(dev)
    for mode in ("max", "closest"):
        if impl is None:
            report(name="pool c=%d h=%d mode=%s%s" % (c, h, mode, " misaligned" if misaligned else ""),
                   arm=pool_arm(c, mode, aligned=not misaligned))
        got = ops.gather_pool(xd, torch.from_numpy(inds).to(dev), mode).cpu()
        assert same_bits(got, torch.from_numpy(want[mode])), ("pool", c, h, mode, misaligned)


# ---- the host rules of kpconv.hip, restated -------------------------------------------------------------------------------------------
MFMA_CIN = {16: 1, 32: 2, 64: 4, 128: 8, 256: 16}         # launch_weighted: cin -> NT of kp_agg_mfma<NT>
DEFORM_ONLY_CIN = 512                                     # agg_mfma_ok: two slices of kp_agg_mfma<16>, deformable only
KPW = ((16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (256, 64, 4), (512, 64, 8))      # cin <= limit -> kp_weighted<G, J>
SMALL_CIN_MAX, FUSED_COUT_STEP, FUSED_COUT_MAX = 5, 32, 128
AGG_MFMA_GRID, AGG_MFMA_WAVES = 256 * 8, 4                # launch_agg_mfma: grid cap, queries (waves) per workgroup
KF_TQ, AGG_GEMM32_GRID = 16, 256 * 4                      # kp_agg_gemm32: queries per tile, grid cap
SMALL_FUSED_LDS_OPT_IN = 48 * 1024                        # launch_small_fused raises the limit ABOVE this many bytes

RULE_TEXT = (          # each restated rule beside the text of kpconv.hip it restates (whitespace-insensitive)
    "return (c == 16 || c == 32 || c == 64 || c == 128 || c == 256 || (c == 512 && a.off)) && a.h > 0 && a.ns > 0 &&",
    "((((uintptr_t)a.x) | ((uintptr_t)a.wf)) & 15) == 0;",
    "case 16: launch_agg_mfma<1>(a, st); break;", "case 32: launch_agg_mfma<2>(a, st); break;",
    "case 64: launch_agg_mfma<4>(a, st); break;", "case 128: launch_agg_mfma<8>(a, st); break;",
    "case 256: launch_agg_mfma<16>(a, st); break;",
    "if (c == 1) hipLaunchKernelGGL(kp_weighted_small<1>", "else if (c == 5) hipLaunchKernelGGL(kp_weighted_small<5>",
    "else if (c <= 16) launch_kpw<16, 1>(a, st);", "else if (c <= 32) launch_kpw<32, 1>(a, st);",
    "else if (c <= 64) launch_kpw<64, 1>(a, st);", "else if (c <= 128) launch_kpw<64, 2>(a, st);",
    "else if (c <= 256) launch_kpw<64, 4>(a, st);", "else if (c <= 512) launch_kpw<64, 8>(a, st);",
    "return a.cin <= 5 && o.cout % 32 == 0 && o.cout <= 128 &&",
    "const int nv = o.cout / 32;", "if (sm > 48 * 1024)",
    "const size_t sm = sizeof(float) * ((size_t)KP_K * CIN * o.cout + 4 * 8 * (KP_WP * CIN + 4));",
    "return a.cin == 32 && o.cout == 32 && !a.off && a.h > 0 && a.ns > 0 && a.nq > 0 && kp_rows_32bit(a) &&",
    "((((uintptr_t)a.x) & 15) | (((uintptr_t)o.out) & 7)) == 0;",
    "if (kp_influence_mode != 1 || !agg_mfma_ok(a)) return ML3D_E_UNSUPPORTED;",
    "} else if (max_neighbors > 0 && small_fused_ok(a, ko)) {", "if (max_neighbors > 0 && agg_gemm32_ok(a, ko)) {",
    "int64_t nb = ((a.nq + 3) / 4 + 7) / 8 * 8;", "if (nb > 256 * 8) nb = 256 * 8;",
    "constexpr int KF_TQ = 16;", "int64_t nb = (tiles + 7) / 8 * 8;", "if (nb > 256 * 4) nb = 256 * 4;",
    "if ((channels & 3) == 0 && (((uintptr_t)features | (uintptr_t)out) & 15) == 0 &&",
    "if (a.off) { hipLaunchKernelGGL((kp_agg_mfma<NT, 1, true>)",
)


def kpconv_source():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, os.pardir, "open3d-ml_amd", "csrc", "kpconv.hip")) as f:
        return re.sub(r"\s+", "", f.read())


def assert_rules_are_the_sources():
    src = kpconv_source()
    for text in RULE_TEXT:
        assert re.sub(r"\s+", "", text) in src, "kpconv.hip no longer says: " + text


def agg_mfma_queries_per_wave(nq):
    """(fewest, most) queries a working wave of kp_agg_mfma walks, whether the last XCD's share is shorter than the others'
    (agg_gemm32_tiles_per_workgroup: the same for the tiles of a workgroup of kp_agg_gemm32, and whether the last tile is partial)."""
    grid = min(AGG_MFMA_GRID, ((nq + 3) // 4 + 7) // 8 * 8)
    per_xcd, stride = (nq + 7) // 8, (grid >> 3) * AGG_MFMA_WAVES
    counts = [len(range(t, max(0, min(per_xcd, nq - x * per_xcd)), stride)) for x in range(8) for t in range(stride)]
    return min(c for c in counts if c), max(counts), nq - 7 * per_xcd != per_xcd


def agg_gemm32_tiles_per_workgroup(nq):
    tiles = (nq + KF_TQ - 1) // KF_TQ
    grid = min(AGG_GEMM32_GRID, (tiles + 7) // 8 * 8)
    per_xcd, stride = (tiles + 7) // 8, grid >> 3
    counts = [len(range(t, max(0, min(per_xcd, tiles - x * per_xcd)), stride)) for x in range(8) for t in range(stride)]
    return min(c for c in counts if c), max(counts), tiles - 7 * per_xcd != per_xcd, nq % KF_TQ != 0


def weighted_arm(cin, nq, h, ns, influence, aligned=True, deformable=False):
    """launch_weighted (features and wf 16-byte aligned = ``aligned``; the rows fit 32-bit offsets at every shape of the tables)."""
    mfma = (cin in MFMA_CIN or (cin == DEFORM_ONLY_CIN and deformable)) and h > 0 and ns > 0 and nq > 0 and aligned
    if deformable:
        assert mfma and influence == 1, "refused"
        return "kp_agg_mfma<%d,deformable>" % MFMA_CIN.get(cin, 16)
    if mfma:
        return "kp_agg_mfma<%d,%d>" % (MFMA_CIN[cin], influence)
    if cin <= SMALL_CIN_MAX:
        return "kp_weighted_small<%d>" % cin
    for limit, g_, j in KPW:
        if cin <= limit:
            return "kp_weighted<%d,%d>" % (g_, j)
    raise AssertionError("unsupported")


def small_fused_lds_bytes(cin, cout):
    return 4 * (R.K_POINTS * cin * cout + 4 * 8 * (16 * cin + 4))


def rigid_arm(cin, cout, nq, h, ns, influence, aligned=True):
    """kpconv_run (weights, bias and out come from the allocator: 16-byte aligned; ``aligned``: the feature matrix)."""
    if nq == 0:
        return "nothing"
    if h > 0 and cin <= SMALL_CIN_MAX and cout % FUSED_COUT_STEP == 0 and cout <= FUSED_COUT_MAX:
        return "kp_small_fused<%d,%d>" % (cin, cout // FUSED_COUT_STEP)
    if h > 0 and cin == 32 and cout == 32 and ns > 0 and aligned:
        return "kp_agg_gemm32<%d>" % influence
    return weighted_arm(cin, nq, h, ns, influence, aligned) + " + gemm"


def pool_arm(c, mode, aligned=True):
    return "%s %s" % ("gather_pool_v4" if c % 4 == 0 and aligned else "gather_pool_k", mode)


# ---- the case tables: (group, body, kwargs) -> test ids; every runner walks CASES ---------------------------------------------------
CASES = []


def _case(group, body, **kw):
    CASES.append(dict(group=group, body=body, kw=kw, id=",".join("%s=%s" % (k, v) for k, v in kw.items())))


for _cin in AGG_CIN:
    for _h in AGG_H:
        _case("agg_cin", "weighted", cin=_cin, nq=33, h=_h, alone=ALONE_ROWS)
for _cin in AGG_MISALIGNED_CIN:
    _case("agg_misaligned", "weighted", cin=_cin, nq=33, h=33, misaligned=True, alone=ALONE_ROWS)
for _cin in AGG_INFLUENCE_CIN:
    for _i in (0, 1, 2):
        _case("agg_influence", "weighted", cin=_cin, nq=33, h=33, influence=_i, alone=ALONE_ROWS)
for _cin in AGG_WIDTH_CIN:
    for _h in H_WIDTHS:
        _case("agg_width", "weighted", cin=_cin, nq=33, h=_h, alone=ALONE_ROWS)
for _cin in AGG_TAIL_CIN:
    for _nq in NQ_TAILS:
        _case("agg_tail", "weighted", cin=_cin, nq=_nq, h=9, alone=ALONE_ROWS if _nq == 33 else ())
_case("agg_long", "weighted", **AGG_LONG)
for _cin in FUSED_CIN:
    for _cout in FUSED_COUT:
        _case("fused_shape", "rigid", cin=_cin, cout=_cout, nq=33, h=9)
for _cin, _cout in FUSED_FULL:
    for _i in (0, 1, 2):
        for _b in (False, True):
            for _a in (0, 1, 2):
                _case("fused_full", "rigid", cin=_cin, cout=_cout, nq=33, h=9, influence=_i, bias=_b, act=_a)
for _h in FUSED_H:
    _case("fused_width", "rigid", cin=4, cout=64, nq=33, h=_h)
for _nq in NQ_TAILS:
    _case("fused_tail", "rigid", cin=2, cout=32, nq=_nq, h=9)
for _cin, _cout in FUSED_LEAVING:
    _case("fused_leaving", "rigid", cin=_cin, cout=_cout, nq=33, h=9)
for _i in (0, 1, 2):
    for _a in (0, 1, 2):
        for _b in (True, False):
            _case("b32_full", "rigid", cin=32, cout=32, nq=33, h=9, influence=_i, bias=_b, act=_a)
for _nq in B32_NQ:
    _case("b32_tail", "rigid", cin=32, cout=32, nq=_nq, h=9)
for _h in B32_H:
    _case("b32_width", "rigid", cin=32, cout=32, nq=33, h=_h)
_case("b32_long", "rigid", cin=32, cout=32, **B32_LONG)
_case("b32_leaving", "rigid", cin=32, cout=48, nq=33, h=9)
_case("b32_leaving", "rigid", cin=32, cout=32, nq=33, h=9, misaligned=True)
for _cin in GEMM_CIN:
    for _cout in GEMM_COUT:
        _case("agg_gemm", "rigid", cin=_cin, cout=_cout, nq=257, h=33)
        if _cin >= 64:
            _case("agg_gemm", "rigid", cin=_cin, cout=_cout, nq=257, h=33, packed=True)
for _cin, _cout in H0_SHAPES:
    _case("h0", "h0", cin=_cin, cout=_cout)
_case("nq0", "nq0")
for _cin, _h, _m in DEFORM_CASES:
    _case("deformable", "deformable", cin=_cin, h=_h, modulated=_m)
for _cin in ADJ_CIN:
    _case("adjoint", "adjoint", cin=_cin, h=33)
for _i in (0, 2):
    _case("adjoint", "adjoint", cin=24, h=33, influence=_i)
for _h in ADJ_H:
    if _h != 33:
        _case("adjoint", "adjoint", cin=24, h=_h)
for _c in POOL_C:
    for _h in POOL_H:
        _case("pool", "pool", c=_c, h=_h)
for _c in POOL_MISALIGNED_C:
    _case("pool", "pool", c=_c, h=9, misaligned=True)

BODIES = dict(weighted=check_weighted, rigid=check_rigid, h0=check_h0, nq0=check_nq0, deformable=check_deformable,
              adjoint=check_adjoint, pool=check_pool)
GROUPS = tuple(dict.fromkeys(c["group"] for c in CASES))
FLOAT_BODIES = ("weighted", "rigid", "deformable", "adjoint")


def cases_of(group):
    return [c for c in CASES if c["group"] == group]


def run_case(dev, case, impl=None, report=_print):
    return BODIES[case["body"]](dev, impl=impl, report=report, **case["kw"])


def arms_of(case):
    """The kernels of kpconv.hip a case reaches on the product, by the restated rules."""
    kw, body = case["kw"], case["body"]
    al = not kw.get("misaligned", False)
    if body == "weighted":
        arms = [weighted_arm(kw["cin"], kw["nq"], kw["h"], NS, kw.get("influence", 1), al)]
        if kw["nq"] == AGG_LONG["nq"] and arms[0].startswith("kp_agg_mfma"):
            lo, hi, ragged = agg_mfma_queries_per_wave(kw["nq"])
            arms += ["kp_agg_mfma long walk"] * (lo == 1 and hi == 2 and ragged)
        return arms
    if body == "rigid":
        arms = [rigid_arm(kw["cin"], kw["cout"], kw["nq"], kw["h"], NS, kw.get("influence", 1), al)]
        if kw["nq"] == B32_LONG["nq"] and arms[0].startswith("kp_agg_gemm32"):
            lo, hi, ragged, partial = agg_gemm32_tiles_per_workgroup(kw["nq"])
            arms += ["kp_agg_gemm32 long walk"] * (lo == 1 and hi == 2 and ragged and partial)
        return arms
    if body == "deformable":
        return [weighted_arm(kw["cin"], 33, kw["h"], NS, 1, deformable=True), weighted_arm(kw["cin"], 33, kw["h"], NS, 1) + " + gemm"]
    if body == "adjoint":
        return ["kp_weighted_adjoint", weighted_arm(kw["cin"], 33, kw["h"], NS, kw.get("influence", 1))]
    if body == "pool":
        return [pool_arm(kw["c"], m, al) for m in ("max", "closest")]
    return []


REQUIRED_ARMS = tuple(
    ["kp_weighted_small<%d>" % c for c in range(1, 6)] + ["kp_small_fused<%d,%d>" % (c, nv) for c in range(1, 6) for nv in range(1, 5)] +
    ["kp_weighted<%d,%d>" % gj for gj in ((16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8))] +
    ["kp_agg_mfma<%d,%s>" % (nt, m) for nt in (1, 2, 4, 8, 16) for m in (0, 1, 2, "deformable")] +
    ["kp_agg_gemm32<%d>" % m for m in (0, 1, 2)] + ["%s %s" % (k, m) for k in ("gather_pool_k", "gather_pool_v4") for m in ("max", "closest")] +
    ["kp_weighted_adjoint", "kp_agg_mfma long walk", "kp_agg_gemm32 long walk"])


def arms_table():
    """arm -> ids of the cases that reach it (``+ gemm`` arms count for their aggregation kernel)."""
    table = {}
    for c in CASES:
        for arm in arms_of(c):
            table.setdefault(arm.replace(" + gemm", ""), []).append("%s[%s]" % (c["group"], c["id"]))
    return table
