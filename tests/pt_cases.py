"""Shared bodies of the PointTransformer op tests (tests/test_emulated_pointtransformer.py runs the small ones on CPU tensors
against the host emulation of csrc/ptransformer.hip, tests/test_gpu_pointtransformer_ops.py all of them on the MI355X), like
tests/multicloud_cases.py.  Every body takes the device and a ``report`` callback that receives the MEASURED figures of each
float comparison before it is asserted.

The one tolerance: every float comparison is against the direct formula of tests/pt_ref.py evaluated in FLOAT64 on CPU
tensors.  ``e32`` = max |formula in float32 - formula in float64| is the error of the reference ALONE at the case's own inputs;
the kernel passes when max |kernel - float64| <= max(1e-5, 4 e32): 1e-5 is what the emulator tests have always applied to
these ops, the factor 4 covers another summation order (MFMA in steps of 4, grouped sums) and another ``expf``.  Everything
else (FPS, clamping, row independence, determinism, k = 1, a = None, new_points) is compared for EQUALITY, bit for bit."""
import numpy as np
import torch

import pt_ref

ATTENTION_WIDTHS = (16, 48, 128, 256, 384, 512)          # every pt_attn_kernel<NS, NT> (NT = 1, 1, 1, 2, 4 as 3 tiles, 4) ...
NSAMPLES = (8, 16)                                       # ... x NS
ATTENTION_GRID = ((32, 8), (32, 16), (512, 16))          # n = 12 293: 6147 / 12 293 groups on a grid of 256 * 24 = 6144
DOWN_SHAPES = ((32, 64, 8), (256, 512, 16), (5, 3, 1), (29, 67, 16), (32, 64, 64))      # (c, c_out, nsample)
INTERP_SHAPES = ((13, 3), (512, 3), (64, 1), (32, 16))                                  # (c, k)
FPS_BOUNDARIES = (4096, 4097, 12288, 12289, 24577, 49153, 65536, 65537)                 # PER = 4 | 12 | 12 | 24 | 48 | 64 | 64 | workspace
FPS_FULL = (1, 2, 63, 64, 65, 1023, 1024, 1025)
BIG_N = 12293
CAP_ROWS = 32771                                         # x 512 channels = 16 778 752 outputs > 65 535 * 256 = 16 776 960


def _print(**kv):
    print(" ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items()), flush=True)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


def _dbl(x):
    if isinstance(x, dict):
        return {k: _dbl(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_dbl(v) for v in x)
    return x.double() if torch.is_tensor(x) and x.is_floating_point() else x


def _dev(x, dev):
    if isinstance(x, dict):
        return {k: _dev(v, dev) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_dev(v, dev) for v in x)
    return x.to(dev) if torch.is_tensor(x) else x


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def judge(report, name, got, ref64, ref32):
    """The tolerance of the module docstring: report the figures, then assert."""
    got = got.detach().cpu()
    err = float((got.double() - ref64).abs().max()) if got.numel() else 0.0
    e32 = float((ref32.double() - ref64).abs().max()) if got.numel() else 0.0
    tol = max(1e-5, 4.0 * e32)
    report(name=name, max_abs_delta=err, e32=e32, tol=tol, ref_abs_max=float(ref64.abs().max()) if got.numel() else 0.0)
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()) and err <= tol, (name, err, e32, tol)
    return err


def refused(fn, what, match="invalid argument"):
    try:
        fn()
    except RuntimeError as e:
        assert match in str(e), (what, e)
        return
    raise AssertionError("%s was accepted" % (what,))


def _in_chunks(fn, n, rows_per_chunk):
    return torch.cat([fn(range(lo, min(n, lo + rows_per_chunk))) for lo in range(0, n, rows_per_chunk)]) if n else fn(None)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
def centred_room(seed, n):
    p = pt_ref.room(seed, n)
    return torch.from_numpy((p - (p.min(0) + p.max(0)) / np.float32(2.0)).astype(np.float32))


def attention_inputs(c, ns, n, dev=None, neighbours="random", hidden_rows=None):
    """-> (qkv, points, idx, params, epilogue) on the CPU, as tests/test_emulated_pointtransformer.py draws them; the neighbour
    lists from ``ops.knn_search`` on ``dev`` or uniform in [0, n).  A fifth of the epilogue scales are negative."""
    from ml3d import ops
    from ml3d.ops import pointtransformer as P
    rng = np.random.default_rng([c, ns, n])
    p = centred_room(5, n)
    if neighbours == "knn":
        idx = ops.knn_search(p.to(dev), p.to(dev), ns).neighbors_index.cpu()
        assert int(idx.min()) >= 0 and int(idx.max()) < n
    else:
        idx = torch.from_numpy(rng.integers(0, n, (n, ns)).astype(np.int32))
    qkv = f32(rng.standard_normal((n, 3 * c)))
    a = pt_ref.random_attention_params(c, 7, P.attention_hidden_rows(c) if hidden_rows is None else hidden_rows)
    sign = np.where(rng.random(c) < 0.2, -1, 1)
    sign[c // 3] = -1
    ep = (f32(rng.uniform(0.6, 1.5, c) * sign), f32(rng.normal(0, 0.2, c)))
    return qkv, p, idx, a, ep


def attention_refs(qkv, p, idx, a, rows_per_chunk=256):
    """(float64, float32) formula WITHOUT the epilogue, in chunks of query rows (the [rows, nsample, c] float64 intermediates of
    a chunk stay below ~0.2 GB at c = 512, nsample = 16)."""
    n = idx.shape[0]
    qd, pd, ad = _dbl(qkv), _dbl(p), _dbl(a)
    r64 = _in_chunks(lambda rows: pt_ref.attention_formula(qd, pd, idx, ad, rows=rows), n, rows_per_chunk)
    r32 = _in_chunks(lambda rows: pt_ref.attention_formula(qkv, p, idx, a, rows=rows), n, rows_per_chunk)
    return r64, r32


def with_epilogue(ref, ep):
    """= what attention_formula(..., ep) appends, in the reference's own dtype."""
    s, t = (x.to(ref.dtype) for x in ep)
    return torch.relu(ref * s + t)


def run_attention(dev, qkv, p, idx, a, ep=None):
    from ml3d import ops
    return ops.pt_attention(qkv.to(dev), p.to(dev), idx.to(dev), _dev(a, dev), epilogue=None if ep is None else _dev(ep, dev)).cpu()


def _attention_case(dev, report, name, c, ns, n, neighbours):
    qkv, p, idx, a, ep = attention_inputs(c, ns, n, dev, neighbours)
    r64, r32 = attention_refs(qkv, p, idx, a)
    plain = run_attention(dev, qkv, p, idx, a)
    judge(report, "%s c=%d ns=%d n=%d plain" % (name, c, ns, n), plain, r64, r32)
    fused = run_attention(dev, qkv, p, idx, a, ep)
    judge(report, "%s c=%d ns=%d n=%d epilogue" % (name, c, ns, n), fused, with_epilogue(r64, ep), with_epilogue(r32, ep))
    if n >= 100:                                               # (the epilogue's ReLU cuts some outputs and passes others)
        assert float(with_epilogue(r64, ep).max()) > 0 and float((with_epilogue(r64, ep) == 0).double().mean()) > 0.1
    # determinism: the same call twice, bit for bit
    assert same_bits(run_attention(dev, qkv, p, idx, a), plain) and same_bits(run_attention(dev, qkv, p, idx, a, ep), fused)


def check_attention_widths(dev, c, ns, report=_print):
    """n = 333 (odd: the last wave of the 8-neighbour form is half empty), the level's own k-NN lists."""
    _attention_case(dev, report, "attention", c, ns, 333, "knn")


def check_attention_grid_stride(dev, c, ns, report=_print):
    """n = 12 293: more groups than the grid of 6144 workgroups, so a workgroup runs 2 - 3 iterations on the same LDS."""
    groups = (BIG_N + 16 // ns - 1) // (16 // ns)
    assert groups > 256 * 24
    _attention_case(dev, report, "attention_grid", c, ns, BIG_N, "random")


def check_attention_tiny(dev, report=_print):
    """n = 1 and n = 5: the lists are longer than the cloud (repeats; at n = 1 every neighbour is the query itself)."""
    for n in (1, 5):
        for ns in NSAMPLES:
            for c in (32, 256):
                _attention_case(dev, report, "attention_tiny", c, ns, n, "random")


def check_attention_clamping(dev, report=_print):
    """-1 and n + 5 in the list: bit-equal to the run with the list clamped into [0, n - 1], as the contract states."""
    for c, ns in ((48, 8), (48, 16), (256, 16)):
        n = 77
        qkv, p, idx, a, ep = attention_inputs(c, ns, n)
        wild = idx.clone()
        rng = np.random.default_rng(c + ns)
        mask = torch.from_numpy(rng.random((n, ns)))
        wild[mask < 0.15] = -1
        wild[mask > 0.85] = n + 5
        wild[n - 1, ns - 1], wild[0, 0] = n + 5, -1
        clamped = wild.clamp(0, n - 1)
        assert int((wild != clamped).sum()) > n
        got, want = run_attention(dev, qkv, p, wild, a, ep), run_attention(dev, qkv, p, clamped, a, ep)
        assert same_bits(got, want), (c, ns)
        r64, r32 = attention_refs(qkv, p, clamped, a)
        judge(report, "attention_clamped c=%d ns=%d n=%d epilogue" % (c, ns, n), got, with_epilogue(r64, ep), with_epilogue(r32, ep))


def check_attention_row_independence(dev, report=_print):
    """nsample = 8, every index < n - 1: rows 0 .. n - 2 of the run on n points are bit-equal to the run on the first n - 1
    points (n even and odd: the dropped row is the second / the only query of the last wave)."""
    for c in (32, 256):
        for n in (333, 334):
            qkv, p, idx, a, ep = attention_inputs(c, 8, n)
            idx = idx.clamp(max=n - 2)
            full = run_attention(dev, qkv, p, idx, a)
            head = run_attention(dev, qkv[:n - 1].contiguous(), p[:n - 1].contiguous(), idx[:n - 1].contiguous(), a)
            assert same_bits(full[:n - 1], head), (c, n)


def check_attention_refusals(dev):
    """c = 24, c = 528, nsample = 12, an epilogue scale without its shift: RuntimeError from the wrapper, and the C entry
    returns -1 on the host, before any launch (the output buffer keeps its fill)."""
    from ml3d import _abi
    from ml3d.ops import _gates
    from ml3d.ops import pointtransformer as P
    L = _abi.get()
    n = 40

    def call(c, ns, rows, ep_scale, ep_shift):
        qkv, p, idx, a, ep = attention_inputs(c, ns, n, hidden_rows=rows)
        qkv, p, idx, a, ep = _dev((qkv, p, idx, a, ep), dev)
        e = (ep[0] if ep_scale else None, ep[1] if ep_shift else None)
        # (c = 528 needs more hidden rows than the wrapper's table knows: its own shape check refuses first)
        refused(lambda: P.pt_attention(qkv, p, idx, a, epilogue=None if e == (None, None) else e), (c, ns, ep_scale, ep_shift),
                "invalid argument" if c <= 512 else "w_w1 has shape")
        out = torch.full((n, c), -7.0, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = L.ml3d_pt_attention(qkv.data_ptr(), p.data_ptr(), idx.data_ptr(), n, c, ns, *[a[k].data_ptr() for k in P.ATTENTION_KEYS],
                                     *[None if t is None else t.data_ptr() for t in e], out.data_ptr(), _gates._stream())
        assert rc == -1 and bool((out.cpu() == -7.0).all()), (c, ns, rc)

    call(24, 8, 16, False, False)
    call(528, 16, 80, False, False)
    call(32, 12, 16, False, False)
    call(32, 8, 16, True, False)
    call(32, 16, 16, False, True)


# ---- TransitionDown -----------------------------------------------------------------------------------------------------------------
def down_inputs(c, cout, ns, n, seed):
    """Weights at the magnitudes of the pseudo-trained model; about a fifth of the scales negative; min(4, c_out - 1) channels
    with a shift of -1000, so that every candidate of theirs is negative and the output is the 0 of the ReLU."""
    rng = np.random.default_rng([c, cout, ns, seed])
    feat = f32(np.abs(rng.standard_normal((n, c))))
    w = rng.uniform(-1, 1, (3 + c, cout)) * 1.6 / np.sqrt(3 + c)
    sc = rng.uniform(0.6, 1.5, cout) * np.where(rng.random(cout) < 0.2, -1, 1)
    sh = rng.normal(0, 0.2, cout)
    dead = rng.choice(cout, min(4, cout - 1), replace=False)
    sh[dead] = -1000.0
    if cout >= 8:
        sc[dead[0]] = -abs(sc[dead[0]])                    # a dead channel with a negative scale among them
        assert int((sc < 0).sum()) >= 2
    return feat, f32(w[3:]), f32(w[:3]), f32(sc), f32(sh), np.sort(dead)


def down_refs(feat, p, samp, nbr, wft, wx, sc, sh, rows_per_chunk=4096):
    m = nbr.shape[0]
    d = _dbl((feat, p, samp, nbr, wft, wx, sc, sh))
    r64 = _in_chunks(lambda rows: pt_ref.transition_down_formula(*d, rows=rows), m, rows_per_chunk)
    r32 = _in_chunks(lambda rows: pt_ref.transition_down_formula(feat, p, samp, nbr, wft, wx, sc, sh, rows=rows), m, rows_per_chunk)
    return r64, r32


def run_down(dev, *args):
    from ml3d import ops
    newp, out = ops.pt_transition_down(*_dev(args, dev))
    return newp.cpu(), out.cpu()


def check_transition_down(dev, c, cout, ns, report=_print):
    from ml3d import ops
    n, m = 1000, 250
    p = centred_room(5, n)
    samp = ops.furthest_point_sampling(p.to(dev), [0, n], [0, m]).cpu()
    assert np.array_equal(samp.numpy(), pt_ref.fps_item(p.numpy(), m))
    nbr = ops.knn_search(p.to(dev), p[samp.long()].contiguous().to(dev), ns).neighbors_index.cpu()
    assert tuple(nbr.shape) == (m, ns) and int(nbr.min()) >= 0 and int(nbr.max()) < n
    feat, wft, wx, sc, sh, dead = down_inputs(c, cout, ns, n, 0)
    newp, got = run_down(dev, feat, p, samp, nbr, wft, wx, sc, sh)
    assert same_bits(newp, p[samp.long()])
    r64, r32 = down_refs(feat, p, samp, nbr, wft, wx, sc, sh)
    judge(report, "transition_down c=%d c_out=%d ns=%d" % (c, cout, ns), got, r64, r32)
    assert bool((r64[:, dead] == 0).all()) and bool((got[:, dead] == 0).all()), "the all-negative channels must be exactly 0"
    assert float(r64.max()) > 0
    newp2, got2 = run_down(dev, feat, p, samp, nbr, wft, wx, sc, sh)
    assert same_bits(got2, got) and same_bits(newp2, newp)


def check_transition_down_clamping_and_refusal(dev):
    from ml3d import ops
    c, cout, ns, n, m = 29, 67, 16, 300, 90
    rng = np.random.default_rng(17)
    p = centred_room(6, n)
    feat, wft, wx, sc, sh, _ = down_inputs(c, cout, ns, n, 1)
    samp = torch.from_numpy(rng.integers(0, n, m).astype(np.int32))
    nbr = torch.from_numpy(rng.integers(0, n, (m, ns)).astype(np.int32))
    samp[[0, 5, 40]] = -1
    samp[[1, 6, m - 1]] = n + 5
    mask = torch.from_numpy(rng.random((m, ns)))
    nbr[mask < 0.1] = -3
    nbr[mask > 0.9] = n + 7
    nbr[m - 1, ns - 1] = n + 7
    wild = run_down(dev, feat, p, samp, nbr, wft, wx, sc, sh)
    tame = run_down(dev, feat, p, samp.clamp(0, n - 1), nbr.clamp(0, n - 1), wft, wx, sc, sh)
    assert same_bits(wild[0], tame[0]) and same_bits(wild[1], tame[1])
    assert same_bits(wild[0], p[samp.clamp(0, n - 1).long()])
    wide = torch.zeros((m, 65), dtype=torch.int32)
    refused(lambda: ops.pt_transition_down(*_dev((feat, p, samp.clamp(0, n - 1), wide, wft, wx, sc, sh), dev)), "nsample = 65")


def check_transition_down_grid_cap(dev, report=_print):
    """m = 32 771 rows sampled with repetition from 2000 points, c_out = 512: 16 778 752 outputs on a grid capped at 65 535
    workgroups of 256, so the first 1792 threads take a second output."""
    c, cout, ns, n, m = 32, 512, 2, 2000, CAP_ROWS
    assert m * cout > 65535 * 256
    rng = np.random.default_rng(23)
    p = centred_room(7, n)
    feat, wft, wx, sc, sh, dead = down_inputs(c, cout, ns, n, 2)
    samp = torch.from_numpy(rng.integers(0, n, m).astype(np.int32))
    nbr = torch.from_numpy(rng.integers(0, n, (m, ns)).astype(np.int32))
    newp, got = run_down(dev, feat, p, samp, nbr, wft, wx, sc, sh)
    assert same_bits(newp, p[samp.long()])
    r64, r32 = down_refs(feat, p, samp, nbr, wft, wx, sc, sh)
    judge(report, "transition_down_grid_cap c=%d c_out=%d ns=%d m=%d" % (c, cout, ns, m), got, r64, r32)
    assert bool((got[:, dead] == 0).all()) and bool((r64[:, dead] == 0).all())


# ---- interpolation ------------------------------------------------------------------------------------------------------------------
def run_interp(dev, a, b, idx, d2):
    from ml3d import ops
    return ops.pt_interpolate(None if a is None else a.to(dev), b.to(dev), idx.to(dev), d2.to(dev)).cpu()


def interp_refs(a, b, idx, d2):
    return pt_ref.interpolate_formula(*_dbl((a, b, idx, d2))), pt_ref.interpolate_formula(a, b, idx, d2)


def check_interpolate(dev, c, k, report=_print):
    from ml3d import ops
    n, n_src = 1000, 250
    rng = np.random.default_rng([c, k])
    p = centred_room(5, n)
    samp = ops.furthest_point_sampling(p.to(dev), [0, n], [0, n_src]).cpu()
    src = p[samp.long()].contiguous()
    r = ops.knn_search(src.to(dev), p.to(dev), k, return_distances=True)
    idx, d2 = r.neighbors_index.cpu(), r.neighbors_distance.cpu()
    assert tuple(idx.shape) == (n, k) and int(idx.min()) >= 0 and int(idx.max()) < n_src and bool(torch.isfinite(d2).all())
    a, b = f32(np.abs(rng.standard_normal((n, c)))), f32(np.abs(rng.standard_normal((n_src, c))))
    got = run_interp(dev, a, b, idx, d2)
    judge(report, "interpolate c=%d k=%d" % (c, k), got, *interp_refs(a, b, idx, d2))
    # a query that IS a source point: distance 0, weight 1 up to the 1e-8 guard
    hit = int(samp[3])
    assert float(d2[hit, 0]) == 0.0 and int(idx[hit, 0]) == 3
    assert float((got[hit] - (a[hit] + b[3])).abs().max()) <= 1e-5
    if k == 1:                                                        # the weight is x / x
        assert same_bits(got, a + b[idx[:, 0].long()])
    # a = None: the interpolation alone, bit-equal to the call with a zero a
    alone = run_interp(dev, None, b, idx, d2)
    assert same_bits(alone, run_interp(dev, torch.zeros_like(a), b, idx, d2))
    judge(report, "interpolate c=%d k=%d a=None" % (c, k), alone, *interp_refs(None, b, idx, d2))
    # a query whose k distances are all 0: equal weights
    flat = d2.clone()
    flat[[7, n - 1]] = 0.0
    got0 = run_interp(dev, a, b, idx, flat)
    judge(report, "interpolate c=%d k=%d zero distances" % (c, k), got0, *interp_refs(a, b, idx, flat))
    for row in (7, n - 1):
        assert float((got0[row] - (a[row] + b[idx[row].long()].double().mean(0))).abs().max()) <= 1e-5
    assert same_bits(run_interp(dev, a, b, idx, d2), got)


def check_interpolate_short_item_and_refusal(dev, report=_print):
    """A source item of two points with k = 3: knn_search pads the third column with -1 / +inf (include/ml3d_hip.h), the
    interpolation then equals the one over the two real neighbours."""
    from ml3d import ops
    rng = np.random.default_rng(29)
    c, n = 24, 37
    src = f32(rng.standard_normal((2, 3)))
    q = f32(rng.standard_normal((n, 3)))
    q[5] = src[1]
    r = ops.knn_search(src.to(dev), q.to(dev), 3, return_distances=True)
    idx, d2 = r.neighbors_index.cpu(), r.neighbors_distance.cpu()
    assert bool((idx[:, 2] == -1).all()) and bool((d2[:, 2] == float("inf")).all())
    assert bool((idx[:, :2] >= 0).all()) and bool((idx[:, :2] < 2).all()) and bool(torch.isfinite(d2[:, :2]).all())
    a, b = f32(rng.standard_normal((n, c))), f32(rng.standard_normal((2, c)))
    got = run_interp(dev, a, b, idx, d2)
    two = (idx[:, :2].contiguous(), d2[:, :2].contiguous())
    judge(report, "interpolate short item c=%d k=3" % c, got, *interp_refs(a, b, *two))
    wide = ops.knn_search(q.to(dev), q.to(dev), 17, return_distances=True)
    refused(lambda: ops.pt_interpolate(a.to(dev), f32(rng.standard_normal((n, c))).to(dev), wide.neighbors_index, wide.neighbors_distance),
            "k = 17")


def check_interpolate_grid_cap(dev, report=_print):
    """n = 32 771, c = 512: 16 778 752 outputs on a grid capped at 65 535 workgroups of 256."""
    from ml3d import ops
    c, k, n, n_src = 512, 3, CAP_ROWS, 500
    assert n * c > 65535 * 256
    rng = np.random.default_rng(31)
    p, src = centred_room(8, n), centred_room(9, n_src)
    r = ops.knn_search(src.to(dev), p.to(dev), k, return_distances=True)
    idx, d2 = r.neighbors_index.cpu(), r.neighbors_distance.cpu()
    a, b = f32(np.abs(rng.standard_normal((n, c), dtype=np.float32))), f32(np.abs(rng.standard_normal((n_src, c))))
    got = run_interp(dev, a, b, idx, d2)
    judge(report, "interpolate_grid_cap c=%d k=%d n=%d" % (c, k, n), got, *interp_refs(a, b, idx, d2))


# ---- furthest point sampling: exact ---------------------------------------------------------------------------------------------------
def run_fps(dev, pts, rs, nrs):
    from ml3d import ops
    out = ops.furthest_point_sampling(torch.from_numpy(pts).to(dev), [int(v) for v in rs], [int(v) for v in nrs])
    assert out.dtype == torch.int32
    return out.cpu().numpy()


def _fps_exact(dev, pts, rs, nrs, twice=True):
    want = pt_ref.fps(pts, rs, nrs)
    got = run_fps(dev, pts, rs, nrs)
    assert got.shape == want.shape and np.array_equal(got, want), int(np.argmax(got != want))
    if twice:
        assert np.array_equal(run_fps(dev, pts, rs, nrs), got), "the same call twice"
    return got


def check_fps_class_boundary(dev, length):
    """One launch class per call (chosen by the LONGEST item): [3 points, m = 3], an empty item, the long item with 12 - 32
    picks, [65 points, m = 65] -- the short items ride in the long item's class (sentinel slots, clamped loads)."""
    picks = 12 + length % 21
    lens, ms = [3, 0, length, 65], [3, 0, picks, 65]
    rs, nrs = np.concatenate(([0], np.cumsum(lens))), np.concatenate(([0], np.cumsum(ms)))
    pts = pt_ref.room(length, int(rs[-1]))
    got = _fps_exact(dev, pts, rs, nrs)
    assert got[0] == 0 and got[3] == 3 and got[3 + picks] == 3 + length
    assert sorted(got[:3].tolist()) == [0, 1, 2] and sorted(got[3 + picks:].tolist()) == list(range(3 + length, 68 + length))


def check_fps_workspace_form(dev):
    """Two items longer than 65 536 points in one call: the second item's minima sit at a non-zero base of the workspace."""
    lens, ms = [65537, 70001], [16, 16]
    rs, nrs = np.concatenate(([0], np.cumsum(lens))), np.concatenate(([0], np.cumsum(ms)))
    got = _fps_exact(dev, pt_ref.room(11, int(rs[-1])), rs, nrs)
    assert got[0] == 0 and got[16] == 65537 and got[16:].min() >= 65537


def lattice(side=17, seed=13):
    g = np.arange(side, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))])


def check_fps_dense_ties(dev):
    """The 17 x 17 x 17 integer lattice in a seeded random order, 150 picks: most picks are exact float32 ties between points of
    different lanes, waves and registers, so every stage of the reduction decides ties (the lowest index wins)."""
    pts = lattice()
    assert pts.shape == (4913, 3)
    want, ties = pt_ref.fps_item(pts, 150, return_ties=True)
    assert len(ties) >= 100, len(ties)
    got = _fps_exact(dev, pts, [0, len(pts)], [0, 150])
    assert np.array_equal(got, want)


def check_fps_full_samples(dev, twice=True):
    """m = n: a permutation of the item in the canonical order; each size alone and all of them as one batch; m = 1.
    ``twice``: repeat every call (the serial emulator, where a repeat shows nothing, spares the thousands of picks)."""
    rng = np.random.default_rng(37)
    clouds = [rng.random((n, 3), dtype=np.float32) for n in FPS_FULL]
    for p in clouds:
        n = len(p)
        got = _fps_exact(dev, p, [0, n], [0, n], twice)
        assert sorted(got.tolist()) == list(range(n)), n
    rs = np.concatenate(([0], np.cumsum([len(p) for p in clouds])))
    got = _fps_exact(dev, np.concatenate(clouds), rs, rs, twice)
    assert sorted(got.tolist()) == list(range(int(rs[-1])))
    got = _fps_exact(dev, np.concatenate(clouds[-2:]), [0, len(clouds[-2]), len(clouds[-2]) + len(clouds[-1])], [0, 1, 2])
    assert got.tolist() == [0, len(clouds[-2])]
