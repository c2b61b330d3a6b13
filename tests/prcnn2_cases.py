"""Shared bodies of the ``ml3d_roi_pool`` tests (PointRCNN stage 2, the pooling): tests/test_emulated_pointrcnn2_ops.py runs them
on CPU tensors against the host emulation of csrc/pointrcnn.hip, tests/test_gpu_pointrcnn2_ops.py on the MI355X,
tests/test_prcnn2_cases_can_fail.py against deliberately wrong stand-ins (every body takes the implementation under test as
``impl``; None = the product's ``ml3d.ops``).

``pool_idx`` and ``empty`` are compared for EQUALITY with the restatement of tests/prcnn2_ref.py, the feature columns bit for bit,
the five leading columns by ``pt_cases.judge`` against the float64 formula within max(1e-5, 4 e32).  The inputs make the
restatement alone decisive: in float64 every point is either EXACTLY on a bound (dyadic boxes with ry = 0: closed faces, the
prefilter's ``> 10``) or at least 1e-3 away from every face, from the 10 m prefilter and -- its score -- from
logit(score_thres); points that are not get redrawn while the inputs are built, no case is skipped."""
import itertools

import numpy as np
import torch

import prcnn2_ref
from pt_cases import _print, judge, refused, same_bits

POOL_N = (1, 63, 64, 65, 257, 700)
POOL_M = (1, 3)
POOL_B = (1, 3)
POOL_S = (1, 8, 64, 512)
POOL_C = (1, 5, 130)
ARMS = ("empty", "one", "s_minus_1", "s", "more")          # cnt of roi 0 of item 0; the other rois take the following arms
RYS = (0.0, np.pi / 2, -np.pi / 2, 3.0)
SCORE_THRES = 0.3
EXTRA_WIDTH = 1.0
MARGIN = 1e-3
SPECIAL = (63, 64, 255, 256)                               # hits at the wave / workgroup-step boundaries, and at n - 1
_COMBOS = tuple(itertools.product(POOL_M, POOL_B, POOL_C))


def pool_cases(n):
    """20 cases (b, m, s, c, arm) per n: every S x every arm, the 12 (M, B, C) triples dealt round."""
    out = []
    for si, s in enumerate(POOL_S):
        for ai, arm in enumerate(ARMS):
            m, b, c = _COMBOS[(si * len(ARMS) + ai + n) % len(_COMBOS)]
            out.append((b, m, s, c, arm))
    return out


def _ops(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _wanted(arm, s):
    return {"empty": 0, "one": 1, "s_minus_1": s - 1, "s": s, "more": s + max(2, s // 4)}[arm]


def pool_inputs(b, n, m, s, c, arm):
    """-> dict: xyz [b, n, 3], feat [b * n, c], scores [b, n], rois [b, m, 7], planned [b, m] hit counts, long (the item-0 roi whose
    half length exceeds the prefilter, or None), poison_from [b] (see ``check_pool``).  With m = 3: roi 1 of item 0 is 26 m long
    (ry = 0) with two decoys INSIDE its faces beyond the prefilter, roi 2 of the last item is an all-zero padding roi.  Rois with
    ry = 0 are dyadic and own up to three points exactly ON their bounds."""
    a0 = ARMS.index(arm)
    rng = np.random.default_rng([b, n, m, s, c, a0])
    rois = np.zeros((b, m, 7), np.float32)
    for i in range(b):
        for j in range(m):
            u = rng.uniform(0.8, 1.25, 3)
            box = np.array([-50 + 45 * j + rng.uniform(-2, 2), rng.uniform(0.5, 2), 20 + 10 * i + rng.uniform(-2, 2), 1.5 * u[0],
                            1.6 * u[1], 3.9 * u[2], RYS[(a0 + i * m + j) % 4]])
            if m == 3 and (i, j) == (0, 1):
                box[5], box[6] = 26.0, 0.0
            if box[6] == 0.0:
                box[:6] = np.round(box[:6] * 8) / 8
            rois[i, j] = box
    if m == 3:
        rois[b - 1, 2] = 0.0
    big = prcnn2_ref.enlarge(rois, EXTRA_WIDTH, np.float64)
    xyz = np.zeros((b, n, 3), np.float32)
    planned = np.zeros((b, m), np.int64)
    poison_from = np.full(b, n, np.int64)

    def background(k):
        return np.stack((rng.uniform(-70, 60, k), rng.uniform(-4, 6, k), rng.uniform(-15, 50, k)), 1)

    def inside(box, k, decoy=False):
        x, y, z, h, w, l, ry = box
        xr = rng.uniform(-0.9, 0.9, k) * min(l / 2, 10.5)
        if decoy:
            xr = rng.uniform(10.5, l / 2 - 0.5, k) * rng.choice((-1.0, 1.0), k)
        zr, yl = rng.uniform(-0.9, 0.9, k) * w / 2, rng.uniform(-0.9, 0.9, k) * h / 2
        ca, sa = np.cos(ry), np.sin(ry)
        return np.stack((x + xr * ca + zr * sa, (y - h / 2) + yl, z - xr * sa + zr * ca), 1)

    def on_bounds(box):
        x, y, z, h, w, l, _ = box
        hl = min(l / 2, prcnn2_ref.PREFILTER)
        cy = y - h / 2
        return np.array([[x, cy - h / 2, z - w / 2], [x + hl, cy, z], [x - hl, cy + h / 2, z + w / 2]])

    for i in range(b):
        free = list(range(n))
        owner = np.full(n, -1)                               # roi, -1 background, -2 decoy
        exact = np.zeros(n, bool)
        pts = background(n)

        def take(k, special=False, avoid=()):
            got = [p for p in SPECIAL + (n - 1,) if p in free][:k] if special else []
            got = list(dict.fromkeys(got))
            rest = [p for p in free if p not in got and p not in avoid]
            got += [int(p) for p in rng.choice(rest, k - len(got), replace=False)] if k > len(got) else []
            for p in got:
                free.remove(p)
            return got

        decoys = take(2, avoid=SPECIAL + (n - 1,)) if (m == 3 and i == 0 and n >= 8) else []
        for p in decoys:
            owner[p] = -2
        for j in range(m):
            k = min(_wanted(ARMS[(a0 + i + j) % len(ARMS)], s), len(free))
            planned[i, j] = k
            mine = take(k, special=(j == 0))
            owner[mine] = j
            if big[i, j, 6] == 0.0:
                for p, q in zip(sorted(mine)[:3], on_bounds(big[i, j])):
                    assert (q == q.astype(np.float32)).all()
                    pts[p], exact[p] = q, True
        pts[(owner != -1) & ~exact] = np.nan                    # drawn below by the owner's own sampler
        for _ in range(200):
            for j in range(m):
                sel = (owner == j) & ~exact
                pts[sel] = np.where(np.isnan(pts[sel]), inside(big[i, j], int(sel.sum())), pts[sel])
            sel = owner == -2
            if sel.any():
                pts[sel] = np.where(np.isnan(pts[sel]), inside(big[0, 1], int(sel.sum()), decoy=True), pts[sel])
            sel = owner == -1
            pts[sel] = np.where(np.isnan(pts[sel]), background(int(sel.sum())), pts[sel])
            pts = pts.astype(np.float32).astype(np.float64)
            bad = np.zeros(n, bool)
            for j in range(m):
                mg = prcnn2_ref.margins(pts, big[i, j])
                bad |= ~(((mg == 0) & exact) | (mg >= MARGIN))
                bad |= prcnn2_ref.in_box(pts, big[i, j], np.float64) != (owner == j)
            assert not (bad & exact).any(), "a point placed on a bound is decided exactly"
            if not bad.any():
                break
            pts[bad] = np.nan                                   # redrawn by the owner's own sampler
        else:
            raise AssertionError("no decisive cloud found")
        xyz[i] = pts
        full = [sorted(np.flatnonzero(owner == j))[s - 1] for j in range(m) if planned[i, j] >= s]
        if len(full) == m:                                      # every roi of the item is full: nothing behind its S-th hit matters
            poison_from[i] = max(full) + 1
    scores = rng.normal(0, 2, (b, n))
    logit = np.log(SCORE_THRES / (1 - SCORE_THRES))
    scores = np.where(np.abs(scores - logit) < 10 * MARGIN, scores + 0.1, scores).astype(np.float32)
    assert np.abs(scores.astype(np.float64) - logit).min() >= MARGIN
    feat = rng.normal(0, 1, (b * n, c)).astype(np.float32)
    return dict(xyz=xyz, feat=feat, scores=scores, rois=rois, planned=planned, poison_from=poison_from,
                long=(0, 1) if m == 3 else None, s=s)


def run_pool(dev, impl, xyz, feat, scores, rois, s):
    """Outputs pre-filled with a sentinel; ``feat`` may already be a (strided) tensor."""
    b, m = rois.shape[:2]
    feat = feat if torch.is_tensor(feat) else _t(feat, dev)
    out = (torch.full((b * m, s, 5 + feat.shape[1]), -7.0, dtype=torch.float32, device=dev),
           torch.full((b, m, s), -9, dtype=torch.int32, device=dev), torch.full((b, m), -9, dtype=torch.int32, device=dev))
    res = _ops(impl).roi_pool(_t(xyz, dev), feat, _t(scores, dev), _t(rois, dev), s, SCORE_THRES, EXTRA_WIDTH, out=out)
    return tuple(r.cpu().numpy() for r in res)


def _same(got, want, what):
    for g, w, part in zip(got, want, ("pts_input", "pool_idx", "empty")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part, g.shape, g.dtype)
        same = np.array_equal(g.view(np.int32), w.view(np.int32))
        assert same, (what, part, np.argwhere(g.view(np.int32) != w.view(np.int32))[:4].tolist())


def check_pool_case(dev, n, case, impl=None, report=_print):
    b, m, s, c, arm = case
    what = "roi_pool n=%d b=%d m=%d s=%d c=%d %s" % (n, b, m, s, c, arm)
    I = pool_inputs(b, n, m, s, c, arm)
    args = (I["xyz"], I["feat"], I["scores"], I["rois"])
    p64, idx, empty, count = prcnn2_ref.roi_pool(*args, s, SCORE_THRES, EXTRA_WIDTH, np.float64)
    p32, idx32, empty32, count32 = prcnn2_ref.roi_pool(*args, s, SCORE_THRES, EXTRA_WIDTH, np.float32)
    assert np.array_equal(idx, idx32) and np.array_equal(count, count32) and np.array_equal(p64[..., 3], p32[..., 3]), "decisive inputs"
    assert np.array_equal(count, I["planned"]), (what, count.tolist(), I["planned"].tolist())
    assert count[0, 0] == min(_wanted(arm, s), n - (2 if m == 3 and n >= 8 else 0)), (what, "the arm of roi 0")
    assert np.array_equal(empty, (count == 0).astype(np.int32))
    if count[0, 0] > 0:
        first = [p for p in SPECIAL + (n - 1,) if p < n][:count[0, 0]]
        assert set(first[:s]) <= set(np.flatnonzero(prcnn2_ref.in_box(I["xyz"][0], prcnn2_ref.enlarge(I["rois"], EXTRA_WIDTH)[0, 0])))
    if m == 3 and n >= 8:                                       # the decoys lie inside the long box's faces, beyond the prefilter
        big = prcnn2_ref.enlarge(I["rois"], EXTRA_WIDTH)[0, 1]
        cut = prcnn2_ref.in_box(I["xyz"][0], big, wrong=("no_prefilter",)) & ~prcnn2_ref.in_box(I["xyz"][0], big)
        assert big[5] / 2 > prcnn2_ref.PREFILTER and cut.sum() >= 2
        assert not I["rois"][b - 1, 2].any(), "the padding roi"
    got = run_pool(dev, impl, *args, s)
    assert got[0].dtype == np.float32 and got[0].shape == (b * m, s, 5 + c)
    assert np.array_equal(got[1], idx), (what, "pool_idx", np.argwhere(got[1] != idx)[:4].tolist())
    assert np.array_equal(got[2], empty), (what, "empty", got[2].tolist(), empty.tolist())
    judge(report, what, torch.from_numpy(got[0][..., :5]), torch.from_numpy(p64[..., :5]), torch.from_numpy(p32[..., :5]))
    assert np.array_equal(got[0][..., 5:].view(np.int32), p32[..., 5:].view(np.int32)), (what, "feature columns bit for bit")
    wide = torch.full((b * n, c + 9), 55.0, dtype=torch.float32)
    wide[:, 4:4 + c] = torch.from_numpy(I["feat"])
    _same(run_pool(dev, impl, I["xyz"], wide.to(dev)[:, 4:4 + c], I["scores"], I["rois"], s), got, (what, "strided feat"))
    if b > 1:
        alone = run_pool(dev, impl, I["xyz"][1:2], I["feat"][n:2 * n], I["scores"][1:2], I["rois"][1:2], s)
        _same(alone, (got[0][m:2 * m], got[1][1:2], got[2][1:2]), (what, "item 1 alone"))
    poisoned = False
    if (I["poison_from"] < n).any():                            # behind the last S-th hit of an item nothing may matter
        xyz, feat, scores = I["xyz"].copy(), I["feat"].copy(), I["scores"].copy()
        for i, lo in enumerate(I["poison_from"]):
            xyz[i, lo:], scores[i, lo:], feat[i * n + lo:(i + 1) * n] = np.nan, np.nan, np.nan
        _same(run_pool(dev, impl, xyz, feat, scores, I["rois"], s), got, (what, "NaN behind the S-th hit"))
        poisoned = True
    return dict(count=count, poisoned=poisoned, rys=set(I["rois"][..., 6].ravel().tolist()))


def check_pool(dev, n, impl=None, report=_print, cases=None):
    """Every case of ``pool_cases(n)``; together they cover every arm feasible at n, all four headings and the early stop."""
    seen, rys, poisoned = set(), set(), 0
    for case in (pool_cases(n) if cases is None else cases):
        r = check_pool_case(dev, n, case, impl, report)
        s, cnt = case[2], r["count"]
        seen |= {"empty"} if (cnt == 0).any() else set()
        seen |= {"one"} if (cnt == 1).any() else set()
        seen |= {"s_minus_1"} if (cnt == s - 1).any() else set()
        seen |= {"s"} if (cnt == s).any() else set()
        seen |= {"more"} if (cnt > s).any() else set()
        rys |= r["rys"]
        poisoned += r["poisoned"]
    if cases is None:
        assert (seen == set(ARMS) if n >= 63 else seen >= {"empty", "one", "s"}) and len(rys) == 4, (n, seen, rys)
        assert poisoned > 0 or n == 1, (n, "no case exercised the early stop")


def check_pool_refusals(dev):
    """The wrapper refuses before any call; the entry point itself returns its codes before any launch (outputs keep their fill)."""
    from ml3d import _abi, ops
    from ml3d.ops import _gates
    xyz, feat, sc, rois = (torch.zeros((2, 10, 3), device=dev), torch.zeros((20, 4), device=dev), torch.zeros((2, 10), device=dev),
                           torch.zeros((2, 3, 7), device=dev))
    refused(lambda: ops.roi_pool(xyz, feat, sc, rois, 0), "num_points 0")
    refused(lambda: ops.roi_pool(xyz, feat[:1].expand(20, 4), sc, rois, 8), "row stride below C")
    refused(lambda: ops.roi_pool(xyz, feat[:19], sc, rois, 8), "feat rows")
    refused(lambda: ops.roi_pool(xyz, feat, sc[:, :9].contiguous(), rois, 8), "scores shape")
    refused(lambda: ops.roi_pool(xyz, feat, sc, rois[..., :6].contiguous(), 8), "6 roi columns")
    refused(lambda: ops.roi_pool(xyz, feat, sc, rois[:1], 8), "batch mismatch")
    refused(lambda: ops.roi_pool(xyz, feat.double(), sc, rois, 8), "float64 feat")
    refused(lambda: ops.roi_pool(xyz, feat, sc, rois, 2 ** 29), "B * M * num_points past int32")
    refused(lambda: ops.roi_pool(xyz, feat, sc, rois, 8, out=(torch.zeros((6, 8, 9), device=dev),) * 3), "out shapes")
    out = (torch.full((6, 8, 9), -7.0, device=dev), torch.full((2, 3, 8), -9, dtype=torch.int32, device=dev),
           torch.full((2, 3), -9, dtype=torch.int32, device=dev))
    lib = _abi.get()

    def raw(ld, c, b, n, m, s):
        with torch.cuda.device(dev):
            return lib.ml3d_roi_pool(xyz.data_ptr(), feat.data_ptr(), ld, c, sc.data_ptr(), rois.data_ptr(), b, n, m, s, 0.3, 1.0,
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _gates._stream())

    assert raw(3, 4, 2, 10, 3, 8) == -1 and raw(4, 4, 2, 10, 3, 0) == -1 and raw(4, -1, 2, 10, 3, 8) == -1
    assert raw(4, 4, 2, 2 ** 30, 3, 8) == -4 and raw(4, 4, 2, 10, 3, 2 ** 29) == -4 and raw(4, 4, 2, 10, 2 ** 30, 8) == -4
    assert all(bool((o.cpu() == v).all()) for o, v in zip(out, (-7.0, -9, -9)))
    assert raw(4, 4, 2, 10, 3, 8) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    # all-zero rois enlarge to boxes of size 2 around the origin, where all ten points of either cloud lie
    assert bool((out[2].cpu() == 0).all()) and bool((out[1].cpu() == torch.arange(8, dtype=torch.int32)).all())


# ---- the model against the reference's stage 2 ------------------------------------------------------------------------------------------
MODEL_GOLDEN = "pointrcnn_rcnn_small"


def _model_and_points(dev, name=MODEL_GOLDEN, mode=None):
    import prcnn_cases
    import prcnn_ref
    g, mcfg = prcnn_cases.load_golden(name)
    if mode is not None:
        mcfg = dict(mcfg, mode=mode)
    model = prcnn_cases.build_model(dev, g, mcfg)
    pts = prcnn_ref.make_points(g["cloud_seeds"], int(g["n"]), int(mcfg["rpn"]["backbone"]["in_channels"]), float(g["cloud_scale"]),
                                g["cloud_offsets"])
    assert abs(pts.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
    return g, mcfg, model, pts


def _with_ops(mode, fn):
    import os
    os.environ["ML3D_PRCNN_OPS"] = mode
    try:
        return fn()
    finally:
        del os.environ["ML3D_PRCNN_OPS"]


def check_model_pooling(dev, report=_print):
    """(a) ``rcnn_from_proposals`` on the product's OWN stage 1, on both ops paths.  The golden's weight seed meets stage 1's own
    robustness conditions (the product's rois come out in the reference's order, within 4e-4 of them: asserted here) and keeps every
    in-box decision of the reference decisive by 1e-3, every pooled point's score 1e-3 from the threshold
    (tools/gen_golden_pointrcnn2.py) -> ``pool_idx`` and ``empty`` EQUAL to the golden's.  The five leading columns: against the
    float64 formula on the product's own rois within max(1e-5, 4 e32); the seg-mask column equal to the golden's."""
    g, mcfg, model, pts = _model_and_points(dev)
    th = mcfg["rcnn"]["target_head"]
    s, thres, extra = th["num_points"], mcfg["score_thres"], th["pool_extra_width"]
    xyz = np.ascontiguousarray(pts[..., :3])
    for mode in ("hip", "torch"):
        r = _with_ops(mode, lambda: model.proposals(_t(pts, dev)))
        out = _with_ops(mode, lambda: model.rcnn_from_proposals(r))
        rois = out["rois"].cpu().numpy()
        err = float(np.abs(rois - g["rois"]).max())
        report(name="%s %s rois vs golden" % (MODEL_GOLDEN, mode), max_abs_delta=err, tol=4e-4)
        assert rois.shape == g["rois"].shape and same_bits(out["rois"], r["rois"]) and err <= 4e-4, (mode, err)
        idx, empty = out["pool_idx"].cpu().numpy(), out["empty"].cpu().numpy()
        assert np.array_equal(idx, g["pool_idx"]), (mode, "pool_idx against the golden", np.argwhere(idx != g["pool_idx"])[:4].tolist())
        assert np.array_equal(empty, g["empty"]), (mode, "empty against the golden")
        got = out["pts_input"].cpu().numpy()
        assert got.shape == g["pts_input"].shape and np.array_equal(got[..., 3], g["pts_input"][..., 3]), (mode, "seg-mask column")
        rows = r["features"].transpose(1, 2).reshape(-1, r["features"].shape[1]).cpu().numpy()
        own = (xyz, rows, r["cls"].cpu().numpy()[:, :, 0], rois, s, thres, extra)
        o64, o32 = prcnn2_ref.roi_pool(*own, np.float64)[0], prcnn2_ref.roi_pool(*own, np.float32)[0]
        judge(report, "%s %s pts_input[..., :5]" % (MODEL_GOLDEN, mode), torch.from_numpy(got[..., :5]), torch.from_numpy(o64[..., :5]),
              torch.from_numpy(o32[..., :5]))
        assert np.array_equal(got[..., 5:].view(np.int32), o32[..., 5:].view(np.int32)), (mode, "feature columns bit for bit")


def check_model_network(dev, report=_print):
    """(b) ``rcnn_network`` on the GOLDEN's rows (bit-identical inputs: the index arrays are decidable): FPS and ball-query indices
    equal to the golden's, cls / reg within max(1e-4, 4.4e-6 scale) on both ops paths, the two paths within the same bound."""
    g, mcfg, model, _ = _model_and_points(dev)
    tol = max(1e-4, 4.4e-6 * float(g["scale"]))
    res = {}
    for mode in ("hip", "torch"):
        net = _with_ops(mode, lambda: model.rcnn_network(_t(g["pts_input"], dev)))
        assert len(net["fps"]) == len(net["ball"]) == int(g["levels"])
        for l in range(int(g["levels"])):
            assert np.array_equal(net["fps"][l].cpu().numpy(), g["fps%d" % l]), (mode, "fps", l)
            assert np.array_equal(net["ball"][l].cpu().numpy(), g["ball%d" % l]), (mode, "ball query", l)
        for part in ("cls", "reg"):
            got = net[part].cpu().numpy()
            err = float(np.abs(got - g[part]).max())
            report(name="%s %s %s" % (MODEL_GOLDEN, mode, part), max_abs_delta=err, tol=tol, scale=float(g["scale"]))
            assert got.shape == g[part].shape and bool(np.isfinite(got).all()) and err <= tol, (mode, part, err, tol)
            res[mode, part] = got
    for part in ("cls", "reg"):
        err = float(np.abs(res["hip", part] - res["torch", part]).max())
        report(name="%s hip vs torch %s" % (MODEL_GOLDEN, part), max_abs_delta=err, tol=tol)
        assert err <= tol, (part, err)


def check_model_plumbing(dev):
    """(c) ``rcnn_forward`` == ``rcnn_from_proposals(proposals())`` bit for bit; roi chunks of 1, 5 and all give the same bits."""
    g, mcfg, model, pts = _model_and_points(dev)
    whole = model.rcnn_forward(_t(pts, dev))
    parts = model.rcnn_from_proposals(model.proposals(_t(pts, dev)))
    assert sorted(whole) == sorted(parts) == ["ball", "cls", "empty", "fps", "pool_idx", "pts_input", "reg", "rois"]
    b, m = whole["rois"].shape[:2]
    assert tuple(whole["cls"].shape) == (b * m, 1) and whole["reg"].shape[0] == b * m and whole["rois"].shape[2] == 7
    for k in ("rois", "cls", "reg", "pts_input"):
        assert same_bits(whole[k], parts[k]), k
    assert torch.equal(whole["pool_idx"], parts["pool_idx"]) and torch.equal(whole["empty"], parts["empty"])
    for chunk in (1, 5, b * m):
        net = model.rcnn_network(whole["pts_input"], chunk=chunk)
        assert same_bits(net["cls"], whole["cls"]) and same_bits(net["reg"], whole["reg"]), chunk
        for l in range(len(net["fps"])):
            assert torch.equal(net["fps"][l], whole["fps"][l]) and torch.equal(net["ball"][l], whole["ball"][l]), (chunk, l)


class _Inputs:
    calib = None


def check_model_inference_end(dev, report=_print):
    """(d) ``inference_end`` on the golden's cls / reg / rois: the golden's kept indices in its order, boxes within 1e-4."""
    g, mcfg, model, _ = _model_and_points(dev)
    results = dict(rois=_t(g["rois"], dev), cls=_t(g["cls"], dev), reg=_t(g["reg"], dev))
    for mode in ("hip", "torch"):
        boxes, scores, keep, count = _with_ops(mode, lambda: model.rcnn_boxes(results))
        boxes, scores, keep, count = boxes.cpu().numpy(), scores.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy()
        err = float(np.abs(boxes - g["boxes"]).max())
        report(name="%s %s decoded boxes" % (MODEL_GOLDEN, mode), max_abs_delta=err, tol=1e-4)
        assert boxes.shape == g["boxes"].shape and err <= 1e-4, (mode, err)
        found = _with_ops(mode, lambda: model.inference_end(results, _Inputs()))
        assert len(found) == len(boxes)
        for i in range(len(boxes)):
            kept = keep[i, :count[i]]
            kept = kept[scores[i, kept] > np.float32(mcfg["score_thres"])]
            want = g["kept"][i][g["kept"][i] >= 0]
            assert np.array_equal(kept, want), (mode, i, kept.tolist(), want.tolist())
            assert len(found[i]) == len(want)
            for obj, j in zip(found[i], want):
                box = g["boxes"][i, j]
                assert obj.label_class == "Car" and abs(float(obj.confidence) - float(scores[i, j])) <= 1e-6
                assert np.abs(np.asarray(obj.size, np.float64) - box[[4, 3, 5]]).max() <= 1e-4 and abs(float(obj.yaw) - box[6]) <= 1e-4
                centre = box[:3].astype(np.float64) + [0, 0, box[3] / 2]
                assert np.abs(np.asarray(obj.center, np.float64) - centre).max() <= 1e-4
        assert sum(len(f) for f in found) > 0, "the golden keeps at least one box"
    rpn_mode = _model_and_points(dev, mode="RPN")[2]
    assert rpn_mode.inference_end(results, _Inputs()) == [[]]


def check_model_refusals(dev):
    """(e) ``forward`` with ``mode="RCNN"`` still raises and names the new method; the two unsupported configurations raise."""
    import prcnn_cases
    g, mcfg, model, pts = _model_and_points(dev)
    assert model.mode == "RCNN"
    try:
        model(_t(pts, dev))
    except NotImplementedError as e:
        assert "RoI stage" in str(e) and "proposals()" in str(e) and "rcnn_forward" in str(e)
    else:
        raise AssertionError("mode='RCNN' forward ran")
    bad = dict(mcfg, rcnn=dict(mcfg["rcnn"], head=dict(mcfg["rcnn"]["head"], post_process=True)))
    for cfg in (bad, dict(mcfg, classes=["Car", "Van", "Bus"])):
        from ml3d.torch.models import PointRCNN
        other = PointRCNN(**cfg, device=dev)
        try:
            other.rcnn_network(_t(g["pts_input"], dev))
        except NotImplementedError as e:
            assert "unsupported" in str(e) or "cls_channel" in str(e)
        else:
            raise AssertionError("an unsupported configuration ran")


# ---- the yaml configuration (GPU) -----------------------------------------------------------------------------------------------------
def check_yaml_configuration(dev, report=_print):
    """``rcnn_forward`` of the KITTI yaml configuration at B = 2, N = 16384 (weights and clouds of tests/golden/pointrcnn_rpn_kitti):
    shapes and finite outputs; the HIP network against the torch formulation on the SAME ``pts_input`` within max(1e-4, 4.4e-6 scale);
    the pooled result against float64 properties that need no margin -- every pooled point lies in the box grown by 1e-4, ``cnt``
    lies between the counts of the box shrunk and grown by 1e-4, the indices ascend up to ``cnt`` and then repeat ``k % cnt``.
    The pseudo-trained RPN's boxes are wild (negative sizes: every roi of ``rcnn_forward`` is empty), so the same checks run a second
    time through ``rcnn_from_proposals`` with every other roi replaced by a car-sized box around a point of the cloud."""
    g, mcfg, model, pts = _model_and_points(dev, "pointrcnn_rpn_kitti", mode="RCNN")
    _yaml_checks(dev, report, model, pts, model.rcnn_forward(_t(pts, dev)), "own rois", 0)
    r = model.proposals(_t(pts, dev))
    rois = r["rois"].cpu().numpy().copy()
    m = rois.shape[1]
    for i in range(len(rois)):
        for j in range(0, m, 2):
            centre = pts[i, (j * 163) % pts.shape[1], :3]
            rois[i, j] = (centre[0], centre[1] + 0.75, centre[2], 1.5, 1.6, 3.9 * (1 + j % 7), 0.37 * j - 3.0)
    r = dict(r, rois=_t(rois, dev))
    _yaml_checks(dev, report, model, pts, model.rcnn_from_proposals(r), "car-sized rois", m // 2 * len(rois))


def _yaml_checks(dev, report, model, pts, out, what, least):
    b, m = out["rois"].shape[:2]
    s, c = model.rcnn.num_points, out["pts_input"].shape[2] - 5
    assert (b, s, c) == (2, 512, 128) and tuple(out["pts_input"].shape) == (b * m, s, 5 + c)
    assert tuple(out["cls"].shape) == (b * m, 1) and tuple(out["reg"].shape) == (b * m, model.rcnn.reg_channel)
    for k in ("cls", "reg", "pts_input"):
        assert bool(torch.isfinite(out[k]).all()), k
    ref = _with_ops("torch", lambda: model.rcnn_network(out["pts_input"]))
    scale = float(max(out["cls"].abs().max(), out["reg"].abs().max(), out["pts_input"].abs().max()))
    tol = max(1e-4, 4.4e-6 * scale)
    for part in ("cls", "reg"):
        err = float((out[part] - ref[part]).abs().max())
        report(name="yaml %s hip vs torch %s" % (what, part), max_abs_delta=err, tol=tol, scale=scale)
        assert err <= tol, (part, err, tol)
    for l in range(len(ref["fps"])):
        assert torch.equal(ref["fps"][l], out["fps"][l]) and torch.equal(ref["ball"][l], out["ball"][l])
    rois, idx, empty = out["rois"].cpu().numpy().astype(np.float64), out["pool_idx"].cpu().numpy(), out["empty"].cpu().numpy()
    xyz = pts[..., :3].astype(np.float64)
    big = prcnn2_ref.enlarge(rois, model.rcnn.pool_extra_width, np.float64)
    nonempty = wrapped = cut = 0
    for i in range(b):
        for j in range(m):
            d = prcnn2_ref.decisive_margins(xyz[i], big[i, j])
            inside = prcnn2_ref.in_box(xyz[i], big[i, j], np.float64)
            lo, hi = int((inside & (d > 1e-4)).sum()), int((inside | (d <= 1e-4)).sum())
            row = idx[i, j]
            if row[0] < 0:
                assert empty[i, j] == 1 and (row == -1).all() and lo == 0, (i, j, lo)
                continue
            nonempty += 1
            assert empty[i, j] == 0
            wrapped, cut = wrapped + (lo < s and hi < s), cut + (lo > s)
            cnt = int(np.argmax(np.diff(row) <= 0)) + 1 if (np.diff(row) <= 0).any() else s
            assert (np.diff(row[:cnt]) > 0).all() and np.array_equal(row, row[np.arange(s) % cnt]), (i, j, "ascending, then k % cnt")
            assert (inside[row] | (d[row] <= 1e-4)).all(), (i, j, "a pooled point outside the box grown by 1e-4")
            assert min(lo, s) <= cnt <= min(hi, s), (i, j, lo, cnt, hi)
            sure = np.flatnonzero(inside & (d > 1e-4))                  # nothing surely inside was passed over
            assert np.isin(sure[sure <= row[cnt - 1]] if cnt == s else sure, row[:cnt]).all(), (i, j, "a hit was passed over")
    report(name="yaml %s pooled" % what, nonempty=nonempty, wrapped=wrapped, cut=cut, rois=b * m)
    assert nonempty >= least and (least == 0 or (wrapped > 0 and cut > 0)), (what, nonempty, wrapped, cut)
