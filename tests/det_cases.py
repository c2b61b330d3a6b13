"""Shared bodies of the ``ops.det_match`` tests (ml3d_det_match: every frame's predictions matched against its ground truth on the
device, the matching of the reference's ``precision_3d``).  tests/test_emulated_det_eval.py runs them on CPU tensors against the
host emulation of the HIP sources, tests/test_gpu_det_eval.py on the MI355X, tests/test_det_cases_can_fail.py against stand-ins:
the right one passes, every wrong one is rejected by every case that covers its edge.

``impl`` is anything with ``det_match``, ``iou_bev`` and ``iou_3d`` of ``ml3d.ops``' signatures (default: ``ml3d.ops``).  The oracle
is tests/det_ref.py fed the ORACLE's IoU matrices (oracle/ops.py); flags, ``fn`` and the AP computed from the flags are compared for
EQUALITY.  That is sound because the inputs are decisive, which every check asserts first: every related pair's oracle IoU is
exactly 0 or >= 1e-3, every non-zero one is >= 1e-3 away from its class's overlap, and in every column the two largest differ by
>= 1e-3 unless they come from bit-identical boxes or the column is all zero (1e-3 = 100 x the 1e-5 that tests/test_gpu_api.py
allows between the device's IoU and the oracle's; an all-zero column elects the class's first prediction, which is the point).  The
one exception is case ``quirks``: axis-aligned boxes on a quarter grid, whose IoUs are computed without rounding on either side, one
of them exactly AT the overlap.
``pair_iou`` must carry the bits of ``impl.iou_bev`` / ``impl.iou_3d`` on the same boxes, lie within 1e-5 of the oracle (equal bits on
the emulator), and keep its sentinel wherever the classes do not relate.  Every call adds into a pre-filled ``out_fn``, writes into a
sentinel-filled flag buffer with guard bytes behind it, and leaves its inputs unchanged."""
import numpy as np
import torch

import det_ref as R

MARGIN = 1e-3
GUARD = 64
SENTINEL_FLAG = 0xA5
SENTINEL_IOU = np.float32(-7.25)
_ORACLE = {}                                      # split name -> per-frame oracle IoUs (computed once per process)


def _impl(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


# ---- splits in the id form of ml3d_det_match -----------------------------------------------------------------------------------------
class Split(object):
    def __init__(self, name, frames, min_overlap, similar, D, exact=False):
        """``frames``: per frame (pred rows [(box7, cls, dmask, score)], target rows [(box7, lab, dmask)])."""
        self.name, self.D, self.exact = name, D, exact
        self.min_overlap, self.similar = np.asarray(min_overlap, np.float32), np.asarray(similar, np.int32)
        self.C = len(min_overlap)
        P = [r for p, _ in frames for r in p]
        T = [r for _, t in frames for r in t]
        self.pred_box = np.array([r[0] for r in P], np.float32).reshape(-1, 7)
        self.pred_cls = np.array([r[1] for r in P], np.int32)
        self.pred_dm = np.array([r[2] for r in P], np.int64).astype(np.uint32).view(np.int32)
        self.score = np.array([r[3] for r in P], np.float64)
        self.tgt_box = np.array([r[0] for r in T], np.float32).reshape(-1, 7)
        self.tgt_lab = np.array([r[1] for r in T], np.int32)
        self.tgt_dm = np.array([r[2] for r in T], np.int64).astype(np.uint32).view(np.int32)
        self.pred_start = np.cumsum([0] + [len(p) for p, _ in frames]).astype(np.int64)
        self.tgt_start = np.cumsum([0] + [len(t) for _, t in frames]).astype(np.int64)
        self.F = len(frames)

    def frame(self, f):
        return slice(self.pred_start[f], self.pred_start[f + 1]), slice(self.tgt_start[f], self.tgt_start[f + 1])

    def related(self, f):
        """bool [P_f, T_f]: the pairs whose classes relate."""
        ps, ts = self.frame(f)
        c, lab = self.pred_cls[ps][:, None], self.tgt_lab[ts][None, :]
        ok = (c >= 0) & (c < self.C)
        sim = self.similar[np.clip(c, 0, self.C - 1)]
        return ok & ((lab == c) | ((sim >= 0) & (lab == sim)))

    def oracle(self):
        """Per frame (iou_bev, iou_3d) float32 [P_f, T_f] of the CPU oracle; only the related pairs are computed, the rest are NaN."""
        if self.name not in _ORACLE:
            from oracle import ops as oops
            out = []
            for f in range(self.F):
                ps, ts = self.frame(f)
                a, b, rel = self.pred_box[ps], self.tgt_box[ts], self.related(f)
                m = [np.full(rel.shape, np.nan, np.float32), np.full(rel.shape, np.nan, np.float32)]
                for c in range(self.C):                    # a class's rows x columns: a rectangle of related pairs
                    rows = np.where(self.pred_cls[ps] == c)[0]
                    cols = np.where(rel[rows[0]])[0] if len(rows) else rows
                    if len(rows) and len(cols):
                        m[0][np.ix_(rows, cols)] = oops.iou_bev(a[rows][:, [0, 2, 3, 5, 6]], b[cols][:, [0, 2, 3, 5, 6]])
                        m[1][np.ix_(rows, cols)] = oops.iou_3d(a[rows], b[cols])
                assert not np.isnan(m[0][rel]).any() and np.isnan(m[0][~rel]).all()
                out.append(m)
            _ORACLE[self.name] = out
        return _ORACLE[self.name]

    def assert_decisive(self):
        for f, ious in enumerate(self.oracle()):
            ps, _ = self.frame(f)
            rel, cls, box = self.related(f), self.pred_cls[ps], self.pred_box[ps]
            for iou in ious:
                for c in range(self.C):
                    rows = np.where(cls == c)[0]
                    if not len(rows):
                        continue
                    cols = np.where(rel[rows[0]])[0]
                    sub = iou[np.ix_(rows, cols)].astype(np.float64)
                    nz = sub[sub != 0]
                    assert (nz >= MARGIN).all(), (self.name, f, "an IoU in (0, 1e-3)")
                    assert (np.abs(nz - np.float64(self.min_overlap[c])) >= MARGIN).all(), (self.name, f, "an IoU at the overlap")
                    for k in range(len(cols)):
                        o = np.argsort(-sub[:, k], kind="stable")
                        if len(o) >= 2 and sub[o[0], k] > 0 and sub[o[0], k] - sub[o[1], k] < MARGIN:
                            assert np.array_equal(box[rows[o[0]]], box[rows[o[1]]]), (self.name, f, "a close race in a column")

    def expected(self):
        """flags uint8 [2, D, NP], fn int64 [2, C, D] from tests/det_ref.py on the oracle's IoUs."""
        flags = np.zeros((2, self.D, len(self.pred_cls)), np.uint8)
        fn = np.zeros((2, self.C, self.D), np.int64)
        pdm, tdm = self.pred_dm.view(np.uint32), self.tgt_dm.view(np.uint32)
        for f, ious in enumerate(self.oracle()):
            ps, ts = self.frame(f)
            for m in range(2):
                fl, n = R.match_ids(np.nan_to_num(ious[m], nan=9.0), self.pred_cls[ps], pdm[ps], self.tgt_lab[ts], tdm[ts],
                                    self.min_overlap, self.similar, self.D)       # (9.0: an unrelated pair that is read shows)
                flags[m][:, ps] = fl
                fn[m] += n
        return flags, fn

    def gt_counts(self):
        tdm = self.tgt_dm.view(np.uint32)
        return np.array([[int((((tdm >> np.uint32(j)) & 1) == 1)[self.tgt_lab == c].sum()) for j in range(self.D)] for c in range(self.C)], np.float64)


def check(dev, impl, S, metrics=3, decisive=True):
    """One ``det_match`` of split ``S``; everything the module's docstring lists."""
    ops = _impl(impl)
    if decisive:
        S.assert_decisive()
    want_flags, want_fn = S.expected()
    NP, C, D = len(S.pred_cls), S.C, S.D
    host = [S.pred_box, S.pred_cls, S.pred_dm, S.tgt_box, S.tgt_lab, S.tgt_dm, S.min_overlap, S.similar]
    t = [torch.from_numpy(a.copy()).to(dev) for a in host]
    pair_start = ops.det_pair_starts(S.pred_start, S.tgt_start) if hasattr(ops, "det_pair_starts") else None
    starts = np.zeros(S.F + 1, np.int64)
    np.cumsum(np.diff(S.pred_start) * np.diff(S.tgt_start), out=starts[1:])
    assert pair_start is None or np.array_equal(pair_start, starts)
    n_pairs = int(starts[-1])
    g = np.random.default_rng(NP * 31 + n_pairs)
    pre_fn = g.integers(1, 1000, size=(2, C, D)).astype(np.int64)
    pre_fn[0, 0, 0] = 2 ** 32 - 1                                     # (the 64-bit carry)
    fn = torch.from_numpy(pre_fn.copy()).to(dev)
    flag_buf = torch.full((2 * D * NP + GUARD,), SENTINEL_FLAG, dtype=torch.uint8, device=dev)
    iou_buf = torch.full((2, n_pairs + 3), float(SENTINEL_IOU), dtype=torch.float32, device=dev)
    got = ops.det_match(t[0], t[1], t[2], S.pred_start, t[3], t[4], t[5], S.tgt_start, t[6], t[7], D, metrics=metrics,
                        out_flags=flag_buf[:2 * D * NP].view(2, D, NP), out_fn=fn, return_iou=True, pair_iou=iou_buf)
    key = (S.name, metrics)
    assert len(got) == 3 and got[1] is fn and got[2] is iou_buf, key
    flags = flag_buf.cpu().numpy()
    assert (flags[2 * D * NP:] == SENTINEL_FLAG).all(), ("written past the flags", key)
    flags = flags[:2 * D * NP].reshape(2, D, NP)
    got_fn, pair = fn.cpu().numpy(), iou_buf.cpu().numpy()
    for m in range(2):
        if not (metrics >> m) & 1:
            if NP and S.F:
                assert (flags[m] == SENTINEL_FLAG).all(), ("a plane that was not asked for was written", key, m)
            assert np.array_equal(got_fn[m], pre_fn[m]), ("fn of a plane that was not asked for changed", key, m)
            assert (pair[m] == SENTINEL_IOU).all(), ("IoUs of a plane that was not asked for were written", key, m)
            continue
        if NP == 0 or S.F == 0:                                       # the documented no-op
            assert np.array_equal(got_fn[m], pre_fn[m]) and (pair[m] == SENTINEL_IOU).all(), key
            continue
        assert np.array_equal(flags[m], want_flags[m]), ("flags", key, m, np.argwhere(flags[m] != want_flags[m])[:5].tolist())
        assert np.array_equal(got_fn[m], pre_fn[m] + want_fn[m]), ("fn must be ADDED to", key, m, (got_fn[m] - pre_fn[m]).tolist(), want_fn[m].tolist())
        assert (pair[m][n_pairs:] == SENTINEL_IOU).all(), ("written past the pairs", key, m)
        gt = S.gt_counts()
        for samples in (41, 11):
            mine = R.ap_from_flags(flags[m], S.score, S.pred_cls, S.pred_dm.view(np.uint32), gt, samples)
            assert np.array_equal(mine, R.ap_from_flags(want_flags[m], S.score, S.pred_cls, S.pred_dm.view(np.uint32), gt, samples)), ("AP", key, m)
        for f, ious in enumerate(S.oracle()):
            ps, ts = S.frame(f)
            rel = S.related(f)
            block = pair[m][starts[f]:starts[f + 1]].reshape(rel.shape)
            assert (block[~rel] == SENTINEL_IOU).all(), ("a pair whose classes do not relate was written", key, m, f)
            if not rel.any():
                continue
            a, b = t[0][ps.start:ps.stop], t[3][ts.start:ts.stop]
            same = (ops.iou_bev(a[:, [0, 2, 3, 5, 6]].contiguous(), b[:, [0, 2, 3, 5, 6]].contiguous()) if m == 0 else ops.iou_3d(a, b)).cpu().numpy()
            assert np.array_equal(block[rel].view(np.uint32), same[rel].view(np.uint32)), ("pair_iou differs from ops.iou_*", key, m, f)
            if torch.device(dev).type == "cpu":
                assert np.array_equal(block[rel].view(np.uint32), ious[m][rel].view(np.uint32)), ("pair_iou differs from the oracle", key, m, f)
            else:
                print("det_match %s, metric %d, frame %d: max |pair_iou - oracle| = %.3g over %d pairs" %
                      (S.name, m, f, np.abs(block[rel].astype(np.float64) - ious[m][rel]).max(), int(rel.sum())))
                assert np.abs(block[rel].astype(np.float64) - ious[m][rel]).max() <= 1e-5, ("pair_iou is not the oracle's", key, m, f)
    for a, b in zip(host, t):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8)), ("an input changed", key)


# ---- generated boxes ---------------------------------------------------------------------------------------------------------------
def _mask(d, D):
    """the bit mask of difficulty ``d`` under difficulties [0, 1, .., D - 1]; -1: none"""
    return 0 if d < 0 else ((1 << D) - 1) & ~((1 << d) - 1)


def _difficulty(g, D):
    return -1 if g.uniform() < 0.1 else int(g.integers(0, D))


def _box(g):
    return [g.uniform(-10, 10), 1.6 + g.uniform(-0.1, 0.1), g.uniform(-10, 10), g.uniform(1.4, 2.0), g.uniform(1.4, 1.8), g.uniform(3.4, 4.4),
            g.uniform(-np.pi, np.pi)]


def _near(g, b, amount):
    b = list(b)
    b[0] += amount * g.uniform(-1, 1)
    b[2] += amount * g.uniform(-1, 1)
    b[1] += 0.2 * amount * g.uniform(-1, 1)
    b[6] += 0.3 * amount * g.uniform(-1, 1)
    return b


def random_split(name, seed, sizes, C, D, with_similar=False, overlap=None):
    """Frames of (P, T) boxes with centres in [-10, 10]^2 and sides of 1.4 .. 4.4, the regime of tests/test_gpu_api.py's IoU test, whose
    1e-5 the device's IoUs are held to here: the device's sinf / cosf differ from libm's in the last bit, a corner is rounded to the
    float32 grid of its coordinate, and the IoU moves by about ulp(coordinate) x perimeter / area -- 1e-6 at these sizes, 1e-5 and more
    from |x| = 100 on.  Targets may overlap one another.  A prediction stands near a random target -- tight, loose, or as a
    bit-identical twin of an earlier prediction -- or anywhere; classes, difficulties (-1 included) and scores are random, the scores
    on a two-decimal grid so that equal ones occur.  A prediction that would make its frame indecisive becomes a box of no class."""
    g = np.random.default_rng(seed)
    similar = [-1] * C
    if with_similar:
        similar[C - 1] = C                                 # the last class's similar label: vocabulary id C
    mo = list(overlap or ([0.5, 0.5, 0.7][:C] if C > 1 else [0.7]))
    frames = []
    for P, T in sizes:
        tg = []
        for k in range(T):
            lab = int(g.integers(0, C))
            if with_similar and g.uniform() < 0.15:
                lab = C
            if g.uniform() < 0.05:
                lab = -1
            tg.append((_box(g), lab, _mask(_difficulty(g, D), D)))
        pr = []
        for k in range(P):
            cls = int(g.integers(0, C)) if g.uniform() > 0.05 else -1
            u = g.uniform()
            if T and u < 0.8:
                tb, tl, _ = tg[int(g.integers(0, T))]
                bx = _near(g, tb, float(g.choice([0.1, 0.3, 0.7])))
                if 0 <= tl < C and g.uniform() < 0.8:
                    cls = tl
                elif tl == C:
                    cls = C - 1
            elif pr and u < 0.9:
                bx, cls = list(pr[int(g.integers(0, len(pr)))][0]), pr[-1][1]          # a twin
            else:
                bx = _box(g)
            pr.append((bx, cls, _mask(_difficulty(g, D), D), float(np.round(g.uniform(0.05, 0.99), 2))))
        frames.append((pr, tg))
    S = Split(name, frames, mo, similar, D)
    for attempt in range(8):                               # the predictions of indecisive pairs: boxes of no class
        _ORACLE.pop(name, None)
        bad = _indecisive_rows(S)
        if not len(bad):
            return S
        S.pred_cls[bad] = -1
    raise AssertionError("no decisive boxes for " + name)


def _indecisive_rows(S):
    bad = set()
    for f, ious in enumerate(S.oracle()):
        ps, _ = S.frame(f)
        rel, cls, box = S.related(f), S.pred_cls[ps], S.pred_box[ps]
        for iou in ious:
            for c in range(S.C):
                rows = np.where(cls == c)[0]
                if not len(rows):
                    continue
                cols = np.where(rel[rows[0]])[0]
                sub = iou[np.ix_(rows, cols)].astype(np.float64)
                close = ((sub != 0) & (sub < MARGIN)) | ((sub != 0) & (np.abs(sub - np.float64(S.min_overlap[c])) < MARGIN))
                bad.update(int(ps.start + rows[r]) for r in np.where(close.any(axis=1))[0])
                for k in range(len(cols)):
                    o = np.argsort(-sub[:, k], kind="stable")
                    if len(o) >= 2 and sub[o[0], k] > 0 and sub[o[0], k] - sub[o[1], k] < MARGIN and \
                            not np.array_equal(box[rows[o[0]]], box[rows[o[1]]]):
                        bad.add(int(ps.start + rows[o[1]]))
    return sorted(bad)


_SPLITS = {}


def split(name):
    """The named split, built once per process."""
    if name not in _SPLITS:
        _SPLITS[name] = _BUILDERS[name]()
    return _SPLITS[name]


def _quirks():
    """Axis-aligned boxes on a quarter grid (every IoU is computed without rounding): C = 2, difficulties [0, 1], overlap 0.5;
    class 0's similar label is vocabulary id 2.  One frame per quirk of the reference."""
    def sq(x, z=0.0, w=2.0, l=2.0):
        return [x, 1.0, z, w, 2.0, l, 0.0]
    E, H, N = 0b11, 0b10, 0b00                              # difficulty 0 (easy), 1 (hard), -1 (none)
    frames = [
        # the tp rule: r1 matches t1 (0.6) without being its best (r0: 1.0), and is the best of t2 (1/3 < overlap): tp all the same
        ([(sq(0.0), 0, E, 0.9), (sq(0.5), 0, E, 0.8)], [(sq(0.0), 0, E), (sq(1.5), 0, E)]),
        # the arg-max runs over the rows of ALL difficulties: the hard r0 (1.0) is the column's best, the easy r1 (0.6) is fp at difficulty 0
        ([(sq(0.0), 0, H, 0.9), (sq(0.5), 0, E, 0.8)], [(sq(0.0), 0, E)]),
        # twins: the FIRST is tp, the second fp; and a column that is all zero elects the first prediction of its class
        ([(sq(0.5), 0, E, 0.7), (sq(0.5), 0, E, 0.7), (sq(0.0, 40.0), 1, E, 0.6), (sq(8.0, 40.0), 1, E, 0.5)],
         [(sq(0.0), 0, E), (sq(4.0, 40.0), 1, E)]),
        # a similar target (id 2): no miss when nothing reaches it; a prediction on it alone is neither tp nor fp; one on nothing is fp
        ([(sq(10.5), 0, E, 0.9), (sq(30.0), 0, E, 0.8)], [(sq(10.0), 2, E), (sq(20.0), 2, E), (sq(50.0), 0, H)]),
        # an IoU exactly AT the overlap counts (>=): a 1 x 2 box inside a 2 x 2 one, 0.5 in both metrics
        ([(sq(0.0), 0, E, 0.9), (sq(20.0), 1, E, 0.4)], [(sq(0.5, 0.0, 1.0, 2.0), 0, E), (sq(20.5, 0.0, 1.0, 2.0), 1, H)]),
        # difficulties are thresholds (0 <= d <= diff), -1 is in none; a box of no class; an easy prediction on a hard target only
        ([(sq(0.0), 0, E, 0.9), (sq(10.0), 0, N, 0.8), (sq(20.0), -1, E, 0.7), (sq(30.0), 1, H, 0.6)],
         [(sq(0.0), 0, H), (sq(10.0), 0, E), (sq(30.0), 1, N), (sq(60.0), -1, E)]),
    ]
    return Split("quirks", frames, [0.5, 0.5], [2, -1], 2, exact=True)


_EDGE = (0, 1, 63, 64, 65)
_BUILDERS = {
    "quirks": _quirks,
    "one_frame": lambda: random_split("one_frame", 41, [(65, 64)], 1, 1),
    "three_frames_a": lambda: random_split("three_frames_a", 42, [(0, 5), (63, 1), (64, 65)], 3, 3, with_similar=True),
    "three_frames_b": lambda: random_split("three_frames_b", 43, [(1, 0), (0, 0), (65, 63)], 3, 1),
    "edges": lambda: random_split("edges", 44, [(p, t) for p in _EDGE for t in _EDGE if p + t <= 66], 1, 3, with_similar=True, overlap=[0.5]),
    "seventy": lambda: random_split("seventy", 45, [(int(p), int(t)) for p, t in np.random.default_rng(7).integers(0, 7, size=(70, 2))], 3, 3,
                                    with_similar=True),
    "large": lambda: random_split("large", 46, [(400, 130)], 1, 1, overlap=[0.5]),
}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def case_quirks(dev, impl=None):
    """The reference's rules one by one, on exact IoUs (see ``_quirks``); the expected flags are also written out here."""
    S = split("quirks")
    flags, fn = S.expected()
    TP, FP = 1, 2
    want0 = [TP, TP, 0, FP, TP, FP, FP, FP, 0, FP, TP, 0, 0, 0, 0, 0]                   # difficulty 0, either metric
    want1 = [TP, TP, TP, FP, TP, FP, FP, FP, 0, FP, TP, TP, TP, 0, 0, 0]                # difficulty 1
    for m in range(2):
        assert flags[m][0].tolist() == want0 and flags[m][1].tolist() == want1, (m, flags[m].tolist())
        assert fn[m].tolist() == [[1, 2], [1, 1]], fn[m].tolist()
    for metrics in (3, 1, 2):
        check(dev, impl, S, metrics=metrics, decisive=False)


def case_sizes(dev, impl=None):
    """F = 1 and 3; P_f and T_f across 0, 1, 63, 64, 65 (a wave's edges, in rows and in columns); C and D in {1, 3}."""
    for name in ("one_frame", "three_frames_a", "three_frames_b", "edges"):
        check(dev, impl, split(name))


def case_seventy_frames(dev, impl=None):
    """70 frames of 0 .. 6 boxes a side, C = 3, D = 3, similar targets: frames without predictions, without targets, with neither."""
    S = split("seventy")
    sizes = set(zip(np.diff(S.pred_start).tolist(), np.diff(S.tgt_start).tolist()))
    assert any(p == 0 and t > 0 for p, t in sizes) and any(t == 0 and p > 0 for p, t in sizes)
    check(dev, impl, S)


def case_metrics(dev, impl=None):
    """``metrics`` 1, 2 and 3: the plane that was not asked for keeps its sentinel, in the flags, in fn and in pair_iou."""
    for metrics in (1, 2, 3):
        check(dev, impl, split("three_frames_a"), metrics=metrics)


def case_large_frame(dev, impl=None):
    """One frame of 400 x 130 boxes in one class: an IoU block of 208 KB, past any LDS tile."""
    check(dev, impl, split("large"))


def case_capacity_and_noops(dev, impl=None):
    """A ``pair_iou`` one element short is refused ("workspace too small") before anything is written; no frames and no
    predictions are no-ops."""
    ops = _impl(impl)
    S = split("three_frames_b")
    t = [torch.from_numpy(a.copy()).to(dev) for a in (S.pred_box, S.pred_cls, S.pred_dm, S.tgt_box, S.tgt_lab, S.tgt_dm, S.min_overlap, S.similar)]
    n_pairs = int((np.diff(S.pred_start) * np.diff(S.tgt_start)).sum())
    short = torch.full((2, n_pairs - 1), float(SENTINEL_IOU), dtype=torch.float32, device=dev)
    flags = torch.full((2, S.D, len(S.pred_cls)), SENTINEL_FLAG, dtype=torch.uint8, device=dev)
    try:
        ops.det_match(t[0], t[1], t[2], S.pred_start, t[3], t[4], t[5], S.tgt_start, t[6], t[7], S.D, out_flags=flags, pair_iou=short)
    except RuntimeError as e:
        assert "workspace too small" in str(e), str(e)
    else:
        raise AssertionError("a pair_iou one element short was accepted")
    assert (flags.cpu().numpy() == SENTINEL_FLAG).all() and (short.cpu().numpy() == SENTINEL_IOU).all()
    none = Split("none", [], S.min_overlap, S.similar, S.D)
    check(dev, impl, none, decisive=False)
    g = np.random.default_rng(5)
    no_pred = Split("no_pred", [([], [(_box(g), 0, 1)]), ([], [])], [0.5], [-1], 1)
    check(dev, impl, no_pred, decisive=False)


CASES = dict(quirks=case_quirks, sizes=case_sizes, seventy_frames=case_seventy_frames, metrics=case_metrics, large_frame=case_large_frame,
             capacity_and_noops=case_capacity_and_noops)


# ---- model level: mAP / ObjdetMetric on the golden's frames ------------------------------------------------------------------------
GOLDEN_SETTINGS = (
    ("one", ["Car"], [0], [0.7], {}),
    ("kitti", ["Pedestrian", "Cyclist", "Car"], [0, 1, 2], [0.5, 0.5, 0.7], {"Van": "Car", "Person_sitting": "Pedestrian"}),
    ("similar", ["Pedestrian", "Cyclist", "Car"], [0, 1, 2], [0.5], {"Car": "Van"}),
)
GOLDEN_FRAMES = 8


def golden_frames(golden, name):
    preds, targets = [], []
    for f in range(GOLDEN_FRAMES):
        k = "%s_%d_" % (name, f)
        p = {"bbox": golden[k + "pred_bbox"], "label": golden[k + "pred_label"], "score": golden[k + "pred_score"]}
        if k + "pred_difficulty" in golden.files:
            p["difficulty"] = golden[k + "pred_difficulty"]
        preds.append(p)
        targets.append({"bbox": golden[k + "tgt_bbox"], "label": golden[k + "tgt_label"], "difficulty": golden[k + "tgt_difficulty"]})
    return preds, targets


def check_golden_model(dev, route):
    """``mAP``, ``precision_3d`` and ``ObjdetMetric`` of the product on the golden's frames, on the device route or with
    ``ML3D_DET_EVAL=host``: the reference's arrays, for equality; and the launches / transfers each route makes."""
    import os
    from ml3d import metrics as M
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_objdet.npz"))
    before = os.environ.get("ML3D_DET_EVAL")
    os.environ["ML3D_DET_EVAL"] = route
    try:
        _golden_model(golden, dev, M, route)
    finally:
        os.environ.pop("ML3D_DET_EVAL")
        if before is not None:
            os.environ["ML3D_DET_EVAL"] = before


def _golden_model(golden, dev, M, route):
    import importlib
    MOD = importlib.import_module(M.__name__ + ".mAP")      # (the package's attribute ``mAP`` is the function)
    for name, classes, difficulties, min_overlap, similar in GOLDEN_SETTINGS:
        preds, targets = golden_frames(golden, name)
        for bev in (True, False):
            tag = "bev" if bev else "3d"
            for samples in (41, 11, 0):
                got = M.mAP(preds, targets, classes, difficulties, min_overlap, bev, samples, similar, device=dev)
                want = golden["%s_mAP_%s_%d" % (name, tag, samples)]
                assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (route, name, tag, samples, got, want)
            mo = list(min_overlap) * (len(classes) if len(min_overlap) == 1 else 1)
            for f in range(GOLDEN_FRAMES):
                det, fns = M.precision_3d(preds[f], targets[f], classes, difficulties, mo, bev, similar, device=dev)
                k = "%s_%d_%s_" % (name, f, tag)
                assert det.shape == golden[k + "detection"].shape and R.rows_of(det) == R.rows_of(golden[k + "detection"]), (route, k)
                assert fns.dtype == np.int64 and np.array_equal(fns, golden[k + "fns"]), (route, k, fns.tolist())
        stats = MOD.STATS
        stats.update(dict.fromkeys(stats, 0))
        M.mAP(preds, targets, classes, difficulties, min_overlap, True, 41, similar, device=dev)
        if route == "device":
            assert stats == {"det_match": 1, "uploads": 1, "readbacks": 1, "iou_launches": 0}, stats
        else:
            assert stats["det_match"] == 0 and stats["iou_launches"] == stats["readbacks"] == stats["uploads"] > 1, stats
        metric = M.ObjdetMetric(classes, difficulties, min_overlap, similar, device=dev)
        metric.update(preds[:3], targets[:3])
        metric.update(preds[3:], targets[3:])
        for turn in range(2):                           # (again after reset(): nothing is left over)
            got = metric.compute()
            assert sorted(got) == ["3d", "bev"]
            for tag in ("bev", "3d"):
                want = golden["%s_mAP_%s_41" % (name, tag)][:, :, 0]
                assert np.array_equal(got[tag], want), (route, name, tag)
                assert metric.overall()[tag] == float(np.mean(want[:, -1]))
            metric.reset()
            metric.update(preds, targets)
    if route == "device":                                   # non-finite boxes: the host route, with a warning
        import warnings
        name, classes, difficulties, min_overlap, similar = GOLDEN_SETTINGS[0]
        preds, targets = golden_frames(golden, name)
        preds[0] = {"bbox": np.full((1, 7), np.nan, np.float32), "label": np.array(["Car"]), "score": np.array([0.5], np.float32)}
        MOD._warned_nonfinite = False
        stats.update(dict.fromkeys(stats, 0))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            M.mAP(preds, targets, classes, difficulties, min_overlap, True, 41, similar, device=dev)
        assert stats["det_match"] == 0 and stats["iou_launches"] > 0 and any("non-finite" in str(w.message) for w in seen)
