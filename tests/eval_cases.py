"""Shared bodies of the ``ops.vote_confusion`` / ``ops.score_confusion`` tests (ml3d_vote_confusion, ml3d_score_confusion: the
confusion matrix of a finished cloud's labels against its ground truth, summed on the device).  tests/test_emulated_eval.py runs
them on CPU tensors against the host emulation of the HIP sources, tests/test_gpu_eval.py on the MI355X,
tests/test_eval_cases_can_fail.py against numpy stand-ins: the right one passes, every wrong one is rejected by every case that
covers its edge.

``impl`` is anything with ``vote_confusion``, ``score_confusion`` and ``vote_project`` of ``ml3d.ops``' signatures (default:
``ml3d.ops``).  The oracle is numpy (tests/eval_ref.py, pinned to the reference by tests/test_eval_host.py) and everything is
compared for EQUALITY: the values are integers.  Every check runs twice -- into a zeroed matrix, and into a matrix and counts that
already hold values, which must be ADDED to -- and the label output is cut out of a sentinel-filled buffer."""
import numpy as np
import torch

import eval_ref as E
import finish_cases as F

SHARE = 1024                                      # points per workgroup (VC_SHARE of csrc/knn.hip)
N_FULL = (0, 1, 63, 64, 65, 257, 3 * SHARE + 5)   # a wave's and a pass's edges; three workgroups and a tail
CLASSES = (1, 2, 19, 64, 65, 256)                 # 64 | 65: the LDS table and the adds straight to the matrix
GUARD = 64
H_NAN = 0x7E01


def _impl(impl):
    if impl is not None:
        return impl
    from ml3d import ops
    return ops


def some_lut(C, which):
    """None (identity) or the table of ``ignored``: first, middle, several."""
    ign = {"identity": None, "first": [0], "middle": [(C + 1) // 2], "several": sorted({0, (C + 1) // 2, C})}[which]
    return None if ign is None else E.label_lut(C, ign).astype(np.int32)


def some_gt(rng, n, C, lut, outside=True):
    """Label values over the whole table, with a negative value and one >= the table's size in between when ``outside``."""
    size = C if lut is None else len(lut)
    gt = rng.integers(0, size, size=n).astype(np.int32)
    if outside and n >= 4:
        gt[1], gt[n // 2], gt[-1] = -1, size, size + 5
    return gt


def check(dev, impl, v, p, gt, lut, a_in=0, want_labels=True, surround=0x7A7A, what=None):
    """One ``vote_confusion`` of votes ``v`` (float16 [n_sub, C]) through ``p`` (int32 [n_full] or None) against ``gt`` and ``lut``.
    The votes are rows [a_in, a_in + n_sub) of a larger buffer whose other halves hold ``surround``."""
    ops = _impl(impl)
    v = np.ascontiguousarray(v, dtype=np.float16)
    (n_sub, C) = v.shape
    p = None if p is None else np.ascontiguousarray(p, dtype=np.int32)
    n_full = n_sub if p is None else p.size
    gt = np.ascontiguousarray(gt, dtype=np.int32)
    assert gt.size == n_full
    pred = np.argmax(v, 1) if p is None else np.argmax(v, 1)[p]
    want_conf, want_counts = E.confusion_fast(pred, gt, lut, C)
    assert int(want_counts.sum()) == n_full and int(want_conf.sum()) == int(want_counts[0])
    whole = np.full((a_in + n_sub + 1, C), surround, np.uint16)
    whole[a_in:a_in + n_sub] = v.view(np.uint16)
    votes = torch.from_numpy(whole.view(np.float16)).to(dev)[a_in:a_in + n_sub]
    proj = None if p is None else torch.from_numpy(p).to(dev)
    gt_dev = torch.from_numpy(gt).to(dev)
    g = np.random.default_rng(C * 1000 + n_full)
    for rnd, sentinel in enumerate((0xA5, 0x3C)):
        pre_conf = np.zeros((C, C), np.int64) if rnd == 0 else g.integers(1, 1000, size=(C, C)).astype(np.int64)
        pre_counts = np.zeros(3, np.int64) if rnd == 0 else np.array([7, 11, 13], np.int64)
        conf, counts = torch.from_numpy(pre_conf.copy()).to(dev), torch.from_numpy(pre_counts.copy()).to(dev)
        lab_buf = torch.full((n_full + GUARD,), sentinel, dtype=torch.uint8, device=dev)
        if rnd == 0:                                  # allocated by the op, zeroed
            got = ops.vote_confusion(votes, proj, gt_dev, lut, labels=lab_buf[:n_full] if want_labels else False)
        else:
            got = ops.vote_confusion(votes, proj, gt_dev, lut, confusion=conf, counts=counts, labels=lab_buf[:n_full] if want_labels else False)
            assert got[0] is conf and got[1] is counts, what
        assert len(got) == (3 if want_labels else 2), what
        assert got[0].dtype == torch.int64 and tuple(got[0].shape) == (C, C) and got[1].dtype == torch.int64 and tuple(got[1].shape) == (3,)
        key = (what, C, n_sub, n_full, a_in, rnd)
        assert np.array_equal(got[1].cpu().numpy(), pre_counts + want_counts), ("counts", key, got[1].cpu().numpy(), want_counts)
        assert np.array_equal(got[0].cpu().numpy(), pre_conf + want_conf), ("confusion", key)
        lab = lab_buf.cpu().numpy()
        if want_labels:
            assert got[2].dtype == torch.uint8 and np.array_equal(got[2].cpu().numpy(), lab[:n_full]), key
            assert np.array_equal(lab[:n_full].astype(np.int64), pred), ("labels", key)
            if n_full and p is not None:
                ref_lab, _ = ops.vote_project(votes, proj, scores=False)
                assert np.array_equal(ref_lab.cpu().numpy(), lab[:n_full]), ("labels differ from vote_project's", key)
        else:
            assert (lab[:n_full] == sentinel).all(), ("labels written without being asked for", key)
        assert (lab[n_full:] == sentinel).all(), ("written past the labels", key)
    assert np.array_equal(votes.cpu().numpy().view(np.uint16), v.view(np.uint16)), ("the votes changed", what)
    assert np.array_equal(gt_dev.cpu().numpy(), gt), ("the ground truth changed", what)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def case_sizes(dev, impl=None):
    """Every C with every n_full: random projections (repeats, unreferenced rows), the four tables in turn, ground truth with values
    outside the table; labels asked for every second time."""
    rng = np.random.default_rng(21)
    tables = ("identity", "first", "middle", "several")
    turn = 0
    for C in CLASSES:
        n_sub = 70
        v = F._votes(rng, n_sub, C)
        for n_full in N_FULL:
            p = rng.integers(0, n_sub, size=n_full).astype(np.int32)
            if n_full >= 2:
                p[0], p[-1] = n_sub - 1, 0
            lut = some_lut(C, tables[turn % 4])
            check(dev, impl, v, p, some_gt(rng, n_full, C, lut), lut, want_labels=bool(turn & 1), what="sizes")
            turn += 1


def case_projection(dev, impl=None):
    """No projection (the identity, n_full == n_sub); repeats and unreferenced rows; votes that start 19, 38 and 57 halves into their
    buffer (odd and even half-word offsets)."""
    rng = np.random.default_rng(22)
    C = 19
    for n in (1, 65, 257, SHARE + 3):
        v = F._votes(rng, n, C)
        check(dev, impl, v, None, some_gt(rng, n, C, None, outside=False), None, what="identity")
        check(dev, impl, v, None, some_gt(rng, n, C, None, outside=False), None, a_in=1, what="identity, odd base")
    n_sub = 200
    v = F._votes(rng, n_sub, C)
    v[:, 0] = 0
    for name, p in (("all indices equal", np.full(300, 77)), ("heavy repeats", rng.integers(0, 7, size=3000) * 28),
                    ("most rows unreferenced", np.array([199, 0, 5, 5, 198])), ("a permutation", rng.permutation(n_sub))):
        for a_in in (0, 1, 2, 3):
            check(dev, impl, v, p, some_gt(rng, len(p), C, None, outside=False), None, a_in=a_in, what=name)


def case_values(dev, impl=None):
    """The special rows of ``finish_cases.special_rows`` (ties, NaN, -0) at C = 19, 20 and 4: the labels are ``vote_project``'s, byte
    for byte, and the matrix is that of those labels."""
    rng = np.random.default_rng(23)
    for C in (19, 20, 4):
        v = F.halves(np.stack(list(F.special_rows(C).values())))
        n = len(v)
        for p in (np.arange(n), np.arange(n)[::-1], rng.integers(0, n, size=5 * n)):
            check(dev, impl, v, p, some_gt(rng, len(p), C, None, outside=False), None, what="values")
        check(dev, impl, v, None, some_gt(rng, n, C, None, outside=False), None, what="values, identity")


def case_lut(dev, impl=None):
    """Identity; ignored first, middle, several; label values below 0 and beyond the table; every point ignored; a table longer
    than the LDS stage (300 entries)."""
    rng = np.random.default_rng(24)
    n_sub, n_full = 90, 700
    for C in (19, 65):
        v = F._votes(rng, n_sub, C)
        p = rng.integers(0, n_sub, size=n_full).astype(np.int32)
        for which in ("identity", "first", "middle", "several"):
            lut = some_lut(C, which)
            check(dev, impl, v, p, some_gt(rng, n_full, C, lut), lut, what="lut " + which)
        lut = np.full(C + 1, -1, np.int32)
        check(dev, impl, v, p, some_gt(rng, n_full, C, lut, outside=False), lut, what="all ignored")
        check(dev, impl, v, p, np.full(n_full, -3, np.int32), None, what="all outside")
        long_lut = np.concatenate([some_lut(C, "several"), rng.integers(-1, C, size=300).astype(np.int32)])
        check(dev, impl, v, p, some_gt(rng, n_full, C, long_lut), long_lut, what="a long table")


def case_accumulate(dev, impl=None):
    """Two calls into one matrix; a cell that holds 2^32 - 1 on entry (the 64-bit carry), on both sides of the LDS switch."""
    ops = _impl(impl)
    rng = np.random.default_rng(25)
    for C in (19, 65):
        n_sub, n_full = 50, 2 * SHARE + 9
        lut = some_lut(C, "first")
        conf = torch.zeros((C, C), dtype=torch.int64, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        total, total_counts = np.zeros((C, C), np.int64), np.zeros(3, np.int64)
        for call in range(2):
            v = F._votes(rng, n_sub, C)
            p = rng.integers(0, n_sub, size=n_full).astype(np.int32)
            gt = some_gt(rng, n_full, C, lut)
            ops.vote_confusion(torch.from_numpy(v).to(dev), torch.from_numpy(p).to(dev), torch.from_numpy(gt).to(dev), lut,
                               confusion=conf, counts=counts)
            c_, n_ = E.confusion_fast(np.argmax(v, 1)[p], gt, lut, C)
            total += c_
            total_counts += n_
            assert np.array_equal(conf.cpu().numpy(), total) and np.array_equal(counts.cpu().numpy(), total_counts), ("two calls", C, call)
        cell = np.unravel_index(int(np.argmax(c_)), c_.shape)
        assert c_[cell] >= 2
        big = np.zeros((C, C), np.int64)
        big[cell] = 2 ** 32 - 1
        conf = torch.from_numpy(big.copy()).to(dev)
        counts = torch.tensor([2 ** 32 - 1, 2 ** 40, -5], dtype=torch.int64, device=dev)
        ops.vote_confusion(torch.from_numpy(v).to(dev), torch.from_numpy(p).to(dev), torch.from_numpy(gt).to(dev), lut, confusion=conf, counts=counts)
        assert np.array_equal(conf.cpu().numpy(), big + c_), ("the 64-bit carry", C)
        assert np.array_equal(counts.cpu().numpy(), np.array([2 ** 32 - 1, 2 ** 40, -5], np.int64) + n_), ("the counts' carry", C)


def case_contention(dev, impl=None):
    """100 000 points that all land on ONE cell (off the diagonal), on both sides of the LDS switch: the count is exact."""
    for C in (19, 65):
        v = np.zeros((3, C), np.float16)
        v[:, 5] = v[:, 7] = 1.0                         # every row predicts 5 (the first of two maxima)
        n = 100000
        p = (np.arange(n) % 3).astype(np.int32)
        gt = np.full(n, 3, np.int32)                    # the identity table: row 2 after the first value is ignored
        lut = some_lut(C, "first")
        check(dev, impl, v, p, gt, lut, what="contention")
        conf, counts = _impl(impl).vote_confusion(torch.from_numpy(v).to(dev), torch.from_numpy(p).to(dev), torch.from_numpy(gt).to(dev), lut)
        assert int(conf.cpu().numpy()[2, 5]) == n and int(conf.sum()) == n and counts.cpu().tolist() == [n, 0, 0]


def case_scores_f32(dev, impl=None):
    """``score_confusion``: float32 rows, contiguous and as the first C columns of a wider matrix (ld > C), with ties, NaN and -0 rows."""
    ops = _impl(impl)
    rng = np.random.default_rng(27)
    for C, n, extra in ((19, 257, 5), (65, 3 * SHARE + 5, 1), (4, 63, 0), (1, 64, 3), (256, 65, 2)):
        wide = rng.standard_normal((n, C + extra)).astype(np.float32)
        wide[:, C:] = 99.0                               # (a kernel that reads past a row's C columns would predict them)
        if C >= 4:
            wide[::5, :C] = 0.0                          # ties in all columns: the first
            wide[3, :C] = -0.0
            wide[3, C - 1] = 0.0                         # -0 ... -0 +0: equal, the first wins
            wide[7, 1], wide[7, 2] = 5.0, np.nan         # a NaN after the numeric maximum
            wide[9, 2], wide[9, 3] = np.nan, np.nan      # two NaNs: the first
        s = torch.from_numpy(wide).to(dev)[:, :C]
        assert extra == 0 or not s.is_contiguous()
        pred = np.argmax(wide[:, :C], 1)
        for which in ("identity", "several"):
            lut = some_lut(C, which)
            gt = some_gt(rng, n, C, lut)
            want_conf, want_counts = E.confusion_fast(pred, gt, lut, C)
            pre = rng.integers(1, 50, size=(C, C)).astype(np.int64)
            conf = torch.from_numpy(pre.copy()).to(dev)
            counts = torch.tensor([1, 2, 3], dtype=torch.int64, device=dev)
            got = ops.score_confusion(s, torch.from_numpy(gt).to(dev), lut, confusion=conf, counts=counts)
            assert got[0] is conf and got[1] is counts
            assert np.array_equal(conf.cpu().numpy(), pre + want_conf), ("score_confusion", C, n, extra, which)
            assert np.array_equal(counts.cpu().numpy(), np.array([1, 2, 3]) + want_counts), ("score_confusion counts", C, n, which)
            got = ops.score_confusion(s.contiguous(), torch.from_numpy(gt).to(dev), lut)
            assert np.array_equal(got[0].cpu().numpy(), want_conf) and np.array_equal(got[1].cpu().numpy(), want_counts)
    conf, counts = ops.score_confusion(torch.zeros((0, 7), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    assert tuple(conf.shape) == (7, 7) and not conf.cpu().numpy().any() and not counts.cpu().numpy().any()


def case_nan_buffer(dev, impl=None):
    """NaN in every half of the votes' buffer OUTSIDE the referenced rows -- the rows around the slice and the rows no index names --
    changes nothing: the same matrix and labels as with zeros there."""
    rng = np.random.default_rng(28)
    for C in (19, 65):
        n_sub, n_full = 120, SHARE + 77
        used = rng.permutation(n_sub)[:40]
        p = used[rng.integers(0, len(used), size=n_full)].astype(np.int32)
        lut = some_lut(C, "middle")
        gt = some_gt(rng, n_full, C, lut)
        v = F._votes(rng, n_sub, C)
        unused = np.setdiff1d(np.arange(n_sub), used)
        v.view(np.uint16)[unused] = H_NAN
        check(dev, impl, v, p, gt, lut, a_in=1, surround=H_NAN, what="NaN around")


def case_python_checks(dev, impl=None):
    """Every bad argument is refused with a RuntimeError that says "invalid argument"; the good call next to them works."""
    ops = _impl(impl)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    v, p, gt = z((8, 19), torch.float16), z(5, torch.int32), z(5, torch.int32)
    wide = z((8, 40), torch.float16)
    s = z((5, 19), torch.float32)
    bad = (lambda: ops.vote_confusion(v.float(), p, gt),                                              # wrong dtypes
           lambda: ops.vote_confusion(v, p.long(), gt),
           lambda: ops.vote_confusion(v, p, gt.long()),
           lambda: ops.vote_confusion(v, p, gt, confusion=z((19, 19), torch.int32)),
           lambda: ops.vote_confusion(v, p, gt, counts=z(3, torch.int32)),
           lambda: ops.vote_confusion(v, p, gt, labels=z(5, torch.int32)),
           lambda: ops.vote_confusion(wide[:, :19], p, gt),                                            # non-contiguous
           lambda: ops.vote_confusion(v, z(10, torch.int32)[::2], gt),
           lambda: ops.vote_confusion(v, p, z(10, torch.int32)[::2]),
           lambda: ops.vote_confusion(v, p, z(4, torch.int32)),                                        # wrong sizes
           lambda: ops.vote_confusion(v, None, gt),                                                    # identity: n_full == n_sub
           lambda: ops.vote_confusion(v, p, gt, confusion=z((19, 20), torch.int64)),
           lambda: ops.vote_confusion(v, p, gt, counts=z(4, torch.int64)),
           lambda: ops.vote_confusion(v, p, gt, labels=z(4, torch.uint8)),
           lambda: ops.vote_confusion(z((8, 257), torch.float16), p, gt),                              # C = 257
           lambda: ops.vote_confusion(z((0, 19), torch.float16), p, gt),                               # n_sub == 0 with n_full > 0
           lambda: ops.vote_confusion(v, p, gt, lut=np.array([0, 19], np.int32)),                      # a table entry >= C
           lambda: ops.vote_confusion(v, p, gt, lut=np.zeros(0, np.int32)),
           lambda: ops.vote_confusion(v, p, gt, lut=np.zeros((2, 2), np.int32)),
           lambda: ops.vote_confusion(v, p, gt, lut=np.zeros(4, np.float32)),
           lambda: ops.score_confusion(s.half(), gt),
           lambda: ops.score_confusion(s, gt.long()),
           lambda: ops.score_confusion(s, z(4, torch.int32)),
           lambda: ops.score_confusion(z((5, 40), torch.float32)[:, ::2], gt),                         # column stride 2
           lambda: ops.score_confusion(z((5, 257), torch.float32), gt),
           lambda: ops.score_confusion(s, gt, lut=np.array([19], np.int32)),
           lambda: ops.score_confusion(s, gt, confusion=z((19, 19), torch.int32)))
    for i, f in enumerate(bad):
        try:
            f()
        except RuntimeError as e:
            assert "invalid argument" in str(e), (i, str(e))
            continue
        raise AssertionError("bad argument %d was accepted" % i)
    conf, counts = ops.vote_confusion(v, p, gt)
    assert int(conf.cpu().numpy()[0, 0]) == 5 and counts.cpu().tolist() == [5, 0, 0]
    conf, counts, lab = ops.vote_confusion(v, p, gt, labels=True)
    assert lab.dtype == torch.uint8 and lab.cpu().tolist() == [0] * 5
    conf, counts = ops.vote_confusion(v, z(0, torch.int32), z(0, torch.int32))
    assert not conf.cpu().numpy().any() and counts.cpu().tolist() == [0, 0, 0]


DATA_CASES = dict(sizes=case_sizes, projection=case_projection, values=case_values, lut=case_lut, accumulate=case_accumulate,
                  contention=case_contention, scores_f32=case_scores_f32, nan_buffer=case_nan_buffer)
CASES = dict(DATA_CASES, python_checks=case_python_checks)


# ---- model level: inference_many(evaluate=True) ------------------------------------------------------------------------------------
def labelled(clouds, num_classes, seed=31):
    """Three clouds: 0 and 2 carry labels of the FULL cloud drawn from [0, C] (so ignored points occur), 1 carries none."""
    g = np.random.default_rng(seed)
    out = []
    for i, c in enumerate(clouds[:3]):
        c = dict(c)
        if i == 1:
            c.pop("label", None)
        else:
            c["label"] = g.integers(0, num_classes + 1, size=len(c["point"])).astype(np.int32)
        out.append(c)
    return out


def _same_plain(x, y, what):
    """predict_labels, predict_scores (None allowed on both sides) equal."""
    assert len(x) == len(y)
    for i, (a, b) in enumerate(zip(x, y)):
        assert np.array_equal(a["predict_labels"], b["predict_labels"]) and a["predict_labels"].dtype == b["predict_labels"].dtype, (what, i)
        if a["predict_scores"] is None or b["predict_scores"] is None:
            assert a["predict_scores"] is None and b["predict_scores"] is None, (what, i)
        else:
            assert a["predict_scores"].dtype == b["predict_scores"].dtype == np.float16
            assert np.array_equal(a["predict_scores"].view(np.uint16), b["predict_scores"].view(np.uint16)), (what, "scores", i)


def check_model_evaluate(model, clouds, seeds, finish):
    """``inference_many(evaluate=True, finish=finish)`` on 3 clouds at 2 in flight (a slot is refilled), with and without scores,
    against the same call without ``evaluate`` and the restatement."""
    from ml3d.torch.modules import SemSegMetric
    cfg = model.cfg
    C = int(cfg.num_classes)
    ign = list(cfg.ignored_label_inds)
    lut = E.label_lut(C, ign)
    clouds = labelled(clouds, C)
    seeds = list(seeds[:3])
    plain = model.inference_many(clouds, seeds=seeds, max_in_flight=2, finish="device")
    plain_info = model.inference_many_info
    for r in plain:
        assert sorted(r) == ["predict_labels", "predict_scores"]
    for return_scores in (True, False):
        what = (finish, return_scores)
        res = model.inference_many(clouds, seeds=seeds, max_in_flight=2, finish=finish, evaluate=True, return_scores=return_scores)
        info = model.inference_many_info
        metric = model.inference_many_metric
        assert isinstance(metric, SemSegMetric)
        F._same_info(info, plain_info, what)
        if return_scores:
            F._same_results(res, plain, what)
        else:
            assert all(r["predict_scores"] is None for r in res), what
            for a, b in zip(res, plain):
                assert a["predict_labels"].dtype == np.int64 and np.array_equal(a["predict_labels"], b["predict_labels"]), what
        total = np.zeros((C, C), np.int64)
        assert "confusion" not in res[1] and "counts" not in res[1], what
        for i in (0, 2):
            want_conf, want_counts = E.confusion_of(res[i]["predict_labels"], clouds[i]["label"], lut, C)
            assert want_counts[1] > 0 and want_counts[0] > 0, "the labels must hold ignored and scored points"
            got_conf, got_counts = res[i]["confusion"], res[i]["counts"]
            assert got_conf.dtype == np.int64 and got_conf.shape == (C, C) and got_counts.dtype == np.int64 and got_counts.shape == (3,)
            assert got_conf.flags.owndata and got_counts.flags.owndata, "a result must own its memory"
            assert np.array_equal(got_conf, want_conf), (what, "confusion", i)
            assert np.array_equal(got_counts, want_counts), (what, "counts", i)
            total += want_conf
        assert np.array_equal(metric.confusion_matrix, total) and metric.num_classes == C, what
        assert np.array_equal(np.asarray(metric.iou(), np.float64), E.iou(total), equal_nan=True), what
        assert np.array_equal(np.asarray(metric.acc(), np.float64), E.acc(total), equal_nan=True), what


def check_wrong_length_label(model, clouds, seeds):
    """A ``label`` that is not one value per raw point raises before any patch runs (``on_batch`` is never called)."""
    clouds = labelled(clouds, int(model.cfg.num_classes))
    clouds[2]["label"] = clouds[2]["label"][:-1]
    called = []
    for finish in ("device", "host"):
        try:
            model.inference_many(clouds, seeds=list(seeds[:3]), max_in_flight=2, finish=finish, evaluate=True,
                                 on_batch=lambda *a: called.append(1))
        except ValueError as e:
            assert "label" in str(e)
        else:
            raise AssertionError("a label of the wrong length was accepted")
    assert not called
    model.inference_many(clouds[:1], seeds=list(seeds[:1]), max_in_flight=2)        # (without evaluate: no metric)
    assert model.inference_many_metric is None
