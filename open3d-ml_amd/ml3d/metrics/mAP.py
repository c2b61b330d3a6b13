"""Detection scoring: ``filter_data``, ``precision_3d``, ``sample_thresholds``, ``mAP`` with the signatures, defaults and return
shapes of the reference's ml3d/metrics/mAP.py, and ``ObjdetMetric``, the detection counterpart of ``SemSegMetric``.

The matching of every frame's predictions against its ground truth is ONE call of ``ops.det_match`` (``ml3d_det_match``: two
launches whatever the number of frames, classes and difficulties): the host maps labels and difficulties to ids and bit masks
with vectorised numpy, uploads the concatenated arrays once, and reads one buffer back -- a flag byte per box, metric and
difficulty, and the miss counts.  The IoU matrices never leave the device.  The AP part runs on the host in float64.

``ML3D_DET_EVAL=host`` (read per call) scores frame by frame on ``ops.iou_bev`` / ``ops.iou_3d`` instead, one upload, launch and
read-back per frame and metric: the route before ``det_match``, kept as the A/B baseline and as the route for non-finite boxes,
which are outside the kernel's contract.  Both routes give equal results.

The contract is the reference's CODE, quirks included (the det_match section): the tp rule, the arg-max over the rows
of all difficulties, and ``similar_classes`` read with the CLASS as key."""
import os
import warnings

import numpy as np
import torch

from .. import ops

_warned_nonfinite = False
STATS = {"det_match": 0, "uploads": 0, "readbacks": 0, "iou_launches": 0}      # counted per route, for tools/bench_det_eval.py


def _route():
    return "host" if os.environ.get("ML3D_DET_EVAL", "device") == "host" else "device"


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _equals(values, name):
    """``values == name`` as a boolean array, all False where numpy will not compare the two element-wise (None, a name of
    another kind)."""
    if name is None:
        return np.zeros(values.shape, bool)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hit = values == name
    return hit if isinstance(hit, np.ndarray) and hit.shape == values.shape else np.zeros(values.shape, bool)


def filter_data(data, labels, diffs=None):
    """The entries of ``data`` (a dict of numpy arrays with a ``label`` entry) whose label is one of ``labels`` and, with ``diffs``
    and a ``difficulty`` entry, whose difficulty d satisfies 0 <= d <= diff for one of them: (filtered dict, kept indices)."""
    lab = np.asarray(data["label"])
    keep = np.zeros(lab.shape, bool)
    for name in labels:
        keep |= _equals(lab, name)
    if diffs is not None and "difficulty" in data:
        d = np.asarray(data["difficulty"])
        ok = np.zeros(lab.shape, bool)
        for diff in diffs:
            ok |= (d >= 0) & (d <= diff)
        keep &= ok
    idx = np.where(keep)[0]
    return {k: data[k][idx] for k in data}, idx


# ---- host side of det_match: labels -> ids, difficulties -> bit masks ----------------------------------------------------------------
def _vocabulary(classes, similar_classes):
    """(names, similar): ids 0 .. C - 1 are ``classes``, the dict's other values follow; ``similar[c]`` = the id of
    ``similar_classes.get(classes[c])`` -- the dict is read with the CLASS as key, as the reference reads it -- or -1."""
    names = list(classes)
    for v in similar_classes.values():
        if not any(v == n for n in names):
            names.append(v)
    similar = np.full(len(classes), -1, np.int32)
    for c, name in enumerate(classes):
        v = similar_classes.get(name)
        if v is not None:
            similar[c] = next(i for i, n in enumerate(names) if n == v)
    return names, similar


def _ids(labels, names):
    """int32 id per label: the index of the FIRST of ``names`` it equals, -1 for none."""
    out = np.full(labels.shape, -1, np.int32)
    for k in range(len(names) - 1, -1, -1):
        out[_equals(labels, names[k])] = k
    return out


class _Side(object):
    """One side (predictions or targets) of a split, concatenated over its frames and cut down to the kept boxes."""

    def __init__(self, frames, names, num_names, difficulties, with_score):
        F = len(frames)
        counts = np.array([len(d["label"]) for d in frames], np.int64)
        frame_of = np.repeat(np.arange(F), counts)
        labs = [np.asarray(d["label"]) for d in frames if len(d["label"])]
        if not labs:
            ids = np.zeros(0, np.int32)
        elif len({a.dtype.kind for a in labs}) == 1:
            ids = _ids(np.concatenate(labs), names[:num_names])
        else:                                              # (frames whose labels are of different kinds: numpy would coerce them)
            ids = np.concatenate([_ids(a, names[:num_names]) for a in labs])
        D = len(difficulties)
        every = np.uint32(0xffffffff if D >= 32 else (1 << D) - 1)
        dm = np.full(ids.shape, every, np.uint32)
        has = np.array(["difficulty" in d for d in frames], bool)
        if has.any():
            diff = np.concatenate([np.asarray(d["difficulty"], np.float64).reshape(-1) if "difficulty" in d else np.zeros(len(d["label"]))
                                   for d in frames] or [np.zeros(0)])
            bits = np.zeros(ids.shape, np.uint32)
            for j, lim in enumerate(difficulties):
                bits |= (((diff >= 0) & (diff <= lim)).astype(np.uint32) << np.uint32(j))
            dm = np.where(has[frame_of], bits, dm).astype(np.uint32)
        keep = ids >= 0
        boxes = [np.asarray(d["bbox"], np.float32).reshape(len(d["label"]), -1)[:, :7] for d in frames if len(d["label"])]
        box = np.concatenate(boxes) if boxes else np.zeros((0, 7), np.float32)
        self.box = np.ascontiguousarray(box[keep], np.float32)
        self.ids = ids[keep]
        self.dmask = dm[keep]
        self.start = np.zeros(F + 1, np.int64)
        np.cumsum(np.bincount(frame_of[keep], minlength=F), out=self.start[1:])
        self.score = None
        if with_score:
            sc = [np.asarray(d["score"], np.float64).reshape(-1) for d in frames if len(d["label"])]
            self.score = (np.concatenate(sc) if sc else np.zeros(0))[keep]


class _Split(object):
    def __init__(self, pred, target, classes, difficulties, min_overlap, similar_classes):
        assert len(pred) == len(target), "one target dict per prediction dict"
        assert 1 <= len(difficulties) <= 32, "1 .. 32 difficulties"
        self.C, self.D, self.F = len(classes), len(difficulties), len(pred)
        names, self.similar = _vocabulary(classes, similar_classes)
        self.pred = _Side(pred, names, self.C, difficulties, True)
        self.tgt = _Side(target, names, len(names), difficulties, False)
        self.min_overlap = np.asarray(min_overlap, np.float32).reshape(self.C)
        bit = (self.tgt.dmask[None, :] >> np.arange(self.D, dtype=np.uint32)[:, None]) & np.uint32(1)       # [D, NT]
        self.gt_cnt = np.zeros((self.C, self.D))
        for c in range(self.C):
            self.gt_cnt[c] = bit[:, self.tgt.ids == c].sum(axis=1)
        self.finite = bool(np.isfinite(self.pred.box).all() and np.isfinite(self.tgt.box).all())


def _pack(arrays):
    """One uint8 buffer holding ``arrays`` at 16-byte offsets, and the offsets."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    buf = np.zeros(max(total, 16), np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, offs


def _match_device(S, metrics, device):
    """flags uint8 [2, D, NP] and fn int64 [2, C, D] of the split through ONE upload, ONE ``ops.det_match``, ONE read-back."""
    NP, C, D = len(S.pred.ids), S.C, S.D
    if NP == 0 or S.F == 0:                                 # (the C entry point's no-op: every target of a difficulty is a miss)
        fn = np.zeros((2, C, D), np.int64)
        for m in range(2):
            if (metrics >> m) & 1:
                fn[m] = S.gt_cnt.astype(np.int64)
        return np.zeros((2, D, NP), np.uint8), fn
    pair_start = ops.det_pair_starts(S.pred.start, S.tgt.start)
    arrays = [S.pred.box, S.pred.ids, S.pred.dmask.view(np.int32), S.pred.start, S.tgt.box, S.tgt.ids, S.tgt.dmask.view(np.int32),
              S.tgt.start, pair_start, S.min_overlap, S.similar]
    dtypes = [torch.float32, torch.int32, torch.int32, torch.int64, torch.float32, torch.int32, torch.int32, torch.int64, torch.int64,
              torch.float32, torch.int32]
    host, offs = _pack(arrays)
    buf = torch.from_numpy(host).to(device)
    STATS["uploads"] += 1
    t = [buf[o:o + a.nbytes].view(dt) for a, o, dt in zip(arrays, offs, dtypes)]
    t[0], t[4] = t[0].view(-1, 7), t[4].view(-1, 7)
    n_fn = 2 * C * D * 8
    out = torch.zeros(n_fn + 2 * D * NP, dtype=torch.uint8, device=device)
    fn_dev, flags_dev = out[:n_fn].view(torch.int64).view(2, C, D), out[n_fn:].view(2, D, NP)
    ops.det_match(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[9], t[10], D, metrics=metrics, out_flags=flags_dev, out_fn=fn_dev,
                  pair_start=t[8], num_pairs=int(pair_start[-1]))
    STATS["det_match"] += 1
    got = out.cpu().numpy()
    STATS["readbacks"] += 1
    return got[n_fn:].reshape(2, D, NP).copy(), got[:n_fn].view(np.int64).reshape(2, C, D).copy()


def match_frame(iou, pcls, pdm, tlab, tdm, min_overlap, similar, D):
    """The matching rules on ONE frame's IoU matrix [P, T] in numpy: (flags uint8 [D, P], fn int64 [C, D]) to ``det_match``'s
    contract.  The host route's matcher."""
    C, P = len(min_overlap), len(pcls)
    flags, fn = np.zeros((D, P), np.uint8), np.zeros((C, D), np.int64)
    for c in range(C):
        rows = np.where(pcls == c)[0]
        own = tlab == c
        cols = np.where(own | ((tlab == similar[c]) if similar[c] >= 0 else np.zeros(len(tlab), bool)))[0]
        sub = iou[np.ix_(rows, cols)]
        own = own[cols]
        mo = min_overlap[c]
        nothing = (sub < mo).all(axis=1)
        reached = ~(sub < mo).all(axis=0) if len(rows) else np.zeros(len(cols), bool)
        best = sub.argmax(axis=0) if len(rows) else np.zeros(len(cols), np.int64)
        for j in range(D):
            r_in = ((pdm[rows] >> np.uint32(j)) & np.uint32(1)).astype(bool)
            t_in = own & ((tdm[cols] >> np.uint32(j)) & np.uint32(1)).astype(bool)
            if not r_in.any():
                fn[c, j] = t_in.sum()
                continue
            match = (sub[:, t_in] >= mo).any(axis=1)
            elected = np.zeros(len(rows), bool)
            elected[best[t_in]] = True
            tp = match & elected & r_in
            fp = (nothing | match) & ~tp & r_in
            flags[j, rows] = tp.astype(np.uint8) | (fp.astype(np.uint8) << 1)
            fn[c, j] = (t_in & ~reached).sum()
    return flags, fn


def _match_host(S, metrics, device):
    """The route before ``det_match``: per frame and metric one upload, one IoU launch and one read-back of the matrix."""
    NP, C, D = len(S.pred.ids), S.C, S.D
    flags, fn = np.zeros((2, D, NP), np.uint8), np.zeros((2, C, D), np.int64)
    for f in range(S.F):
        p0, p1, t0, t1 = S.pred.start[f], S.pred.start[f + 1], S.tgt.start[f], S.tgt.start[f + 1]
        for m in range(2):
            if not (metrics >> m) & 1:
                continue
            a, b = S.pred.box[p0:p1], S.tgt.box[t0:t1]
            if p1 > p0 and t1 > t0:
                if m == 0:
                    a, b = a[:, [0, 2, 3, 5, 6]], b[:, [0, 2, 3, 5, 6]]
                both = torch.from_numpy(np.concatenate([a, b])).to(device)
                iou = (ops.iou_bev if m == 0 else ops.iou_3d)(both[:len(a)], both[len(a):]).cpu().numpy()
                STATS["uploads"] += 1
                STATS["iou_launches"] += 1
                STATS["readbacks"] += 1
            else:
                iou = np.zeros((p1 - p0, t1 - t0), np.float32)
            fl, n = match_frame(iou, S.pred.ids[p0:p1], S.pred.dmask[p0:p1], S.tgt.ids[t0:t1], S.tgt.dmask[t0:t1], S.min_overlap,
                                S.similar, D)
            flags[m][:, p0:p1] = fl
            fn[m] += n
    return flags, fn


def _match(S, metrics, device):
    global _warned_nonfinite
    route = _route()
    if route == "device" and not S.finite:
        if not _warned_nonfinite:
            warnings.warn("mAP: non-finite boxes are outside ml3d_det_match's contract; scoring frame by frame on the host route")
            _warned_nonfinite = True
        route = "host"
    return (_match_host if route == "host" else _match_device)(S, metrics, _device(device))


def _detection(S, flags):
    """float64 [C, D, NP, 3] = (score, tp, fp) of the boxes of pred_idx, zeros elsewhere; ``flags`` uint8 [D, NP] of one metric."""
    det = np.zeros((S.C, S.D, len(S.pred.ids), 3))
    bit = ((S.pred.dmask[None, :] >> np.arange(S.D, dtype=np.uint32)[:, None]) & np.uint32(1)).astype(bool)
    for c in range(S.C):
        sel = bit & (S.pred.ids == c)[None, :]
        det[c, :, :, 0] = np.where(sel, S.pred.score[None, :], 0.0)
        det[c, :, :, 1] = np.where(sel, flags & 1, 0)
        det[c, :, :, 2] = np.where(sel, (flags >> 1) & 1, 0)
    return det


def precision_3d(pred, target, classes=[0], difficulties=[0], min_overlap=[0.5], bev=True, similar_classes={}, device=None):
    """One frame: (``detection`` float64 [C, D, n_kept, 3] = (score, tp, fp) per box of ``filter_data(pred, classes)``, at the box's
    position among those kept boxes, zeros where the box is of another class or difficulty; ``fns`` int64 [C, D, 1])."""
    if len(min_overlap) != len(classes):
        min_overlap = list(min_overlap) * len(classes)
    S = _Split([pred], [target], classes, difficulties, min_overlap, similar_classes)
    m = 0 if bev else 1
    flags, fn = _match(S, 1 << m, device)
    return _detection(S, flags[m]), fn[m][:, :, None].astype(np.int64)


def sample_thresholds(scores, gt_cnt, sample_cnt=41):
    """The scores at which recall passes the next of ``sample_cnt`` equally spaced levels, walking the scores downwards."""
    ordered = np.sort(scores)[::-1]
    last = len(ordered) - 1
    step = 1 / (sample_cnt - 1.0)
    level = 0
    picked = []
    for i, s in enumerate(ordered):
        here = (i + 1) / gt_cnt
        ahead = (i + 2) / gt_cnt if i < last else here
        if i < last and (ahead - level) < (level - here):
            continue
        picked.append(s)
        level += step
    return picked


def _average_precision(score, tp, fp, gt_cnt, samples):
    """AP (in percent) of one (class, difficulty): score, tp, fp of its boxes."""
    thresholds = sample_thresholds(score[tp > 0], gt_cnt, samples)
    if len(thresholds) == 0:
        return 0.0
    order = np.argsort(score, kind="stable")
    s_sorted = score[order]
    tp_below = np.concatenate([[0.0], np.cumsum(tp[order])])        # (sums of 0 / 1: exact)
    fp_below = np.concatenate([[0.0], np.cumsum(fp[order])])
    prec = np.zeros((len(thresholds),))
    for ti in range(len(thresholds) - 1, -1, -1):
        k = np.searchsorted(s_sorted, thresholds[ti], side="left")  # boxes with score >= threshold: s_sorted[k:]
        tp_acc, fp_acc = tp_below[-1] - tp_below[k], fp_below[-1] - fp_below[k]
        if (tp_acc + fp_acc) > 0:
            prec[ti] = tp_acc / (tp_acc + fp_acc)
        prec[ti] = np.max(prec[ti:], axis=-1)
    if len(prec[::4]) < int(samples / 4 + 1):
        return np.sum(prec) / len(prec) * 100
    return np.sum(prec[::4]) / int(samples / 4 + 1) * 100


def _ap_table(S, flags, samples):
    """float64 [C, D] from one metric's flags."""
    ap = np.zeros((S.C, S.D))
    if samples <= 0:
        return ap
    for c in range(S.C):
        rows = np.where(S.pred.ids == c)[0]
        for j in range(S.D):
            sel = rows[((S.pred.dmask[rows] >> np.uint32(j)) & np.uint32(1)).astype(bool)]
            fl = flags[j, sel]
            ap[c, j] = _average_precision(S.pred.score[sel], (fl & 1).astype(np.float64), ((fl >> 1) & 1).astype(np.float64),
                                          S.gt_cnt[c, j], samples)
    return ap


def mAP(pred, target, classes=[0], difficulties=[0], min_overlap=[0.5], bev=True, samples=41, similar_classes={}, device=None):
    """AP per class and difficulty, float64 [C, D, 1] in percent, of the lists of prediction and target dicts (``bbox`` [n, 7],
    ``label``, ``score``, optionally ``difficulty``): sampled at ``samples`` recall levels, every fourth of which counts."""
    if len(min_overlap) != len(classes):
        assert len(min_overlap) == 1
        min_overlap = list(min_overlap) * len(classes)
    S = _Split(pred, target, classes, difficulties, min_overlap, similar_classes)
    if samples <= 0:
        return np.zeros((S.C, S.D, 1))
    m = 0 if bev else 1
    flags, _ = _match(S, 1 << m, device)
    return _ap_table(S, flags[m], samples)[:, :, None]


class ObjdetMetric(object):
    """Collects prediction / target dicts on the host and scores them in one pass: ``compute()`` is one ``det_match`` for BEV and
    3-D together (one polygon clip per pair feeds both) and returns ``{"bev": [C, D], "3d": [C, D]}``, what two ``mAP`` calls
    return without the trailing axis."""

    def __init__(self, classes, difficulties=[0], min_overlap=[0.5], similar_classes={}, samples=41, device=None):
        self.classes, self.difficulties, self.similar_classes = list(classes), list(difficulties), dict(similar_classes)
        min_overlap = list(min_overlap)
        if len(min_overlap) != len(self.classes):
            assert len(min_overlap) == 1
            min_overlap = min_overlap * len(self.classes)
        self.min_overlap, self.samples, self.device = min_overlap, samples, device
        self.reset()

    def reset(self):
        self._pred, self._target, self._result, self.fn = [], [], None, None

    def update(self, pred_dicts, target_dicts):
        if isinstance(pred_dicts, dict):
            pred_dicts, target_dicts = [pred_dicts], [target_dicts]
        assert len(pred_dicts) == len(target_dicts)
        self._pred.extend(pred_dicts)
        self._target.extend(target_dicts)
        self._result = None

    def compute(self):
        S = _Split(self._pred, self._target, self.classes, self.difficulties, self.min_overlap, self.similar_classes)
        if self.samples <= 0:
            flags = np.zeros((2, S.D, len(S.pred.ids)), np.uint8)
        else:
            flags, self.fn = _match(S, 3, self.device)
        self._result = {"bev": _ap_table(S, flags[0], self.samples), "3d": _ap_table(S, flags[1], self.samples)}
        return self._result

    def overall(self):
        """The two numbers ``run_valid`` logs: the mean over the classes of the LAST difficulty's AP."""
        r = self._result if self._result is not None else self.compute()
        return {k: float(np.mean(v[:, -1])) for k, v in r.items()}
