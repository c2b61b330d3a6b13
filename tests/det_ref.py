"""numpy restatement of the detection metric (the reference's ml3d/metrics/mAP.py: ``precision_3d`` and ``mAP``), written for the
tests and independent of the product's code: plain loops over frames, classes, difficulties and boxes.  It takes IoU MATRICES as
inputs (the oracle's, in the tests), so it restates the matching and the AP, not the geometry.  tools/gen_golden_det_eval.py
asserts that it reproduces the reference on tests/golden/eval_objdet.npz.

Two levels:
* ``match_ids``      one frame in the id form of ``ml3d_det_match`` (class ids, difficulty bit masks): flags [D, P], fn [C, D];
* ``precision_3d`` / ``mAP``   dicts in, like the reference, with one IoU matrix per frame over the frame's UNFILTERED boxes.
"""
import numpy as np


def match_ids(iou, pcls, pdm, tlab, tdm, min_overlap, similar, D):
    """flags uint8 [D, P] (bit 0 tp, bit 1 fp) and fn int64 [C, D] of one frame.  ``iou`` float32 [P, T]."""
    C, P, T = len(min_overlap), len(pcls), len(tlab)
    flags, fn = np.zeros((D, P), np.uint8), np.zeros((C, D), np.int64)
    for c in range(C):
        mo = np.float32(min_overlap[c])
        rows = [p for p in range(P) if pcls[p] == c]
        cols = [t for t in range(T) if tlab[t] == c or (similar[c] >= 0 and tlab[t] == similar[c])]
        for j in range(D):
            pred_idx = [p for p in rows if (int(pdm[p]) >> j) & 1]
            target_idx = [t for t in cols if tlab[t] == c and (int(tdm[t]) >> j) & 1]
            if not pred_idx:
                fn[c, j] = len(target_idx)
                continue
            elected = set()
            for t in target_idx:
                best = rows[0]
                for p in rows[1:]:
                    if iou[p, t] > iou[best, t]:
                        best = p
                elected.add(best)
            for p in pred_idx:
                fp = all(iou[p, t] < mo for t in cols)
                match = any(iou[p, t] >= mo for t in target_idx)
                tp = False
                if match:
                    fp = True
                    if p in elected:
                        tp, fp = True, False
                flags[j, p] = int(tp) | (int(fp) << 1)
            fn[c, j] = sum(1 for t in target_idx if all(iou[p, t] < mo for p in rows))
    return flags, fn


def vocabulary(classes, similar_classes):
    names = list(classes)
    for v in similar_classes.values():
        if v not in names:
            names.append(v)
    similar = [-1] * len(classes)
    for c, name in enumerate(classes):
        v = similar_classes.get(name)            # (the dict is read with the CLASS as key)
        if v is not None:
            similar[c] = names.index(v)
    return names, similar


def ids_and_masks(data, names, difficulties):
    n = len(data["label"])
    ids, masks = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        for k, name in enumerate(names):
            if data["label"][i] == name:
                ids[i] = k
                break
        for j, lim in enumerate(difficulties):
            if "difficulty" not in data or 0 <= data["difficulty"][i] <= lim:
                masks[i] |= 1 << j
    return ids, masks


def frame_flags(pred, target, iou, classes, difficulties, min_overlap, similar_classes):
    """One frame: (kept = indices of the predictions whose label is in ``classes``, flags uint8 [D, len(kept)], fn [C, D]).
    ``iou`` is [len(pred), len(target)] over the unfiltered boxes."""
    names, similar = vocabulary(classes, similar_classes)
    pc, pm = ids_and_masks(pred, list(classes), difficulties)
    tl, tm = ids_and_masks(target, names, difficulties)
    kept = np.where(pc >= 0)[0]
    iou = np.asarray(iou, np.float32).reshape(len(pc), len(tl))
    flags, fn = match_ids(iou[kept], pc[kept], pm[kept], tl, tm, min_overlap, similar, len(difficulties))
    return kept, flags, fn, pc[kept], pm[kept]


def rows_of(detection):
    """The sorted non-zero (score, tp, fp) rows of every (class, difficulty) of a ``detection`` array [C, D, n, 3]: what AP depends on."""
    out = []
    for c in range(detection.shape[0]):
        for j in range(detection.shape[1]):
            d = detection[c, j]
            d = d[np.any(d != 0, axis=1)]
            out.append(sorted(map(tuple, d.tolist())))
    return out


def precision_3d(pred, target, iou, classes, difficulties, min_overlap, similar_classes):
    """(detection float64 [C, D, n_kept, 3], fns int64 [C, D, 1]); rows at the position among the kept boxes."""
    kept, flags, fn, pc, pm = frame_flags(pred, target, iou, classes, difficulties, min_overlap, similar_classes)
    det = np.zeros((len(classes), len(difficulties), len(kept), 3))
    for c in range(len(classes)):
        for j in range(len(difficulties)):
            for r in range(len(kept)):
                if pc[r] == c and (int(pm[r]) >> j) & 1:
                    det[c, j, r] = (pred["score"][kept[r]], flags[j, r] & 1, (flags[j, r] >> 1) & 1)
    return det, fn[:, :, None]


def thresholds_of(scores, gt_cnt, samples):
    scores = sorted((float(s) for s in scores), reverse=True)
    out, recall = [], 0
    for i, s in enumerate(scores):
        left = (i + 1) / gt_cnt
        last = i == len(scores) - 1
        right = left if last else (i + 2) / gt_cnt
        if not last and (right - recall) < (recall - left):
            continue
        out.append(s)
        recall += 1 / (samples - 1.0)
    return out


def average_precision(rows, gt_cnt, samples):
    """``rows``: (score, tp, fp) triples of one (class, difficulty).  Percent, float64."""
    if samples <= 0:
        return 0.0
    th = thresholds_of([s for s, tp, _ in rows if tp > 0], np.float64(gt_cnt), samples)
    if not th:
        return 0.0
    prec = np.zeros(len(th))
    for k in range(len(th) - 1, -1, -1):
        tp = float(sum(r[1] for r in rows if r[0] >= th[k]))
        fp = float(sum(r[2] for r in rows if r[0] >= th[k]))
        if tp + fp > 0:
            prec[k] = tp / (tp + fp)
        prec[k] = prec[k:].max()
    need = int(samples / 4 + 1)
    if len(prec[::4]) < need:
        return np.sum(prec) / len(prec) * 100
    return np.sum(prec[::4]) / need * 100


def ap_from_flags(flags, scores, pcls, pdm, gt_cnt, samples):
    """float64 [C, D]: ``flags`` uint8 [D, NP] of a whole split in id form, ``gt_cnt`` [C, D]."""
    C, D = gt_cnt.shape
    ap = np.zeros((C, D))
    for c in range(C):
        for j in range(D):
            rows = [(float(scores[p]), float(flags[j, p] & 1), float((flags[j, p] >> 1) & 1))
                    for p in range(len(pcls)) if pcls[p] == c and (int(pdm[p]) >> j) & 1]
            ap[c, j] = average_precision(rows, gt_cnt[c, j], samples)
    return ap


def gt_counts(targets, classes, difficulties):
    cnt = np.zeros((len(classes), len(difficulties)))
    for t in targets:
        ids, masks = ids_and_masks(t, list(classes), difficulties)
        for c in range(len(classes)):
            for j in range(len(difficulties)):
                cnt[c, j] += sum(1 for i in range(len(ids)) if ids[i] == c and (int(masks[i]) >> j) & 1)
    return cnt


def mAP(preds, targets, ious, classes, difficulties, min_overlap, samples, similar_classes):
    """float64 [C, D, 1] of a list of frames with one IoU matrix each."""
    C, D = len(classes), len(difficulties)
    if len(min_overlap) != C:
        min_overlap = list(min_overlap) * C
    rows = [[[] for _ in range(D)] for _ in range(C)]
    for pred, target, iou in zip(preds, targets, ious):
        det, _ = precision_3d(pred, target, iou, classes, difficulties, min_overlap, similar_classes)
        for c in range(C):
            for j in range(D):
                rows[c][j].extend(tuple(r) for r in det[c, j].tolist() if any(v != 0 for v in r))
    gt = gt_counts(targets, classes, difficulties)
    out = np.zeros((C, D, 1))
    for c in range(C):
        for j in range(D):
            out[c, j, 0] = average_precision(rows[c][j], gt[c, j], samples)
    return out
