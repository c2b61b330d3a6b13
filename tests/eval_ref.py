"""The numpy restatement of ground-truth scoring: the reference's ``filter_valid_label`` (ml3d/torch/modules/losses/semseg_loss.py:7-38)
and ``SemSegMetric`` (ml3d/torch/modules/metrics/semseg_metric.py), and the contract of ``ml3d_vote_confusion`` in their terms.
tests/test_eval_host.py pins it to tests/golden/eval_semseg.npz, which tools/gen_golden_eval.py wrote from the REAL reference; the
op and model tests judge the product by it where the reference does not exist."""
import numpy as np


def label_lut(num_classes, ignored_label_inds):
    """int64 table label VALUE -> matrix row, -1 for an ignored value: an identity over the classes with a zero inserted at every
    ignored index >= 0, in LIST order (the reference's ``reducing_list``), then -1 at every ignored index."""
    table = list(range(int(num_classes)))
    for i in ignored_label_inds:
        if i >= 0:
            table = table[:i] + [0] + table[i:]
    table = np.asarray(table, np.int64)
    for i in ignored_label_inds:
        if 0 <= i < table.size:
            table[i] = -1
    return table


def filter_valid(labels, num_classes, ignored_label_inds):
    """(indices of the points the reference keeps, their renumbered labels)."""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    ignored = np.zeros(labels.shape, bool)
    for i in ignored_label_inds:
        ignored |= labels == i
    keep = np.nonzero(~ignored)[0]
    table = list(range(int(num_classes)))
    for i in ignored_label_inds:
        if i >= 0:
            table = table[:i] + [0] + table[i:]
    return keep, np.asarray(table, np.int64)[labels[keep]]


def first_argmax(rows):
    """np.argmax over the last axis: the first maximum, the first NaN wins."""
    return np.argmax(np.asarray(rows), axis=-1)


def confusion_of(pred, gt, lut, num_classes):
    """(confusion int64 [C, C] with row = truth and column = prediction, counts int64 [3] = scored, ignored, outside the table)."""
    C = int(num_classes)
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    gt = np.asarray(gt).reshape(-1).astype(np.int64)
    lut = np.arange(C, dtype=np.int64) if lut is None else np.asarray(lut).astype(np.int64)
    conf = np.zeros((C, C), np.int64)
    counts = np.zeros(3, np.int64)
    for p, g in zip(pred.tolist(), gt.tolist()):
        if g < 0 or g >= lut.size:
            counts[2] += 1
        elif lut[g] < 0:
            counts[1] += 1
        else:
            conf[lut[g], p] += 1
            counts[0] += 1
    return conf, counts


def confusion_fast(pred, gt, lut, num_classes):
    """``confusion_of`` by bincount, for the large cases."""
    C = int(num_classes)
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    gt = np.asarray(gt).reshape(-1).astype(np.int64)
    lut = np.arange(C, dtype=np.int64) if lut is None else np.asarray(lut).astype(np.int64)
    inside = (gt >= 0) & (gt < lut.size)
    row = np.full(gt.shape, -1, np.int64)
    row[inside] = lut[gt[inside]]
    ok = inside & (row >= 0)
    conf = np.bincount(C * row[ok] + pred[ok], minlength=C * C).reshape(C, C).astype(np.int64)
    return conf, np.array([ok.sum(), (inside & ~ok).sum(), (~inside).sum()], np.int64)


def acc(conf):
    """semseg_metric.py:26-56: per-class accuracy, then their nanmean (NaN where a class has no points)."""
    out = []
    for c in range(conf.shape[0]):
        tp = int(conf[c, c])
        fn = int(conf[c, :].sum()) - tp
        out.append(float("nan") if tp + fn == 0 else tp / (tp + fn))
    out.append(np.nanmean(out))
    return np.asarray(out, np.float64)


def iou(conf):
    """semseg_metric.py:58-89: per-class IoU, then the mIoU."""
    out = []
    for c in range(conf.shape[0]):
        tp = int(conf[c, c])
        fn = int(conf[c, :].sum()) - tp
        fp = int(conf[:, c].sum()) - tp
        out.append(float("nan") if tp + fp + fn == 0 else tp / (tp + fp + fn))
    out.append(np.nanmean(out))
    return np.asarray(out, np.float64)
