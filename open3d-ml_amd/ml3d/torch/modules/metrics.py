"""``SemSegMetric``: the confusion matrix, per-class accuracy and IoU of semantic segmentation -- the reference's
ml3d/torch/modules/metrics/semseg_metric.py, the parity metric of SURVEY.md.  Device tensors are scored on the device
(``ops.score_confusion``) and the matrix stays there until it is asked for; host inputs are scored by numpy to the same contract."""
import warnings

import numpy as np
import torch

from ... import ops
from ...metrics.mAP import ObjdetMetric   # noqa: F401  (the detection counterpart, scored by ops.det_match)


def host_confusion(pred, gt, lut, num_classes):
    """``ops.vote_confusion``'s contract on host arrays of predicted labels and label VALUES: (int64 [C, C] with row = truth and
    column = prediction, int64 [3] = points scored, ignored (``lut`` < 0), outside the table).  ``lut=None``: the identity."""
    n_cls = int(num_classes)
    table = np.arange(n_cls, dtype=np.int64) if lut is None else np.asarray(lut, dtype=np.int64)
    pred = np.asarray(pred, dtype=np.int64).ravel()
    gt = np.asarray(gt, dtype=np.int64).ravel()
    known = (gt >= 0) & (gt < table.size)
    rows = np.where(known, table[np.where(known, gt, 0)], n_cls)          # n_cls: outside
    scored = rows < n_cls
    scored &= rows >= 0
    cells = np.bincount(rows[scored] * n_cls + pred[scored], minlength=n_cls * n_cls)
    n_scored, n_known = int(scored.sum()), int(known.sum())
    return cells.reshape(n_cls, n_cls).astype(np.int64), np.array([n_scored, n_known - n_scored, gt.size - n_known], dtype=np.int64)


def _ratios(num, den):
    """num / den per class as float64, NaN where den is 0, followed by the mean of the entries that are not NaN."""
    den = den.astype(np.float64)
    per_class = np.full(den.shape, np.nan)
    np.divide(num.astype(np.float64), den, out=per_class, where=den != 0)
    return [float(v) for v in per_class] + [float(np.nanmean(per_class))]


class SemSegMetric(object):
    """Accumulates a confusion matrix (row = truth, column = prediction) and computes accuracy and IoU from it."""

    def __init__(self):
        self._host = None          # numpy int64 [C, C]: what arrived on the host
        self._dev = None           # device int64 [C, C]: what was scored on the device, not yet read back
        self._dev_counts = None    # device int64 [3], likewise
        self._host_counts = np.zeros(3, np.int64)
        self.num_classes = None

    @property
    def confusion_matrix(self):
        """numpy int64 [C, C], or None before the first update.  Reads the device part back, once."""
        if self._dev is not None:
            part = self._dev.cpu().numpy()
            self._dev = None
            self._host = part if self._host is None else self._host + part
        return self._host

    def _classes(self, C):
        if self.num_classes is None or (self._host is None and self._dev is None):      # (the first update, or the first after reset())
            self.num_classes = int(C)
        assert self.num_classes == int(C), "confusion matrices of %d and %d classes" % (self.num_classes, int(C))

    def add_confusion(self, conf):
        """Add a [C, C] confusion matrix: a numpy array, or a device tensor (int64; added on the device)."""
        if isinstance(conf, torch.Tensor) and conf.device.type != "cpu":
            self._classes(conf.shape[0])
            self._dev = conf.to(torch.int64).clone() if self._dev is None else self._dev.add_(conf)
            return
        conf = np.asarray(conf.numpy() if isinstance(conf, torch.Tensor) else conf).astype(np.int64)
        assert conf.ndim == 2 and conf.shape[0] == conf.shape[1]
        self._classes(conf.shape[0])
        self._host = conf.copy() if self._host is None else self._host + conf

    def update(self, scores, labels, ignored_label_inds=None):
        """``scores`` [..., C] and ``labels`` [...]: labels that are already valid (the reference's call, after filter_valid_label)
        or, with ``ignored_label_inds``, the dataset's label values, which go through ``ops.label_lut`` here.  Device tensors are
        scored by ``ops.score_confusion``, host inputs by numpy, with ONE contract: a label outside the table is not scored on
        either path but counted in ``counts[2]`` (the reference would fold such labels into other cells or raise; a warning is
        issued when the counts are read and hold any)."""
        C = int(scores.shape[-1])
        lut = None if ignored_label_inds is None else ops.label_lut(C, ignored_label_inds)
        if isinstance(scores, torch.Tensor) and scores.device.type != "cpu":
            self._classes(C)
            s = scores.detach().reshape(-1, C).float()
            gt = labels.detach().reshape(-1).to(device=s.device, dtype=torch.int32).contiguous()
            if self._dev is None:
                self._dev = torch.zeros((C, C), dtype=torch.int64, device=s.device)
            if self._dev_counts is None:
                self._dev_counts = torch.zeros(3, dtype=torch.int64, device=s.device)
            ops.score_confusion(s if s.stride(-1) == 1 else s.contiguous(), gt, lut, confusion=self._dev, counts=self._dev_counts)
            return
        s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
        lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        conf, counts = host_confusion(np.argmax(s.reshape(-1, C), axis=1), lab, lut, C)
        self.add_confusion(conf)
        self._host_counts += counts

    @property
    def counts(self):
        """numpy int64 [3]: the points ``update`` scored, ignored and found outside the label table so far (matrices handed to
        ``add_confusion`` bring no counts).  Reads the device part back."""
        if self._dev_counts is not None:
            self._host_counts += self._dev_counts.cpu().numpy()
            self._dev_counts = None
        if self._host_counts[2]:
            warnings.warn("SemSegMetric: %d labels lay outside the label table and were not scored" % int(self._host_counts[2]))
        return self._host_counts.copy()

    def acc(self):
        """Per-class accuracy (NaN for a class without points) followed by the mean of the others; None before the first update."""
        cm = self.confusion_matrix
        if cm is None:
            return None
        return _ratios(np.diagonal(cm), cm.sum(axis=1))

    def iou(self):
        """Per-class IoU (NaN for a class neither present nor predicted) followed by the mIoU; None before the first update."""
        cm = self.confusion_matrix
        if cm is None:
            return None
        hits = np.diagonal(cm)
        return _ratios(hits, cm.sum(axis=1) + cm.sum(axis=0) - hits)

    def reset(self):
        self._host = self._dev = self._dev_counts = None
        self._host_counts = np.zeros(3, np.int64)
