"""CPU, no library: the bodies of tests/eval_cases.py run against numpy stand-ins for ``ops.vote_confusion`` / ``ops.score_confusion``.
The right one passes every case; each wrong one is rejected by every case that covers its edge:

* a transposed matrix                          * the LAST maximum instead of the first
* ignored points counted (in row 0)            * overwrite instead of add
* the LUT not applied                          * out-of-range label values clamped instead of skipped
"""
import numpy as np
import pytest
import torch

import eval_cases as V
import test_finish_cases_can_fail as FF


def _last_max(v):
    return v.shape[1] - 1 - np.argmax(v[:, ::-1], 1)


class Standin:
    """``vote_confusion`` / ``score_confusion`` / ``vote_project`` in numpy on CPU tensors, with one switch per wrong behaviour."""

    def __init__(self, transposed=False, count_ignored=False, apply_lut=True, argmax=FF._first_max, add=True, clamp=False):
        self.transposed, self.count_ignored, self.apply_lut, self.argmax, self.add, self.clamp = \
            transposed, count_ignored, apply_lut, argmax, add, clamp
        self.vote_project = FF.standin()                  # (the RIGHT labels: what out_labels is compared with)

    def _sum(self, pred, gt, lut, C, confusion, counts):
        lut = np.arange(C, dtype=np.int64) if (lut is None or not self.apply_lut) else np.asarray(lut).astype(np.int64)
        gt = gt.numpy().astype(np.int64)
        if self.clamp:
            gt = np.clip(gt, 0, lut.size - 1)
        if self.count_ignored:
            lut = np.where(lut < 0, 0, lut)               # (the reference's table before the ignored entries are marked)
        inside = (gt >= 0) & (gt < lut.size)
        row = np.full(gt.shape, -1, np.int64)
        row[inside] = lut[gt[inside]]
        inside &= row < C
        ok = inside & (row >= 0)
        conf = np.bincount(C * row[ok] + pred[ok], minlength=C * C).reshape(C, C).astype(np.int64)
        if self.transposed:
            conf = conf.T.copy()
        cnt = np.array([ok.sum(), (inside & ~ok).sum(), (~inside).sum()], np.int64)
        if confusion is None:
            confusion = torch.zeros((C, C), dtype=torch.int64)
        if counts is None:
            counts = torch.zeros(3, dtype=torch.int64)
        if self.add:
            confusion += torch.from_numpy(conf)
            counts += torch.from_numpy(cnt)
        else:
            confusion.copy_(torch.from_numpy(conf))
            counts.copy_(torch.from_numpy(cnt))
        return confusion, counts

    def vote_confusion(self, votes, proj_inds, gt_labels, lut=None, confusion=None, counts=None, labels=False):
        v = FF._rows(votes).view(np.float16)
        C = v.shape[1]
        pred = self.argmax(v) if proj_inds is None else self.argmax(v)[proj_inds.numpy()]
        confusion, counts = self._sum(pred, gt_labels, lut, C, confusion, counts)
        if labels is False:
            return confusion, counts
        out = labels if isinstance(labels, torch.Tensor) else torch.empty(len(pred), dtype=torch.uint8)
        out.copy_(torch.from_numpy(pred.astype(np.uint8)))
        return confusion, counts, out

    def score_confusion(self, scores, gt_labels, lut=None, confusion=None, counts=None):
        s = scores.numpy()
        return self._sum(self.argmax(s) if len(s) else np.zeros(0, np.int64), gt_labels, lut, s.shape[1], confusion, counts)


EVERY = tuple(sorted(V.DATA_CASES))
WRONG = {
    "transposed": (Standin(transposed=True), EVERY),                                  # every case has cells off the diagonal
    "ignored counted": (Standin(count_ignored=True), ("sizes", "lut", "accumulate", "scores_f32", "nan_buffer")),
    "LUT not applied": (Standin(apply_lut=False), ("sizes", "lut", "accumulate", "contention", "scores_f32", "nan_buffer")),
    "last maximum": (Standin(argmax=_last_max), EVERY),                               # every case has tied rows and C > 1
    "overwrite": (Standin(add=False), EVERY),                                         # every case adds to a non-zero matrix
    "clamped": (Standin(clamp=True), ("sizes", "lut", "accumulate", "scores_f32", "nan_buffer")),
}


@pytest.mark.parametrize("case", EVERY)
def test_the_right_standin_passes(case):
    V.DATA_CASES[case]("cpu", Standin())


@pytest.mark.parametrize("name,case", [(n, c) for n in sorted(WRONG) for c in WRONG[n][1]])
def test_a_wrong_standin_is_rejected_where_its_edge_is_covered(name, case):
    with pytest.raises(AssertionError):
        V.DATA_CASES[case]("cpu", WRONG[name][0])
