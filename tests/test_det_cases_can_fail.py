"""CPU, no library: the bodies of tests/det_cases.py run against stand-ins for ``ops.det_match`` (numpy on CPU tensors, the IoUs in
float64 from the CPU oracle's).  The right one passes every case; each wrong one is rejected by every case that covers its edge:

* the tp rule as "best AND matches that same target"      * similar targets counted as misses
* the arg-max over the rows of ``pred_idx`` only            * similar targets allowed to give tp
* ties to the LAST row                                      * ``>`` in place of ``>=`` at the overlap
* ``fn`` overwritten instead of added to                    * difficulty tested as ``==`` (a box counts in its own level only)
"""
import numpy as np
import pytest
import torch

import det_cases as V
from oracle import ops as oops

_IOU = {}


def _oracle_iou(a, b, mode3d):
    key = (a.tobytes(), b.tobytes(), mode3d)
    if key not in _IOU:
        _IOU[key] = (oops.iou_3d(a, b) if mode3d else oops.iou_bev(a[:, [0, 2, 3, 5, 6]], b[:, [0, 2, 3, 5, 6]])).reshape(len(a), len(b))
    return _IOU[key]


class Standin:
    """``det_match`` / ``iou_bev`` / ``iou_3d`` / ``det_pair_starts`` with one switch per wrong behaviour."""

    def __init__(self, same_target=False, pred_idx_argmax=False, last_tie=False, similar_missed=False, similar_tp=False, strict=False,
                 add=True, own_level=False):
        self.same_target, self.pred_idx_argmax, self.last_tie, self.similar_missed, self.similar_tp, self.strict, self.add, self.own_level = \
            same_target, pred_idx_argmax, last_tie, similar_missed, similar_tp, strict, add, own_level

    @staticmethod
    def det_pair_starts(ps, ts):
        out = np.zeros(len(ps), np.int64)
        np.cumsum(np.diff(ps) * np.diff(ts), out=out[1:])
        return out

    @staticmethod
    def iou_bev(a, b):
        a, b = a.numpy(), b.numpy()
        pad = lambda x: np.stack([x[:, 0], 0 * x[:, 0], x[:, 1], x[:, 2], 1 + 0 * x[:, 0], x[:, 3], x[:, 4]], 1).astype(np.float32)
        return torch.from_numpy(_oracle_iou(pad(a), pad(b), False))

    @staticmethod
    def iou_3d(a, b):
        return torch.from_numpy(_oracle_iou(a.numpy(), b.numpy(), True))

    def _levels(self, mask, D):
        bits = [(int(mask) >> j) & 1 for j in range(D)]
        if self.own_level and any(bits):
            first = bits.index(1)
            bits = [int(j == first) for j in range(D)]
        return bits

    def _frame(self, iou, pcls, pdm, tlab, tdm, mo, similar, D):
        C, P, T = len(mo), len(pcls), len(tlab)
        iou = iou.astype(np.float64)
        flags, fn = np.zeros((D, P), np.uint8), np.zeros((C, D), np.int64)
        hit = (lambda v, m: v > m) if self.strict else (lambda v, m: v >= m)
        for c in range(C):
            m = np.float64(mo[c])
            rows = np.where(pcls == c)[0]
            own = tlab == c
            sim = (tlab == similar[c]) & (similar[c] >= 0)
            cols = np.where(own | sim)[0]
            for j in range(D):
                r_in = np.array([r for r in rows if self._levels(pdm[r], D)[j]], np.int64)
                counted = own | sim if (self.similar_missed or self.similar_tp) else own
                t_in = np.array([t for t in cols if (counted[t] if self.similar_tp else own[t]) and self._levels(tdm[t], D)[j]], np.int64)
                t_miss = np.array([t for t in cols if (counted[t] if self.similar_missed else own[t]) and self._levels(tdm[t], D)[j]], np.int64)
                if not len(r_in):
                    fn[c, j] = len(t_miss)
                    continue
                pool = r_in if self.pred_idx_argmax else rows
                best = {}
                for t in t_in:
                    col = iou[pool, t]
                    k = len(col) - 1 - int(np.argmax(col[::-1])) if self.last_tie else int(np.argmax(col))
                    best[int(t)] = int(pool[k])
                for r in r_in:
                    fp = not any(hit(iou[r, t], m) for t in cols)
                    matched = [int(t) for t in t_in if hit(iou[r, t], m)]
                    tp = False
                    if matched:
                        fp = True
                        elected = any(best[t] == r for t in matched) if self.same_target else r in best.values()
                        if elected:
                            tp, fp = True, False
                    flags[j, r] = int(tp) | (int(fp) << 1)
                fn[c, j] = sum(1 for t in t_miss if not any(hit(iou[r, t], m) for r in rows))
        return flags, fn

    def det_match(self, pred_box, pred_cls, pred_dmask, pred_start, tgt_box, tgt_lab, tgt_dmask, tgt_start, min_overlap, similar,
                  num_difficulties, metrics=3, out_flags=None, out_fn=None, return_iou=False, pair_iou=None):
        D, mo, sim = int(num_difficulties), min_overlap.numpy(), similar.numpy()
        pb, pc, pm = pred_box.numpy(), pred_cls.numpy(), pred_dmask.numpy().view(np.uint32)
        tb, tl, tm = tgt_box.numpy(), tgt_lab.numpy(), tgt_dmask.numpy().view(np.uint32)
        starts = self.det_pair_starts(pred_start, tgt_start)
        if pair_iou.shape[1] < starts[-1]:
            raise RuntimeError("ml3d_det_match: workspace too small")
        F, C = len(pred_start) - 1, len(mo)
        if F == 0 or len(pc) == 0:
            return out_flags, out_fn, pair_iou
        for m in range(2):
            if not (metrics >> m) & 1:
                continue
            total = np.zeros((C, D), np.int64)
            for f in range(F):
                ps, ts = slice(pred_start[f], pred_start[f + 1]), slice(tgt_start[f], tgt_start[f + 1])
                c, lab = pc[ps][:, None], tl[ts][None, :]
                s = sim[np.clip(c, 0, C - 1)]
                rel = (c >= 0) & (c < C) & ((lab == c) | ((s >= 0) & (lab == s)))
                iou = np.zeros(rel.shape, np.float32)
                for k in range(C):
                    rows = np.where(pc[ps] == k)[0]
                    cols = np.where(rel[rows[0]])[0] if len(rows) else rows
                    if len(rows) and len(cols):
                        iou[np.ix_(rows, cols)] = _oracle_iou(pb[ps][rows], tb[ts][cols], m == 1)
                block = pair_iou[m, starts[f]:starts[f + 1]].view(rel.shape)
                block[torch.from_numpy(rel)] = torch.from_numpy(iou[rel])
                fl, n = self._frame(iou, pc[ps], pm[ps], tl[ts], tm[ts], mo, sim, D)
                out_flags[m][:, ps] = torch.from_numpy(fl)
                total += n
            if self.add:
                out_fn[m] += torch.from_numpy(total)
            else:
                out_fn[m] = torch.from_numpy(total)
        return out_flags, out_fn, pair_iou


DATA = ("quirks", "sizes", "seventy_frames", "metrics", "large_frame")
WRONG = {
    "tp needs the same target": (Standin(same_target=True), ("quirks",)),                           # quirks, frame 0
    "arg-max over pred_idx": (Standin(pred_idx_argmax=True), ("quirks", "sizes", "seventy_frames", "metrics")),      # D > 1 and mixed difficulties
    "ties to the last row": (Standin(last_tie=True), DATA),                                          # every case has twins or all-zero columns
    "similar targets missed": (Standin(similar_missed=True), ("quirks", "sizes", "seventy_frames", "metrics")),      # the cases with similar labels
    "similar targets give tp": (Standin(similar_tp=True), ("quirks", "sizes", "seventy_frames", "metrics")),
    "> at the overlap": (Standin(strict=True), ("quirks",)),                                         # quirks, frame 4: the exact 0.5
    "fn overwritten": (Standin(add=False), DATA),                                                    # every case adds to a non-zero fn
    "difficulty ==": (Standin(own_level=True), ("quirks", "sizes", "seventy_frames", "metrics")),    # D > 1
}


@pytest.mark.parametrize("case", sorted(V.CASES))
def test_the_right_standin_passes(case):
    V.CASES[case]("cpu", Standin())


@pytest.mark.parametrize("name,case", [(n, c) for n in sorted(WRONG) for c in WRONG[n][1]])
def test_a_wrong_standin_is_rejected_where_its_edge_is_covered(name, case):
    with pytest.raises(AssertionError):
        V.CASES[case]("cpu", WRONG[name][0])
