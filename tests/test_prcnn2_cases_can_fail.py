"""CPU, no kernel involved: the pooling bodies of tests/prcnn2_cases.py CAN fail.  Each body runs against a stand-in written in
numpy float64 (tests/prcnn2_ref.py): the CORRECT stand-in passes every case (so the bodies judge what they are given, nothing
else), and each deliberately wrong one is rejected by EVERY case that covers its edge --

* the four vertical faces are open                                  (cases with a non-empty roi at ry = 0: points ON its faces),
* slots behind the last hit are filled with point 0, not wrapped    (cases with a roi holding 0 < cnt < S hits, not all of them point 0),
* ``cy = y + h / 2``                                                (cases with a non-empty roi),
* the canonical rotation's sign is flipped                          (cases with a roi whose heading is not 0),
* the canonical transform is taken on the enlarged box              (every case),
* the 10 m prefilter is dropped                                     (cases with the 26 m roi and a decoy in front of its S-th hit),
* an empty roi is not flagged / gets -0.5 in the depth column       (cases with an empty roi)."""
import numpy as np
import pytest
import torch

import prcnn2_cases as C
import prcnn2_ref


class StandIn:
    def __init__(self, *wrong):
        self.wrong = wrong

    def roi_pool(self, xyz, feat, scores, rois, num_points=512, score_thres=0.3, extra_width=1.0, out=None):
        r = prcnn2_ref.roi_pool(xyz.numpy(), feat.numpy(), scores.numpy(), rois.numpy(), num_points, score_thres, extra_width,
                                np.float64, wrong=self.wrong)
        return torch.from_numpy(r[0].astype(np.float32)), torch.from_numpy(r[1]), torch.from_numpy(r[2])


def _covers(wrong, n, case):
    b, m, s, c, arm = case
    I = C.pool_inputs(b, n, m, s, c, arm)
    _, idx, _, count = prcnn2_ref.roi_pool(I["xyz"], I["feat"], I["scores"], I["rois"], s, C.SCORE_THRES, C.EXTRA_WIDTH, np.float64)
    ry = I["rois"][..., 6]
    if wrong == "open_faces":
        return bool(((ry == 0) & (count > 0)).any())
    if wrong == "zero_fill":
        return bool(((count > 0) & (count < s) & (idx[..., -1] != 0)).any())
    if wrong == "cy_plus":
        return bool((count > 0).any())
    if wrong == "rot_sign":
        return bool((ry != 0).any())
    if wrong == "transform_enlarged":
        return True
    if wrong == "no_prefilter":                                  # a decoy in front of the long roi's last slot that counts
        if m != 3 or n < 8:
            return False
        big = prcnn2_ref.enlarge(I["rois"], C.EXTRA_WIDTH)[0, 1]
        cut = prcnn2_ref.in_box(I["xyz"][0], big, wrong=("no_prefilter",)) & ~prcnn2_ref.in_box(I["xyz"][0], big)
        return bool(count[0, 1] < s or np.flatnonzero(cut)[0] < idx[0, 1, -1])
    return bool((count == 0).any())                              # empty_unflagged, empty_depth


@pytest.mark.parametrize("n", C.POOL_N)
def test_the_correct_stand_in_passes_every_case(n):
    C.check_pool("cpu", n, StandIn(), report=lambda **kv: None)


@pytest.mark.parametrize("wrong", prcnn2_ref.WRONG_POOL)
@pytest.mark.parametrize("n", C.POOL_N)
def test_a_wrong_pooling_is_rejected_by_every_case_that_covers_it(n, wrong):
    covered = [case for case in C.pool_cases(n) if _covers(wrong, n, case)]
    assert len(covered) >= (5 if n >= 63 else 0), (wrong, n, len(covered))
    for case in covered:
        with pytest.raises(AssertionError):
            C.check_pool_case("cpu", n, case, StandIn(wrong), report=lambda **kv: None)
