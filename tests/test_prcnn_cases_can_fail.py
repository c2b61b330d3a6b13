"""CPU, no kernel involved: the decode and proposal bodies of tests/prcnn_cases.py CAN fail.  Each body runs against a stand-in
written in numpy (float64 for the decode): the CORRECT stand-in passes every body (so the bodies judge what they are given, nothing
else), and each deliberately wrong one is rejected by every case that covers its edge --

* the LAST maximal bin wins a tie instead of the first              (every decode case: rows 0, 3, 6, ... tie in every argmax),
* the z residual is taken from the x block                          (every decode case: half of its flag sets have residuals),
* the ``ry > pi`` wrap is omitted                                   (every decode case: row 0 lies past the wrap),
* the far zone's fallback starts at the near zone's row 0           (the "far_empty" cases with more near rows than pre_near),
* the zone test is ``z >= 0``                                       (the "both" cases with a near quota: a top-scored box AT z = 0),
* the post-NMS cut is applied before the NMS                        (the "both" cases where a suppressed candidate sits in front),
* the padding is not written                                        (the cases with fewer survivors than nms_post)."""
import numpy as np
import pytest
import torch

import prcnn_cases as C
import prcnn_ref


class StandIn:
    def __init__(self, *wrong):
        self.wrong = wrong

    def bin_decode(self, roi, pred_reg, anchor_size, loc_scope, loc_bin_size, num_head_bin, get_xz_fine=True, get_y_by_bin=False,
                   loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False):
        out = prcnn_ref.decode(roi.numpy(), pred_reg.numpy(), anchor_size, loc_scope, loc_bin_size, num_head_bin, get_xz_fine, get_y_by_bin,
                               loc_y_scope, loc_y_bin_size, get_ry_fine, dtype=np.float64, wrong=self.wrong)
        return torch.from_numpy(out.astype(np.float32))

    def rpn_proposals(self, scores, boxes, nms_pre, nms_post, nms_thres, out=None):
        res = prcnn_ref.proposals(scores.numpy(), boxes.numpy(), nms_pre, nms_post, nms_thres, wrong=self.wrong,
                                  out=None if out is None else [o.numpy() for o in out])
        return tuple(torch.from_numpy(r) for r in res)


DECODE = [(n, bins) for n in C.DECODE_N for bins in C.DECODE_BINS]
DECODE_IDS = ["n%d-H%d" % (n, bins[2]) for n, bins in DECODE]


def test_the_correct_stand_in_passes_every_body():
    for n, bins in DECODE:
        C.check_decode("cpu", n, bins, StandIn(), report=lambda **kv: None)
    for n in (1, 64, 65, 700):
        for pre, post in C.PROP_PRE_POST:
            C.check_proposals("cpu", n, pre, post, "both", impl=StandIn())
    for kind in C.PROP_KINDS:
        for pre, post in ((10, 4), (9000, 100)):
            C.check_proposals("cpu", 65, pre, post, kind, batches=(3,), impl=StandIn())
            C.check_proposals("cpu", 700, pre, post, kind, batches=(3,), impl=StandIn())


@pytest.mark.parametrize("wrong", prcnn_ref.WRONG_DECODE)
@pytest.mark.parametrize("n,bins", DECODE, ids=DECODE_IDS)
def test_a_wrong_decode_is_rejected_by_every_decode_case(n, bins, wrong):
    with pytest.raises(AssertionError):
        C.check_decode("cpu", n, bins, StandIn(wrong), report=lambda **kv: None)


@pytest.mark.parametrize("n,pre,post", [(65, 10, 4), (700, 10, 4), (700, 3, 1), (5000, 9000, 100)])
def test_a_fallback_from_row_0_is_rejected(n, pre, post):
    with pytest.raises(AssertionError):
        C.check_proposals("cpu", n, pre, post, "far_empty", batches=(3,), impl=StandIn("fallback_from_0"))


@pytest.mark.parametrize("n", [64, 65, 700])
@pytest.mark.parametrize("pre,post", [(10, 4), (9000, 100)])
def test_a_zone_that_starts_at_zero_inclusive_is_rejected(n, pre, post):
    with pytest.raises(AssertionError):
        C.check_proposals("cpu", n, pre, post, "both", impl=StandIn("zone_ge_0"))


@pytest.mark.parametrize("n,pre,post", [(700, 9000, 100), (5000, 9000, 100)])
def test_a_cut_before_the_nms_is_rejected(n, pre, post):
    with pytest.raises(AssertionError):
        C.check_proposals("cpu", n, pre, post, "both", batches=(1,), impl=StandIn("cut_before_nms"))


@pytest.mark.parametrize("kind", ["all_suppressed", "both_empty", "near_empty"])
@pytest.mark.parametrize("n,pre,post", [(65, 10, 4), (700, 9000, 100)])
def test_unwritten_padding_is_rejected(n, pre, post, kind):
    with pytest.raises(AssertionError):
        C.check_proposals("cpu", n, pre, post, kind, batches=(3,), impl=StandIn("no_padding"))
