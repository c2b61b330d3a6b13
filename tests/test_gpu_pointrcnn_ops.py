"""GPU: both kernels families of csrc/pointrcnn.hip on the MI355X -- the bodies of tests/prcnn_cases.py (shared with
tests/test_emulated_pointrcnn_ops.py, which runs them on the host emulator).  ``ml3d_bin_decode`` at every flag combination, both
roi widths and both bin sets against the float64 formula on the CPU within max(1e-5, 4 e32), with exact ties in every argmax and
rows on both sides of the ``ry > pi`` wrap; ``ml3d_rpn_proposals`` for EQUALITY (order, indices, box bits) with the numpy
restatement of tests/prcnn_ref.py, its scratch filled with NaN bytes and its outputs pre-filled with a sentinel.  Every decode
case prints its measured figures before it asserts."""
import pytest

import prcnn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("bins", C.DECODE_BINS, ids=["H%d" % b[2] for b in C.DECODE_BINS])
@pytest.mark.parametrize("n", C.DECODE_N)
def test_decode_all_flags_and_widths_against_float64(n, bins):
    C.check_decode(DEV, n, bins)


def test_decode_refuses_a_wrong_channel_count():
    C.check_decode_refusals(DEV)


@pytest.mark.parametrize("pre,post", C.PROP_PRE_POST)
@pytest.mark.parametrize("n", C.PROP_N)
def test_proposals_equal_the_restatement(n, pre, post):
    C.check_proposals(DEV, n, pre, post)


@pytest.mark.parametrize("pre,post", ((10, 4), (9000, 100)))
@pytest.mark.parametrize("kind", C.PROP_KINDS)
@pytest.mark.parametrize("n", (65, 700))
def test_proposals_zone_and_suppression_arms(n, kind, pre, post):
    C.check_proposals(DEV, n, pre, post, kind, batches=(3,))


def test_proposals_refusals():
    C.check_proposal_refusals(DEV)
