"""GPU: ``ml3d_roi_pool`` of csrc/pointrcnn.hip on the MI355X -- the bodies of tests/prcnn2_cases.py (shared with
tests/test_emulated_pointrcnn2_ops.py, which runs them on the host emulator).  Per point count 20 cases over every num_points
{1, 8, 64, 512} x every hit-count arm {0, 1, S - 1, S, > S} with the batch sizes, roi counts and feature widths dealt round:
``pool_idx`` / ``empty`` for EQUALITY with the numpy restatement of tests/prcnn2_ref.py, the five leading columns against the
float64 formula within max(1e-5, 4 e32), the feature columns bit for bit; outputs pre-filled with a sentinel, a strided ``feat``,
an item pooled alone, NaN behind the last hit that counts.  Every case prints its measured figures before it asserts."""
import pytest

import prcnn2_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", C.POOL_N)
def test_roi_pool_equals_the_restatement(n):
    C.check_pool(DEV, n)


def test_roi_pool_refusals():
    C.check_pool_refusals(DEV)
