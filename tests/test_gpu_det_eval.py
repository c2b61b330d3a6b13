"""GPU: ``ops.det_match`` and ``ml3d.metrics`` on the MI355X -- the bodies of tests/det_cases.py: flags, ``fn`` and AP equal to
tests/det_ref.py on the oracle's IoUs, ``pair_iou`` bit-equal to ``ops.iou_bev`` / ``ops.iou_3d`` and within 1e-5 of the oracle."""
import pytest

import det_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", sorted(V.CASES))
def test_det_match_case(case):
    V.CASES[case](DEV)


@pytest.mark.parametrize("route", ["device", "host"])
def test_map_and_objdetmetric_reproduce_the_reference(route):
    """``mAP`` / ``precision_3d`` / ``ObjdetMetric`` on the frames of tests/golden/eval_objdet.npz: the reference's arrays, through
    ``det_match`` and with ``ML3D_DET_EVAL=host``."""
    V.check_golden_model(DEV, route)
