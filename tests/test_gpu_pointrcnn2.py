"""GPU: PointRCNN stage 2 on the MI355X -- the model bodies of tests/prcnn2_cases.py (shared with tests/test_emulated_pointrcnn2.py)
against tests/golden/pointrcnn_rcnn_small.npz (the REAL reference's ``RCNN.forward`` on PyTorch-CPU), and the KITTI yaml
configuration at B = 2, N = 16384: the HIP network against the torch formulation on the same rows, the pooling against float64
properties that need no margin.  Every float comparison prints its measured figures before it asserts."""
import pytest

import prcnn2_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_pooling_equals_the_golden_on_its_rois_and_the_restatement_on_the_models_own():
    C.check_model_pooling(DEV)


def test_network_on_the_goldens_rows_on_both_paths():
    C.check_model_network(DEV)


def test_rcnn_forward_is_its_two_halves_and_chunks_do_not_change_a_bit():
    C.check_model_plumbing(DEV)


def test_inference_end_reproduces_the_goldens_detections():
    C.check_model_inference_end(DEV)


def test_forward_still_refuses_and_names_the_new_method():
    C.check_model_refusals(DEV)


def test_yaml_configuration_runs_and_pools_what_float64_allows():
    C.check_yaml_configuration(DEV)
