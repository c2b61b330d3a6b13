"""GPU: the device finish of the multi-cloud loops and of the single-cloud loops on the MI355X -- the bodies of
tests/test_emulated_multicloud_finish.py (tests/finish_cases.py) on the same clouds, KPFCNN at its full widths.  Equality everywhere:
``inference_many(finish="device")`` against ``finish="host"`` on the same model, clouds and seeds."""
import numpy as np
import pytest

import finish_cases as F
import kpconv_multicloud_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("in_flight", [1, 2])
def test_randlanet_device_finish_equals_host_finish(in_flight):
    """4 clouds, max_in_flight 1 and 2: a cloud retires while another is active, and every admission rebuilds the buffers while
    the retire's copies may still be on their way."""
    make, clouds, seeds = F.randla_setup(DEV)
    F.check_finish_device_equals_host(make(), clouds, seeds, in_flight)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_kpfcnn_device_finish_equals_host_finish(in_flight):
    make, clouds, seeds = F.kpconv_setup(DEV, K.MODEL_CFG)
    F.check_finish_device_equals_host(make(), clouds, seeds, in_flight)


def test_single_cloud_loops_finish_like_the_host_formula():
    make, clouds, seeds = F.randla_setup(DEV)
    F.check_single_cloud_finish(make(seed=seeds[2]), clouds[2])
    make, clouds, seeds = F.kpconv_setup(DEV, K.MODEL_CFG)
    state = np.random.get_state()
    try:
        np.random.seed(seeds[2])
        F.check_single_cloud_finish(make(), clouds[2])
    finally:
        np.random.set_state(state)


def test_a_bad_finish_value_raises_and_a_state_without_device_indices_uploads_them():
    make, clouds, seeds = F.randla_setup(DEV)
    F.check_bad_finish(make(), clouds, seeds)
    make, clouds, seeds = F.kpconv_setup(DEV, K.MODEL_CFG)
    F.check_bad_finish(make(), clouds, seeds)
    F.check_pickled_tree_takes_one_upload(DEV)
