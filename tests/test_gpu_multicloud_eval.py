"""GPU: ``inference_many(evaluate=True)`` of RandLA-Net and KPFCNN on the MI355X -- the bodies of
tests/test_emulated_multicloud_eval.py (tests/eval_cases.py) on the same clouds, KPFCNN at its full widths.  Equality everywhere."""
import pytest

import eval_cases as V
import finish_cases as F
import kpconv_multicloud_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("finish", ["device", "host"])
def test_randlanet_evaluate(finish):
    make, clouds, seeds = F.randla_setup(DEV)
    V.check_model_evaluate(make(), clouds, seeds, finish)


@pytest.mark.parametrize("finish", ["device", "host"])
def test_kpfcnn_evaluate(finish):
    make, clouds, seeds = F.kpconv_setup(DEV, K.MODEL_CFG)
    V.check_model_evaluate(make(), clouds, seeds, finish)


def test_a_label_of_the_wrong_length_raises_before_any_patch_runs():
    make, clouds, seeds = F.randla_setup(DEV)
    V.check_wrong_length_label(make(), clouds, seeds)
    make, clouds, seeds = F.kpconv_setup(DEV, K.MODEL_CFG)
    V.check_wrong_length_label(make(), clouds, seeds)
