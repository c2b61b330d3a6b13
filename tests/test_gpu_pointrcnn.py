"""GPU: the ``PointRCNN`` class (stage 1) on the MI355X against the goldens of tools/gen_golden_pointrcnn.py (the REAL reference
on PyTorch-CPU) -- the bodies of tests/prcnn_cases.py.  Both cases: state layout, strict load, cls / reg within
max(1e-4, 4.4e-6 scale) on the HIP path AND the torch formulation (``ML3D_PRCNN_OPS=torch``), the rois equal to the restatement of
tests/prcnn_ref.py applied to the product's OWN cls / reg / xyz (order and index exact, boxes within 1e-5).  The small case also
matches the golden's proposals directly.  Every comparison prints its figure before it asserts.

Measured on an MI355X (max |product - golden|): small case cls 6.8e-5, reg 2.5e-5 (hip) / 2.6e-5 (torch), rois 2.1e-5 / 1.9e-5 under
bounds of 1e-4 and 4e-4; KITTI case (scale 41.6, bound 1.83e-4) cls 8.0e-5, reg 3.7e-5 / 3.9e-5; rois against the restatement on the
product's own heads: 0 in every case.  The three tests take 7 s, the KITTI case 3.7 s of them (two forwards of 2 x 16 384 points and
the CPU restatement's NMS over 6300 candidates)."""
import pytest

import prcnn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", C.MODEL_GOLDENS)
def test_model_against_the_reference_golden_on_both_paths(name):
    C.check_model(DEV, name)


def test_rpn_mode_keys_and_the_refusals():
    C.check_model_modes(DEV)
