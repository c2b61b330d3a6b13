"""GPU: ``ops.vote_confusion`` / ``ops.score_confusion`` and ``SemSegMetric`` on the MI355X -- the bodies of tests/eval_cases.py,
compared with numpy for equality."""
import os

import numpy as np
import pytest
import torch

import eval_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_semseg.npz")


@pytest.mark.parametrize("case", sorted(V.CASES))
def test_confusion_case(case):
    V.CASES[case](DEV)


def test_semsegmetric_on_device_tensors_reproduces_the_reference():
    """Device scores and labels go through ``ops.score_confusion`` and stay on the device until the matrix is asked for: the
    reference's matrices, accuracies and IoUs (tests/golden/eval_semseg.npz), both ways of calling it."""
    from ml3d.torch.modules import SemSegMetric
    golden = np.load(GOLDEN)
    for name, classes, ignored in (("c19_ign0", 19, [0]), ("c13_none", 13, []), ("c8_ign05", 8, [0, 5]), ("c8_ign50", 8, [5, 0])):
        filtered, raw = SemSegMetric(), SemSegMetric()
        for part in range(2):
            g = lambda key: golden["%s_%d_%s" % (name, part, key)]
            filtered.update(torch.from_numpy(g("scores")[g("valid_index")]).to(DEV), torch.from_numpy(g("valid_labels")).to(DEV))
            raw.update(torch.from_numpy(g("scores")).to(DEV), torch.from_numpy(g("labels")).to(DEV), ignored_label_inds=ignored)
            for m in (filtered, raw):
                assert m._dev is not None and m._dev.is_cuda, "the matrix must stay on the device until it is asked for"
                assert np.array_equal(m.confusion_matrix, g("confusion")) and m.confusion_matrix.dtype == np.int64
                assert np.array_equal(np.asarray(m.acc(), np.float64), g("acc"), equal_nan=True)
                assert np.array_equal(np.asarray(m.iou(), np.float64), g("iou"), equal_nan=True)
        on_device = SemSegMetric()
        on_device.add_confusion(torch.from_numpy(golden[name + "_0_confusion"]).to(DEV))
        on_device.add_confusion(golden[name + "_1_confusion"] - golden[name + "_0_confusion"])
        assert np.array_equal(on_device.confusion_matrix, golden[name + "_1_confusion"])


def test_semsegmetric_counts_labels_outside_the_table_on_the_device():
    """The device path of ``update`` keeps the op's counts: the same numbers as the host path (tests/test_eval_host.py)."""
    from ml3d.torch.modules import SemSegMetric
    scores = torch.eye(3, dtype=torch.float32)[[0, 1, 2, 2, 1]].to(DEV)
    m = SemSegMetric()
    m.update(scores, torch.tensor([0, 1, 3, -1, 2]).to(DEV))
    assert m.confusion_matrix.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0]]
    with pytest.warns(UserWarning, match="outside the label table"):
        assert m.counts.tolist() == [3, 0, 2]
    m.reset()
    m.update(scores, torch.tensor([1, 2, 0, 0, 3]).to(DEV), ignored_label_inds=[0])
    assert m.counts.tolist() == [3, 2, 0] and m.confusion_matrix.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0]]
