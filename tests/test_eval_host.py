"""CPU, no GPU: ground-truth scoring on the host.  The numpy restatement of tests/eval_ref.py is pinned to
tests/golden/eval_semseg.npz, which tools/gen_golden_eval.py wrote from the REAL reference's ``filter_valid_label`` and
``SemSegMetric``; the product's host pieces (``ops.label_lut``, ``SemSegMetric`` on host inputs, ``metrics.host_confusion``) are
pinned to the same file; and every invalid argument of the two C entries is refused before any HIP call (the hipcc-built library)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import eval_ref as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_semseg.npz")
SETTINGS = (("c19_ign0", 19, [0]), ("c13_none", 13, []), ("c8_ign05", 8, [0, 5]), ("c8_ign50", 8, [5, 0]))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,classes,ignored", SETTINGS)
def test_the_restatement_reproduces_the_reference(golden, name, classes, ignored):
    assert golden[name + "_ignored"].tolist() == ignored
    lut = E.label_lut(classes, ignored)
    assert np.array_equal(lut, golden[name + "_lut"])
    total = np.zeros((classes, classes), np.int64)
    for part in range(2):
        g = lambda key: golden["%s_%d_%s" % (name, part, key)]
        keep, renumbered = E.filter_valid(g("labels"), classes, ignored)
        assert np.array_equal(keep, g("valid_index")) and np.array_equal(renumbered, g("valid_labels"))
        # the table says what the filter says: -1 exactly at the dropped points, the renumbered label elsewhere
        rows = lut[g("labels")]
        assert np.array_equal(np.nonzero(rows >= 0)[0], keep) and np.array_equal(rows[keep], renumbered)
        pred = E.first_argmax(g("scores"))
        conf, counts = E.confusion_of(pred, g("labels"), lut, classes)
        fast = E.confusion_fast(pred, g("labels"), lut, classes)
        assert np.array_equal(conf, fast[0]) and np.array_equal(counts, fast[1])
        assert counts.tolist() == [len(keep), len(pred) - len(keep), 0]
        total += conf
        assert np.array_equal(total, g("confusion"))
        assert np.array_equal(E.acc(total), g("acc"), equal_nan=True) and np.array_equal(E.iou(total), g("iou"), equal_nan=True)
        assert np.isnan(g("acc")).any() and np.isnan(g("iou")).any()


def test_the_list_order_of_the_ignored_indices_matters(golden):
    assert not np.array_equal(golden["c8_ign05_lut"], golden["c8_ign50_lut"])
    assert not np.array_equal(golden["c8_ign05_0_confusion"], golden["c8_ign50_0_confusion"]) or \
        not np.array_equal(golden["c8_ign05_0_labels"], golden["c8_ign50_0_labels"])


@pytest.mark.parametrize("name,classes,ignored", SETTINGS)
def test_label_lut_and_host_confusion_of_the_product(golden, name, classes, ignored):
    from ml3d import ops
    from ml3d.torch.modules.metrics import host_confusion
    lut = ops.label_lut(classes, ignored)
    assert lut.dtype == np.int32 and np.array_equal(lut, golden[name + "_lut"])
    labels = golden[name + "_0_labels"].copy()
    labels[3], labels[4] = -1, len(lut)                      # outside the table: counted, nothing else
    pred = E.first_argmax(golden[name + "_0_scores"])
    want = E.confusion_of(pred, labels, lut, classes)
    got = host_confusion(pred, labels, lut, classes)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[1][2] == 2


@pytest.mark.parametrize("name,classes,ignored", SETTINGS)
def test_semsegmetric_on_host_inputs(golden, name, classes, ignored):
    from ml3d.torch.modules import SemSegMetric
    filtered, raw = SemSegMetric(), SemSegMetric()
    assert filtered.confusion_matrix is None and filtered.acc() is None and filtered.iou() is None and filtered.num_classes is None
    for part in range(2):
        g = lambda key: golden["%s_%d_%s" % (name, part, key)]
        # the reference's call: scores and labels after filter_valid_label, as torch tensors ...
        filtered.update(torch.from_numpy(g("scores")[g("valid_index")]), torch.from_numpy(g("valid_labels")))
        # ... and the dataset's values with the ignored list, as numpy arrays
        raw.update(g("scores"), g("labels"), ignored_label_inds=ignored)
        for m in (filtered, raw):
            assert m.num_classes == classes and m.confusion_matrix.dtype == np.int64
            assert np.array_equal(m.confusion_matrix, g("confusion"))
            assert np.array_equal(np.asarray(m.acc(), np.float64), g("acc"), equal_nan=True)
            assert np.array_equal(np.asarray(m.iou(), np.float64), g("iou"), equal_nan=True)
            assert len(m.acc()) == classes + 1 and len(m.iou()) == classes + 1
    summed = SemSegMetric()
    summed.add_confusion(golden[name + "_0_confusion"])
    summed.add_confusion(torch.from_numpy(golden[name + "_1_confusion"] - golden[name + "_0_confusion"]))
    assert np.array_equal(summed.confusion_matrix, golden[name + "_1_confusion"])
    summed.reset()
    assert summed.confusion_matrix is None and summed.iou() is None
    summed.update(np.zeros((4, 3), np.float32), np.array([0, 1, 2, 2]))
    assert summed.num_classes == 3 and summed.confusion_matrix.tolist() == [[1, 0, 0], [1, 0, 0], [2, 0, 0]]


def test_device_ops_refuse_cpu_tensors():
    from ml3d import ops
    v, p, gt = torch.zeros((8, 19), dtype=torch.float16), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    for f in (lambda: ops.vote_confusion(v, p, gt), lambda: ops.score_confusion(torch.zeros((5, 19)), gt)):
        with pytest.raises(RuntimeError):
            f()


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call (the hipcc-built library, no GPU)."""
    import __graft_entry__ as ge
    from ml3d import _abi
    ge.build()
    L = _abi.get()
    INVALID = -1
    p = C.c_void_p(256)                      # a non-null "device pointer": never followed, every call below returns before a launch

    def vote(votes=p, n_sub=100, classes=19, proj=p, n_full=10, gt=p, lut=p, lut_size=20, conf=p, counts=p, labels=p):
        return L.ml3d_vote_confusion(votes, n_sub, classes, proj, n_full, gt, lut, lut_size, conf, counts, labels, None)
    assert vote(n_full=0) == 0 and vote(n_full=0, n_sub=0) == 0 and vote(n_full=0, n_sub=0, proj=None) == 0      # nothing to do: no launch
    assert vote(votes=None) == INVALID and vote(gt=None) == INVALID and vote(conf=None) == INVALID and vote(counts=None) == INVALID
    assert vote(classes=0) == INVALID and vote(classes=257) == INVALID and vote(classes=-1) == INVALID
    assert vote(classes=257, n_full=0) == INVALID
    assert vote(n_sub=0) == INVALID and vote(n_sub=-1) == INVALID and vote(n_full=-1) == INVALID
    assert vote(n_full=1 << 31) == INVALID and vote(n_sub=1 << 31) == INVALID and vote(n_sub=1 << 40, n_full=1 << 40) == INVALID
    assert vote(proj=None, n_sub=100, n_full=10) == INVALID            # the identity needs n_full == n_sub
    assert vote(proj=None, n_sub=0, n_full=5) == INVALID
    assert vote(lut_size=0) == INVALID and vote(lut_size=-4) == INVALID

    def score(scores=p, ld=19, n=10, classes=19, gt=p, lut=p, lut_size=20, conf=p, counts=p):
        return L.ml3d_score_confusion(scores, ld, n, classes, gt, lut, lut_size, conf, counts, None)
    assert score(n=0) == 0
    assert score(scores=None) == INVALID and score(gt=None) == INVALID and score(conf=None) == INVALID and score(counts=None) == INVALID
    assert score(classes=0) == INVALID and score(classes=257, ld=300) == INVALID and score(ld=18) == INVALID
    assert score(n=-1) == INVALID and score(n=1 << 31) == INVALID and score(n=1 << 40) == INVALID
    assert score(lut_size=0) == INVALID


def test_semsegmetric_counts_labels_outside_the_table_and_does_not_score_them():
    """One contract on both paths of ``update`` (the device path: tests/test_gpu_eval.py): a label outside the table is counted."""
    import warnings
    from ml3d.torch.modules import SemSegMetric
    m = SemSegMetric()
    scores = np.eye(3, dtype=np.float32)[[0, 1, 2, 2, 1]]
    m.update(scores, np.array([0, 1, 3, -1, 2]))                          # identity table over 3 classes: 3 and -1 lie outside
    assert m.confusion_matrix.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0]]
    with pytest.warns(UserWarning, match="outside the label table"):
        assert m.counts.tolist() == [3, 0, 2]
    m.reset()
    m.update(scores, np.array([1, 2, 0, 0, 3]), ignored_label_inds=[0])    # table [-1, 0, 1, 2]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert m.counts.tolist() == [3, 2, 0]
    assert m.confusion_matrix.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0]]
