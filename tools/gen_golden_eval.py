#!/usr/bin/env python3
"""tests/golden/eval_semseg.npz from the REAL reference's ``filter_valid_label`` and ``SemSegMetric`` on PyTorch-CPU.

The reference's ``ml3d/torch/modules/losses/semseg_loss.py`` and ``ml3d/torch/modules/metrics/semseg_metric.py`` are imported through
``oracle.ref_shim``, as tools/gen_golden_pointrcnn.py imports the reference.  Per setting -- (C = 19, ignored [0]), (C = 13, []),
(C = 8, [0, 5]) and (C = 8, [5, 0]), where the list order shows -- the file holds the inputs (float32 scores, the dataset's label
values), the indices of the points the reference keeps (its filtered scores are the inputs' rows at them, asserted here) and
their filtered labels, the confusion matrix after the first and after a second update, and ``acc()`` / ``iou()``
with their NaN positions (one class of every setting has no points and is never predicted).  The script ASSERTS that the numpy
restatement of tests/eval_ref.py reproduces every array.  It needs the reference checkout, so it runs on the authoring machine only;
the tests read the ``.npz`` file.  Nothing of the reference's text is stored.

    python tools/gen_golden_eval.py            # write the file
    python tools/gen_golden_eval.py --check    # regenerate and compare every array with the committed file
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

from oracle import ref_shim  # noqa: E402
import eval_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "eval_semseg.npz")
SETTINGS = (("c19_ign0", 19, [0]), ("c13_none", 13, []), ("c8_ign05", 8, [0, 5]), ("c8_ign50", 8, [5, 0]))
N = 64


def reference_modules():
    ref_shim.install()
    loss = importlib.import_module("ml3d.torch.modules.losses.semseg_loss")
    metric = importlib.import_module("ml3d.torch.modules.metrics.semseg_metric")
    for m in (loss, metric):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), m.__file__
    return loss.filter_valid_label, metric.SemSegMetric


def inputs(seed, C, ignored):
    """Scores with ties and a NaN row; label values over the whole table [0, C + ignored indices) but for one kept value, whose
    class has no points; that class's score column is the lowest everywhere, so it is never predicted either: NaN in acc AND iou."""
    g = np.random.default_rng(seed)
    n_values = C + len([i for i in ignored if i >= 0])
    scores = (np.round(g.standard_normal((N, C)) * 4) / 4).astype(np.float32)      # a quarter grid: ties occur, and it compresses
    scores[::7] = np.round(scores[::7])                       # more ties: the first maximum
    scores[5, 2] = np.nan
    lut = eval_ref.label_lut(C, ignored)
    empty_value = int(np.nonzero(lut == C - 2)[0][-1])        # a kept value: its class C - 2 gets no points ...
    scores[:, C - 2] = -9.0                                   # ... and no prediction (the NaN row predicts column 2)
    labels = g.integers(0, n_values, size=N)
    labels[labels == empty_value] = int(np.nonzero(lut == 1)[0][0])
    return scores, labels.astype(np.int64)


def generate():
    filter_valid_label, SemSegMetric = reference_modules()
    out = {}
    for s, (name, C, ignored) in enumerate(SETTINGS):
        metric = SemSegMetric()
        for part in range(2):
            scores, labels = inputs(100 + 10 * s + part, C, ignored)
            vs, vl = filter_valid_label(torch.from_numpy(scores), torch.from_numpy(labels), C, ignored, torch.device("cpu"))
            metric.update(vs, vl)
            conf = np.asarray(metric.confusion_matrix).astype(np.int64)
            acc, iou = np.asarray(metric.acc(), np.float64), np.asarray(metric.iou(), np.float64)
            key = "%s_%d_" % (name, part)
            out.update({key + "scores": scores, key + "labels": labels, key + "valid_index": eval_ref.filter_valid(labels, C, ignored)[0].astype(np.int64),
                        key + "valid_labels": vl.numpy().astype(np.int64), key + "confusion": conf, key + "acc": acc, key + "iou": iou})
            assert np.isnan(acc[C - 2]) and np.isnan(iou[C - 2]) and not np.isnan(acc[-1]) and not np.isnan(iou[-1]), (name, acc, iou)
            # the restatement reproduces the reference
            keep, renum = eval_ref.filter_valid(labels, C, ignored)
            assert np.array_equal(renum, out[key + "valid_labels"]) and np.array_equal(scores[keep].view(np.uint32), vs.numpy().view(np.uint32))
            lut = eval_ref.label_lut(C, ignored)
            total = np.zeros((C, C), np.int64)
            for q in range(part + 1):
                c_, counts = eval_ref.confusion_of(eval_ref.first_argmax(out["%s_%d_scores" % (name, q)]), out["%s_%d_labels" % (name, q)], lut, C)
                assert counts[2] == 0 and counts[0] == len(out["%s_%d_valid_labels" % (name, q)])
                total += c_
            assert np.array_equal(total, conf), name
            assert np.array_equal(eval_ref.acc(conf), acc, equal_nan=True) and np.array_equal(eval_ref.iou(conf), iou, equal_nan=True), name
        out[name + "_ignored"] = np.asarray(ignored, np.int64)
        out[name + "_lut"] = eval_ref.label_lut(C, ignored)
    a, b = out["c8_ign05_lut"], out["c8_ign50_lut"]
    assert not np.array_equal(a, b), "the list order must show in the table"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = generate()
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "array names differ"
        for k in out:
            assert old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k], equal_nan=old[k].dtype.kind == "f"), k
        print("check ok: %d arrays" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
