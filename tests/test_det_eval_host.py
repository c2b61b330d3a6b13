"""CPU, no emulator: tests/det_ref.py -- the numpy restatement the ``det_match`` cases are compared with -- reproduces the REAL
reference on tests/golden/eval_objdet.npz (written by tools/gen_golden_det_eval.py): every frame's ``detection`` rows and ``fns``,
the ``gt`` counts and every mAP array as float64, from the golden's IoU matrices.  Also the host halves of ``ml3d.metrics`` that need
no device: ``filter_data``, ``sample_thresholds``, the label / difficulty encoding and the host matcher."""
import importlib
import os

import numpy as np
import pytest

import det_cases as V
import det_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_objdet.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("setting", V.GOLDEN_SETTINGS, ids=[s[0] for s in V.GOLDEN_SETTINGS])
def test_det_ref_reproduces_the_reference(golden, setting):
    name, classes, difficulties, min_overlap, similar = setting
    preds, targets = V.golden_frames(golden, name)
    mo = list(min_overlap) * (len(classes) if len(min_overlap) == 1 else 1)
    assert np.array_equal(R.gt_counts(targets, classes, difficulties), golden[name + "_gt"])
    for tag in ("bev", "3d"):
        ious = [golden["%s_%d_iou_%s" % (name, f, tag)] for f in range(V.GOLDEN_FRAMES)]
        for f in range(V.GOLDEN_FRAMES):
            det, fns = R.precision_3d(preds[f], targets[f], ious[f], classes, difficulties, mo, similar)
            k = "%s_%d_%s_" % (name, f, tag)
            assert det.shape == golden[k + "detection"].shape and R.rows_of(det) == R.rows_of(golden[k + "detection"]), k
            assert np.array_equal(fns, golden[k + "fns"]), k
        for samples in (41, 11, 0):
            want = golden["%s_mAP_%s_%d" % (name, tag, samples)]
            got = R.mAP(preds, targets, ious, classes, difficulties, min_overlap, samples, similar)
            assert got.dtype == np.float64 and np.array_equal(got, want), (name, tag, samples)
            assert samples > 0 or not want.any()
        assert golden["%s_mAP_%s_41" % (name, tag)].any()


def test_the_golden_holds_what_it_is_there_for(golden):
    empty = lambda k: len(golden[k]) == 0
    assert empty("kitti_0_pred_label") and not empty("kitti_0_tgt_label")           # a frame without predictions
    assert not empty("kitti_1_pred_label") and empty("kitti_1_tgt_label")           # ... without targets
    assert empty("kitti_2_pred_label") and empty("kitti_2_tgt_label")               # ... with neither
    assert "Tram" in golden["kitti_3_pred_label"] and -1 in golden["kitti_3_pred_difficulty"] and -1 in golden["kitti_3_tgt_difficulty"]
    assert "kitti_6_pred_difficulty" not in golden.files                             # predictions without `difficulty`
    box = golden["kitti_3_pred_bbox"]
    assert np.array_equal(box[0], box[1]) and golden["kitti_3_pred_score"][0] == golden["kitti_3_pred_score"][1]       # twins, equal scores
    # the KITTI dict is inert, the dict keyed by a class is not: Van targets are columns of Car only in `similar`
    a, b = golden["kitti_3_bev_detection"], golden["similar_3_bev_detection"]
    assert R.rows_of(a) != R.rows_of(b)


def test_host_halves_of_the_product_agree_with_det_ref(golden):
    """``filter_data`` / ``sample_thresholds`` / the id encoding / ``match_frame`` of ml3d.metrics.mAP, without any device."""
    M = importlib.import_module("ml3d.metrics.mAP")
    name, classes, difficulties, min_overlap, similar = V.GOLDEN_SETTINGS[2]
    preds, targets = V.golden_frames(golden, name)
    mo = list(min_overlap) * len(classes)
    S = M._Split(preds, targets, classes, difficulties, mo, similar)
    assert np.array_equal(S.gt_cnt, golden[name + "_gt"]) and S.similar.tolist() == [-1, -1, 3] and S.finite
    names, _ = R.vocabulary(classes, similar)
    for f in range(V.GOLDEN_FRAMES):
        kept, flags, fn, pc, pm = R.frame_flags(preds[f], targets[f], golden["%s_%d_iou_bev" % (name, f)], classes, difficulties, mo, similar)
        ps, ts = slice(S.pred.start[f], S.pred.start[f + 1]), slice(S.tgt.start[f], S.tgt.start[f + 1])
        assert np.array_equal(S.pred.ids[ps], pc) and np.array_equal(S.pred.dmask[ps], pm)
        tl, tm = R.ids_and_masks(targets[f], names, difficulties)
        assert np.array_equal(S.tgt.ids[ts], tl[tl >= 0]) and np.array_equal(S.tgt.dmask[ts], tm[tl >= 0])
        iou = golden["%s_%d_iou_bev" % (name, f)].reshape(len(preds[f]["label"]), len(targets[f]["label"]))[kept][:, tl >= 0]
        got_flags, got_fn = M.match_frame(iou, S.pred.ids[ps], S.pred.dmask[ps], S.tgt.ids[ts], S.tgt.dmask[ts], S.min_overlap, S.similar, S.D)
        assert np.array_equal(got_flags, flags) and np.array_equal(got_fn, fn), f
        sub, idx = M.filter_data(preds[f], classes, difficulties)
        assert np.array_equal(idx, [i for i in kept if "difficulty" not in preds[f] or 0 <= preds[f]["difficulty"][i] <= 2])
        assert sorted(sub) == sorted(preds[f]) and len(sub["bbox"]) == len(idx)
    g = np.random.default_rng(3)
    for n, gt, samples in ((0, 5.0, 41), (1, 1.0, 41), (7, 9.0, 41), (30, 31.0, 11), (60, 60.0, 41), (12, 40.0, 5)):
        scores = np.round(g.uniform(size=n), 2)
        assert M.sample_thresholds(scores, np.float64(gt), samples) == R.thresholds_of(scores, np.float64(gt), samples)
