#!/usr/bin/env python3
"""tests/golden/eval_objdet.npz from the REAL reference's ``precision_3d`` and ``mAP`` (ml3d/metrics/mAP.py).

The reference's module is imported through ``oracle.ref_shim``, as tools/gen_golden_eval.py imports the reference, with its
``iou_bev`` / ``iou_3d`` bound to ``oracle.ops.iou_bev`` / ``iou_3d``.  Three settings --

* ``one``      1 class, difficulties [0], overlap [0.7], no similar classes;
* ``kitti``    3 classes, [0, 1, 2], [0.5, 0.5, 0.7], the KITTI YAML's dict ({Van: Car, Person_sitting: Pedestrian}), which is INERT:
               the reference reads the dict with the class as key;
* ``similar``  3 classes, [0, 1, 2], one overlap broadcast, a dict keyed BY a class ({Car: Van}), so that similar targets exist

-- of 8 frames of at most 12 boxes a side.  Together the frames hold: a frame without predictions, one without targets, one with
neither, predictions of a class outside ``classes``, difficulty -1 on both sides, a prediction that overlaps only a similar-class
target, one that overlaps only a harder target, two bit-identical predictions on one target, a target no prediction reaches, a
class whose columns are all zero, equal scores, a frame whose predictions carry no ``difficulty``; ``samples`` in {41, 11, 0};
(class, difficulty) pairs with fewer thresholds than ``samples / 4 + 1`` and with more.

The file stores the inputs, the oracle's IoU matrices (over each frame's unfiltered boxes), each frame's ``detection`` and ``fns``,
the ``gt`` counts and the mAP arrays.  The script ASSERTS, trying seeds until both hold,
(1) that tests/det_ref.py reproduces every array (flags and fns equal, mAP equal as float64), and
(2) that the inputs are decisive: every related pair's IoU, both metrics, is exactly 0 or >= 1e-3; every non-zero IoU is >= 1e-3
    away from its class's overlap; in every column the two largest IoUs differ by >= 1e-3 unless they come from bit-identical
    boxes (or the column is all zero, where the election of the first row is the point).  1e-3 = 100 x the 1e-5 that
    tests/test_gpu_api.py allows between the device's IoU and the oracle's.
It needs the reference checkout, so it runs on the authoring machine only; the tests read the ``.npz`` file.  Nothing of the
reference's text is stored.

    python tools/gen_golden_det_eval.py            # write the file
    python tools/gen_golden_det_eval.py --check    # regenerate and compare every array with the committed file
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

from oracle import ops as oops  # noqa: E402
from oracle import ref_shim  # noqa: E402
import det_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "eval_objdet.npz")
MARGIN = 1e-3
THREE = ["Pedestrian", "Cyclist", "Car"]
SETTINGS = (
    ("one", ["Car"], [0], [0.7], {}),
    ("kitti", THREE, [0, 1, 2], [0.5, 0.5, 0.7], {"Van": "Car", "Person_sitting": "Pedestrian"}),
    ("similar", THREE, [0, 1, 2], [0.5], {"Car": "Van"}),
)
SAMPLES = (41, 11, 0)
SIZE = {"Car": (1.6, 1.5, 3.9), "Van": (1.9, 2.0, 5.0), "Pedestrian": (0.6, 1.7, 0.8), "Cyclist": (0.6, 1.7, 1.8),
        "Tram": (2.5, 3.5, 12.0), "DontCare": (1.0, 1.0, 1.0), "Person_sitting": (0.6, 1.2, 0.8)}


def reference_module():
    ref_shim.install()
    m = importlib.import_module("ml3d.metrics.mAP")
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), m.__file__
    assert m.iou_bev is oops.iou_bev and m.iou_3d is oops.iou_3d
    return m


def box(g, name, slot):
    """A box of ``name``'s size at grid slot ``slot`` (slots are 20 m apart: boxes of different slots never touch)."""
    w, h, l = SIZE[name]
    return [20.0 * (slot % 4) + g.uniform(-1, 1), 1.6 + g.uniform(-0.1, 0.1), 20.0 * (slot // 4) + 10 + g.uniform(-1, 1),
            w * g.uniform(0.9, 1.1), h * g.uniform(0.9, 1.1), l * g.uniform(0.9, 1.1), g.uniform(-np.pi, np.pi)]


def near(g, b, amount):
    """``b`` moved, turned and scaled by up to ``amount`` (0: a bit-identical copy)."""
    b = list(b)
    b[0] += amount * g.uniform(-1, 1)
    b[2] += amount * g.uniform(-1, 1)
    b[1] += 0.2 * amount * g.uniform(-1, 1)
    b[6] += 0.3 * amount * g.uniform(-1, 1)
    for k in (3, 4, 5):
        b[k] *= 1 + 0.15 * amount * g.uniform(-1, 1)
    return b


def as_dicts(preds, targets, pred_difficulty=True):
    """lists of (box, label, score, difficulty) / (box, label, difficulty) -> the two dicts of numpy arrays."""
    p = {"bbox": np.array([b for b, _, _, _ in preds], np.float32).reshape(-1, 7), "label": np.array([n for _, n, _, _ in preds], dtype="<U16"),
         "score": np.array([s for _, _, s, _ in preds], np.float32)}
    if pred_difficulty:
        p["difficulty"] = np.array([d for _, _, _, d in preds], np.int64)
    t = {"bbox": np.array([b for b, _, _ in targets], np.float32).reshape(-1, 7), "label": np.array([n for _, n, _ in targets], dtype="<U16"),
         "difficulty": np.array([d for _, _, d in targets], np.int64)}
    return p, t


def frames(seed, classes):
    g = np.random.default_rng(seed)
    sc = lambda: float(np.round(g.uniform(0.05, 0.99), 2))          # two decimals: equal scores occur
    main = classes[-1]                                               # Car
    out = []
    # 0: no predictions   1: no targets   2: neither
    out.append(as_dicts([], [(box(g, main, 0), main, 0), (box(g, main, 1), main, 1), (box(g, "Van", 2), "Van", 0)]))
    out.append(as_dicts([(box(g, main, 0), main, sc(), 0), (box(g, main, 1), main, sc(), 1), (box(g, "Tram", 2), "Tram", sc(), 0)], []))
    out.append(as_dicts([], []))
    # 3: the special boxes
    T, P = [], []
    t0 = box(g, main, 0); T.append((t0, main, 0))                    # two bit-identical predictions on one target, equal scores
    twin = near(g, t0, 0.3); P += [(twin, main, 0.77, 0), (list(twin), main, 0.77, 0)]
    t1 = box(g, main, 1); T.append((t1, main, 2))                    # a harder target, and an easy prediction on it alone
    P.append((near(g, t1, 0.2), main, sc(), 0))
    t2 = box(g, "Van", 2); T.append((t2, "Van", 0))                  # a similar-class target, and a prediction on it alone
    P.append((near(g, t2, 0.2), main, sc(), 0))
    T.append((box(g, main, 3), main, 0))                             # a target no prediction reaches
    t4 = box(g, main, 4); T.append((t4, main, -1))                   # difficulty -1 on both sides
    P.append((near(g, t4, 0.2), main, sc(), -1))
    t5 = box(g, main, 5); T.append((t5, main, 1))                    # a loose and a tight prediction; the tight one is HARDER
    P += [(near(g, t5, 0.5), main, sc(), 0), (near(g, t5, 0.1), main, sc(), 2)]
    P.append((box(g, "Tram", 6), "Tram", sc(), 0))                   # a class outside `classes`
    T.append((box(g, "DontCare", 7), "DontCare", 0))
    P.append((box(g, main, 8), main, sc(), 1))                       # a prediction on nothing
    if len(classes) > 1:
        T.append((box(g, classes[0], 9), classes[0], 0))
        P.append((near(g, T[-1][0], 0.1), classes[0], sc(), 0))
    out.append(as_dicts(P, T))
    # 4: a class whose columns are all zero (its predictions stand elsewhere)
    other = classes[1] if len(classes) > 1 else main
    T = [(box(g, other, 0), other, 0), (box(g, other, 1), other, 1), (box(g, main, 2), main, 0)]
    P = [(box(g, other, 4), other, sc(), 1), (box(g, other, 5), other, sc(), 0), (near(g, T[2][0], 0.2), main, sc(), 0)]
    out.append(as_dicts(P, T))
    # 5 .. 7: many boxes; frame 6's predictions carry no `difficulty`
    for f in (5, 6, 7):
        T, P = [], []
        for slot in range(11):
            name = main if slot < 7 or len(classes) == 1 else classes[slot % 2]
            if slot == 10:
                name = "Van"
            T.append((box(g, name, slot), name, int(g.integers(0, 3)) if slot else -1))
        for slot in g.permutation(11)[:9]:
            name = T[slot][1] if T[slot][1] != "Van" else main
            P.append((near(g, T[slot][0], float(g.choice([0.1, 0.25, 0.6]))), name, sc(), int(g.integers(0, 3))))
        P += [(near(g, T[1][0], 0.4), main, sc(), 0), (box(g, "Tram", 11), "Tram", sc(), 0), (box(g, main, 12), main, sc(), 2)]
        out.append(as_dicts(P, T, pred_difficulty=f != 6))
    return out


def decisive(pred, target, iou_b, iou_3, classes, difficulties, min_overlap, similar_classes):
    names, similar = det_ref.vocabulary(classes, similar_classes)
    pc, _ = det_ref.ids_and_masks(pred, list(classes), difficulties)
    tl, _ = det_ref.ids_and_masks(target, names, difficulties)
    mo = list(min_overlap) * (len(classes) if len(min_overlap) == 1 else 1)
    for iou in (iou_b, iou_3):
        for c in range(len(classes)):
            rows = np.where(pc == c)[0]
            cols = np.where((tl == c) | ((tl == similar[c]) & (similar[c] >= 0)))[0]
            sub = iou[np.ix_(rows, cols)].astype(np.float64)
            nz = sub[sub != 0]
            if (nz < MARGIN).any() or (np.abs(nz - np.float64(np.float32(mo[c]))) < MARGIN).any():
                return False
            for k, t in enumerate(cols):
                order = np.argsort(-sub[:, k], kind="stable")
                if len(order) >= 2 and sub[order[0], k] > 0 and sub[order[0], k] - sub[order[1], k] < MARGIN and \
                        not np.array_equal(pred["bbox"][rows[order[0]]], pred["bbox"][rows[order[1]]]):
                    return False
    return True


def generate_setting(ref, name, classes, difficulties, min_overlap, similar, seed):
    """The arrays of one setting, or None when the seed's boxes are not decisive."""
    out = {}
    fr = frames(seed, classes)
    preds, targets = [p for p, _ in fr], [t for _, t in fr]
    ious = {True: [], False: []}
    mo_full = list(min_overlap) * (len(classes) if len(min_overlap) == 1 else 1)
    for f, (p, t) in enumerate(fr):
        iou_b = oops.iou_bev(p["bbox"][:, [0, 2, 3, 5, 6]], t["bbox"][:, [0, 2, 3, 5, 6]]).reshape(len(p["label"]), len(t["label"]))
        iou_3 = oops.iou_3d(p["bbox"], t["bbox"]).reshape(len(p["label"]), len(t["label"]))
        if not decisive(p, t, iou_b, iou_3, classes, difficulties, min_overlap, similar):
            return None
        ious[True].append(iou_b)
        ious[False].append(iou_3)
        key = "%s_%d_" % (name, f)
        out.update({key + "pred_bbox": p["bbox"], key + "pred_label": p["label"], key + "pred_score": p["score"],
                    key + "tgt_bbox": t["bbox"], key + "tgt_label": t["label"], key + "tgt_difficulty": t["difficulty"],
                    key + "iou_bev": iou_b, key + "iou_3d": iou_3})
        if "difficulty" in p:
            out[key + "pred_difficulty"] = p["difficulty"]
        for bev in (True, False):
            det, fns = ref.precision_3d(p, t, classes, difficulties, mo_full, bev, similar)
            tag = key + ("bev_" if bev else "3d_")
            out[tag + "detection"], out[tag + "fns"] = np.asarray(det, np.float64), np.asarray(fns, np.int64)
            mine, mine_fn = det_ref.precision_3d(p, t, ious[bev][-1], classes, difficulties, mo_full, similar)
            assert det_ref.rows_of(mine) == det_ref.rows_of(out[tag + "detection"]), (name, f, bev, "detection")
            assert np.array_equal(mine_fn, out[tag + "fns"]), (name, f, bev, "fns")
    out[name + "_gt"] = det_ref.gt_counts(targets, classes, difficulties)
    branches = set()
    for bev in (True, False):
        for samples in SAMPLES:
            ap = np.asarray(ref.mAP(preds, targets, classes, difficulties, min_overlap, bev, samples, similar), np.float64)
            out["%s_mAP_%s_%d" % (name, "bev" if bev else "3d", samples)] = ap
            mine = det_ref.mAP(preds, targets, ious[bev], classes, difficulties, min_overlap, samples, similar)
            assert np.array_equal(mine, ap), (name, bev, samples, mine, ap)
            if samples > 0:
                # which of the two final expressions a (class, difficulty) takes: needs the number of thresholds
                C, D = len(classes), len(difficulties)
                rows = [[[] for _ in range(D)] for _ in range(C)]
                for p, t, iou in zip(preds, targets, ious[bev]):
                    det, _ = det_ref.precision_3d(p, t, iou, classes, difficulties, mo_full, similar)
                    for c in range(C):
                        for j in range(D):
                            rows[c][j].extend(tuple(r) for r in det[c, j].tolist() if any(v != 0 for v in r))
                for c in range(C):
                    for j in range(D):
                        n = len(det_ref.thresholds_of([s for s, tp, _ in rows[c][j] if tp > 0], out[name + "_gt"][c, j], samples))
                        if n:
                            branches.add("few" if len(range(n)[::4]) < int(samples / 4 + 1) else "many")
    return out, branches


def generate():
    ref = reference_module()
    out, seen = {}, set()
    for s, (name, classes, difficulties, min_overlap, similar) in enumerate(SETTINGS):
        for seed in range(1000 * s, 1000 * s + 200):
            got = generate_setting(ref, name, classes, difficulties, min_overlap, similar, seed)
            if got is not None and (name == "one" or "many" in got[1]):
                break
        else:
            raise AssertionError("no decisive seed for " + name)
        out.update(got[0])
        out[name + "_seed"] = np.int64(seed)
        seen |= got[1]
    assert seen == {"few", "many"}, seen
    # the special boxes do what they are there for (setting `similar`, frame 3, BEV, the easiest difficulty of Car)
    det = out["similar_3_bev_detection"][2, 0]
    assert sorted(det[det[:, 0] == np.float64(np.float32(0.77))][:, 1:].tolist()) == [[0.0, 1.0], [1.0, 0.0]], "the twins: one tp, one fp"
    assert (out["kitti_4_bev_detection"][1, :, :, 1] == 0).all() and out["kitti_4_bev_fns"][1, 2, 0] == 2, "the all-zero class"
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
            assert old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k]), k
        print("check ok: %d arrays" % len(out))
        return
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
