#!/usr/bin/env python3
"""tests/golden/pointrcnn_rpn_{small,kitti}.npz from the REAL reference's stage 1 on PyTorch-CPU.

The reference's ``ml3d/torch/models/point_rcnn.py`` is imported through ``oracle.ref_shim``; its wheel ops are stood in for by
the CPU restatements of tests/pn2_ref.py (furthest point sampling, ball query, 3-NN, interpolation, as
tools/gen_golden_pointnet2.py does) and, for ``nms``, by the repository's CPU oracle (the shim's own wiring).  The reference
``PointRCNN`` is built on the CPU with the pseudo-trained weights of ``prcnn_ref.make_state_dict`` and run in eval mode:
``rpn(points)`` and ``rpn.proposal_layer(...)``.  The script ASSERTS that the numpy restatement of tests/prcnn_ref.py, fed the
reference's own cls / reg / xyz, reproduces the reference's rois and scores BIT FOR BIT and in order -- that pins the restatement,
which judges the product where the reference does not exist.  For the small case it takes the FIRST weight seed, counting up, at
which the reference alone is robust (``robust()`` below: conditions on the inputs).  It needs the reference checkout, so it runs on
the authoring machine only; the tests read the ``.npz`` files.  Nothing of the reference's text is stored.

    python tools/gen_golden_pointrcnn.py            # write both files
    python tools/gen_golden_pointrcnn.py --check    # regenerate and compare every array with the committed file
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

from oracle import ref_shim  # noqa: E402
from oracle import ops as oops  # noqa: E402
import pn2_ref  # noqa: E402
import prcnn_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SMALL_BACKBONE = dict(in_channels=3, use_xyz=True,
                      SA_config=dict(npoints=[256, 64], radius=[[0.5, 1.0], [1.0, 2.0]], nsample=[[16, 32], [16, 32]],
                                     mlps=[[[16, 16, 32], [32, 32, 64]], [[32, 32, 64], [64, 48, 64]]]),
                      fp_mlps=[[64, 32], [64, 64]])
MEAN_SIZE = [1.52563191462, 1.62856739989, 3.88311640418]
# offsets: z (column 2) is the depth the zones are cut on.  small: item 0 straddles 40 m (both zones), item 1 lies wholly inside
# the near zone (EMPTY far zone: the fallback arm); kitti: item 0 straddles, item 1 near.
CASES = dict(
    pointrcnn_rpn_small=dict(rpn=dict(backbone=SMALL_BACKBONE, cls_in_ch=32, cls_out_ch=[32], reg_in_ch=32, reg_out_ch=[32],
                                      head=dict(loc_xz_fine=True, loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, nms_pre=64,
                                                nms_post=32, nms_thres=0.85, nms_post_val=16, nms_thres_val=0.8, mean_size=MEAN_SIZE)),
                             n=1024, cloud_seeds=[51, 52], scale=1.0, offsets=[[-3.0, -1.0, 37.5], [-3.0, -1.0, 12.0]], first_seed=2025,
                             search=True, row_stride=1),
    pointrcnn_rpn_kitti=dict(yaml="pointrcnn_kitti", n=16384, cloud_seeds=[61, 62], scale=2.0,
                             offsets=[[-6.0, -3.0, 35.0], [-6.0, -3.0, 8.0]], first_seed=2025, search=False, row_stride=64),
)


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def reference_modules():
    ref_shim.install()
    sys.modules["open3d.core.cuda"].device_count = lambda: 1
    mod = importlib.import_module("ml3d.torch.models.point_rcnn")
    utils = importlib.import_module("ml3d.torch.utils.pointnet.pointnet2_utils")
    for m in (mod, utils):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), m.__file__
    cpu = pn2_ref.torch_ops()
    utils.furthest_point_sampling, utils.ball_query = cpu["furthest_point_sampling"], cpu["ball_query"]
    utils.three_nn, utils.three_interpolate = cpu["three_nn"], cpu["three_interpolate"]
    return mod


def robust(cls, reg, xyz, head, report, pairs=True):
    """The reference alone is robust at these inputs: magnitudes inside [5, 23]; among each zone's taken candidates plus the next
    one in order the consecutive score gaps, every candidate row's argmax margins and every candidate pair's distance of its BEV
    IoU from the threshold at least 1e-3."""
    b, n = cls.shape[:2]
    mc, mr = float(np.abs(cls).max()), float(np.abs(reg).max())
    ok = 5.0 <= mc <= 23.0 and 5.0 <= mr <= 23.0
    detail = {}
    boxes = prcnn_ref.decode(xyz.reshape(b * n, 3), reg.reshape(b * n, -1), head["mean_size"], head["loc_scope"], head["loc_bin_size"],
                             head["num_head_bin"], head["loc_xz_fine"], detail=detail).reshape(b, n, 7)
    margin = detail["margin"].reshape(b, n)
    thr = head["nms_thres_val"]
    gap = mar = iou_d = np.inf
    for k in range(b):
        order, zones, nexts = prcnn_ref.zone_candidates(cls[k, :, 0], boxes[k], head["nms_pre"], with_next=True)
        for pos, nxt in zip(zones, nexts):
            if len(pos) == 0:
                continue
            more = pos if nxt is None else np.concatenate((pos, [nxt]))
            s = cls[k, order[more], 0].astype(np.float64)
            if len(s) > 1:
                gap = min(gap, float(np.min(s[:-1] - s[1:])))
            mar = min(mar, float(margin[k, order[pos]].min()))
            if not pairs:                                             # (thousands of candidates: the figure is only reported)
                continue
            c = boxes[k][order[pos]][:, [0, 2, 3, 5, 6]]
            iou = oops.iou_bev(c, c).astype(np.float64)
            iou_d = min(iou_d, float(np.abs(iou[np.triu_indices(len(pos), 1)] - thr).min()) if len(pos) > 1 else np.inf)
    report("max|cls| %.2f max|reg| %.2f, score gap %.2e, argmax margin %.2e, IoU distance from the threshold %.2e" % (mc, mr, gap, mar, iou_d))
    return ok and gap >= 1e-3 and mar >= 1e-3 and iou_d >= 1e-3, max(mc, mr)


def run_case(name, case):
    mod = reference_modules()
    if "yaml" in case:
        from ml3d.utils import Config          # the reference's, through the shim
        cfg = Config.load_from_file(os.path.join(ref_shim.REF_ROOT, "ml3d", "configs", case["yaml"] + ".yml"))
        rpn, rcnn = plain(cfg.model.rpn), plain(cfg.model.rcnn)
        rpn["backbone"].setdefault("use_xyz", True)
    else:
        rpn, rcnn = plain(case["rpn"]), {}
    mcfg = dict(rpn=rpn, rcnn=rcnn, mode="RPN", classes=["Car"], npoints=case["n"])
    torch.manual_seed(0)
    model = mod.PointRCNN(device="cpu", augment={}, **json.loads(json.dumps(mcfg)))      # (the constructors edit the lists they are given)
    shapes = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    model.eval()
    head = dict(prcnn_ref_defaults(), **rpn["head"])
    pts = prcnn_ref.make_points(case["cloud_seeds"], case["n"], int(rpn["backbone"]["in_channels"]), case["scale"], case["offsets"])
    seed = case["first_seed"]
    while True:
        model.load_state_dict(prcnn_ref.make_state_dict([k for k, _ in shapes], [s for _, s in shapes], seed))
        t0 = time.time()
        with torch.no_grad():
            cls, reg, xyz, feat = model.rpn(torch.from_numpy(pts))
            try:
                rois, roi_scores = model.rpn.proposal_layer(cls[:, :, 0], reg.clone(), xyz)
            except AssertionError:                                    # (the reference's own assertion: an empty near zone)
                rois = None
        cls, reg, xyz = cls.numpy(), reg.numpy(), xyz.numpy()
        print("%s: weights seed %d, reference stage 1 in %.1f s" % (name, seed, time.time() - t0))
        good, scale = robust(cls, reg, xyz, head, lambda s: print("    " + s), pairs=case["search"])
        good = good and rois is not None
        assert rois is not None or case["search"], "the reference asserts on an empty near zone"
        if good or not case["search"]:
            break
        seed += 1
        assert seed < case["first_seed"] + 2000
    assert np.array_equal(xyz, pts[..., :3])
    # the restatement on the reference's own head outputs: bit for bit, in order
    r_rois, r_scores, r_index, boxes = prcnn_ref.rpn_stage(cls, reg, xyz, head)
    rois, roi_scores = rois.numpy(), roi_scores.numpy()
    assert rois.shape == r_rois.shape and np.array_equal(rois.view(np.int32), r_rois.view(np.int32)), "restated rois differ from the reference's"
    assert np.array_equal(roi_scores.view(np.int32), r_scores.view(np.int32)), "restated roi scores differ from the reference's"
    filled = (r_index >= 0).sum(1)
    print("    restatement == reference: %s proposals per item, far zone %s" %
          (filled.tolist(), ["empty" if not ((boxes[k, :, 2] > 40) & (boxes[k, :, 2] <= 80)).any() else "populated" for k in range(len(pts))]))
    st = case["row_stride"]
    return dict(model_json=json.dumps(mcfg), weights_seed=seed, cloud_seeds=np.asarray(case["cloud_seeds"]), n=case["n"],
                cloud_scale=float(case["scale"]), cloud_offsets=np.asarray(case["offsets"], np.float32),
                points_sum=float(pts.astype(np.float64).sum()), state_keys=np.asarray([k for k, _ in shapes]),
                state_shapes=np.asarray([json.dumps(s) for _, s in shapes]), scale=scale, row_stride=st,
                cls=np.ascontiguousarray(cls[:, ::st]), reg=np.ascontiguousarray(reg[:, ::st]), rois=rois, roi_scores=roi_scores,
                roi_index=r_index.astype(np.int32))


def prcnn_ref_defaults():
    return dict(nms_pre=9000, nms_post=512, nms_thres=0.85, nms_post_val=None, nms_thres_val=None, loc_xz_fine=True, loc_scope=3.0,
                loc_bin_size=0.5, num_head_bin=12, get_y_by_bin=False, get_ry_fine=False, loc_y_scope=0.5, loc_y_bin_size=0.25)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing")
    ap.add_argument("names", nargs="*", default=list(CASES))
    a = ap.parse_args(argv)
    bad = 0
    for name in a.names:
        g = run_case(name, CASES[name])
        path = os.path.join(OUT, name + ".npz")
        if a.check:
            old = np.load(path)
            for k, v in g.items():
                if k not in old.files or not np.array_equal(np.asarray(v), old[k]):
                    print("%s: %s DIFFERS" % (name, k))
                    bad += 1
            print("%s: %s" % (name, "every array equal" if not bad else "differences found"))
        else:
            np.savez_compressed(path, **g)
            assert os.path.getsize(path) < 600 * 1024, "golden files stay under 600 KB"
            print("%s: wrote %s (%.0f KB), scale %.2f, weights seed %d" % (name, path, os.path.getsize(path) / 1024, g["scale"], g["weights_seed"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
