#!/usr/bin/env python3
"""tests/golden/pointrcnn_rcnn_small.npz from the REAL reference's stage 2 (``RCNN.forward`` and ``rcnn.proposal_layer``) on
PyTorch-CPU, behind the stage-1 small case of tools/gen_golden_pointrcnn.py (same clouds, same backbone and RPN configuration, the
same pseudo-trained weights and weight-seed search, extended by the stage-2 conditions below) with a small stage-2 configuration.

The reference is imported through ``oracle.ref_shim`` exactly as the stage-1 generator does.  Its ``roipool3d_utils.roi_pool`` comes
from the open3d wheel, which this project does not have: IN THIS PROCESS it is bound to ``prcnn2_ref.wheel_roi_pool``, the numpy
restatement of the PointRCNN ``roipool3d`` kernel the wheel's op was taken from -- for the wheel's op the restatement IS the oracle
(the one unpinned assumption of stage 2); everything around it (enlarge_box3d, the extra columns, the canonical transform, the
network, the decode, the NMS wiring) is the reference's own code.  FPS / ball query / nms are stood in for as in stage 1.

Conditions on the reference alone, all at ``FIRST_SEED`` (found by ``--scan``; the margins are printed): stage 1's own
``robust()`` (so the product's stage 1 reproduces the reference's rois in order, within 4e-4); every in-box decision DECISIVE by at
least ``IN_BOX_MARGIN`` = 1e-3; every pooled point's score at least 1e-3 from logit(score_thres); every final score at least 1e-3
from score_thres; every pair of decoded boxes at least 1e-3 from nms_thres in BEV IoU; among the rois one that wraps
(0 < hits < S), one that is cut (hits >= S) and an empty one; at least one final box and at least one roi that is not one.  Nothing of the reference's text is stored.

    python tools/gen_golden_pointrcnn2.py            # write the file
    python tools/gen_golden_pointrcnn2.py --check    # regenerate and compare every array with the committed file
    python tools/gen_golden_pointrcnn2.py --scan FIRST STRIDE COUNT    # look for a weight seed that meets the conditions
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
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    sys.path.insert(0, p)

import gen_golden_pointrcnn as G1  # noqa: E402
from oracle import ops as oops  # noqa: E402
import prcnn_ref  # noqa: E402
import prcnn2_ref  # noqa: E402

NAME = "pointrcnn_rcnn_small"
SCORE_THRES = 0.3
# how far every point stays from changing sides of a pooled box: the product's own rois lie within 4e-4 of the reference's
IN_BOX_MARGIN = 1e-3
# Stage 1's small case with 4 rois per cloud instead of 16.  MEASURED at 16: a band of 1e-3 around the faces of the 32 enlarged boxes
# (they cut through the room's walls) holds a point at 24 of 25 seeds, and stage 1's ``robust()`` passes one seed in ~185; no seed of
# 2025 .. 4024 met both.  At 4 about one seed in 30 000 meets every condition; FIRST_SEED is the one the scan (``--scan``) of
# 2025 .. 62 024 found.
NMS_POST_VAL = 4
FIRST_SEED = 43085
RCNN_SMALL = dict(in_channels=32, xyz_up_layer=[32, 32], cls_out_ch=[32, 32], reg_out_ch=[32, 32],
                  SA_config=dict(npoints=[16, 8, -1], radius=[0.5, 1.0, 100], nsample=[16, 16, 16],
                                 mlps=[[32, 32, 32], [32, 32, 64], [64, 64, 64]]),
                  head=dict(loc_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=True, loc_scope=1.5,
                            loc_bin_size=0.5, num_head_bin=9, mean_size=G1.MEAN_SIZE, post_process=False, nms_thres=0.1),
                  target_head=dict(pool_extra_width=1.0, num_points=64))


def stage2_conditions(xyz, rpn_cls, rois, pool_idx, cls, boxes, thr, report):
    b, m = rois.shape[:2]
    big = prcnn2_ref.enlarge(rois, RCNN_SMALL["target_head"]["pool_extra_width"], np.float64)
    logit = np.log(SCORE_THRES / (1 - SCORE_THRES))
    box_m = seg_m = iou_d = np.inf
    near = 0
    for k in range(b):
        for j in range(m):
            d = prcnn2_ref.decisive_margins(xyz[k], big[k, j])
            box_m = min(box_m, float(d.min()))
            near += int((d < 1e-3).sum())
            if pool_idx[k, j, 0] >= 0:
                seg_m = min(seg_m, float(np.abs(rpn_cls[k, pool_idx[k, j], 0].astype(np.float64) - logit).min()))
        c = boxes[k][:, [0, 2, 3, 5, 6]]
        iou = oops.iou_bev(c, c).astype(np.float64)
        iou_d = min(iou_d, float(np.abs(iou[np.triu_indices(m, 1)] - thr).min()))
    score_m = float(np.abs(1 / (1 + np.exp(-cls.astype(np.float64))) - SCORE_THRES).min())
    report("in-box decisive margin %.2e (%d decisions within 1e-3), seg-mask margin %.2e, final-score margin %.2e, IoU distance from "
           "the threshold %.2e" % (box_m, near, seg_m, score_m, iou_d))
    return box_m >= IN_BOX_MARGIN and seg_m >= 1e-3 and score_m >= 1e-3 and iou_d >= 1e-3


def run_case(first=None, stride=1, limit=2000, quiet=False):
    case = G1.plain(G1.CASES["pointrcnn_rpn_small"])
    case["rpn"]["head"]["nms_post_val"] = NMS_POST_VAL
    say = (lambda s: None) if quiet else print
    head = dict(G1.prcnn_ref_defaults(), **case["rpn"]["head"])
    mod = G1.reference_modules()
    rp = importlib.import_module("ml3d.torch.utils.roipool3d.roipool3d_utils")
    utils = importlib.import_module("ml3d.torch.utils.pointnet.pointnet2_utils")

    def wheel(pts, boxes, feats, s):
        pooled, empty = prcnn2_ref.wheel_roi_pool(pts.numpy(), boxes.numpy(), feats.numpy(), s)
        return torch.from_numpy(pooled), torch.from_numpy(empty)

    rp.roi_pool = wheel
    seen = dict(fps=[], ball=[])
    plain_fps, plain_ball = utils.furthest_point_sampling, utils.ball_query

    def fps(*a, **k):
        r = plain_fps(*a, **k)
        seen["fps"].append(r.numpy().astype(np.int32))
        return r

    def ball(*a, **k):
        r = plain_ball(*a, **k)
        seen["ball"].append(r.numpy().astype(np.int32))
        return r

    rpn, rcnn = G1.plain(case["rpn"]), G1.plain(RCNN_SMALL)
    mcfg = dict(rpn=rpn, rcnn=rcnn, mode="RCNN", classes=["Car"], npoints=case["n"], score_thres=SCORE_THRES)
    torch.manual_seed(0)
    model = mod.PointRCNN(device="cpu", augment={}, **json.loads(json.dumps(mcfg)))      # (the constructors edit the lists they are given)
    shapes = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    model.eval()
    pts = prcnn_ref.make_points(case["cloud_seeds"], case["n"], int(rpn["backbone"]["in_channels"]), case["scale"], case["offsets"])
    plain_break = model.rcnn._break_up_pc

    def break_up(pc):
        seen["pts_input"] = pc.detach().clone().numpy()
        return plain_break(pc)

    model.rcnn._break_up_pc = break_up
    s_pts, extra = RCNN_SMALL["target_head"]["num_points"], RCNN_SMALL["target_head"]["pool_extra_width"]
    rh = RCNN_SMALL["head"]
    seed = (FIRST_SEED if first is None else first) - stride
    last = seed + stride * limit
    while True:
        seed += stride
        if seed > last:
            return None
        model.load_state_dict(prcnn_ref.make_state_dict([k for k, _ in shapes], [s for _, s in shapes], seed))
        t0 = time.time()
        with torch.no_grad():
            cls, reg, xyz, feat = model.rpn(torch.from_numpy(pts))
            try:
                rois, _ = model.rpn.proposal_layer(cls[:, :, 0], reg.clone(), xyz)
            except AssertionError:                                    # (the reference's own assertion: an empty near zone)
                continue
            # the cheap conditions first: the pooled boxes against the cloud, then stage 1's own robustness
            big = prcnn2_ref.enlarge(rois.numpy(), extra, np.float64)
            xyz64 = xyz.numpy().astype(np.float64)
            box_m = min(float(prcnn2_ref.decisive_margins(xyz64[k], big[k, j]).min()) for k in range(big.shape[0]) for j in range(big.shape[1]))
            hits = np.array([[int(prcnn2_ref.in_box(xyz64[k], big[k, j], np.float64).sum()) for j in range(big.shape[1])] for k in range(big.shape[0])])
            if box_m < IN_BOX_MARGIN or not ((hits == 0).any() and ((hits > 0) & (hits < s_pts)).any() and (hits >= s_pts).any()):
                continue
            if not G1.robust(cls.numpy(), reg.numpy(), xyz.numpy(), head, lambda s: say("    " + s))[0]:
                continue
            # point_rcnn.py:132-138
            seg_mask = (torch.sigmoid(cls[:, :, 0]) > SCORE_THRES).float()
            pts_depth = torch.norm(xyz, p=2, dim=2)
            utils.furthest_point_sampling, utils.ball_query = fps, ball
            seen["fps"], seen["ball"] = [], []
            try:
                out = model.rcnn(rois, [None], xyz, feat.permute((0, 2, 1)), seg_mask, pts_depth)
            finally:
                utils.furthest_point_sampling, utils.ball_query = plain_fps, plain_ball
            b, m = rois.shape[:2]
            r_cls, r_reg = out["cls"].view(b, m, -1), out["reg"].view(b, m, -1)
            boxes = mod.decode_bbox_target(rois.view(-1, 7), r_reg.view(b * m, -1), anchor_size=torch.tensor(rh["mean_size"]),
                                           loc_scope=rh["loc_scope"], loc_bin_size=rh["loc_bin_size"], num_head_bin=rh["num_head_bin"],
                                           get_xz_fine=rh["loc_xz_fine"], get_y_by_bin=rh["get_y_by_bin"], get_ry_fine=rh["get_ry_fine"],
                                           loc_y_scope=rh["loc_y_scope"], loc_y_bin_size=rh["loc_y_bin_size"]).view(b, m, 7).numpy()
            kept_boxes, kept_scores = model.rcnn.proposal_layer(r_cls, r_reg, rois)
        say("%s: weights seed %d, reference stages 1 + 2 in %.1f s" % (NAME, seed, time.time() - t0))
        rois_n, cls_n, xyz_n = rois.numpy(), cls.numpy(), xyz.numpy()
        rows = feat.permute((0, 2, 1)).contiguous().view(b * case["n"], -1).numpy()
        p32, pool_idx, empty, count = prcnn2_ref.roi_pool(xyz_n, rows, cls_n[:, :, 0], rois_n, s_pts, SCORE_THRES, extra)
        err = float(np.abs(p32 - seen["pts_input"]).max())
        exact = [3] + list(range(5, p32.shape[2]))                   # (the depth column: torch.norm sums in its own order)
        assert np.array_equal(p32[..., exact].view(np.int32), seen["pts_input"][..., exact].view(np.int32)) and err <= 1e-5, \
            "the restated pts_input differs from the reference's: %g" % err
        say("    restated pts_input == reference's: seg mask and features bit for bit, xyz and depth within %.2e; %d of %d rois empty, "
              "hits per roi %s" % (err, int(empty.sum()), b * m, np.minimum(count, s_pts).ravel().tolist()))
        raw = out["cls"].view(b, m).numpy()
        survivors = [oops.nms(prcnn_ref.bev_of(boxes[k]), raw[k], rh["nms_thres"]) for k in range(b)]
        final = sum(int((1 / (1 + np.exp(-raw[k][survivors[k]].astype(np.float64))) > SCORE_THRES).sum()) for k in range(b))
        seg = p32[empty.ravel() == 0][..., 3]
        varied = bool(((count > 0) & (count < s_pts)).any()) and bool((count >= s_pts).any()) and bool((count == 0).any()) and \
            1 <= final < b * m
        say("    varied %s (final boxes %d of %d rois, NMS survivors %s)" % (varied, final, b * m, [len(v) for v in survivors]))
        if varied and stage2_conditions(xyz_n, cls_n, rois_n, pool_idx, out["cls"].numpy(), boxes, rh["nms_thres"], lambda s: say("    " + s)):
            break
    # the reference's own kept boxes are the decoded boxes at the oracle NMS's indices, in its order
    kept = np.full((b, m), -1, np.int32)
    for k in range(b):
        keep = oops.nms(prcnn_ref.bev_of(boxes[k]), out["cls"].view(b, m).numpy()[k], rh["nms_thres"])
        assert np.array_equal(boxes[k][keep], kept_boxes[k].numpy()) and np.array_equal(out["cls"].view(b, m).numpy()[k][keep], kept_scores[k].numpy()[:, 0])
        sig = torch.sigmoid(kept_scores[k][:, 0]).numpy()
        final = keep[sig > np.float32(SCORE_THRES)]
        kept[k, :len(final)] = final
    say("    kept per item after NMS and the score threshold: %s" % (kept >= 0).sum(1).tolist())
    scale = float(max(np.abs(out["cls"].numpy()).max(), np.abs(out["reg"].numpy()).max(), np.abs(seen["pts_input"]).max()))
    levels = len(seen["fps"])
    g = dict(model_json=json.dumps(mcfg), weights_seed=seed, cloud_seeds=np.asarray(case["cloud_seeds"]), n=case["n"],
             cloud_scale=float(case["scale"]), cloud_offsets=np.asarray(case["offsets"], np.float32),
             points_sum=float(pts.astype(np.float64).sum()), state_keys=np.asarray([k for k, _ in shapes]),
             state_shapes=np.asarray([json.dumps(s) for _, s in shapes]), scale=scale, rois=rois_n,
             rpn_cls=np.ascontiguousarray(cls_n[:, :, 0]), pool_idx=pool_idx, empty=empty, pts_input=seen["pts_input"],
             cls=out["cls"].numpy(), reg=out["reg"].numpy(), boxes=boxes, kept=kept, levels=levels)
    for l in range(levels):
        g["fps%d" % l], g["ball%d" % l] = seen["fps"][l], seen["ball"][l]
    return g


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing")
    ap.add_argument("--scan", type=int, nargs=3, metavar=("FIRST", "STRIDE", "COUNT"), default=None,
                    help="print the first weight seed of FIRST, FIRST + STRIDE, ... (COUNT of them) that meets every condition")
    a = ap.parse_args(argv)
    if a.scan:
        g = run_case(a.scan[0], a.scan[1], a.scan[2], quiet=True)
        print("scan from %d by %d: %s" % (a.scan[0], a.scan[1], "none" if g is None else "FOUND %d" % int(g["weights_seed"])), flush=True)
        return 0
    g = run_case()
    assert g is not None and int(g["weights_seed"]) == FIRST_SEED, "FIRST_SEED no longer meets the conditions"
    path = os.path.join(G1.OUT, NAME + ".npz")
    bad = 0
    if a.check:
        old = np.load(path)
        for k, v in g.items():
            if k not in old.files or not np.array_equal(np.asarray(v), old[k]):
                print("%s: %s DIFFERS" % (NAME, k))
                bad += 1
        print("%s: %s" % (NAME, "every array equal" if not bad else "differences found"))
    else:
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) < 600 * 1024, "golden files stay under 600 KB"
        print("%s: wrote %s (%.0f KB), scale %.2f, weights seed %d" % (NAME, path, os.path.getsize(path) / 1024, g["scale"], g["weights_seed"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
