#!/usr/bin/env python3
"""PointRCNN stage 2 on the MI355X: RoI pooling, the RCNN network and the decode + NMS of ``inference_end`` on the native HIP path
against the torch formulation (``ML3D_PRCNN_OPS=torch``) of the same commit, alternating in one process on the SAME inputs.

The model is pointrcnn_kitti.yml (read from tests/golden/pointrcnn_rpn_kitti.npz, which stores it) with the golden's pseudo-trained
weights, B synthetic clouds of 16 384 points already on the device, ``nms_post_val`` = 100 rois per cloud.  The pseudo-trained RPN's
own boxes have negative sizes and pool nothing, so the rois are car-sized boxes (every seventh up to seven car lengths long) around
points of the cloud: the pooling has hits to rank and rows to copy.  Per stage (pooling / up + merge / each SA level / heads /
decode + NMS) a step is the stage over all roi chunks with a device synchronise on both sides of every call: the small stages are a
few launches each, so their rows are upper bounds that include launch and synchronise overhead; `sum of stages` adds them up.
`whole call` is ``rcnn_from_proposals`` + ``rcnn_boxes`` timed as ONE call, one synchronise at its end.  Median / p95 ms, and the
device kernels of one whole call on both paths (torch profiler).

    python tools/bench_pointrcnn_rcnn.py --steps 30 --warmup 3 --out profiles/pointrcnn_rcnn_bench.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "open3d-ml_amd"), ROOT):
    sys.path.insert(0, p)

import prcnn_ref  # noqa: E402
from bench_pointrcnn_rpn import launches, stats  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--out", default=None, help="markdown file for the table (the JSON line goes to stdout)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointrcnn_rcnn: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d.ops import pointrcnn as prcnn_ops
    from ml3d.torch.models import PointRCNN, point_rcnn
    g = np.load(os.path.join(ROOT, "tests", "golden", "pointrcnn_rpn_kitti.npz"))
    mcfg = dict(json.loads(str(g["model_json"])), mode="RCNN")
    dev = torch.device("cuda:0")
    model = PointRCNN(**mcfg, device=dev)
    keys, shapes = [str(k) for k in g["state_keys"]], [json.loads(str(s)) for s in g["state_shapes"]]
    model.load_state_dict(prcnn_ref.make_state_dict(keys, shapes, int(g["weights_seed"])), strict=True)
    rc = model.rcnn
    n0 = int(g["n"])
    res = dict(model="pointrcnn_kitti, stage 2", points_per_cloud=n0, steps=a.steps, warmup=a.warmup, chunk=a.chunk,
               device=torch.cuda.get_device_name(0), runs=[])
    for batch in a.batches:
        offsets = [g["cloud_offsets"][i % len(g["cloud_offsets"])] for i in range(batch)]
        pts = prcnn_ref.make_points(range(100, 100 + batch), n0, int(mcfg["rpn"]["backbone"]["in_channels"]), float(g["cloud_scale"]), offsets)
        r = model.proposals(torch.from_numpy(pts).to(dev))
        rois = r["rois"].cpu().numpy().copy()
        m = rois.shape[1]
        for i in range(batch):
            for j in range(m):
                c = pts[i, (j * 163) % n0, :3]
                rois[i, j] = (c[0], c[1] + 0.75, c[2], 1.5, 1.6, 3.9 * (1 + 6 * (j % 7 == 0)), 0.37 * j - 3.0)
        r = dict(r, rois=torch.from_numpy(rois).to(dev))
        xyz, rows, scores = r["xyz"], r["feature_rows"], r["cls"].reshape(batch, n0)
        names = ["pooling", "up + merge"] + ["SA level %d" % i for i in range(len(rc.SA_modules))] + ["heads", "decode + NMS", "sum of stages", "whole call"]
        times = {mode: {k: [] for k in names} for mode in ("hip", "torch")}
        outs = {}

        def clock(bucket, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = fn()
            torch.cuda.synchronize()
            bucket.append(bucket.pop() + (time.perf_counter() - t0) * 1e3)
            return v

        def step(mode, keep):
            hip = mode == "hip"
            os.environ["ML3D_PRCNN_OPS"] = mode
            T = times[mode]
            for k in names:
                T[k].append(0.0)
            pool = prcnn_ops.roi_pool if hip else point_rcnn._torch_roi_pool
            with torch.no_grad():
                pin, idx, empty = clock(T["pooling"], lambda: pool(xyz, rows, scores, r["rois"], rc.num_points, model.score_thres,
                                                                     rc.pool_extra_width))
                parts = []
                for lo in range(0, pin.shape[0], a.chunk):
                    x, f = clock(T["up + merge"], lambda: rc._up_merge(pin[lo:lo + a.chunk], hip))
                    for i in range(len(rc.SA_modules)):
                        x, f = clock(T["SA level %d" % i], lambda: rc._level(i, x, f, hip))[:2]
                    parts.append(f)
                heads = clock(T["heads"], lambda: rc._heads(torch.cat(parts), hip))
                results = dict(rois=r["rois"], cls=heads["cls"], reg=heads["reg"])
                boxes = clock(T["decode + NMS"], lambda: model.rcnn_boxes(results))
            T["sum of stages"][-1] = sum(T[k][-1] for k in names[:-2])
            clock(T["whole call"], lambda: model.rcnn_boxes(model.rcnn_from_proposals(r, chunk=a.chunk)))
            if not keep:
                for k in names:
                    T[k].pop()
            outs[mode] = dict(cls=heads["cls"], count=boxes[3], hits=int((empty == 0).sum()))

        for _ in range(a.warmup):
            for mode in times:
                step(mode, False)
        for _ in range(a.steps):
            for mode in times:                                      # alternating: both paths see the same box at the same time
                step(mode, True)
        run = dict(batch=batch, rois=int(batch * m), nonempty=outs["hip"]["hits"], stages={})
        for k in names:
            run["stages"][k] = {mode: stats(times[mode][k]) for mode in times}
        run["max_abs_cls_delta"] = float((outs["hip"]["cls"] - outs["torch"]["cls"]).abs().max())

        def whole(mode):
            os.environ["ML3D_PRCNN_OPS"] = mode
            model.rcnn_boxes(model.rcnn_from_proposals(r, chunk=a.chunk))

        run["launches"] = {mode: launches(lambda: whole(mode)) for mode in ("hip", "torch")}
        res["runs"].append(run)
    os.environ.pop("ML3D_PRCNN_OPS", None)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(res))
    return 0


def markdown(res):
    L = ["# PointRCNN stage 2 (pointrcnn_kitti.yml): HIP path against the torch path of the same commit", "",
         "Written by `tools/bench_pointrcnn_rcnn.py --steps %d --warmup %d --chunk %d` on %s; %d points per cloud, 100 car-sized rois per "
         "cloud around points of the cloud, everything already on the device, both paths alternate in one process on the same inputs; a "
         "stage's time is summed over the roi chunks with a device synchronise around every call (rows of a few tenths of a millisecond "
         "are upper bounds: launch and synchronise overhead); `whole call` is `rcnn_from_proposals` + `rcnn_boxes` as one call with one "
         "synchronise at its end." %
         (res["steps"], res["warmup"], res["chunk"], res["device"], res["points_per_cloud"]), "",
         "| B | stage | hip median ms | hip p95 ms | torch median ms | torch p95 ms | torch / hip | share of hip | drift ms (hip, torch) |",
         "|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        total = r["stages"]["sum of stages"]["hip"]["median_ms"]
        for k, p in r["stages"].items():
            L.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.0f %% | %.3f, %.3f |" %
                     (r["batch"], k, p["hip"]["median_ms"], p["hip"]["p95_ms"], p["torch"]["median_ms"], p["torch"]["p95_ms"],
                      p["torch"]["median_ms"] / max(p["hip"]["median_ms"], 1e-9), 100 * p["hip"]["median_ms"] / max(total, 1e-9),
                      p["hip"]["half_gap_ms"], p["torch"]["half_gap_ms"]))
    L += ["", "| B | rois | non-empty rois | device kernels of stage 2, hip | device kernels of stage 2, torch | max abs cls delta hip - torch |",
          "|---|---|---|---|---|---|"]
    for r in res["runs"]:
        L.append("| %d | %d | %d | %s | %s | %.3g |" % (r["batch"], r["rois"], r["nonempty"], r["launches"]["hip"], r["launches"]["torch"],
                                                      r["max_abs_cls_delta"]))
    for r in res["runs"]:
        parts = {k: v["hip"]["median_ms"] for k, v in r["stages"].items() if k not in ("sum of stages", "whole call")}
        top = max(parts, key=parts.get)
        L += ["", "B = %d: the largest stage of the HIP path is `%s` (%.1f ms of the stages' %.1f ms); the whole call takes %.1f ms "
              "(torch formulation: %.1f ms)." % (r["batch"], top, parts[top], r["stages"]["sum of stages"]["hip"]["median_ms"],
                                               r["stages"]["whole call"]["hip"]["median_ms"], r["stages"]["whole call"]["torch"]["median_ms"])]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
