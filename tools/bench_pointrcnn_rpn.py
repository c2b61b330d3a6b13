#!/usr/bin/env python3
"""PointRCNN stage 1 on the MI355X: ``PointRCNN.proposals()`` on the native HIP path against the torch formulation
(``ML3D_PRCNN_OPS=torch``) of the same commit behind the SAME backbone, alternating in one process.

The model is pointrcnn_kitti.yml (read from tests/golden/pointrcnn_rpn_kitti.npz, which stores it) with the golden's pseudo-trained
weights; a step is one call on B synthetic clouds of 16 384 points already on the device (the clouds of tools/bench_pointnet2.py
moved to depths that fill both zones), device synchronise before the clock stops.  For B = 1 and B = 4 it reports median / p95 ms
of the whole call and of the share behind the backbone alone (heads + decode + proposals on a cached backbone output), and the
kernel launches of that share on both paths (torch profiler, device activities).

    python tools/bench_pointrcnn_rpn.py --steps 30 --warmup 3 --out profiles/pointrcnn_rpn_bench.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "open3d-ml_amd"), ROOT):
    sys.path.insert(0, p)

import prcnn_ref  # noqa: E402


def launches(fn):
    """Device kernels of one call (torch profiler), or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA")))
    except Exception:
        return None


def stats(t):
    t = np.asarray(t)
    half = len(t) // 2
    return dict(median_ms=float(np.median(t)), p95_ms=float(np.percentile(t, 95)), min_ms=float(t.min()),
                half_gap_ms=float(abs(np.median(t[:half]) - np.median(t[half:]))) if half else 0.0)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--out", default=None, help="markdown file for the table (the JSON line goes to stdout)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointrcnn_rpn: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d.torch.models import PointRCNN
    g = np.load(os.path.join(ROOT, "tests", "golden", "pointrcnn_rpn_kitti.npz"))
    mcfg = json.loads(str(g["model_json"]))
    dev = torch.device("cuda:0")
    model = PointRCNN(**mcfg, device=dev)
    keys, shapes = [str(k) for k in g["state_keys"]], [json.loads(str(s)) for s in g["state_shapes"]]
    model.load_state_dict(prcnn_ref.make_state_dict(keys, shapes, int(g["weights_seed"])), strict=True)
    n0 = int(g["n"])
    res = dict(model="pointrcnn_kitti, stage 1", points_per_cloud=n0, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               runs=[])
    for batch in a.batches:
        offsets = [g["cloud_offsets"][i % len(g["cloud_offsets"])] for i in range(batch)]
        pc = torch.from_numpy(prcnn_ref.make_points(range(100, 100 + batch), n0, int(mcfg["rpn"]["backbone"]["in_channels"]),
                                                    float(g["cloud_scale"]), offsets)).to(dev)
        xyz, feat = model.rpn.backbone(pc)

        def step(mode, tail):
            os.environ["ML3D_PRCNN_OPS"] = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.proposals_from_features(xyz, feat, mode == "hip") if tail else model.proposals(pc)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        run = dict(batch=batch)
        for tail in (False, True):
            outs, times = {}, dict(hip=[], torch=[])
            for _ in range(a.warmup):
                for mode in times:
                    outs[mode] = step(mode, tail)[1]
            for _ in range(a.steps):
                for mode in times:                                  # alternating: both paths see the same box at the same time
                    times[mode].append(step(mode, tail)[0])
            part = {mode: stats(t) for mode, t in times.items()}
            part["torch_over_hip"] = part["torch"]["median_ms"] / part["hip"]["median_ms"]
            run["tail" if tail else "whole"] = part
            run["same_roi_index"] = bool(torch.equal(outs["hip"]["roi_index"], outs["torch"]["roi_index"]))
            run["proposals_per_item"] = (outs["hip"]["roi_index"] >= 0).sum(1).tolist()
        run["tail_launches"] = {mode: launches(lambda: model.proposals_from_features(xyz, feat, mode == "hip")) for mode in ("hip", "torch")}
        res["runs"].append(run)
    os.environ.pop("ML3D_PRCNN_OPS", None)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(res))
    return 0


def markdown(res):
    L = ["# PointRCNN stage 1 (pointrcnn_kitti.yml): HIP path against the torch path of the same commit", "",
         "Written by `tools/bench_pointrcnn_rpn.py --steps %d --warmup %d` on %s; %d points per cloud, clouds already on the device, both "
         "paths alternate in one process behind the same backbone.  `whole` = `PointRCNN.proposals()`; `tail` = heads + decode + "
         "proposals on a cached backbone output." % (res["steps"], res["warmup"], res["device"], res["points_per_cloud"]), "",
         "| B | part | hip median ms | hip p95 ms | torch median ms | torch p95 ms | torch / hip | drift ms (hip, torch) |",
         "|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        for part in ("whole", "tail"):
            p = r[part]
            L.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.3f, %.3f |" %
                     (r["batch"], part, p["hip"]["median_ms"], p["hip"]["p95_ms"], p["torch"]["median_ms"], p["torch"]["p95_ms"],
                      p["torch_over_hip"], p["hip"]["half_gap_ms"], p["torch"]["half_gap_ms"]))
    L += ["", "| B | device kernels of the tail, hip | device kernels of the tail, torch | same roi_index on both paths | proposals per item |",
          "|---|---|---|---|---|"]
    for r in res["runs"]:
        L.append("| %d | %s | %s | %s | %s |" % (r["batch"], r["tail_launches"]["hip"], r["tail_launches"]["torch"], r["same_roi_index"],
                                               r["proposals_per_item"]))
    if not all(r["same_roi_index"] for r in res["runs"]):
        L += ["", "Where `roi_index` differs between the paths: the two paths' heads run on different GEMMs (last-bit differences in "
              "`cls`), and these clouds are not selected for robustness as the golden's are -- near-tied scores change places."]
    slow = [r["batch"] for r in res["runs"] if r["tail"]["torch_over_hip"] < 1.0]
    L += ["", "The HIP tail is %s." % ("faster than the torch formulation at every batch size measured" if not slow else
                                      "NOT faster than the torch formulation at B = %s" % ", ".join(map(str, slow)))]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
