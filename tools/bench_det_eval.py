#!/usr/bin/env python3
"""Time the detection metric on a synthetic validation split (no dataset, no checkout): 3769 frames (KITTI's validation split),
about 50 predictions and 15 targets a frame, 3 classes, 3 difficulties, seeded.  Three ways, alternating, after a warm-up:

* ``ObjdetMetric.compute()``                 one ``det_match`` for BEV and 3-D together;
* two ``mAP`` calls, device route            one ``det_match`` each;
* two ``mAP`` calls, ``ML3D_DET_EVAL=host``  per frame and metric one upload, one IoU launch, one read-back: the route before
                                             ``det_match``, the baseline.

Each time is a host clock around a call that ends in a read-back (a device synchronise) and includes the host's encoding and AP
parts; the median and the spread (min .. max) of the repeats are reported with the launches and transfers each route makes (counted
by ``ml3d.metrics.mAP.STATS``), and the three results are compared for equality.  Needs the GPU.

    python tools/bench_det_eval.py --out profiles/det_eval_bench.md
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd")):
    sys.path.insert(0, p)

CLASSES, DIFFICULTIES, MIN_OVERLAP = [0, 1, 2], [0, 1, 2], [0.5, 0.5, 0.7]


def synthetic_split(frames, seed=0, mean_pred=50, mean_tgt=15):
    g = np.random.default_rng(seed)
    preds, targets = [], []
    for _ in range(frames):
        T, P = int(g.poisson(mean_tgt)), int(g.poisson(mean_pred))
        side = int(np.ceil(np.sqrt(max(T, 1))))
        k = np.arange(T)
        tb = np.stack([12.0 * (k % side) + g.uniform(-1, 1, T), 1.6 + g.uniform(-0.1, 0.1, T), 12.0 * (k // side) + g.uniform(-1, 1, T),
                       g.uniform(1.4, 2.0, T), g.uniform(1.4, 1.8, T), g.uniform(3.4, 4.4, T), g.uniform(-np.pi, np.pi, T)], 1)
        tl = g.integers(0, 4, T)                                          # label 3: a class that is not evaluated
        on = g.integers(0, max(T, 1), P)
        hit = (g.uniform(size=P) < 0.8) & (T > 0)
        pb = np.stack([-40.0 - 12.0 * np.arange(P), np.full(P, 1.6), np.full(P, -40.0), g.uniform(1.4, 2.0, P), g.uniform(1.4, 1.8, P),
                       g.uniform(3.4, 4.4, P), g.uniform(-np.pi, np.pi, P)], 1)
        pl = g.integers(0, 4, P)
        if T:
            near = tb[on] + np.stack([g.uniform(-0.5, 0.5, P), g.uniform(-0.05, 0.05, P), g.uniform(-0.5, 0.5, P), np.zeros(P), np.zeros(P),
                                      np.zeros(P), g.uniform(-0.15, 0.15, P)], 1)
            pb = np.where(hit[:, None], near, pb)
            pl = np.where(hit & (g.uniform(size=P) < 0.9), tl[on], pl)
        preds.append({"bbox": pb.astype(np.float32), "label": pl, "score": g.uniform(size=P).astype(np.float32), "difficulty": g.integers(-1, 3, P)})
        targets.append({"bbox": tb.astype(np.float32), "label": tl, "difficulty": g.integers(-1, 3, T)})
    return preds, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="write the markdown report here")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_det_eval.py measures on the GPU; there is no CPU fallback"
    from ml3d import metrics as M
    mod = importlib.import_module("ml3d.metrics.mAP")
    preds, targets = synthetic_split(args.frames)
    n_pred, n_tgt = sum(len(p["label"]) for p in preds), sum(len(t["label"]) for t in targets)

    def objdet():
        m = M.ObjdetMetric(CLASSES, DIFFICULTIES, MIN_OVERLAP)
        m.update(preds, targets)
        r = m.compute()
        return np.stack([r["bev"], r["3d"]])

    def two_map():
        return np.stack([M.mAP(preds, targets, CLASSES, DIFFICULTIES, MIN_OVERLAP, bev=b)[:, :, 0] for b in (True, False)])

    def host():
        os.environ["ML3D_DET_EVAL"] = "host"
        try:
            return two_map()
        finally:
            del os.environ["ML3D_DET_EVAL"]

    routes = (("ObjdetMetric.compute()", objdet), ("2 x mAP, device route", two_map), ("2 x mAP, ML3D_DET_EVAL=host", host))
    times, stats, results = {n: [] for n, _ in routes}, {}, {}
    for rep in range(args.warmup + args.repeats):
        for name, fn in routes:                                           # alternating: the routes share whatever else the host does
            mod.STATS.update(dict.fromkeys(mod.STATS, 0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(dt)
            stats[name] = dict(mod.STATS)
    first = results[routes[0][0]]
    equal = all(np.array_equal(first, results[n]) for n, _ in routes)
    # the host parts of the device route, timed apart (host clocks; the match ends in a read-back)
    t0 = time.perf_counter()
    S = mod._Split(preds, targets, CLASSES, DIFFICULTIES, MIN_OVERLAP, {})
    t1 = time.perf_counter()
    flags, _ = mod._match(S, 3, None)
    t2 = time.perf_counter()
    mod._ap_table(S, flags[0], 41), mod._ap_table(S, flags[1], 41)
    t3 = time.perf_counter()
    parts = {"encode_s": t1 - t0, "upload_match_readback_s": t2 - t1, "ap_s": t3 - t2}
    pairs = int((np.diff(S.pred.start) * np.diff(S.tgt.start)).sum())
    rows = []
    for name, _ in routes:
        ts = times[name]
        st = stats[name]
        launches = 2 * st["det_match"] + st["iou_launches"]
        rows.append({"route": name, "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "kernel_launches": launches,
                     "uploads": st["uploads"], "readbacks": st["readbacks"]})
    report = {"frames": args.frames, "predictions": n_pred, "targets": n_tgt, "kept_pairs_per_plane": pairs, "repeats": args.repeats,
              "results_equal": equal, "routes": rows, "device_route_parts": parts, "device": torch.cuda.get_device_name(0),
              "mAP_bev_last_difficulty": first[0][:, -1].tolist(), "mAP_3d_last_difficulty": first[1][:, -1].tolist()}
    print(json.dumps(report))
    if args.out:
        base = rows[2]["median_s"]
        lines = ["# Detection metric: `det_match` against the per-frame host loop", "",
                 "`python tools/bench_det_eval.py` on %s: %d frames, %d predictions, %d targets (seeded), 3 classes, 3 difficulties," %
                 (report["device"], args.frames, n_pred, n_tgt),
                 "%d (prediction, target) pairs per plane after the class filter.  Host clock around each call (each ends in a read-back);" % pairs,
                 "median of %d alternating repeats after %d warm-up, spread = min .. max.  The times include the host's label / difficulty" %
                 (args.repeats, args.warmup),
                 "encoding and the float64 AP part.", "",
                 "| route | median s | spread s | kernel launches | uploads | read-backs | vs host route |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append("| %s | %.4f | %.4f .. %.4f | %d | %d | %d | %.1f x |" % (r["route"], r["median_s"], r["min_s"], r["max_s"],
                                                                                 r["kernel_launches"], r["uploads"], r["readbacks"], base / r["median_s"]))
        lines += ["", "The three routes' AP tables are %s." % ("EQUAL (float64, every class and difficulty)" if equal else "NOT equal"), "",
                  "One `ObjdetMetric.compute()` apart (single run, host clocks): encoding %.4f s, upload + `det_match` + read-back %.4f s, AP %.4f s." %
                  (parts["encode_s"], parts["upload_match_readback_s"], parts["ap_s"]), ""]
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
    assert equal, "the routes disagree"


if __name__ == "__main__":
    main()
