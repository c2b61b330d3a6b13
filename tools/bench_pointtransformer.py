#!/usr/bin/env python3
"""PointTransformer inference on the MI355X: the fused HIP path against the torch formulation (``ML3D_PT_OPS=torch``) on the
SAME native k-NN / FPS indices, alternating in one process.

The model is the ``model`` section of pointtransformer_s3dis.yml (read from tests/golden/pointtransformer_s3dis.npz, which
stores it) with pseudo-trained weights; a step is one batch of 3 synthetic room clouds of 40 960 points (``num_points`` of the
YAML): upload of the host arrays, forward, device synchronise before the clock stops.  Prints and writes one JSON object:
median / p95 ms per batch and clouds per second for both paths, the run-to-run spread of each (median of the first against the
second half of its steps) and the deviation between the two paths' logits.

    python tools/bench_pointtransformer.py --steps 60 --warmup 5 --out profiles/pointtransformer_bench.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_pointtransformer.py --only hip --steps 5 --warmup 2
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

import pt_ref  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=3)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--only", choices=("hip", "torch"), default=None, help="one path only (for a profiler pass)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointtransformer: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d.torch.dataloaders import PointTransformerBatch
    from ml3d.torch.models import PointTransformer
    g = np.load(os.path.join(ROOT, "tests", "golden", "pointtransformer_s3dis.npz"))
    mcfg = json.loads(str(g["model_json"]))
    dev = torch.device("cuda:0")
    model = PointTransformer(**mcfg, device=dev)
    model.load_state_dict(pt_ref.make_state_dict(mcfg, int(g["weights_seed"])))
    model.eval()
    model.packed_params()
    pts, feat, rs = pt_ref.make_batch_arrays(range(100, 100 + a.clouds), [a.points] * a.clouds)
    items = [{"data": dict(point=torch.from_numpy(pts[rs[i]:rs[i + 1]]).pin_memory(),
                           feat=torch.from_numpy(feat[rs[i]:rs[i + 1]]).pin_memory(),
                           label=torch.zeros(int(rs[i + 1] - rs[i]), dtype=torch.int64))} for i in range(a.clouds)]

    def step(mode):
        os.environ["ML3D_PT_OPS"] = mode
        t0 = time.perf_counter()
        out = model(PointTransformerBatch(items).to(dev))          # the upload is part of the step
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    modes = [a.only] if a.only else ["hip", "torch"]
    outs = {}
    for _ in range(a.warmup):
        for mode in modes:
            outs[mode] = step(mode)[1]
    times = {mode: [] for mode in modes}
    for _ in range(a.steps):
        for mode in modes:                                          # alternating: both paths see the same box at the same time
            times[mode].append(step(mode)[0])

    res = dict(model="pointtransformer_s3dis", blocks=mcfg["blocks"], clouds_per_batch=a.clouds, points_per_cloud=a.points,
               steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for mode in modes:
        t = np.asarray(times[mode])
        half = len(t) // 2
        res[mode] = dict(median_ms=float(np.median(t)), p95_ms=float(np.percentile(t, 95)), min_ms=float(t.min()),
                         clouds_per_s=float(a.clouds / (np.median(t) * 1e-3)),
                         spread_ms=float(abs(np.median(t[:half]) - np.median(t[half:]))) if half else 0.0)
    if len(modes) == 2:
        res["speedup_hip_over_torch"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
        res["max_abs_logit_delta"] = float((outs["hip"] - outs["torch"]).abs().max())
        res["logit_scale"] = float(outs["torch"].abs().max())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
