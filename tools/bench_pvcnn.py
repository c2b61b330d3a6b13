#!/usr/bin/env python3
"""PVCNN inference on the MI355X: the native HIP path against the torch formulation (``ML3D_PVCNN_OPS=torch``) on the SAME
native voxel coordinates, alternating in one process.

The model is the ``model`` section of pvcnn_s3dis.yml (read from tests/golden/pvcnn_s3dis.npz, which stores it) with
pseudo-trained weights; a step is one batch of the YAML's shape, 4 synthetic room clouds of 40 960 points: upload of the
pinned host arrays, forward, device synchronise before the clock stops.  Prints and writes one JSON object: median / p95 ms per
batch and clouds per second for both paths, the drift of each (median of the first against the second half of its steps), the
deviation between the two paths' logits and, per convolution layer, the time of the native kernel alone (HIP events around 20
back-to-back launches) with its float32-equivalent TFLOP/s (2 * 27 * cin * cout * B * r^3 operations; cin as the kernel sees it,
i.e. the first layer's 9 channels padded to 32).

    python tools/bench_pvcnn.py --steps 40 --warmup 4 --out profiles/pvcnn_bench.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_pvcnn.py --only hip --steps 5 --warmup 2 --no-layers
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

import pvcnn_ref  # noqa: E402


def conv_layers(model, batch, reps=20):
    """Each distinct convolution of the model alone, native kernel and F.conv3d, on a grid of the density a cloud leaves."""
    from ml3d import ops
    from ml3d.torch.models import pvcnn as native
    P = model.packed_params()
    out, seen = [], set()
    for e in P["blocks"]:
        if e["kind"] != "pvconv":
            continue
        for tag, cin in (("c1", e["cin_pad"]), ("c2", e["cout"])):
            key = (e["r"], cin, e["cout"])
            if key in seen:
                continue
            seen.add(key)
            r, cout = e["r"], e["cout"]
            x = torch.randn((batch, r, r, r, cin), device=model.device) * (torch.rand((batch, r, r, r, 1), device=model.device) < 0.1)
            row = dict(r=r, cin=cin, cout=cout, gflop=2.0 * 27 * cin * cout * batch * r ** 3 / 1e9)
            for name, fn in (("hip", lambda: ops.conv3d_ndhwc(x, e[tag]["packed"], e[tag]["b"], cout)),
                             ("torch", lambda: native._torch_conv3d(x, e[tag]["w"], e[tag]["b"], cout))):
                for _ in range(3):
                    fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / reps
                row[name + "_ms"] = ms
                row[name + "_tflops"] = row["gflop"] / ms
            out.append(row)
    return out


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--only", choices=("hip", "torch"), default=None, help="one path only (for a profiler pass)")
    ap.add_argument("--no-layers", action="store_true", help="skip the per-layer convolution timings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pvcnn: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d.torch.models import PVCNN
    g = np.load(os.path.join(ROOT, "tests", "golden", "pvcnn_s3dis.npz"))
    mcfg = json.loads(str(g["model_json"]))
    dev = torch.device("cuda:0")
    model = PVCNN(**mcfg, device=dev)
    model.load_state_dict(pvcnn_ref.make_state_dict(mcfg, int(g["weights_seed"])))
    model.eval()
    model.packed_params()
    point, feat = pvcnn_ref.make_inputs(range(100, 100 + a.clouds), a.points, lattice=False)
    host = dict(point=torch.from_numpy(point).pin_memory(), feat=torch.from_numpy(feat).pin_memory())

    def step(mode):
        os.environ["ML3D_PVCNN_OPS"] = mode
        t0 = time.perf_counter()
        out = model(host)                                           # the upload is part of the step
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

    res = dict(model="pvcnn_s3dis", width_multiplier=mcfg["width_multiplier"],
               voxel_resolution_multiplier=mcfg["voxel_resolution_multiplier"], clouds_per_batch=a.clouds,
               points_per_cloud=a.points, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for mode in modes:
        t = np.asarray(times[mode])
        half = len(t) // 2
        res[mode] = dict(median_ms=float(np.median(t)), p95_ms=float(np.percentile(t, 95)), min_ms=float(t.min()),
                         clouds_per_s=float(a.clouds / (np.median(t) * 1e-3)),
                         half_gap_ms=float(abs(np.median(t[:half]) - np.median(t[half:]))) if half else 0.0)
    if len(modes) == 2:
        res["speedup_hip_over_torch"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
        res["difference_ms"] = res["torch"]["median_ms"] - res["hip"]["median_ms"]
        res["drift_ms"] = max(res["hip"]["half_gap_ms"], res["torch"]["half_gap_ms"])
        res["max_abs_logit_delta"] = float((outs["hip"] - outs["torch"]).abs().max())
        res["logit_scale"] = float(outs["torch"].abs().max())
    if not a.no_layers:
        res["conv_layers"] = conv_layers(model, a.clouds)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
