#!/usr/bin/env python3
"""SparseConvUnet inference on the MI355X: the native HIP path against the torch formulation (``ML3D_SCN_OPS=torch``) on the
SAME native rulebooks and folded weights, alternating in one process.

The model is the ``model`` section of sparseconvunet_scannet.yml (read from tests/golden/sparseconvunet_scannet.npz, which
stores it) with pseudo-trained weights; a step is one batch of ``--clouds`` synthetic rooms of ``--points`` points at the
YAML's 2 cm voxels: upload of the pinned host arrays, rulebook build, forward, device synchronise before the clock stops.
Prints and writes one JSON object: median / p95 ms per batch for both paths, the drift of each (median of the first against
the second half of its steps), the deviation between the two paths' logits, the rulebook build alone (HIP events) and its share
of the native forward, and per level the submanifold convolution C -> C alone (HIP events around back-to-back launches) with
its float32-equivalent TFLOP/s counted over the neighbours that EXIST (2 * pairs * cin * cout) and over the padded 27 taps the
kernel multiplies.

    python tools/bench_sparseconvunet.py --steps 30 --warmup 4 --out profiles/sparseconvunet_bench.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_sparseconvunet.py --only hip --steps 5 --warmup 2 --no-layers
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

import scn_ref  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def conv_levels(model, pyr, reps=10):
    """The submanifold convolution C_l -> C_l of every level alone, native kernel and torch formulation."""
    from ml3d import ops
    from ml3d.torch.models import sparseconvunet as native
    out = []
    for l, c in enumerate(model.planes):
        rows = pyr.rows(l)
        rule = pyr.nbr27(l).contiguous()
        pairs = int((rule >= 0).sum())
        w = torch.randn((27, c, c), device=model.device) / float(np.sqrt(5 * c))
        wt, _, cp, _ = ops.pack_sparse_weights(w)
        p = dict(w=wt, b=None, packed=ops.pack_bf16x3(wt), n=c, cp=cp, k2=0, act=0, taps=27)
        x = torch.randn((rows, cp), device=model.device)
        y = torch.empty((rows, c), device=model.device)
        row = dict(level=l, rows=rows, channels=c, pairs=pairs, gflop_pairs=2.0 * pairs * c * c / 1e9,
                   gflop_padded=2.0 * rows * 27 * cp * c / 1e9)
        row["hip_ms"] = timed(lambda: ops.sparse_conv(x, rule, p["packed"], c, cp=cp, out=y), reps)
        row["torch_ms"] = timed(lambda: native._torch_conv(x, rule, p, y, None, None), reps)
        row["hip_tflops_pairs"] = row["gflop_pairs"] / row["hip_ms"]
        row["hip_tflops_padded"] = row["gflop_padded"] / row["hip_ms"]
        out.append(row)
    return out


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--clouds", type=int, default=1)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--only", choices=("hip", "torch"), default=None, help="one path only (for a profiler pass)")
    ap.add_argument("--no-layers", action="store_true", help="skip the per-level convolution timings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparseconvunet: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d import ops
    from ml3d.torch.models import SparseConvUnet
    g = np.load(os.path.join(ROOT, "tests", "golden", "sparseconvunet_scannet.npz"))
    mcfg = json.loads(str(g["model_json"]))
    dev = torch.device("cuda:0")
    model = SparseConvUnet(**mcfg, device=dev)
    model.load_state_dict(scn_ref.make_state_dict(mcfg, int(g["weights_seed"]), gain=float(g["weight_gain"])))
    model.eval()
    model.packed_params()
    rooms = [scn_ref.room(200 + i, a.points, voxel_size=float(mcfg["voxel_size"]), lattice=False, origin=(100, 200, 50))
             for i in range(a.clouds)]
    host = dict(point=[torch.from_numpy(p).pin_memory() for p, _ in rooms], feat=[torch.from_numpy(f).pin_memory() for _, f in rooms])

    def step(mode):
        os.environ["ML3D_SCN_OPS"] = mode
        t0 = time.perf_counter()
        out = model(host)                                           # upload and rulebook build are part of the step
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

    pyr = model.last_pyramid
    res = dict(model="sparseconvunet_scannet", multiplier=mcfg["multiplier"], clouds_per_batch=a.clouds, points_per_cloud=a.points,
               level_rows=pyr.read_counts(), steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    for mode in modes:
        t = np.asarray(times[mode])
        half = len(t) // 2
        res[mode] = dict(median_ms=float(np.median(t)), p95_ms=float(np.percentile(t, 95)), min_ms=float(t.min()),
                         half_gap_ms=float(abs(np.median(t[:half]) - np.median(t[half:]))) if half else 0.0)
    if len(modes) == 2:
        res["speedup_hip_over_torch"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
        res["difference_ms"] = res["torch"]["median_ms"] - res["hip"]["median_ms"]
        res["drift_ms"] = max(res["hip"]["half_gap_ms"], res["torch"]["half_gap_ms"])
        res["max_abs_logit_delta"] = float((outs["hip"] - outs["torch"]).abs().max())
        res["logit_scale"] = float(outs["torch"].abs().max())
    points = torch.cat([p.to(dev) for p in host["point"]]).contiguous()
    feat = torch.cat([f.to(dev) for f in host["feat"]]).contiguous()
    splits = np.concatenate([[0], np.cumsum([len(p) for p in host["point"]])]).astype(np.int64)
    res["build_ms"] = timed(lambda: ops.scn_build(points, feat, splits), 10)
    if "hip" in res:
        res["build_share_of_hip_forward"] = res["build_ms"] / res["hip"]["median_ms"]
    if not a.no_layers:
        res["conv_levels"] = conv_levels(model, pyr)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
