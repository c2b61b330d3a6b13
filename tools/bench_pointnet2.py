#!/usr/bin/env python3
"""PointNet++ MSG backbone inference on the MI355X: the native HIP path against the torch formulation
(``ML3D_PN2_OPS=torch``) of the same commit, on the SAME native FPS / ball-query / 3-NN indices, alternating in one process.

The model is ``rpn.backbone`` of pointrcnn_kitti.yml (read from tests/golden/pointnet2_kitti.npz, which stores it) with the
golden's pseudo-trained weights; a step is one forward of B clouds of 16 384 points already on the device, device synchronise
before the clock stops.  For B = 1 and B = 4 it reports median / p95 ms per forward for both paths and their ratio, the share of
every op of the HIP forward (HIP events around each call of one instrumented forward: the sum also counts the gaps between
kernels of an op) and, for every fused set-abstraction shape of the model, the kernel alone with its achieved fraction of the
f32 matrix peak it runs on (2 * rows * (c1 * c2p + c2p * c3) operations as executed, 157.3 TFLOP/s).

    python tools/bench_pointnet2.py --steps 30 --warmup 3 --out profiles/pointnet2_bench.md
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

import pn2_ref  # noqa: E402

F32_MATRIX_PEAK_TFLOPS = 157.3


def op_shares(model, pc):
    """One HIP forward with HIP events around every op call -> {op: ms}."""
    from ml3d import ops
    from ml3d.ops import pointnet2 as pn2_ops
    spans, saved = [], []

    def wrap(mod, name, tag):
        fn = getattr(mod, name)
        saved.append((mod, name, fn))

        def timed(*a, **k):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = fn(*a, **k)
            t1.record()
            spans.append((tag, t0, t1))
            return r
        setattr(mod, name, timed)

    wrap(ops, "furthest_point_sampling", "fps")
    wrap(ops, "linear", "linear (first SA layer per source point, FP MLPs)")
    wrap(pn2_ops, "ball_query", "ball_query")
    wrap(pn2_ops, "pn2_sa_mlp_max", "sa_mlp_max (fused and unfused scales)")
    wrap(pn2_ops, "three_nn", "three_nn")
    wrap(pn2_ops, "pn2_interpolate", "interpolate")
    try:
        os.environ["ML3D_PN2_OPS"] = "hip"
        model(pc)
        torch.cuda.synchronize()
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)
    out = {}
    for tag, t0, t1 in spans:
        out[tag] = out.get(tag, 0.0) + t0.elapsed_time(t1)
    return out


def sa_kernels(model, batch, n0, reps=20):
    """Every fused set-abstraction shape of the model alone, at the model's own row counts."""
    from ml3d.ops import pointnet2 as pn2_ops
    P, rows_out, n = model.packed_params(), [], n0
    dev = model.device
    for sa, p in zip(model.SA_modules, P["sa"]):
        m = sa.npoint
        for s, sc in enumerate(p["scales"]):
            c1, c2, c3 = sc["hip"]["widths"]
            ns = sa.nsamples[s]
            row = dict(batch=batch, n=n, m=m, nsample=ns, widths=[c1, c2, c3], fused=bool(sc["hip"]["fused"]))
            y = torch.randn((batch * n, c1), device=dev)
            xyz, ctr = torch.rand((batch, n, 3), device=dev), torch.rand((batch, m, 3), device=dev)
            idx = torch.randint(0, n, (batch, m, ns), dtype=torch.int32, device=dev)
            fn = lambda: pn2_ops.pn2_sa_mlp_max(y, xyz, ctr, idx, sc["hip"])       # noqa: E731
            for _ in range(3):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / reps
            c2p = (c2 + 31) // 32 * 32 if row["fused"] else c2
            gflop = 2.0 * batch * m * ns * (c1 * c2p + c2p * c3) / 1e9
            row.update(ms=ms, gflop=gflop, tflops=gflop / ms, fraction_of_f32_matrix_peak=gflop / ms / F32_MATRIX_PEAK_TFLOPS)
            rows_out.append(row)
        n = m
    return rows_out


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--out", default=None, help="markdown file for the table (the JSON line goes to stdout)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet2: needs an MI355X (no CPU fallback, no CPU timing)")
    from ml3d.torch.modules import Pointnet2MSG
    g = np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_kitti.npz"))
    mcfg = json.loads(str(g["model_json"]))
    dev = torch.device("cuda:0")
    model = Pointnet2MSG(**mcfg, device=dev)
    keys, shapes = [str(k) for k in g["state_keys"]], [json.loads(str(s)) for s in g["state_shapes"]]
    model.load_state_dict(pn2_ref.make_state_dict(keys, shapes, int(g["weights_seed"])))
    n0 = int(g["n"])
    res = dict(model="pointrcnn_kitti rpn.backbone", points_per_cloud=n0, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), runs=[])
    for batch in a.batches:
        pc = torch.from_numpy(pn2_ref.make_pointcloud(range(100, 100 + batch), n0, int(mcfg["in_channels"]), float(g["cloud_scale"]),
                                                      g["cloud_offset"])).to(dev)

        def step(mode):
            os.environ["ML3D_PN2_OPS"] = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model(pc)[1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        outs, times = {}, dict(hip=[], torch=[])
        for _ in range(a.warmup):
            for mode in times:
                outs[mode] = step(mode)[1]
        for _ in range(a.steps):
            for mode in times:                                      # alternating: both paths see the same box at the same time
                times[mode].append(step(mode)[0])
        run = dict(batch=batch)
        for mode, t in times.items():
            t = np.asarray(t)
            half = len(t) // 2
            run[mode] = dict(median_ms=float(np.median(t)), p95_ms=float(np.percentile(t, 95)), min_ms=float(t.min()),
                             half_gap_ms=float(abs(np.median(t[:half]) - np.median(t[half:]))) if half else 0.0)
        run["torch_over_hip"] = run["torch"]["median_ms"] / run["hip"]["median_ms"]
        run["max_abs_feature_delta"] = float((outs["hip"] - outs["torch"]).abs().max())
        run["feature_scale"] = float(outs["torch"].abs().max())
        run["op_ms"] = op_shares(model, pc)
        run["sa_kernels"] = sa_kernels(model, batch, n0)
        res["runs"].append(run)
    os.environ.pop("ML3D_PN2_OPS", None)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(markdown(res))
    return 0


def markdown(res):
    L = ["# PointNet++ MSG backbone (pointrcnn_kitti.yml `rpn.backbone`): HIP path against the torch path of the same commit", "",
         "Written by `tools/bench_pointnet2.py --steps %d --warmup %d` on %s; %d points per cloud, clouds already on the device, "
         "both paths alternate in one process on the same native FPS / ball-query / 3-NN indices." %
         (res["steps"], res["warmup"], res["device"], res["points_per_cloud"]), "",
         "| B | hip median ms | hip p95 ms | torch median ms | torch p95 ms | torch / hip | drift ms (hip, torch) | max abs feature delta (scale) |",
         "|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        L.append("| %d | %.3f | %.3f | %.3f | %.3f | %.2f | %.3f, %.3f | %.2e (%.1f) |" %
                 (r["batch"], r["hip"]["median_ms"], r["hip"]["p95_ms"], r["torch"]["median_ms"], r["torch"]["p95_ms"],
                  r["torch_over_hip"], r["hip"]["half_gap_ms"], r["torch"]["half_gap_ms"], r["max_abs_feature_delta"], r["feature_scale"]))
    for r in res["runs"]:
        total = sum(r["op_ms"].values())
        L += ["", "## B = %d: share of each op in one instrumented HIP forward (HIP events around every call, %.3f ms in all)" % (r["batch"], total),
              "", "| op | ms | share |", "|---|---|---|"]
        for k, v in sorted(r["op_ms"].items(), key=lambda kv: -kv[1]):
            L.append("| %s | %.3f | %.0f %% |" % (k, v, 100.0 * v / total))
        L += ["", "## B = %d: each set-abstraction scale alone (20 back-to-back calls)" % r["batch"], "",
              "| source points | centres | nsample | widths | route | ms | GFLOP as executed | TFLOP/s | fraction of the f32 matrix peak (157.3) |",
              "|---|---|---|---|---|---|---|---|---|"]
        for k in r["sa_kernels"]:
            L.append("| %d | %d | %d | %s | %s | %.4f | %.3f | %.2f | %s |" %
                     (k["n"], k["m"], k["nsample"], "-".join(map(str, k["widths"])), "fused" if k["fused"] else "unfused", k["ms"],
                      k["gflop"], k["tflops"], ("%.1f %%" % (100 * k["fraction_of_f32_matrix_peak"])) if k["fused"] else "n/a (three kernels)"))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
