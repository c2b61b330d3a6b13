"""Time of one ``ops.randla_knn_pyramid`` call (grid build + search, tile order of the two finest levels as the engine asks) by batch
size and by cloud size, on the library in the tree: the measurement behind knn.hip's GRID_PYRAMID_MIN_BATCH / GRID_PYRAMID_MAX_N0.
Run it once per build (the launch chain: -DML3D_GRID_PYRAMID_FUSED=0; the one-workgroup-per-cloud builder without limits:
-DML3D_GRID_PYRAMID_MIN_BATCH=1 -DML3D_GRID_PYRAMID_MAX_N0=268435456) and compare the tables; the search is the same launch on the
same grids in both, so the difference of two rows is the difference of the builds.
usage: python tools/pyramid_build_sweep.py <label>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd")):
    sys.path.insert(0, p)
import synth_data  # noqa: E402
from ml3d import ops  # noqa: E402

RATIOS, K = [4, 4, 4, 4], 16


def one(frames, B, reps=9, warm=3):
    n0 = frames.shape[1]
    pts = frames[torch.arange(B) % frames.shape[0]].contiguous()
    n = [n0]
    for r in RATIOS:
        n.append(n[-1] // r)
    order = [torch.empty(B * n[l], dtype=torch.int32, device=pts.device) if l < 2 else None for l in range(len(RATIOS))]
    out = ops.randla_knn_pyramid(pts, RATIOS, K, tile_order=order)
    ts = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.randla_knn_pyramid(pts, RATIOS, K, out=out, tile_order=order)
        b.record()
        b.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "tree"
    dev = torch.device("cuda:0")
    frames = {}
    for n0 in (16384, 45056, 65536, 98304, 131072):
        frames[n0] = torch.from_numpy(np.stack([synth_data.semantickitti_patch(i, n0) for i in range(4)])).to(dev)
    for B in (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 192, 256, 384):
        print("%s batch %4d n0 %6d  %.3f ms" % (label, B, 45056, one(frames[45056], B)), flush=True)
    for n0 in (16384, 65536, 98304, 131072):
        for B in (128, 256):
            print("%s batch %4d n0 %6d  %.3f ms" % (label, B, n0, one(frames[n0], B)), flush=True)


if __name__ == "__main__":
    main()
