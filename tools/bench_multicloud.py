"""Model-class API throughput of RandLA-Net on SEVERAL clouds: ``RandLANet.inference_many`` (clouds in lock step, one batched
sampler call + one forward at batch A per round) at ``max_in_flight`` 1, 4 and 16 against the same clouds fed one after another
through ``inference_begin`` / ``inference_preprocess`` / forward / ``inference_end`` -- in ONE process, alternating, after a
warm-up pass of every mode, medians and the spread over the repeats (never best-of).  Prints one JSON line
(``preprocess_only``: the preprocessing of the clouds alone, which every mode's time contains).

    python tools/bench_multicloud.py [--clouds 16] [--repeats 7] [--in-flight 1,4,16] [--finish device|host]

``--finish``: the ``finish`` of every ``inference_many`` call (default: the model's own default) -- where a finished cloud's votes
become its result; ``host`` is the blocking read-back + numpy finish kept as the A/B baseline (profiles/multicloud_finish_bench.md).

Clouds: synthetic SemanticKITTI-sized sweeps (``synth_data.lidar_sweep``, the generator bench.py uses), the first ``--clouds``
seeds from 5000 on whose 0.06 m sub-cloud keeps more than num_points = 45 056 points (a smaller one would take the host path and
measure something else).  Every mode segments every cloud to completion with the same per-cloud seeds, so all modes cut exactly
the same patches; preprocessing is part of every mode's time.  On a revision without ``inference_many`` only the sequential
loop is measured (how the parent commit's number in profiles/multicloud_bench.md was taken)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth_data          # noqa: E402
import synth_weights       # noqa: E402


def make_clouds(count, num_points):
    """-> (clouds, total number of points of their sub-clouds as numpy's voxel grid counts them)"""
    clouds, seed, total = [], 5000, 0
    while len(clouds) < count:
        sweep = synth_data.lidar_sweep(seed)
        seed += 1
        n_sub = synth_data._grid_barycentre(sweep, 0.06).shape[0]
        if n_sub < num_points + num_points // 16:
            continue
        clouds.append(dict(point=sweep, feat=None, label=np.zeros(sweep.shape[0], np.int32)))
        total += n_sub
    return clouds, total


def sequential(model, clouds, seeds):
    """The single-cloud loop, cloud after cloud -> number of patches."""
    patches = 0
    for cloud, seed in zip(clouds, seeds):
        model.rng = np.random.default_rng(seed)
        model.inference_begin(dict(cloud))
        assert model._dev_loop is not None
        while True:
            inp = model.inference_preprocess()
            patches += 1
            if model.inference_end(inp, model(inp["data"])):
                break
    torch.cuda.synchronize()
    return patches


def preprocess_only(model, clouds):
    """What every mode pays per cloud before its first patch (grid subsampling, search structure, projection indices)."""
    for cloud in clouds:
        model.preprocess(dict(cloud), {"split": "test"})
    torch.cuda.synchronize()
    return 0


def many(model, clouds, seeds, in_flight, finish=None):
    count = [0]

    def on_batch(slots, inputs, logits):
        count[0] += len(slots)

    kw = {} if finish is None else {"finish": finish}
    res = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, on_batch=on_batch, **kw)
    torch.cuda.synchronize()
    assert all(r is not None for r in res)
    return count[0]


def stats(times, patches, clouds):
    t = np.asarray(times)
    return {"s_median": float(np.median(t)), "s_min": float(t.min()), "s_max": float(t.max()),
            "patches_per_s_median": float(patches / np.median(t)), "patches_per_s_min": float(patches / t.max()),
            "patches_per_s_max": float(patches / t.min()), "clouds_per_s_median": float(clouds / np.median(t)),
            "clouds_per_s_min": float(clouds / t.max()), "clouds_per_s_max": float(clouds / t.min()), "runs": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--in-flight", default="1,4,16")
    ap.add_argument("--finish", choices=("device", "host"), default=None)
    args = ap.parse_args()
    from ml3d.torch.models import RandLANet
    cfg = dict(synth_weights.RANDLANET_SEMANTICKITTI_CFG, grid_size=0.06, augment={"recenter": {"dim": [0, 1]}})
    dev = torch.device("cuda:0")
    model = RandLANet(**cfg, device=dev, seed=5)
    model.load_state_dict(synth_weights.randlanet_state_dict(cfg, 2024))
    model.eval()
    clouds, n_sub = make_clouds(args.clouds, int(cfg["num_points"]))
    seeds = list(range(900, 900 + len(clouds)))
    modes = [("sequential", None)]
    if hasattr(RandLANet, "inference_many"):
        modes += [("inference_many_%d" % int(f), int(f)) for f in args.in_flight.split(",")]
    run = lambda f: sequential(model, clouds, seeds) if f is None else \
        (preprocess_only(model, clouds) if f == "pre" else many(model, clouds, seeds, f, args.finish))
    patches = {name: run(f) for name, f in modes}                       # warm-up: every mode once, untimed
    assert len(set(patches.values())) == 1, patches                     # the same seeds cut the same patches in every mode
    modes.append(("preprocess_only", "pre"))                            # side measurement: the per-cloud share of every mode's time
    patches["preprocess_only"] = 0
    times = {name: [] for name, _ in modes}
    for _ in range(args.repeats):                                       # alternating: a drift of the machine hits every mode alike
        for name, f in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = run(f)
            times[name].append(time.perf_counter() - t0)
            assert n == patches[name]
    n = patches["sequential"]
    out = {"tool": "bench_multicloud", "clouds": len(clouds), "num_points": int(cfg["num_points"]), "patches": n,
           "sub_cloud_points_total": int(n_sub),
           "hip_graphs": bool(getattr(model, "use_graphs", False)), "repeats": args.repeats, "finish": args.finish or "default"}
    for name, _ in modes:
        out[name] = stats(times[name], n if name != "preprocess_only" else 0, len(clouds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
