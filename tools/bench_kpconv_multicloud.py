"""Model-class API throughput of KPFCNN on SEVERAL clouds: ``KPFCNN.inference_many`` (clouds in lock step: one batched radius
query + one batched crop per sub-round, one forward over all clouds' batches) at ``max_in_flight`` 1, 4 and 8 against the same
clouds fed one after another through ``inference_begin`` / ``inference_preprocess`` / forward / ``inference_end`` under
``np.random.seed`` -- in ONE process, alternating, after a warm-up pass of every mode, medians and the spread over the repeats
(never best-of).  Prints one JSON line and, with ``--markdown FILE``, writes the table of profiles/kpconv_multicloud_bench.md.

    python tools/bench_kpconv_multicloud.py [--clouds 8] [--repeats 5] [--in-flight 1,4,8] [--small] [--half 7.0] [--markdown FILE]
                                            [--finish device|host]

``--finish``: the ``finish`` of every ``inference_many`` call (default: the model's own default) -- where a finished cloud's votes
become its result; ``host`` is the blocking read-back + numpy finish kept as the A/B baseline (profiles/multicloud_finish_bench.md).

Clouds: synthetic Toronto3D-shaped tiles (``synth_data.toronto3d_tile``) at the sizes of kpconv_toronto3d.yml (0.08 m grid, 4 m
spheres, batches of 5 000 .. 10 000 points; ``--small``: the tests' sizes, 0.12 m grid, 1 m spheres, batches of 600 .. 800).
Every mode segments every cloud to completion with the same per-cloud seeds, so all
modes cut exactly the same spheres; preprocessing is part of every mode's time."""
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

CFG = dict(synth_weights.TORONTO3D_CFG, min_in_points=5000, augment_color=1, augment_noise=0.0001, augment_rotation="vertical",
           augment_scale_anisotropic=False, augment_scale_max=1.1, augment_scale_min=0.9, augment_symmetries=[True, False, False],
           t_normalize=dict(method="linear", normalize_points=False, feat_bias=0, feat_scale=255))


def sequential(model, clouds, seeds):
    """The single-cloud loop, cloud after cloud -> (spheres, batches)."""
    spheres = batches = 0
    for cloud, seed in zip(clouds, seeds):
        np.random.seed(seed)
        model.inference_begin(dict(cloud))
        while True:
            inp = model.inference_preprocess()
            batches += 1
            spheres += len(inp["data"].lengths[0])
            if model.inference_end(inp, model(inp["data"])):
                break
    torch.cuda.synchronize()
    return spheres, batches


def many(model, clouds, seeds, in_flight, finish=None):
    count = [0, 0]

    def on_batch(spheres, batch, logits):
        count[0] += len(spheres)
        count[1] += 1

    kw = {} if finish is None else {"finish": finish}
    res = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, on_batch=on_batch, **kw)
    torch.cuda.synchronize()
    assert all(r is not None for r in res)
    return count[0], count[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--in-flight", default="1,4,8")
    ap.add_argument("--half", type=float, default=7.0)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--finish", choices=("device", "host"), default=None)
    ap.add_argument("--small", action="store_true", help="0.12 m grid, 1 m spheres, batches of 600 .. 800 points (the tests' sizes)")
    args = ap.parse_args()
    from ml3d.torch.models.kpconv import KPFCNN
    if args.small:
        CFG.update(first_subsampling_dl=0.12, in_radius=1.0, min_in_points=600, max_in_points=800, batch_limit=800)
    dev = torch.device("cuda:0")
    model = KPFCNN(**CFG, device=dev)
    model.load_state_dict(synth_weights.kpconv_state_dict(CFG, 2024))
    model.eval()
    clouds = []
    for i in range(args.clouds):
        t = synth_data.toronto3d_tile(700 + i, half=args.half, density=0.25)
        clouds.append(dict(point=t["point"], feat=t["feat"], label=t["label"]))
    seeds = list(range(900, 900 + len(clouds)))
    modes = [("sequential", None)]
    if hasattr(KPFCNN, "inference_many"):
        modes += [("inference_many_%d" % int(f), int(f)) for f in args.in_flight.split(",")]
    run = lambda f: sequential(model, clouds, seeds) if f is None else many(model, clouds, seeds, f, args.finish)
    counts = {name: run(f) for name, f in modes}                        # warm-up: every mode once, untimed
    assert len({c[0] for c in counts.values()}) == 1, counts            # the same seeds cut the same spheres in every mode
    times = {name: [] for name, _ in modes}
    extra = {name: {} for name, _ in modes}
    for _ in range(args.repeats):                                       # alternating: a drift of the machine hits every mode alike
        for name, f in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = run(f)
            times[name].append(time.perf_counter() - t0)
            assert n == counts[name]
            if f is not None:
                extra[name] = dict(model.inference_many_stats)
    n = counts["sequential"][0]
    out = {"tool": "bench_kpconv_multicloud", "clouds": len(clouds), "spheres": n, "repeats": args.repeats,
           "raw_points_total": int(sum(len(c["point"]) for c in clouds)), "finish": args.finish or "default"}
    for name, _ in modes:
        t = np.asarray(times[name])
        out[name] = {"s_median": float(np.median(t)), "s_min": float(t.min()), "s_max": float(t.max()),
                     "spheres_per_s_median": float(n / np.median(t)), "spheres_per_s_min": float(n / t.max()),
                     "spheres_per_s_max": float(n / t.min()), "forwards": counts[name][1], "runs": int(t.size)}
        if extra[name]:
            out[name].update(read_backs=extra[name]["read_backs"], sub_rounds=extra[name]["sub_rounds"],
                             host_draw_share=float(extra[name]["host_draw_seconds"] / t[-1]))
    print(json.dumps(out))
    if args.markdown:
        base = out["sequential"]["spheres_per_s_median"]
        rows = ["| mode | spheres/s (median, min .. max of %d runs) | vs sequential | forwards | sampler read-backs | host draws, share of the time |" % args.repeats,
                "|---|---|---|---|---|---|"]
        for name, _ in modes:
            r = out[name]
            rows.append("| %s | %.0f (%.0f .. %.0f) | %.2fx | %d | %s | %s |" % (
                name, r["spheres_per_s_median"], r["spheres_per_s_min"], r["spheres_per_s_max"], r["spheres_per_s_median"] / base,
                r["forwards"], r.get("read_backs", "one ragged list per sphere + retries"),
                "%.1f %%" % (100 * r["host_draw_share"]) if "host_draw_share" in r else "(the whole crop is host work)"))
        with open(args.markdown, "w") as f:
            head = ("# KPFCNN on several clouds: `inference_many` against the sequential single-cloud loop\n\n"
                    "`python tools/bench_kpconv_multicloud.py --clouds %d --repeats %d%s --half %g`, one process on one MI355X, modes "
                    "alternating after a warm-up pass of each; %d synthetic Toronto3D-shaped tiles (%d raw points in all), %.2f m grid, "
                    "%.1f m spheres, batches of %d .. %d points, every mode cutting the same %d spheres with the same seeds.\n\n")
            f.write(head % (len(clouds), args.repeats, " --small" if args.small else "", args.half, len(clouds), out["raw_points_total"],
                            CFG["first_subsampling_dl"], CFG["in_radius"], CFG["min_in_points"], CFG["max_in_points"], n))
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
