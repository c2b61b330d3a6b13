"""Evaluation runs through ``inference_many``: what scoring every finished cloud against ground truth costs, three ways, in ONE
process, alternating, after a warm-up pass of every mode -- medians and the spread over the repeats, never best-of:

  plain   ``inference_many(finish="device")`` and nothing else (the default path; runs on a revision without ``evaluate`` too)
  a       ``plain`` + the scoring a user writes today: the label table and ``np.bincount`` on the returned labels, per cloud
  b       ``inference_many(finish="device", evaluate=True)``
  c       ``inference_many(finish="device", evaluate=True, return_scores=False)``

    python tools/bench_multicloud_eval.py [--model randla|kpconv] [--clouds N] [--repeats 7] [--in-flight F] [--plain-only]
                                          [--kernel] [--ab-lib OTHER_BUILD.so]

``--model randla``: the 16 synthetic sweeps at 16 in flight of tools/bench_multicloud.py (profiles/multicloud_finish_bench.md);
``--model kpconv``: the 8 small tiles at 8 in flight of ``tools/bench_kpconv_multicloud.py --small --half 2.5``
(profiles/kpconv_multicloud_bench.md).  The ground truth is drawn per raw point from [0, C], so ignored points occur.  Modes a, b
and c must produce the same matrices (asserted).  ``--plain-only`` measures ``plain`` alone: how the parent revision's number is
taken.  ``--kernel``: ``ml3d_vote_confusion`` alone at a sweep's sizes (75 000 x 19 votes, 130 000 indices), 100 calls back to back
between two events, median (min - max) of 7, for a matrix that is mostly diagonal and for uniformly random ground truth;
``--ab-lib``: the same from a second build of the library (``-DML3D_CONFUSION_WAVE_MERGE=1``), whose results must be equal.
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth_data          # noqa: E402
import synth_weights       # noqa: E402


def user_lut(num_classes, ignored):
    """What a user writes today: the reference's table with -1 at the ignored values."""
    table = list(range(num_classes))
    for i in ignored:
        if i >= 0:
            table = table[:i] + [0] + table[i:]
    table = np.asarray(table, np.int64)
    table[[i for i in ignored if 0 <= i < table.size]] = -1
    return table


def user_scoring(results, clouds, lut, C):
    total = np.zeros((C, C), np.int64)
    for r, c in zip(results, clouds):
        row = lut[c["label"]]
        ok = row >= 0
        total += np.bincount(C * row[ok] + r["predict_labels"][ok], minlength=C * C).reshape(C, C)
    return total


def setup(args):
    dev = torch.device("cuda:0")
    if args.model == "randla":
        import bench_multicloud as B
        from ml3d.torch.models import RandLANet
        cfg = dict(synth_weights.RANDLANET_SEMANTICKITTI_CFG, grid_size=0.06, augment={"recenter": {"dim": [0, 1]}})
        model = RandLANet(**cfg, device=dev, seed=5)
        model.load_state_dict(synth_weights.randlanet_state_dict(cfg, 2024))
        clouds, _ = B.make_clouds(args.clouds or 16, int(cfg["num_points"]))
        in_flight = args.in_flight or 16
    else:
        import bench_kpconv_multicloud as K
        from ml3d.torch.models.kpconv import KPFCNN
        K.CFG.update(first_subsampling_dl=0.12, in_radius=1.0, min_in_points=600, max_in_points=800, batch_limit=800)
        model = KPFCNN(**K.CFG, device=dev)
        model.load_state_dict(synth_weights.kpconv_state_dict(K.CFG, 2024))
        clouds = []
        for i in range(args.clouds or 8):
            t = synth_data.toronto3d_tile(700 + i, half=2.5, density=0.25)
            clouds.append(dict(point=t["point"], feat=t["feat"], label=t["label"]))
        in_flight = args.in_flight or 8
    model.eval()
    C = int(model.cfg.num_classes)
    g = np.random.default_rng(77)
    for c in clouds:
        c["label"] = g.integers(0, C + 1, size=len(c["point"])).astype(np.int32)
    return model, clouds, list(range(900, 900 + len(clouds))), in_flight, C


def kernel_times(ab_lib):
    """µs per ``ml3d_vote_confusion`` call, per build and ground-truth distribution: {build: {distribution: [median, min, max]}}."""
    from ml3d import _abi
    dev = torch.device("cuda:0")
    n_sub, n_full, C = 75000, 130000, 19
    g = np.random.default_rng(3)
    votes = g.random((n_sub, C)).astype(np.float16)
    proj = np.sort(g.integers(0, n_sub, size=n_full)).astype(np.int32)
    pred = np.argmax(votes, 1)[proj]
    lut = user_lut(C, [0]).astype(np.int32)
    diagonal = (pred + 1).astype(np.int32)                       # the value whose row is the prediction ...
    off = g.random(n_full) < 0.1
    diagonal[off] = g.integers(0, C + 1, size=int(off.sum()))    # ... but for a tenth of the points
    gts = {"mostly_diagonal": diagonal, "uniform": g.integers(0, C + 1, size=n_full).astype(np.int32)}
    libs = {"default_build": _abi.get()}
    if ab_lib:
        libs["ab_build"] = _abi.bind(ctypes.CDLL(ab_lib))
    d_votes, d_proj, d_lut = torch.from_numpy(votes).to(dev), torch.from_numpy(proj).to(dev), torch.from_numpy(lut).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for build, lib in libs.items():
        out[build] = {}
        for name, gt in gts.items():
            d_gt = torch.from_numpy(gt).to(dev)
            both = torch.zeros(C * C + 3, dtype=torch.int64, device=dev)
            labels = torch.empty(n_full, dtype=torch.uint8, device=dev)
            call = lambda: lib.ml3d_vote_confusion(d_votes.data_ptr(), n_sub, C, d_proj.data_ptr(), n_full, d_gt.data_ptr(), d_lut.data_ptr(),
                                                   int(d_lut.numel()), both.data_ptr(), both.data_ptr() + 8 * C * C, labels.data_ptr(), stream)
            assert call() == 0
            row = lut[gt].astype(np.int64)
            ok = row >= 0
            want = np.bincount(C * row[ok] + pred[ok], minlength=C * C)
            got = both.cpu().numpy()
            assert np.array_equal(got[:C * C], want) and got[C * C:].tolist() == [int(ok.sum()), int((~ok).sum()), 0], (build, name)
            assert np.array_equal(labels.cpu().numpy(), pred.astype(np.uint8)), (build, name)
            times = []
            for _ in range(9):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(100):
                    call()
                t1.record()
                t1.synchronize()
                times.append(t0.elapsed_time(t1) * 10.0)          # ms per 100 calls -> µs per call
            t = np.asarray(times[2:])
            out[build][name] = [float(np.median(t)), float(t.min()), float(t.max())]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("randla", "kpconv"), default="randla")
    ap.add_argument("--clouds", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--in-flight", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--ab-lib", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_multicloud_eval", "model": args.model, "repeats": args.repeats}
    if args.kernel:
        out["kernel_us"] = kernel_times(args.ab_lib)
        print(json.dumps(out))
        return
    model, clouds, seeds, in_flight, C = setup(args)
    lut = user_lut(C, list(model.cfg.ignored_label_inds))
    units = [0]

    def on_batch(slots, inputs, logits):
        units[0] += len(slots)

    def run(mode):
        units[0] = 0
        kw = {"b": dict(evaluate=True), "c": dict(evaluate=True, return_scores=False)}.get(mode, {})
        res = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, on_batch=on_batch, finish="device", **kw)
        conf = None
        if mode == "a":
            conf = user_scoring(res, clouds, lut, C)
        elif mode in ("b", "c"):
            conf = model.inference_many_metric.confusion_matrix
        torch.cuda.synchronize()
        return units[0], conf

    modes = ["plain"] if args.plain_only else ["plain", "a", "b", "c"]
    warm = {m: run(m) for m in modes}
    assert len({w[0] for w in warm.values()}) == 1, "every mode must cut the same patches"
    if not args.plain_only:
        assert np.array_equal(warm["a"][1], warm["b"][1]) and np.array_equal(warm["a"][1], warm["c"][1]), "the three scorings differ"
        out["scored_points"] = int(warm["a"][1].sum())
    times = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(m)
            times[m].append(time.perf_counter() - t0)
    n = warm["plain"][0]
    out.update(clouds=len(clouds), in_flight=in_flight, units=n, raw_points=int(sum(len(c["point"]) for c in clouds)))
    for m in modes:
        t = np.asarray(times[m])
        out[m] = {"units_per_s_median": float(n / np.median(t)), "units_per_s_min": float(n / t.max()), "units_per_s_max": float(n / t.min()),
                  "s_median": float(np.median(t))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
