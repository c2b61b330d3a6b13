#!/usr/bin/env python3
"""tests/golden/pointtransformer_{small,s3dis}.npz from the REAL reference forward on PyTorch-CPU.

The reference's ``ml3d/torch/models/point_transformer.py`` is pure PyTorch apart from two calls into the ``open3d`` wheel:
``knn_batch`` (k-NN) and ``furthest_point_sample_v2`` (FPS).  This script imports the reference's own module through
``oracle.ref_shim``, replaces exactly those two module attributes by CPU stand-ins (the oracle's batched k-NN; the numpy
restatement of the FPS contract in tests/pt_ref.py) and runs the reference's ``PointTransformer`` in eval mode on seeded
synthetic rooms with pseudo-trained weights (``pt_ref.make_state_dict``).  It needs the reference checkout, so it runs on
the authoring machine only; the tests read the ``.npz`` files.  Nothing of the reference's text is stored.

    python tools/gen_golden_pointtransformer.py            # write both files
    python tools/gen_golden_pointtransformer.py --check    # regenerate and compare every array with the committed file
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

from oracle import ops as oops  # noqa: E402
from oracle import ref_shim  # noqa: E402
import pt_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# weights_seed: with pt_ref.make_state_dict's recipe the largest |logit| of the reference varies between about 3 and 13 from seed
# to seed; each case uses the FIRST seed, counting up from 2025 (small) / 2026 (s3dis), whose logits fall inside the [5, 23]
# window asserted below (non-trivial logits, and below 23 the project's plain 1e-4 tolerance applies).
CASES = dict(
    pointtransformer_small=dict(model=dict(name="PointTransformer", blocks=[2, 2, 2, 2, 2], in_channels=6, num_classes=13,
                                           voxel_size=0.04, max_voxels=50000),
                                sizes=[6000, 4096], cloud_seeds=[11, 12], weights_seed=2026, logit_stride=1),
    pointtransformer_s3dis=dict(yaml="pointtransformer_s3dis", sizes=[50000, 33000, 4096], cloud_seeds=[21, 22, 23],
                                weights_seed=2028, logit_stride=8),
)


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


class _Batch:
    pass


def run_case(name, case):
    ref_shim.install()
    mod = importlib.import_module("ml3d.torch.models.point_transformer")
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), mod.__file__
    if "yaml" in case:
        from ml3d.utils import Config          # the reference's, through the shim
        cfg = Config.load_from_file(os.path.join(ref_shim.REF_ROOT, "ml3d", "configs", case["yaml"] + ".yml"))
        mcfg = plain(cfg.model)
    else:
        mcfg = dict(case["model"])
    searches, samplings = [], []

    def knn_batch(points, queries, k, points_row_splits, queries_row_splits, return_distances=True):
        idx, d2 = oops.knn_search_batched(points.detach().numpy(), points_row_splits.numpy(), queries.detach().numpy(),
                                          queries_row_splits.numpy(), int(k))
        searches.append((int(points.shape[0]), int(queries.shape[0]), int(k), pt_ref.knn_checksum(idx)))
        idx = torch.from_numpy(idx.astype(np.int64)).reshape(-1, k)
        return (idx, torch.from_numpy(d2).reshape(-1, k)) if return_distances else idx

    def fps_v2(point, row_splits, new_row_splits):
        idx = pt_ref.fps(point.detach().numpy(), row_splits.numpy(), new_row_splits.numpy())
        samplings.append(idx)
        return torch.from_numpy(idx)

    mod.knn_batch, mod.furthest_point_sample_v2 = knn_batch, fps_v2
    torch.manual_seed(0)
    model = mod.PointTransformer(**mcfg)
    ref_sd = model.state_dict()
    shapes = [(k, tuple(v.shape)) for k, v in ref_sd.items()]
    assert shapes == pt_ref.state_shapes(mcfg), "pt_ref.state_shapes does not restate the reference's layout"
    model.load_state_dict(pt_ref.make_state_dict(mcfg, case["weights_seed"], shapes))
    model.eval()
    pts, feat, rs = pt_ref.make_batch_arrays(case["cloud_seeds"], case["sizes"])
    b = _Batch()
    b.point, b.feat, b.row_splits = torch.from_numpy(pts), torch.from_numpy(feat), torch.from_numpy(rs)
    t0 = time.time()
    with torch.no_grad():
        logits = model(b).numpy()
    print("%s: reference forward on %d points in %.1f s, %d k-NN searches" % (name, len(pts), time.time() - t0, len(searches)))
    scale = float(np.abs(logits).max())
    assert 5.0 <= scale <= 23.0, "logit scale %.2f outside [5, 23]" % scale
    level_n = [int(r[-1]) for r in pt_ref.level_row_splits(rs)]
    nsample = (8, 16, 16, 16, 16)
    g = dict(model_json=json.dumps(mcfg), weights_seed=case["weights_seed"], cloud_seeds=np.asarray(case["cloud_seeds"]),
             sizes=np.asarray(case["sizes"]), points_sum=float(pts.astype(np.float64).sum()),
             state_keys=np.asarray([k for k, _ in shapes]), state_shapes=np.asarray([json.dumps(list(s)) for _, s in shapes]),
             logit_scale=scale, logit_stride=case["logit_stride"], logits=logits[::case["logit_stride"]].astype(np.float32),
             labels=logits.argmax(1).astype(np.uint8), n_searches=len(searches))
    assert len(samplings) == 4
    for l, idx in enumerate(samplings):
        g["fps%d" % (l + 1)] = idx.astype(np.int32)

    def checksum(n_p, n_q, k):
        hits = {c for (a, b_, kk, c) in searches if (a, b_, kk) == (n_p, n_q, k)}
        assert len(hits) == 1, (n_p, n_q, k, hits)          # every repeat of a search gave the same neighbours
        return hits.pop()
    for l in range(5):
        g["knn_self%d" % l] = checksum(level_n[l], level_n[l], nsample[l])
    for l in range(1, 5):
        g["knn_down%d" % l] = checksum(level_n[l - 1], level_n[l], nsample[l])
    for l in range(4):
        g["knn_up%d" % l] = checksum(level_n[l + 1], level_n[l], 3)
    srt = np.sort(logits, 1)
    g["min_margin"] = float((srt[:, -1] - srt[:, -2]).min())
    return g


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing")
    ap.add_argument("names", nargs="*", default=list(CASES))
    a = ap.parse_args(argv)
    bad = 0
    for name in a.names:
        g = run_case(name, CASES[name])
        path = os.path.join(OUT, name + ".npz")
        if a.check:
            old = np.load(path)
            for k, v in g.items():
                if k not in old.files or not np.array_equal(np.asarray(v), old[k]):
                    print("%s: %s DIFFERS" % (name, k))
                    bad += 1
            print("%s: %s" % (name, "every array equal" if not bad else "differences found"))
        else:
            np.savez_compressed(path, **g)
            print("%s: wrote %s (%.0f KB), logit scale %.2f, smallest top-1/top-2 margin %.2e" %
                  (name, path, os.path.getsize(path) / 1024, g["logit_scale"], g["min_margin"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
