#!/usr/bin/env python3
"""tests/golden/pvcnn_{small,s3dis}.npz from the REAL reference forward on PyTorch-CPU.

The reference's ``ml3d/torch/models/pvcnn.py`` is pure PyTorch apart from one call into the ``open3d`` wheel,
``trilinear_devoxelize_forward``, which it only imports when a CUDA device is present.  This script imports the reference's
own module through ``oracle.ref_shim``, sets exactly that module attribute to a torch-CPU stand-in of the contract in
include/ml3d_hip.h (tests/pvcnn_ref.py) and runs the reference's ``PVCNN`` in eval mode on seeded LATTICE rooms with
pseudo-trained weights (``pvcnn_ref.make_state_dict``); ``Voxelization.forward`` is wrapped to record what it returned.  On a
2^-6 m lattice every float32 partial sum of a coordinate is exact, so the reference's float32 mean equals the contract's
double-sum mean bit for bit; the script ASSERTS that ``pvcnn_ref.voxel_coords`` reproduces the reference's voxel coordinates
and indices bit for bit (a torch build whose ``norm`` rounds differently fails here, not in a GPU test).  It needs the
reference checkout, so it runs on the authoring machine only; the tests read the ``.npz`` files.  Nothing of the reference's
text is stored.

    python tools/gen_golden_pvcnn.py            # write both files
    python tools/gen_golden_pvcnn.py --check    # regenerate and compare every array with the committed file
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

from oracle import ref_shim  # noqa: E402
import pvcnn_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# weights_seed: each case uses the FIRST seed, counting up from `seed_start`, whose reference logits have max |logit| inside
# [5, 23] (non-trivial logits, and below 23 the project's plain 1e-4 tolerance applies); the search runs on the case's own input.
CASES = dict(
    pvcnn_small=dict(model=dict(name="PVCNN", num_classes=13, num_points=1000, extra_feature_channels=6, width_multiplier=0.5,
                                voxel_resolution_multiplier=0.375),
                     n=1000, cloud_seeds=[51, 52], seed_start=2030, logit_stride=1, full_vox=True),
    pvcnn_s3dis=dict(yaml="pvcnn_s3dis", n=40960, cloud_seeds=[61, 62, 63], seed_start=2040, logit_stride=16, full_vox=False),
)


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def run_case(name, case, known_seed=None):
    ref_shim.install()
    mod = importlib.import_module("ml3d.torch.models.pvcnn")
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), mod.__file__
    if "yaml" in case:
        from ml3d.utils import Config          # the reference's, through the shim
        cfg = Config.load_from_file(os.path.join(ref_shim.REF_ROOT, "ml3d", "configs", case["yaml"] + ".yml"))
        mcfg = plain(cfg.model)
        for k in ("ckpt_path",):
            mcfg.pop(k, None)
        if mcfg.get("augment") == "None":
            mcfg["augment"] = None
    else:
        mcfg = dict(case["model"])
    mod.trilinear_devoxelize_forward = pvcnn_ref.torch_devoxelize_forward
    recorded = []
    plain_forward = mod.Voxelization.forward

    def recording_forward(self, features, coords):
        grid, norm_coords = plain_forward(self, features, coords)
        recorded.append((int(self.r), norm_coords.detach().numpy().copy()))
        return grid, norm_coords

    mod.Voxelization.forward = recording_forward
    try:
        torch.manual_seed(0)
        model = mod.PVCNN(device="cpu", **mcfg)
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert shapes == pvcnn_ref.state_shapes(mcfg), "pvcnn_ref.state_shapes does not restate the reference's layout"
        model.eval()
        point, feat = pvcnn_ref.make_inputs(case["cloud_seeds"], case["n"])
        inputs = dict(point=torch.from_numpy(point), feat=torch.from_numpy(feat))
        seed = case["seed_start"] if known_seed is None else known_seed
        while True:
            model.load_state_dict(pvcnn_ref.make_state_dict(mcfg, seed, shapes))
            del recorded[:]
            t0 = time.time()
            with torch.no_grad():
                logits = model(inputs).numpy()
            scale = float(np.abs(logits).max())
            print("%s: reference forward on %d x %d points in %.1f s, weights seed %d, logit scale %.2f" %
                  (name, point.shape[0], point.shape[2], time.time() - t0, seed, scale))
            if 5.0 <= scale <= 23.0:
                break
            assert known_seed is None, "logit scale %.2f outside [5, 23]" % scale
            seed += 1
    finally:
        mod.Voxelization.forward = plain_forward
    B, _, N = point.shape
    assert logits.shape == (B, N, int(mcfg["num_classes"]))
    logits = logits.reshape(B * N, -1)
    # ---- the contract's restatement against what the reference computed, bit for bit ----------------------------------------
    res = sorted(set(r for r, _ in recorded))
    stats, vox = pvcnn_ref.voxel_coords(point, res)
    for r, norm_coords in recorded:
        v = np.ascontiguousarray(norm_coords.transpose(0, 2, 1)).reshape(B * N, 3)
        assert np.array_equal(v, vox[r][0]), "r = %d: the reference's voxel coordinates differ from the contract's" % r
        c = np.rint(v).astype(np.int64)
        assert np.array_equal((c[:, 0] * r + c[:, 1]) * r + c[:, 2], vox[r][1]), r
    ref_mean = inputs["point"].mean(2).numpy()
    assert np.array_equal(ref_mean, stats[:, :3]), "torch's float32 mean differs from the contract's on the lattice clouds"
    g = dict(model_json=json.dumps(mcfg), weights_seed=seed, seed_start=case["seed_start"],
             cloud_seeds=np.asarray(case["cloud_seeds"]), n=case["n"], points_sum=float(point.astype(np.float64).sum()),
             state_keys=np.asarray([k for k, _ in shapes]), state_shapes=np.asarray([json.dumps(list(s)) for _, s in shapes]),
             logit_scale=scale, logit_stride=case["logit_stride"], logits=logits[::case["logit_stride"]].astype(np.float32),
             labels=logits.argmax(1).astype(np.uint8), stats=stats, resolutions=np.asarray(res))
    for r in res:
        idx = vox[r][1].reshape(B, N)
        g["vox%d" % r] = idx.astype(np.int32) if case["full_vox"] else np.int64(pvcnn_ref.vox_checksum(idx))
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
        path = os.path.join(OUT, name + ".npz")
        # --check re-runs the committed seed (and asserts its window) instead of repeating the search
        g = run_case(name, CASES[name], known_seed=int(np.load(path)["weights_seed"]) if a.check else None)
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
            assert os.path.getsize(path) < 600 * 1024
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
