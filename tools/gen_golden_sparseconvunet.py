#!/usr/bin/env python3
"""tests/golden/sparseconvunet_{small,scannet}.npz from the REAL reference forward on PyTorch-CPU.

The reference's ``ml3d/torch/models/sparseconvnet.py`` is pure PyTorch apart from four names it takes from the ``open3d``
wheel: ``SparseConv``, ``SparseConvTranspose``, ``voxelize`` and ``reduce_subarrays_sum``.  The wheel is not available to this
project, so their semantics are the UNPINNED contract of include/ml3d_hip.h.  This script imports the reference's own module
through ``oracle.ref_shim``, sets exactly those four module attributes to the torch-CPU stand-ins of tests/scn_ref.py (which
work on arbitrary positions by dictionary lookup), ASSERTS that the reference's ``state_dict`` layout equals
``scn_ref.state_shapes`` and runs the reference's ``SparseConvUnet`` in eval mode on seeded synthetic rooms (colours on a 2^-6
lattice: the voxel means are exact in any summation order) with pseudo-trained weights (``scn_ref.make_state_dict``).  It needs
the reference checkout, so it runs on the authoring machine only; the tests read the ``.npz`` files.  Nothing of the
reference's text is stored: arrays and the model configuration only.

    python tools/gen_golden_sparseconvunet.py            # write both files
    python tools/gen_golden_sparseconvunet.py --check    # regenerate and compare every array with the committed file
"""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

from oracle import ref_shim  # noqa: E402
import scn_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# gain: the weight scale of scn_ref.make_state_dict (the deep residual configuration grows faster per layer);
# weights_seed: the FIRST seed, counting up from `seed_start`, whose reference logits have max |logit| inside [5, 23]
CASES = dict(
    sparseconvunet_small=dict(model=dict(name="SparseConvUnet", multiplier=16, voxel_size=0.05, conv_block_reps=2,
                                         residual_blocks=False, in_channels=3, num_classes=20, grid_size=4096),
                              clouds=[(71, 2600), (72, 1500)], voxel_size=0.2, seed_start=3030, logit_stride=1, gain=2.0),
    sparseconvunet_scannet=dict(yaml="sparseconvunet_scannet", clouds=[(81, 40000)], voxel_size=0.05, seed_start=3040,
                                logit_stride=8, gain=1.6),
)


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def make_inputs(case):
    return scn_ref.golden_inputs(case["clouds"], case["voxel_size"])


def run_case(name, case, known_seed=None):
    ref_shim.install()
    mod = importlib.import_module("ml3d.torch.models.sparseconvnet")
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(ref_shim.REF_ROOT)), mod.__file__
    if "yaml" in case:
        from ml3d.utils import Config          # the reference's, through the shim
        cfg = Config.load_from_file(os.path.join(ref_shim.REF_ROOT, "ml3d", "configs", case["yaml"] + ".yml"))
        mcfg = plain(cfg.model)
        mcfg.pop("ckpt_path", None)
    else:
        mcfg = dict(case["model"])
    mod.SparseConv, mod.SparseConvTranspose = scn_ref.SparseConv, scn_ref.SparseConvTranspose
    mod.voxelize, mod.reduce_subarrays_sum = scn_ref.voxelize, scn_ref.reduce_subarrays_sum
    torch.manual_seed(0)
    model = mod.SparseConvUnet(device="cpu", **mcfg)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert shapes == scn_ref.state_shapes(mcfg), "scn_ref.state_shapes does not restate the reference's layout"
    model.eval()
    pts, fts = make_inputs(case)
    inputs = types.SimpleNamespace(point=[torch.from_numpy(p) for p in pts], feat=[torch.from_numpy(f) for f in fts],
                                   batch_lengths=[len(p) for p in pts])
    seed = case["seed_start"] if known_seed is None else known_seed
    while True:
        model.load_state_dict(scn_ref.make_state_dict(mcfg, seed, shapes, gain=case['gain']))
        t0 = time.time()
        with torch.no_grad():
            logits = model(inputs).numpy()
        scale = float(np.abs(logits).max())
        print("%s: reference forward on %s points in %.1f s, weights seed %d, logit scale %.2f" %
              (name, [len(p) for p in pts], time.time() - t0, seed, scale))
        if 5.0 <= scale <= 23.0:
            break
        assert known_seed is None, "logit scale %.2f outside [5, 23]" % scale
        seed += 1
    n = sum(len(p) for p in pts)
    assert logits.shape == (n, int(mcfg["num_classes"]))
    splits = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    pyr = scn_ref.build(np.concatenate(pts), np.concatenate(fts), splits)
    srt = np.sort(logits, 1)
    return dict(model_json=json.dumps(mcfg), weights_seed=seed, seed_start=case["seed_start"],
                clouds=np.asarray(case["clouds"]), weight_gain=case["gain"], room_voxel_size=case["voxel_size"],
                points_sum=float(np.concatenate(pts).astype(np.float64).sum()),
                state_keys=np.asarray([k for k, _ in shapes]), state_shapes=np.asarray([json.dumps(list(s)) for _, s in shapes]),
                logit_scale=scale, logit_stride=case["logit_stride"], logits=logits[::case["logit_stride"]].astype(np.float32),
                labels=logits.argmax(1).astype(np.uint8), margins=(srt[:, -1] - srt[:, -2]).astype(np.float16),
                min_margin=float((srt[:, -1] - srt[:, -2]).min()), level_counts=pyr["counts"])


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing")
    ap.add_argument("names", nargs="*", default=list(CASES))
    a = ap.parse_args(argv)
    bad = 0
    for name in a.names:
        path = os.path.join(OUT, name + ".npz")
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
            print("%s: wrote %s (%.0f KB), logit scale %.2f, smallest top-1/top-2 margin %.2e, level sizes %s" %
                  (name, path, os.path.getsize(path) / 1024, g["logit_scale"], g["min_margin"], g["level_counts"].tolist()))
            assert os.path.getsize(path) < 600 * 1024
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
