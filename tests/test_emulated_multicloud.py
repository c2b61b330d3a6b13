"""CPU: the multi-cloud patch loop (ml3d_possibility_argmin, ml3d_patch_batch, RandLANet.inference_many) executed against the HOST
EMULATION of the HIP sources (tests/hipemu), like tests/test_emulated_api.py: each case runs in its own interpreter because
tests/emu_runtime.py monkeypatches the package's device gates.  The bodies live in tests/multicloud_cases.py (shared with the
GPU suite); the runs of tests 3 and 4 are made ONCE, pickled, and asserted on here."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys, pickle
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import emu_runtime
emu_runtime.install("ml3d")
import multicloud_cases as M
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=900,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_possibility_argmin_matches_numpy_per_segment():
    """Test 1: first index of the minimum and the minimum per cloud, segments off wave and tile boundaries, repeated minima (also
    across tiles), a minimum at the last element, an inactive slot between active ones left untouched."""
    _run('M.check_possibility_argmin("cpu")\nprint("ok")\n')


def test_device_patch_batch_equals_the_single_cloud_ops_per_cloud():
    """Test 2: out_sel / out_pts / out_feats / the possibilities bit-equal to nearest_to_center + device_patch per cloud, out_row ==
    out_sel + split; clouds of k, k + 1 and ~3k points, one with duplicated points, dims_mask 0 / 3 / 7, with and without extra
    features, an inactive cloud whose possibilities do not change."""
    _run('M.check_device_patch_batch("cpu")\nprint("ok")\n')


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """inference_many on 4 clouds at max_in_flight 2 and 1, and the 4 single-cloud runs, made once."""
    out = str(tmp_path_factory.mktemp("multicloud") / "runs.pkl")
    _run(r'''
in_ch, aug = M.AUGMENTS[1]
cfg = dict(M.SMALL, in_channels=in_ch, augment=aug, grid_size=M.SMALL_GRID)
clouds, seeds = M.small_clouds()
clouds = M.with_features(clouds, in_ch)
two = M.collect(cfg, "cpu", clouds, seeds, 2)
one = M.collect(cfg, "cpu", clouds, seeds, 1, batch_one=False)
singles = {i: M.run_single(cfg, "cpu", c, s) for i, (c, s) in enumerate(zip(clouds, seeds))}
pickle.dump(dict(two=two, one=one, singles=singles), open(%r, "wb"))
print("ok")
''' % out)
    return pickle.load(open(out, "rb"))


def test_inference_many_reproduces_four_single_cloud_runs(runs):
    """Test 3: 4 clouds, max_in_flight = 2 (admission; the active set shrinks at the end) against RandLANet(seed=seeds[i]) runs:
    per cloud and patch point_inds / coords[0] / features / labels / every neighbor_indices[l], interp_idx[l] array-equal, the
    number of patches and the final possibilities equal; votes = the recorded logits replayed through update_probs, float16
    array-equal, predict_labels = their argmax under proj_inds; every logits row within 1e-4 of the patch forwarded at batch 1."""
    import multicloud_cases as M
    two = runs["two"]
    sizes = [len(b) for b in two["batches"]]
    assert max(sizes) == 2 and sizes[-1] == 1, sizes                     # full batches, and a tail with one cloud left
    first = {c: min(r for r, b in enumerate(two["batches"]) if c in b) for c in range(4)}
    assert first[0] == first[1] == 0 and first[2] > 0 and first[3] > first[2], first      # clouds 2 and 3 were admitted later
    assert all(r is not None for r in two["results"])
    M.assert_many_is_single(two, runs["singles"])
    for i in range(4):
        assert len(two["batch_one"][i]) == len(two["patches"][i]) > 0


def test_max_in_flight_one_gives_the_same_results(runs):
    """Test 4: the degenerate case of the same code: one cloud in flight, every admission rebuilds the buffers."""
    import multicloud_cases as M
    one = runs["one"]
    assert all(len(b) == 1 for b in one["batches"])
    assert [b[0] for b in one["batches"]] == sorted(b[0] for b in one["batches"])      # cloud after cloud, in input order
    M.assert_many_is_single(one, runs["singles"])
    M.assert_same_run(one, runs["two"])
    # at batch 1 the forward is the single-cloud loop's forward: here even the results are the single runs'
    for i, (res1, *_rest) in runs["singles"].items():
        assert np.array_equal(one["results"][i]["predict_labels"], res1["predict_labels"])
        assert np.array_equal(one["results"][i]["predict_scores"].view(np.uint16), res1["predict_scores"].view(np.uint16))


def test_a_cloud_smaller_than_num_points_takes_the_host_path():
    """Test 5: a cloud with fewer than num_points points after preprocessing is served by the single-cloud host loop, after the
    batched ones, with its generator: its result is the single-cloud run's, and results come back in input order."""
    _run(r'''
in_ch, aug = M.AUGMENTS[0]
cfg = dict(M.SMALL, in_channels=in_ch, augment=aug, grid_size=M.SMALL_GRID)
clouds, seeds = M.small_clouds()
clouds = M.with_features([clouds[2], M.tile_small(), clouds[0]], in_ch)
seeds = [7, 8, 9]
run = M.collect(cfg, "cpu", clouds, seeds, 2, batch_one=False)
assert sorted(run["patches"]) == [0, 2], sorted(run["patches"])          # cloud 1 never entered a batch
singles = {i: M.run_single(cfg, "cpu", c, s) for i, (c, s) in enumerate(zip(clouds, seeds))}
res1, got1, poss1, votes1, proj = singles[1]
assert len(poss1) < cfg["num_points"] and len(clouds[1]["point"]) == len(proj)
got = run["results"][1]
assert np.array_equal(got["predict_labels"], res1["predict_labels"])
assert np.array_equal(got["predict_scores"].view(np.uint16), res1["predict_scores"].view(np.uint16))
assert run["info"][1]["num_patches"] == len(got1) and np.array_equal(run["info"][1]["possibility"], poss1)
M.assert_many_is_single(run, singles)
for i, c in enumerate(clouds):                                            # input order
    assert run["results"][i]["predict_labels"].shape == (len(c["point"]),)
print("ok")
''')


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Test 6: argument validation happens before any HIP call (the hipcc-built library, no GPU): null pointers, k larger than a
    cloud, a workspace too small, non-monotone splits -> the ML3D_E_* code."""
    import __graft_entry__ as ge
    from ml3d import _abi
    ge.build()
    L = _abi.get()
    INVALID, WORKSPACE = -1, -2
    splits = np.array([0, 100, 300, 1000], np.int64)
    act = np.array([0, 2], np.int32)
    p = C.c_void_p(256)                      # a non-null "device pointer": never followed, every call below fails validation first
    sp, ap = splits.ctypes.data, act.ctypes.data
    big = 1 << 30
    assert L.ml3d_possibility_argmin_workspace_bytes(-1, 3) == 0 and L.ml3d_patch_batch_workspace_bytes(10, -1, 5) == 0
    assert L.ml3d_possibility_argmin_workspace_bytes(800, 2) > 0
    argmin = lambda poss=p, s=sp, n=3, a=ap, na=2, oi=p, om=p, ws=p, wsb=big: \
        L.ml3d_possibility_argmin(poss, s, n, a, na, oi, om, ws, wsb, None)
    assert argmin(poss=None) == INVALID and argmin(s=None) == INVALID and argmin(a=None) == INVALID
    assert argmin(oi=None) == INVALID and argmin(om=None) == INVALID and argmin(ws=None) == INVALID
    assert argmin(wsb=64) == WORKSPACE
    assert argmin(na=0) == INVALID and argmin(na=4) == INVALID and argmin(n=0) == INVALID and argmin(n=257) == INVALID
    bad = np.array([0, 300, 100, 1000], np.int64)                       # non-monotone splits
    assert argmin(s=bad.ctypes.data) == INVALID
    off = np.array([5, 100, 300, 1000], np.int64)                       # splits[0] != 0
    assert argmin(s=off.ctypes.data) == INVALID
    for slots in ([2, 0], [0, 0], [0, 3], [-1, 2]):                     # unsorted / repeated / out of range
        a = np.array(slots, np.int32)
        assert argmin(a=a.ctypes.data) == INVALID, slots
    empty = np.array([0, 0, 300, 1000], np.int64)                       # an empty ACTIVE cloud
    assert argmin(s=empty.ctypes.data) == INVALID

    def patch(pts=p, poss=p, s=sp, n=3, a=ap, na=2, ci=p, perm=p, k=100, mask=3, extra=None, ne=0, op=p, of=p, os_=p, orow=p, ws=p,
              wsb=big):
        return L.ml3d_patch_batch(pts, poss, s, n, a, na, ci, perm, k, mask, extra, ne, 0.0, 1.0, op, of, os_, orow, ws, wsb, None)
    for name in ("pts", "poss", "s", "a", "ci", "perm", "op", "of", "os_", "orow", "ws"):
        assert patch(**{name: None}) == INVALID, name
    assert patch(k=101) == INVALID                                      # k larger than cloud 0 (100 points)
    assert patch(k=0) == INVALID and patch(mask=8) == INVALID and patch(ne=3) == INVALID and patch(ne=-1) == INVALID
    assert patch(s=bad.ctypes.data) == INVALID
    assert patch(wsb=L.ml3d_patch_batch_workspace_bytes(800, 2, 100) - 1) == WORKSPACE
    assert patch(wsb=64) == WORKSPACE
