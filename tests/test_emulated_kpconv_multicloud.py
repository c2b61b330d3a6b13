"""CPU: the multi-cloud KPConv sphere loop (ml3d_sphere_select, ml3d_sphere_batch, KPFCNN.inference_many) executed against the HOST
EMULATION of the HIP sources (tests/hipemu), like tests/test_emulated_multicloud.py: each case runs in its own interpreter because
tests/emu_runtime.py monkeypatches the package's device gates.  The bodies live in tests/kpconv_multicloud_cases.py (shared with
the GPU suite); the model-level runs are made ONCE, pickled, and asserted on here."""
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
import kpconv_multicloud_cases as M
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=1500,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_sphere_select_equals_fixed_radius_search_per_cloud():
    """Per cloud the indices and the count of ops.fixed_radius_search for that one query on that cloud alone; a centre on the
    isolated point gives count 1; possibilities unchanged; an inactive slot's count and the entries behind the lists untouched."""
    _run('M.check_sphere_select("cpu")\nprint("ok")\n')


def test_device_sphere_batch_equals_the_numpy_crop_bit_for_bit():
    """Points, columns, out_sel, out_row, the float64 possibilities and the in-place colour array after one and two calls against
    the numpy restatement of _crop_sphere (sequential float32 column sums), for keep x zero_extra x n_extra 0 / 3 x dims_mask
    0 / 4 / 7; one call serving all clouds equals calls serving one cloud at a time."""
    _run('M.check_device_sphere_batch("cpu")\nprint("ok")\n')


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The FIRST batch of every cloud: inference_many on the 4 clouds at max_in_flight 4 (stopped from on_batch) and the 4
    single-cloud loops, made once.  The emulator takes seconds per forward, so the runs to completion -- final
    possibilities, votes, admission and retirement, the host-loop fallbacks -- are the GPU suite's (tests/test_gpu_kpconv_multicloud.py,
    the same clouds and seeds), and the network here has a quarter of the widths (M.EMU_CFG)."""
    out = str(tmp_path_factory.mktemp("kpconv_multicloud") / "runs.pkl")
    _run(r'''
clouds = M.model_clouds()
singles = {i: M.run_single(M.EMU_CFG, "cpu", c, s, max_batches=1) for i, (c, s) in enumerate(zip(clouds, M.SEEDS))}
runs = {S: M.collect(M.EMU_CFG, "cpu", clouds, M.SEEDS, S, max_batches=1) for S in (4,)}
pickle.dump(dict(singles=singles, runs=runs), open(%r, "wb"))
print("ok")
''' % out)
    return pickle.load(open(out, "rb"))


@pytest.mark.parametrize("in_flight", [4])
def test_first_batches_of_inference_many_are_the_single_cloud_loops(runs, in_flight):
    """Every batch a cloud made in lock step (out_sel, point bits, column bits, labels, the neighbour / pool / upsample matrices of
    its spheres) equals the batch of the same ordinal of its single-cloud loop; logits within the KPFCNN tolerance."""
    import kpconv_multicloud_cases as M
    run = runs["runs"][in_flight]
    assert max(len(b) for b in run["batches"]) == in_flight and len(run["recs"]) >= in_flight
    assert all(len(v) >= 1 for v in run["recs"].values())
    M.assert_many_is_single(run, runs["singles"], partial=True)
    M.assert_logits_within_tolerance(run, runs["singles"])
    assert run["stats"]["read_backs"] == run["stats"]["sub_rounds"]


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call (the hipcc-built library, no GPU)."""
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
    assert L.ml3d_sphere_select_workspace_bytes(-1, 2) == 0 and L.ml3d_sphere_batch_workspace_bytes(2, -1) == 0
    assert L.ml3d_sphere_select_workspace_bytes(800, 2) > 800 * 12

    def select(pts=p, s=sp, n=3, a=ap, na=2, ci=p, r=1.0, oi=p, cap=800, oc=p, ws=p, wsb=big):
        return L.ml3d_sphere_select(pts, s, n, a, na, ci, r, oi, cap, oc, ws, wsb, None)
    for name in ("pts", "s", "a", "ci", "oi", "oc", "ws"):
        assert select(**{name: None}) == INVALID, name
    assert select(r=-1.0) == INVALID and select(r=float("nan")) == INVALID and select(cap=799) == INVALID
    assert select(na=0) == INVALID and select(n=257) == INVALID and select(wsb=64) == WORKSPACE
    bad = np.array([0, 300, 100, 1000], np.int64)
    assert select(s=bad.ctypes.data) == INVALID
    offs = np.array([0, 50], np.int64)
    n_a = np.array([50, 60], np.int32)
    m_a = np.array([-1, 20], np.int32)
    zero = np.zeros(2, np.int32)

    def batch(pts=p, poss=p, s=sp, n=3, a=ap, na=2, ci=p, cand=p, off=offs.ctypes.data, cnt=n_a.ctypes.data, perm=p, keep=None,
              m=None, z=zero.ctypes.data, mask=7, extra=None, ne=0, op=p, oc=p, os_=p, orow=p, ws=p, wsb=big):
        return L.ml3d_sphere_batch(pts, poss, s, n, a, na, ci, cand, off, cnt, perm, keep, m, z, mask, extra, ne, 0.0, 255.0, 1, op, oc,
                                   os_, orow, ws, wsb, None)
    for name in ("pts", "poss", "s", "a", "ci", "cand", "off", "cnt", "perm", "z", "op", "oc", "os_", "orow", "ws"):
        assert batch(**{name: None}) == INVALID, name
    assert batch(mask=8) == INVALID and batch(ne=3) == INVALID and batch(ne=-1) == INVALID and batch(keep=p) == INVALID
    too_many = np.array([101, 60], np.int32)                            # more candidates than cloud 0 has points
    assert batch(cnt=too_many.ctypes.data) == INVALID
    cut = np.array([-1, 61], np.int32)                                  # a cut larger than the sphere
    assert batch(keep=p, m=cut.ctypes.data) == INVALID
    assert batch(keep=p, m=m_a.ctypes.data, wsb=64) == WORKSPACE and batch(wsb=64) == WORKSPACE
