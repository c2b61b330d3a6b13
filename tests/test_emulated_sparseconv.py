"""CPU: csrc/sparseconv.hip and the rulebook loader of csrc/gemm.hip through the HOST EMULATION (tests/hipemu), reached the way
tests/test_emulated_pvcnn.py reaches its kernels: each case runs in its own interpreter with tests/emu_runtime.py installed, so
the product's own Python wrappers (``ml3d.ops.sparseconv``, the ``SparseConvUnet`` class) drive the emulated kernels.

* ``ml3d_scn_build`` ARRAY-EQUAL to the dictionary-lookup restatement (tests/scn_ref.py) on the edge batch of the GPU test and on
  a one-item cloud whose deepest level is a single row;
* ``ml3d_sparse_conv_bf16x3`` against the float64 direct formula, <= 1e-5 at outputs of order 1 (derivation: the header of
  tests/test_gpu_sparseconv.py);
* the whole ``sparseconvunet_small`` forward against the reference's golden: level sizes exact, logits within
  ``max(1e-4, 4.4e-6 * logit_scale)`` (the rule of tests/test_gpu_configs.py), and the torch formulation within the same."""
import os
import subprocess
import sys

import pytest

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys, json
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch
import emu_runtime
emu_runtime.install("ml3d")
import scn_ref
from ml3d import ops, _abi
def t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype))
def check_pyramid(pts, feat, rs):
    ref = scn_ref.build(pts, feat, rs)
    pyr = ops.scn_build(t(pts), t(feat), rs)
    assert pyr.read_counts() == ref["counts"].tolist(), (pyr.read_counts(), ref["counts"])
    assert np.array_equal(pyr.index_map.numpy(), ref["index_map"])
    assert np.array_equal(pyr.feat0[:, :3].numpy(), ref["feat0"]) and not pyr.feat0[:, 3:].any()
    for l in range(7):
        assert np.array_equal(pyr.coords(l).numpy(), ref["coords"][l]), l
        assert np.array_equal(pyr.nbr27(l).numpy(), ref["nbr27"][l]), l
        if l >= 1:
            assert np.array_equal(pyr.child8(l).numpy(), ref["child8"][l]), l
        if l < 6:
            assert np.array_equal(pyr.parent(l).numpy(), ref["parent"][l]), l
            assert np.array_equal(pyr.ptap(l).numpy(), ref["ptap"][l]), l
            assert np.array_equal(pyr.up8(l).numpy(), ref["up8"][l]), l
    return ref, pyr
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=1500,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_build_array_equal_and_conv_against_the_direct_formula():
    _run(r'''
ref, pyr = check_pyramid(*scn_ref.edge_batch())
dref, _ = check_pyramid(*scn_ref.deep_cloud())
assert dref["counts"][-1] == 1
# a point outside the grid is dropped (index_map -1), never aliased onto another voxel
pts, feat, rs = scn_ref.edge_batch()
pts = pts.copy(); pts[5] = (4096.5, 3.5, 3.5); pts[6] = (-0.5, 3.5, 3.5)
r2, p2 = check_pyramid(pts, feat, rs)
assert r2["index_map"][5] == -1 and r2["index_map"][6] == -1
# refused on the host, before any kernel
L = _abi.get()
assert L.ml3d_scn_build(None, None, 0, 3, 10, None, 1, 7, 4096, None, None, None, None, None, None, None, None, None, 0, None, 0, None) == -1
assert L.ml3d_sparse_conv_bf16x3(None, 0, 0, 32, None, 27, 10, None, 0, 0, None, 32, None, None, 0, 0, 0.0, None, 32, None) == -1
rng = np.random.default_rng(0)
m0, m1 = int(ref["counts"][0]), int(ref["counts"][1])
for cin, cout, taps in ((32, 32, 27), (96, 64, 27), (64, 96, 8), (16, 48, 27)):
    rule_ref, rule = (ref["nbr27"][0], pyr.nbr27(0)) if taps == 27 else (ref["child8"][1], pyr.child8(1))
    x = rng.uniform(-1, 1, (m0, cin)).astype(np.float32)
    w = (rng.uniform(-1, 1, (taps, cin, cout)) * np.sqrt(3.0 / (0.25 * taps * cin))).astype(np.float32)
    wt, _, cp, _ = ops.pack_sparse_weights(t(w))
    xp = torch.zeros((m0, cp)); xp[:, :cin] = t(x)
    out = ops.sparse_conv(xp, rule.contiguous(), ops.pack_bf16x3(wt), cout, cp=cp).numpy()
    want = scn_ref.conv_direct(x, rule_ref, w)
    err = np.abs(out - want).max()
    assert 0.5 < np.abs(want).max() < 8 and err <= 1e-5 * max(1.0, np.abs(want).max()), (cin, cout, taps, err)
# transposed, into a column slice; bias + residual + ReLU; the dense second block
y = rng.uniform(-1, 1, (m1, 64)).astype(np.float32)
w = (rng.uniform(-1, 1, (8, 64, 32)) * np.sqrt(3.0 / 64)).astype(np.float32)
wt, _, cp, _ = ops.pack_sparse_weights(t(w))
join = torch.full((m0, 64), 7.0)
ops.sparse_conv(t(y), pyr.up8(0).contiguous(), ops.pack_bf16x3(wt), 32, cp=cp, out=join[:, 32:])
want = np.stack([y[ref["parent"][0][i]].astype(np.float64) @ w[ref["ptap"][0][i]].astype(np.float64) for i in range(m0)])
assert (join[:, :32] == 7.0).all() and np.abs(join[:, 32:].numpy() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
x = rng.uniform(-1, 1, (m0, 32)).astype(np.float32); x2 = rng.uniform(-1, 1, (m0, 64)).astype(np.float32)
res = rng.uniform(-1, 1, (m0, 32)).astype(np.float32); bias = rng.uniform(-1, 1, 32).astype(np.float32)
w3 = (rng.uniform(-1, 1, (27, 32, 32)) * np.sqrt(3.0 / (0.25 * 27 * 32))).astype(np.float32)
w2 = (rng.uniform(-1, 1, (64, 32)) * np.sqrt(3.0 / 64)).astype(np.float32)
rule = pyr.nbr27(0).contiguous()
wt, _, cp, _ = ops.pack_sparse_weights(t(w3))
out = ops.sparse_conv(t(x), rule, ops.pack_bf16x3(wt), 32, cp=cp, bias=t(bias), residual=t(res), act=2).numpy()
want = scn_ref.conv_direct(x, ref["nbr27"][0], w3, bias=bias, residual=res, relu=True)
assert np.abs(out - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
wt, _, cp, k2 = ops.pack_sparse_weights(t(w3), extra=t(w2))
out = ops.sparse_conv(t(x), rule, ops.pack_bf16x3(wt), 32, cp=cp, a2=t(x2), k2=k2).numpy()
want = scn_ref.conv_direct(x, ref["nbr27"][0], w3, x2=x2, w2=w2)
assert np.abs(out - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
s, b = rng.normal(size=32).astype(np.float32), rng.normal(size=32).astype(np.float32)
assert np.array_equal(ops.scn_bn_relu(t(x), t(s), t(b)).numpy(), np.maximum(x * s + b, 0))
''')


def test_small_golden_forward():
    _run(r'''
from ml3d.torch.models import SparseConvUnet
g = np.load(os.path.join(ROOT, "tests", "golden", "sparseconvunet_small.npz"))
mcfg = json.loads(str(g["model_json"]))
m = SparseConvUnet(**mcfg, device="cpu")
m.load_state_dict(scn_ref.make_state_dict(mcfg, int(g["weights_seed"]), gain=float(g["weight_gain"])))
pts, fts = scn_ref.golden_inputs(g["clouds"], float(g["room_voxel_size"]))
assert abs(np.concatenate(pts).astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
inp = dict(point=[t(p) for p in pts], feat=[t(f) for f in fts])
tol = max(1e-4, 4.4e-6 * float(g["logit_scale"]))
out = m(inp).numpy()
assert m.last_pyramid.read_counts() == g["level_counts"].tolist()
err = np.abs(out - g["logits"]).max()
print("native (emulated): max |d logit| = %.3g, tolerance %.3g" % (err, tol))
assert out.shape == g["logits"].shape and err <= tol, err
os.environ["ML3D_SCN_OPS"] = "torch"
err = np.abs(m(inp).numpy() - g["logits"]).max()
assert err <= tol, err
''')
