"""CPU: csrc/pvcnn.hip and the 3-D loader of csrc/gemm.hip through the HOST EMULATION (tests/hipemu), reached the way
tests/test_emulated_pointtransformer.py reaches its kernels: each case runs in its own interpreter with tests/emu_runtime.py
installed, so the product's own Python wrappers (``ml3d.ops.pvcnn``, the ``PVCNN`` class) drive the emulated kernels.

* the voxel coordinates: EXACT against the numpy restatement of the contract (tests/pvcnn_ref.py) on a lattice room, on a
  real-valued cloud and on constructed edge cases (a point at the maximum norm, v exactly integral, v exactly k + 0.5 decided
  by half-to-even, all points coincident);
* scatter-mean, 3 x 3 x 3 convolution, trilinear gather and column maximum against direct formulas, <= 1e-5 (the sums have at
  most 27 * 32 = 864 terms of order 1 / sqrt(864) each: float32 rounding of the reference formula itself is ~1e-6);
* the whole ``pvcnn_small`` forward against the reference's golden: ``stats`` and voxel indices exact, logits within
  ``max(1e-4, 4.4e-6 * logit_scale)`` (the rule of tests/test_gpu_configs.py)."""
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
import pt_ref, pvcnn_ref
from ml3d import ops, _abi
def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))
def check_coords(coords, res):
    stats, vox = ops.pvcnn_voxel_coords(f32(coords), res)
    rstats, rvox = pvcnn_ref.voxel_coords(coords, res)
    assert stats.dtype == torch.float32 and np.array_equal(stats.numpy(), rstats), (stats.numpy(), rstats)
    for r in res:
        v, idx = vox[r]
        assert idx.dtype == torch.int32 and np.array_equal(v.numpy(), rvox[r][0]), r
        assert np.array_equal(idx.numpy(), rvox[r][1]), (r, int(np.argmax(idx.numpy() != rvox[r][1])))
    return stats.numpy(), {r: (vox[r][0].numpy(), vox[r][1].numpy()) for r in res}
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=1500,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_voxel_coords_exact_on_a_lattice_room_and_a_real_valued_cloud():
    _run(r'''
lat = np.stack([pvcnn_ref.lattice_room(s, 3000).T for s in (1, 2)])
stats, _ = check_coords(lat, [12, 6, 64])
# on the lattice the float32 mean of torch-CPU equals the contract's double-sum mean bit for bit
assert np.array_equal(torch.from_numpy(lat).mean(2).numpy(), stats[:, :3])
real = np.stack([pvcnn_ref.real_room(s, 2500).T + np.float32([[12.25], [-7.5], [1.5]]) for s in (3, 4, 5)])
check_coords(real, [5, 32])
check_coords(real[:1, :, :1], [7])               # one point: it is its own mean
''')


def test_voxel_coords_edge_cases():
    _run(r'''
# mean exactly 0 (every point with its mirror image), maximum norm 64 at (+-64, 0, 0): scale = 128 + 1e-6 = 128 in float32, so
# at r = 8 v = x / 16 + 4 exactly
half = np.float32([[64, 0, 0], [8, 24, 16], [0, 40, -8], [-56, 0, 8], [16, -16, 16]])
pts = np.concatenate([half, -half]).T[None]
stats, vox = check_coords(pts, [8])
assert stats.tolist() == [[0.0, 0.0, 0.0, 128.0]]
v, idx = vox[8]
want_v = np.float32([[7, 4, 4], [4.5, 5.5, 5], [4, 6.5, 3.5], [0.5, 4, 4.5], [5, 3, 5],
                     [0, 4, 4], [3.5, 2.5, 3], [4, 1.5, 4.5], [7, 4, 3.5], [3, 5, 3]])          # (8.0 and 7.5 clamp to 7)
want_c = np.int32([[7, 4, 4], [4, 6, 5], [4, 6, 4], [0, 4, 4], [5, 3, 5],
                   [0, 4, 4], [4, 2, 3], [4, 2, 4], [7, 4, 4], [3, 5, 3]])                       # halves go to the EVEN cell
assert np.array_equal(v, want_v), v
assert np.array_equal(idx, (want_c[:, 0] * 8 + want_c[:, 1]) * 8 + want_c[:, 2]), idx
# all points coincident: d = 0, scale = 1e-6, v = r / 2 on every axis; r = 5 -> 2.5 -> cell 2
same = np.tile(np.float32([[1.5], [-2.0], [0.25]]), (1, 200))[None]
stats, vox = check_coords(same, [5, 6])
assert stats[0, 3] == np.float32(1e-6) and (vox[5][0] == 2.5).all() and (vox[5][1] == 62).all() and (vox[6][1] == 129).all()
# refused on the host, before any kernel
L = _abi.get()
assert L.ml3d_pvcnn_voxel_coords(None, 1, 10, None, 0, None, None, None, None) == -1
assert L.ml3d_avg_voxelize(None, 0, 0, None, 0, 0, 0, None, 0, None, 0, None) == -1
assert L.ml3d_conv3d_ndhwc_bf16x3(None, 1, 4, 4, 4, 32, None, None, 1, 0.1, 32, None, 32, None) == -1
assert L.ml3d_trilinear_devoxelize(None, 0, 0, 0, None, 0, 0, None, 0, None, 0, None) == -1
assert L.ml3d_segment_max_rows(None, 0, 0, 0, 0, None, 0, None, 0, None) == -1
x = torch.zeros((2, 4, 4, 4, 9))
w, b, cp = ops.pack_conv3d_weights(torch.zeros((32, 9, 3, 3, 3)))
try:
    ops.conv3d_ndhwc(x, ops.pack_bf16x3(w), b, 32)          # 9 channels were not padded to 32
    raise SystemExit("an unpadded 9-channel volume was accepted")
except RuntimeError as e:
    assert "multiple of 32" in str(e)
''')


@pytest.mark.parametrize("r,cin,cout", [(6, 9, 32), (12, 32, 32), (5, 32, 64)])
def test_ops_against_the_direct_formulas(r, cin, cout):
    _run(r'''
r, cin, cout = %d, %d, %d
B, N = 2, 1000
rng = np.random.default_rng(100 * r + cin)
coords = np.stack([pvcnn_ref.real_room(s, N).T for s in (6, 7)])
stats, vox = ops.pvcnn_voxel_coords(f32(coords), [r])
v, idx = vox[r]
cp = (cin + 31) // 32 * 32
# (b) scatter-mean of a column slice of a wider buffer, zero-padded to cp channels; twice: the same bits
wide = f32(rng.standard_normal((B * N, cin + 8)))
feat = wide[:, 4:4 + cin]
grid = ops.avg_voxelize(feat, idx, B, r, out_channels=cp)
ref = pvcnn_ref.avg_voxelize(feat.numpy(), idx.numpy(), B, r, out_channels=cp)
err = float(np.abs(grid.numpy() - ref).max())
print("avg_voxelize r=%%d c=%%d: max|d| = %%.3g, equal to the serial sum: %%s" %% (r, cin, err, np.array_equal(grid.numpy(), ref)))
assert grid.shape == (B, r, r, r, cp) and err <= 1e-5 and torch.equal(grid, ops.avg_voxelize(feat, idx, B, r, out_channels=cp))
assert (grid[..., cin:] == 0).all() and int((ref != 0).any(-1).sum()) == len(np.unique(idx.numpy().astype(np.int64) + np.repeat([0, r ** 3], N)))
# (c) the convolution with a folded BatchNorm3d(eps = 1e-4), bias and LeakyReLU(0.1) against float64 conv3d
w5 = torch.from_numpy(rng.uniform(-1, 1, (cout, cin, 3, 3, 3)) * 2.0 / np.sqrt(27 * cin))
cb = torch.from_numpy(rng.uniform(-1, 1, cout) / np.sqrt(27 * cin))
gamma = torch.from_numpy(rng.uniform(0.6, 1.5, cout) * np.where(rng.random(cout) < 0.2, -1, 1))
beta, mean, var = (torch.from_numpy(a) for a in (rng.normal(0, 0.2, cout), rng.normal(0, 0.2, cout), rng.uniform(0.5, 1.5, cout)))
scale = gamma / torch.sqrt(var + 1e-4)
w, bias, cp2 = ops.pack_conv3d_weights(w5, scale, beta - mean * scale, cb)
assert cp2 == cp and w.shape == (27 * cp, cout)
out = ops.conv3d_ndhwc(grid, ops.pack_bf16x3(w), bias, cout, act=1, slope=0.1)
x64 = grid[..., :cin].double().permute(0, 4, 1, 2, 3)
y = torch.nn.functional.conv3d(x64, w5, cb, padding=1)
y = (y - mean.view(1, -1, 1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1, 1) + 1e-4) * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)
y = torch.nn.functional.leaky_relu(y, 0.1).permute(0, 2, 3, 4, 1)
err = float((out.double() - y).abs().max())
print("conv3d r=%%d %%d -> %%d: max|d| = %%.3g at |ref| <= %%.3g" %% (r, cin, cout, err, float(y.abs().max())))
assert out.shape == (B, r, r, r, cout) and err <= 1e-5, err
# (d) the trilinear gather into a column slice, with the addend aliasing the output
buf = f32(rng.standard_normal((B * N, cout + 16)))
sl = buf[:, 8:8 + cout]
ref = pvcnn_ref.devoxelize(out.numpy(), v.numpy(), addend=sl.numpy().copy())
keep = buf.clone()
got = ops.trilinear_devoxelize(out, v, addend=sl, out=sl)
err = float(np.abs(sl.numpy() - ref).max())
print("devoxelize r=%%d c=%%d: max|d| = %%.3g" %% (r, cout, err))
assert got.data_ptr() == sl.data_ptr() and err <= 1e-5, err
assert torch.equal(buf[:, :8], keep[:, :8]) and torch.equal(buf[:, 8 + cout:], keep[:, 8 + cout:])
plain = ops.trilinear_devoxelize(out, v)
assert float(np.abs(plain.numpy() - pvcnn_ref.devoxelize(out.numpy(), v.numpy())).max()) <= 1e-5
# points on cell corners and at r - 1: the value IS the corner's
cv = f32([[0, 0, 0], [r - 1, r - 1, r - 1], [1, 2, r - 1], [r - 1, 0, 3]] * (B // 2) + [[2, 2, 2], [0, r - 1, 0], [3, 1, 0], [1, 1, 1]] * (B // 2))
got = ops.trilinear_devoxelize(out, cv)
for i, (a, b_, c) in enumerate(cv.long().tolist()):
    assert torch.equal(got[i], out[i // 4, a, b_, c]), i
# (e) the per-item column maximum of a column slice
mx = ops.segment_max_rows(sl, B)
assert torch.equal(mx, sl.reshape(B, N, cout).max(1)[0])
''' % (r, cin, cout))


def test_small_model_forward_against_the_reference_golden():
    out = _run(r'''
from ml3d.torch.models import PVCNN
g = np.load(os.path.join(ROOT, "tests", "golden", "pvcnn_small.npz"))
mcfg = json.loads(str(g["model_json"]))
m = PVCNN(**mcfg, device="cpu")
sd = m.state_dict()
assert list(sd) == [str(k) for k in g["state_keys"]]
assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g["state_shapes"]]
assert [(k, tuple(v.shape)) for k, v in sd.items()] == pvcnn_ref.state_shapes(mcfg)
m.load_state_dict(pvcnn_ref.make_state_dict(mcfg, int(g["weights_seed"])))
point, feat = pvcnn_ref.make_inputs(g["cloud_seeds"], int(g["n"]))
assert abs(point.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
inp = dict(point=torch.from_numpy(point), feat=torch.from_numpy(feat))
out = m(inp)
B, N = point.shape[0], point.shape[2]
assert out.shape == (B, N, 13)
out = out.reshape(B * N, 13).numpy()
assert np.array_equal(m.last_voxels["stats"].numpy(), g["stats"])
for r in g["resolutions"]:
    assert np.array_equal(m.last_voxels["vox"][int(r)].numpy(), g["vox%%d" %% r]), r
tol = max(1e-4, 4.4e-6 * float(g["logit_scale"]))
err = float(np.abs(out - g["logits"]).max())
print("small forward: max|dlogit| = %%.3g (tol %%.3g), logit scale %%.2f, labels differing %%d" %%
      (err, tol, float(g["logit_scale"]), int((out.argmax(1) != g["labels"]).sum())))
assert err <= tol, err
# the torch formulation (the A/B baseline) on the same voxel coordinates: the same result within the same rule
os.environ["ML3D_PVCNN_OPS"] = "torch"
alt = m(inp).reshape(B * N, 13).numpy()
err = float(np.abs(alt - g["logits"]).max())
print("torch formulation: max|dlogit| = %%.3g" %% err)
assert err <= tol, err
m.train()
try:
    m(inp)
    raise SystemExit("a forward in training mode was accepted")
except NotImplementedError:
    pass
''' % ())
    assert "small forward" in out
