"""CPU: csrc/ptransformer.hip through the HOST EMULATION (tests/hipemu), reached the way ``KPFCNN(..., device="cpu")`` is in
tests/test_emulated_api.py: each case runs in its own interpreter with tests/emu_runtime.py installed, so the product's own
Python wrappers (``ml3d.ops.pointtransformer``, the ``PointTransformer`` class) drive the emulated kernels.

* furthest point sampling: EXACT against the numpy restatement of the contract (tests/pt_ref.py), including an exact float32
  tie between the two best candidates and the edge cases;
* the fused attention, TransitionDown and interpolation kernels against direct torch-CPU formulas, <= 1e-5;
* the whole ``pointtransformer_small`` forward against the reference's logits, <= 1e-4, FPS / k-NN indices exact, and the
  state-dict layout equal to the reference's;
* the bodies of tests/pt_cases.py that tests/test_gpu_pointtransformer_ops.py runs on the MI355X, here for every case of at
  most 1025 points (and the furthest-point-sampling cases, which are cheap at any size): floats against the float64 formula
  within max(1e-5, 4 e32), everything else for equality.  This run is where those bodies themselves get debugged."""
import os
import subprocess
import sys

import pytest

import emu
import pt_cases as C      # (the shape tables only: the bodies run in the subprocess)

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
import pt_ref, synth_data
from ml3d import ops, _abi
'''


def _run(body):
    emu.lib()
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body], capture_output=True, text=True, timeout=1500,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_fps_matches_the_contract_on_a_room():
    _run(r'''
pts = pt_ref.room(1, 4096)
out = ops.furthest_point_sampling(torch.from_numpy(pts), [0, 4096], [0, 1024])
assert out.dtype == torch.int32 and np.array_equal(out.numpy(), pt_ref.fps_item(pts, 1024))
assert out[0] == 0 and len(set(out.tolist())) == 1024
''')


def test_fps_takes_the_lowest_index_at_an_exact_float32_tie():
    """toronto3d_sphere(0, 50000) has 25 836 points; at pick 1 124 its two best candidates have the same float32 minimum
    distance (asserted here through the numpy restatement), so the tie rule decides every later pick."""
    _run(r'''
pts = synth_data.toronto3d_sphere(0, 50000)
assert pts.shape == (25836, 3)
ref, ties = pt_ref.fps_item(pts, 1500, return_ties=True)
assert 1124 in ties, ties
out = ops.furthest_point_sampling(torch.from_numpy(pts), [0, len(pts)], [0, 1500])
assert np.array_equal(out.numpy(), ref), int(np.argmax(out.numpy() != ref))
''')


def test_fps_edge_cases():
    _run(r'''
rng = np.random.default_rng(3)
# m == n: every point once (distinct random points), in the canonical order
p = rng.random((300, 3), dtype=np.float32)
out = ops.furthest_point_sampling(torch.from_numpy(p), [0, 300], [0, 300]).numpy()
assert np.array_equal(out, pt_ref.fps_item(p, 300)) and sorted(out.tolist()) == list(range(300))
# identical points: every minimum is 0 after the first pick, the lowest index wins every time
same = np.tile(np.float32([[1.5, -2.0, 0.25]]), (200, 1))
out = ops.furthest_point_sampling(torch.from_numpy(same), [0, 200], [0, 50]).numpy()
assert np.array_equal(out, np.zeros(50, np.int32)) and np.array_equal(out, pt_ref.fps_item(same, 50))
# an empty item, an item that samples nothing, and two items of different length: GLOBAL rows
pts = np.concatenate([pt_ref.room(2, 700), pt_ref.room(3, 5000), pt_ref.room(4, 90)])
rs, nrs = [0, 700, 700, 5700, 5790], [0, 175, 175, 1425, 1425]
out = ops.furthest_point_sampling(torch.from_numpy(pts), rs, nrs).numpy()
assert np.array_equal(out, pt_ref.fps(pts, rs, nrs))
assert out[0] == 0 and out[175] == 700 and out[175:].min() >= 700 and out.max() < 5700
# m > n: refused on the host, before any kernel (the output buffer stays untouched)
L = _abi.get()
q = np.ascontiguousarray(pts[:100]); o = np.full(101, -7, np.int32)
a, b = np.asarray([0, 100], np.int64), np.asarray([0, 101], np.int64)
rc = L.ml3d_furthest_point_sampling(q.ctypes.data, a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, 1, 100,
                                    o.ctypes.data, None, 0, None)
assert rc == -1 and (o == -7).all()
try:
    ops.furthest_point_sampling(torch.from_numpy(q), [0, 100], [0, 101])
    raise SystemExit("m > n accepted")
except RuntimeError as e:
    assert "invalid argument" in str(e)
''')


_OPS_INPUTS = r'''
from ml3d.ops import pointtransformer as P
def case(c, ns, n=600):
    rng = np.random.default_rng(100 * c + ns)
    p = pt_ref.room(5, n)
    p = torch.from_numpy(p - (p.min(0) + p.max(0)) / 2)
    idx = ops.knn_search(p, p, ns).neighbors_index
    return rng, p, idx
def f32(a):
    return torch.from_numpy(np.asarray(a, np.float32))
'''


@pytest.mark.parametrize("c,ns", [(32, 8), (32, 16), (128, 8), (128, 16)])
def test_attention_kernel_against_the_direct_formula(c, ns):
    _run(_OPS_INPUTS + r'''
c, ns = %d, %d
rng, p, idx = case(c, ns)
n = p.shape[0]
qkv = f32(rng.standard_normal((n, 3 * c)))
a = pt_ref.random_attention_params(c, 7, P.attention_hidden_rows(c))
ep = (f32(rng.uniform(0.6, 1.5, c) * np.where(rng.random(c) < 0.2, -1, 1)), f32(rng.normal(0, 0.2, c)))
for e in (None, ep):
    out = ops.pt_attention(qkv, p, idx, a, epilogue=e)
    ref = pt_ref.attention_formula(qkv, p, idx, a, e)
    err = float((out - ref).abs().max())
    print("attention c=%%d ns=%%d epilogue=%%s: max|d| = %%.3g at |ref| <= %%.3g" %% (c, ns, e is not None, err, float(ref.abs().max())))
    assert err <= 1e-5, err
# an odd number of queries (two queries share a wave when nsample is 8): the last group is half empty
out = ops.pt_attention(qkv[:n - 1].contiguous(), p[:n - 1].contiguous(), idx[:n - 1].clamp(max=n - 2).contiguous(), a)
ref = pt_ref.attention_formula(qkv[:n - 1], p[:n - 1], idx[:n - 1].clamp(max=n - 2), a)
assert float((out - ref).abs().max()) <= 1e-5
''' % (c, ns))


@pytest.mark.parametrize("c,ns", [(32, 8), (32, 16), (128, 8), (128, 16)])
def test_transition_kernels_against_the_direct_formulas(c, ns):
    """Weights and features at the magnitudes of the pseudo-trained model (Linear weights uniform in +-1.6 / sqrt(fan_in),
    post-ReLU features of order 1, BatchNorm scales in +-[0.6, 1.5]: a fifth of them negative, so the maximum must follow the
    affine step)."""
    _run(_OPS_INPUTS + r'''
c, ns = %d, %d
rng, p, idx_self = case(c, ns)
n, cout = p.shape[0], 2 * c
feat = f32(np.abs(rng.standard_normal((n, c))))
samp = ops.furthest_point_sampling(p, [0, n], [0, n // 4])
newp = p[samp.long()].contiguous()
nbr = ops.knn_search(p, newp, ns).neighbors_index
w = rng.uniform(-1, 1, (3 + c, cout)) * 1.6 / np.sqrt(3 + c)
wx, wft = f32(w[:3]), f32(w[3:])
sc, sh = f32(rng.uniform(0.6, 1.5, cout) * np.where(rng.random(cout) < 0.2, -1, 1)), f32(rng.normal(0, 0.2, cout))
got_p, got = ops.pt_transition_down(feat, p, samp, nbr, wft, wx, sc, sh)
ref = pt_ref.transition_down_formula(feat, p, samp, nbr, wft, wx, sc, sh)
err = float((got - ref).abs().max())
print("transition_down c=%%d ns=%%d: max|d| = %%.3g" %% (c, ns, err))
assert torch.equal(got_p, newp) and err <= 1e-5, err
r = ops.knn_search(newp, p, 3, return_distances=True)
a = f32(np.abs(rng.standard_normal((n, cout))))
got = ops.pt_interpolate(a, ref, r.neighbors_index, r.neighbors_distance)
want = pt_ref.interpolate_formula(a, ref, r.neighbors_index, r.neighbors_distance)
err = float((got - want).abs().max())
print("interpolate c=%%d: max|d| = %%.3g" %% (cout, err))
assert err <= 1e-5, err
# a sampled point coincides with one of the queries: distance 0 -> weight 1 up to the 1e-8 guard
hit = int(samp[0])
assert float(r.neighbors_distance[hit, 0]) == 0.0 and float((got[hit] - (a[hit] + ref[0])).abs().max()) <= 1e-5
''' % (c, ns))


def test_small_model_forward_against_the_reference_golden():
    out = _run(r'''
from ml3d.torch.models import PointTransformer
from ml3d.torch.dataloaders import PointTransformerBatch
g = np.load(os.path.join(ROOT, "tests", "golden", "pointtransformer_small.npz"))
mcfg = json.loads(str(g["model_json"]))
m = PointTransformer(**mcfg, device="cpu")
sd = m.state_dict()
assert list(sd) == [str(k) for k in g["state_keys"]]
assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g["state_shapes"]]
assert [(k, tuple(v.shape)) for k, v in sd.items()] == pt_ref.state_shapes(mcfg)
m.load_state_dict(pt_ref.make_state_dict(mcfg, int(g["weights_seed"])))
pts, feat, rs = pt_ref.make_batch_arrays(g["cloud_seeds"], g["sizes"])
assert abs(pts.astype(np.float64).sum() - float(g["points_sum"])) < 1e-6
items = [{"data": dict(point=pts[rs[i]:rs[i + 1]], feat=feat[rs[i]:rs[i + 1]], label=np.zeros(rs[i + 1] - rs[i], np.int64))}
         for i in range(len(rs) - 1)]
out = m(PointTransformerBatch(items)).numpy()
used = m.last_indices
for l in range(4):
    assert np.array_equal(used["fps"][l].numpy(), g["fps%%d" %% (l + 1)]), l
    assert pt_ref.knn_checksum(used["knn_down"][l].numpy()) == int(g["knn_down%%d" %% (l + 1)]), l
    assert pt_ref.knn_checksum(used["knn_up"][l].numpy()) == int(g["knn_up%%d" %% l]), l
for l in range(5):
    assert pt_ref.knn_checksum(used["knn_self"][l].numpy()) == int(g["knn_self%%d" %% l]), l
err = float(np.abs(out - g["logits"]).max())
print("small forward: max|dlogit| = %%.3g, logit scale %%.2f, labels differing %%d" %%
      (err, float(g["logit_scale"]), int((out.argmax(1) != g["labels"]).sum())))
assert out.shape == g["logits"].shape and err <= 1e-4, err
''' % ())
    assert "small forward" in out


# ---- the bodies of tests/pt_cases.py (shared with tests/test_gpu_pointtransformer_ops.py) ------------------------------------------
def _case(body):
    out = _run("import pt_cases as C\n" + body + "\nprint('cases ok')\n")
    assert "cases ok" in out
    return out


@pytest.mark.parametrize("c", C.ATTENTION_WIDTHS)
def test_cases_attention_every_instantiation_against_float64(c):
    out = _case("for ns in C.NSAMPLES:\n    C.check_attention_widths('cpu', %d, ns)" % c)
    assert out.count("max_abs_delta") == 4


def test_cases_attention_tiny_clamping_row_independence_refusals():
    _case("C.check_attention_tiny('cpu')\nC.check_attention_clamping('cpu')\nC.check_attention_row_independence('cpu')\n"
          "C.check_attention_refusals('cpu')")


@pytest.mark.parametrize("c,cout,ns", C.DOWN_SHAPES)
def test_cases_transition_down_against_float64(c, cout, ns):
    _case("C.check_transition_down('cpu', %d, %d, %d)" % (c, cout, ns))


def test_cases_transition_down_clamping_and_interpolate_short_item_and_refusals():
    _case("C.check_transition_down_clamping_and_refusal('cpu')\nC.check_interpolate_short_item_and_refusal('cpu')")


@pytest.mark.parametrize("c,k", C.INTERP_SHAPES)
def test_cases_interpolate_against_float64(c, k):
    _case("C.check_interpolate('cpu', %d, %d)" % (c, k))


def test_cases_grid_stride_loops_at_the_narrow_width():
    """Beyond 1025 points, but cheap on the emulator at c = 32: the attention's grid of 6144 workgroups and the two grids capped
    at 65 535 (c = 512 at n = 12 293 is left to the GPU)."""
    _case("for c, ns in C.ATTENTION_GRID:\n    if c == 32:\n        C.check_attention_grid_stride('cpu', c, ns)\n"
          "C.check_transition_down_grid_cap('cpu')\nC.check_interpolate_grid_cap('cpu')")


def test_cases_fps_launch_classes_workspace_form_and_dense_ties():
    _case("for length in C.FPS_BOUNDARIES:\n    C.check_fps_class_boundary('cpu', length)\n"
          "C.check_fps_workspace_form('cpu')\nC.check_fps_dense_ties('cpu')")


def test_cases_fps_full_samples():
    _case("C.check_fps_full_samples('cpu', twice=False)")
