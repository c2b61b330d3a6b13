"""CPU: the bodies of tests/randla_cases.py (which tests/test_gpu_randla_paths.py runs on the MI355X) against the HOST EMULATION of
csrc/randla.hip, in child interpreters with tests/emu_runtime.py installed as in tests/test_emulated_gemm.py, for every row of at
most about 2 000 rows per level (the emulator's device reports 4 CUs, so the rows sized by a grid cap are small there and still
make workers take a second tile).  Two passes:

* plain: the product's dispatch (below 65 536 rows every per-point Linear is a tile GEMM or ``linear_act``);
* ``ML3D_RANDLA_FUSE_ROWS=1`` (the library's one test hook, read once per process, launched like ``_run_variant`` of
  tests/test_emulated_kernels.py): the same rows with ``mlp_wave_s<ShapeLin...>`` and the ``ShapeEnc64`` chain in them; the
  restated rules of randla_cases read the same variable, so the classes a row asserts follow.

Logits against float64 within max(1e-5, 4 e32), everything else for equality.  This file is what can be run and debugged on a
machine without a GPU; what the emulator's cooperative fibers cannot show (missing waits, the matrix unit's lane maps) is the GPU
file's business."""
import os
import subprocess
import sys

import pytest

import emu
import randla_cases as G      # (the case table only: the bodies run in the child)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_runtime
emu_runtime.install("ml3d")
import randla_cases as G
'''

PLAIN, FUSED = {}, {"ML3D_RANDLA_FUSE_ROWS": "1"}
NETS = sorted(set(c[0] for c in G.CASES))


def _child(body, hooks):
    emu.lib()
    env = {k: v for k, v in os.environ.items() if k != "ML3D_RANDLA_FUSE_ROWS"}
    env.update(hooks)
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp", env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
    return r.stdout


def _rows_of(net, hooks):
    """The emulated rows of a net; the second pass only those whose kernels the hook changes (the attention kernels do not
    depend on it)."""
    rows = [i for i, c in enumerate(G.CASES) if c[0] == net and G.emulated(c)]
    if hooks:
        rows = [i for i in rows if G.kernels_with_fuse_rows(G.CASES[i], 1) != G.kernels_with_fuse_rows(G.CASES[i], None)]
    return rows


@pytest.mark.parametrize("net", NETS)
def test_rows_of_one_net_against_float64_and_under_a_tile_order(net):
    rows = _rows_of(net, PLAIN)
    out = _child("for i in %r:\n    G.check_case('cpu', i, orders=(('reversed', 'random')[i %% 2],))" % (rows,), PLAIN)
    assert out.count("max_abs_delta") == len(rows) > 0


# (in the 128-, 256- and 512-wide nets the hook changes nothing but fc1's 64 -> 32 Linear and the 32 -> 32 mlp, which the narrow nets run
# at a tenth of the emulation time)
FUSED_NETS = [n for n in NETS if _rows_of(n, FUSED) and not n.startswith(("b3_", "stage512"))]


@pytest.mark.parametrize("net", FUSED_NETS)
def test_rows_whose_linears_fuse_under_the_row_threshold_hook(net):
    rows = _rows_of(net, FUSED)
    out = _child("for i in %r:\n    G.check_case('cpu', i, orders=())" % (rows,), FUSED)
    assert out.count("max_abs_delta") == len(rows) > 0


def test_exact_checks_and_refusals():
    _child("for i in %r:\n    G.check_exact('cpu', i)\nG.check_refusals('cpu')" % (list(G.EXACT_EMULATED),), PLAIN)


def test_the_fused_pass_reaches_the_fused_classes():
    """The classes the second pass is for, derived by the restated rules under the hook (the child asserts them per row)."""
    out = _child("print(sorted(set(k for c in G.CASES if G.emulated(c) for k in G.kernels_of(c, G.EMU_CUS))))", FUSED)
    for k in ("mlp_wave_s<ShapeLin8x8>", "mlp_wave_s<ShapeLin16x8>", "mlp_wave_s<ShapeLin32x32>", "mlp_wave_s<ShapeLin32x64>", "mlp_wave_s<ShapeLin64x32>",
              "mlp_chain_b3<ShapeEnc64>", "mlp_chain_b3<ShapeDecFc1>", "mlp_chain_b3<ShapeFc1>"):
        assert k in out, k
