"""CPU: the bodies of tests/gemm_cases.py (which tests/test_gpu_gemm.py runs on the MI355X) against the HOST EMULATION of
csrc/gemm.hip, each in its own interpreter with tests/emu_runtime.py installed as in tests/test_emulated_pointtransformer.py, for
every case of at most about 2 000 rows.  Three passes:

* plain: the product's dispatch (the f32 convolutions stay on gemm_tile: nothing small passes big_bn's 256-tile bar);
* ``ML3D_GEMM_BIG_MIN_TILES=1`` (a hook of the emulator build): the same f32 convolutions through gemm_tile2;
* ``ML3D_CONV_WINDOW=0`` (likewise): the stride-1 3 x 3 convolutions with ``packed`` through gemm_tile_bf3 instead of conv3x3s1_bf3.

Floats against float64 within max(1e-5, 4 e32), everything else for equality (tests/gemm_cases.py).  This run is where the
bodies themselves get debugged before a GPU visit; what the cooperative fibers of the emulator cannot show (missing waits, the
lane-to-row map of the matrix unit, the tile remap) is the GPU file's business."""
import os
import subprocess
import sys

import pytest

import emu
import gemm_cases as G      # (the shape tables only: the bodies run in the subprocess)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not emu.available(), reason="clang++ for the host emulator not found")

_PRELUDE = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, "open3d-ml_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import emu_runtime
emu_runtime.install("ml3d")
import gemm_cases as G
'''

PLAIN, BIG, NO_WINDOW = {}, {"ML3D_GEMM_BIG_MIN_TILES": "1"}, {"ML3D_CONV_WINDOW": "0"}
_HOOKS = ("ML3D_GEMM_BIG_MIN_TILES", "ML3D_CONV_WINDOW")


def _case(body, hooks=PLAIN):
    emu.lib()
    env = {k: v for k, v in os.environ.items() if k not in _HOOKS}
    env.update(hooks)
    r = subprocess.run([sys.executable, "-c", _PRELUDE % {"root": ROOT} + body + "\nprint('cases ok')\n"], capture_output=True,
                       text=True, timeout=1500, cwd="/tmp", env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout
    return r.stdout


_both = pytest.mark.parametrize("hooks", [PLAIN, BIG], ids=["plain", "big_min_tiles_1"])
_window = pytest.mark.parametrize("hooks", [PLAIN, BIG, NO_WINDOW], ids=["plain", "big_min_tiles_1", "conv_window_0"])


@_both
def test_cases_linear_plain_two_blocks_and_generic_loader(hooks):
    out = _case("for m in G.A1_M:\n    G.check_linear_plain('cpu', m)\nG.check_linear_two_blocks('cpu')\n"
                "G.check_linear_generic_loader('cpu')", hooks)
    assert out.count("max_abs_delta") == len(G.A1_M) * len(G.A1_N) * len(G.A1_K) + 1 + len(G.A3)


@_both
def test_cases_linear_split_k(hooks):
    assert _case("G.check_linear_split_k('cpu')", hooks).count("max_abs_delta") == 2 * len(G.A4)


@_both
def test_cases_conv_f32_and_channel_slice(hooks):
    _case("G.check_conv_f32_small('cpu')\nG.check_conv_into_channel_slice('cpu')", hooks)


@_both
def test_cases_bf16x3_linear(hooks):
    out = _case("for m in G.C1_M:\n    G.check_bf3_linear('cpu', m)\nG.check_bf3_two_blocks('cpu')\nG.check_bf3_rows_on_slices('cpu')", hooks)
    assert out.count("max_abs_delta") == len(G.C1_M) * len(G.C1_N) * len(G.C1_K) + 2 + 3


@_both
def test_cases_bf16x3_split_k(hooks):
    assert _case("G.check_bf3_split_k('cpu')", hooks).count("max_abs_delta") == 2 * len(G.C4)


@_window
def test_cases_bf16x3_window_convolutions(hooks):
    out = _case("for i in range(len(G.D1)):\n    G.check_conv_bf3_window('cpu', i)\nG.check_exact_conv('cpu', G.EXACT_CONV[1])", hooks)
    assert out.count("max_abs_delta") == len(G.D1)


@_both
def test_cases_bf16x3_general_convolution_and_deconvolution(hooks):
    _case("G.check_conv_bf3_general('cpu')\nfor s in G.D4_STRIDES:\n    G.check_deconv_into_concat_slice('cpu', s)", hooks)


@_both
def test_cases_exact_checks(hooks):
    _case("for i in range(len(G.EXACT_ROWS)):\n    G.check_exact_rows('cpu', i)\nG.check_exact_conv('cpu', G.EXACT_CONV[0])\n"
          "G.check_empty_and_refused('cpu')", hooks)
