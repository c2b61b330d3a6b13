"""GPU: every kernel family, tile class and split path of csrc/gemm.hip ONE AT A TIME on the MI355X, through the public Python
entries only -- the bodies and shape tables of tests/gemm_cases.py (shared with tests/test_emulated_gemm.py, which runs the
cases of at most about 2 000 rows on the host emulator): ``gemm_tile<RowsLoader | ConvLoader, PLAIN, DEPTH>`` plain, generic,
split along K and above 12 288 workgroups, ``gemm_tile2<ConvLoader2, BN, KC>`` at sizes that pass ``big_bn``'s 256-tile bar
(with ``xcd_tile`` remainders 0, 3, 4 and 6), ``gemm_tile_bf3<RowsLoader2 | ConvLoader2, 64 | 128>`` unsplit and through both
branches of ``bf3_splits``, ``conv3x3s1_bf3<64 | 128>`` on narrow and short images, ``gemm_reduce`` behind both split rules,
column slices and the pixel-shuffle store.  Floats against the direct formula in FLOAT64 on the CPU within max(1e-5, 4 e32),
e32 = the float32 formula's own distance from float64 at the same inputs (pt_cases.judge); determinism, power-of-two scalings,
row / column independence, slack and refusals for equality, bit for bit.  The measured figures of every float comparison are
appended to the per-YAML parity record of tests/test_gpu_configs.py (family ``gemm_ops``).

Measured on an MI355X: max |kernel - float64| / e32 per comparison (the kernel each one ran, established with a scratch build, is
in profiles/gemm_gpu_tests.md); all 187 are inside max(1e-5, 4 e32), the closest (B3, 2 x 131 x 127 x 64 -> 128,
gemm_tile2<ConvLoader2, 128, 64>) at 0.50 of it.  Every exact check passed bit for bit on every path.
  A1 ops.linear plain (M, N, K): (1, 4, 32) 3.18e-07 / 1.19e-07, (1, 4, 96) 1.55e-07 / 2.14e-07, (1, 64, 32) 2.73e-07 /
    3.17e-07, (1, 64, 96) 3.73e-07 / 7.19e-07, (1, 68, 32) 3.29e-07 / 4.83e-07, (1, 68, 96) 8.85e-07 / 8.85e-07, (1, 132, 32)
    3.52e-07 / 5.03e-07, (1, 132, 96) 1.04e-06 / 1.04e-06, (63, 4, 32) 4.75e-07 / 4.32e-07, (63, 4, 96) 5.53e-07 / 1.02e-06,
    (63, 64, 32) 5.67e-07 / 6.20e-07, (63, 64, 96) 1.23e-06 / 1.16e-06, (63, 68, 32) 5.77e-07 / 5.95e-07, (63, 68, 96) 1.18e-06
    / 1.04e-06, (63, 132, 32) 8.89e-07 / 7.17e-07, (63, 132, 96) 1.08e-06 / 1.25e-06, (64, 4, 32) 3.26e-07 / 3.62e-07, (64, 4,
    96) 7.57e-07 / 7.12e-07, (64, 64, 32) 8.63e-07 / 7.54e-07, (64, 64, 96) 1.11e-06 / 1.06e-06, (64, 68, 32) 8.14e-07 /
    6.75e-07, (64, 68, 96) 1.05e-06 / 1.37e-06, (64, 132, 32) 6.94e-07 / 8.25e-07, (64, 132, 96) 1.16e-06 / 1.29e-06, (65, 4,
    32) 3.89e-07 / 4.59e-07, (65, 4, 96) 8.00e-07 / 9.47e-07, (65, 64, 32) 6.60e-07 / 6.05e-07, (65, 64, 96) 1.07e-06 /
    1.19e-06, (65, 68, 32) 8.24e-07 / 6.86e-07, (65, 68, 96) 1.04e-06 / 9.70e-07, (65, 132, 32) 7.15e-07 / 9.03e-07, (65, 132,
    96) 1.19e-06 / 1.28e-06, (129, 4, 32) 6.93e-07 / 6.11e-07, (129, 4, 96) 8.94e-07 / 1.04e-06, (129, 64, 32) 7.75e-07 /
    6.79e-07, (129, 64, 96) 1.06e-06 / 1.22e-06, (129, 68, 32) 7.30e-07 / 9.67e-07, (129, 68, 96) 1.25e-06 / 1.49e-06, (129,
    132, 32) 9.27e-07 / 1.38e-06, (129, 132, 96) 1.32e-06 / 1.32e-06
  A2 two blocks: (300, 64, 32 + 64) 1.40e-06 / 1.27e-06
  A3 generic loader: (130, 36, 40) 6.79e-07 / 9.86e-07, (130, 36, 5) 3.47e-07 / 3.47e-07, (130, 19, 64) 1.03e-06 / 1.27e-06,
    (70, 1, 64) 4.19e-07 / 5.59e-07, (130, 36, 48 + 32) 1.08e-06 / 1.04e-06, (130, 36, 64) gather 1.00e-06 / 1.00e-06, (130,
    36, 32 + 64) gather 1.03e-06 / 9.39e-07
  A4 split-K: (130, 36, 544) act 1 residual rows 8.61e-07 / 2.21e-06, (130, 36, 544) act 2 9.66e-07 / 1.53e-06, (200, 68, 1000)
    act 1 residual rows 1.13e-06 / 3.78e-06, (200, 68, 1000) act 2 1.20e-06 / 2.97e-06, (65, 19, 800) act 1 residual rows
    8.47e-07 / 1.75e-06, (65, 19, 800) act 2 7.53e-07 / 1.62e-06, (77, 20, 640) act 1 residual gather 7.96e-07 / 1.39e-06, (77,
    20, 640) act 2 8.04e-07 / 1.67e-06
  A5 DEPTH 1: (393280, 68, 32) 1.58e-06 / 1.75e-06, (786496, 8, 12) 1.30e-06 / 1.01e-06
  B1 f32 conv, gemm_tile: 2x17x9x48 -> 20 3x3/1 3.18e-06 / 2.05e-06, 2x17x9x4 -> 12 3x3/2 4.82e-07 / 3.89e-07, 2x7x5x8 -> 12
    1x1/1 4.97e-07 / 4.97e-07, 1x9x7x8 -> 20 5x5/1 2.09e-06 / 9.59e-07
  B2 f32 conv split-K: 1x20x28x64 -> 64 3x3/1 1.52e-06 / 1.43e-06, 1x20x28x128 -> 64 3x3/2 9.41e-07 / 1.09e-06
  B3 f32 conv, gemm_tile2: 2x131x127x32 -> 64 3x3/1 3.51e-06 / 1.87e-06, 2x131x127x32 -> 36 3x3/1 3.75e-06 / 2.71e-06,
    2x131x127x32 -> 128 3x3/1 3.58e-06 / 2.94e-06, 2x131x127x32 -> 72 3x3/1 3.43e-06 / 2.91e-06, 2x131x127x64 -> 128 3x3/1
    5.01e-06 / 2.29e-06, 2x262x254x32 -> 64 3x3/2 3.62e-06 / 2.04e-06, 2x131x127x256 -> 64 1x1/1 3.21e-06 / 2.02e-06,
    1x183x181x32 -> 64 3x3/1 3.81e-06 / 2.09e-06, 1x183x181x32 -> 192 3x3/1 3.64e-06 / 2.55e-06
  B5 f32 conv DEPTH 1: 1x887x887x4 -> 8 3x3/1 1.67e-06 / 1.47e-06
  B4 channel slice: f32 channel slice 1.44e-06 / 1.36e-06, bf3 channel slice 1.82e-06 / 1.36e-06
  C1 linear_bf16x3 (M, N, K): (1, 4, 32) 1.07e-07 / 1.19e-07, (1, 4, 96) 2.28e-07 / 2.14e-07, (1, 20, 32) 1.14e-07 / 5.61e-07,
    (1, 20, 96) 2.71e-07 / 2.38e-07, (1, 64, 32) 3.37e-07 / 5.20e-07, (1, 64, 96) 4.10e-07 / 3.71e-07, (1, 65, 32) 2.68e-07 /
    1.91e-07, (1, 65, 96) 7.50e-07 / 6.00e-07, (1, 72, 32) 1.23e-07 / 3.06e-07, (1, 72, 96) 3.93e-07 / 3.95e-07, (1, 128, 32)
    2.38e-07 / 3.27e-07, (1, 128, 96) 4.52e-07 / 3.04e-07, (1, 132, 32) 1.95e-07 / 5.03e-07, (1, 132, 96) 3.42e-07 / 1.04e-06,
    (1, 200, 32) 2.98e-07 / 3.72e-07, (1, 200, 96) 5.50e-07 / 7.44e-07, (127, 4, 32) 3.69e-07 / 4.05e-07, (127, 4, 96) 5.14e-07
    / 6.77e-07, (127, 20, 32) 3.43e-07 / 5.70e-07, (127, 20, 96) 1.11e-06 / 1.12e-06, (127, 64, 32) 6.01e-07 / 7.05e-07, (127,
    64, 96) 1.01e-06 / 1.24e-06, (127, 65, 32) 5.20e-07 / 7.98e-07, (127, 65, 96) 8.39e-07 / 1.21e-06, (127, 72, 32) 7.87e-07 /
    6.56e-07, (127, 72, 96) 1.05e-06 / 1.23e-06, (127, 128, 32) 7.64e-07 / 8.98e-07, (127, 128, 96) 1.16e-06 / 1.65e-06, (127,
    132, 32) 8.22e-07 / 9.36e-07, (127, 132, 96) 1.18e-06 / 1.10e-06, (127, 200, 32) 6.76e-07 / 1.09e-06, (127, 200, 96)
    1.17e-06 / 1.79e-06, (128, 4, 32) 2.43e-07 / 8.18e-07, (128, 4, 96) 7.65e-07 / 7.61e-07, (128, 20, 32) 7.69e-07 / 7.89e-07,
    (128, 20, 96) 8.81e-07 / 1.16e-06, (128, 64, 32) 5.11e-07 / 7.46e-07, (128, 64, 96) 8.75e-07 / 1.83e-06, (128, 65, 32)
    5.37e-07 / 7.95e-07, (128, 65, 96) 9.49e-07 / 1.41e-06, (128, 72, 32) 5.95e-07 / 9.93e-07, (128, 72, 96) 1.20e-06 /
    1.10e-06, (128, 128, 32) 6.41e-07 / 8.32e-07, (128, 128, 96) 1.17e-06 / 1.42e-06, (128, 132, 32) 5.42e-07 / 6.84e-07, (128,
    132, 96) 1.06e-06 / 1.28e-06, (128, 200, 32) 9.44e-07 / 9.37e-07, (128, 200, 96) 1.32e-06 / 1.40e-06, (129, 4, 32) 3.87e-07
    / 5.76e-07, (129, 4, 96) 9.32e-07 / 1.02e-06, (129, 20, 32) 4.36e-07 / 6.64e-07, (129, 20, 96) 7.74e-07 / 1.15e-06, (129,
    64, 32) 5.58e-07 / 7.52e-07, (129, 64, 96) 1.15e-06 / 1.11e-06, (129, 65, 32) 7.89e-07 / 6.75e-07, (129, 65, 96) 1.02e-06 /
    1.67e-06, (129, 72, 32) 6.14e-07 / 8.44e-07, (129, 72, 96) 1.16e-06 / 1.24e-06, (129, 128, 32) 9.61e-07 / 8.29e-07, (129,
    128, 96) 1.37e-06 / 1.33e-06, (129, 132, 32) 4.95e-07 / 7.31e-07, (129, 132, 96) 1.37e-06 / 1.39e-06, (129, 200, 32)
    5.80e-07 / 9.27e-07, (129, 200, 96) 1.25e-06 / 1.48e-06, (257, 4, 32) 4.55e-07 / 6.49e-07, (257, 4, 96) 6.41e-07 /
    6.90e-07, (257, 20, 32) 6.69e-07 / 7.03e-07, (257, 20, 96) 8.60e-07 / 1.10e-06, (257, 64, 32) 6.24e-07 / 1.10e-06, (257,
    64, 96) 1.13e-06 / 1.43e-06, (257, 65, 32) 6.78e-07 / 8.96e-07, (257, 65, 96) 1.16e-06 / 1.41e-06, (257, 72, 32) 6.93e-07 /
    8.33e-07, (257, 72, 96) 9.50e-07 / 1.21e-06, (257, 128, 32) 6.80e-07 / 1.06e-06, (257, 128, 96) 1.04e-06 / 1.59e-06, (257,
    132, 32) 7.61e-07 / 1.02e-06, (257, 132, 96) 1.10e-06 / 1.46e-06, (257, 200, 32) 8.12e-07 / 1.03e-06, (257, 200, 96)
    1.12e-06 / 1.50e-06
  C2 two blocks: (300, 64, 32 + 64) 1.14e-06 / 1.27e-06, (300, 136, 32 + 64) 1.10e-06 / 1.50e-06
  C3 linear_rows_bf16x3 on slices: bf3 slices m=257 n=72 k=64 8.31e-07 / 1.07e-06, bf3 slices m=130 n=20 k=64 8.10e-07 /
    7.16e-07, bf3 slices m=129 n=72 k=544 1.22e-06 / 3.82e-06
  C4 split-K: (129, 72, 544) act 1 residual rows 9.76e-07 / 2.95e-06, (129, 72, 544) act 2 8.59e-07 / 2.48e-06, (257, 200,
    1056) act 1 residual rows 9.87e-07 / 3.10e-06, (257, 200, 1056) act 2 9.41e-07 / 3.06e-06, (130, 40, 1024) act 1 residual
    gather 7.59e-07 / 2.14e-06, (130, 40, 1024) act 2 6.71e-07 / 2.42e-06
  C5 split-K, 513 tiles: (65537, 128, 512) 1.61e-06 / 2.70e-06, (65537, 64, 512) 1.77e-06 / 2.44e-06
  D1 window conv: 2x13x11x32 -> 64 3x3/1 2.38e-06 / 1.78e-06, 1x3x140x64 -> 128 3x3/1 2.68e-06 / 2.03e-06, 3x9x16x32 -> 200
    3x3/1 2.19e-06 / 1.81e-06, 2x1x37x64 -> 40 3x3/1 1.13e-06 / 8.27e-07, 2x45x1x32 -> 64 3x3/1 5.44e-07 / 4.23e-07, 1x16x16x96
    -> 64 3x3/1 3.06e-06 / 1.28e-06
  D2 general bf16x3 conv: 2x12x14x64 -> 128 3x3/2 2.61e-06 / 1.35e-06, 1x9x7x64 -> 48 1x1/1 7.23e-07 / 9.13e-07, 1x9x7x32 -> 40
    5x5/1 2.47e-06 / 1.41e-06, 2x5x5x32 -> 20 3x3/2 6.47e-07 / 4.48e-07, 2x31x9x96 -> 132 3x3/2 3.72e-06 / 2.22e-06
  D3 7x7 fallback: 1x9x8x32 -> 24 7x7/1 7.87e-07 / 1.75e-06
  D4 deconv: f32 deconv stride=1 9.50e-07 / 1.43e-06, bf3 deconv stride=1 7.33e-07 / 1.43e-06, f32 deconv stride=2 9.37e-07 /
    1.17e-06, bf3 deconv stride=2 8.34e-07 / 1.17e-06, f32 deconv stride=4 1.09e-06 / 1.13e-06, bf3 deconv stride=4 1.28e-06 /
    1.13e-06
The 52 tests take 5.5 s together, the slowest (A5, 393 280 rows: mostly its float64 reference) 0.83 s.
"""
import pytest

import gemm_cases as G
from test_gpu_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def report(**kv):
    print(" ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items()), flush=True)
    record(kv.pop("name"), family="gemm_ops", **kv)


# ---- A: ops.linear -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", G.A1_M)
def test_linear_plain_rows_against_float64(m):
    G.check_linear_plain(DEV, m, report)


def test_linear_two_plain_blocks_with_a_residual():
    G.check_linear_two_blocks(DEV, report)


def test_linear_generic_loader_tails_scalar_loads_and_gathers():
    G.check_linear_generic_loader(DEV, report)


def test_linear_split_k_with_an_uneven_last_slice():
    G.check_linear_split_k(DEV, report)


@pytest.mark.parametrize("index", range(len(G.A5)))
def test_linear_one_chunk_pipeline_above_12288_workgroups(index):
    G.check_linear_depth1(DEV, index, report)


# ---- B: the f32 convolution ----------------------------------------------------------------------------------------------------------
def test_conv_f32_tile_kernel_unsplit_and_split_k():
    G.check_conv_f32_small(DEV, report)


@pytest.mark.parametrize("index", range(len(G.B3)))
def test_conv_f32_register_blocked_kernel_every_instantiation(index):
    G.check_conv_f32_big(DEV, index, report)


def test_conv_f32_one_chunk_pipeline_above_12288_workgroups():
    G.check_conv_f32_depth1(DEV, report)


def test_conv_into_a_channel_slice_leaves_the_rest_alone():
    G.check_conv_into_channel_slice(DEV, report)


# ---- C: the bf16x3 Linears -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", G.C1_M)
def test_bf16x3_linear_against_float64(m):
    G.check_bf3_linear(DEV, m, report)


def test_bf16x3_linear_two_blocks_with_a_residual():
    G.check_bf3_two_blocks(DEV, report)


def test_bf16x3_linear_rows_on_column_slices_with_poisoned_slack():
    G.check_bf3_rows_on_slices(DEV, report)


def test_bf16x3_split_k_with_an_uneven_last_slice():
    G.check_bf3_split_k(DEV, report)


@pytest.mark.parametrize("index", range(len(G.C5)))
def test_bf16x3_split_k_of_513_row_tiles(index):
    G.check_bf3_split_k_many_tiles(DEV, index, report)


# ---- D: convolutions on the bf16 pipe, transposed convolution ------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(G.D1)))
def test_bf16x3_window_convolution(index):
    G.check_conv_bf3_window(DEV, index, report)


def test_bf16x3_general_convolution_and_the_49_tap_fallback():
    G.check_conv_bf3_general(DEV, report)


@pytest.mark.parametrize("stride", G.D4_STRIDES)
def test_deconv_into_a_concat_slice_on_both_paths(stride):
    G.check_deconv_into_concat_slice(DEV, stride, report)


# ---- exact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(G.EXACT_ROWS)))
def test_rows_determinism_scalings_and_independence_bit_for_bit(index):
    G.check_exact_rows(DEV, index)


@pytest.mark.parametrize("shape", G.EXACT_CONV + (G.EXACT_CONV_BIG,))
def test_conv_determinism_and_scalings_bit_for_bit(shape):
    G.check_exact_conv(DEV, shape)


def test_empty_and_refused_problems():
    G.check_empty_and_refused(DEV)
