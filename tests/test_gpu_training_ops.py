"""GPU: every dispatch arm of csrc/train.hip and the four differentiable entry points of csrc/randla.hip ONE AT A TIME on the MI355X
-- the bodies and tables of tests/train_cases.py (shared with tests/test_emulated_training_ops.py, which runs them on the host
emulator; tests/test_train_cases_can_fail.py shows that they can fail and that the tables reach every kernel).  ``ml3d_gemm_tn``
(strided, with and without the column sums), BatchNorm forward / backward (null gamma / beta, the running buffers through
``ops.BatchNormActFunction``), the row gathers and their adjoints, the fused attention stage both ways, the deformed KPConv
aggregation both ways, the offset regulariser, ``GatherMaxFunction`` and ``AttentivePoolFunction`` against the formulas of
tests/train_ref.py in FLOAT64 on the CPU, within max(1e-5, 4 e32) where e32 is the float32 formula's own distance from float64 at
the same inputs; gather / max forwards, repeated calls of everything without float atomics and the sentinel padding for equality.
Every case prints its measured figures before it asserts.

Measured on an MI355X, per kernel family: the float comparisons, max |kernel - float64| / e32 at its two extremes, and the
comparison nearest its bound.  The 1e-5 floor is the bound of all but ~70 of the 1200 comparisons; NO family needs more than 4 e32:
a ratio above 4 occurs only far under the floor (5 comparisons, at errors of 1.6e-6 or less), so the bound stands as stated.
  gemm_tn_k, col_reduce_k<0>          170  0.01 .. 3.97  m = 128, k = 33, n = 65, strided: 2.0e-6 at e32 2.0e-6 (slices by tiles, m = 65 665: 2.6e-6)
  BatchNorm forward (ABI)             264  0.03 .. 5.4   rows = 2, c = 512, y: 6.4e-6 at e32 6.4e-6, tol 2.5e-5; 5.4 e32 = 5.5e-7 (rows = 2, c = 5)
  BatchNorm backward (ABI)            174  0.15 .. 4.4   rows = 2, c = 257, gx: 1.19e-5 at e32 1.17e-5, tol 4.7e-5; 4.4 e32 = 2.9e-7 (rows = 7, c = 1)
  ops.BatchNormActFunction             28  0.33 .. 1.07  rows = 2, c = 340, gx: 5.5e-5 at e32 5.4e-5, tol 2.2e-4 (1 / sqrt(var) of two rows)
  gathers and adjoints                 47  0.78 .. 1.40  past the 8192-workgroup cap, max adjoint: 3.5e-6 at e32 2.5e-6
  attn_stage_fwd_k<64>                 34  0.67 .. 2.3   B N = 65, d = 96: 3.2e-6 at e32 3.0e-6, tol 1.2e-5
  attn_stage_fwd_k<32>                 13  0.63 .. 2.3   B N = 65, d = 256: 6.0e-6 at e32 3.2e-6, tol 1.3e-5 (the 160 MB cap case: 8.2e-6 at e32 4.9e-6)
  attn_stage_bwd_k<16>                 46  0.03 .. 2.9   d = 6, B N = 34, gw: 2.3e-6 at e32 3.2e-6
  attn_stage_bwd_k<64>                 39  0.31 .. 3.1   d = 18, B N = 1, gw: 2.2e-6 at e32 7.9e-7 (three-level sum, B N = 2050, gw: 1.4e-6 at e32 4.5e-6)
  attn_stage_bwd_k<128>                36  0.52 .. 1.2   d = 96, B N = 1, gw: 2.3e-6 at e32 2.3e-6
  attn_stage_bwd_k<256>                46  0.79 .. 3.5   d = 256, B N = 5, gw: 2.6e-6 at e32 2.1e-6
  kp_deformed_weighted_k               17  0.50 .. 1.2   cin = 8, a support on a kernel point: 1.3e-6 at e32 1.2e-6
  kp_deformed_weighted_bwd_k           34  0.38 .. 2.9   cin = 200, gkp: 1.5e-6 at e32 5.3e-7
  kp_offset_reg_k                     105  0.04 .. 1.4   K = 16, h = 1, grep: 2.8e-6 at e32 2.1e-6
  gather_max_adjoint                   12  0.92 .. 1.7   c = 6, n_out = 8: 3.6e-7 at e32 2.1e-7
  attentive_pool_k<false|true>        135  0.42 .. 8.8   k = 31, c = 64, gscores: 2.1e-6 at e32 1.1e-6; 8.8 e32 = 1.5e-6 (k = 32, c = 1, one row)
``grad_bias`` of the attention stage (reference ~1e-16) stays below 5e-7.  The 341 tests take 6.5 s, the largest (BatchNorm past
the 4096-workgroup cap, 4.2 M elements) 0.9 s."""
import pytest

import train_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cases(*groups):
    cases = [c for g in groups for c in C.cases_of(g)]
    return pytest.mark.parametrize("case", cases, ids=[c["id"] for c in cases])


@_cases("gemm_kn")
def test_gemm_tn_every_tile_shape(case):
    C.run_case(DEV, case)


@_cases("gemm_m", "gemm_strided")
def test_gemm_tn_row_counts_slices_and_strides(case):
    C.run_case(DEV, case)


@_cases("gemm_by_tiles")
def test_gemm_tn_slices_limited_by_the_tile_count(case):
    C.run_case(DEV, case)


@_cases("bn_c", "bn_rows")
def test_batchnorm_channel_counts_and_row_counts(case):
    C.run_case(DEV, case)


@_cases("bn_full")
def test_batchnorm_activation_and_null_gamma_beta(case):
    C.run_case(DEV, case)


@_cases("bn_function")
def test_batchnorm_function_and_running_buffers(case):
    C.run_case(DEV, case)


@_cases("bn_cap")
def test_batchnorm_past_the_4096_workgroup_cap(case):
    C.run_case(DEV, case)


@_cases("gathers")
def test_gathers_and_adjoints_shadows_ties_and_strides(case):
    C.run_case(DEV, case)


@_cases("gathers_cap")
def test_gathers_past_the_8192_workgroup_cap(case):
    C.run_case(DEV, case)


@_cases("attn_shapes")
def test_attention_stage_every_width_class(case):
    C.run_case(DEV, case)


@_cases("attn_rows")
def test_attention_stage_point_counts_and_batch_straddling_tiles(case):
    C.run_case(DEV, case)


@_cases("attn_levels")
def test_attention_stage_three_level_sum_and_more_tiles_than_groups(case):
    C.run_case(DEV, case)


@_cases("attn_cap")
def test_attention_stage_at_the_160_mb_cap(case):
    C.run_case(DEV, case)


@_cases("deformed")
def test_deformed_kpconv_aggregation(case):
    C.run_case(DEV, case)


@_cases("regulariser")
def test_offset_regulariser(case):
    C.run_case(DEV, case)


@_cases("gather_max")
def test_randla_gather_max(case):
    C.run_case(DEV, case)


@_cases("attentive_pool")
def test_randla_attentive_pool(case):
    C.run_case(DEV, case)


@pytest.mark.parametrize("family", C.REFUSAL_FAMILIES)
def test_refusals(family):
    C.check_refusals(DEV, family)
