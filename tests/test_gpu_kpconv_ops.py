"""GPU: every dispatch arm of csrc/kpconv.hip ONE AT A TIME on the MI355X -- the bodies and tables of tests/kp_cases.py (shared
with tests/test_emulated_kpconv_ops.py, which runs them on the host emulator; tests/test_kp_cases_can_fail.py shows that they can
fail and that the tables reach every kernel the file dispatches).  ``ops.kpconv_weighted``, ``ops.kpconv_rigid`` (fused first
layer, the 32 -> 32 block, aggregation + GEMM, float and bf16x3 contraction), ``ops.kpconv_deformable`` and
``ops.kpconv_weighted_backward`` against the formulas of tests/kp_ref.py in FLOAT64 on the CPU, within max(1e-5, 4 e32) where e32
is the float32 formula's own distance from float64 at the same inputs; repeated calls, rows computed alone, all-shadow rows, H = 0
and ``ops.gather_pool`` for equality.  Every case prints its measured figures before it asserts.

Measured on an MI355X, per kernel family, max |kernel - float64| / e32 at its two extremes and the case nearest its bound (the
1e-5 floor is the bound of all but a handful of cases: ``tol`` reaches 1.8e-5 at cin = 24, h = 260):
  kp_weighted<G, J>        81 cases  0.73 .. 2.0   nearest the bound: cin = 24, h = 260: 6.8e-6 at e32 4.5e-6, tol 1.8e-5
  kp_weighted_small<CIN>   47 cases  0.31 .. 2.1   cin = 4, h = 127: 2.7e-6 at e32 2.5e-6
  kp_agg_mfma<NT, MODE>    66 cases  0.66 .. 2.0   deformable cin = 64, h = 260: 4.2e-6 at e32 2.4e-6 (long walk, 8221 queries: 6.6e-7 at e32 6.2e-7)
  kp_agg_gemm32<MODE>      31 cases  0.40 .. 1.8   h = 260: 3.3e-6 at e32 2.4e-6 (long walk, 16 517 queries: 9.8e-7 at e32 1.7e-6)
  kp_small_fused<CIN, NV>  88 cases  0.61 .. 2.6   4 -> 64, h = 131: 3.0e-6 at e32 2.7e-6, tol 1.09e-5
  aggregation + f32 GEMM   35 cases  0.26 .. 1.7   16 -> 64: 2.7e-6 at e32 1.6e-6
  aggregation + bf16x3     12 cases  0.25 .. 1.1   256 -> 64: 1.65e-6 at e32 1.54e-6 -- the bf16x3 contraction needs no wider bound
  gaussian influence       (inside the rows above) at most 2.02 e32 (5 -> 128, 1.5e-6): ``expf`` needs no wider bound either
  kp_weighted_adjoint      11 cases  0.65 .. 3.0   cin = 1: 9.0e-7 at e32 3.0e-7; h = 131: 1.8e-6 at e32 1.4e-6; the inner-product
                                                   identity differs by at most 1.1e-5 where its bound is 3e-3 or more
The 425 tests take 4.6 s."""
import pytest

import kp_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cases(*groups):
    cases = [c for g in groups for c in C.cases_of(g)]
    return pytest.mark.parametrize("case", cases, ids=[c["id"] for c in cases])


@_cases("agg_cin")
def test_aggregation_every_channel_count(case):
    C.run_case(DEV, case)


@_cases("agg_misaligned")
def test_aggregation_features_not_16_byte_aligned(case):
    C.run_case(DEV, case)


@_cases("agg_influence")
def test_aggregation_constant_linear_gaussian(case):
    C.run_case(DEV, case)


@_cases("agg_width")
def test_aggregation_every_row_width(case):
    C.run_case(DEV, case)


@_cases("agg_tail")
def test_aggregation_query_tails(case):
    C.run_case(DEV, case)


@_cases("agg_long")
def test_aggregation_long_walk_second_query_per_wave(case):
    C.run_case(DEV, case)


@_cases("fused_shape")
def test_fused_first_layer_every_instantiation(case):
    C.run_case(DEV, case)


@_cases("fused_full")
def test_fused_first_layer_influence_bias_activation(case):
    C.run_case(DEV, case)


@_cases("fused_width", "fused_tail")
def test_fused_first_layer_row_widths_and_query_tails(case):
    C.run_case(DEV, case)


@_cases("fused_leaving")
def test_first_layer_widths_that_leave_the_fused_kernel(case):
    C.run_case(DEV, case)


@_cases("b32_full")
def test_block_32_to_32_influence_bias_activation(case):
    C.run_case(DEV, case)


@_cases("b32_tail", "b32_width")
def test_block_32_to_32_query_tails_and_row_widths(case):
    C.run_case(DEV, case)


@_cases("b32_long")
def test_block_32_to_32_long_walk_second_tile_per_workgroup(case):
    C.run_case(DEV, case)


@_cases("b32_leaving")
def test_block_32_shapes_that_leave_the_one_kernel_block(case):
    C.run_case(DEV, case)


@_cases("agg_gemm")
def test_aggregation_plus_gemm_float_and_bf16x3(case):
    C.run_case(DEV, case)


@_cases("h0", "nq0")
def test_no_neighbour_columns_and_no_queries(case):
    C.run_case(DEV, case)


@_cases("deformable")
def test_deformable(case):
    C.run_case(DEV, case)


def test_deformable_refusals():
    C.check_deformable_refusals(DEV)


@_cases("adjoint")
def test_adjoint_against_float64_and_the_forward(case):
    C.run_case(DEV, case)


@_cases("pool")
def test_gather_pool_bit_for_bit(case):
    C.run_case(DEV, case)
