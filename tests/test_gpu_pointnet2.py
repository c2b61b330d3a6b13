"""GPU: every kernel of csrc/pointnet2.hip on the MI355X -- the bodies of tests/pn2_cases.py (shared with
tests/test_emulated_pointnet2.py, which runs them on the host emulator).  Ball query and the three nearest neighbours for
EQUALITY with the numpy restatements of tests/pn2_ref.py; the set-abstraction body (fused kernel at widths up to 128, unfused
route at 128-196-256) and the interpolation against the direct formula in FLOAT64 on the CPU, within max(1e-5, 4 e32) where e32
is the float32 formula's own distance from float64 at the same inputs; slice writes, rows computed alone and repeated calls bit
for bit.  Every case prints its measured figures before it asserts.

Measured on an MI355X (max |kernel - float64| / e32): set abstraction between 4.0e-7 / 3.1e-7 (32-32-64, nsample 16, m = 67) and
1.4e-6 / 1.1e-6 (128-196-256 unfused, nsample 32, m = 67), every case under the 1e-5 floor; interpolation 2.8e-7 .. 6.0e-7 at e32 of
the same size.  Module against the REAL reference forward: small golden 9.1e-6 (hip) / 6.0e-6 (torch), hip against torch 9.5e-6;
KITTI golden (feature scale 21.8, bound 1e-4) 3.8e-5 (hip) / 4.4e-5 (torch), hip against torch 5.7e-5.  The 39 tests take 3.5 s."""
import pytest

import pn2_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("m", C.BALL_M)
@pytest.mark.parametrize("n", C.BALL_N)
def test_ball_query_both_scales_in_one_scan_equal_the_contract(n, m):
    C.check_ball_query(DEV, n, m)


def test_ball_query_truncation_padding_no_hit_and_early_fill():
    C.check_ball_query_properties(DEV)


def test_ball_query_boundary_and_duplicates():
    C.check_ball_query_boundary_and_duplicates(DEV)


def test_ball_query_batch_items_equal_their_single_runs():
    C.check_ball_query_batch(DEV)


def test_ball_query_refusals():
    C.check_ball_query_refusals(DEV)


@pytest.mark.parametrize("m", C.SA_M)
@pytest.mark.parametrize("ns", C.SA_NSAMPLE)
@pytest.mark.parametrize("cf,widths", C.SA_CASES, ids=["-".join(map(str, w)) for _, w in C.SA_CASES])
def test_set_abstraction_against_float64(cf, widths, ns, m):
    C.check_sa(DEV, cf, widths, ns, m)


def test_set_abstraction_refusals():
    C.check_sa_refusals(DEV)


@pytest.mark.parametrize("name", C.MODULE_GOLDENS)
def test_module_forward_against_the_reference_golden(name):
    C.check_module(DEV, name)


def test_three_nn_order_ties_and_refusal():
    C.check_three_nn(DEV)


@pytest.mark.parametrize("c", C.INTERP_C)
def test_interpolate_against_float64(c):
    C.check_interpolate(DEV, c)
