"""GPU: every kernel of csrc/ptransformer.hip ONE AT A TIME on the MI355X -- the bodies of tests/pt_cases.py (shared with
tests/test_emulated_pointtransformer.py, which runs the small ones on the host emulator): every ``pt_attn_kernel<NS, NT>``
instantiation and the contract's odd widths, the grid-stride loops of the three capped grids, the contract edges (clamped
indices, nsample 1 .. 64, k 1 .. 16, a = NULL, short items, refusals) and every launch class of the furthest point sampling at
its boundary.  Floats against the direct formula in FLOAT64 on the CPU, within max(1e-5, 4 e32) where e32 is the float32
formula's own distance from float64 at the same inputs (tests/pt_cases.py); everything else for equality.  The measured figures
of every float comparison are appended to the per-YAML parity record of tests/test_gpu_configs.py (family
``pointtransformer_ops``).

Measured on an MI355X: max |kernel - float64| / e32 per case, the larger of the runs with and without the epilogue (of a,
a = None and zero distances for the interpolation); every case is inside max(1e-5, 4 e32), the closest (TransitionDown 256 -> 512) at 0.37 of it.
  attention, n = 333, (c, nsample): (16, 8) 4.26e-7 / 3.79e-7, (16, 16) 3.04e-7 / 3.31e-7, (48, 8) 1.09e-6 / 5.58e-7,
    (48, 16) 8.24e-7 / 5.10e-7, (128, 8) 1.26e-6 / 1.08e-6, (128, 16) 1.30e-6 / 1.08e-6, (256, 8) 1.36e-6 / 1.09e-6,
    (256, 16) 9.86e-7 / 7.66e-7, (384, 8) 1.54e-6 / 1.52e-6, (384, 16) 1.91e-6 / 9.06e-7, (512, 8) 1.71e-6 / 1.15e-6,
    (512, 16) 2.08e-6 / 1.14e-6
  attention, n = 12 293, random lists: (32, 8) 2.91e-6 / 3.41e-6, (32, 16) 2.85e-6 / 2.72e-6, (512, 16) 1.10e-5 / 8.43e-6
    (bound 3.37e-5, |ref| up to 17.8)
  attention, n = 1: (32, 8) 2.96e-7 / 2.96e-7, (256, 8) 6.91e-7 / 6.91e-7, (32, 16) 5.53e-7 / 3.15e-7, (256, 16) 4.71e-7 / 3.32e-7;
    n = 5: (32, 8) 5.38e-7 / 7.44e-7, (256, 8) 2.42e-6 / 2.26e-6, (32, 16) 9.19e-7 / 7.09e-7, (256, 16) 2.90e-6 / 2.41e-6
  attention, clamped lists, n = 77: (48, 8) 1.33e-6 / 1.09e-6, (48, 16) 2.10e-6 / 2.02e-6, (256, 16) 2.68e-6 / 3.04e-6
  TransitionDown (c, c_out, nsample): (32, 64, 8) 9.11e-7 / 9.40e-7, (256, 512, 16) 3.68e-6 / 2.23e-6, (5, 3, 1) 7.20e-8 / 1.45e-7,
    (29, 67, 16) 1.48e-6 / 1.29e-6, (32, 64, 64) 1.02e-6 / 1.00e-6; m = 32 771 x 512: 1.70e-6 / 3.10e-6
  interpolation (c, k): (13, 3) 6.94e-7 / 5.04e-7, (512, 3) 6.22e-7 / 7.72e-7, (64, 1) 2.38e-7 / 2.38e-7, (32, 16) 1.05e-6 / 1.43e-6;
    short item 3.34e-7 / 3.92e-7; n = 32 771 x 512: 7.58e-7 / 9.29e-7
The 43 tests take 7 s together, the slowest (attention, c = 512 at n = 12 293: the float64 reference) 3 s."""
import pytest

import pt_cases as C
from test_gpu_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def report(**kv):
    print(" ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items()), flush=True)
    record(kv.pop("name"), family="pointtransformer_ops", **kv)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", C.NSAMPLES)
@pytest.mark.parametrize("c", C.ATTENTION_WIDTHS)
def test_attention_every_instantiation_against_float64(c, ns):
    C.check_attention_widths(DEV, c, ns, report)


@pytest.mark.parametrize("c,ns", C.ATTENTION_GRID)
def test_attention_grid_stride_loop_against_float64(c, ns):
    C.check_attention_grid_stride(DEV, c, ns, report)


def test_attention_on_one_and_five_points():
    C.check_attention_tiny(DEV, report)


def test_attention_clamps_neighbour_indices_as_the_contract_states():
    C.check_attention_clamping(DEV, report)


def test_attention_rows_do_not_depend_on_the_last_query():
    C.check_attention_row_independence(DEV, report)


def test_attention_refuses_what_the_contract_excludes():
    C.check_attention_refusals(DEV)


# ---- TransitionDown -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cout,ns", C.DOWN_SHAPES)
def test_transition_down_against_float64(c, cout, ns):
    C.check_transition_down(DEV, c, cout, ns, report)


def test_transition_down_clamps_indices_and_refuses_65_neighbours():
    C.check_transition_down_clamping_and_refusal(DEV)


def test_transition_down_beyond_the_grid_cap():
    C.check_transition_down_grid_cap(DEV, report)


# ---- interpolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,k", C.INTERP_SHAPES)
def test_interpolate_against_float64(c, k):
    C.check_interpolate(DEV, c, k, report)


def test_interpolate_short_source_item_and_17_neighbours():
    C.check_interpolate_short_item_and_refusal(DEV, report)


def test_interpolate_beyond_the_grid_cap():
    C.check_interpolate_grid_cap(DEV, report)


# ---- furthest point sampling --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", C.FPS_BOUNDARIES)
def test_fps_launch_class_boundary(length):
    C.check_fps_class_boundary(DEV, length)


def test_fps_workspace_form_with_two_long_items():
    C.check_fps_workspace_form(DEV)


def test_fps_dense_float32_ties_on_a_lattice():
    C.check_fps_dense_ties(DEV)


def test_fps_full_samples():
    C.check_fps_full_samples(DEV)
