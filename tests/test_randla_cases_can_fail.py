"""CPU, no kernel involved: the rows of tests/randla_cases.py CAN fail.  For EVERY row of the table, at the shape the GPU file runs
it at on the MI355X (256 CUs for the rows sized by a grid cap; the loop and fused rows included, cloud by cloud as their references
are), the float64 oracle runs again with a fault injected into the layer under test (``randlanet_ref._lfa`` wrapped for the
last encoder layer), and the row's own bound max(1e-5, 4 e32) must REJECT it:

(a) one neighbour index of the last point of the last cloud replaced by another,
(b) one output channel zeroed on the points of one tile -- the channel and tile of cloud 0's largest output value, so the most
    visible channel, not a typical one (randla_cases.moved_by says why),
(c) uniform relative noise of 2^-12 (about a bf16x3 product that lost its second AND third plane's cross terms).

Noise of 2^-17 (one lost third plane) is printed, not required.  The restated host rules are checked on the way: every row derives
its class at the emulator's 4 CUs, at 256 and at 304."""
import pytest

import randla_cases as G

ROWS = range(len(G.CASES))


@pytest.mark.parametrize("cus", [G.EMU_CUS, 256, 304])
def test_every_row_reaches_the_class_it_states(cus):
    for c in G.CASES:
        G.derive(c, cus)


def test_every_reachable_kernel_appears():
    seen = set(k for c in G.CASES for k in G.kernels_of(c, 256))
    for k in ("lfa_stage<8>", "lfa_stage<512>", "lfa_attn_mfma16<EPI>", "lfa_attn_mfma16<no EPI>", "lfa_attn_wave<32, SPLIT>",
              "lfa_attn_wave_b3<64>", "lfa_attn_b3<128>", "lfa_attn_b3<256>", "head_fc0_mlp1", "linear_act", "gemm_rows",
              "gemm_rows a2 bias2", "gemm_rows a2 gather", "gemm_rows_bf16x3", "gemm_rows_bf16x3 a2 bias2", G.SPLIT_DEC,
              "mlp_wave_s<ShapeLin8x8>", "mlp_wave_s<ShapeLin16x8>", "mlp_wave_s<ShapeLin32x32>", "mlp_wave_s<ShapeLin32x64>", "mlp_wave_s<ShapeLin64x32>",
              "mlp_chain_b3<ShapeEnc64>", "mlp_chain_b3<ShapeDecFc1>", "mlp_chain_b3<ShapeFc1>", "gather_max4"):
        assert k in seen, k
    # no shape of test size reaches these (profiles/randla_gpu_tests.md gives the rule that excludes each)
    for k in seen:
        assert not k.startswith(("lfa_attn_pf", "lfa_attn_wave<64")) and "no SPLIT" not in k and k != "gather_max", k
        assert "ShapeEnc16" not in k, k


@pytest.mark.parametrize("index", ROWS, ids=[G.CASE_IDS[i] for i in ROWS])
def test_the_bound_of_a_row_rejects_a_faulty_layer(index):
    G.check_can_fail(index)
