"""GPU: ``ops.randla_knn_pyramid(..., tile_order=...)`` on the cases of tests/pyramid_build_cases.py against the CPU oracle, bit
for bit -- every level's 16-NN rows, every level's 1-NN interpolation index, and each level's tile order a permutation of each
cloud's rows.  Calls of at least 48 clouds of at most 131 072 points (pyramid_build_cases.MIN_BATCH_FUSED / MAX_N0_FUSED) get
their grids from grid_build_pyramid (one launch, one workgroup per cloud: box, probe, set-up, and per level zero / histogram /
scan / scatter, csrc/grid.hip): the ``*_fused`` cases and the 300-cloud batch; every other case, the two at the limits among
them, shows the launch chain still serving what the builder does not take.  What only the GPU can show is here: a missing wait between two phases of the
workgroup, a table word read from a stale cache line, neighbouring workgroups treading on each other's table ranges (the mixed
batch, the 300-cloud batch with several workgroups per CU) -- each loses, doubles or misplaces points, which the search then
misses.  The comparison of the two builders' grids word for word is tests/test_emulated_pyramid_build.py's."""
import numpy as np
import pytest
import torch

import pyramid_build_cases as PC

pytestmark = pytest.mark.gpu


def _run(name):
    from ml3d import ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pts, ratios, _ = PC.case(name)
    B, n0, _ = pts.shape
    n = PC.sizes(n0, ratios)
    d = torch.device("cuda:0")
    tp = torch.from_numpy(np.array(pts)).to(d)
    order = [torch.full((B * n[l],), -9, dtype=torch.int32, device=d) for l in range(len(ratios))]
    nbr, itp = ops.randla_knn_pyramid(tp, ratios, PC.K, tile_order=order)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in nbr], [x.cpu().numpy() for x in itp], [x.cpu().numpy() for x in order]


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_pyramid_matches_the_oracle_bit_for_bit(name):
    PC.check(name, *_run(name))


def test_twenty_calls_in_one_process_return_identical_results():
    """Nothing a call leaves behind (table words, the probe's bitmaps in the level-0 table range, cache lines) may reach the next:
    twenty calls, all equal to the first and to the oracle.  (The tile order is arrival order inside a cell and may differ.)"""
    name = "four_levels_fused"
    first = _run(name)
    PC.check(name, *first)
    for _ in range(19):
        nbr, itp, order = _run(name)
        for a, b in zip(first[0] + first[1], nbr + itp):
            assert np.array_equal(a, b)
        PC.check(name, nbr, itp, order)
