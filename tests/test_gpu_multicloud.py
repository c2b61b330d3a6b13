"""GPU: the multi-cloud patch loop on the MI355X -- the bodies of tests/test_emulated_multicloud.py (tests/multicloud_cases.py) at
the same small shapes, one case at the SemanticKITTI YAML's size (num_points = 45 056, 4 layers: the sort across many tiles, the
45 056-row mean chains side by side) and a determinism case.  Equality everywhere; the one tolerance is the 1e-4 that
tests/test_gpu_randlanet.py applies to RandLA logits (a patch forwarded at batch A against batch 1)."""
import numpy as np
import pytest
import torch

import multicloud_cases as M
import synth_data
import synth_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_possibility_argmin_matches_numpy_per_segment():
    M.check_possibility_argmin(DEV)


def test_device_patch_batch_equals_the_single_cloud_ops_per_cloud():
    M.check_device_patch_batch(DEV)


def _small():
    in_ch, aug = M.AUGMENTS[1]
    cfg = dict(M.SMALL, in_channels=in_ch, augment=aug, grid_size=M.SMALL_GRID)
    clouds, seeds = M.small_clouds()
    return cfg, M.with_features(clouds, in_ch), seeds


@pytest.fixture(scope="module")
def small_run():
    cfg, clouds, seeds = _small()
    return M.collect(cfg, DEV, clouds, seeds, 2)


def test_inference_many_reproduces_four_single_cloud_runs(small_run):
    cfg, clouds, seeds = _small()
    singles = {i: M.run_single(cfg, DEV, c, s) for i, (c, s) in enumerate(zip(clouds, seeds))}
    sizes = [len(b) for b in small_run["batches"]]
    assert max(sizes) == 2 and sizes[-1] == 1, sizes
    M.assert_many_is_single(small_run, singles)


def test_the_same_call_twice_gives_the_same_votes(small_run):
    cfg, clouds, seeds = _small()
    again = M.collect(cfg, DEV, clouds, seeds, 2, batch_one=False)
    assert again["batches"] == small_run["batches"]
    for i in range(len(clouds)):
        a, b = again["results"][i], small_run["results"][i]
        assert np.array_equal(a["predict_scores"].view(np.uint16), b["predict_scores"].view(np.uint16)), i
        assert np.array_equal(a["predict_labels"], b["predict_labels"]), i


def test_first_rounds_at_the_semantickitti_size_equal_single_cloud_loops():
    """num_points = 45 056, 4 layers, 3 sweeps of different sizes all in flight, the first 4 rounds, patch for patch against the
    single-cloud device loops; the logits of a patch at batch 3 against the single-cloud loop's batch 1 within 1e-4."""
    cfg = dict(synth_weights.RANDLANET_SEMANTICKITTI_CFG, grid_size=0.06, augment={"recenter": {"dim": [0, 1]}})
    assert cfg["num_points"] == 45056 and cfg["num_layers"] == 4
    clouds = []
    for seed, n_az in ((5000, 2048), (5001, 1536), (5003, 1792)):
        sweep = synth_data.lidar_sweep(seed, n_azimuth=n_az)
        clouds.append(dict(point=sweep, feat=None, label=(np.arange(sweep.shape[0]) % 19).astype(np.int32)))
    seeds, rounds = [31, 32, 33], 4
    m = M.make_model(cfg, DEV)
    m.load_state_dict(synth_weights.randlanet_state_dict(cfg, 2024))
    patches = {}

    class _Stop(Exception):
        pass

    def on_batch(slots, inputs, logits):
        M._record(slots, inputs, logits, patches)
        if len(patches[0]) >= rounds:
            raise _Stop

    with pytest.raises(_Stop):
        m.inference_many(clouds, seeds=seeds, max_in_flight=3, on_batch=on_batch)
    sizes = set()
    for i, (c, s) in enumerate(zip(clouds, seeds)):
        one = M.make_model(cfg, DEV, seed=s)
        one.load_state_dict(synth_weights.randlanet_state_dict(cfg, 2024))
        one.inference_begin(dict(c))
        assert one._dev_loop is not None
        sizes.add(int(one._dev_loop["points"].shape[0]))
        assert len(patches[i]) == rounds
        for step in range(rounds):
            inp = one.inference_preprocess()["data"]
            res = one(inp)
            one.inference_end({"data": inp}, res)
            y = dict(point_inds=M._np(inp["point_inds"][0]), coords0=M._np(inp["coords"][0][0]), features=M._np(inp["features"][0]),
                     labels=M._np(inp["labels"][0]), nbr=[M._np(t[0]) for t in inp["neighbor_indices"]],
                     itp=[M._np(t[0]) for t in inp["interp_idx"]])
            M.same_patch(patches[i][step], y, (i, step))
            err = float(np.abs(patches[i][step]["logits"] - M._np(res[0])).max())
            assert err <= M.LOGIT_TOL, (i, step, err)
    assert len(sizes) == 3 and min(sizes) > 45056, sizes
