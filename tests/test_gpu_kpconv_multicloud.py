"""GPU: the multi-cloud KPConv sphere loop on the MI355X -- the bodies of tests/kpconv_multicloud_cases.py at the emulator's
shapes: ``ops.sphere_select`` / ``ops.device_sphere_batch`` bit for bit against ``ops.fixed_radius_search`` and numpy,
``KPFCNN.inference_many`` against single-cloud runs.  Equality everywhere; the one tolerance is the 1e-4 that
tests/test_gpu_kpconv.py applies to KPFCNN logits (a sphere forwarded in the big batch against its own cloud's batch)."""
import numpy as np
import pytest

import kpconv_multicloud_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_sphere_select_equals_fixed_radius_search_per_cloud():
    M.check_sphere_select(DEV)


def test_device_sphere_batch_equals_the_numpy_crop_bit_for_bit():
    M.check_device_sphere_batch(DEV)


@pytest.fixture(scope="module")
def singles():
    clouds = M.model_clouds()
    return {i: M.run_single(M.MODEL_CFG, DEV, c, s) for i, (c, s) in enumerate(zip(clouds, M.SEEDS))}


@pytest.fixture(scope="module")
def runs():
    clouds = M.model_clouds()
    return {S: M.collect(M.MODEL_CFG, DEV, clouds, M.SEEDS, S) for S in (1, 3, 4)}


def test_the_inputs_make_batches_of_two_and_three_spheres_cuts_and_retries(singles):
    M.assert_inputs_qualify(singles, M.MODEL_CFG)


@pytest.mark.parametrize("in_flight", [1, 3, 4])
def test_inference_many_reproduces_the_single_cloud_runs(singles, runs, in_flight):
    run = runs[in_flight]
    assert all(r is not None for r in run["results"]) and sorted(run["recs"]) == [0, 1, 2, 3]
    assert max(sum(n for _, n in b) for b in run["batches"]) > 3 or in_flight == 1        # a real batch: spheres of several clouds
    assert max(len(b) for b in run["batches"]) == min(in_flight, 4)
    M.assert_many_is_single(run, singles)
    assert run["info"][M.FAR_CLOUD]["retries"] > 0
    assert run["stats"]["read_backs"] == run["stats"]["sub_rounds"]                       # ONE read-back per sub-round


@pytest.mark.parametrize("in_flight", [1, 3, 4])
def test_logits_in_the_big_batch_stay_within_the_kpfcnn_tolerance(singles, runs, in_flight):
    M.assert_logits_within_tolerance(runs[in_flight], singles)


def test_more_clouds_than_slots_are_admitted_as_others_retire(singles, runs):
    run = runs[3]
    first = {c: min(r for r, b in enumerate(run["batches"]) if c in [x for x, _ in b]) for c in range(4)}
    assert first[0] == first[1] == first[2] == 0 and first[3] > 0, first


def test_one_in_flight_is_the_sequential_loop(singles, runs):
    run = runs[1]
    assert all(len(b) == 1 for b in run["batches"])
    for i, (res1, *_rest) in singles.items():                  # the same batches through the same forward: even the votes agree
        assert np.array_equal(run["results"][i]["predict_labels"], res1["predict_labels"])
        assert np.array_equal(run["results"][i]["predict_scores"].view(np.uint16), res1["predict_scores"].view(np.uint16))


def test_the_same_seeds_twice_give_the_same_run(runs):
    again = M.collect(M.MODEL_CFG, DEV, M.model_clouds(), M.SEEDS, 3)
    M.assert_same_run(again, runs[3])


@pytest.mark.parametrize("why", ["sklearn", "normalize_points"])
def test_a_model_that_must_fall_back_gives_the_single_cloud_result(why):
    cfg = dict(M.MODEL_CFG)
    if why == "sklearn":
        pytest.importorskip("sklearn")
        cfg["sampler_index"] = "sklearn"
    else:
        cfg["t_normalize"] = dict(cfg["t_normalize"], normalize_points=True)
    M.check_fallback(DEV, cfg, M.model_clouds()[0], 77)
