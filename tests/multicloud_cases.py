"""Shared bodies of the multi-cloud patch loop tests (tests/test_emulated_multicloud.py runs them on CPU tensors against the host
emulation of the HIP sources, tests/test_gpu_multicloud.py on the MI355X): ``ops.possibility_argmin`` against numpy per segment,
``ops.device_patch_batch`` against the single-cloud ops per cloud, ``RandLANet.inference_many`` against single-cloud runs.
Everything the sampler produces is compared for EQUALITY: a cloud's patches depend only on its own possibilities and its own
shuffle draws, so lock step changes nothing.  The only tolerance is the one tests/test_gpu_randlanet.py applies to RandLA
logits (1e-4), for the same patch forwarded at batch A and at batch 1."""
import numpy as np
import torch

import synth_data
from oracle import randlanet_ref as R

LOGIT_TOL = 1e-4          # tests/test_gpu_randlanet.py: TOL

SMALL = dict(num_neighbors=16, num_layers=2, num_points=640, num_classes=5, sub_sampling_ratio=[4, 4], dim_features=8,
             dim_output=[16, 32], grid_size=0.25)
AUGMENTS = ((3, {"recenter": {"dim": [0, 1]}}),
            (6, {"recenter": {"dim": [0, 1, 2]}, "normalize": {"feat": {"method": "linear", "bias": 0, "scale": 255}}}))


def _np(t):
    return t.detach().cpu().numpy()


# ---- test 1 ------------------------------------------------------------------------------------------------------------------------
def check_possibility_argmin(dev):
    from ml3d import ops
    rng = np.random.default_rng(11)
    lengths = [1, 63, 64, 65, 300, 257, 1000, 5000, 2048, 2049]        # off wave (64) and tile (2048) boundaries; 5000 = 3 tiles
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    poss = rng.random(int(splits[-1]))
    seg = lambda s: poss[splits[s]:splits[s + 1]]
    seg(6)[[100, 700, 999]] = -1.0                 # a repeated minimum: the first index wins
    seg(7)[[2047, 2048, 4999]] = -2.0              # ... also when the repeats lie in different tiles
    seg(5)[256] = -3.0                             # the minimum at the segment's last element
    seg(9)[2048] = -4.0                            # ... alone in the last tile
    seg(4)[:] = -9.0                               # the INACTIVE slot (between active ones) holds the smallest values of all
    active = [s for s in range(len(lengths)) if s != 4]
    d = torch.from_numpy(poss).to(dev)
    idx = torch.full((len(lengths),), -7, dtype=torch.int32, device=dev)
    mins = torch.full((len(lengths),), 7.5, dtype=torch.float64, device=dev)
    got = ops.possibility_argmin(d, splits, active, out=(idx, mins))
    assert got[0] is idx and got[1] is mins
    idx, mins = _np(idx), _np(mins)
    for s in active:
        assert idx[s] == np.argmin(seg(s)) and mins[s] == np.min(seg(s)), (s, idx[s], mins[s])
    assert idx[6] == 100 and idx[7] == 2047 and idx[5] == 256 and idx[9] == 2048
    assert idx[4] == -7 and mins[4] == 7.5, "an inactive slot's outputs must be untouched"
    assert np.array_equal(_np(d), poss)
    # all slots (active=None), fresh outputs; and a second call gives the same answer (deterministic)
    i2, m2 = ops.possibility_argmin(d, splits)
    i3, m3 = ops.possibility_argmin(d, splits)
    for s in range(len(lengths)):
        assert _np(i2)[s] == np.argmin(seg(s)) and _np(m2)[s] == np.min(seg(s))
    assert torch.equal(i2, i3) and torch.equal(m2, m3)
    # the wrapper's checks
    for bad in (lambda: ops.possibility_argmin(d.float(), splits), lambda: ops.possibility_argmin(d, splits[::-1].copy()),
                lambda: ops.possibility_argmin(d, splits, [3, 2]), lambda: ops.possibility_argmin(d[:-1], splits),
                lambda: ops.possibility_argmin(d, [0, 0, int(splits[-1])])):
        try:
            bad()
        except RuntimeError:
            continue
        raise AssertionError("a bad argument was accepted")


# ---- test 2 ------------------------------------------------------------------------------------------------------------------------
def check_device_patch_batch(dev, k=640):
    from ml3d import ops
    tile = synth_data.toronto3d_tile(5, half=3.0, density=0.3)
    P, F = tile["point"], tile["feat"]
    rng = np.random.default_rng(3)
    pick = lambda n: rng.choice(len(P), n, replace=False)
    sets = [pick(k), pick(k + 1), pick(3 * k - 7), pick(900), pick(k + 150)]
    dup = sets[4]
    dup[200:500] = dup[:300]                      # duplicated points: equal distances, the order is by ascending index
    inactive = 3
    pts = [np.ascontiguousarray(P[s]) for s in sets]
    ext = [np.ascontiguousarray(F[s]) for s in sets]
    splits = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    active = [s for s in range(len(sets)) if s != inactive]
    poss0 = [rng.random(len(p)) * 1e-3 for p in pts]
    poss0[1][[17, 400]] = 0.0                    # a repeated minimum
    perms = np.stack([rng.permutation(k).astype(np.int32) for _ in active])
    cat_pts = torch.from_numpy(np.concatenate(pts)).to(dev)
    cat_ext = torch.from_numpy(np.concatenate(ext)).to(dev)
    for dims in ((), (0, 1), (0, 1, 2)):          # dims_mask 0, 3, 7
        for with_extra in (False, True):
            bias, scale = (0.0, 255.0) if with_extra else (0.0, 1.0)
            cat_poss = torch.from_numpy(np.concatenate(poss0)).to(dev)
            idx, _ = ops.possibility_argmin(cat_poss, splits, active)
            out = ops.device_patch_batch(cat_pts, cat_poss, splits, active, idx, torch.from_numpy(perms).to(dev), k, dims,
                                         cat_ext if with_extra else None, bias, scale)
            b_pts, b_feats, b_sel, b_row = (_np(t) for t in out)
            after = _np(cat_poss)
            for a, s in enumerate(active):
                p1 = torch.from_numpy(pts[s]).to(dev)
                q1 = torch.from_numpy(poss0[s].copy()).to(dev)
                c1 = torch.argmin(q1).reshape(1)
                assert int(c1) == int(_np(idx)[s])
                perm = torch.from_numpy(perms[a]).to(dev)
                near = ops.nearest_to_center(p1, p1[int(c1)], k)
                s_pts, s_feats, s_sel = ops.device_patch(p1, q1, c1, perm, k, dims, torch.from_numpy(ext[s]).to(dev) if with_extra else None,
                                                         bias, scale)
                assert np.array_equal(_np(near)[perms[a]], _np(s_sel))
                assert np.array_equal(b_sel[a], _np(s_sel)), (dims, with_extra, s)
                assert np.array_equal(b_row[a], b_sel[a] + splits[s])
                assert np.array_equal(b_pts[a].view(np.uint32), _np(s_pts).view(np.uint32)), (dims, with_extra, s)
                assert np.array_equal(b_feats[a].view(np.uint32), _np(s_feats).view(np.uint32)), (dims, with_extra, s)
                assert np.array_equal(after[splits[s]:splits[s + 1]], _np(q1)), (dims, with_extra, s)
                assert len(np.unique(b_sel[a])) == k
            s = inactive
            assert np.array_equal(after[splits[s]:splits[s + 1]], poss0[s]), "an inactive cloud's possibilities must not change"
    # the wrapper's checks: k larger than an active cloud, a permutation of the wrong shape, unsorted slots
    cat_poss = torch.from_numpy(np.concatenate(poss0)).to(dev)
    idx, _ = ops.possibility_argmin(cat_poss, splits)
    dperm = torch.from_numpy(perms).to(dev)
    for bad in (lambda: ops.device_patch_batch(cat_pts, cat_poss, splits, None, idx, torch.zeros((5, k + 2), dtype=torch.int32, device=dev), k + 2),
                lambda: ops.device_patch_batch(cat_pts, cat_poss, splits, active, idx, dperm[:3], k),
                lambda: ops.device_patch_batch(cat_pts, cat_poss, splits, active[::-1], idx, dperm, k)):
        try:
            bad()
        except RuntimeError:
            continue
        raise AssertionError("a bad argument was accepted")
    assert np.array_equal(_np(cat_poss), np.concatenate(poss0))


# ---- tests 3 - 5 -------------------------------------------------------------------------------------------------------------------
def make_model(cfg, dev, seed=None, weights_seed=4):
    from ml3d.torch.models import RandLANet
    m = RandLANet(**cfg, device=dev, **({} if seed is None else {"seed": seed}))
    m.load_state_dict(R.make_state_dict(cfg, weights_seed))
    return m.eval()


def _record(slots, inputs, logits, into):
    """on_batch: per cloud, the list of its patches (everything the batcher's layout carries, one batch row each)."""
    for b, c in enumerate(slots):
        rec = dict(point_inds=_np(inputs["point_inds"][b]), coords0=_np(inputs["coords"][0][b]), features=_np(inputs["features"][b]),
                   labels=_np(inputs["labels"][b]), nbr=[_np(t[b]) for t in inputs["neighbor_indices"]],
                   itp=[_np(t[b]) for t in inputs["interp_idx"]], logits=_np(logits[b]), batch=len(slots))
        into.setdefault(c, []).append(rec)


def run_single(cfg, dev, cloud, seed, max_patches=None):
    """The single-cloud loop to completion -> (result | None, [patch, ...], final possibilities, votes, proj_inds)."""
    m = make_model(cfg, dev, seed=seed)
    m.inference_begin(dict(cloud))
    got, done = [], False
    while not done and (max_patches is None or len(got) < max_patches):
        inp = m.inference_preprocess()["data"]
        res = m(inp)
        done = m.inference_end({"data": inp}, res)
        got.append(dict(point_inds=_np(inp["point_inds"][0]), coords0=_np(inp["coords"][0][0]), features=_np(inp["features"][0]),
                        labels=_np(inp["labels"][0]), nbr=[_np(t[0]) for t in inp["neighbor_indices"]],
                        itp=[_np(t[0]) for t in inp["interp_idx"]], logits=_np(res[0])))
    poss = _np(m._dev_loop["possibility"]) if m._dev_loop is not None else np.asarray(m.possibility)
    return (m.inference_result if done else None), got, poss.copy(), _np(m.test_probs).copy(), np.asarray(m.inference_proj_inds)


def same_patch(x, y, what):
    assert np.array_equal(x["point_inds"], y["point_inds"]), what
    assert np.array_equal(x["coords0"].view(np.uint32), y["coords0"].view(np.uint32)), what
    assert np.array_equal(x["features"].view(np.uint32), y["features"].view(np.uint32)), what
    assert np.array_equal(x["labels"], y["labels"]), what
    for l in range(len(x["nbr"])):
        assert np.array_equal(x["nbr"][l], y["nbr"][l]) and np.array_equal(x["itp"][l], y["itp"][l]), (what, l)


def replay_votes(cfg, dev, patches, n_points):
    """The recorded logits of ONE cloud, in order, through the existing update_probs on a fresh accumulator -> float16 votes."""
    m = make_model(cfg, dev)
    votes = torch.zeros((n_points, cfg["num_classes"]), dtype=torch.float16, device=dev)
    for p in patches:
        m.update_probs({"data": {"point_inds": [torch.from_numpy(p["point_inds"]).to(dev)]}}, torch.from_numpy(p["logits"][None]).to(dev), votes)
    return _np(votes)


def logits_at_batch_one(cfg, dev, patches):
    """Every recorded patch forwarded alone (batch 1) -> list of logits [k, classes]."""
    m = make_model(cfg, dev)
    out = []
    for p in patches:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)[None]).to(dev)
        out.append(_np(m({"coords": [t(p["coords0"])], "features": t(p["features"]), "neighbor_indices": [t(x) for x in p["nbr"]],
                          "interp_idx": [t(x) for x in p["itp"]]})[0]))
    return out


def collect(cfg, dev, clouds, seeds, max_in_flight, batch_one=True):
    """One inference_many run to completion and what the comparisons need from the model besides it: per cloud the recorded
    logits replayed through update_probs, and (``batch_one``) every recorded patch forwarded alone."""
    m = make_model(cfg, dev)
    patches, batches = {}, []

    def on_batch(slots, inputs, logits):
        _record(slots, inputs, logits, patches)
        batches.append(list(slots))

    results = m.inference_many(clouds, seeds=seeds, max_in_flight=max_in_flight, on_batch=on_batch)
    info = m.inference_many_info
    run = dict(results=results, patches=patches, batches=batches, info=info, votes={}, batch_one={})
    for i, mine in patches.items():
        run["votes"][i] = replay_votes(cfg, dev, mine, len(info[i]["possibility"]))
        if batch_one:
            run["batch_one"][i] = logits_at_batch_one(cfg, dev, mine)
    return run


def assert_many_is_single(run, singles, clouds=None):
    """``run`` = collect(...), ``singles`` = {cloud: run_single(...) to completion}: the lock-step run IS the single-cloud runs."""
    for i, (res1, got1, poss1, votes1, proj) in singles.items():
        if i not in run["patches"]:
            continue                                              # (a cloud of the host path: compared by its results)
        mine = run["patches"][i]
        assert len(mine) == len(got1) == run["info"][i]["num_patches"], ("number of patches", i, len(mine), len(got1))
        for step, (x, y) in enumerate(zip(mine, got1)):
            same_patch(x, y, (i, step))
        assert np.array_equal(run["info"][i]["possibility"], poss1), ("final possibilities", i)
        # votes: the recorded logits replayed through update_probs (no forwards of different batch sizes are compared)
        votes, res = run["votes"][i], run["results"][i]
        assert res["predict_scores"].dtype == np.float16 and votes.dtype == np.float16
        assert np.array_equal(res["predict_scores"].view(np.uint16), votes[proj].view(np.uint16)), i
        assert np.array_equal(res["predict_labels"], np.argmax(votes, 1)[proj]), i
        assert res["predict_labels"].shape == res1["predict_labels"].shape
        for step, (p, l1) in enumerate(zip(mine, run["batch_one"].get(i, []))):
            err = float(np.abs(p["logits"] - l1).max())
            assert err <= LOGIT_TOL, ("logits at batch %d against batch 1" % p["batch"], i, step, err)


def assert_same_run(x, y):
    """Two inference_many runs of the same clouds and seeds with different ``max_in_flight``: the same patches, possibilities and
    patch counts exactly; results built from the same votes whenever the forward gave the same logits (compared as in
    assert_many_is_single: each run against the replay of ITS OWN logits), logits of the same patch within LOGIT_TOL."""
    assert sorted(x["patches"]) == sorted(y["patches"])
    for i in x["patches"]:
        assert len(x["patches"][i]) == len(y["patches"][i]) and x["info"][i]["num_patches"] == y["info"][i]["num_patches"]
        for step, (p, q) in enumerate(zip(x["patches"][i], y["patches"][i])):
            same_patch(p, q, (i, step))
            assert float(np.abs(p["logits"] - q["logits"]).max()) <= LOGIT_TOL, (i, step)
        assert np.array_equal(x["info"][i]["possibility"], y["info"][i]["possibility"])
        assert x["results"][i]["predict_labels"].shape == y["results"][i]["predict_labels"].shape
        if all(np.array_equal(p["logits"], q["logits"]) for p, q in zip(x["patches"][i], y["patches"][i])):
            assert np.array_equal(x["results"][i]["predict_scores"].view(np.uint16), y["results"][i]["predict_scores"].view(np.uint16))
            assert np.array_equal(x["results"][i]["predict_labels"], y["results"][i]["predict_labels"])


SMALL_GRID = 0.4          # sub-clouds of ~700 to ~1300 points: 4 to 9 patches of 640 each


def small_clouds():
    """Four raw clouds of different sizes after the 0.4 m subsampling (about 930, 1280, 710 and 1050 points) and their seeds;
    (tile_small: about 600 points, fewer than num_points = 640)."""
    clouds = []
    for seed, half in ((21, 2.0), (22, 2.5), (23, 1.5), (24, 2.2)):
        t = synth_data.toronto3d_tile(seed, half=half, density=0.1)
        clouds.append(dict(point=t["point"], feat=t["feat"], label=t["label"]))
    return clouds, [101, 102, 103, 104]


def tile_small():
    t = synth_data.toronto3d_tile(25, half=1.0, density=0.1)
    return dict(point=t["point"], feat=t["feat"], label=t["label"])


def with_features(clouds, in_ch):
    return [dict(c, feat=c["feat"] if in_ch == 6 else None) for c in clouds]
