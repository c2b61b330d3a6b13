"""Shared bodies of the multi-cloud KPConv sphere loop tests (tests/test_emulated_kpconv_multicloud.py runs them on CPU tensors
against the host emulation of the HIP sources, tests/test_gpu_kpconv_multicloud.py on the MI355X): ``ops.sphere_select`` against
``ops.fixed_radius_search`` per cloud, ``ops.device_sphere_batch`` against a numpy restatement of ``KPFCNN._crop_sphere``'s
arithmetic, ``KPFCNN.inference_many`` against single-cloud runs.  Everything the sampler produces is compared for EQUALITY: a
cloud's spheres depend only on its own possibilities and its own draws, so lock step changes nothing.  The only tolerance is
the one tests/test_gpu_kpconv.py applies to KPFCNN logits (1e-4), for a sphere forwarded in the big batch and in its own cloud's."""
import numpy as np
import torch

import synth_data
import synth_weights

LOGIT_TOL = 1e-4          # tests/test_gpu_kpconv.py: TOL


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- op level ----------------------------------------------------------------------------------------------------------------------
RADIUS = 1.8
FAR = 1            # the cloud with an isolated far point (its last)
INACTIVE = 3


def op_clouds():
    """5 clouds of 300 .. 3 000 points cut out of one tile (cloud FAR with an isolated point far away as its last), their colours,
    row splits and the active slots (all but INACTIVE)."""
    tile = synth_data.toronto3d_tile(5, half=3.0, density=0.3)
    P, F = tile["point"], tile["feat"]
    rng = np.random.default_rng(7)
    sizes = [300, 1200, 3000, 700, 2049]
    pts = [np.ascontiguousarray(P[s]) for s in (rng.choice(len(P), n, replace=False) for n in sizes)]
    ext = [np.ascontiguousarray(F[rng.choice(len(F), n, replace=False)]) for n in sizes]
    pts[FAR][-1] = (250.0, -90.0, 40.0)
    splits = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return pts, ext, splits, [s for s in range(len(sizes)) if s != INACTIVE]


def check_sphere_select(dev):
    from ml3d import ops
    pts, _, splits, active = op_clouds()
    rng = np.random.default_rng(8)
    cat = torch.from_numpy(np.concatenate(pts)).to(dev)
    poss = torch.from_numpy(rng.random(int(splits[-1]))).to(dev)
    before = _np(poss).copy()
    for centre_on_far in (False, True):
        idx, _ = ops.possibility_argmin(poss, splits)
        if centre_on_far:
            idx[FAR] = len(pts[FAR]) - 1
        total = int(np.diff(splits)[active].sum())
        out = torch.full((total + 5,), -9, dtype=torch.int32, device=dev)
        cnt = torch.full((len(pts),), -7, dtype=torch.int32, device=dev)
        got = ops.sphere_select(cat, splits, active, idx, RADIUS, out=(out, cnt))
        assert got[0] is out and got[1] is cnt
        out, cnt, c = _np(out), _np(cnt), _np(idx)
        at = 0
        for s in active:
            p1 = torch.from_numpy(pts[s]).to(dev)
            ref = ops.fixed_radius_search(p1, p1[int(c[s]):int(c[s]) + 1].contiguous(), RADIUS)
            row = _np(ref.neighbors_index)
            assert cnt[s] == len(row), (s, cnt[s], len(row))
            assert np.array_equal(out[at:at + len(row)], row), s
            if not (s == FAR and centre_on_far):
                assert 10 <= len(row) <= 700, (s, len(row))
            at += len(row)
        assert np.all(out[at:] == -9), "entries behind the lists must be untouched"
        assert cnt[INACTIVE] == -7, "an inactive slot's count must be untouched"
        if centre_on_far:
            assert cnt[FAR] == 1
        assert np.array_equal(_np(poss), before)
    # fresh outputs; the wrapper's checks
    i2, c2 = ops.sphere_select(cat, splits, None, idx, RADIUS)
    assert i2.numel() == int(splits[-1]) and c2.numel() == len(pts)
    for bad in (lambda: ops.sphere_select(cat, splits, [2, 0], idx, RADIUS), lambda: ops.sphere_select(cat, splits, active, idx[:3], RADIUS),
                lambda: ops.sphere_select(cat, splits, active, idx, -1.0), lambda: ops.sphere_select(cat[:-1], splits, active, idx, RADIUS),
                lambda: ops.sphere_select(cat, splits, active, idx, RADIUS, out=(torch.empty(10, dtype=torch.int32, device=dev), c2))):
        try:
            bad()
        except RuntimeError:
            continue
        raise AssertionError("a bad argument was accepted")


def seq_mean(a):
    """numpy's mean(0) of a C-contiguous float32 [n, 3] array as ml3d_patch_recenter's contract states it: the float32 column sums
    added row by row, divided by n."""
    return np.add.accumulate(a.astype(np.float32), axis=0, dtype=np.float32)[-1] / np.float32(a.shape[0])


def ref_crop(points, poss, extra, centre_index, cand, perm, keep, zero, axes, bias, scale, linear):
    """``KPFCNN._crop_sphere`` + the sampler's bump for one sphere, restated: ``poss`` / ``extra`` are modified in place."""
    centre = points[centre_index].reshape(1, -1)
    picked = cand[perm]
    pc = points[picked]
    dists = np.sum(np.square((pc - centre).astype(np.float32)), axis=1)
    poss[picked] += np.square(1 - dists / np.max(dists))
    sphere = pc - centre
    sphere[:, axes] = sphere[:, axes] - seq_mean(sphere)[axes]
    if linear and extra is not None:
        extra -= np.float32(bias)
        extra /= np.float32(scale)
    columns = sphere.copy() if extra is None else np.hstack((sphere, extra[picked, :]))
    if keep is not None:
        sphere, columns, picked = sphere[keep, :], columns[keep, :], picked[keep]
    if zero:
        columns[:, 3:] *= 0
    return sphere, columns, picked


def check_device_sphere_batch(dev):
    from ml3d import ops
    pts, ext, splits, active = op_clouds()
    rng = np.random.default_rng(9)
    cat_pts = torch.from_numpy(np.concatenate(pts)).to(dev)
    poss0 = [rng.random(len(p)) * 1e-3 for p in pts]
    bias, scale = 3.0, 255.0

    def run(groups, with_keep, zero_on, n_extra, axes, calls=2):
        """``calls`` sub-rounds served by one ``device_sphere_batch`` per group of slots -> per call {slot: outputs}, final state."""
        rs = np.random.default_rng(10)
        poss = torch.from_numpy(np.concatenate(poss0)).to(dev)
        extra = torch.from_numpy(np.concatenate(ext)).to(dev) if n_extra else None
        steps = []
        for call in range(calls):
            idx, _ = ops.possibility_argmin(poss, splits, active)
            cand, cnt = ops.sphere_select(cat_pts, splits, active, idx, RADIUS)
            cnt_h, cand_h, idx_h = _np(cnt), _np(cand), _np(idx)
            offs = dict(zip(active, np.concatenate([[0], np.cumsum(cnt_h[active])])[:-1]))
            draws = {}
            for a, s in enumerate(active):
                n = int(cnt_h[s])
                perm = rs.permutation(n).astype(np.int32)
                keep = rs.choice(n, size=max(1, n // 3), replace=False).astype(np.int32) if with_keep and a != 1 else None
                draws[s] = (perm, keep, bool(zero_on and a != 2))
            got = {}
            for g in groups:
                keeps = [draws[s][1] for s in g if draws[s][1] is not None]
                perm_d = torch.from_numpy(np.concatenate([draws[s][0] for s in g])).to(dev)
                keep_d = torch.from_numpy(np.concatenate(keeps)).to(dev) if keeps else None
                m_a = [-1 if draws[s][1] is None else len(draws[s][1]) for s in g]
                o_pts, o_cols, o_sel, o_row, o_off = ops.device_sphere_batch(
                    cat_pts, poss, splits, g, idx, cand, [offs[s] for s in g], [cnt_h[s] for s in g], perm_d, keep_d,
                    m_a if keeps else None, [draws[s][2] for s in g], axes, extra, bias, scale, True)
                for j, s in enumerate(g):
                    a, b = int(o_off[j]), int(o_off[j + 1])
                    got[s] = tuple(_np(t[a:b]).copy() for t in (o_pts, o_cols, o_sel, o_row))
            steps.append(dict(got=got, draws=draws, centre=idx_h.copy(), cand={s: cand_h[offs[s]:offs[s] + cnt_h[s]].copy() for s in active}))
        return steps, _np(poss).copy(), None if extra is None else _np(extra).copy()

    for with_keep in (False, True):
        for zero_on in (False, True):
            for n_extra in (0, 3):
                for axes in ((), (2,), (0, 1, 2)):               # dims_mask 0 / 4 / 7
                    what = (with_keep, zero_on, n_extra, axes)
                    steps, poss_d, extra_d = run([active], with_keep, zero_on, n_extra, axes)
                    poss_h = [p.copy() for p in poss0]
                    extra_h = [e.copy() for e in ext] if n_extra else [None] * len(pts)
                    for call, st in enumerate(steps):
                        for s in active:
                            perm, keep, zero = st["draws"][s]
                            r_pts, r_cols, r_sel = ref_crop(pts[s], poss_h[s], extra_h[s], int(st["centre"][s]), st["cand"][s].astype(np.int64),
                                                            perm, keep, zero, list(axes), bias, scale, True)
                            g_pts, g_cols, g_sel, g_row = st["got"][s]
                            assert np.array_equal(g_sel, r_sel), (what, call, s)
                            assert np.array_equal(g_row, r_sel + splits[s]), (what, call, s)
                            assert np.array_equal(_bits(g_pts), _bits(r_pts)), (what, call, s)
                            assert g_cols.shape == r_cols.shape and np.array_equal(_bits(g_cols), _bits(r_cols)), (what, call, s)
                            assert len(g_sel) == (len(perm) if keep is None else len(keep))
                        if call == 0 and n_extra:                # after ONE call: every active cloud's colours rescaled once
                            once = [(e - np.float32(bias)) / np.float32(scale) for e in ext]
                            for s in active:
                                assert np.array_equal(_bits(extra_h[s]), _bits(once[s]))
                    for s in range(len(pts)):
                        a, b = int(splits[s]), int(splits[s + 1])
                        assert np.array_equal(poss_d[a:b], poss_h[s]), (what, "possibilities", s)
                        if n_extra:                              # after TWO calls: rescaled twice (the inactive cloud never)
                            assert np.array_equal(_bits(extra_d[a:b]), _bits(extra_h[s])), (what, "colours", s)
                    assert np.array_equal(poss_d[splits[INACTIVE]:splits[INACTIVE + 1]], poss0[INACTIVE])
                    if n_extra:
                        twice = (ext[0] - np.float32(bias)) / np.float32(scale)
                        twice = (twice - np.float32(bias)) / np.float32(scale)
                        assert np.array_equal(_bits(extra_d[:splits[1]]), _bits(twice))
                    # one call serving all clouds == calls serving one cloud at a time
                    alone, poss_1, extra_1 = run([[s] for s in active], with_keep, zero_on, n_extra, axes)
                    for x, y in zip(steps, alone):
                        for s in active:
                            for u, v in zip(x["got"][s], y["got"][s]):
                                assert u.dtype == v.dtype and np.array_equal(u.view(np.uint32), v.view(np.uint32)), (what, s)
                    assert np.array_equal(poss_d, poss_1)
                    assert extra_d is None or np.array_equal(_bits(extra_d), _bits(extra_1))
    # the wrapper's checks: CPU-side shapes
    poss = torch.from_numpy(np.concatenate(poss0)).to(dev)
    idx, _ = ops.possibility_argmin(poss, splits, active)
    cand, cnt = ops.sphere_select(cat_pts, splits, active, idx, RADIUS)
    n0 = int(_np(cnt)[0])
    perm = torch.arange(n0, dtype=torch.int32, device=dev)
    for bad in (lambda: ops.device_sphere_batch(cat_pts, poss, splits, [0], idx, cand, [0], [n0], perm[:-1]),
                lambda: ops.device_sphere_batch(cat_pts, poss, splits, [0], idx, cand, [0], [len(pts[0]) + 1], perm),
                lambda: ops.device_sphere_batch(cat_pts, poss, splits, [0], idx, cand, [cand.numel()], [n0], perm),
                lambda: ops.device_sphere_batch(cat_pts, poss, splits, [0], idx, cand, [0], [n0], perm, perm[:3], [4]),
                lambda: ops.device_sphere_batch(cat_pts, poss.float(), splits, [0], idx, cand, [0], [n0], perm)):
        try:
            bad()
        except RuntimeError:
            continue
        raise AssertionError("a bad argument was accepted")
    assert np.array_equal(_np(poss), np.concatenate(poss0))


# ---- model level -------------------------------------------------------------------------------------------------------------------
# the architecture and widths of the kpconv_small golden's config (kpconv_toronto3d.yml) with the YAML's augmentation keys; spheres
# of 1.3 m on a 0.15 m grid, batches of at least MIN_IN points cut at MAX_IN
MODEL_CFG = dict(synth_weights.TORONTO3D_CFG, in_features_dim=5, first_subsampling_dl=0.12, in_radius=1.0, min_in_points=600,
                 max_in_points=800, batch_limit=800, augment_color=0.8, augment_noise=0.0001, augment_rotation="vertical",
                 augment_scale_anisotropic=False, augment_scale_max=1.1, augment_scale_min=0.9, augment_symmetries=[True, False, False],
                 t_normalize=dict(method="linear", normalize_points=False, feat_bias=0, feat_scale=255))
# the host emulator runs the same architecture at a quarter of the widths (a full-width forward takes it ~12 s)
EMU_CFG = dict(MODEL_CFG, first_features_dim=32)
SEEDS = [201, 202, 203, 204]
FAR_CLOUD = 2


def model_clouds():
    """Four raw clouds with colours, 2 000 .. 6 000 points after the 0.15 m subsampling; cloud FAR_CLOUD carries an isolated point."""
    clouds = []
    for i, (seed, half) in enumerate(((31, 1.3), (32, 1.6), (33, 1.45), (34, 1.8))):
        t = synth_data.toronto3d_tile(seed, half=half, density=0.15)
        c = dict(point=t["point"].copy(), feat=t["feat"].copy(), label=t["label"].copy())
        if i == FAR_CLOUD:
            c["point"][0] = (40.0, 40.0, 12.0)
        clouds.append(c)
    return clouds


def make_model(cfg, dev, weights_seed=6):
    from ml3d.torch.models.kpconv import KPFCNN
    m = KPFCNN(**cfg, device=dev)
    m.load_state_dict(synth_weights.kpconv_state_dict(cfg, weights_seed))
    return m.eval()


def _local(mat, lo, hi, shadow, base):
    """Rows [lo, hi) of a neighbour / pool / upsample matrix with indices made local to the cloud's first sphere: the shadow
    index -> -1, trailing all-shadow columns dropped (the padding width is the longest row of the WHOLE batch)."""
    m = _np(mat[lo:hi]).astype(np.int64)
    m = np.where(m >= shadow, -1, m - base)
    keep = m.shape[1]
    while keep > 0 and np.all(m[:, keep - 1] == -1):
        keep -= 1
    return m[:, :keep]


def record(spheres, batch, logits, into, batches):
    """on_batch: per cloud the list of its batches, each everything the network sees of that cloud's spheres."""
    lens = [_np(l).astype(np.int64) if isinstance(l, torch.Tensor) else np.asarray(l, np.int64) for l in batch.lengths]
    L = len(batch.points)
    clouds = []
    for c, _, _ in spheres:
        if c not in clouds:
            clouds.append(c)
    batches.append([(c, sum(1 for x in spheres if x[0] == c)) for c in clouds])
    lg = _np(logits)
    for c in clouds:
        js = [j for j, x in enumerate(spheres) if x[0] == c]
        assert js == list(range(js[0], js[-1] + 1)) and [spheres[j][2] for j in js] == list(range(len(js)))
        assert len({spheres[j][1] for j in js}) == 1 and spheres[js[0]][1] == len(into.get(c, []))
        rec = dict(lengths=[l[js[0]:js[-1] + 1].copy() for l in lens], spheres=len(js), total=len(spheres))
        lo = [int(l[:js[0]].sum()) for l in lens]
        hi = [int(l[:js[-1] + 1].sum()) for l in lens]
        rec["points"] = [_np(batch.points[l][lo[l]:hi[l]]).copy() for l in range(L)]
        rec["features"] = _np(batch.features[lo[0]:hi[0]]).copy()
        rec["labels"] = _np(batch.labels[lo[0]:hi[0]]).copy()
        rec["sel"] = [np.asarray(_np(x) if isinstance(x, torch.Tensor) else x).astype(np.int64) for x in (batch.reproj_masks[j] for j in js)]
        rec["nbr"] = [_local(batch.neighbors[l], lo[l], hi[l], batch.points[l].shape[0], lo[l]) for l in range(L)]
        rec["pool"] = [_local(batch.pools[l], lo[l + 1], hi[l + 1], batch.points[l].shape[0], lo[l]) for l in range(L - 1)]
        rec["up"] = [_local(batch.upsamples[l], lo[l], hi[l], batch.points[l + 1].shape[0], lo[l + 1]) for l in range(L - 1)]
        rec["logits"] = lg[lo[0]:hi[0]].copy()
        into.setdefault(c, []).append(rec)


def run_single(cfg, dev, cloud, seed, max_batches=None):
    """The single-cloud loop under np.random.seed(seed), to completion or for ``max_batches`` batches -> (result | None, [batch, ...],
    possibilities, proj_inds, retries)."""
    m = make_model(cfg, dev)
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        m.inference_begin(dict(cloud, feat=None if cloud.get("feat") is None else cloud["feat"].copy()))
        tree, queries = m.inference_data["search_tree"], []
        query = tree.query_radius
        tree.query_radius = lambda *a, **k: (queries.append(1), query(*a, **k))[1]       # (counted: queries - spheres = retries)
        got, batches, done = {}, [], False
        while not done and (max_batches is None or len(got.get(0, [])) < max_batches):
            inp = m.inference_preprocess()
            res = m(inp["data"])
            b = inp["data"]
            record([(0, len(got.get(0, [])), o) for o in range(len(b.reproj_masks))], b, res, got, batches)
            done = m.inference_end(inp, res)
        m.single_retries = len(queries) - sum(b["spheres"] for b in got[0])
        return (m.inference_result if done else None), got[0], np.array(m.possibility), np.asarray(m.inference_proj_inds), m.single_retries
    finally:
        np.random.set_state(state)


def same_batch(x, y, what):
    assert x["spheres"] == y["spheres"], (what, "spheres in the batch", x["spheres"], y["spheres"])
    for l, (a, b) in enumerate(zip(x["lengths"], y["lengths"])):
        assert np.array_equal(a, b), (what, "lengths", l)
    assert len(x["sel"]) == len(y["sel"])
    for a, b in zip(x["sel"], y["sel"]):
        assert np.array_equal(a, b), (what, "out_sel")
    for l, (a, b) in enumerate(zip(x["points"], y["points"])):
        assert np.array_equal(_bits(a), _bits(b)), (what, "points", l)
    assert np.array_equal(_bits(x["features"]), _bits(y["features"])), (what, "columns")
    assert np.array_equal(x["labels"], y["labels"]), (what, "labels")
    for name in ("nbr", "pool", "up"):
        for l, (a, b) in enumerate(zip(x[name], y[name])):
            assert a.shape == b.shape and np.array_equal(a, b), (what, name, l)


def replay_votes(dev, mine, n_points, num_classes):
    """The recorded logits of ONE cloud, in sphere order, through ops.vote_update on a fresh accumulator -> float16 votes."""
    from ml3d import ops
    votes = torch.zeros((n_points, num_classes), dtype=torch.float16, device=dev)
    for rec in mine:
        at = 0
        for sel in rec["sel"]:
            ops.vote_update(votes, torch.from_numpy(sel.astype(np.int32)).to(dev), torch.from_numpy(rec["logits"][at:at + len(sel)]).to(dev), 0.95)
            at += len(sel)
    return _np(votes)


class _Stop(Exception):
    pass


def collect(cfg, dev, clouds, seeds, max_in_flight, model=None, max_batches=None):
    """One inference_many run, to completion or (``max_batches``) until every cloud has that many batches, and, per cloud, its
    recorded logits replayed through ops.vote_update."""
    m = make_model(cfg, dev) if model is None else model
    recs, batches = {}, []

    def on_batch(spheres, batch, logits):
        record(spheres, batch, logits, recs, batches)
        if max_batches is not None and len(recs) == len(clouds) and min(len(v) for v in recs.values()) >= max_batches:
            raise _Stop

    results = None
    try:
        results = m.inference_many([dict(c, feat=None if c.get("feat") is None else c["feat"].copy()) for c in clouds], seeds=seeds,
                                   max_in_flight=max_in_flight, on_batch=on_batch)
    except _Stop:
        pass
    info = m.inference_many_info
    votes = {i: replay_votes(dev, mine, len(info[i]["possibility"]), cfg["num_classes"]) for i, mine in recs.items() if info[i] is not None}
    return dict(results=results, recs=recs, batches=batches, info=info, votes=votes, stats=dict(m.inference_many_stats))


def assert_inputs_qualify(singles, cfg):
    """Conditions on the INPUTS, checked on the single-cloud runs: (a) batches of 2 and of 3 spheres occur (a sphere at a tile's
    corner holds a quarter of an interior one's points, so longer batches occur as well), (b) at least one sphere exceeds its budget
    (it is cut), and the isolated point makes its cloud retry."""
    sizes = [b["spheres"] for _, got, *_ in singles.values() for b in got]
    assert {2, 3} <= set(sizes), sorted(set(sizes))
    cap = min(cfg["batch_limit"], cfg["max_in_points"])
    assert any(int(b["lengths"][0].sum()) == cap for _, got, *_ in singles.values() for b in got), "no sphere was cut to its budget"
    assert singles[FAR_CLOUD][4] > 0, "the isolated point never made its cloud retry"


def assert_many_is_single(run, singles, partial=False):
    """``run`` = collect(...), ``singles`` = {cloud: run_single(...)}: the lock-step run IS the single-cloud runs.  ``partial``: both
    were stopped early; the batches both made are compared.  (Logits: assert_logits_within_tolerance.)"""
    for i, (res1, got1, poss1, proj, retries1) in singles.items():
        if i not in run["recs"]:
            continue
        mine, info = run["recs"][i], run["info"][i]
        if not partial:
            assert len(mine) == len(got1) == info["num_batches"], ("number of batches", i, len(mine), len(got1))
            assert info["num_spheres"] == sum(b["spheres"] for b in got1), ("number of spheres", i)
            assert info["retries"] == retries1, ("retries", i, info["retries"], retries1)
        assert min(len(mine), len(got1)) > 0
        for step, (x, y) in enumerate(zip(mine, got1)):
            same_batch(x, y, (i, step))
        if partial:
            continue
        assert info["possibility"].dtype == np.float64 and np.array_equal(info["possibility"], poss1), ("final possibilities", i)
        votes, res = run["votes"][i], run["results"][i]
        assert res["predict_scores"].dtype == np.float16 and votes.dtype == np.float16
        assert np.array_equal(res["predict_scores"].view(np.uint16), votes[proj].view(np.uint16)), i
        assert np.array_equal(res["predict_labels"], np.argmax(votes, 1)[proj]), i
        assert res["predict_labels"].shape == res1["predict_labels"].shape


def assert_logits_within_tolerance(run, singles):
    """Logits of a sphere in the big batch against the same sphere forwarded in its own cloud's batch, within LOGIT_TOL.
    (The reference's ``max_pool`` lets the shadow neighbour's zero row take part in the maximum, so the forward depends on the
    longest pooling row of the whole batch: without ``KPFCNN._pools_of_own_batches`` the same sphere's logits moved by 0.0117 in
    a forward over 9 spheres and by 0.113 over 13, at max|logits| 3.83.)"""
    for i, (res1, got1, *_rest) in singles.items():
        for step, (x, y) in enumerate(zip(run["recs"].get(i, []), got1)):
            err, size = float(np.abs(x["logits"] - y["logits"]).max()), float(np.abs(y["logits"]).max())
            print("cloud %d batch %d: %d spheres in the forward, logits max|d| %.3g at max|ref| %.3g" % (i, step, x["total"], err, size))
            assert err <= LOGIT_TOL, ("logits against the cloud's own batch", x["total"], i, step, err, size)


def assert_same_run(x, y):
    """Two inference_many runs with the same clouds and seeds: identical in everything, logits included, when made alike."""
    assert x["batches"] == y["batches"] and sorted(x["recs"]) == sorted(y["recs"])
    for i in x["recs"]:
        for step, (p, q) in enumerate(zip(x["recs"][i], y["recs"][i])):
            same_batch(p, q, (i, step))
            assert np.array_equal(_bits(p["logits"]), _bits(q["logits"])), (i, step)
        assert np.array_equal(x["info"][i]["possibility"], y["info"][i]["possibility"])
        assert np.array_equal(x["results"][i]["predict_scores"].view(np.uint16), y["results"][i]["predict_scores"].view(np.uint16))
        assert np.array_equal(x["results"][i]["predict_labels"], y["results"][i]["predict_labels"])


def check_fallback(dev, cfg, cloud, seed):
    """A model that must fall back gives the single-cloud result exactly and leaves np.random's global state as it found it."""
    res1, got1, poss1, proj, _ = run_single(cfg, dev, cloud, seed)
    m = make_model(cfg, dev)
    np.random.seed(4321)
    before = np.random.get_state()
    called = []
    res = m.inference_many([dict(cloud, feat=None if cloud.get("feat") is None else cloud["feat"].copy())], seeds=[seed], max_in_flight=2,
                           on_batch=lambda *a: called.append(a))[0]
    after = np.random.get_state()
    assert not called, "the host loop serves this model: no lock-step batch"
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert np.array_equal(res["predict_labels"], res1["predict_labels"])
    assert np.array_equal(res["predict_scores"].view(np.uint16), res1["predict_scores"].view(np.uint16))
    info = m.inference_many_info[0]
    assert info["num_batches"] == len(got1) and np.array_equal(info["possibility"], poss1)
