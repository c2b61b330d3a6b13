"""Shared bodies of the ``ops.vote_project`` tests (ml3d_vote_project: the float16 vote accumulator of a sub-cloud taken through
``proj_inds`` to the full cloud).  tests/test_emulated_vote_project.py runs them on CPU tensors against the host emulation of the HIP
sources, tests/test_gpu_vote_project.py on the MI355X, tests/test_finish_cases_can_fail.py against wrong stand-ins, which every
case that covers a stand-in's edge must reject.

The oracle is numpy -- ``np.argmax(v, 1)[p]`` and ``v[p]`` -- and everything is compared for EQUALITY: labels as integers, scores as
uint16 bit patterns.  Every call writes into outputs cut out of larger sentinel-filled buffers, twice with two different sentinels:
each expected byte must appear under both (so it was written), everything around the outputs must keep the sentinel."""
import numpy as np
import torch

CLASSES = (1, 2, 13, 19, 20, 64, 255, 256)        # odd ones: every second row is 2-byte aligned only; 255 / 256: the uint8 edge
N_SUB = (1, 63, 64, 65, 1000)
N_FULL = (0, 1, 63, 64, 65, 257, 5000)            # tails at both ends of a wave (64) and of a workgroup (128)
GUARD = 64                                        # elements / rows after each output
SENTINELS = ((0xA5, 0x7E5A), (0x3C, 0x81C3))      # (label byte, score bits): a NaN with a payload, a negative subnormal

H_MAX, H_INF, H_NEG_INF, H_NEG_ZERO = 0x7BFF, 0x7C00, 0xFC00, 0x8000
H_NAN_A, H_NAN_B, H_NAN_S = 0x7E01, 0xFE55, 0x7C01          # quiet, quiet negative, SIGNALLING with payload 1
H_SUB_MIN, H_SUB_MAX = 0x0001, 0x03FF                       # subnormals


def _the_op():
    from ml3d import ops
    return ops.vote_project


def halves(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16)


def check(dev, op, v, p, a_in=0, a_out=0, scores=True, what=None):
    """One call of ``op`` on votes ``v`` (float16 [n_sub, C]) and ``p`` (int32 [n_full]) against numpy.  The votes are rows
    [a_in, a_in + n_sub) of a larger buffer, the scores rows [a_out, a_out + n_full) of one, each output has a guard tail."""
    op = op or _the_op()
    v = np.ascontiguousarray(v, dtype=np.float16)
    p = np.ascontiguousarray(p, dtype=np.int32)
    (n_sub, C), n_full = v.shape, p.size
    want_labels = np.argmax(v, 1)[p]
    want_bits = v[p].view(np.uint16).reshape(n_full, C)
    assert want_labels.dtype == np.int64
    whole = np.full((a_in + n_sub + 1, C), 0x7A7A, np.uint16)       # rows in front of and behind the slice: large finite values
    whole[a_in:a_in + n_sub] = v.view(np.uint16)
    votes = torch.from_numpy(whole.view(np.float16)).to(dev)[a_in:a_in + n_sub]
    proj = torch.from_numpy(p).to(dev)
    for lab_s, sc_s in SENTINELS:
        lab_buf = torch.full((n_full + GUARD,), lab_s, dtype=torch.uint8, device=dev)
        sc_host = np.full((a_out + n_full + GUARD, C), sc_s, np.uint16)
        sc_buf = torch.from_numpy(sc_host.view(np.float16)).to(dev)
        out_scores = sc_buf[a_out:a_out + n_full]
        got = op(votes, proj, out_labels=lab_buf[:n_full], out_scores=out_scores, scores=scores)
        labels, sc = got
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n_full,), what
        lab = lab_buf.cpu().numpy()
        assert np.array_equal(labels.cpu().numpy(), lab[:n_full]), what
        assert np.array_equal(lab[:n_full].astype(np.int64), want_labels), ("labels", what, C, n_sub, n_full, a_in, a_out)
        assert (lab[n_full:] == lab_s).all(), ("written past the labels", what, C, n_sub, n_full)
        bits = sc_buf.cpu().numpy().view(np.uint16)
        if scores:
            assert sc.dtype == torch.float16 and tuple(sc.shape) == (n_full, C), what
            assert np.array_equal(sc.cpu().numpy().view(np.uint16).reshape(n_full, C), want_bits), ("returned scores", what)
            assert np.array_equal(bits[a_out:a_out + n_full], want_bits), ("scores", what, C, n_sub, n_full, a_in, a_out)
        else:
            assert sc is None, what
            assert (bits[a_out:a_out + n_full] == sc_s).all(), ("scores=False must leave the scores alone", what)
        assert (bits[:a_out] == sc_s).all() and (bits[a_out + n_full:] == sc_s).all(), ("written around the scores", what, C, n_sub, n_full)
    assert np.array_equal(votes.cpu().numpy().view(np.uint16), v.view(np.uint16)), ("the votes changed", what)


def _votes(rng, n_sub, C):
    """Plausible accumulators: non-negative float16 with distinct entries in most rows, every third row unvisited (all zero)."""
    v = rng.random((n_sub, C)).astype(np.float16)
    v[2::3] = 0
    if C >= 255:
        v[::2, C - 1] = 2.0             # the maximum in the LAST column: labels 254 and 255
    return v


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def case_sizes(dev, op=None):
    """Every C with every (n_sub, n_full): random projections (repeats, unreferenced rows), rows 0 and n_sub - 1 always taken."""
    rng = np.random.default_rng(5)
    for C in CLASSES:
        for n_sub in N_SUB:
            v = _votes(rng, n_sub, C)
            for n_full in N_FULL:
                p = rng.integers(0, n_sub, size=n_full).astype(np.int32)
                if n_full >= 2:
                    p[0], p[-1] = n_sub - 1, 0
                check(dev, op, v, p, what="sizes")


def case_base_offsets(dev, op=None):
    """C = 19: the votes are ``buffer[a:]`` and the scores ``buffer[a:a + n_full]`` for a in {1, 2, 3} -- bases 19, 38, 57 halves into
    their buffers, odd and even half-word offsets -- in every combination of the two."""
    rng = np.random.default_rng(6)
    C = 19
    for a_in in (1, 2, 3):
        for a_out in (1, 2, 3):
            for n_sub, n_full in ((65, 257), (1000, 63), (64, 64), (63, 1)):
                v = _votes(rng, n_sub, C)
                p = rng.integers(0, n_sub, size=n_full).astype(np.int32)
                check(dev, op, v, p, a_in=a_in, a_out=a_out, what="base offsets")


def special_rows(C):
    """Rows [r, C] of float16 bit patterns, one per special value, C >= 4."""
    z = lambda: np.zeros(C, np.uint16)
    one, two, half = 0x3C00, 0x4000, 0x3800
    rows = {}
    rows["all zero (unvisited: label 0)"] = z()
    r = z(); r[[1, C - 1]] = one; rows["tie in 2 columns"] = r
    r = z(); r[[1, 2, C - 1]] = one; rows["tie in 3 columns"] = r
    r = z(); r[:] = half; rows["tie in all columns"] = r
    r = z(); r[:] = H_NEG_ZERO; r[C - 1] = 0; rows["-0 ... -0 +0: equal, the first wins"] = r
    r = z(); r[0] = 0; r[1:] = H_NEG_ZERO; rows["+0 -0 ... -0"] = r
    r = z(); r[:] = H_NEG_ZERO; r[2] = 0; rows["-0 -0 +0 -0 ..."] = r
    r = z(); r[:] = one; r[2] = H_INF; r[C - 1] = H_INF; rows["+inf twice"] = r
    r = z(); r[:] = H_NEG_INF; rows["all -inf"] = r
    r = z(); r[:] = H_NEG_INF; r[C - 1] = 0xFBFF; rows["-inf and the most negative finite"] = r
    r = z(); r[:] = H_MAX; r[1] = H_INF; rows["+inf among the largest finite"] = r
    r = z(); r[0] = one; r[1] = H_NAN_A; r[2] = two; rows["a NaN before the numeric maximum"] = r
    r = z(); r[0] = one; r[1] = two; r[C - 1] = H_NAN_S; rows["a NaN after the numeric maximum"] = r
    r = z(); r[0] = H_INF; r[2] = H_NAN_B; r[3] = H_NAN_A; rows["two NaNs after +inf: the first NaN"] = r
    r = z(); r[:] = H_NAN_S; r[0] = one; rows["NaNs from column 1 on"] = r
    r = z(); r[0] = H_NAN_B; r[1:] = H_INF; rows["a negative NaN first"] = r
    r = z(); r[1] = H_SUB_MIN; r[2] = H_SUB_MAX; r[3] = H_SUB_MAX; rows["subnormals"] = r
    r = z(); r[:] = 0x8001; r[C - 2] = H_NEG_ZERO; rows["negative subnormals and -0"] = r
    r = z(); r[:] = 0x7BFE; r[C - 1] = H_MAX; rows["the largest finite half, last"] = r
    r = z(); r[:] = H_MAX; rows["the largest finite half everywhere"] = r
    return rows


def case_values(dev, op=None):
    """The special rows at C = 19 (odd pitch), 20 and 4, under the identity, a reversal and a projection with repeats."""
    rng = np.random.default_rng(7)
    for C in (19, 20, 4):
        rows = special_rows(C)
        v = halves(np.stack(list(rows.values())))
        n = len(v)
        expect = np.argmax(v, 1)
        names = list(rows)
        assert expect[names.index("tie in 2 columns")] == 1 and expect[names.index("a NaN after the numeric maximum")] == C - 1
        assert expect[names.index("-0 ... -0 +0: equal, the first wins")] == 0 and expect[names.index("two NaNs after +inf: the first NaN")] == 2
        for p in (np.arange(n), np.arange(n)[::-1], rng.integers(0, n, size=5 * n)):
            check(dev, op, v, p, what="values")


def case_projections(dev, op=None):
    rng = np.random.default_rng(8)
    C, n_sub = 19, 200
    v = _votes(rng, n_sub, C)
    v[:, 0] = 0                                                  # (no row's label is 0 by accident: an unprojected answer differs)
    for name, p in (("identity", np.arange(n_sub)),
                    ("all indices equal", np.full(300, 77)),
                    ("all indices the last row", np.full(129, n_sub - 1)),
                    ("a permutation", rng.permutation(n_sub)),
                    ("n_full > n_sub, heavy repeats", rng.integers(0, 7, size=3000) * 28),
                    ("n_full < n_sub, most rows unreferenced", np.array([199, 0, 5, 5, 198])),
                    ("rows 0 and n_sub - 1 only", np.array([0, n_sub - 1] * 40))):
        check(dev, op, v, p, what=name)


def case_labels_only(dev, op=None):
    """scores=False: the same labels, and a scores buffer that was passed in stays as it was."""
    rng = np.random.default_rng(9)
    for C, n_sub, n_full in ((19, 65, 257), (256, 64, 65), (1, 63, 64)):
        v = _votes(rng, n_sub, C)
        check(dev, op, v, rng.integers(0, n_sub, size=n_full), a_in=1, a_out=1, scores=False, what="labels only")
    op = op or _the_op()
    labels, none = op(torch.from_numpy(v).to(dev), torch.zeros(3, dtype=torch.int32, device=dev), scores=False)
    assert none is None and labels.dtype == torch.uint8 and labels.cpu().tolist() == [0, 0, 0]
    labels, sc = op(torch.from_numpy(v).to(dev), torch.zeros(0, dtype=torch.int32, device=dev))
    assert tuple(labels.shape) == (0,) and tuple(sc.shape) == (0, 1) and sc.dtype == torch.float16


def case_python_checks(dev, op=None):
    op = op or _the_op()
    v = torch.zeros((8, 19), dtype=torch.float16, device=dev)
    p = torch.zeros(5, dtype=torch.int32, device=dev)
    wide = torch.zeros((8, 40), dtype=torch.float16, device=dev)
    bad = (lambda: op(v.float(), p),                                                      # wrong dtypes
           lambda: op(v, p.long()),
           lambda: op(v, p, out_labels=torch.zeros(5, dtype=torch.int32, device=dev)),
           lambda: op(v, p, out_scores=torch.zeros((5, 19), dtype=torch.float32, device=dev)),
           lambda: op(wide[:, :19], p),                                                    # non-contiguous
           lambda: op(v, torch.zeros(10, dtype=torch.int32, device=dev)[::2]),
           lambda: op(v, p, out_scores=wide[:5, :19]),
           lambda: op(v, p, out_labels=torch.zeros(4, dtype=torch.uint8, device=dev)),       # wrong sizes
           lambda: op(v, p, out_scores=torch.zeros((5, 20), dtype=torch.float16, device=dev)),
           lambda: op(torch.zeros((8, 257), dtype=torch.float16, device=dev), p),            # C = 257
           lambda: op(torch.zeros((0, 19), dtype=torch.float16, device=dev), p))             # n_sub == 0 with n_full > 0
    for i, f in enumerate(bad):
        try:
            f()
        except RuntimeError:
            continue
        raise AssertionError("bad argument %d was accepted" % i)
    labels, sc = op(v, p)                                           # ... and the good call next to them
    assert labels.cpu().tolist() == [0] * 5 and not sc.cpu().numpy().view(np.uint16).any()


# ---- model level: inference_many(finish="device") against finish="host", the single-cloud loops against the host formula ------------
def _same_results(x, y, what):
    assert len(x) == len(y)
    for i, (a, b) in enumerate(zip(x, y)):
        assert a is not None and b is not None, (what, i)
        assert a["predict_labels"].dtype == b["predict_labels"].dtype == np.int64, (what, i, a["predict_labels"].dtype)
        assert a["predict_scores"].dtype == b["predict_scores"].dtype == np.float16, (what, i)
        assert a["predict_labels"].shape == b["predict_labels"].shape and a["predict_scores"].shape == b["predict_scores"].shape
        assert np.array_equal(a["predict_labels"], b["predict_labels"]), (what, "labels", i)
        assert np.array_equal(a["predict_scores"].view(np.uint16), b["predict_scores"].view(np.uint16)), (what, "scores", i)


def _same_info(x, y, what):
    for i, (a, b) in enumerate(zip(x, y)):
        assert sorted(a) == sorted(b)
        for key in a:
            if key == "possibility":
                assert a[key].dtype == b[key].dtype == np.float64 and np.array_equal(a[key], b[key]), (what, "possibility", i)
            else:
                assert a[key] == b[key], (what, key, i)


def _snapshot(results, info):
    return ([{k: v.copy() for k, v in r.items()} for r in results], [dict(d, possibility=d["possibility"].copy()) for d in info])


def randla_setup(dev):
    """(model factory, clouds, seeds): the four small clouds and the two-layer network of tests/multicloud_cases.py."""
    import multicloud_cases as M
    in_ch, aug = M.AUGMENTS[1]
    cfg = dict(M.SMALL, in_channels=in_ch, augment=aug, grid_size=M.SMALL_GRID)
    clouds, seeds = M.small_clouds()
    return (lambda **kw: M.make_model(cfg, dev, **kw)), M.with_features(clouds, in_ch), seeds


def kpconv_setup(dev, base_cfg):
    """(model factory, clouds, seeds): the network of tests/kpconv_multicloud_cases.py (``base_cfg``: its MODEL_CFG or EMU_CFG) on
    four sparse tiles of a few hundred points after a 0.4 m subsampling, with spheres that hold most of a tile: every cloud
    finishes after a handful of batches, which keeps a run to completion within the emulator's reach."""
    import kpconv_multicloud_cases as K
    import synth_data
    cfg = dict(base_cfg, first_subsampling_dl=0.4, in_radius=3.0, min_in_points=150, max_in_points=400, batch_limit=400)
    clouds = []
    for seed, half, density in ((41, 1.0, 0.03), (42, 1.3, 0.04), (43, 1.1, 0.02), (44, 1.2, 0.03)):
        t = synth_data.toronto3d_tile(seed, half=half, density=density)
        clouds.append(dict(point=t["point"].copy(), feat=t["feat"].copy(), label=t["label"].copy()))
    return (lambda: K.make_model(cfg, dev)), clouds, K.SEEDS


def check_finish_device_equals_host(model, clouds, seeds, in_flight):
    """``inference_many(finish="device")`` == ``inference_many(finish="host")`` on the same model, clouds and seeds: labels, scores
    (bits), dtypes, possibilities and counters.  Then the device run again: the FIRST run's arrays, which must own their memory,
    still hold what they held (a reused staging buffer or device buffer would show) and the run repeats itself."""
    dev_res = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, finish="device")
    dev_info = model.inference_many_info
    kept_res, kept_info = _snapshot(dev_res, dev_info)
    for r, d in zip(dev_res, dev_info):
        for arr in (r["predict_labels"], r["predict_scores"], d["possibility"]):
            assert arr.base is None and arr.flags.owndata and arr.flags.writeable, "a result must own its memory"
    host_res = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, finish="host")
    host_info = model.inference_many_info
    _same_results(dev_res, host_res, "device against host")
    _same_info(dev_info, host_info, "device against host")
    again = model.inference_many(clouds, seeds=seeds, max_in_flight=in_flight, finish="device")
    _same_results(dev_res, kept_res, "the first run's results after two more runs")
    _same_info(dev_info, kept_info, "the first run's info after two more runs")
    _same_results(again, kept_res, "the device run repeated")
    for i, c in enumerate(clouds):
        assert dev_res[i]["predict_labels"].shape == (len(c["point"]),)
        assert dev_res[i]["predict_scores"].shape == (len(c["point"]), int(model.cfg.num_classes))
    return dev_res, dev_info


def check_single_cloud_finish(model, cloud):
    """The ``inference_begin ... inference_end`` loop to completion: its result is the host formula on its own ``test_probs`` and
    ``inference_proj_inds``, dtypes included."""
    model.inference_begin(dict(cloud))
    while True:
        inp = model.inference_preprocess()
        if model.inference_end(inp, model(inp["data"])):
            break
    probs = model.test_probs.cpu().numpy()
    proj = np.asarray(model.inference_proj_inds)
    res = model.inference_result
    assert probs.dtype == np.float16 and probs.any() and len(proj) == len(cloud["point"])
    want_labels, want_scores = np.argmax(probs, 1)[proj], probs[proj]
    assert sorted(res) == ["predict_labels", "predict_scores"]
    assert res["predict_labels"].dtype == want_labels.dtype == np.int64 and res["predict_scores"].dtype == np.float16
    assert np.array_equal(res["predict_labels"], want_labels)
    assert np.array_equal(res["predict_scores"].view(np.uint16), want_scores.view(np.uint16))
    # a tree that came out of a pickle carries no device copy of the projection: one upload, the same result
    model._inference_proj_dev = None
    from ml3d.torch.models._multicloud import finish_cloud
    res2 = finish_cloud(model.test_probs, proj)
    assert np.array_equal(res2["predict_labels"], want_labels)
    assert np.array_equal(res2["predict_scores"].view(np.uint16), want_scores.view(np.uint16))


def check_bad_finish(model, clouds, seeds):
    for bad in ("gpu", None, "Device", 1):
        try:
            model.inference_many(clouds, seeds=seeds, max_in_flight=2, finish=bad)
        except ValueError as e:
            assert "finish" in str(e)
            continue
        raise AssertionError("finish=%r was accepted" % (bad,))


def check_pickled_tree_takes_one_upload(dev):
    """``CloudSlots`` with a state that carries no ``proj_dev`` (its tree came out of a pickle): the device retire uploads the host
    indices once and hands over the same result as the host retire; with ``proj_dev`` it never looks at ``proj_inds``."""
    from ml3d.torch.models._multicloud import CloudSlots
    C, rows = 19, (70, 131, 64)

    def run(finish, with_dev):
        g = np.random.default_rng(13)
        clouds = []
        for i, n in enumerate(rows):
            proj = g.integers(0, n, size=3 * n + 1).astype(np.int32)
            st = dict(cloud=i, n=n, proj_inds=proj if not with_dev else None, points=torch.zeros((n, 3), device=dev),
                      possibility=torch.from_numpy(g.random(n)).to(dev), label=torch.zeros(n, dtype=torch.int32, device=dev), feat=None)
            if with_dev:
                st["proj_dev"] = torch.from_numpy(proj).to(dev)
            clouds.append(st)
        waiting, gone = iter(clouds), {}
        t = CloudSlots(2, lambda: next(waiting, None), lambda st, res, poss: gone.__setitem__(st["cloud"], (res, poss)), torch.device(dev), C,
                       finish)
        for step, slot in enumerate((1, 0, 1)):              # cloud 1 retires while 0 is active; 2 is admitted: a rebuild follows
            v = _votes(np.random.default_rng(20 + step), int(t.splits[-1]), C)
            t.buf["votes"].copy_(torch.from_numpy(v).to(dev))
            t.replace_finished([slot])
        t.drain()
        assert sorted(gone) == [0, 1, 2] and not t._pending
        return gone
    host = run("host", False)
    for with_dev in (False, True):
        got = run("device", with_dev)
        for i in host:
            _same_results([got[i][0]], [host[i][0]], ("slots", with_dev, i))
            assert np.array_equal(got[i][1], host[i][1]) and got[i][1].base is None


CASES = dict(sizes=case_sizes, base_offsets=case_base_offsets, values=case_values, projections=case_projections,
             labels_only=case_labels_only, python_checks=case_python_checks)
