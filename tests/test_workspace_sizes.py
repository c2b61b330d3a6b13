"""Workspace sizes and workspace checks of libml3d_hip, on the host emulation of the library.

(a) Every ml3d_*_workspace_bytes entry returns what tests/golden/workspace_sizes.json records.  Python allocates exactly these
    numbers, so they are observable behaviour; the table was recorded from the commit BEFORE the layouts moved to csrc/workspace.h:
        python tests/test_workspace_sizes.py --record [out.json]
    run in a checkout of that commit rewrites the table from the library built there.
(b) One op of each group runs in a buffer of exactly workspace_bytes whose start lies 8 bytes past a 256-byte boundary (so the
    alignment slack is really used) and gives what it gives in a generous buffer; one byte less is ML3D_E_WORKSPACE.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "workspace_sizes.json")
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "open3d-ml_amd")]

import emu  # noqa: E402
from ml3d import _abi  # noqa: E402

E_WORKSPACE = -2
N13 = [0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 45056, 1200000]
BATCH = [1, 2, 63, 64]
RAD_LDS_ROW, SCN_MAX_LEVELS, NMSB_MAX, KP_K = 256, 12, 4096, 15
RANDLA_CFGS = {
    "kitti4": dict(num_layers=4, in_channels=3, dim_features=8, num_classes=19, num_neighbors=16, dim_output=[16, 64, 128, 256],
                   sub_sampling_ratio=[4, 4, 4, 4]),
    "s3dis5": dict(num_layers=5, in_channels=6, dim_features=8, num_classes=13, num_neighbors=16, dim_output=[16, 64, 128, 256, 512],
                   sub_sampling_ratio=[4, 4, 4, 4, 2]),
}


def cases():
    """(entry, [arguments]) for every size entry of the ABI; an int32 array argument is a list, a RandLA descriptor
    [config name, batch, points]."""
    out = []
    add = lambda name, *a: out.append(("ml3d_%s_workspace_bytes" % name, list(a)))
    for n in N13:
        for b in BATCH:
            add("knn", n, n, b)
            for nq in (n, 257):
                for total in (0, 1, 16 * nq):
                    add("radius", n, nq, b, total)
            for cap in (1, 40, RAD_LDS_ROW):
                add("radius_dense", n, n, b, cap)
            add("voxelize", n, b)
            add("subsample", n, b)
            for layers, cap in ((1, 1), (5, 40), (_abi.KPBATCH_MAX_LAYERS, RAD_LDS_ROW)):
                add("kpconv_batch", n, b, layers, cap)
            for k in (0, 1, 1024, 45056):
                add("patch_batch", n, b, k)
            for ratios in ([4, 4, 4, 4, 2], [1]):
                add("randla_pyramid", b, n, len(ratios), ratios)
            add("fps", n, b)
            add("avg_voxelize", b, n)
            for c in (1, 64, 1024):
                add("segment_max_rows", b, n, c)
                add("randla_attention_stage_backward", b, n, c, 2 * c)
        if n > 0:          # (the shared GEMM's split-K sizing divides by the row count: zero rows are not a case of these three)
            for cin, cout in ((1, 1), (64, 128), (512, 512)):
                add("kpconv", n, cin, cout, KP_K)
            for nn, k in ((1, 1), (64, 128), (512, 1024)):
                add("linear", n, nn, k)
                add("linear_bf16x3", n, nn, k)
        for p in (1, 32, 100):
            for units in ([64], [32, 64], [64, 64, 128, 128]):
                add("pillar_features", n, p, len(units), units)
        add("nms", n)
        for rows in [0] + BATCH:
            for k in (0, 1, 100, NMSB_MAX):
                add("topk_rows", rows, n, k)              # (k > n: 0)
            add("sphere_select", n, rows)
            add("sphere_batch", rows, n)
        add("nearest_to_center", n)
        for clouds in (0, 1, 2, 63, 64, 256):
            add("possibility_argmin", n, clouds)
        for levels in (1, 7, SCN_MAX_LEVELS):
            add("scn_build", n, levels)
    for b in [0] + BATCH:
        for k in (0, 1, 100, NMSB_MAX):
            for nc in (1, 3):
                add("pp_boxes", b, k, nc)
        for oh, ow in ((1, 1), (31, 33), (248, 216)):
            for cin, cout, kh, kw in ((1, 1, 1, 1), (64, 128, 3, 3), (384, 64, 1, 1)):
                if b > 0:
                    add("conv2d", b, oh, ow, cin, cout, kh, kw)
        for name in RANDLA_CFGS:
            for n in (0, 1024, 2048, 4096, 45056):
                add("randla_forward", [name, b, n])
    for c in (0, 1, 8, 255, 256, 1024):
        add("batchnorm_train", c)
    # arguments an entry answers with 0
    add("knn", 1024, 1024, 0)
    add("radius", -1, 10, 1, 0), add("radius", 10, -1, 1, 0), add("radius", 10, 10, 0, 0), add("radius", 10, 10, 1, -1)
    add("radius_dense", 10, 10, 1, 0), add("radius_dense", 10, 10, 1, RAD_LDS_ROW + 1), add("radius_dense", 10, 10, 0, 8)
    add("voxelize", -1, 1), add("voxelize", 10, 0), add("subsample", -1, 1), add("subsample", 10, 0)
    add("kpconv_batch", 10, 1, 0, 8), add("kpconv_batch", 10, 1, _abi.KPBATCH_MAX_LAYERS + 1, 8), add("kpconv_batch", 10, 1, 2, 0)
    add("kpconv_batch", 10, 1, 2, RAD_LDS_ROW + 1), add("kpconv_batch", 10, 0, 2, 8), add("kpconv_batch", -1, 1, 2, 8)
    add("kpconv", 10, 8, 8, KP_K - 1), add("kpconv", 10, 0, 8, KP_K), add("kpconv", 10, 8, 0, KP_K), add("kpconv", -1, 8, 8, KP_K)
    add("pillar_features", 10, 0, 1, [64]), add("pillar_features", 10, 32, 0, [64]), add("pillar_features", -1, 32, 1, [64])
    add("nms", -1), add("nearest_to_center", -1)
    add("topk_rows", 1, 100, NMSB_MAX + 1), add("topk_rows", -1, 100, 10), add("topk_rows", 1, 10, 11)
    add("pp_boxes", 1, NMSB_MAX + 1, 3), add("pp_boxes", 1, 10, 0), add("pp_boxes", -1, 10, 3)
    add("possibility_argmin", -1, 3), add("possibility_argmin", 10, -1)
    add("patch_batch", -1, 1, 1), add("patch_batch", 10, -1, 5), add("patch_batch", 10, 1, -1)
    add("sphere_select", -1, 1), add("sphere_select", 10, -1), add("sphere_batch", -1, 10), add("sphere_batch", 1, -1)
    add("randla_pyramid", 1, 1024, 0, [4]), add("randla_pyramid", 1, 1024, 9, [2] * 9), add("randla_pyramid", 1, 1024, 2, [4, 0])
    add("fps", -1, 1), add("fps", 10, 0), add("avg_voxelize", 0, 10), add("avg_voxelize", 1, 0)
    add("segment_max_rows", 0, 10, 8), add("segment_max_rows", 1, 0, 8), add("segment_max_rows", 1, 10, 0)
    add("scn_build", 0, 3), add("scn_build", 10, 0), add("scn_build", 10, SCN_MAX_LEVELS + 1)
    return out


def call(L, name, args):
    if name == "ml3d_randla_forward_workspace_bytes":
        cfg, b, n = args[0]
        return int(L.ml3d_randla_forward_workspace_bytes(C.byref(_abi.make_desc(RANDLA_CFGS[cfg], b, n))))
    keep = [(C.c_int32 * len(a))(*a) if isinstance(a, list) else a for a in args]
    return int(getattr(L, name)(*keep))


def measure():
    L = emu.lib()
    table = {}
    for name, args in cases():
        table.setdefault(name, []).append([args, call(L, name, args)])
    return table


needs_emu = pytest.mark.skipif(not emu.available(), reason="host compiler for the emulated library missing")


@needs_emu
def test_every_size_entry_returns_the_recorded_bytes():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = measure()
    bound = sorted(s for s in _abi.SYMBOLS if s.startswith("ml3d_") and s.endswith("_workspace_bytes"))
    assert sorted(got) == bound == sorted(want), "every size entry bound in _abi.py is covered"
    for name in bound:
        assert [a for a, _ in got[name]] == [a for a, _ in want[name]], name + ": the table is stale (--record)"
        bad = [(a, w, g) for (a, w), (_, g) in zip(want[name], got[name]) if w != g]
        assert not bad, "%s: %d of %d sizes changed, e.g. args %s: %d -> %d" % ((name, len(bad), len(want[name])) + bad[0])
        assert any(w > 0 for _, w in want[name]), name


# ---- (b) exact fit, one byte short -------------------------------------------------------------------------------------------------
def _buffer(nbytes):
    """-> (owner, address): `nbytes` usable bytes starting 8 bytes past a 256-byte boundary"""
    raw = np.zeros(int(nbytes) + 512, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data) % 256 + 8


def _clouds(seed, n0=150, n1=113, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n0 + n1, 3)) * scale).astype(np.float32), np.array([0, n0, n0 + n1], np.int64)


def _knn(L):
    pts, rs = _clouds(1)
    n, k = len(pts), 8

    def run(ws, wsb):
        idx, d2 = np.full((n, k), -7, np.int32), np.zeros((n, k), np.float32)
        rc = L.ml3d_knn_search(pts.ctypes.data, rs.ctypes.data, pts.ctypes.data, rs.ctypes.data, 2, n, n, k, 0, idx.ctypes.data,
                               d2.ctypes.data, ws, wsb, None)
        return rc, [idx, d2]
    return L.ml3d_knn_workspace_bytes(n, n, 2), run


def _radius(L):
    """count and fill in ONE workspace sized for the result (no spill buffer): the fill is the call that needs all of it"""
    pts, rs = _clouds(2)
    n, r = len(pts), 0.25
    idx0, rs0 = emu.radius(pts, rs, pts, rs, r)
    total = len(idx0)
    assert total > n

    def run(ws, wsb):
        splits, stats, idx = np.zeros(n + 1, np.int64), np.zeros(2, np.int64), np.full(total, -5, np.int32)
        rc = L.ml3d_radius_count(pts.ctypes.data, rs.ctypes.data, pts.ctypes.data, rs.ctypes.data, 2, n, n, r, splits.ctypes.data,
                                 stats.ctypes.data, ws, wsb, None)
        if rc == 0:
            assert stats[0] == total
            rc = L.ml3d_radius_fill(pts.ctypes.data, rs.ctypes.data, pts.ctypes.data, rs.ctypes.data, 2, n, n, r, splits.ctypes.data,
                                    total, 0, 0, n, idx.ctypes.data, None, ws, wsb, None, 0, None)
        return rc, [splits, idx]
    return L.ml3d_radius_workspace_bytes(n, n, 2, total), run


def _voxelize(L):
    pts, rs = _clouds(3, scale=4.0)
    n = len(pts)
    vs, lo, hi = np.full(3, 0.5, np.float32), np.zeros(3, np.float32), np.full(3, 4.0, np.float32)

    def run(ws, wsb):
        bs, stats = np.zeros(3, np.int64), np.zeros(2, np.int64)
        rc = L.ml3d_voxelize_count(pts.ctypes.data, 3, rs.ctypes.data, 2, n, vs.ctypes.data, lo.ctypes.data, hi.ctypes.data, 2**62,
                                   2**62, bs.ctypes.data, stats.ctypes.data, ws, wsb, None)
        if rc:
            return rc, []
        coords, pidx, prs = np.full((stats[0], 3), -1, np.int32), np.full(stats[1], -1, np.int64), np.full(stats[0] + 1, -1, np.int64)
        rc = L.ml3d_voxelize_fill(2, n, vs.ctypes.data, lo.ctypes.data, hi.ctypes.data, 2**62, 2**62, bs.ctypes.data,
                                  coords.ctypes.data, pidx.ctypes.data, prs.ctypes.data, ws, wsb, None)
        return rc, [bs, stats, coords, pidx, prs]
    return L.ml3d_voxelize_workspace_bytes(n, 2), run


def _avg_voxelize(L):
    rng = np.random.default_rng(4)
    b, n, c, r = 2, 130, 5, 4
    feat = rng.random((b * n, c)).astype(np.float32)
    vox = rng.integers(0, r ** 3, b * n).astype(np.int32)

    def run(ws, wsb):
        raw = np.full(b * r ** 3 * c + 8, 7.0, np.float32)
        grid = raw[(-raw.ctypes.data) % 16 // 4:][:b * r ** 3 * c]              # (the op wants a 16-byte aligned grid)
        rc = L.ml3d_avg_voxelize(feat.ctypes.data, c, c, vox.ctypes.data, b, n, r, grid.ctypes.data, c, ws, wsb, None)
        return rc, [grid]
    return L.ml3d_avg_voxelize_workspace_bytes(b, n), run


def _scn_build(L):
    rng = np.random.default_rng(5)
    levels, g, c, pitch = 2, 16, 3, 4
    rs = np.array([0, 120, 200], np.int64)
    n = int(rs[-1])
    pts = (rng.integers(0, g, (n, 3)) + 0.5).astype(np.float32)
    feat = rng.random((n, c)).astype(np.float32)

    def run(ws, wsb):
        i32 = lambda *shape: np.full(shape, -9, np.int32)
        outs = [i32(levels), i32(levels, n, 4), i32(levels, n, 27), i32(levels, n, 8), i32(levels, n), i32(levels, n), i32(levels, n, 8),
                i32(n), np.zeros((n, pitch), np.float32)]
        rc = L.ml3d_scn_build(pts.ctypes.data, feat.ctypes.data, c, c, n, rs.ctypes.data, 2, levels, g, *[o.ctypes.data for o in outs[:8]],
                              outs[8].ctypes.data, pitch, ws, wsb, None)
        return rc, outs
    return L.ml3d_scn_build_workspace_bytes(n, levels), run


def _nms(L):
    rng = np.random.default_rng(6)
    n = 150
    boxes = np.concatenate([rng.random((n, 2)) * 10, 1 + rng.random((n, 2)) * 2, rng.random((n, 1)) * 3], 1).astype(np.float32)
    scores = rng.random(n).astype(np.float32)

    def run(ws, wsb):
        keep, cnt = np.full(n, -1, np.int64), np.zeros(1, np.int64)
        rc = L.ml3d_nms(boxes.ctypes.data, scores.ctypes.data, n, 0.3, keep.ctypes.data, cnt.ctypes.data, ws, wsb, None)
        return rc, [keep, cnt]
    return L.ml3d_nms_workspace_bytes(n), run


def _possibility_argmin(L):
    rng = np.random.default_rng(7)
    splits, active = np.array([0, 100, 180, 300], np.int64), np.array([0, 2], np.int32)
    poss = rng.random(300)

    def run(ws, wsb):
        idx, val = np.full(2, -1, np.int32), np.zeros(2, np.float64)
        rc = L.ml3d_possibility_argmin(poss.ctypes.data, splits.ctypes.data, 3, active.ctypes.data, 2, idx.ctypes.data, val.ctypes.data,
                                       ws, wsb, None)
        return rc, [idx, val]
    return L.ml3d_possibility_argmin_workspace_bytes(220, 2), run         # (the op sizes by the points of the ACTIVE clouds)


@needs_emu
@pytest.mark.parametrize("op", [_knn, _radius, _voxelize, _avg_voxelize, _scn_build, _nms, _possibility_argmin],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_exact_fit_runs_and_one_byte_short_is_refused(op):
    need, run = op(emu.lib())
    assert need > 0
    own, roomy = _buffer(need + 4096)
    rc, want = run(roomy, need + 4096)
    assert rc == 0, rc
    own, exact = _buffer(need)
    rc, got = run(exact, need)
    assert rc == 0, rc
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    rc, _ = run(exact, need - 1)
    assert rc == E_WORKSPACE, rc


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    table = measure()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in sorted(table.items())) + "\n}\n")
    print("%s: %d entries, %d sizes" % (path, len(table), sum(len(v) for v in table.values())))
