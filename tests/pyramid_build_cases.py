"""Case table of the k-NN pyramid's grid builders (csrc/grid.hip: the one-workgroup-per-cloud builder and the launch chain), shared
by tests/test_gpu_pyramid_build.py (MI355X) and tests/test_emulated_pyramid_build.py (host emulator).  Not a test module.

A case is a [B, n0, 3] batch and the sub-sampling ratios.  ``check`` compares what a pyramid call returned with the oracle, bit
for bit: every level's 16-NN rows, every level's 1-NN interpolation index into the next level, and -- the grids' own output --
that each level's tile order is, cloud by cloud, a permutation of that cloud's rows.  The search is exact on any grid, so equal
indices do not prove equal grids; what they prove is that every point sits in the cell the search looks for it in, that the
cell-start words delimit it, and that no point was lost or doubled.  The oracle's answer is computed once per shape and kept."""
import functools

import numpy as np

import synth_data
from oracle import ops as oops

K = 16
# knn.hip: the one-workgroup-per-cloud builder serves calls of at least MIN_BATCH_FUSED clouds of at most MAX_N0_FUSED points,
# the launch chain everything else
MIN_BATCH_FUSED = 48
MAX_N0_FUSED = 131072


def _mixed(n0):
    """Five kinds of cloud side by side, so neighbouring workgroups see very different grids and base offsets."""
    rng = np.random.default_rng(77)
    cube = rng.uniform(-5.0, 5.0, (n0, 3))
    plane = rng.uniform(-20.0, 20.0, (n0, 3))
    plane[:, 2] = 1.25                                            # one zero extent
    same = np.tile(np.array([[3.0, -2.0, 0.5]]), (n0, 1))           # every extent zero
    outlier = rng.normal(0.0, 1.0, (n0, 3))
    outlier[n0 // 3] = (1.0e4, 1.0e4, 1.0e4)
    half = rng.uniform(-3.0, 3.0, (n0 // 2, 3))
    dup = np.concatenate([half, half])[rng.permutation(n0)]       # every point twice
    return np.stack([cube, plane, same, outlier, dup]).astype(np.float32)


def _patches(first, B, n0):
    return np.stack([synth_data.semantickitti_patch(first + i, n0) for i in range(B)]).astype(np.float32)


# name: (distinct clouds, ratios, batch).  The batch repeats the distinct clouds in turn (cloud b = distinct[b % len]); the oracle runs
# once per distinct cloud.  The first six are the shapes at their smallest; at these batch sizes the library's path choice hands all
# but `many_clouds` to the launch chain, so each shape comes again with at least MIN_BATCH_FUSED clouds, which the one-workgroup
# builder serves.
_SHAPES = {
    # levels 4096, 1024, 256, 64: the last one takes the n <= 64 one-cell branch
    "four_levels": (lambda: _patches(40, 3, 4096), [4, 4, 4, 4], 3),
    # sizes that divide no workgroup size; levels floor to 2500, 625, 156, 39 (next would be 9)
    "odd_sizes": (lambda: _patches(50, 2, 2500), [4, 4, 4, 4], 2),
    # probe stride 4 (n0 >= 8192) and 16 (n0 >= 32768)
    "probe_stride_4": (lambda: _patches(60, 2, 8192), [4, 4], 2),
    "probe_stride_16": (lambda: _patches(62, 2, 32768), [4, 4], 2),
    "mixed_clouds": (lambda: _mixed(4096), [4, 4, 4, 4], 5),
    "one_cloud": (lambda: _patches(70, 1, 4096), [4, 4, 4, 4], 1),
}
CASES = dict(_SHAPES)
# more workgroups than CUs
CASES["many_clouds"] = (lambda: np.stack([synth_data.uniform_cloud(900 + i, 1024) for i in range(300)]).astype(np.float32), [4, 4], 300)
for _name, (_make, _ratios, _b) in _SHAPES.items():
    CASES[_name + "_fused"] = (_make, _ratios, -(-MIN_BATCH_FUSED // _b) * _b)
# the limits themselves: one cloud short of the batch bound, and clouds just above the size bound -- the launch chain serves both
CASES["below_min_batch"] = (lambda: _patches(75, 1, 1024), [4, 4], MIN_BATCH_FUSED - 1)
CASES["above_max_n0"] = (lambda: _patches(80, 1, MAX_N0_FUSED + 4), [4, 4], MIN_BATCH_FUSED)
# (the host emulator runs every case but the 6 million points of the last)
EMULATED = tuple(sorted(c for c in CASES if c != "above_max_n0"))
FUSED = tuple(sorted(c for c in CASES if CASES[c][2] >= MIN_BATCH_FUSED and c != "above_max_n0"))


def sizes(n0, ratios):
    n = [n0]
    for r in ratios:
        n.append(n[-1] // r)
    return n


@functools.lru_cache(maxsize=None)
def _distinct(make):
    pts = np.ascontiguousarray(make()[..., :3], np.float32)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _reference(make, ratios):
    pts = _distinct(make)
    D, n0, _ = pts.shape
    n = sizes(n0, ratios)
    ref = []
    for l in range(len(ratios)):
        nb = np.stack([oops.knn_search(pts[d, :n[l]], pts[d, :n[l]], K) for d in range(D)])
        if n[l + 1] > 0:
            it = np.stack([oops.knn_search(pts[d, :n[l + 1]], pts[d, :n[l]], 1).reshape(-1) for d in range(D)])
        else:
            it = np.full((D, n[l]), -1, np.int32)
        nb.setflags(write=False)
        it.setflags(write=False)
        ref.append((nb, it))
    return ref


def case(name):
    """-> (points [B, n0, 3], ratios, reference): reference[l] = (neighbours [D, n_l, K], interpolation [D, n_l]) of the D distinct
    clouds, cloud b of the batch being distinct cloud b % D.  The reference is computed once per shape and shared, read-only."""
    make, ratios, B = CASES[name]
    d = _distinct(make)
    return d[np.arange(B) % d.shape[0]], list(ratios), _reference(make, tuple(ratios))


def _up(x):
    return (x + 255) & ~255


GRID_SEG_WORDS = 21          # grid.h GridSeg: 21 four-byte fields
SEG_DIMS, SEG_CELL_BASE, SEG_N, SEG_SORTED_BASE = slice(6, 9), 9, 10, 11


def emulated_grids(name):
    """One pyramid call on the host emulator with the workspace kept: -> {key: array} of the results AND of the grids as a search
    sees them, per level l: ``segs<l>`` the GridSeg records as words, ``starts<l>`` the cell-start words of every cloud's read
    range [cell_base, cell_base + ncells], ``members<l>`` the point indices of the cell-sorted array ordered by (cell, index) --
    order inside a cell is arrival order and not part of a grid's identity.  The offsets restate grid_ws / pyramid_ws (grid.hip,
    knn.hip); a record's ``n`` field is checked against the level size, so a layout that moved fails here and not silently."""
    import ctypes as C

    import emu
    from ml3d import _abi
    pts, ratios, _ = case(name)
    pts = np.ascontiguousarray(pts)
    L = emu.lib()
    B, n0, _ = pts.shape
    nl = len(ratios)
    n = sizes(n0, ratios)
    r = (C.c_int32 * nl)(*ratios)
    wsb = L.ml3d_randla_pyramid_workspace_bytes(B, n0, nl, r)
    buf = np.zeros(wsb + 256, np.uint8)
    skew = (-buf.ctypes.data) % 256
    ws = buf[skew:skew + wsb]
    nbr = [np.full((B, n[l], K), -9, np.int32) for l in range(nl)]
    itp = [np.full((B, n[l], 1), -9, np.int32) for l in range(nl)]
    order = [np.full(B * n[l], -9, np.int32) for l in range(nl)]
    rc = L.ml3d_randla_knn_pyramid_ordered(pts.ctypes.data, B, n0, nl, r, K, _abi.ptr_table([x.ctypes.data for x in nbr]),
                                           _abi.ptr_table([x.ctypes.data for x in itp]),
                                           _abi.ptr_table([x.ctypes.data for x in order]), ws.ctypes.data, wsb, None, None)
    assert rc == 0, rc
    out = {}
    at = 0
    for l in range(nl):
        out["nbr%d" % l], out["itp%d" % l], out["order%d" % l] = nbr[l], itp[l], order[l]
        if n[l] == 0:
            continue
        nt = n[l] * B
        tc = 8 * nt + 64 * B
        o_segs = at
        o_bitmap = o_segs + _up(4 * GRID_SEG_WORDS * B) + _up(24 * B) + _up(20 * B)
        o_cells = o_bitmap + _up(4 * 5 * ((tc + 31) // 32 + B))
        o_sorted = o_cells + _up(4 * (tc + 2)) + _up(4 * ((tc + 2 + 1023) // 1024 + 1))
        segs = ws[o_segs:o_segs + 4 * GRID_SEG_WORDS * B].view(np.int32).reshape(B, GRID_SEG_WORDS)
        assert np.all(segs[:, SEG_N] == n[l]) and np.all(segs[:, SEG_SORTED_BASE] == np.arange(B) * n[l]), (name, l, "workspace layout")
        cells = ws[o_cells:o_cells + 4 * (tc + 2)].view(np.int32)
        sorted_w = ws[o_sorted:o_sorted + 16 * nt].view(np.int32).reshape(nt, 4)[:, 3]
        starts, members = [], []
        for b in range(B):
            ncells = int(np.prod(segs[b, SEG_DIMS].astype(np.int64)))
            cs = cells[segs[b, SEG_CELL_BASE]:segs[b, SEG_CELL_BASE] + ncells + 1]
            assert cs[0] == b * n[l] and cs[-1] == (b + 1) * n[l] and np.all(np.diff(cs) >= 0), (name, l, b, "cell starts")
            cell_of_slot = np.repeat(np.arange(ncells), np.diff(cs))
            idx = sorted_w[b * n[l]:(b + 1) * n[l]]
            members.append(idx[np.lexsort((idx, cell_of_slot))])
            starts.append(cs)
        out["segs%d" % l] = segs.copy()
        out["starts%d" % l] = np.concatenate(starts)
        out["members%d" % l] = np.concatenate(members)
        at += _up(L.ml3d_knn_workspace_bytes(nt, 0, B)) + 256         # (pyramid_ws: the nested grid, then 256 bytes of slack)
    return out


def check(name, nbr, itp, order):
    """nbr[l] [B, n_l, K], itp[l] [B, n_l, 1], order[l] [B * n_l]: numpy arrays of one pyramid call on case ``name``."""
    pts, ratios, ref = case(name)
    B, n0, _ = pts.shape
    n = sizes(n0, ratios)
    which = np.arange(B) % ref[0][0].shape[0]
    for l in range(len(ratios)):
        assert np.array_equal(np.asarray(nbr[l]), ref[l][0][which]), (name, "neighbours", l)
        assert np.array_equal(np.asarray(itp[l]).reshape(B, n[l]), ref[l][1][which]), (name, "interpolation", l)
        o = np.asarray(order[l]).reshape(B, n[l]).astype(np.int64)
        rows = np.arange(B, dtype=np.int64)[:, None] * n[l] + np.arange(n[l], dtype=np.int64)[None, :]
        assert np.array_equal(np.sort(o, axis=1), rows), (name, "tile order", l)
