"""Shared bodies of the RandLA forward's per-kernel tests (csrc/randla.hip through ``ops.randla_forward`` with precomputed index
tables, the way tests/emu.py::randla_forward drives the emulator), like tests/gemm_cases.py and tests/pt_cases.py:
tests/test_emulated_randla_paths.py runs the rows of at most about 2 000 rows per level on CPU tensors against the host
emulation, tests/test_gpu_randla_paths.py all of them on the MI355X, tests/test_randla_cases_can_fail.py shows on the CPU that
the bound of every row, at the shape the card runs it at, rejects a faulty layer.  Every body takes the device and a ``report`` callback that receives the
MEASURED figures of each float comparison before it is asserted.

The one tolerance is ``pt_cases.judge``: the reference is ``oracle.randlanet_ref.forward`` in FLOAT64 (state dict, coordinates and
features cast to double), ``e32`` the distance of the same function in float32 from it at the case's own inputs; a case passes
within max(1e-5, 4 e32), and that bound never exceeds the 1e-4 of tests/test_gpu_randlanet.py.  The kernel's own output is never
the yardstick.  Everything else (a tile order, two runs, other clouds beside a cloud, a workspace of NaN bytes, refusals) is
compared for EQUALITY, bit for bit.

LOCALISED: each attention width is the LAST encoder layer of a one- or two-layer net, so that nothing deep dilutes an error of
the layer under test (in the four-layer net a lost bf16 plane of layer 3 moves the logits by 1.1e-5, a tenth of the end-to-end
tolerance).  Each row of CASES states the dispatch class it is meant to reach; the class is DERIVED by ``plan`` from a
restatement of the host rules of randla.hip (next to the constants they use) and asserted before anything runs, so that a changed
shape or rule that leaves its class fails here and not silently.  Grid caps that depend on the CU count use the device's count
(the emulator's hipDeviceGetAttribute answers 4)."""
import functools
import os
import time

import numpy as np
import torch

import synth_data
from oracle import ops as oops
from oracle import randlanet_ref as R
from pt_cases import _print, judge, same_bits

# ---- constants of randla.hip ---------------------------------------------------------------------------------------------------------
RK = 16                                           # neighbours per point
LFA_THREADS = 256                                 # lfa_stage: TP = max(1, 256 / D) points per tile
LFA_GRID = 8192                                   # launch_lfa's grid cap, in tiles
LFA_LDS_MAX = 160 * 1024
ATTN16_GRID, A16_TP = 4096, 16                    # launch_attn_mfma16
ATTN_MFMA_WIDTHS = (16, 32, 64, 128, 256)
MFMA_TP = {128: 4, 256: 2}                        # MfmaCfg<D>::TP (attn_mfma_fits)
B3_TP = {128: (8, 8), 256: (4, 2)}                # B3Cfg<D, STAGE>::TP: ML3D_B3_TP256_S1 = 4, _S2 = 2
WAVE_W = {32: 16, 64: 12}                         # waves (= 2-point tiles in flight) per workgroup of lfa_attn_wave / _wave_b3
ATTN_B3, LIN_B3_MINK, CHAIN_B3 = 3, 256, 1        # the build-time switches at their defaults
LIN_SHAPES = {(16, 8): "ShapeLin16x8", (8, 8): "ShapeLin8x8", (64, 32): "ShapeLin64x32", (32, 32): "ShapeLin32x32",
              (32, 64): "ShapeLin32x64"}
EMU_CUS = 4                                       # tests/hipemu/include/hip/hip_runtime.h
TOL_CAP = 1e-4


def cdiv(a, b):
    return (a + b - 1) // b


def fuse_rows():
    """64 * 1024 in the product; the emulator build reads ML3D_RANDLA_FUSE_ROWS (tests/test_emulated_randla_paths.py, second pass)."""
    return int(os.environ.get("ML3D_RANDLA_FUSE_ROWS", str(64 * 1024)))


def device_cus(dev):
    dev = torch.device(dev)
    return torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else EMU_CUS


def levels(n0, ratios):
    n = [int(n0)]
    for r in ratios:
        n.append(n[-1] // r)
    return n


# ---- the host rules of randla.hip, restated -----------------------------------------------------------------------------------------
def xcd_chunk_tiles(tiles, batch):
    if batch <= 0 or tiles < 64:
        return 0
    nch = batch
    while nch < 32:
        nch *= 2
    return cdiv(tiles, nch)


def attn_mfma_fits(dd, m, n0, n):
    return dd in ATTN_MFMA_WIDTHS and m < 2 ** 30 and n0 < 2 ** 30 and (dd <= 64 or n >= MFMA_TP[dd])


def split_rule(dd, m):
    return 32 <= dd <= 256 and m * dd * 4 < 2 ** 32 and m < 2 ** 30


def b3_attn_rule(dd, m, n):
    return (ATTN_B3 & 1) != 0 and split_rule(dd, m) and dd in B3_TP and n >= B3_TP[dd][0]


def epi16_rule(dd, d_in):
    return dd == 16 and d_in == 8


def lfa_smem_bytes(dd, stage, d_in):
    tp = max(1, LFA_THREADS // dd)
    f = tp * (dd * 20 + 4) * (2 if stage == 2 else 1) + tp * RK * 12 + tp * dd
    if stage == 2:
        f += tp * dd + tp * ((d_in + 3) & ~3)
    return f * 4 + tp * RK * 4


def walk(tiles, grid, tiles_per_wg, chunk):
    """TileWalk::next of the attention kernels: every worker slot's tiles -> (most tiles one slot takes); every tile exactly once."""
    seen = np.zeros(tiles, np.int32)
    most = 0
    if chunk == 0:
        step = grid * tiles_per_wg
        for s in range(min(step, tiles)):
            seen[s::step] += 1
        most = cdiv(tiles, step)
    else:
        assert grid % 8 == 0
        step = (grid // 8) * tiles_per_wg
        for xcd in range(8):
            own = [c * chunk + j for c in range(xcd, cdiv(tiles, chunk), 8) for j in range(chunk)]   # positions, holes included
            for s in range(min(step, len(own))):
                mine = [t for t in own[s::step] if t < tiles]
                most = max(most, len(mine))
                seen[mine] += 1
    assert int(seen.min()) == 1 and int(seen.max()) == 1, "a tile is skipped or visited twice"
    return most


def attn_launch(name, m, n, batch, tp, tiles_per_wg, cap, remap=True):
    """launch_attn_tiles (remap) or launch_lfa -> the geometry of one stage."""
    tiles = cdiv(m, tp)
    grid = min(cdiv(tiles, tiles_per_wg), cap)
    chunk = xcd_chunk_tiles(tiles, batch) if remap else 0
    if chunk:
        grid = (grid + 7) & ~7
    return dict(kernel=name, tp=tp, tiles=tiles, grid=grid, chunk=chunk, chunks=cdiv(tiles, chunk) if chunk else 0,
                remainder=bool(chunk) and tiles % chunk != 0, partial=m % tp != 0, straddle=batch > 1 and n % tp != 0,
                most=walk(tiles, grid, tiles_per_wg, chunk))


def attention_stages(dd, d_in, batch, n, n0, cus):
    """The two attention launches of a layer of width dd -> [stage 1, stage 2] (None: no kernel for this width)."""
    m = batch * n
    if attn_mfma_fits(dd, m, n0, n):
        if dd == 16:
            name = "lfa_attn_mfma16<%s>" % ("EPI" if epi16_rule(dd, d_in) else "no EPI")
            return [attn_launch(name, m, n, batch, A16_TP, 1, ATTN16_GRID)] * 2
        split = split_rule(dd, m)
        if dd <= 64:
            if dd == 64 and (ATTN_B3 & 2) and split:
                name = "lfa_attn_wave_b3<64>"
            else:
                name = "lfa_attn_wave<%d, %s>" % (dd, "SPLIT" if split else "no SPLIT")
            return [attn_launch(name, m, n, batch, 2, WAVE_W[dd], cus)] * 2
        if b3_attn_rule(dd, m, n):
            return [attn_launch("lfa_attn_b3<%d>" % dd, m, n, batch, B3_TP[dd][s], 1, cus) for s in (0, 1)]
        return [attn_launch("lfa_attn_pf<%d, %s>" % (dd, "SPLIT" if split else "no SPLIT"), m, n, batch, MFMA_TP[dd], 1, 2560)] * 2
    if dd not in (8, 16, 32, 64, 128, 256, 512) or max(lfa_smem_bytes(dd, 1, d_in), lfa_smem_bytes(dd, 2, d_in)) > LFA_LDS_MAX:
        return None
    return [attn_launch("lfa_stage<%d>" % dd, m, n, batch, max(1, LFA_THREADS // dd), 1, LFA_GRID, remap=False)] * 2


def linear_class(m, c0, c1, cout, fuse, gather=False, bias2=False):
    """launch_linear_auto's order: a shape-compiled per-wave kernel (from ``fuse`` rows on), the bf16x3 tile GEMM, the f32 tile
    GEMM, linear_act.  (Where the bf16x3 GEMM answers ML3D_E_UNSUPPORTED the f32 tile GEMM runs instead: no shape the rule
    below lets through is refused by it, and the kernel trace of profiles/randla_gpu_tests.md shows none.)"""
    if c1 == 0 and m >= fuse and (c0, cout) in LIN_SHAPES:
        return "mlp_wave_s<%s>" % LIN_SHAPES[(c0, cout)]
    k = c0 + c1
    if LIN_B3_MINK > 0 and not gather and c0 % 32 == 0 and c1 % 32 == 0 and k >= LIN_B3_MINK and cout % 4 == 0:
        return "gemm_rows_bf16x3" + (" a2 bias2" if bias2 else "")
    if k >= 8:
        return "gemm_rows" + (" a2" if c1 else "") + (" bias2" if bias2 else "") + (" gather" if gather else "")
    return "linear_act"


def fc1_matches(shape, c0, c1, classes, gathered_rows_per_item=None):
    """mlp_shape_matches<ShapeDecFc1 | ShapeFc1> for the chains the forward builds."""
    if classes > 32:
        return False
    if shape == "ShapeDecFc1":
        return (c0, c1) == (32, 32) and gathered_rows_per_item >= 32
    return (c0, c1) == (32, 0)


def plan(cfg, batch, n0, cus, fuse=None):
    """Every launch of ml3d_randla_forward_ordered in order -> [(tag, kernel, geometry | None)]; None when the forward refuses.
    ``fuse``: the row threshold of the fused per-point kernels (None: fuse_rows())."""
    fuse = fuse_rows() if fuse is None else fuse
    lin = lambda m, c0, c1, cout, **kw: linear_class(m, c0, c1, cout, fuse, **kw)
    nl, dims, ratios = cfg["num_layers"], cfg["dim_output"], cfg["sub_sampling_ratio"]
    n = levels(n0, ratios)
    if cfg["num_neighbors"] != RK or n[nl] < 1 or n[nl - 1] < RK or any(d < 2 or d % 2 for d in dims):
        return None
    ops = []
    head = cfg["dim_features"] == 8 and dims[0] == 16
    if head:
        ops.append(("fc0+mlp1", "head_fc0_mlp1", None))
    else:
        ops.append(("fc0", lin(batch * n0, cfg["in_channels"], 0, cfg["dim_features"]), None))
    d_in = cfg["dim_features"]
    for l, dd in enumerate(dims):
        m, h = batch * n[l], dd // 2
        if not (l == 0 and head):
            ops.append(("mlp1.%d" % l, lin(m, d_in, 0, h), None))
        st = attention_stages(dd, d_in, batch, n[l], n0, cus)
        if st is None:
            return None
        if st[0]["kernel"].startswith("lfa_stage"):
            ops += [("attn1.%d" % l, st[0]["kernel"], st[0]), ("attn2.%d" % l, st[1]["kernel"], st[1])]
        else:
            epi, split = epi16_rule(dd, d_in), split_rule(dd, m)
            if split:
                ops.append(("gscore1.%d" % l, lin(m, h, 0, dd), None))
            ops.append(("attn1.%d" % l, st[0]["kernel"], st[0]))
            if not epi:
                ops.append(("pool1.%d" % l, lin(m, dd, 0, h), None))
            if split:
                ops.append(("gscore2.%d" % l, lin(m, h, 0, dd), None))
            ops.append(("attn2.%d" % l, st[1]["kernel"], st[1]))
            if not epi:
                if m >= fuse and (dd, d_in) == (64, 32):                  # chain_compiled: ShapeEnc64 (ShapeEnc16 = the epilogue's shape)
                    ops.append(("pool2+mlp2.%d" % l, ("mlp_chain_b3" if CHAIN_B3 else "mlp_wave_s") + "<ShapeEnc64>", None))
                else:
                    ops.append(("pool2.%d" % l, lin(m, dd, 0, dd), None))
                    ops.append(("mlp2.%d" % l, lin(m, dd, d_in, 2 * dd, bias2=True), None))
        c2 = 2 * dd
        ok4 = c2 % 4 == 0 and c2 // 4 <= 256 and n[l] * c2 < 2 ** 32 and batch < 65536
        ops.append(("pool.%d" % l, "gather_max4" if ok4 else "gather_max", None))
        d_in = c2
    ops.append(("mlp", lin(batch * n[nl], d_in, 0, d_in), None))
    ed = R.encoder_dims(cfg)
    cprev, chain = d_in, "mlp_chain_b3" if CHAIN_B3 else "mlp_wave_s"
    for i in range(nl):
        lev, skip = nl - 1 - i, ed[nl - 1 - i]
        if i == nl - 1 and fc1_matches("ShapeDecFc1", skip, cprev, cfg["num_classes"], n[lev]):
            ops.append(("dec+fc1", chain + "<ShapeDecFc1>", None))
            return ops
        if n[lev] >= 64 and skip % 4 == 0 and cprev % 4 == 0 and skip >= 8:
            ops.append(("dec.%d" % i, "gemm_rows up + gemm_rows item-local gathered residual", None))
        else:
            ops.append(("dec.%d" % i, lin(batch * n[lev], skip, cprev, skip, gather=True), None))
        cprev = skip
    if fc1_matches("ShapeFc1", cprev, 0, cfg["num_classes"]):
        ops.append(("fc1", chain + "<ShapeFc1>", None))
    else:
        m = batch * n0
        ops.append(("fc1", " + ".join(lin(m, a, 0, b) for a, b in ((cprev, 64), (64, 32), (32, cfg["num_classes"]))), None))
    return ops


# ---- the nets: the width under test is the last encoder layer -----------------------------------------------------------------------
def net(dim_features, dim_output, ratios=None, in_channels=3, num_classes=5):
    ratios = list(ratios) if ratios else [4] * len(dim_output)
    return dict(num_neighbors=RK, num_layers=len(dim_output), num_classes=num_classes, sub_sampling_ratio=ratios,
                in_channels=in_channels, dim_features=dim_features, dim_output=list(dim_output))


# name -> (cfg, attention kernel of the last layer, {tag: kernel} of per-point launches below fuse_rows, the same from fuse_rows on)
NETS = {
    "stage8": (net(8, [8]), "lfa_stage<8>", {"fc0": "linear_act", "mlp1.0": "gemm_rows", "mlp": "gemm_rows"}, {}),
    "stage512": (net(64, [512]), "lfa_stage<512>", {"fc0": "linear_act", "mlp": "gemm_rows_bf16x3"}, {}),
    "stage512_after256": (net(32, [256, 512], [4, 2]), "lfa_stage<512>",
                          {"mlp2.0": "gemm_rows_bf16x3 a2 bias2", "mlp1.1": "gemm_rows_bf16x3", "mlp": "gemm_rows_bf16x3"}, {}),
    "mfma16_epi": (net(8, [16]), "lfa_attn_mfma16<EPI>", {"fc0+mlp1": "head_fc0_mlp1"}, {"fc0+mlp1": "head_fc0_mlp1"}),
    "mfma16_epi_c6": (net(8, [16], in_channels=6, num_classes=7), "lfa_attn_mfma16<EPI>", {"fc0+mlp1": "head_fc0_mlp1"}, {}),
    "mfma16_epi_fc40": (net(8, [16], num_classes=40), "lfa_attn_mfma16<EPI>", {"fc1": "gemm_rows + gemm_rows + gemm_rows"},
                        {"fc1": "mlp_wave_s<ShapeLin32x64> + mlp_wave_s<ShapeLin64x32> + gemm_rows"}),
    "mfma16": (net(16, [16], in_channels=4), "lfa_attn_mfma16<no EPI>",
               {"fc0": "linear_act", "mlp1.0": "gemm_rows", "pool1.0": "gemm_rows", "mlp2.0": "gemm_rows a2 bias2"},
               {"fc0": "linear_act", "mlp1.0": "mlp_wave_s<ShapeLin16x8>", "pool1.0": "mlp_wave_s<ShapeLin16x8>",
                "mlp2.0": "gemm_rows a2 bias2"}),
    "wave32": (net(8, [32]), "lfa_attn_wave<32, SPLIT>", {"fc0": "linear_act", "gscore1.0": "gemm_rows", "mlp2.0": "gemm_rows a2 bias2"}, {}),
    # 8 input channels: fc0 is an 8 -> 8 Linear outside the head (the one caller of ShapeLin8x8)
    "wave32_c8": (net(8, [32], in_channels=8), "lfa_attn_wave<32, SPLIT>", {"fc0": "gemm_rows"}, {"fc0": "mlp_wave_s<ShapeLin8x8>"}),
    "wave_b3_64": (net(32, [64]), "lfa_attn_wave_b3<64>",
                   {"mlp1.0": "gemm_rows", "gscore1.0": "gemm_rows", "pool1.0": "gemm_rows", "pool2.0": "gemm_rows",
                    "mlp2.0": "gemm_rows a2 bias2"},
                   {"mlp1.0": "mlp_wave_s<ShapeLin32x32>", "gscore1.0": "mlp_wave_s<ShapeLin32x64>",
                    "gscore2.0": "mlp_wave_s<ShapeLin32x64>", "pool1.0": "mlp_wave_s<ShapeLin64x32>",
                    "pool2+mlp2.0": "mlp_chain_b3<ShapeEnc64>"}),
    "b3_128": (net(128, [128]), "lfa_attn_b3<128>", {"fc0": "linear_act", "mlp2.0": "gemm_rows_bf16x3 a2 bias2", "mlp": "gemm_rows_bf16x3"}, {}),
    "b3_256": (net(64, [256]), "lfa_attn_b3<256>", {"mlp2.0": "gemm_rows_bf16x3 a2 bias2", "mlp": "gemm_rows_bf16x3"}, {}),
}

# ---- the rows: (net, situation, B, points per cloud, expectations) --------------------------------------------------------------------
# n = ("cap", k): just above a grid cap of cus * k rows = (cus * k // B + 3) | 1 points per cloud (odd: the last tile is partial and
# tiles straddle clouds), at least 17.  Expectations: remap (exact), and, where stated, chunks / remainder / partial / straddle /
# second (some worker takes a second tile) / dec (kernel of the last decoder stage) / fc1.
SPLIT_DEC = "gemm_rows up + gemm_rows item-local gathered residual"
DIRECT_DEC = "gemm_rows a2 gather"


def _rows(name, ragged_n, one_cloud_n, loop, ragged_dec, remap=True, scale=1, tiny_dec=DIRECT_DEC, **tiny):
    """The five situations of one attention class (``ordered`` runs inside every row: check_case)."""
    rows = [(name, "tiny", 1, 16 * scale, dict(remap=False, dec=tiny_dec, **tiny)),                 # every neighbour row lists the whole cloud
            (name, "tiny2", 3, 23 * scale, dict(remap=False, straddle=True, partial=True, dec=tiny_dec, **tiny)),   # < 64 tiles: remap off
            (name, "ragged", 3, ragged_n, dict(remap=remap, partial=True, straddle=True, dec=ragged_dec, **({"remainder": True} if remap else {})))]
    if remap:
        rows.append((name, "remap1", 1, one_cloud_n, dict(remap=True, chunks_max=32, straddle=False)))
    if loop is not None:
        rows.append((name, "loop", loop[0], loop[1], dict(second=True, partial=True, straddle=True)))
    return rows


FC1, DECFC1 = "mlp_chain_b3<ShapeFc1>", "mlp_chain_b3<ShapeDecFc1>"
CASES = (
    _rows("stage8", 275, None, (3, 87383), SPLIT_DEC, remap=False) +            # loop: 262 149 rows = 8193 tiles of 32 > 8192
    _rows("stage512", 34, None, (3, 2733), DIRECT_DEC, remap=False) +           # loop: 8199 tiles of one point
    _rows("stage512_after256", 136, None, None, SPLIT_DEC, remap=False, scale=4, tiny_dec=SPLIT_DEC) +   # level 1: 34 points per cloud, d_in = 512
    _rows("mfma16_epi", 343, 1029, (8, 8197), DECFC1, fc1=FC1) +                # loop: 65 576 rows = 4099 tiles of 16 > 4096, >= fuse_rows
    _rows("mfma16", 343, 1029, (8, 8197), DECFC1, fc1=FC1) +
    _rows("wave32", 275, 131, (3, ("cap", 32)), SPLIT_DEC) +
    _rows("wave_b3_64", 275, 131, (3, ("cap", 24)), SPLIT_DEC) +
    _rows("b3_128", 275, 517, (3, ("cap", 8)), SPLIT_DEC) +
    _rows("b3_256", 89, 261, (3, ("cap", 4)), SPLIT_DEC) +
    [("mfma16_epi_c6", "ragged", 3, 343, dict(remap=True, partial=True, straddle=True, dec=DECFC1)),
     ("mfma16_epi_fc40", "ragged", 3, 343, dict(remap=True, dec=SPLIT_DEC)),
     # the fused per-point kernels of levels of >= 65 536 rows: 65 576 rows leave a partial 32-row tile (8 rows) and 8197 % 32 != 0
     # puts a cloud boundary inside a tile
     ("wave_b3_64", "fused", 8, 8197, dict(remap=True, fused=True)),
     ("wave32_c8", "ragged", 3, 275, dict(remap=True, partial=True, straddle=True, dec=SPLIT_DEC)),
     ("wave32_c8", "fused", 8, 8197, dict(remap=True, fused=True))])
CASE_IDS = ["%s-%s" % (c[0], c[1]) for c in CASES]
KNN_MAX_ROWS = 12000                               # above: seeded in-range index tables (the forward accepts any)
EMU_MAX_ROWS = 2100


def case_points(case, cus):
    n = case[3]
    if isinstance(n, tuple):
        n = max(17, (((cus + 7) & ~7) * n[1] // case[2] + 3) | 1)       # (the remap rounds a grid up to the 8 XCDs)
    return n


def emulated(case):
    """The rows the host emulator can afford (nothing else is decided here): at most about 2 000 rows per level; of the two-layer net (7 to 9 s per emulated forward:
    a 256-wide layer in front of the 512-wide one) only the ragged row."""
    if case[0] == "stage512_after256" and case[1] != "ragged":
        return False
    return case[2] * case_points(case, EMU_CUS) <= EMU_MAX_ROWS


def derive(case, cus):
    """plan() of the row + its stated expectations, asserted -> (cfg, B, n0, ops)."""
    name, situation, batch, _, want = case
    cfg, kernel, lin, lin_fused = NETS[name]
    n0 = case_points(case, cus)
    ops = plan(cfg, batch, n0, cus)
    assert ops is not None, (name, situation)
    by_tag = {t: (k, g) for t, k, g in ops}
    last = cfg["num_layers"] - 1
    m_last = batch * levels(n0, cfg["sub_sampling_ratio"])[last]
    fused = m_last >= fuse_rows()
    assert fused or not want.get("fused"), (name, situation, m_last)
    for tag, k in (lin_fused if (fused and lin_fused) else lin).items():
        assert by_tag[tag][0] == k, (name, situation, tag, by_tag[tag][0], k)
    for s in (1, 2):
        k, g = by_tag["attn%d.%d" % (s, last)]
        assert k == kernel, (name, situation, k, kernel)
        assert bool(g["chunk"]) == want.get("remap", bool(g["chunk"])), (name, situation, s, g)
        for key in ("remainder", "partial", "straddle"):
            if key in want and not (g["tp"] == 1 and key != "remainder"):        # (one-point tiles are never partial)
                assert g[key] == want[key], (name, situation, s, key, g)
        if "chunks_max" in want:
            assert batch < g["chunks"] <= want["chunks_max"], (name, situation, g)
        if want.get("second"):
            assert g["most"] >= 2, (name, situation, s, g)
    dec = [k for t, k, _ in ops if t.startswith("dec")][-1]
    assert dec == want.get("dec", dec), (name, situation, dec)
    if "fc1" in want:
        assert by_tag["fc1"][0] == want["fc1"], (name, situation, by_tag["fc1"][0])
    return cfg, batch, n0, ops


def kernels_of(case, cus):
    return [k for _, k, _ in derive(case, cus)[3]]


# ---- inputs and references ---------------------------------------------------------------------------------------------------------
def _seed(case):
    return CASES.index(case) + 1 if case in CASES else 99


@functools.lru_cache(maxsize=2)
def _inputs(name, batch, n0, seed):
    """-> (state dict, points [B, n0, 3], features, neighbour tables, interpolation tables), numpy, per level [B, n_l, 16 | 1]."""
    cfg = NETS[name][0]
    sd = R.make_state_dict(cfg, 100 + seed)
    pts = synth_data.uniform_cloud(seed, batch * n0).reshape(batch, n0, 3)
    rng = np.random.default_rng(seed)
    c = cfg["in_channels"]
    feats = pts.copy() if c == 3 else np.concatenate([pts, rng.random((batch, n0, c - 3), dtype=np.float32)], 2)
    n = levels(n0, cfg["sub_sampling_ratio"])
    if batch * n0 <= KNN_MAX_ROWS:
        inp = R.build_inputs(pts, feats, cfg, oops.knn_search)
        nbr = [np.ascontiguousarray(x.numpy().astype(np.int32)) for x in inp["neighbor_indices"]]
        itp = [np.ascontiguousarray(x.numpy().astype(np.int32)) for x in inp["interp_idx"]]
    else:
        nbr = [rng.integers(0, n[l], (batch, n[l], RK), dtype=np.int32) for l in range(cfg["num_layers"])]
        itp = [rng.integers(0, n[l + 1], (batch, n[l], 1), dtype=np.int32) for l in range(cfg["num_layers"])]
    for l in range(cfg["num_layers"]):
        assert nbr[l].shape == (batch, n[l], RK) and 0 <= nbr[l].min() and nbr[l].max() < n[l]
        assert itp[l].shape == (batch, n[l], 1) and 0 <= itp[l].min() and itp[l].max() < n[l + 1]
    return sd, pts, feats, nbr, itp


def oracle_inputs(cfg, pts, feats, nbr, itp, clouds=None, dtype=torch.float64):
    """The dict oracle.randlanet_ref.forward takes, for the clouds ``clouds`` (all: None)."""
    sel = slice(None) if clouds is None else clouds
    n = levels(pts.shape[1], cfg["sub_sampling_ratio"])
    nl = cfg["num_layers"]
    return {"coords": [torch.from_numpy(pts[sel, :n[l]]).to(dtype) for l in range(nl)],
            "neighbor_indices": [torch.from_numpy(nbr[l][sel].astype(np.int64)) for l in range(nl)],
            "sub_idx": [torch.from_numpy(nbr[l][sel, :n[l + 1]].astype(np.int64)) for l in range(nl)],
            "interp_idx": [torch.from_numpy(itp[l][sel].astype(np.int64)) for l in range(nl)],
            "features": torch.from_numpy(feats[sel]).to(dtype)}


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def oracle(cfg, sd, pts, feats, nbr, itp, dtype):
    """oracle.randlanet_ref.forward in ``dtype``, cloud by cloud (clouds are independent: the float64 intermediates of one
    cloud stay below a few hundred MB at every shape of CASES)."""
    s = cast_sd(sd, dtype)
    per_cloud = pts.shape[0] * pts.shape[1] > EMU_MAX_ROWS
    if not per_cloud:
        return R.forward(s, cfg, oracle_inputs(cfg, pts, feats, nbr, itp, None, dtype))
    return torch.cat([R.forward(s, cfg, oracle_inputs(cfg, pts, feats, nbr, itp, slice(b, b + 1), dtype)) for b in range(pts.shape[0])])


@functools.lru_cache(maxsize=4)
def _references(name, batch, n0, seed):
    """(float64, float32) logits of the oracle: computed once per row, shared by the tests that need them, never modified."""
    cfg = NETS[name][0]
    sd, pts, feats, nbr, itp = _inputs(name, batch, n0, seed)
    t = time.time()
    r64 = oracle(cfg, sd, pts, feats, nbr, itp, torch.float64)
    r32 = oracle(cfg, sd, pts, feats, nbr, itp, torch.float32)
    return r64, r32, time.time() - t


def bound_of(r64, r32):
    e32 = float((r32.double() - r64).abs().max())
    tol = max(1e-5, 4.0 * e32)
    assert tol <= TOL_CAP, ("the bound would exceed the end-to-end tolerance", e32)
    return e32, tol


# ---- running the forward -------------------------------------------------------------------------------------------------------------
def tile_orders(cfg, batch, n0, kind, seed=4):
    """Cloud-major orders of every level, reversed or seeded-random, as test_randla_forward_with_a_tile_order_is_bit_identical."""
    rng = np.random.default_rng(seed)
    out = []
    for n in levels(n0, cfg["sub_sampling_ratio"])[:-1]:
        o = np.arange(batch * n, dtype=np.int32).reshape(batch, n)
        o = o[:, ::-1] if kind == "reversed" else np.stack([rng.permutation(row) for row in o])
        out.append(np.ascontiguousarray(o.reshape(-1)))
    return out


def run_forward(dev, cfg, sd, pts, feats, nbr, itp, order=None, workspace=None, num_neighbors=None, nan_out=False):
    """``workspace``: a byte to fill a caller-provided workspace with (None: the op's own); ``nan_out``: a caller-provided output
    pre-filled with NaN, so that a row the forward does not write shows."""
    from ml3d import _abi, ops
    from ml3d.torch.models import _randla_pack
    batch, n0, _ = pts.shape
    desc = _abi.make_desc(cfg if num_neighbors is None else dict(cfg, num_neighbors=num_neighbors), batch, n0)
    off = _abi.randla_param_offsets(_abi.get(), desc)
    params = torch.from_numpy(_randla_pack.pack(sd, cfg, off)).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ws = None
    if workspace is not None:
        import ctypes as C
        wsb = int(_abi.get().ml3d_randla_forward_workspace_bytes(C.byref(desc)))
        ws = torch.full((wsb,), workspace, dtype=torch.uint8, device=dev)
    out = ops.randla_forward(desc, params, t(feats), t(pts), [t(x) for x in nbr], [t(x) for x in itp],
                             tile_order=None if order is None else [t(o) for o in order], workspace=ws,
                             out=torch.full((batch, n0, cfg["num_classes"]), float("nan"), device=dev) if nan_out else None)
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    return out.cpu()


def check_case(dev, index, report=_print, orders=("reversed", "random")):
    """One row: derive and assert its classes, run it, judge it against float64, then the same with a reversed and a random
    ``tile_order``: bit for bit the unordered result (the emulator runs take one of the two orders per row).  The ordered runs
    get a workspace of NaN bytes and an output pre-filled with NaN: an ordered instance that skipped a tile or a row could
    otherwise find the unordered run's correct values still lying in a recycled allocation."""
    case = CASES[index]
    cfg, batch, n0, ops = derive(case, device_cus(dev))
    seed = _seed(case)
    sd, pts, feats, nbr, itp = _inputs(case[0], batch, n0, seed)
    r64, r32, ref_s = _references(case[0], batch, n0, seed)
    bound_of(r64, r32)
    t = time.time()
    got = run_forward(dev, cfg, sd, pts, feats, nbr, itp)
    run_s = time.time() - t
    attn = [g for tag, _, g in ops if tag.startswith("attn") and tag.endswith(".%d" % (cfg["num_layers"] - 1))]
    extra = dict(kernels=" | ".join(sorted(set(k for _, k, _ in ops))), rows=batch * n0, reference_seconds=round(ref_s, 2),
                 forward_seconds=round(run_s, 2), tiles=[g["tiles"] for g in attn], grid=[g["grid"] for g in attn],
                 chunk=[g["chunk"] for g in attn], most_tiles_per_worker=[g["most"] for g in attn])
    judge(lambda **kv: report(**kv, **extra), CASE_IDS[index], got, r64, r32)
    for kind in orders:
        out = run_forward(dev, cfg, sd, pts, feats, nbr, itp, order=tile_orders(cfg, batch, n0, kind), workspace=0xFF, nan_out=True)
        assert same_bits(out, got), (CASE_IDS[index], "tile_order", kind, float((out - got).abs().max()))


# ---- exact checks, on the ragged row of every class ---------------------------------------------------------------------------------
EXACT = tuple(i for i, c in enumerate(CASES) if c[1] == "ragged")
EXACT_EMULATED = tuple(i for i in EXACT if CASES[i][0] in ("stage8", "mfma16_epi", "mfma16", "wave32", "wave_b3_64", "b3_128", "b3_256"))


def kernels_with_fuse_rows(case, rows, cus=EMU_CUS):
    """The kernels of a row with the fused per-point kernels from ``rows`` rows on (None: the product's threshold)."""
    return [k for _, k, _ in plan(NETS[case[0]][0], case[2], case_points(case, cus), cus, fuse=64 * 1024 if rows is None else rows)]


def check_exact(dev, index):
    case = CASES[index]
    cfg, batch, n0, _ = derive(case, device_cus(dev))
    sd, pts, feats, nbr, itp = _inputs(case[0], batch, n0, _seed(case))
    base = run_forward(dev, cfg, sd, pts, feats, nbr, itp, workspace=0)
    assert bool(torch.isfinite(base).all())
    # two runs give the same bits (the second in the op's own workspace)
    assert same_bits(run_forward(dev, cfg, sd, pts, feats, nbr, itp), base), (CASE_IDS[index], "second run")
    # a workspace of NaN bytes gives the bits of the zeroed one: no kernel reads scratch it did not write
    assert same_bits(run_forward(dev, cfg, sd, pts, feats, nbr, itp, workspace=0xFF), base), (CASE_IDS[index], "workspace of NaN bytes")
    # cloud 0 keeps its bits beside other clouds (B unchanged: the same classes)
    _, pts2, feats2, nbr2, itp2 = _inputs(case[0], batch, n0, _seed(case) + 50)
    mix = lambda a, b: np.ascontiguousarray(np.concatenate([a[:1], b[1:]], 0))
    other = run_forward(dev, cfg, sd, mix(pts, pts2), mix(feats, feats2), [mix(a, b) for a, b in zip(nbr, nbr2)],
                        [mix(a, b) for a, b in zip(itp, itp2)])
    assert same_bits(other[0], base[0]) and not same_bits(other[1], base[1]), (CASE_IDS[index], "other clouds")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(fn, what, match):
    try:
        fn()
    except RuntimeError as e:
        assert match in str(e), (what, str(e))
        return
    raise AssertionError("%s was accepted" % (what,))


def check_refusals(dev):
    batch, n0 = 2, 64
    cfg = net(8, [16, 64], [4, 1])
    sd = R.make_state_dict(cfg, 3)
    pts = synth_data.uniform_cloud(5, batch * n0).reshape(batch, n0, 3)
    inp = R.build_inputs(pts, pts.copy(), cfg, oops.knn_search)
    nbr = [np.ascontiguousarray(x.numpy().astype(np.int32)) for x in inp["neighbor_indices"]]
    itp = [np.ascontiguousarray(x.numpy().astype(np.int32)) for x in inp["interp_idx"]]
    assert bool(torch.isfinite(run_forward(dev, cfg, sd, pts, pts.copy(), nbr, itp)).all())          # the accepted twin
    # an even width without a kernel
    odd = net(8, [16, 24], [4, 1])
    assert plan(odd, batch, n0, device_cus(dev)) is None
    _refused(lambda: run_forward(dev, odd, R.make_state_dict(odd, 3), pts, pts.copy(), nbr, itp), "width 24", "unsupported configuration")
    # a last level of fewer than 16 points (tests/test_emulated_kernels.py::test_forward_rejects_levels_with_fewer_than_16_points)
    few = net(8, [16, 64], [4, 2])
    assert plan(few, batch, 60, device_cus(dev)) is None                                              # 60 / 4 = 15 points at level 1
    z = lambda n, k: np.zeros((batch, n, k), np.int32)
    _refused(lambda: run_forward(dev, few, R.make_state_dict(few, 3), pts[:, :60], pts[:, :60].copy(), [z(60, 16), z(15, 16)],
                                 [z(60, 1), z(15, 1)]), "15 points at the last level", "unsupported configuration")
    # num_neighbors != 16
    assert plan(dict(cfg, num_neighbors=8), batch, n0, device_cus(dev)) is None
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), [x[:, :, :8].copy() for x in nbr], itp, num_neighbors=8),
             "8 neighbours", "unsupported configuration")
    # the shape and dtype checks of ops.randla_forward
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts[:, :, :2].copy(), nbr, itp), "2 feature columns", "shape does not match")
    _refused(lambda: run_forward(dev, cfg, sd, pts.astype(np.float64), pts.copy(), nbr, itp), "float64 points", "contiguous float32")
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), [x.astype(np.int64) for x in nbr], itp), "int64 neighbours", "contiguous int32")
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), nbr[:1], itp), "one neighbour table", "index tensors")
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), [nbr[0][:, :-1].copy(), nbr[1]], itp), "a short neighbour table", "neighbor_idx[0]")
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), nbr, [itp[0], itp[1][:, :-1].copy()]), "a short interpolation table", "interp_idx[1]")
    _refused(lambda: run_forward(dev, cfg, sd, pts, pts.copy(), nbr, itp, order=[np.zeros(5, np.int32), np.zeros(batch * 16, np.int32)]),
             "a short tile order", "tile_order[0]")
    from ml3d import _abi, ops
    from ml3d.torch.models import _randla_pack
    desc = _abi.make_desc(cfg, batch, n0)
    params = torch.from_numpy(_randla_pack.pack(sd, cfg, _abi.randla_param_offsets(_abi.get(), desc))).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _refused(lambda: ops.randla_forward(desc, params, t(pts), t(pts), [t(x) for x in nbr], [t(x) for x in itp],
                                        workspace=torch.zeros(64, dtype=torch.uint8, device=dev)), "a 64-byte workspace", "workspace too small")


# ---- fault injection into the float64 oracle (CPU only): the bound of a row must reject a faulty layer -------------------------------
FAULTS = ("neighbour", "channel", "noise12")
FAULT_CUS = 256                                    # the rows sized by a grid cap are checked at the MI355X's shapes


def moved_by(case, fault, r64, cus=FAULT_CUS):
    """max |faulty float64 oracle - float64 oracle| with ``fault`` inside the LAST encoder layer (randlanet_ref._lfa wrapped for
    that layer only).  Cloud by cloud where ``oracle`` goes cloud by cloud; a cloud the fault does not touch is not computed again."""
    cfg, batch, n0, ops = derive(case, cus)
    sd, pts, feats, nbr, itp = _inputs(case[0], batch, n0, _seed(case))
    last = cfg["num_layers"] - 1
    tp = [g for tag, _, g in ops if tag == "attn2.%d" % last][0]["tp"]
    real = R._lfa
    state = {}

    def lfa(sd_, name, coords, feat, idx):
        if name != "encoder.%d" % last:
            return real(sd_, name, coords, feat, idx)
        if fault == "neighbour" and state["has_last"]:  # (a) one neighbour index of the last point of the last cloud replaced by another
            idx = idx.clone()
            idx[-1, -1, 5] = (idx[-1, -1, 5] + idx.shape[1] // 2) % idx.shape[1]
        out = real(sd_, name, coords, feat, idx)      # (B, 2 d, n, 1)
        if fault == "channel" and state["has_first"]:  # (b) one output channel zeroed on the points of one tile: the tile of cloud 0
            out = out.clone()                          # and the channel that hold the cloud's LARGEST output, the most visible one (a
            ch, pt = divmod(int(out[0, :, :, 0].argmax()), out.shape[2])       # deeper layer is seen only through the max over
            out[0, ch, pt // tp * tp:(pt // tp + 1) * tp] = 0                  # neighbours, and lrelu 0.01 leaves most of a wide row near 0)
        elif fault.startswith("noise"):                # (c) uniform relative noise of 2^-12 (2^-17: reported only)
            g = torch.Generator().manual_seed(7 + state["first"])
            out = out * (1 + 2.0 ** -int(fault[5:]) * (2 * torch.rand(out.shape, generator=g, dtype=out.dtype) - 1))
        return out

    per_cloud = batch * n0 > EMU_MAX_ROWS
    slices = [slice(b, b + 1) for b in range(batch)] if per_cloud else [slice(0, batch)]
    if fault == "neighbour":
        slices = slices[-1:]
    elif fault == "channel":
        slices = slices[:1]
    s64, moved = cast_sd(sd, torch.float64), 0.0
    R._lfa = lfa
    try:
        for sl in slices:
            state.update(first=sl.start, has_first=sl.start == 0, has_last=sl.stop == batch)
            out = R.forward(s64, cfg, oracle_inputs(cfg, pts, feats, nbr, itp, sl))
            moved = max(moved, float((out - r64[sl]).abs().max()))
    finally:
        R._lfa = real
    return moved


def check_can_fail(index, report=_print, cus=FAULT_CUS):
    case = CASES[index]
    _, batch, n0, _ = derive(case, cus)
    t = time.time()
    r64, r32, _ = _references(case[0], batch, n0, _seed(case))
    e32, tol = bound_of(r64, r32)
    moved = {f: moved_by(case, f, r64, cus) for f in FAULTS + ("noise17",)}
    report(name=CASE_IDS[index], rows=batch * n0, e32=e32, tol=tol, seconds=round(time.time() - t, 2), **moved)
    for f in FAULTS:
        assert moved[f] > tol, (CASE_IDS[index], f, moved[f], tol)
