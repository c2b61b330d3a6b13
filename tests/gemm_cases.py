"""Shared bodies of the shared GEMM's op tests (csrc/gemm.hip through its public Python entries: ``ops.linear``,
``ops.pack_bf16x3``, ``ops.linear_bf16x3``, ``ops.linear_rows_bf16x3``, ``ops.conv2d_nhwc``, ``ops.deconv2d_nhwc``), like
tests/pt_cases.py: tests/test_emulated_gemm.py runs every case of at most about 2 000 rows on CPU tensors against the host
emulation, tests/test_gpu_gemm.py all of them on the MI355X.  Every body takes the device and a ``report`` callback that receives
the MEASURED figures of each float comparison before it is asserted.

The one tolerance is ``pt_cases.judge``: the reference is the direct formula in FLOAT64 on CPU tensors, ``e32`` the distance of
the same formula in float32 from it at the case's own inputs, a case passes within max(1e-5, 4 e32).  Inputs as the epilogue test
of tests/test_gpu_pointpillars.py draws them: standard normal ``a``, ``w / sqrt(K)`` (sums of unit variance at every K), standard
normal bias and residual -- at these 1e-5 is what the emulator and GPU GEMM tests have always applied.  Everything else
(determinism, power-of-two scalings, row / column independence, slack of slices, refusals) is compared for EQUALITY, bit for bit.

Each row of a table is the smallest shape that reaches one dispatch class; the class is DERIVED below from a restatement of the
host rules of gemm.hip and asserted next to the expectation the table states, so that a changed shape (or a changed rule) that
leaves its class fails here and not silently.  Constants: GM_BM = GM_BN = 64, GM_KC = 32 (gemm_tile), G2_BM = 128 (gemm_tile2,
gemm_tile_bf3, conv3x3s1_bf3), BF_KC = 32."""
import os

import numpy as np
import torch

from pt_cases import _print, judge, same_bits

GM_BM = GM_BN = 64
GM_KC = 32
G2_BM = 128
BF_KC = 32
SLOPE = 0.2


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the host rules of gemm.hip, restated ----------------------------------------------------------------------------------------
def pick_splits(m, n, k):
    """One split if there are >= 256 tiles of 64 x 64 (>= 1024 when K >= 768) or K < 512; else min(ceil(aim / tiles), K / 128, 32)."""
    tiles = cdiv(m, GM_BM) * cdiv(n, GM_BN)
    thr, aim = (1024, 1024) if k >= 768 else (256, 512)
    if tiles >= thr or k < 512:
        return 1
    return max(1, min(cdiv(aim, tiles), k // 128, 32))


def slices(k, s, kc):
    """gemm_launch / launch_bf3: slices of whole chunks -> (slices actually launched, their depth, depth of the last)."""
    kper = cdiv(cdiv(k, s), kc) * kc
    cnt = cdiv(k, kper)
    return cnt, kper, k - (cnt - 1) * kper


def big_min_tiles():
    """256 in the product; the emulator build reads ML3D_GEMM_BIG_MIN_TILES (tests/test_emulated_gemm.py, second pass)."""
    return int(os.environ.get("ML3D_GEMM_BIG_MIN_TILES", "256"))


def big_bn(m, n, k, c):
    mt = big_min_tiles()
    if n % 4 or k % GM_KC or k < (0 if mt <= 1 else 256) or c % GM_KC:
        return 0
    rows = cdiv(m, G2_BM)
    if n > 64 and rows * cdiv(n, 128) >= 2 * mt:
        return 128
    if rows * cdiv(n, 64) >= mt:
        return 128 if (n > 64 and rows * cdiv(n, 128) >= mt) else 64
    return 0


def rows_f32_class(m, n, k1, k2=0, gather=False):
    """-> ("tile", PLAIN, DEPTH, slices, depth of the last slice) of ops.linear."""
    k = k1 + k2
    cnt, kper, last = slices(k, pick_splits(m, n, k), GM_KC)
    vec = k1 % 4 == 0 and k2 % 4 == 0
    plain = vec and n % 4 == 0 and not gather and (k2 == 0 or k1 % GM_KC == 0) and k % GM_KC == 0
    depth = 2 if cdiv(m, GM_BM) * cdiv(n, GM_BN) * cnt <= 12288 else 1
    return ("tile", plain, depth, cnt, last)


def conv_out(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_f32_class(b, h, w, c, n, k, stride, pad):
    """-> ("tile", False, DEPTH, slices, last) or ("tile2", BN, KC, grid x * grid y) of ops.conv2d_nhwc without ``packed``."""
    oh, ow = conv_out(h, w, k, stride, pad)
    m, kk = b * oh * ow, k * k * c
    s = pick_splits(m, n, kk)
    bn = big_bn(m, n, kk, c) if (s == 1 and k * k <= 32) else 0
    if bn:
        kc = 64 if (bn == 128 and kk % 64 == 0 and c % 64 == 0) else 32
        return ("tile2", bn, kc, cdiv(m, G2_BM) * cdiv(n, bn))
    cnt, kper, last = slices(kk, s, GM_KC)
    return ("tile", False, 2 if cdiv(m, GM_BM) * cdiv(n, GM_BN) * cnt <= 12288 else 1, cnt, last)


def bf3_splits(m, n, k):
    tiles = cdiv(m, G2_BM) * (cdiv(n, 128) if n > 64 else 1)
    slots = 256 * (2 if n > 64 else 4)
    if k < 512 or tiles >= 3 * slots:
        return 1
    if tiles >= 512:
        best, best_cost = 1, float(cdiv(tiles, slots))
        for c in range(2, min(4, k // 128) + 1):
            cost = cdiv(tiles * c, slots) / c + 0.1
            if cost < best_cost - 1e-9:
                best, best_cost = c, cost
        return best
    return max(1, min(cdiv(768, tiles), k // 128, 32))


def rows_bf3_class(m, n, k):
    """-> ("bf3", BN, slices, depth of the last slice) of ops.linear_bf16x3 / linear_rows_bf16x3."""
    cnt, kper, last = slices(k, bf3_splits(m, n, k), BF_KC)
    return ("bf3", 128 if n > 64 else 64, cnt, last)


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
# epilogue modes (bias, act, residual rows), rotated over the shapes of A1 / C1
MODES = ((False, 0, False), (True, 1, False), (True, 2, False), (False, 2, False), (True, 0, True), (False, 1, True))

A1_M = (1, 63, 64, 65, 129)                       # one partial tile | one row short | exact | one row over | two tiles + 1
A1_N = (4, 64, 68, 132)
A1_K = (32, 96)                                   # one chunk | three: all K % 32 == 0, N % 4 == 0 -> PLAIN, DEPTH 2, one slice
# A2: two plain blocks with a residual.  A3: the generic loader (PLAIN false): (m, n, k1, k2, gather, why)
A3 = ((130, 36, 40, 0, False, "K % 32 != 0: vector loads, K tail"),
      (130, 36, 5, 0, False, "k1 % 4 != 0: scalar loads"),
      (130, 19, 64, 0, False, "N % 4 != 0: bvec = 0"),
      (70, 1, 64, 0, False, "N = 1: bvec = 0"),
      (130, 36, 48, 32, False, "first block not chunk-aligned"),
      (130, 36, 64, 0, True, "gathered rows"),
      (130, 36, 32, 64, True, "gathered rows | a2"))
# A4: split-K: (m, n, k, residual, (PLAIN, DEPTH, slices, last))
A4 = ((130, 36, 544, None, (True, 2, 4, 64)),     # 3 tiles, K < 768: min(ceil(512 / 3), 4) = 4 slices of ceil(136 / 32) * 32 = 160
      (200, 68, 1000, None, (False, 2, 7, 40)),   # 8 tiles, K >= 768: min(128, 7) = 7 of ceil(143 / 32) * 32 = 160; K % 32 = 8
      (65, 19, 800, None, (False, 2, 5, 160)),    # 2 tiles: min(512, 6) = 6 -> ceil(134 / 32) * 32 = 160 deep = 5 slices; N % 4 = 3
      (77, 20, 640, "gather", (True, 2, 5, 128)))  # 2 tiles: min(256, 5) = 5 slices of 128; gathered residual through gemm_reduce
# A5: DEPTH 1, above 12 288 workgroups: (m, n, k, (PLAIN, DEPTH, slices, last), workgroups)
A5 = ((393280, 68, 32, (True, 1, 1, 32), 12290),  # 6145 x 2 tiles, the second column tile 4 wide
      (786496, 8, 12, (False, 1, 1, 12), 12289))  # 12 289 x 1, K % 4 == 0 but no whole chunk

# B: (b, h, w, c, n, k, stride, pad, class)
B1 = ((2, 17, 9, 48, 20, 3, 1, 1, ("tile", False, 2, 1, 432)),     # K = 432 < 512; C % 32 = 16: a chunk straddles two taps
      (2, 17, 9, 4, 12, 3, 2, 1, ("tile", False, 2, 1, 36)),       # K = 36: 9 taps in two chunks
      (2, 7, 5, 8, 12, 1, 1, 0, ("tile", False, 2, 1, 8)),         # 1 x 1 / pad 0
      (1, 9, 7, 8, 20, 5, 1, 2, ("tile", False, 2, 1, 200)))       # 5 x 5 / pad 2
B2 = ((1, 20, 28, 64, 64, 3, 1, 1, ("tile", False, 2, 4, 96)),     # M = 560: 9 tiles, K = 576: min(57, 4) = 4 slices of 160, last 96
      (1, 20, 28, 128, 64, 3, 2, 1, ("tile", False, 2, 9, 128)))   # M = 140: 3 tiles, K = 1152: min(342, 9) = 9 slices of 128
# B5: gemm_tile<ConvLoader, false, DEPTH = 1>: 887 x 887 = 786 769 pixels = 12 294 row tiles x 1 > 12 288 workgroups; C = 4 keeps the
# problem off gemm_tile2 (C % 32 != 0).  50 MB of output, a 28 MFLOP product.
B5 = (1, 887, 887, 4, 8, 3, 1, 1, ("tile", False, 1, 1, 36))
# B3: gemm_tile2 on real sizes (the product has no hook).  2 x 131 x 127: M = 33 274 = 260 tiles of 128 rows (>= 256); tile 129
# holds the last rows of image 0 and the first of image 1, 127 is odd so every image row breaks inside a tile.  big_kc gives
# KC = 64 only next to BN = 128, so gemm_tile2<ConvLoader2, 64, 64> has no caller: three of the four instantiations are reachable.
# grid x * grid y mod 8 is xcd_tile's remainder: 260 -> 4, 259 -> 3, 518 -> 6 (N = 192; at N = 128 the grid is 259 x 1 again).
B3 = ((2, 131, 127, 32, 64, 3, 1, 1, ("tile2", 64, 32, 260)),
      (2, 131, 127, 32, 36, 3, 1, 1, ("tile2", 64, 32, 260)),      # ragged column tile
      (2, 131, 127, 32, 128, 3, 1, 1, ("tile2", 128, 32, 260)),
      (2, 131, 127, 32, 72, 3, 1, 1, ("tile2", 128, 32, 260)),     # ragged
      (2, 131, 127, 64, 128, 3, 1, 1, ("tile2", 128, 64, 260)),
      (2, 262, 254, 32, 64, 3, 2, 1, ("tile2", 64, 32, 260)),      # stride 2 onto 131 x 127
      (2, 131, 127, 256, 64, 1, 1, 0, ("tile2", 64, 32, 260)),     # K = 256: the lowest K big_bn takes
      (1, 183, 181, 32, 64, 3, 1, 1, ("tile2", 64, 32, 259)),      # M = 33 123: 259 = 3 (mod 8)
      (1, 183, 181, 32, 192, 3, 1, 1, ("tile2", 128, 32, 518)))    # 259 x 2 = 6 (mod 8)
B4 = (2, 17, 9, 32, 20, 3, 1, 1)                                   # into columns 8 .. 28 of a 40-wide map

C1_M = (1, 127, 128, 129, 257)
C1_N = (4, 20, 64, 65, 72, 128, 132, 200)         # BN = 64 up to N = 64, BN = 128 above; 200 = two column tiles, the second ragged
C1_K = (32, 96)
# C4: split-K, tiles < 512: (m, n, k, residual, (BN, slices, last))
C4 = ((129, 72, 544, None, (128, 4, 64)),         # 2 tiles: min(384, 4) = 4 slices of 160
      (257, 200, 1056, None, (128, 7, 96)),       # 3 x 2 tiles: min(128, 8) = 8 -> ceil(132 / 32) * 32 = 160 deep = 7 slices
      (130, 40, 1024, "gather", (64, 8, 128)))    # 2 tiles (N <= 64: one column tile): min(384, 8) = 8 slices of 128
# C5: split-K, tiles >= 512 (one to three rounds of workgroups): (m, n, k, (BN, slices, last))
C5 = ((65537, 128, 512, (128, 4, 128)),           # 513 tiles on 512 slots: rounds(s) / s + 0.1 = 2 | 1.6 | 1.43 | 1.35 -> 4
      (65537, 64, 512, (64, 3, 128)))             # 513 tiles on 1024 slots: 1 | 1.1 | 0.77 | 0.85 -> 3 slices of 192 / 192 / 128

# D1: 3 x 3 / stride 1 / pad 1 with ``packed``: conv3x3s1_bf3<64 | 128> (gemm_tile_bf3<ConvLoader2> under ML3D_CONV_WINDOW=0 on the
# emulator): (c, n, (h, w), b) -- image rows shorter and longer than a 128-pixel tile, a tile spanning two images, one-pixel maps
D1 = ((32, 64, (13, 11), 2), (64, 128, (3, 140), 1), (32, 200, (9, 16), 3), (64, 40, (1, 37), 2), (32, 64, (45, 1), 2),
      (96, 64, (16, 16), 1))
# D2: gemm_tile_bf3<ConvLoader2, 64 | 128>: (b, h, w, c, n, k, stride, pad)
D2 = ((2, 12, 14, 64, 128, 3, 2, 1),              # stride 2
      (1, 9, 7, 64, 48, 1, 1, 0),                 # 1 x 1 / pad 0
      (1, 9, 7, 32, 40, 5, 1, 2),                 # 25 taps
      (2, 5, 5, 32, 20, 3, 2, 1),                 # N = 20
      (2, 31, 9, 96, 132, 3, 2, 1))               # N = 128 + 4, three chunks per tap
D3 = (1, 9, 8, 32, 24, 7, 1, 3)                   # 49 taps > 32: the packed call is refused and the f32 kernel runs
D4_STRIDES = (1, 2, 4)

# the exact checks: (path, m, n, k1, k2, class)
EXACT_ROWS = (("f32", 130, 36, 64, 0, ("tile", True, 2, 1, 64)),
              ("f32", 130, 19, 40, 0, ("tile", False, 2, 1, 40)),
              ("f32", 130, 36, 544, 0, ("tile", True, 2, 4, 64)),
              ("bf3", 129, 20, 64, 0, ("bf3", 64, 1, 64)),
              ("bf3", 257, 72, 96, 0, ("bf3", 128, 1, 96)),
              ("bf3", 129, 72, 544, 0, ("bf3", 128, 4, 64)))
# (b, h, w, c, n, packed): f32 gemm_tile (gemm_tile2 under the emulator's hook) and the window kernel; B3's first row on the GPU
EXACT_CONV = ((2, 13, 11, 32, 64, False), (2, 13, 11, 32, 64, True))
EXACT_CONV_BIG = (2, 131, 127, 32, 64, False)


# ---- references --------------------------------------------------------------------------------------------------------------------
def act_of(x, act):
    return {0: x, 1: torch.where(x > 0, x, x * SLOPE), 2: torch.relu(x)}[act]


def randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))


def weights(rng, k, n):
    return torch.from_numpy((rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32))


def gathered_rows(src, idx):
    """rows src[idx], zero where idx is outside [0, len(src)): the rule of the row gather and of the gathered residual"""
    ok = (idx >= 0) & (idx < src.shape[0])
    return src[idx.clamp(0, src.shape[0] - 1).long()] * ok[:, None].to(src.dtype)


def rows_formula(dt, a, w, bias, a2, gather, residual, residual_gather, act):
    x = a.to(dt)
    if gather is not None:
        x = gathered_rows(x, gather[:, 0])
    if a2 is not None:
        x = torch.cat([x, a2.to(dt)], 1)
    y = x @ w.to(dt)
    if bias is not None:
        y = y + bias.to(dt)
    if residual is not None:
        y = y + (residual.to(dt) if residual_gather is None else
                 gathered_rows(residual.to(dt), residual_gather.reshape(len(residual_gather), -1)[:, 0]))
    return act_of(y, act)


def conv_formula(dt, x, w, bias, k, stride, pad, act):
    """im2col by slicing + one product: columns ordered (ky, kx, ci) as the weight rows are"""
    b, h, wd, c = x.shape
    oh, ow = conv_out(h, wd, k, stride, pad)
    xp = torch.nn.functional.pad(x.to(dt), (0, 0, pad, pad, pad, pad))
    cols = torch.cat([xp[:, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride, :]
                      for ky in range(k) for kx in range(k)], -1)
    y = cols.reshape(-1, k * k * c) @ w.to(dt)
    if bias is not None:
        y = y + bias.to(dt)
    return act_of(y, act).reshape(b, oh, ow, -1)


def deconv_formula(dt, x, w, bias, s, cout, act):
    """kernel == stride: a product with [ci, (dy, dx, co)] weights + pixel shuffle"""
    b, h, wd, c = x.shape
    y = (x.to(dt).reshape(-1, c) @ w.to(dt)).reshape(b, h, wd, s, s, cout) + bias.to(dt)
    return act_of(y, act).permute(0, 1, 3, 2, 4, 5).reshape(b, h * s, wd * s, cout)


# ---- runners -----------------------------------------------------------------------------------------------------------------------
def _to(dev, t):
    return None if t is None else t.to(dev)


def lib():
    from ml3d import _abi
    return _abi.get()


def pack(dev, w):
    from ml3d import ops
    pk = ops.pack_bf16x3(w.to(dev))
    assert pk is not None and pk.dtype == torch.uint8
    return pk


def run_rows(dev, path, a, w, bias=None, a2=None, gather=None, residual=None, residual_gather=None, act=0, packed=None):
    from ml3d import ops
    if path == "f32":
        out = ops.linear(a.to(dev), w.to(dev), _to(dev, bias), a2=_to(dev, a2), gather=_to(dev, gather), residual=_to(dev, residual),
                         act=act, slope=SLOPE, residual_gather=_to(dev, residual_gather))
    else:
        assert gather is None
        out = ops.linear_bf16x3(a.to(dev), pack(dev, w) if packed is None else packed, w.shape[1], _to(dev, bias), act=act, slope=SLOPE,
                                a2=_to(dev, a2), residual=_to(dev, residual), residual_gather=_to(dev, residual_gather))
        assert out is not None
    return out.cpu()


def run_conv(dev, x, w, bias, k, stride, pad, act, packed=False):
    from ml3d import ops
    return ops.conv2d_nhwc(x.to(dev), w.to(dev), _to(dev, bias), k, k, stride, pad, act=act, slope=SLOPE,
                           packed=pack(dev, w) if packed else None).cpu()


def workspace_slices(path, m, n, k):
    """The slice count the library sizes its partials for (both ``*_workspace_bytes`` add 512 bytes of alignment slack)."""
    L = lib()
    wsb = int((L.ml3d_linear_workspace_bytes if path == "f32" else L.ml3d_linear_bf16x3_workspace_bytes)(m, n, k))
    part = wsb - 512
    assert part >= 0 and part % (4 * m * n) == 0, (wsb, m, n)
    return max(1, part // (4 * m * n))


def check_rows_class(path, m, n, k1, k2, gather, expect):
    """the table's class == the restated rules, and the library's workspace == the restated split rule"""
    k = k1 + k2
    got = rows_f32_class(m, n, k1, k2, gather) if path == "f32" else rows_bf3_class(m, n, k)
    assert got == expect, (path, m, n, k1, k2, got, expect)
    assert workspace_slices(path, m, n, k) == (pick_splits if path == "f32" else bf3_splits)(m, n, k), (path, m, n, k)


def rows_case(dev, report, name, path, m, n, k1, k2=0, mode=(True, 1, False), gather=False, residual=None, expect=None):
    """One Linear against float64.  ``residual``: None | "rows" | "gather" (a coarse residual picked by the first column of an
    int32 [m, 3] matrix with one index == its row count and one == -1).  ``gather``: a [m, 3] int32 row gather of ``a`` with one
    index == a.shape[0] and one == -1 (both zero rows)."""
    bias_on, act, res_rows = mode
    if res_rows and residual is None:
        residual = "rows"
    rng = np.random.default_rng([m, n, k1, k2, act])
    k = k1 + k2
    if expect is not None:
        check_rows_class(path, m, n, k1, k2, gather, expect)
    src_rows = max(1, m // 3) if gather else m
    a = randn(rng, src_rows, k1)
    a2 = randn(rng, m, k2) if k2 else None
    w = weights(rng, k, n)
    bias = randn(rng, n) if bias_on else None
    g = None
    if gather:
        g = torch.from_numpy(rng.integers(0, src_rows, (m, 3)).astype(np.int32))
        g[m // 2, 0], g[m - 1, 0] = src_rows, -1
    res = rg = None
    if residual == "rows":
        res = randn(rng, m, n)
    elif residual == "gather":
        mc = max(2, m // 3)
        res = randn(rng, mc, n)
        rg = torch.from_numpy(rng.integers(0, mc, (m, 3)).astype(np.int32))
        rg[m // 3, 0], rg[m - 2, 0] = mc, -1
    got = run_rows(dev, path, a, w, bias, a2, g, res, rg, act)
    refs = [rows_formula(dt, a, w, bias, a2, g, res, rg, act) for dt in (torch.float64, torch.float32)]
    judge(report, "%s %s m=%d n=%d k=%d+%d act=%d%s%s%s" % (name, path, m, n, k1, k2, act, " bias" if bias_on else "",
                                                            " res=" + residual if residual else "", " gather" if gather else ""),
          got, *refs)
    return got


# ---- A: ops.linear -------------------------------------------------------------------------------------------------------------------
def check_linear_plain(dev, m, report=_print):
    """A1: gemm_tile<RowsLoader, PLAIN, 2>, the epilogue modes rotated over N x K."""
    i = A1_M.index(m)
    for n in A1_N:
        for k in A1_K:
            rows_case(dev, report, "A1", "f32", m, n, k, mode=MODES[i % len(MODES)], expect=("tile", True, 2, 1, k))
            i += 1


def check_linear_two_blocks(dev, report=_print):
    """A2: [a | a2] with chunk-aligned widths stays PLAIN; 300 rows = 4 full tiles + 44."""
    rows_case(dev, report, "A2", "f32", 300, 64, 32, 64, mode=(True, 1, True), expect=("tile", True, 2, 1, 96))


def check_linear_generic_loader(dev, report=_print):
    """A3: every reason for which a Linear leaves the PLAIN loop."""
    for i, (m, n, k1, k2, gather, why) in enumerate(A3):
        rows_case(dev, report, "A3", "f32", m, n, k1, k2, mode=MODES[(i + 1) % len(MODES)], gather=gather,
                  expect=("tile", False, 2, 1, k1 + k2))


def check_linear_split_k(dev, report=_print):
    """A4: K cut into slices with an uneven last one, partials summed by gemm_reduce (epilogue there)."""
    for m, n, k, residual, cls in A4:
        rows_case(dev, report, "A4", "f32", m, n, k, mode=(True, 1, False), residual=residual or "rows", expect=("tile",) + cls)
        rows_case(dev, report, "A4", "f32", m, n, k, mode=(False, 2, False), expect=("tile",) + cls)


def check_linear_depth1(dev, index, report=_print):
    """A5: more than 12 288 workgroups: the one-chunk pipeline.  The float64 reference is < 1 GFLOP."""
    m, n, k, cls, wgs = A5[index]
    assert cdiv(m, GM_BM) * cdiv(n, GM_BN) == wgs > 12288
    rows_case(dev, report, "A5", "f32", m, n, k, mode=(True, 1, False), expect=("tile",) + cls)


# ---- B: ops.conv2d_nhwc, f32 ---------------------------------------------------------------------------------------------------------
def conv_inputs(b, h, w, c, n, k, seed=0):
    rng = np.random.default_rng([b, h, w, c, n, k, seed])
    return randn(rng, b, h, w, c), weights(rng, k * k * c, n), randn(rng, n)


def conv_case(dev, report, name, shape, act=2, packed=False, expect=None):
    b, h, w, c, n, k, stride, pad = shape
    if expect is not None and not packed:
        got_cls = conv_f32_class(*shape)
        if "ML3D_GEMM_BIG_MIN_TILES" not in os.environ:              # (the table states the product's class)
            assert got_cls == expect, (shape, got_cls, expect)
        oh, ow = conv_out(h, w, k, stride, pad)
        wsb = int(lib().ml3d_conv2d_workspace_bytes(b, oh, ow, c, n, k, k))
        s = pick_splits(b * oh * ow, n, k * k * c)
        assert wsb - 512 == (4 * b * oh * ow * n * s if s > 1 else 0), (shape, wsb, s)
    x, wt, bias = conv_inputs(b, h, w, c, n, k)
    got = run_conv(dev, x, wt, bias, k, stride, pad, act, packed)
    refs = [conv_formula(dt, x, wt, bias, k, stride, pad, act) for dt in (torch.float64, torch.float32)]
    judge(report, "%s %s %dx%dx%dx%d -> %d k=%d s=%d p=%d act=%d" % (name, "bf3" if packed else "f32", b, h, w, c, n, k, stride, pad, act),
          got, *refs)


def check_conv_f32_small(dev, report=_print):
    """B1 + B2: gemm_tile<ConvLoader>, one slice and split-K."""
    for i, row in enumerate(B1 + B2):
        conv_case(dev, report, "B1" if i < len(B1) else "B2", row[:8], act=(2, 1, 0)[i % 3], expect=row[8])


def check_conv_f32_big(dev, index, report=_print):
    """B3: gemm_tile2<ConvLoader2, BN, KC> at sizes that pass big_bn's 256-tile bar."""
    row = B3[index]
    conv_case(dev, report, "B3", row[:8], act=(2, 1)[index % 2], expect=row[8])


def check_conv_f32_depth1(dev, report=_print):
    """B5: the one-chunk pipeline behind the convolution loader."""
    assert cdiv(B5[1] * B5[2], GM_BM) > 12288
    conv_case(dev, report, "B5", B5[:8], act=1, expect=B5[8])


def check_conv_into_channel_slice(dev, report=_print):
    """B4 (+ its packed twin): out= / out_channel_offset= write columns 8 .. 28 of a 40-wide map; the rest keeps its -1."""
    from ml3d import ops
    b, h, w, c, n, k, stride, pad = B4
    x, wt, bias = conv_inputs(*B4[:6])
    refs = [conv_formula(dt, x, wt, bias, k, stride, pad, 2) for dt in (torch.float64, torch.float32)]
    for packed in (False, True):
        big = torch.full((b, h, w, 40), -1.0, dtype=torch.float32, device=dev)
        ops.conv2d_nhwc(x.to(dev), wt.to(dev), bias.to(dev), k, k, stride, pad, act=2, out=big, out_channel_offset=8,
                        packed=pack(dev, wt) if packed else None)
        big = big.cpu()
        judge(report, "B4 %s channel slice" % ("bf3" if packed else "f32"), big[..., 8:8 + n], *refs)
        assert bool((big[..., :8] == -1).all()) and bool((big[..., 8 + n:] == -1).all())


# ---- C: the bf16x3 Linears -----------------------------------------------------------------------------------------------------------
def check_bf3_linear(dev, m, report=_print):
    """C1: gemm_tile_bf3<RowsLoader2, 64 | 128>, the epilogue modes rotated over N x K."""
    i = C1_M.index(m)
    for n in C1_N:
        for k in C1_K:
            rows_case(dev, report, "C1", "bf3", m, n, k, mode=MODES[i % len(MODES)], expect=("bf3", 128 if n > 64 else 64, 1, k))
            i += 1


def check_bf3_two_blocks(dev, report=_print):
    """C2: [a | a2] (32 | 64 columns), residual, leaky ReLU, both tile widths."""
    for n in (64, 136):
        rows_case(dev, report, "C2", "bf3", 300, n, 32, 64, mode=(True, 1, True), expect=("bf3", 128 if n > 64 else 64, 1, 96))


def check_bf3_rows_on_slices(dev, report=_print):
    """C3: linear_rows_bf16x3 with ``a`` = columns 32 .. 96 of a [M, 160] buffer whose other columns are NaN and ``out`` = columns
    8 .. 8 + N of a [M, N + 24] buffer prefilled with -1, a 1-D residual gather: finite, and the slack keeps its -1."""
    from ml3d import ops
    for m, n, k in ((257, 72, 64), (130, 20, 64), (129, 72, 544)):          # BN = 128 | 64 | split-K (the partials are dense)
        rng = np.random.default_rng([m, n, k, 3])
        wide = torch.full((m, 160 if k == 64 else 32 + k + 32), float("nan"), dtype=torch.float32)
        a = randn(rng, m, k)
        wide[:, 32:32 + k] = a
        w, bias = weights(rng, k, n), randn(rng, n)
        mc = m // 3
        res = randn(rng, mc, n)
        rg = torch.from_numpy(rng.integers(0, mc, m).astype(np.int32))
        rg[5], rg[m - 1] = mc, -1
        dwide = wide.to(dev)
        dout = torch.full((m, n + 24), -1.0, dtype=torch.float32, device=dev)
        ret = ops.linear_rows_bf16x3(dwide[:, 32:32 + k], pack(dev, w), n, bias.to(dev), act=1, slope=SLOPE, out=dout[:, 8:8 + n],
                                     residual=res.to(dev), residual_gather=rg.to(dev))
        assert ret.data_ptr() == dout[:, 8:8 + n].data_ptr()
        out = dout.cpu()
        refs = [rows_formula(dt, a, w, bias, None, None, res, rg, 1) for dt in (torch.float64, torch.float32)]
        judge(report, "C3 bf3 slices m=%d n=%d k=%d" % (m, n, k), out[:, 8:8 + n], *refs)
        assert bool((out[:, :8] == -1).all()) and bool((out[:, 8 + n:] == -1).all())
        assert same_bits(out[:, 8:8 + n], run_rows(dev, "bf3", a, w, bias, None, None, res, rg.reshape(m, 1), 1)), "slices vs dense rows"


def check_bf3_split_k(dev, report=_print):
    """C4: the low-tile branch of bf3_splits, uneven last slice, gemm_reduce's epilogue."""
    for m, n, k, residual, cls in C4:
        rows_case(dev, report, "C4", "bf3", m, n, k, mode=(True, 1, False), residual=residual or "rows", expect=("bf3",) + cls)
        rows_case(dev, report, "C4", "bf3", m, n, k, mode=(False, 2, False), expect=("bf3",) + cls)


def check_bf3_split_k_many_tiles(dev, index, report=_print):
    """C5: 513 tiles of 128 rows: the "one to three rounds" branch.  The branch is chosen by M; K = 512 is the least it takes."""
    m, n, k, cls = C5[index]
    assert cdiv(m, G2_BM) >= 512
    rows_case(dev, report, "C5", "bf3", m, n, k, mode=(True, 1, False), expect=("bf3",) + cls)


# ---- D: convolutions with ``packed`` and the transposed convolution -------------------------------------------------------------------
def check_conv_bf3_window(dev, index, report=_print):
    """D1: conv3x3s1_bf3<64 | 128>."""
    c, n, (h, w), b = D1[index]
    conv_case(dev, report, "D1", (b, h, w, c, n, 3, 1, 1), act=2, packed=True)


def check_conv_bf3_general(dev, report=_print):
    """D2: gemm_tile_bf3<ConvLoader2>; D3: 49 taps fall back to the f32 kernel."""
    for i, shape in enumerate(D2):
        conv_case(dev, report, "D2", shape, act=(2, 0, 1)[i % 3], packed=True)
    assert lib().ml3d_gemm_pack_bf16x3_bytes(49 * 32, 24) > 0          # (the weights ARE packable: the convolution refuses)
    conv_case(dev, report, "D3", D3, act=2, packed=True)
    x, wt, bias = conv_inputs(*D3[:6])
    assert same_bits(run_conv(dev, x, wt, bias, 7, 1, 3, 2, True), run_conv(dev, x, wt, bias, 7, 1, 3, 2, False)), "7 x 7 ran elsewhere"


def check_deconv_into_concat_slice(dev, stride, report=_print):
    """D4: the transposed convolution (kernel == stride) into columns 40 .. 72 of an 80-wide map, f32 and bf16x3."""
    from ml3d import ops
    rng = np.random.default_rng(stride)
    cin, cout, b, h, w = 64, 32, 2, 6, 5
    x, wt, bias = randn(rng, b, h, w, cin), weights(rng, cin, stride * stride * cout), randn(rng, cout)
    refs = [deconv_formula(dt, x, wt, bias, stride, cout, 2) for dt in (torch.float64, torch.float32)]
    for packed in (False, True):
        big = torch.full((b, h * stride, w * stride, 80), -1.0, dtype=torch.float32, device=dev)
        ops.deconv2d_nhwc(x.to(dev), wt.to(dev), bias.to(dev), stride, cout, act=2, out=big, out_channel_offset=40,
                          packed=pack(dev, wt) if packed else None)
        big = big.cpu()
        judge(report, "D4 %s deconv stride=%d" % ("bf3" if packed else "f32", stride), big[..., 40:72], *refs)
        assert bool((big[..., :40] == -1).all()) and bool((big[..., 72:] == -1).all())


# ---- exact checks --------------------------------------------------------------------------------------------------------------------
def pow2(rng, n, lo=-20, hi=20):
    return torch.from_numpy(np.ldexp(np.float32(1.0), rng.integers(lo, hi + 1, n)).astype(np.float32))


def exact_rows_inputs(path, m, n, k1, k2, cls):
    check_rows_class(path, m, n, k1, k2, False, cls)
    rng = np.random.default_rng([m, n, k1, k2, 11])
    k = k1 + k2
    return rng, randn(rng, m, k), weights(rng, k, n), randn(rng, n), randn(rng, m, n)


def check_exact_rows(dev, index):
    """Determinism, power-of-two scalings along K / of rows and columns, row and column independence of one rows problem."""
    path, m, n, k1, k2, cls = EXACT_ROWS[index]
    rng, a, w, bias, res = exact_rows_inputs(path, m, n, k1, k2, cls)
    k = k1 + k2
    base = run_rows(dev, path, a, w, bias, residual=res, act=1)
    # 1. the same call twice
    assert same_bits(run_rows(dev, path, a, w, bias, residual=res, act=1), base), "determinism"
    # 2. a[:, k] 2^s_k against w[k, :] 2^-s_k: every product (on the bf16 pipe: of every pair of planes) is unchanged
    s = pow2(rng, k)
    assert same_bits(run_rows(dev, path, a * s, w / s[:, None], bias, residual=res, act=1), base), "scaling along K"
    # 3. rows of a and columns of w scaled, no bias / residual: the output scaled back is the unscaled one
    bare = run_rows(dev, path, a, w)
    assert same_bits(run_rows(dev, path, a, w), bare)
    sr, sc = pow2(rng, m), pow2(rng, n)
    scaled = run_rows(dev, path, a * sr[:, None], w * sc)
    assert bool(torch.isfinite(scaled).all())
    assert same_bits(scaled / sr[:, None] / sc, bare), "scaling of rows and columns"
    # 4. every third row finite (over three 32-row blocks: every position of the block and both 4-row halves of the MFMA row
    #    map), the others NaN: the finite rows do not move.  The same for the columns of w.
    keep = torch.arange(m) % 3 == 0
    poisoned = torch.where(keep[:, None], a, torch.full_like(a, float("nan")))
    got = run_rows(dev, path, poisoned, w, bias, residual=res, act=1)
    assert same_bits(got[keep], base[keep]), "row independence"
    assert bool(torch.isnan(got[~keep]).all()) if m > 1 else True
    keep = torch.arange(n) % 3 == 0
    poisoned = torch.where(keep[None, :], w, torch.full_like(w, float("nan")))
    got = run_rows(dev, path, a, poisoned, bias, residual=res, act=1)
    assert same_bits(got[:, keep], base[:, keep]), "column independence"
    assert bool(torch.isnan(got[:, ~keep]).all())


def check_exact_conv(dev, shape):
    """Determinism and the two scalings a convolution admits: channel ci of x by 2^s against rows (tap, ci) of w by 2^-s, and
    the columns of w (no bias)."""
    b, h, w, c, n, packed = shape
    x, wt, bias = conv_inputs(b, h, w, c, n, 3, seed=1)
    rng = np.random.default_rng([b, h, w, c, n, 12])
    base = run_conv(dev, x, wt, bias, 3, 1, 1, 2, packed)
    assert same_bits(run_conv(dev, x, wt, bias, 3, 1, 1, 2, packed), base), "determinism"
    s = pow2(rng, c)
    assert same_bits(run_conv(dev, x * s, wt / s.repeat(9)[:, None], bias, 3, 1, 1, 2, packed), base), "scaling along K"
    bare = run_conv(dev, x, wt, None, 3, 1, 1, 0, packed)
    sc = pow2(rng, n)
    assert same_bits(run_conv(dev, x, wt * sc, None, 3, 1, 1, 0, packed) / sc, bare), "scaling of columns"


def check_empty_and_refused(dev):
    """M = 0 returns an empty tensor; K = 40 cannot be packed; a first block of 48 columns is not eligible on the bf16 pipe."""
    from ml3d import ops
    rng = np.random.default_rng(5)
    w = weights(rng, 64, 8)
    out = ops.linear(torch.zeros((0, 64)).to(dev), w.to(dev), randn(rng, 8).to(dev))
    assert tuple(out.shape) == (0, 8) and out.dtype == torch.float32
    out = ops.linear_bf16x3(torch.zeros((0, 64)).to(dev), pack(dev, w), 8)
    assert out is not None and tuple(out.shape) == (0, 8)
    assert ops.pack_bf16x3(weights(rng, 40, 64).to(dev)) is None
    w96 = weights(rng, 96, 8)
    assert ops.linear_bf16x3(randn(rng, 10, 48).to(dev), pack(dev, w96), 8, a2=randn(rng, 10, 48).to(dev)) is None
    assert ops.linear_bf16x3(randn(rng, 10, 64).to(dev), pack(dev, w96), 8, a2=randn(rng, 10, 32).to(dev)) is not None
