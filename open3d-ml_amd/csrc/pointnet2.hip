// pointnet2.hip — PointNet++ multi-scale-grouping backbone inference (the reference's ml3d/torch/modules/pointnet.py and
// ml3d/torch/utils/pointnet/pointnet2_utils.py): ball query, the set-abstraction body (grouped MLP + maximum) as one kernel, the
// first grouped layer alone for the wide scales, and the three-point feature propagation.  Contracts: include/ml3d_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ml3d_hip.h"

namespace {

typedef float pn2_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------------
// (a) Ball query.  One wave per centre, 64 points per step.  All scales of a multi-scale-grouping level share ONE scan: the
// distance is computed once, every scale ballots its own hits and appends them at (hits so far) + (hits in lower lanes), which is
// ascending point order.  The scan of a centre ends when every scale is full.  Everything that steers control flow (the counts,
// the first hit) comes out of a ballot and is wave-uniform.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int BQ_MAX_SCALES = 4;
constexpr int BQ_WAVES = 4;

struct BallScales {
    int count;
    float r2[BQ_MAX_SCALES];
    int nsample[BQ_MAX_SCALES];
    int32_t* out[BQ_MAX_SCALES];
};

__global__ __launch_bounds__(64 * BQ_WAVES) void pn2_ball_query_kernel(const float* __restrict__ pts, const float* __restrict__ ctr,
                                                                     int64_t n, int64_t m, int64_t centres, BallScales sc) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int64_t q = (int64_t)blockIdx.x * BQ_WAVES + wave; q < centres; q += (int64_t)gridDim.x * BQ_WAVES) {
        const float* p = pts + (q / m) * n * 3;
        const float cx = ctr[3 * q], cy = ctr[3 * q + 1], cz = ctr[3 * q + 2];
        int cnt[BQ_MAX_SCALES], first[BQ_MAX_SCALES];
#pragma unroll
        for (int s = 0; s < BQ_MAX_SCALES; ++s) { cnt[s] = 0; first[s] = 0; }
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t j = base + lane;
            const int64_t jj = j < n ? j : n - 1;
            const float dx = cx - p[3 * jj], dy = cy - p[3 * jj + 1], dz = cz - p[3 * jj + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;      // (-ffp-contract=off: three products, two sums, in this order)
            bool open = false;
#pragma unroll
            for (int s = 0; s < BQ_MAX_SCALES; ++s) {
                if (s < sc.count && cnt[s] < sc.nsample[s]) {
                    const bool hit = j < n && d2 < sc.r2[s];
                    const unsigned long long mask = __ballot(hit);
                    if (mask) {
                        const int slot = cnt[s] + __popcll(mask & ((1ull << lane) - 1ull));
                        if (hit && slot < sc.nsample[s]) sc.out[s][q * sc.nsample[s] + slot] = (int32_t)j;
                        if (cnt[s] == 0) first[s] = (int)base + (__ffsll(mask) - 1);
                        cnt[s] += __popcll(mask);
                    }
                    open = open || cnt[s] < sc.nsample[s];
                }
            }
            if (!open) break;
        }
#pragma unroll
        for (int s = 0; s < BQ_MAX_SCALES; ++s) {
            if (s < sc.count) {
                // fewer hits than slots: the rest repeats the first hit; no hit at all: first[s] is still 0
                for (int t = (cnt[s] < sc.nsample[s] ? cnt[s] : sc.nsample[s]) + lane; t < sc.nsample[s]; t += 64)
                    sc.out[s][q * sc.nsample[s] + t] = first[s];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// (b) Set abstraction, one scale.  The first 1x1 convolution is linear, so W [p_j - c_i | f_j] = Wx (p_j - c_i) + y_j with
// y = f Wf computed once per SOURCE point (ml3d_linear; the algebra of pt_transition_down).  The position part stays on the exact
// difference p_j - c_i: formed as (Wx p_j) - (Wx c_i) it would cancel two numbers of the size of the coordinates (tens of metres in
// a lidar frame) down to the size of a ball (decimetres), an error of ~1e-5 per level that four levels carry to the output.
// A wave owns a tile of 32 grouped rows (two centres at nsample 16, one at nsample 32):
//   1. h1[row] = relu((Wx (p - c) + y[src(row)]) + b1)                 -> LDS [32][c1]
//   2. h2 = relu(h1 W2 + b2) on v_mfma_f32_32x32x2_f32, 32 columns at a time -> LDS [32][pad32(c2)]
//   3. relu(h2 W3 + b3) likewise; the maximum over a centre's rows is taken in the accumulator registers (a lane holds 8 rows of
//      each centre for its column; the other 8 sit 32 lanes away) and written into the caller's column slice.
// The folded BatchNorm scale lives in the weights, the shift is the bias.  Nothing [centres, nsample, c] reaches memory.
// An output depends on its own rows alone (an MFMA element is the sum over k of ITS row and ITS column, in a fixed order): a centre
// computed alone gives the same bits.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SA_MAXC = 128;
constexpr int SA_LD = SA_MAXC + 1;      // odd row stride: the 32 rows of an A-operand read fall into 32 different banks

struct SaParams {
    const float* y; int64_t ldy;      // NULL: no feature part
    const float* pts; const float* ctr; const int32_t* idx;
    int64_t n, m, centres;
    int ns, c1, c2p, c3;
    const float *wx, *b1, *w2, *b2, *w3, *b3;
    float* out; int64_t ldo;
};

// acc = A[32 x K] (LDS, row stride SA_LD) . W[K x 32] (columns col0 .. col0 + 31 of a [K, ldw] matrix)
__device__ __forceinline__ pn2_f32x16 sa_tile_product(const float* h, int K, const float* __restrict__ w, int ldw, int col0, int lane) {
    pn2_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int row = lane & 31, half = lane >> 5;
    const float* a = h + row * SA_LD + half;
    const float* b = w + (size_t)half * ldw + col0 + row;
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[(size_t)k * ldw], acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(64) void pn2_sa_kernel(SaParams p) {
    __shared__ float s_h1[32 * SA_LD];
    __shared__ float s_h2[32 * SA_LD];
    __shared__ int64_t s_src[32];
    __shared__ float s_d[32][3];
    const int lane = (int)threadIdx.x;
    const int cpt = 32 / p.ns;                                    // centres per tile: 2 or 1
    const int64_t tiles = (p.centres + cpt - 1) / cpt;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (lane < 32) {
            int64_t q = tile * cpt + lane / p.ns;
            if (q >= p.centres) q = p.centres - 1;                // (the odd last centre's twin: computed, never written)
            int64_t j = p.idx[q * p.ns + lane % p.ns];
            j = j < 0 ? 0 : (j >= p.n ? p.n - 1 : j);
            const int64_t src = (q / p.m) * p.n + j;
            s_src[lane] = src;
            s_d[lane][0] = p.pts[3 * src] - p.ctr[3 * q];
            s_d[lane][1] = p.pts[3 * src + 1] - p.ctr[3 * q + 1];
            s_d[lane][2] = p.pts[3 * src + 2] - p.ctr[3 * q + 2];
        }
        __syncthreads();
        for (int e = lane; e < 32 * p.c1; e += 64) {
            const int row = e / p.c1, ch = e - row * p.c1;
            float v = (p.wx[ch] * s_d[row][0] + p.wx[p.c1 + ch] * s_d[row][1]) + p.wx[2 * p.c1 + ch] * s_d[row][2];
            if (p.y) v += p.y[s_src[row] * p.ldy + ch];
            s_h1[row * SA_LD + ch] = fmaxf(v + p.b1[ch], 0.f);
        }
        __syncthreads();
        const int col = lane & 31, half = lane >> 5;
        for (int c0 = 0; c0 < p.c2p; c0 += 32) {
            const pn2_f32x16 acc = sa_tile_product(s_h1, p.c1, p.w2, p.c2p, c0, lane);
            const float b = p.b2[c0 + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) s_h2[((r & 3) + 8 * (r >> 2) + 4 * half) * SA_LD + c0 + col] = fmaxf(acc[r] + b, 0.f);
        }
        __syncthreads();
        for (int c0 = 0; c0 < p.c3; c0 += 32) {
            const pn2_f32x16 acc = sa_tile_product(s_h2, p.c2p, p.w3, p.c3, c0, lane);
            const float b = p.b3[c0 + col];
            float lo = 0.f, hi = 0.f;                             // rows 0 - 15 / 16 - 31 (every candidate is a ReLU output)
#pragma unroll
            for (int r = 0; r < 8; ++r) lo = fmaxf(lo, fmaxf(acc[r] + b, 0.f));
#pragma unroll
            for (int r = 8; r < 16; ++r) hi = fmaxf(hi, fmaxf(acc[r] + b, 0.f));
            lo = fmaxf(lo, __shfl_xor(lo, 32));
            hi = fmaxf(hi, __shfl_xor(hi, 32));
            if (half == 0) {
                if (cpt == 1) {
                    p.out[tile * p.ldo + c0 + col] = fmaxf(lo, hi);
                } else {
                    p.out[(2 * tile) * p.ldo + c0 + col] = lo;
                    if (2 * tile + 1 < p.centres) p.out[(2 * tile + 1) * p.ldo + c0 + col] = hi;
                }
            }
        }
        __syncthreads();
    }
}

// (c) the first grouped layer alone (the scales too wide for the fused kernel): one thread per (grouped row, channel)
__global__ __launch_bounds__(256) void pn2_group_kernel(const float* __restrict__ y, int64_t ldy, const float* __restrict__ pts,
                                                        const float* __restrict__ ctr, const int32_t* __restrict__ idx, int64_t n,
                                                        int64_t m, int64_t rows, int ns, int c1, const float* __restrict__ wx,
                                                        const float* __restrict__ b1, float* __restrict__ out, int64_t ldo) {
    const int64_t total = rows * c1;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t r = o / c1, q = r / ns;
        const int ch = (int)(o - r * c1);
        int64_t j = idx[r];
        j = j < 0 ? 0 : (j >= n ? n - 1 : j);
        const int64_t src = (q / m) * n + j;
        const float dx = pts[3 * src] - ctr[3 * q], dy = pts[3 * src + 1] - ctr[3 * q + 1], dz = pts[3 * src + 2] - ctr[3 * q + 2];
        float v = (wx[ch] * dx + wx[c1 + ch] * dy) + wx[2 * c1 + ch] * dz;
        if (y) v += y[src * ldy + ch];
        out[r * ldo + ch] = fmaxf(v + b1[ch], 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// (d) Three-point feature propagation: one thread per (row, channel); the three weights are recomputed per channel (three
// square roots and four divisions against three gathered loads).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pn2_interp_kernel(const float* __restrict__ known, int64_t ldk, int64_t mk, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ d2, const float* __restrict__ weight, int64_t n,
                                                         int64_t rows, int c, float* __restrict__ out, int64_t ldo) {
    const int64_t total = rows * c;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t i = o / c;
        const int ch = (int)(o - i * c);
        const float* kb = known + (i / n) * mk * ldk + ch;
        float w[3];
        if (weight) {
#pragma unroll
            for (int t = 0; t < 3; ++t) w[t] = weight[3 * i + t];
        } else {
#pragma unroll
            for (int t = 0; t < 3; ++t) w[t] = 1.0f / (sqrtf(d2[3 * i + t]) + 1e-8f);
            const float norm = (w[0] + w[1]) + w[2];
#pragma unroll
            for (int t = 0; t < 3; ++t) w[t] = w[t] / norm;
        }
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            int64_t j = idx[3 * i + t];
            j = j < 0 ? 0 : (j >= mk ? mk - 1 : j);
            acc += w[t] * kb[j * ldk];
        }
        out[i * ldo + ch] = acc;
    }
}

unsigned capped_grid(int64_t blocks, int64_t cap) { return (unsigned)(blocks < cap ? blocks : cap); }

}  // namespace

extern "C" int ml3d_ball_query(const float* points, const float* centres, int64_t batch, int64_t n, int64_t m, int scales,
                               const float* radii_host, const int32_t* nsample_host, int32_t* const* out_host, void* stream) {
    if (batch < 0 || n < 0 || m < 0 || scales < 1 || scales > BQ_MAX_SCALES || !radii_host || !nsample_host || !out_host)
        return ML3D_E_INVALID;
    BallScales sc;
    sc.count = scales;
    for (int s = 0; s < BQ_MAX_SCALES; ++s) { sc.r2[s] = 0.f; sc.nsample[s] = 0; sc.out[s] = nullptr; }
    for (int s = 0; s < scales; ++s) {
        const float r = radii_host[s];
        if (!(r >= 0.f) || nsample_host[s] < 1 || nsample_host[s] > 65536) return ML3D_E_INVALID;
        sc.r2[s] = r * r;
        sc.nsample[s] = nsample_host[s];
        sc.out[s] = out_host[s];
    }
    const int64_t total = batch * m;
    if (total == 0) return 0;
    if (n == 0 || n >= (1ll << 31) || !points || !centres) return ML3D_E_INVALID;
    for (int s = 0; s < scales; ++s)
        if (!sc.out[s]) return ML3D_E_INVALID;
    hipLaunchKernelGGL(pn2_ball_query_kernel, dim3(capped_grid((total + BQ_WAVES - 1) / BQ_WAVES, 1 << 20)), dim3(64 * BQ_WAVES), 0,
                       (hipStream_t)stream, points, centres, n, m, total, sc);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_pn2_sa_fused_supported(int nsample, int c1, int c2, int c3) {
    const int c2p = (c2 + 31) & ~31;
    return (nsample == 16 || nsample == 32) && c1 >= 2 && c1 <= SA_MAXC && (c1 & 1) == 0 && c2 >= 1 && c2p <= SA_MAXC && c3 >= 32 &&
           c3 <= SA_MAXC && (c3 & 31) == 0;
}

extern "C" int ml3d_pn2_sa_mlp_max(const float* y, int64_t ldy, const float* points, const float* centres, const int32_t* idx,
                                   int64_t batch, int64_t n, int64_t m, int nsample, int c1, int c2, int c3, const float* w_x,
                                   const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* out,
                                   int64_t ldo, void* stream) {
    if (batch < 0 || n < 0 || m < 0 || nsample < 1 || c1 < 1 || c2 < 1 || c3 < 1 || (y && ldy < c1) || ldo < c3) return ML3D_E_INVALID;
    if (!ml3d_pn2_sa_fused_supported(nsample, c1, c2, c3)) return ML3D_E_UNSUPPORTED;
    const int64_t total = batch * m;
    if (total == 0) return 0;
    if (n == 0 || n >= (1ll << 31) || !points || !centres || !idx || !w_x || !b1 || !w2 || !b2 || !w3 || !b3 || !out) return ML3D_E_INVALID;
    SaParams p;
    p.y = y; p.ldy = ldy; p.pts = points; p.ctr = centres; p.idx = idx;
    p.n = n; p.m = m; p.centres = total;
    p.ns = nsample; p.c1 = c1; p.c2p = (c2 + 31) & ~31; p.c3 = c3;
    p.wx = w_x; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.w3 = w3; p.b3 = b3;
    p.out = out; p.ldo = ldo;
    const int cpt = 32 / nsample;
    hipLaunchKernelGGL(pn2_sa_kernel, dim3(capped_grid((total + cpt - 1) / cpt, 1 << 20)), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_pn2_group_rows(const float* y, int64_t ldy, const float* points, const float* centres, const int32_t* idx,
                                   int64_t batch, int64_t n, int64_t m, int nsample, int c1, const float* w_x, const float* b1,
                                   float* out, int64_t ldo, void* stream) {
    if (batch < 0 || n < 0 || m < 0 || nsample < 1 || c1 < 1 || (y && ldy < c1) || ldo < c1) return ML3D_E_INVALID;
    const int64_t rows = batch * m * nsample;
    if (rows == 0) return 0;
    if (n == 0 || n >= (1ll << 31) || !points || !centres || !idx || !w_x || !b1 || !out) return ML3D_E_INVALID;
    hipLaunchKernelGGL(pn2_group_kernel, dim3(capped_grid((rows * c1 + 255) / 256, 65535)), dim3(256), 0, (hipStream_t)stream, y, ldy,
                       points, centres, idx, n, m, rows, nsample, c1, w_x, b1, out, ldo);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_pn2_interpolate(const float* known, int64_t ldk, int64_t batch, int64_t m_known, const int32_t* idx,
                                    const float* dist2, const float* weight, int64_t n, int c, float* out, int64_t ldo,
                                    void* stream) {
    if (batch < 0 || n < 0 || m_known < 0 || c < 1 || ldk < c || ldo < c || (dist2 != nullptr) == (weight != nullptr))
        return ML3D_E_INVALID;
    const int64_t rows = batch * n;
    if (m_known < 3) return ML3D_E_INVALID;
    if (rows == 0) return 0;
    if (!known || !idx || !out) return ML3D_E_INVALID;
    hipLaunchKernelGGL(pn2_interp_kernel, dim3(capped_grid((rows * c + 255) / 256, 65535)), dim3(256), 0, (hipStream_t)stream, known, ldk,
                       m_known, idx, dist2, weight, n, rows, c, out, ldo);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
