// PVCNN inference (ml3d/torch/models/pvcnn.py of the reference): the Voxelization normalisation with an exact contract, the
// deterministic scatter-mean onto a channels-last voxel grid, the entry point of the 3 x 3 x 3 convolution (the kernel is
// gemm.hip's bf16x3 tile kernel behind Conv3dLoader), the trilinear gather back to the points and the per-item column maximum.
// Contracts: include/ml3d_hip.h.  gfx950 only; the same source builds under tests/hipemu.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gemm.h"
#include "grid.h"
#include "ml3d_hip.h"
#include "sort.h"

namespace ml3d {

#define PV_T 1024
#define PV_WAVES (PV_T / 64)
#define PV_MAX_RES 8

// ---------------------------------------------------------------------------------------------------------------------------
// (a) voxel coordinates.  pv_stats: ONE workgroup per item, two sweeps over its [3][n] coordinates.  Thread t owns points t,
// t + 1024, ...; sums are carried in double (exact for any cloud whose coordinates span less than 2^13 in magnitude: 24 + 16 +
// 13 bits), reduced by shuffles and one LDS round in a FIXED order, rounded to float once.  The maximum norm is order-free.
// ---------------------------------------------------------------------------------------------------------------------------
// (sqrtf, not __fsqrt_rn: this toolchain's __fsqrt_rn is the NATIVE square root, 1 ulp off on some inputs, while sqrtf is the
//  correctly rounded one -- hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, which also makes __fdiv_rn's x / y exact)
__device__ __forceinline__ float pv_norm(float dx, float dy, float dz) {
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx))));
}

__global__ __launch_bounds__(PV_T) void pv_stats(const float* __restrict__ coords, int n, float* __restrict__ stats) {
    __shared__ double s_sum[3][PV_WAVES];
    __shared__ float s_max[PV_WAVES];
    __shared__ float s_mean[3];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* x = coords + (int64_t)b * 3 * n;
    const float* y = x + n;
    const float* z = y + n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = t; i < n; i += PV_T) { s0 += (double)x[i]; s1 += (double)y[i]; s2 += (double)z[i]; }
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_down(s0, o); s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); }
    if (lane == 0) { s_sum[0][wave] = s0; s_sum[1][wave] = s1; s_sum[2][wave] = s2; }
    __syncthreads();
    if (t < 3) {
        double s = 0.0;
        for (int w = 0; w < PV_WAVES; ++w) s += s_sum[t][w];
        s_mean[t] = __fdiv_rn((float)s, (float)n);
    }
    __syncthreads();
    const float mx = s_mean[0], my = s_mean[1], mz = s_mean[2];
    float best = 0.f;
    for (int i = t; i < n; i += PV_T)
        best = fmaxf(best, pv_norm(__fsub_rn(x[i], mx), __fsub_rn(y[i], my), __fsub_rn(z[i], mz)));
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_down(best, o));
    if (lane == 0) s_max[wave] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < PV_WAVES; ++w) best = fmaxf(best, s_max[w]);
        float* o = stats + 4 * b;
        o[0] = mx; o[1] = my; o[2] = mz;
        o[3] = __fadd_rn(__fmul_rn(best, 2.0f), 1e-6f);
    }
}

struct PvRes {
    int num;
    int r[PV_MAX_RES];
    float* v[PV_MAX_RES];
    int32_t* idx[PV_MAX_RES];
};

__device__ __forceinline__ float pv_axis(float x, float mean, float scale, int r) {
    const float v = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(x, mean), scale), 0.5f), (float)r);
    return fminf(fmaxf(v, 0.f), (float)(r - 1));
}

__global__ __launch_bounds__(256) void pv_coords(const float* __restrict__ coords, int n, int64_t total,
                                                 const float* __restrict__ stats, PvRes R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / n), p = (int)(i - (int64_t)b * n);
    const float* x = coords + (int64_t)b * 3 * n;
    const float px = x[p], py = x[n + p], pz = x[2 * (int64_t)n + p];
    const float* s = stats + 4 * b;
    const float mx = s[0], my = s[1], mz = s[2], scale = s[3];
    for (int k = 0; k < R.num; ++k) {
        const int r = R.r[k];
        const float vx = pv_axis(px, mx, scale, r), vy = pv_axis(py, my, scale, r), vz = pv_axis(pz, mz, scale, r);
        float* o = R.v[k] + 3 * i;
        o[0] = vx; o[1] = vy; o[2] = vz;
        // (a NaN coordinate -- not a cloud -- clamps to cell 0 instead of leaving the grid)
        int cx = (int)rintf(vx), cy = (int)rintf(vy), cz = (int)rintf(vz);
        cx = cx < 0 ? 0 : (cx > r - 1 ? r - 1 : cx);
        cy = cy < 0 ? 0 : (cy > r - 1 ? r - 1 : cy);
        cz = cz < 0 ? 0 : (cz > r - 1 ? r - 1 : cz);
        R.idx[k][i] = (cx * r + cy) * r + cz;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// (b) scatter-mean: stable radix sort of (item * r^3 + cell, point) pairs, then one thread per (head of a run, channels) adds the
// run's feature rows in ASCENDING point order -- the order a serial scatter_add visits them -- and divides by the count.  No float
// atomics: the same input gives the same bits.  Cells without a point keep the zero a fill kernel wrote.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_keys(const int32_t* __restrict__ vox, int64_t total, int n, int cells, u64 invalid,
                                               u64* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = vox[i];
    keys[i] = (c >= 0 && c < cells) ? (u64)(i / n) * (u64)cells + (u64)c : invalid;      // (a cell outside the grid: dropped)
    vals[i] = (uint32_t)i;
}

template <int VEC>
__global__ __launch_bounds__(256) void pv_segment_mean(const u64* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t total,
                                                       u64 invalid, const float* __restrict__ feat, int64_t ldf, int cq,
                                                       float* __restrict__ grid, int64_t ldg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total * cq) return;
    const int64_t p = t / cq;
    const int c = (int)(t - p * cq) * VEC;
    const u64 key = keys[p];
    if (key >= invalid || (p > 0 && keys[p - 1] == key)) return;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    int cnt = 0;
    for (int64_t j = p; j < total && keys[j] == key; ++j, ++cnt) {
        const float* f = feat + (int64_t)vals[j] * ldf + c;
        if (VEC == 4) {
            const float4 q = *reinterpret_cast<const float4*>(f);
            acc[0] = __fadd_rn(acc[0], q.x); acc[1] = __fadd_rn(acc[1], q.y);
            acc[VEC - 2] = __fadd_rn(acc[VEC - 2], q.z); acc[VEC - 1] = __fadd_rn(acc[VEC - 1], q.w);
        } else {
            acc[0] = __fadd_rn(acc[0], f[0]);
        }
    }
    const float d = (float)cnt;
    float* o = grid + (int64_t)key * ldg + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = __fdiv_rn(acc[e], d);
}

struct AvgVoxWs { u64* keys; uint32_t* vals; SortWs sort; };      // (key, point) pairs [batch * n] and the sort's scratch
static AvgVoxWs avg_vox_ws(WsLayout& L, int64_t m) {
    AvgVoxWs o;
    o.keys = L.take<u64>((size_t)m);
    o.vals = L.take<uint32_t>((size_t)m);
    o.sort = ws_nest(L, sort_ws, m);
    L.pad(256);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------------
// (d) trilinear gather.  One thread per (point, VEC channels): eight corner rows of the channels-last grid, contiguous runs.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pv_corner(float v, int r, int& lo, int& hi, float& f) {
    const float lof = floorf(v);
    f = __fsub_rn(v, lof);
    lo = (int)lof;
    lo = lo < 0 ? 0 : (lo > r - 1 ? r - 1 : lo);            // (v outside [0, r - 1] or NaN never leaves the grid)
    hi = lo + (f > 0.f ? 1 : 0);
    hi = hi > r - 1 ? r - 1 : hi;
    if (!(f >= 0.f && f <= 1.f)) f = 0.f;
}

template <int VEC>
__global__ __launch_bounds__(256) void pv_devoxelize(const float* __restrict__ grid, int64_t ldg, int r, int cq,
                                                     const float* __restrict__ v, int n, int64_t total,
                                                     const float* __restrict__ addend, int64_t lda, float* __restrict__ out,
                                                     int64_t ldc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total * cq) return;
    const int64_t i = t / cq;
    const int c = (int)(t - i * cq) * VEC;
    const int b = (int)(i / n);
    int lo[3], hi[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pv_corner(v[3 * i + a], r, lo[a], hi[a], f[a]);
    const float* g = grid + (int64_t)b * r * r * r * ldg + c;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int ix = (k & 4) ? hi[0] : lo[0], iy = (k & 2) ? hi[1] : lo[1], iz = (k & 1) ? hi[2] : lo[2];
        const float wx = (k & 4) ? f[0] : __fsub_rn(1.f, f[0]), wy = (k & 2) ? f[1] : __fsub_rn(1.f, f[1]);
        const float wz = (k & 1) ? f[2] : __fsub_rn(1.f, f[2]);
        const float w = __fmul_rn(__fmul_rn(wx, wy), wz);
        const float* q = g + (int64_t)((ix * r + iy) * r + iz) * ldg;
        if (VEC == 4) {
            const float4 u = *reinterpret_cast<const float4*>(q);
            acc[0] = fmaf(w, u.x, acc[0]); acc[1] = fmaf(w, u.y, acc[1]);
            acc[VEC - 2] = fmaf(w, u.z, acc[VEC - 2]); acc[VEC - 1] = fmaf(w, u.w, acc[VEC - 1]);
        } else {
            acc[0] = fmaf(w, q[0], acc[0]);
        }
    }
    if (addend) {
        const float* a = addend + i * lda + c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = __fadd_rn(acc[e], a[e]);
    }
    float* o = out + i * ldc + c;
    if (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[VEC - 2], acc[VEC - 1]);
    else o[0] = acc[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// (e) per-item column maximum in two steps (no atomics): PV_MAX_ROWS rows per workgroup, a thread per column (coalesced rows).
// ---------------------------------------------------------------------------------------------------------------------------
#define PV_MAX_ROWS 256

__global__ __launch_bounds__(256) void pv_colmax(const float* __restrict__ x, int64_t ldx, int64_t rows_per_item, int rows_per_block,
                                                 int c, float* __restrict__ out, int64_t out_item_stride, int64_t out_block_stride) {
    const int col = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (col >= c) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows_per_item ? r0 + rows_per_block : rows_per_item;
    const float* p = x + ((int64_t)blockIdx.z * rows_per_item + r0) * ldx + col;
    float m = -INFINITY;
    for (int64_t r = r0; r < r1; ++r, p += ldx) m = fmaxf(m, *p);
    out[(int64_t)blockIdx.z * out_item_stride + (int64_t)blockIdx.y * out_block_stride + col] = m;
}

}  // namespace ml3d

using namespace ml3d;

extern "C" int ml3d_pvcnn_voxel_coords(const float* coords, int64_t batch, int64_t n, const int32_t* resolutions_host,
                                       int num_resolutions, float* stats, float* const* out_v_host,
                                       int32_t* const* out_index_host, void* stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || n > 0x7fffffff / 4 || num_resolutions < 0 || num_resolutions > PV_MAX_RES ||
        !coords || !stats || (num_resolutions > 0 && (!resolutions_host || !out_v_host || !out_index_host)))
        return ML3D_E_INVALID;
    PvRes R;
    R.num = num_resolutions;
    for (int k = 0; k < PV_MAX_RES; ++k) { R.r[k] = 1; R.v[k] = nullptr; R.idx[k] = nullptr; }
    for (int k = 0; k < num_resolutions; ++k) {
        if (resolutions_host[k] < 1 || resolutions_host[k] > 1024 || !out_v_host[k] || !out_index_host[k]) return ML3D_E_INVALID;
        R.r[k] = resolutions_host[k]; R.v[k] = out_v_host[k]; R.idx[k] = out_index_host[k];
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pv_stats, dim3((unsigned)batch), dim3(PV_T), 0, st, coords, (int)n, stats);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    if (num_resolutions == 0) return 0;
    const int64_t total = batch * n;
    hipLaunchKernelGGL(pv_coords, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, coords, (int)n, total, (const float*)stats, R);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" size_t ml3d_avg_voxelize_workspace_bytes(int64_t batch, int64_t n) {
    if (batch <= 0 || n <= 0) return 0;
    return ws_bytes_of(avg_vox_ws, batch * n);
}

extern "C" int ml3d_avg_voxelize(const float* feat, int64_t ldf, int c, const int32_t* vox_index, int64_t batch, int64_t n, int r,
                                 float* grid, int64_t ldg, void* workspace, size_t workspace_bytes, void* stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || c <= 0 || r < 1 || r > 64 || ldf < c || ldg < c || !feat || !vox_index || !grid ||
        batch * n > 0x7fffffff / 4 || (((uintptr_t)grid) & 15) != 0)
        return ML3D_E_INVALID;
    const int64_t total = batch * n;
    const int cells = r * r * r;
    if ((int64_t)batch * cells * ldg >= ((int64_t)1 << 40)) return ML3D_E_INVALID;
    AvgVoxWs W;
    if (!workspace || !ws_carve(workspace, workspace_bytes, &W, avg_vox_ws, total)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const u64 invalid = (u64)batch * (u64)cells;
    const int key_bits = key_bits_for(invalid);
    const unsigned nb = (unsigned)((total + 255) / 256);
    zero_async(grid, sizeof(float) * (size_t)batch * (size_t)cells * (size_t)ldg, st);
    hipLaunchKernelGGL(pv_keys, dim3(nb), dim3(256), 0, st, vox_index, total, (int)n, cells, invalid, W.keys, W.vals);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    if (sort_pairs_u64(W.keys, W.vals, total, key_bits, W.sort, st, true)) return ML3D_E_LAUNCH;
    if (sort_result_in_alt(total, key_bits)) { W.keys = W.sort.keys_alt; W.vals = W.sort.vals_alt; }
    const bool vec = (c & 3) == 0 && (ldf & 3) == 0 && (ldg & 3) == 0 && (((uintptr_t)feat) & 15) == 0;
    const int cq = vec ? c / 4 : c;
    const unsigned ns = (unsigned)((total * cq + 255) / 256);
    if (vec) hipLaunchKernelGGL((pv_segment_mean<4>), dim3(ns), dim3(256), 0, st, (const u64*)W.keys, (const uint32_t*)W.vals, total, invalid, feat, ldf, cq, grid, ldg);
    else hipLaunchKernelGGL((pv_segment_mean<1>), dim3(ns), dim3(256), 0, st, (const u64*)W.keys, (const uint32_t*)W.vals, total, invalid, feat, ldf, cq, grid, ldg);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_conv3d_ndhwc_bf16x3(const float* in, int64_t batch, int d, int h, int w, int cin, const void* packed,
                                        const float* bias, int act, float slope, int cout, float* out, int64_t out_voxel_stride,
                                        void* stream) {
    if (batch <= 0 || batch > 65535 || d <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || act < 0 || act > 2 || !in || !packed ||
        !out || out_voxel_stride < cout)
        return ML3D_E_INVALID;
    Conv3dA A;
    A.in = in; A.B = (int)batch; A.D = d; A.H = h; A.W = w; A.C = cin;
    if (!gemm_conv3d_bf16x3_ok(A)) return ML3D_E_UNSUPPORTED;
    return gemm_conv3d_bf16x3(A, packed, cout, Epilogue::of(bias, act, slope), out, out_voxel_stride, (hipStream_t)stream);
}

extern "C" int ml3d_trilinear_devoxelize(const float* grid, int64_t ldg, int r, int c, const float* v, int64_t batch, int64_t n,
                                         const float* addend, int64_t lda, float* out, int64_t ldc, void* stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || c <= 0 || r < 1 || r > 1024 || ldg < c || ldc < c || (addend && lda < c) || !grid ||
        !v || !out || batch * n > 0x7fffffff / 4)
        return ML3D_E_INVALID;
    const int64_t total = batch * n;
    const bool vec = (c & 3) == 0 && (ldg & 3) == 0 && (ldc & 3) == 0 && (!addend || (lda & 3) == 0) &&
                     ((((uintptr_t)grid) | ((uintptr_t)out) | ((uintptr_t)addend)) & 15) == 0;
    const int cq = vec ? c / 4 : c;
    const unsigned nb = (unsigned)((total * cq + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((pv_devoxelize<4>), dim3(nb), dim3(256), 0, st, grid, ldg, r, cq, v, (int)n, total, addend, lda, out, ldc);
    else hipLaunchKernelGGL((pv_devoxelize<1>), dim3(nb), dim3(256), 0, st, grid, ldg, r, cq, v, (int)n, total, addend, lda, out, ldc);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" size_t ml3d_segment_max_rows_workspace_bytes(int64_t batch, int64_t n, int c) {
    if (batch <= 0 || n <= 0 || c <= 0) return 0;
    return sizeof(float) * (size_t)batch * (size_t)((n + PV_MAX_ROWS - 1) / PV_MAX_ROWS) * (size_t)c + 512;
}

extern "C" int ml3d_segment_max_rows(const float* x, int64_t ldx, int64_t batch, int64_t n, int c, float* out, int64_t ldo,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (batch <= 0 || batch > 65535 || n <= 0 || c <= 0 || ldx < c || ldo < c || !x || !out) return ML3D_E_INVALID;
    const int64_t chunks = (n + PV_MAX_ROWS - 1) / PV_MAX_ROWS;
    if (chunks > 65535) return ML3D_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < ml3d_segment_max_rows_workspace_bytes(batch, n, c)) return ML3D_E_WORKSPACE;
    float* part = (float*)ws_align(workspace);
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = (unsigned)((c + 255) / 256);
    hipLaunchKernelGGL(pv_colmax, dim3(gx, (unsigned)chunks, (unsigned)batch), dim3(256), 0, st, x, ldx, n, PV_MAX_ROWS, c, part,
                       chunks * c, (int64_t)c);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    hipLaunchKernelGGL(pv_colmax, dim3(gx, 1u, (unsigned)batch), dim3(256), 0, st, (const float*)part, (int64_t)c, chunks, (int)chunks, c,
                       out, ldo, (int64_t)0);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
