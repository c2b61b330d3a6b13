// SparseConvUnet inference (ml3d/torch/models/sparseconvnet.py of the reference): the voxel pyramid with its rulebooks built in
// one call from sorted 64-bit keys, the entry point of the rulebook convolution (the kernel is gemm.hip's bf16x3 tile kernel
// behind SparseConvLoader) and the BatchNorm + ReLU rows pass.  Contracts: include/ml3d_hip.h.  gfx950 only; the same source
// builds under tests/hipemu.
//
// Keys: (item << 36) | (x << 24) | (y << 12) | z -- ascending key order is ascending (item, x, y, z).  Level l + 1 holds the distinct
// coord >> 1 of level l; the halved keys of a sorted level are NOT sorted (x >> 1 merges two x planes whose y runs interleave), so
// every level is one more stable radix sort, over the fixed upper bound of n elements with the rows past the level's count carrying
// an invalid key that sorts last: the counts stay on the device, nothing is read back here.  Neighbours are found by binary search
// in the level's sorted unique keys (log2(M) probes of an L2-resident array; no table to size, no probing order to fix); a
// neighbour coordinate outside [0, grid_size) is rejected BEFORE a key is formed, so -1 and 4096 never alias another voxel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "grid.h"
#include "ml3d_hip.h"
#include "sort.h"

namespace ml3d {

#define SCN_MAX_LEVELS 12
#define SCN_MAX_ITEMS 4096
constexpr u64 SCN_XYZ = ((u64)1 << 36) - 1;
constexpr u64 SCN_HALF = 0x7FF7FF7FFull;          // (xyz >> 1) keeps 11 bits per axis

__device__ __forceinline__ int scn_x(u64 k) { return (int)((k >> 24) & 4095); }
__device__ __forceinline__ int scn_y(u64 k) { return (int)((k >> 12) & 4095); }
__device__ __forceinline__ int scn_z(u64 k) { return (int)(k & 4095); }
__device__ __forceinline__ int scn_parity_tap(u64 k) { return (int)(((k & 1) << 2) | (((k >> 12) & 1) << 1) | ((k >> 24) & 1)); }

// level 0 keys of one item's points [first, last): floor of the position (voxel centres are int + 0.5)
__global__ __launch_bounds__(256) void scn_point_keys(const float* __restrict__ points, int64_t first, int64_t last, u64 item,
                                                      int grid_size, u64 invalid, u64* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
    const int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= last) return;
    const float* p = points + 3 * i;
    const float fx = floorf(p[0]), fy = floorf(p[1]), fz = floorf(p[2]);
    const float g = (float)grid_size;
    // (a NaN fails every comparison: dropped like a point outside the grid)
    const bool ok = fx >= 0.f && fx < g && fy >= 0.f && fy < g && fz >= 0.f && fz < g;
    keys[i] = ok ? (item << 36) | ((u64)(int)fx << 24) | ((u64)(int)fy << 12) | (u64)(int)fz : invalid;
    vals[i] = (uint32_t)i;
}

// keys of the parents of level l's rows; rows past the level's count get the invalid key
__global__ __launch_bounds__(256) void scn_parent_keys(const u64* __restrict__ ukeys, const int32_t* __restrict__ count, int64_t n,
                                                       u64 invalid, u64* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 k = invalid;
    if (i < *count) {
        const u64 c = ukeys[i];
        k = (c & ~SCN_XYZ) | (((c & SCN_XYZ) >> 1) & SCN_HALF);
    }
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void scn_heads(const u64* __restrict__ keys, int64_t n, u64 invalid, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    flag[i] = (k < invalid && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void scn_fill_i32(int32_t* __restrict__ p, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__device__ __forceinline__ void scn_store_coord(int32_t* __restrict__ coords, int64_t row, u64 k) {
    int32_t* c = coords + 4 * row;
    c[0] = (int32_t)(k >> 36); c[1] = scn_x(k); c[2] = scn_y(k); c[3] = scn_z(k);
}

// level 0 from the sorted (key, point) pairs; `incl` = inclusive scan of the head flags.  The head of a run adds the run's feature
// rows in ASCENDING point order (the sort is stable and started from ascending values) and divides by the count.
__global__ __launch_bounds__(256) void scn_level0(const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  const int* __restrict__ incl, int64_t n, u64 invalid, const float* __restrict__ feat,
                                                  int64_t ldf, int cf, u64* __restrict__ ukeys, int32_t* __restrict__ coords,
                                                  int32_t* __restrict__ index_map, float* __restrict__ feat0, int64_t ldo,
                                                  int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *count = incl[i];
    const u64 k = keys[i];
    if (k >= invalid) { index_map[vals[i]] = -1; return; }
    const int row = incl[i] - 1;
    index_map[vals[i]] = row;
    if (i > 0 && keys[i - 1] == k) return;
    ukeys[row] = k;
    scn_store_coord(coords, row, k);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int64_t j = i; j < n && keys[j] == k; ++j, ++cnt) {
        const float* f = feat + (int64_t)vals[j] * ldf;
        for (int c = 0; c < cf; ++c) acc[c] = __fadd_rn(acc[c], f[c]);
    }
    const float d = (float)cnt;
    float* o = feat0 + (int64_t)row * ldo;
    for (int c = 0; c < cf; ++c) o[c] = __fdiv_rn(acc[c], d);
}

// level l + 1 from the sorted (parent key, child row) pairs: child -> (parent row, parity tap), parent -> its <= 8 children, and
// the transposed rulebook up8 (row c: parent at column tap, -1 elsewhere)
__global__ __launch_bounds__(256) void scn_level_up(const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    const int* __restrict__ incl, int64_t n, u64 invalid,
                                                    const u64* __restrict__ child_keys, u64* __restrict__ ukeys,
                                                    int32_t* __restrict__ coords, int32_t* __restrict__ parent,
                                                    int32_t* __restrict__ ptap, int32_t* __restrict__ up8, int32_t* __restrict__ child8,
                                                    int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *count = incl[i];
    const u64 k = keys[i];
    if (k >= invalid) return;
    const int row = incl[i] - 1;
    const int64_t c = (int64_t)vals[i];
    const int tap = scn_parity_tap(child_keys[c]);
    parent[c] = row;
    ptap[c] = tap;
    up8[8 * c + tap] = row;
    child8[8 * (int64_t)row + tap] = (int32_t)c;
    if (i > 0 && keys[i - 1] == k) return;
    ukeys[row] = k;
    scn_store_coord(coords, row, k);
}

// nbr27[row, t], t = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): the row of the voxel at (x + dx, y + dy, z + dz) of the same item
__global__ __launch_bounds__(256) void scn_neighbours(const u64* __restrict__ ukeys, const int32_t* __restrict__ count, int64_t n,
                                                      int grid_size, int32_t* __restrict__ nbr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 27) return;
    const int64_t row = t / 27;
    const int m = *count;
    if (row >= m) return;
    const int tap = (int)(t - row * 27);
    const int dz = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dx = tap % 3 - 1;
    const u64 k = ukeys[row];
    const int x = scn_x(k) + dx, y = scn_y(k) + dy, z = scn_z(k) + dz;
    int32_t found = -1;
    if (tap == 13) {
        found = (int32_t)row;
    } else if (x >= 0 && x < grid_size && y >= 0 && y < grid_size && z >= 0 && z < grid_size) {
        const u64 want = (k & ~SCN_XYZ) | ((u64)x << 24) | ((u64)y << 12) | (u64)z;
        int lo = 0, hi = m;                        // first key >= want
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ukeys[mid] < want) lo = mid + 1; else hi = mid;
        }
        if (lo < m && ukeys[lo] == want) found = lo;
    }
    nbr[t] = found;
}

// out = max(in * scale + shift, 0) on rows (unfused multiply and add, the order of an eval-mode BatchNorm written as scale / shift)
__global__ __launch_bounds__(256) void scn_bn_relu_rows(const float* __restrict__ in, int64_t ldi, int64_t m, int c,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, int64_t ldo) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * c) return;
    const int64_t r = t / c;
    const int col = (int)(t - r * c);
    const float v = __fadd_rn(__fmul_rn(in[r * ldi + col], scale[col]), shift[col]);
    out[r * ldo + col] = v > 0.f ? v : 0.f;
}

// keys, vals [n]; incl [n] head flags -> inclusive scan; block_sums: scan scratch; ukeys [levels][n] the unique keys of every level
struct ScnBuildWs { u64* keys; uint32_t* vals; int *incl, *block_sums; u64* ukeys; SortWs sort; };
static ScnBuildWs scn_build_ws(WsLayout& L, int64_t n, int levels) {
    ScnBuildWs o;
    o.keys = L.take<u64>((size_t)n);
    o.vals = L.take<uint32_t>((size_t)n);
    o.incl = L.take<int>((size_t)n);
    o.block_sums = L.take<int>((size_t)((n + 1023) / 1024 + 2));
    o.ukeys = L.take<u64>((size_t)n * (size_t)levels);
    o.sort = ws_nest(L, sort_ws, n);
    L.pad(768);
    return o;
}

static inline unsigned scn_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace ml3d

using namespace ml3d;

extern "C" size_t ml3d_scn_build_workspace_bytes(int64_t n, int levels) {
    if (n <= 0 || levels <= 0 || levels > SCN_MAX_LEVELS) return 0;
    return ws_bytes_of(scn_build_ws, n, levels);
}

extern "C" int ml3d_scn_build(const float* points, const float* feat, int64_t ldf, int feat_channels, int64_t n,
                              const int64_t* row_splits_host, int batch, int levels, int grid_size, int32_t* counts,
                              int32_t* coords, int32_t* nbr27, int32_t* child8, int32_t* parent, int32_t* ptap, int32_t* up8,
                              int32_t* index_map, float* feat0, int64_t ldo, void* workspace, size_t workspace_bytes, void* stream) {
    if (!points || !feat || !row_splits_host || !counts || !coords || !nbr27 || !child8 || !parent || !ptap || !up8 || !index_map ||
        !feat0 || n <= 0 || n > 0x7fffffff / 32 || batch <= 0 || batch > SCN_MAX_ITEMS || levels <= 0 || levels > SCN_MAX_LEVELS ||
        grid_size < 1 || grid_size > 4096 || feat_channels < 1 || feat_channels > 4 || ldf < feat_channels || ldo < feat_channels)
        return ML3D_E_INVALID;
    if (row_splits_host[0] != 0 || row_splits_host[batch] != n) return ML3D_E_INVALID;
    for (int b = 0; b < batch; ++b)
        if (row_splits_host[b + 1] < row_splits_host[b]) return ML3D_E_INVALID;
    ScnBuildWs W;
    if (!workspace || !ws_carve(workspace, workspace_bytes, &W, scn_build_ws, n, levels)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const u64 invalid = (u64)batch << 36;
    const int key_bits = key_bits_for(invalid);
    const unsigned nb = scn_blocks(n);

    // rulebook entries nobody writes are -1 (absent child / not this row's parity); rows past a level's count stay -1 as well
    hipLaunchKernelGGL(scn_fill_i32, dim3(scn_blocks(n * 8 * levels)), dim3(256), 0, st, child8, n * 8 * levels, (int32_t)-1);
    hipLaunchKernelGGL(scn_fill_i32, dim3(scn_blocks(n * 8 * levels)), dim3(256), 0, st, up8, n * 8 * levels, (int32_t)-1);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;

    for (int b = 0; b < batch; ++b) {
        const int64_t first = row_splits_host[b], last = row_splits_host[b + 1];
        if (last == first) continue;
        hipLaunchKernelGGL(scn_point_keys, dim3(scn_blocks(last - first)), dim3(256), 0, st, points, first, last, (u64)b, grid_size,
                           invalid, W.keys, W.vals);
    }
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    for (int l = 0; l < levels; ++l) {
        u64* uk = W.ukeys + (size_t)l * (size_t)n;
        int32_t* co = coords + (size_t)l * (size_t)n * 4;
        if (l > 0) {
            hipLaunchKernelGGL(scn_parent_keys, dim3(nb), dim3(256), 0, st, (const u64*)(uk - n), (const int32_t*)(counts + l - 1), n,
                               invalid, W.keys, W.vals);
            if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
        }
        if (sort_pairs_u64(W.keys, W.vals, n, key_bits, W.sort, st, true)) return ML3D_E_LAUNCH;
        const bool alt = sort_result_in_alt(n, key_bits);
        const u64* sk = alt ? W.sort.keys_alt : W.keys;
        const uint32_t* sv = alt ? W.sort.vals_alt : W.vals;
        hipLaunchKernelGGL(scn_heads, dim3(nb), dim3(256), 0, st, sk, n, invalid, W.incl);
        if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
        if (scan_inclusive_i32(W.incl, n, W.block_sums, st)) return ML3D_E_LAUNCH;
        if (l == 0) {
            hipLaunchKernelGGL(scn_level0, dim3(nb), dim3(256), 0, st, sk, sv, (const int*)W.incl, n, invalid, feat, ldf, feat_channels, uk,
                               co, index_map, feat0, ldo, counts);
        } else {
            const size_t lo = (size_t)(l - 1) * (size_t)n;
            hipLaunchKernelGGL(scn_level_up, dim3(nb), dim3(256), 0, st, sk, sv, (const int*)W.incl, n, invalid, (const u64*)(uk - n), uk, co,
                               parent + lo, ptap + lo, up8 + lo * 8, child8 + (size_t)l * (size_t)n * 8, counts + l);
        }
        if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
        hipLaunchKernelGGL(scn_neighbours, dim3(scn_blocks(n * 27)), dim3(256), 0, st, (const u64*)uk, (const int32_t*)(counts + l), n,
                           grid_size, nbr27 + (size_t)l * (size_t)n * 27);
        if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    }
    return 0;
}

extern "C" int ml3d_sparse_conv_bf16x3(const float* in, int64_t ldi, int64_t in_rows, int cp, const int32_t* rule, int taps,
                                       int64_t m, const float* a2, int64_t lda2, int k2, const void* packed, int n,
                                       const float* bias, const float* residual, int64_t ldr, int act, float slope, float* out,
                                       int64_t ldc, void* stream) {
    if (act < 0 || act > 2 || !out || ldc < n || (residual && ldr < n)) return ML3D_E_INVALID;
    SparseConvA A = {in, ldi, in_rows, cp, rule, taps, a2, lda2, k2};
    return gemm_sparse_conv_bf16x3(A, m, packed, n, Epilogue::of(bias, act, slope).residual_rows(residual, ldr), out, ldc, (hipStream_t)stream);
}

extern "C" int ml3d_scn_bn_relu(const float* in, int64_t ldi, int64_t m, int c, const float* scale, const float* shift, float* out,
                                int64_t ldo, void* stream) {
    if (!in || !scale || !shift || !out || m < 0 || c <= 0 || ldi < c || ldo < c || m * c > 0x7fffffffll * 128) return ML3D_E_INVALID;
    if (m == 0) return 0;
    hipLaunchKernelGGL(scn_bn_relu_rows, dim3(scn_blocks(m * c)), dim3(256), 0, (hipStream_t)stream, in, ldi, m, c, scale, shift, out, ldo);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
