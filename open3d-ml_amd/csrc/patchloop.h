// patchloop.h — the per-element arithmetic of the spatially regular patch loop, shared by the single-cloud entries (knn.hip:
// ml3d_nearest_to_center*, ml3d_patch_crop, ml3d_patch_recenter) and the batched ones (patchloop.hip: ml3d_patch_batch).  The batched
// round must give every cloud the bits the single-cloud entries give it, so both call the SAME expressions; everything here is
// numpy's / scikit-learn's arithmetic in their order (ml3d_hip.h), compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ml3d {

// sklearn KDTree's order key: the float64 reduced distance (dx*dx + dy*dy) + dz*dz of the float32 point to the float32 centre
__device__ __forceinline__ double center_d2_f64(float x, float y, float z, double cx, double cy, double cz) {
    const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
    return (dx * dx + dy * dy) + dz * dz;      // three products, two sums, no FMA
}

// np.sum(np.square((pc - center).astype(np.float32)), axis=1): three float32 squares added left to right
__device__ __forceinline__ float patch_d2_f32(float x, float y, float z, const float* __restrict__ center) {
    const float dx = __fsub_rn(x, center[0]), dy = __fsub_rn(y, center[1]), dz = __fsub_rn(z, center[2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// np.square(1 - dists / np.max(dists)) in float32, added to the float64 possibility by the caller
__device__ __forceinline__ float patch_bump_f32(float d2, float d2max) {
    const float t = __fsub_rn(1.0f, __fdiv_rn(d2, d2max));
    return __fmul_rn(t, t);
}

// the 'normalize.feat' augmentation of one extra feature
__device__ __forceinline__ float patch_feat_f32(float v, float bias, float scale) { return __fdiv_rn(__fsub_rn(v, bias), scale); }

// mean_out[0..2] = numpy's mean(0) of the C-contiguous float32 [k, 3] array pts: the SEQUENTIAL float32 sum of a column over rows
// 0..k-1, divided by k.  To be called by all 256 threads of a workgroup (it holds barriers and 60 KB of LDS).
// Two LDS stages of 2 560 rows (column-major): waves 1..3 transpose stage i + 1 in while threads 0..2 of wave 0 add
// their column of stage i IN ROW ORDER -- the chain is the 45 056 dependent additions, so everything else is kept off it: the
// next stage's global reads and LDS writes run beside it, 16-byte LDS reads, eight of them (32 values) in flight under the 32
// adds of the previous block, two register blocks in ping-pong (no copies)
__device__ __forceinline__ void patch_mean_seq_body(const float* __restrict__ pts, int64_t k, float* __restrict__ mean_out) {
    constexpr int ROWS = 2560;            // 30 KB of LDS per stage
    __shared__ __attribute__((aligned(16))) float buf[2][3 * ROWS];
    auto fill = [&](int64_t base, float* dst, int first, int step) {
        if (base >= k) return;
        const int rows = (int)min<int64_t>(ROWS, k - base);
        for (int e = first; e < rows * 3; e += step) {
            const int r = e / 3, c = e - 3 * r;
            dst[c * ROWS + r] = pts[3 * base + e];
        }
    };
    fill(0, buf[0], threadIdx.x, 256);
    __syncthreads();
    float s = 0.f;
    int stage = 0;
    for (int64_t base = 0; base < k; base += ROWS, stage ^= 1) {
        const int rows = (int)min<int64_t>(ROWS, k - base);
        if (threadIdx.x >= 64) {
            fill(base + ROWS, buf[stage ^ 1], threadIdx.x - 64, 192);
        } else if (threadIdx.x < 3) {
            const float* col = buf[stage] + threadIdx.x * ROWS;
            const float4* col4 = reinterpret_cast<const float4*>(col);
            int r = 0;
            // blocks of 256 rows as STRAIGHT-LINE code, eight groups of 32 rows: the 16-byte LDS reads of group g + 1 are issued,
            // then the 32 dependent adds of group g run under them -- two register sets in ping-pong with nothing carried
            // around a loop (the rolled two-block loop this replaces paid a v_mov per add for half of the rows, the phi copies
            // of its prefetch registers); only a block's first group is exposed, once per 256 adds.  The scheduling barriers keep
            // the compiler from hoisting all 64 reads to the top (it did: the first add then waited for 46 of them).
            for (; r + 256 <= rows; r += 256) {
                const float4* c4 = col4 + r / 4;
                float4 a[8], b[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = c4[i];
#pragma unroll
                for (int g = 0; g < 8; g += 2) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) b[i] = c4[8 * (g + 1) + i];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { s = __fadd_rn(s, a[i].x); s = __fadd_rn(s, a[i].y); s = __fadd_rn(s, a[i].z); s = __fadd_rn(s, a[i].w); }
                    __builtin_amdgcn_sched_barrier(0);
                    if (g + 2 < 8) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) a[i] = c4[8 * (g + 2) + i];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { s = __fadd_rn(s, b[i].x); s = __fadd_rn(s, b[i].y); s = __fadd_rn(s, b[i].z); s = __fadd_rn(s, b[i].w); }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            for (; r < rows; ++r) s = __fadd_rn(s, col[r]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) mean_out[threadIdx.x] = __fdiv_rn(s, (float)k);
}

}  // namespace ml3d
