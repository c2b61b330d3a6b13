// patchloop.hip — the spatially regular patch loop for SEVERAL clouds in lock step (gfx950; ml3d_hip.h, "multi-cloud patch loop").
//
// The single-cloud loop (knn.hip: ml3d_nearest_to_center_dev -> ml3d_patch_crop -> ml3d_patch_recenter) is a chain of small,
// dependent launches per patch -- an 8-pass radix sort of one cloud, one workgroup adding 45 056 floats in order -- and C clouds
// make C such chains.  The patches of a cloud depend on nothing but that cloud's possibilities and its own shuffles, so the
// clouds can advance together: one round here cuts one patch out of EVERY active cloud, bit for bit the patch the single-cloud
// entries would cut (the arithmetic is shared through patchloop.h), with the launches of one chain:
//   ml3d_possibility_argmin   per-tile partial (minimum, first index) -> one wave per cloud combines them   [2 launches]
//   ml3d_patch_batch          keys of all active points -> ONE 64-bit sort by distance -> one stable 8-bit pass by cloud ->
//                             crop + distances + maxima -> possibility bump -> the A sequential means SIDE BY SIDE (one workgroup
//                             per cloud) -> recentre + features
// KPFCNN's input-sphere loop (kpconv.py:446-531) advances several clouds the same way, one SUB-ROUND per sphere:
//   ml3d_sphere_select        keys (cloud, float32 d2 | all ones outside the radius) -> ONE sort -> the leading hits of every segment
//   ml3d_sphere_batch         gather through the shuffle + distances + maxima -> possibility bump -> the sequential means side by side
//                             -> in-place rescale of the clouds' cached colours -> recentre + columns + cut + colour drop
// The clouds lie back to back in device arrays; their boundaries (cloud_row_splits) and the list of active slots are HOST arrays,
// read during the call and carried to the kernels by value (PbItems): no upload, no allocation, kernel nodes only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grid.h"
#include "ml3d_hip.h"
#include "patchloop.h"
#include "sort.h"

namespace ml3d {

constexpr int PB_ITEMS = 64;          // active clouds one launch serves (a call with more launches its item kernels in chunks)
constexpr int PB_MAX_CLOUDS = 256;    // the cloud of a point is an 8-bit sort key
constexpr int PB_TILE = 2048;         // possibilities per argmin tile (256 threads x 8)

// the active clouds of one launch, by value in the kernel arguments (1.3 KB)
struct PbItems {
    int slot[PB_ITEMS];        // cloud slot (index into cloud_row_splits / the per-cloud outputs)
    int start[PB_ITEMS];       // first row of the cloud in the concatenated arrays
    int len[PB_ITEMS];         // its number of points
    int cstart[PB_ITEMS];      // first position of the cloud among the points of the ACTIVE clouds (the sort's index space)
    int tile0[PB_ITEMS];       // first argmin tile of the cloud
    int first;                 // ordinal of item 0 of this launch among the active clouds of the call
};

// (value, index) pairs order like np.argmin: the smaller value, on equal values the smaller index
__device__ __forceinline__ void argmin_take(double& v, int& i, double ov, int oi) {
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void argmin_wave(double& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        argmin_take(v, i, ov, oi);
    }
}
constexpr int ARGMIN_NONE = 0x7fffffff;

// stage one: tile blockIdx.x of item blockIdx.y (tiles never cross a cloud boundary) -> its minimum and the first index holding it
__global__ void __launch_bounds__(256)
pb_argmin_tiles(const double* __restrict__ poss, PbItems it, double* __restrict__ part_v, int* __restrict__ part_i) {
    __shared__ double sv[4];
    __shared__ int si[4];
    const int a = blockIdx.y;
    const int len = it.len[a];
    const int t0 = (int)blockIdx.x * PB_TILE;
    if (t0 >= len) return;                                   // (uniform over the workgroup)
    const int end = min(len, t0 + PB_TILE);
    const double* p = poss + it.start[a];
    double v = __longlong_as_double(0x7ff0000000000000ll);   // +inf
    int idx = ARGMIN_NONE;
    for (int i = t0 + (int)threadIdx.x; i < end; i += 256) {
        const double x = p[i];
        if (x < v || idx == ARGMIN_NONE) { v = x; idx = i; }  // ascending i per thread: '<' keeps the first
    }
    argmin_wave(v, idx);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) argmin_take(v, idx, sv[w], si[w]);
        part_v[it.tile0[a] + blockIdx.x] = v;
        part_i[it.tile0[a] + blockIdx.x] = idx;
    }
}

// stage two: one wave per item combines its tiles' partial results
__global__ void __launch_bounds__(64)
pb_argmin_final(const double* __restrict__ part_v, const int* __restrict__ part_i, PbItems it, int32_t* __restrict__ out_index,
                double* __restrict__ out_min) {
    const int a = blockIdx.x;
    const int tiles = (it.len[a] + PB_TILE - 1) / PB_TILE;
    double v = __longlong_as_double(0x7ff0000000000000ll);
    int idx = ARGMIN_NONE;
    for (int t = threadIdx.x; t < tiles; t += 64) argmin_take(v, idx, part_v[it.tile0[a] + t], part_i[it.tile0[a] + t]);
    argmin_wave(v, idx);
    if (threadIdx.x == 0) { out_index[it.slot[a]] = idx; out_min[it.slot[a]] = v; }
}

// the centre of the cloud in `slot` (rows [start, start + len)): the point its argmin picked (an index outside the cloud is
// clamped, never followed)
__device__ __forceinline__ const float* pb_center(const float* __restrict__ pts, int start, int len, int slot,
                                                  const int32_t* __restrict__ center_index) {
    int c = center_index[slot];
    c = c < 0 ? 0 : (c >= len ? len - 1 : c);
    return pts + 3 * ((int64_t)start + c);
}

// sort keys of the points of the active clouds: position cstart[a] + i <- (float64 reduced distance to the cloud's own centre, i)
__global__ void __launch_bounds__(256)
pb_keys(const float* __restrict__ pts, PbItems it, const int32_t* __restrict__ center_index, u64* __restrict__ keys,
        uint32_t* __restrict__ vals, uint32_t* __restrict__ item_of) {
    const int a = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= it.len[a]) return;
    const float* c = pb_center(pts, it.start[a], it.len[a], it.slot[a], center_index);
    const float* p = pts + 3 * ((int64_t)it.start[a] + i);
    const double d2 = center_d2_f64(p[0], p[1], p[2], (double)c[0], (double)c[1], (double)c[2]);
    const int64_t pos = (int64_t)it.cstart[a] + i;
    keys[pos] = (u64)__double_as_longlong(d2);
    vals[pos] = (uint32_t)pos;                                // ascending within a cloud: the stable sort breaks ties by index
    item_of[pos] = (uint32_t)(it.first + a);
}

// the second sort's key: the cloud (ordinal among the active ones) of the point now at sorted position i
__global__ void __launch_bounds__(256)
pb_item_keys(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ item_of, int64_t m, u64* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) keys[i] = (u64)item_of[vals[i]];
}

// ml3d_patch_crop's gather for item blockIdx.y: sorted[cstart .. cstart + len) are the cloud's points by ascending distance
__global__ void __launch_bounds__(256)
pb_gather(const float* __restrict__ pts, const uint32_t* __restrict__ sorted, PbItems it, const int32_t* __restrict__ center_index,
          const int32_t* __restrict__ perm, int64_t k, float* __restrict__ out_pts, int32_t* __restrict__ out_sel,
          int32_t* __restrict__ out_row, float* __restrict__ d2, unsigned* __restrict__ d2max_bits) {
    const int a = blockIdx.y;
    const int64_t item = it.first + a;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float d = 0.f;
    if (j < k) {
        int32_t q = perm[item * k + j];
        q = q < 0 ? 0 : (q >= k ? (int32_t)(k - 1) : q);       // (a shuffle of 0..k-1; anything else is clamped, never followed)
        const int32_t i = (int32_t)(sorted[(int64_t)it.cstart[a] + q] - (uint32_t)it.cstart[a]);
        const int64_t row = (int64_t)it.start[a] + i;
        const float x = pts[3 * row], y = pts[3 * row + 1], z = pts[3 * row + 2];
        const int64_t o = item * k + j;
        out_pts[3 * o] = x; out_pts[3 * o + 1] = y; out_pts[3 * o + 2] = z;
        out_sel[o] = i;
        out_row[o] = (int32_t)row;
        d = patch_d2_f32(x, y, z, pb_center(pts, it.start[a], it.len[a], it.slot[a], center_index));
        d2[o] = d;
    }
    // max of non-negative floats == max of their bit patterns
    unsigned b = __float_as_uint(d);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, o));
    if ((threadIdx.x & 63) == 0) atomicMax(d2max_bits + item, b);
}

__global__ void __launch_bounds__(256)
pb_bump(const int32_t* __restrict__ out_row, const float* __restrict__ d2, const unsigned* __restrict__ d2max_bits, int64_t k,
        double* __restrict__ possibility) {
    const int64_t item = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const int64_t o = item * k + j;
    possibility[out_row[o]] += (double)patch_bump_f32(d2[o], __uint_as_float(d2max_bits[item]));
}

// the A sequential column sums side by side: one workgroup per item
__global__ void __launch_bounds__(256)
pb_mean_seq(const float* __restrict__ pts, int64_t k, float* __restrict__ mean) {
    patch_mean_seq_body(pts + 3 * k * (int64_t)blockIdx.x, k, mean + 4 * (int64_t)blockIdx.x);
}

__global__ void __launch_bounds__(256)
pb_apply(float* __restrict__ pts, int64_t k, int dims_mask, const float* __restrict__ mean, const int32_t* __restrict__ out_row,
         const float* __restrict__ extra, int n_extra, float bias, float scale, float* __restrict__ feats) {
    const int64_t item = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const int64_t o = item * k + j;
    const int C = 3 + n_extra;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float v = pts[3 * o + d];
        if (dims_mask & (1 << d)) { v = __fsub_rn(v, mean[4 * item + d]); pts[3 * o + d] = v; }
        feats[o * C + d] = v;
    }
    const float* ex = n_extra ? extra + (int64_t)out_row[o] * n_extra : nullptr;
    for (int c = 0; c < n_extra; ++c) feats[o * C + 3 + c] = patch_feat_f32(ex[c], bias, scale);
}

// ---- the sphere loop of KPFCNN (kpconv.py:446-531 around semseg_spatially_regular.py:62-108) for several clouds -----------------------
// ml3d_sphere_select: the radius query of every active cloud's centre as ONE sort.  Key of point i of item a = (a, bits of its
// float32 distance) for a point inside the sphere, (a, all ones) for one outside: after the stable sort an item's hits stand first in
// its segment, ascending in (d2, index) -- ml3d_radius_fill's row for that query (the same dist2_canon, the same d2 <= r * r).
__global__ void __launch_bounds__(256)
ss_keys(const float* __restrict__ pts, PbItems it, const int32_t* __restrict__ center_index, float r2, u64* __restrict__ keys,
        uint32_t* __restrict__ vals, int* __restrict__ cnt) {
    const int a = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if ((int)blockIdx.x * 256 >= it.len[a]) return;           // (uniform over the workgroup)
    bool hit = false;
    if (i < it.len[a]) {
        const float* c = pb_center(pts, it.start[a], it.len[a], it.slot[a], center_index);
        const float* p = pts + 3 * ((int64_t)it.start[a] + i);
        const float d2 = dist2_canon(c[0], c[1], c[2], p[0], p[1], p[2]);
        hit = d2 <= r2;
        const int64_t pos = (int64_t)it.cstart[a] + i;
        keys[pos] = ((u64)(uint32_t)(it.first + a) << 32) | (u64)(hit ? __float_as_uint(d2) : 0xffffffffu);
        vals[pos] = (uint32_t)pos;
    }
    const int n = __popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt + it.first + a, n);
}

// the lists back to back in active order: item a's starts at the sum of the counts before it (at most 255 of them, summed per workgroup)
__global__ void __launch_bounds__(256)
ss_emit(const uint32_t* __restrict__ sorted, PbItems it, const int* __restrict__ cnt, int32_t* __restrict__ out_index,
        int32_t* __restrict__ out_count) {
    __shared__ int part[4];
    const int a = blockIdx.y;
    const int item = it.first + a;
    const int n = cnt[item];
    if (blockIdx.x == 0 && threadIdx.x == 0) out_count[it.slot[a]] = n;
    if ((int)blockIdx.x * 256 >= n) return;                   // (uniform over the workgroup)
    int v = (int)threadIdx.x < item ? cnt[threadIdx.x] : 0;   // item < PB_MAX_CLOUDS == 256 threads
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const int64_t off = (int64_t)part[0] + part[1] + part[2] + part[3];
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j < n) out_index[off + j] = (int32_t)(sorted[(int64_t)it.cstart[a] + j] - (uint32_t)it.cstart[a]);
}

// ml3d_sphere_batch: the spheres of one call, by value in the kernel arguments (2.6 KB)
struct SbItems {
    int start[PB_ITEMS];       // first row of the sphere's cloud in the concatenated arrays
    int len[PB_ITEMS];         // the cloud's number of points
    int center[PB_ITEMS];      // slot of the cloud (index into center_index)
    int cand[PB_ITEMS];        // first entry of the sphere's candidate list
    int n[PB_ITEMS];           // its length = the sphere's points before the cut
    int in0[PB_ITEMS];         // first entry of the sphere in perm and in the per-point scratch
    int keep0[PB_ITEMS];       // first entry of its rows in keep; -1: no cut
    int out0[PB_ITEMS];        // first output row
    int m[PB_ITEMS];           // output rows
    int zero[PB_ITEMS];        // columns 3.. of the output are multiplied by zero
    int first;                 // ordinal of item 0 of this launch among the items of the call
};

// picked = cand[perm]; distances to the centre and their maximum; sphere = p - centre (rows in the shuffle's order)
__global__ void __launch_bounds__(256)
sb_gather(const float* __restrict__ pts, SbItems it, const int32_t* __restrict__ center_index, const int32_t* __restrict__ cand,
          const int32_t* __restrict__ perm, float* __restrict__ sph, int32_t* __restrict__ row_of, float* __restrict__ d2,
          unsigned* __restrict__ d2max_bits) {
    const int a = blockIdx.y;
    const int n = it.n[a];
    if ((int)blockIdx.x * 256 >= n) return;                   // (uniform over the workgroup)
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    float d = 0.f;
    if (j < n) {
        int q = perm[(int64_t)it.in0[a] + j];
        q = q < 0 ? 0 : (q >= n ? n - 1 : q);                 // (a shuffle of 0..n-1; anything else is clamped, never followed)
        int i = cand[(int64_t)it.cand[a] + q];
        i = i < 0 ? 0 : (i >= it.len[a] ? it.len[a] - 1 : i);
        const int64_t row = (int64_t)it.start[a] + i;
        const float* c = pb_center(pts, it.start[a], it.len[a], it.center[a], center_index);
        const float x = pts[3 * row], y = pts[3 * row + 1], z = pts[3 * row + 2];
        const int64_t o = (int64_t)it.in0[a] + j;
        d = patch_d2_f32(x, y, z, c);
        d2[o] = d;
        row_of[o] = (int32_t)row;
        sph[3 * o] = __fsub_rn(x, c[0]); sph[3 * o + 1] = __fsub_rn(y, c[1]); sph[3 * o + 2] = __fsub_rn(z, c[2]);
    }
    unsigned b = __float_as_uint(d);                          // max of non-negative floats == max of their bit patterns
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, o));
    if ((threadIdx.x & 63) == 0) atomicMax(d2max_bits + it.first + a, b);
}

__global__ void __launch_bounds__(256)
sb_bump(SbItems it, const int32_t* __restrict__ row_of, const float* __restrict__ d2, const unsigned* __restrict__ d2max_bits,
        double* __restrict__ possibility) {
    const int a = blockIdx.y;
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= it.n[a]) return;
    const int64_t o = (int64_t)it.in0[a] + j;
    possibility[row_of[o]] += (double)patch_bump_f32(d2[o], __uint_as_float(d2max_bits[it.first + a]));
}

// the sequential column sums of the spheres side by side: one workgroup per item
__global__ void __launch_bounds__(256)
sb_mean_seq(const float* __restrict__ sph, SbItems it, float* __restrict__ mean) {
    const int a = blockIdx.x;
    patch_mean_seq_body(sph + 3 * (int64_t)it.in0[a], it.n[a], mean + 4 * (int64_t)(it.first + a));
}

// trans_normalize's 'linear' rescale of the cloud's CACHED features, in place, once per sphere (kpconv.py:500-503 through
// transforms.py:18-22: the reference renormalises the cached array every time, cumulatively)
__global__ void __launch_bounds__(256)
sb_rescale(float* __restrict__ extra, SbItems it, int n_extra, float bias, float scale) {
    const int a = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)it.len[a] * n_extra) return;
    float* p = extra + (int64_t)it.start[a] * n_extra + e;
    *p = patch_feat_f32(*p, bias, scale);
}

// recentre on the mean, columns = [sphere | extra[picked]], the cut (rows keep), the colour drop
__global__ void __launch_bounds__(256)
sb_emit(SbItems it, const float* __restrict__ sph, const int32_t* __restrict__ row_of, const float* __restrict__ mean,
        const int32_t* __restrict__ keep, int dims_mask, const float* __restrict__ extra, int n_extra, float* __restrict__ out_pts,
        float* __restrict__ out_columns, int32_t* __restrict__ out_sel, int32_t* __restrict__ out_row) {
    const int a = blockIdx.y;
    const int jo = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (jo >= it.m[a]) return;
    int j = jo;
    if (it.keep0[a] >= 0) {
        j = keep[(int64_t)it.keep0[a] + jo];
        j = j < 0 ? 0 : (j >= it.n[a] ? it.n[a] - 1 : j);
    }
    const int64_t i = (int64_t)it.in0[a] + j, o = (int64_t)it.out0[a] + jo;
    const int C = 3 + n_extra;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float v = sph[3 * i + d];
        if (dims_mask & (1 << d)) v = __fsub_rn(v, mean[4 * (int64_t)(it.first + a) + d]);
        out_pts[3 * o + d] = v;
        out_columns[o * C + d] = v;
    }
    const int32_t row = row_of[i];
    for (int c = 0; c < n_extra; ++c) {
        const float v = extra[(int64_t)row * n_extra + c];
        out_columns[o * C + 3 + c] = it.zero[a] ? __fmul_rn(v, 0.f) : v;      // columns[:, 3:] *= 0 (kpconv.py:526-527)
    }
    out_sel[o] = row - it.start[a];
    out_row[o] = row;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// the active clouds of a call, checked: splits monotone from 0, slots strictly ascending (so distinct) and inside [0, n_clouds),
// every active cloud with at least min_len points.  Returns the points of the active clouds, < 0 on a bad argument.
static int64_t pb_check(const int64_t* splits, int64_t n_clouds, const int32_t* active, int64_t n_active, int64_t min_len) {
    if (!splits || !active || n_clouds < 1 || n_clouds > PB_MAX_CLOUDS || n_active < 1 || n_active > n_clouds) return -1;
    if (splits[0] != 0) return -1;
    for (int64_t c = 0; c < n_clouds; ++c)
        if (splits[c + 1] < splits[c]) return -1;
    if (splits[n_clouds] > 0x7ffffff0ll) return -1;
    int64_t m = 0;
    for (int64_t a = 0; a < n_active; ++a) {
        const int64_t s = active[a];
        if (s < 0 || s >= n_clouds || (a > 0 && s <= active[a - 1])) return -1;
        const int64_t len = splits[s + 1] - splits[s];
        if (len < 1 || len < min_len) return -1;
        m += len;
    }
    return m;
}

// items [first, first + count) of the call as a kernel argument; *longest = the longest of them
static PbItems pb_items(const int64_t* splits, const int32_t* active, int64_t first, int count, int* longest) {
    PbItems it;
    int64_t cstart = 0, tile0 = 0;
    for (int64_t a = 0; a < first; ++a) {
        const int64_t len = splits[active[a] + 1] - splits[active[a]];
        cstart += len;
        tile0 += (len + PB_TILE - 1) / PB_TILE;
    }
    *longest = 0;
    for (int a = 0; a < PB_ITEMS; ++a) {
        const bool live = a < count;
        const int64_t s = live ? active[first + a] : 0;
        const int64_t len = live ? splits[s + 1] - splits[s] : 0;
        it.slot[a] = (int)s; it.start[a] = live ? (int)splits[s] : 0; it.len[a] = (int)len;
        it.cstart[a] = (int)cstart; it.tile0[a] = (int)tile0;
        cstart += len;
        tile0 += (len + PB_TILE - 1) / PB_TILE;
        if (len > *longest) *longest = (int)len;
    }
    it.first = (int)first;
    return it;
}

// the active clouds of a call in chunks of PB_ITEMS: launch(items of the chunk, their number, the longest of them)
template <class F>
static void pb_chunks(const int64_t* splits, const int32_t* active, int64_t n_active, F&& launch) {
    for (int64_t first = 0; first < n_active; first += PB_ITEMS) {
        const int count = n_active - first < PB_ITEMS ? (int)(n_active - first) : PB_ITEMS;
        int longest;
        const PbItems it = pb_items(splits, active, first, count, &longest);
        launch(it, count, longest);
    }
}

// ---- workspace layouts (workspace.h), one per op ---------------------------------------------------------------------------------------
struct ArgminWs { double* part_v; int* part_i; };      // [tiles] each: a tile's minimum and where it is
static ArgminWs argmin_ws(WsLayout& L, int64_t n_points, int64_t n_clouds) {
    const size_t tiles = (size_t)(n_points / PB_TILE + n_clouds + 1);
    ArgminWs o;
    o.part_v = L.take<double>(tiles);
    o.part_i = L.take<int>(tiles);
    L.pad(256);
    return o;
}

// mx [n_active] bits of the largest float32 distance, mean [n_active][4] column means, d2 [n_active][k]; keys .. item_of [m]
struct PatchBatchWs { unsigned* mx; float *mean, *d2; u64* keys; uint32_t *vals, *item_of; SortWs sort; };
// mx, mean and d2 stay neighbours in this order: the op zeroes mx and mean with ONE fill, from mx up to d2
static PatchBatchWs patch_batch_ws(WsLayout& L, int64_t n_points, int64_t n_active, int64_t k) {
    const int64_t m = n_points > 0 ? n_points : 1;
    PatchBatchWs o;
    o.mx = L.take<unsigned>((size_t)n_active);
    o.mean = L.take<float>(4 * (size_t)n_active);
    o.d2 = L.take<float>((size_t)n_active * (size_t)k);
    o.keys = L.take<u64>((size_t)m);
    o.vals = L.take<uint32_t>((size_t)m);
    o.item_of = L.take<uint32_t>((size_t)m);
    o.sort = ws_nest(L, sort_ws, m);
    L.pad(256);
    return o;
}

struct SphereSelectWs { int* cnt; u64* keys; uint32_t* vals; SortWs sort; };      // cnt [n_active]: hits per item
static SphereSelectWs sphere_select_ws(WsLayout& L, int64_t n_points, int64_t n_active) {
    const int64_t m = n_points > 0 ? n_points : 1;
    SphereSelectWs o;
    o.cnt = L.take<int>((size_t)(n_active > 0 ? n_active : 1));
    o.keys = L.take<u64>((size_t)m);
    o.vals = L.take<uint32_t>((size_t)m);
    o.sort = ws_nest(L, sort_ws, m);
    L.pad(256);
    return o;
}

// mx, mean as above; sph [n_in][3] p - centre, in the shuffle's order; d2, row_of [n_in]
struct SphereBatchWs { unsigned* mx; float *mean, *sph, *d2; int32_t* row_of; };
// mx, mean and sph stay neighbours in this order: the op zeroes mx and mean with ONE fill, from mx up to sph
static SphereBatchWs sphere_batch_ws(WsLayout& L, int64_t n_items, int64_t n_in) {
    const size_t a = (size_t)(n_items > 0 ? n_items : 1), n = (size_t)(n_in > 0 ? n_in : 1);
    SphereBatchWs o;
    o.mx = L.take<unsigned>(a);
    o.mean = L.take<float>(4 * a);
    o.sph = L.take<float>(3 * n);
    o.d2 = L.take<float>(n);
    o.row_of = L.take<int32_t>(n);
    L.pad(256);
    return o;
}

}  // namespace ml3d

using namespace ml3d;

extern "C" size_t ml3d_possibility_argmin_workspace_bytes(int64_t n_points, int64_t n_clouds) {
    if (n_points < 0 || n_clouds < 0) return 0;
    return ws_bytes_of(argmin_ws, n_points, n_clouds);
}

extern "C" int ml3d_possibility_argmin(const double* possibility, const int64_t* cloud_row_splits_host, int64_t n_clouds,
                                       const int32_t* active_host, int64_t n_active, int32_t* out_index, double* out_min,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    const int64_t m = pb_check(cloud_row_splits_host, n_clouds, active_host, n_active, 1);
    if (m < 0 || !possibility || !out_index || !out_min || !workspace) return ML3D_E_INVALID;
    ArgminWs W;
    if (!ws_carve(workspace, workspace_bytes, &W, argmin_ws, m, n_active)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& it, int count, int longest) {
        hipLaunchKernelGGL(pb_argmin_tiles, dim3((unsigned)((longest + PB_TILE - 1) / PB_TILE), (unsigned)count), dim3(256), 0, st,
                           possibility, it, W.part_v, W.part_i);
        hipLaunchKernelGGL(pb_argmin_final, dim3((unsigned)count), dim3(64), 0, st, W.part_v, W.part_i, it, out_index, out_min);
    });
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" size_t ml3d_patch_batch_workspace_bytes(int64_t n_points, int64_t n_active, int64_t k) {
    if (n_points < 0 || n_active < 0 || k < 0) return 0;
    return ws_bytes_of(patch_batch_ws, n_points, n_active, k);
}

extern "C" int ml3d_patch_batch(const float* points, double* possibility, const int64_t* cloud_row_splits_host, int64_t n_clouds,
                                const int32_t* active_host, int64_t n_active, const int32_t* center_index, const int32_t* perm,
                                int64_t k, int dims_mask, const float* extra, int n_extra, float feat_bias, float feat_scale,
                                float* out_pts, float* out_features, int32_t* out_sel, int32_t* out_row, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (k < 1 || n_extra < 0 || (n_extra > 0 && !extra) || (dims_mask & ~7)) return ML3D_E_INVALID;
    const int64_t m = pb_check(cloud_row_splits_host, n_clouds, active_host, n_active, k);
    if (m < 0 || n_active * k > 0x7ffffff0ll) return ML3D_E_INVALID;
    if (!points || !possibility || !center_index || !perm || !out_pts || !out_features || !out_sel || !out_row || !workspace)
        return ML3D_E_INVALID;
    PatchBatchWs W;
    if (!ws_carve(workspace, workspace_bytes, &W, patch_batch_ws, m, n_active, k)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    zero_async(W.mx, (size_t)((char*)W.d2 - (char*)W.mx), st);      // mx and mean (a fill kernel, not hipMemsetAsync: grid.h)
    const unsigned kblocks = (unsigned)((k + 255) / 256);
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& it, int count, int longest) {
        hipLaunchKernelGGL(pb_keys, dim3((unsigned)((longest + 255) / 256), (unsigned)count), dim3(256), 0, st, points, it, center_index,
                           W.keys, W.vals, W.item_of);
    });
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    // all points of the active clouds by distance to their own cloud's centre, then ONE stable pass by cloud: every cloud's
    // points end up contiguous (in the order of the active list) and ascending in (distance, index)
    if (sort_pairs_u64(W.keys, W.vals, m, 64, W.sort, st)) return ML3D_E_LAUNCH;
    const uint32_t* sorted = W.vals;
    if (n_active > 1) {
        int bits = 1;
        while ((1ll << bits) < n_active) ++bits;
        hipLaunchKernelGGL(pb_item_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, W.vals, W.item_of, m, W.keys);
        if (sort_pairs_u64(W.keys, W.vals, m, bits, W.sort, st, true)) return ML3D_E_LAUNCH;
        if (sort_result_in_alt(m, bits)) sorted = W.sort.vals_alt;
    }
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& it, int count, int) {
        hipLaunchKernelGGL(pb_gather, dim3(kblocks, (unsigned)count), dim3(256), 0, st, points, sorted, it, center_index, perm, k, out_pts,
                           out_sel, out_row, W.d2, W.mx);
    });
    hipLaunchKernelGGL(pb_bump, dim3(kblocks, (unsigned)n_active), dim3(256), 0, st, out_row, W.d2, W.mx, k, possibility);
    if (dims_mask) hipLaunchKernelGGL(pb_mean_seq, dim3((unsigned)n_active), dim3(256), 0, st, out_pts, k, W.mean);
    hipLaunchKernelGGL(pb_apply, dim3(kblocks, (unsigned)n_active), dim3(256), 0, st, out_pts, k, dims_mask, W.mean, out_row, extra, n_extra,
                       feat_bias, feat_scale, out_features);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" size_t ml3d_sphere_select_workspace_bytes(int64_t n_points, int64_t n_active) {
    if (n_points < 0 || n_active < 0) return 0;
    return ws_bytes_of(sphere_select_ws, n_points, n_active);
}

extern "C" int ml3d_sphere_select(const float* points, const int64_t* cloud_row_splits_host, int64_t n_clouds,
                                  const int32_t* active_host, int64_t n_active, const int32_t* center_index, float radius,
                                  int32_t* out_index, int64_t out_capacity, int32_t* out_count, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!(radius >= 0.f)) return ML3D_E_INVALID;
    const int64_t m = pb_check(cloud_row_splits_host, n_clouds, active_host, n_active, 1);
    if (m < 0 || !points || !center_index || !out_index || !out_count || !workspace || out_capacity < m) return ML3D_E_INVALID;
    SphereSelectWs W;
    if (!ws_carve(workspace, workspace_bytes, &W, sphere_select_ws, m, n_active)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    zero_async(W.cnt, ws_up(4 * (size_t)n_active), st);
    const float r2 = radius * radius;                                        // (ml3d_radius_fill's own bound)
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& it, int count, int longest) {
        hipLaunchKernelGGL(ss_keys, dim3((unsigned)((longest + 255) / 256), (unsigned)count), dim3(256), 0, st, points, it, center_index,
                           r2, W.keys, W.vals, W.cnt);
    });
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    int bits = 32;
    while ((1ll << (bits - 32)) < n_active) ++bits;
    if (sort_pairs_u64(W.keys, W.vals, m, bits, W.sort, st, true)) return ML3D_E_LAUNCH;
    const uint32_t* sorted = sort_result_in_alt(m, bits) ? W.sort.vals_alt : W.vals;
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& it, int count, int longest) {
        hipLaunchKernelGGL(ss_emit, dim3((unsigned)((longest + 255) / 256), (unsigned)count), dim3(256), 0, st, sorted, it, W.cnt, out_index,
                           out_count);
    });
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" size_t ml3d_sphere_batch_workspace_bytes(int64_t n_items, int64_t n_in) {
    if (n_items < 0 || n_in < 0) return 0;
    return ws_bytes_of(sphere_batch_ws, n_items, n_in);
}

extern "C" int ml3d_sphere_batch(const float* points, double* possibility, const int64_t* cloud_row_splits_host, int64_t n_clouds,
                                 const int32_t* active_host, int64_t n_active, const int32_t* center_index, const int32_t* cand,
                                 const int64_t* cand_offset_host, const int32_t* n_host, const int32_t* perm, const int32_t* keep,
                                 const int32_t* m_host, const int32_t* zero_extra_host, int dims_mask, float* extra, int n_extra,
                                 float feat_bias, float feat_scale, int linear, float* out_pts, float* out_columns, int32_t* out_sel,
                                 int32_t* out_row, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_extra < 0 || (n_extra > 0 && !extra) || (dims_mask & ~7) || !cand_offset_host || !n_host || !zero_extra_host ||
        (keep && !m_host))
        return ML3D_E_INVALID;
    if (pb_check(cloud_row_splits_host, n_clouds, active_host, n_active, 1) < 0) return ML3D_E_INVALID;
    if (!points || !possibility || !center_index || !cand || !perm || !out_pts || !out_columns || !out_sel || !out_row || !workspace)
        return ML3D_E_INVALID;
    int64_t n_in = 0, n_out = 0;
    for (int64_t a = 0; a < n_active; ++a) {
        const int64_t s = active_host[a], len = cloud_row_splits_host[s + 1] - cloud_row_splits_host[s];
        const int64_t n = n_host[a], m = keep && m_host[a] >= 0 ? m_host[a] : n;
        if (n < 1 || n > len || m < 1 || m > n || cand_offset_host[a] < 0 || cand_offset_host[a] + n > 0x7ffffff0ll) return ML3D_E_INVALID;
        n_in += n;
        n_out += m;
    }
    if (n_in > 0x7ffffff0ll) return ML3D_E_INVALID;
    SphereBatchWs W;
    if (!ws_carve(workspace, workspace_bytes, &W, sphere_batch_ws, n_active, n_in)) return ML3D_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    zero_async(W.mx, (size_t)((char*)W.sph - (char*)W.mx), st);      // mx and mean
    int64_t in0 = 0, keep0 = 0, out0 = 0;
    pb_chunks(cloud_row_splits_host, active_host, n_active, [&](const PbItems& cl, int count, int max_len) {
        const int64_t first = cl.first;
        SbItems it;
        int max_n = 0, max_m = 0;
        for (int a = 0; a < PB_ITEMS; ++a) {
            const bool live = a < count;
            const int64_t n = live ? n_host[first + a] : 0;
            const bool cut = live && keep && m_host[first + a] >= 0;
            const int64_t m = cut ? m_host[first + a] : n;
            it.start[a] = cl.start[a]; it.len[a] = cl.len[a]; it.center[a] = cl.slot[a];
            it.cand[a] = live ? (int)cand_offset_host[first + a] : 0;
            it.n[a] = (int)n; it.in0[a] = (int)in0; it.keep0[a] = cut ? (int)keep0 : -1; it.out0[a] = (int)out0; it.m[a] = (int)m;
            it.zero[a] = live && zero_extra_host[first + a] ? 1 : 0;
            in0 += n; out0 += m;
            if (cut) keep0 += m;
            if (n > max_n) max_n = (int)n;
            if (m > max_m) max_m = (int)m;
        }
        it.first = cl.first;
        const dim3 gn((unsigned)((max_n + 255) / 256), (unsigned)count), gm((unsigned)((max_m + 255) / 256), (unsigned)count);
        hipLaunchKernelGGL(sb_gather, gn, dim3(256), 0, st, points, it, center_index, cand, perm, W.sph, W.row_of, W.d2, W.mx);
        hipLaunchKernelGGL(sb_bump, gn, dim3(256), 0, st, it, W.row_of, W.d2, W.mx, possibility);
        if (dims_mask) hipLaunchKernelGGL(sb_mean_seq, dim3((unsigned)count), dim3(256), 0, st, W.sph, it, W.mean);
        if (linear && n_extra)
            hipLaunchKernelGGL(sb_rescale, dim3((unsigned)(((int64_t)max_len * n_extra + 255) / 256), (unsigned)count), dim3(256), 0, st,
                               extra, it, n_extra, feat_bias, feat_scale);
        hipLaunchKernelGGL(sb_emit, gm, dim3(256), 0, st, it, W.sph, W.row_of, W.mean, keep, dims_mask, extra, n_extra, out_pts, out_columns,
                           out_sel, out_row);
    });
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
