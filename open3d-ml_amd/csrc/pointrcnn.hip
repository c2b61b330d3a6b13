// pointrcnn.hip — PointRCNN stage 1 above the backbone (gfx950): bin-based box decoding and the zoned region proposals.
//
// ml3d_bin_decode restates decode_bbox_target (ml3d/torch/models/point_rcnn.py:1153-1272) with rotate_pc_along_y_torch
// (:1275-1295): per row the argmax over the x / z (/ y) / heading bins, the residual of the winning bin, the size residuals.
// Bandwidth-bound (C floats read, 7 written per row; C = 76 for the KITTI RPN): a group of 16 lanes owns a row, lane l reads
// the columns l, l + 16, ... of a segment, so the four rows of a wave are read as one run of consecutive addresses; the argmax
// of a segment is a 4-step xor-shuffle inside the group.  No atomics, no LDS.
//
// ml3d_rpn_proposals restates ProposalLayer.forward(post_process=True) + distance_based_proposal (:1020-1150) for the whole
// batch without a read-back: it is latency-bound (2 B small dependent problems), so the per-item Python loop becomes
//   rpn_keys      key = (item, ~ordered(score)), value = row                         -> ONE stable radix sort for the batch (sort.h)
//   rpn_zones     one workgroup per item walks its rows in score order: ranks inside the two distance zones by ballot /
//                 popcount, the first int(0.7 nms_pre) near and nms_pre - int(0.7 nms_pre) far rows (or the near zone's
//                 next rows when the far zone is empty) -> per zone the BEV boxes of xywhr_to_xyxyr, PADDED to the zone's
//                 fixed capacity with boxes that overlap nothing, so that the host knows every NMS problem's size
//   ml3d_nms      the existing rotated-BEV NMS, once per (item, zone), on scores that restate the walk order
//   rpn_collect   one workgroup per item: the first int(0.7 nms_post) near and nms_post - int(0.7 nms_post) far survivors,
//                 near rows first; y += h / 2; zero / -1 padding.
//
// ml3d_roi_pool produces the rows RCNN.forward reads as pts_input (:848-887) in one launch: the open3d wheel's roi_pool on the
// enlarged boxes, the two extra per-point columns and the canonical transform, without the [B, N, 2 + C] concat.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "grid.h"
#include "ml3d_hip.h"
#include "sort.h"

namespace ml3d {

// ---- bin decode ----------------------------------------------------------------------------------------------------------------------
constexpr int DEC_LANES = 16;                    // lanes per row
constexpr int DEC_ROWS = 256 / DEC_LANES;        // rows per workgroup

struct DecodeArgs {
    float anchor[3];
    float loc_scope, loc_bin_size, loc_y_scope, loc_y_bin_size;
    int per_loc_bin_num, loc_y_bin_num, num_head_bin;
    int xz_fine, y_by_bin, ry_fine;
};

// argmax of row[lo .. lo + len) over the 16 lanes of a group, ties to the lowest column (torch.argmax); every lane of the
// WAVE takes part in the shuffles
__device__ __forceinline__ int group_argmax(const float* __restrict__ row, int lo, int len, int gl) {
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int c = gl; c < len; c += DEC_LANES) {
        const float v = row[lo + c];
        if (v > best || at == 0x7fffffff) { best = v; at = c; }
    }
#pragma unroll
    for (int o = DEC_LANES / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, DEC_LANES);
        const int oa = __shfl_xor(at, o, DEC_LANES);
        if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
    }
    return at == 0x7fffffff ? 0 : at;
}

__global__ void __launch_bounds__(256)
bin_decode_rows(const float* __restrict__ roi, int roi_width, const float* __restrict__ reg, int64_t ld, int64_t n, DecodeArgs A,
                float* __restrict__ out) {
    const int gl = threadIdx.x & (DEC_LANES - 1);
    const int64_t r = (int64_t)blockIdx.x * DEC_ROWS + (threadIdx.x / DEC_LANES);
    const bool live = r < n;
    const float* row = reg + (live ? r : n - 1) * ld;          // (a row past the end reads the last one and writes nothing)
    const int L = A.per_loc_bin_num;
    const int x_bin = group_argmax(row, 0, L, gl);
    const int z_bin = group_argmax(row, L, L, gl);
    int off = A.xz_fine ? 4 * L : 2 * L;
    int y_bin = 0;
    const int y_at = off;
    if (A.y_by_bin) {
        y_bin = group_argmax(row, off, A.loc_y_bin_num, gl);
        off += 2 * A.loc_y_bin_num;
    } else {
        off += 1;
    }
    const int H = A.num_head_bin;
    const int ry_bin = group_argmax(row, off, H, gl);
    if (!live || gl != 0) return;
    const float half_bin = (float)((double)A.loc_bin_size / 2.0);
    float px = __fsub_rn(__fadd_rn(__fmul_rn((float)x_bin, A.loc_bin_size), half_bin), A.loc_scope);
    float pz = __fsub_rn(__fadd_rn(__fmul_rn((float)z_bin, A.loc_bin_size), half_bin), A.loc_scope);
    if (A.xz_fine) {
        px = __fadd_rn(px, __fmul_rn(row[2 * L + x_bin], A.loc_bin_size));
        pz = __fadd_rn(pz, __fmul_rn(row[3 * L + z_bin], A.loc_bin_size));
    }
    const float* q = roi + r * roi_width;
    float py;
    if (A.y_by_bin) {
        const float half_y = (float)((double)A.loc_y_bin_size / 2.0);
        const float y_res = __fmul_rn(row[y_at + A.loc_y_bin_num + y_bin], A.loc_y_bin_size);
        py = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn((float)y_bin, A.loc_y_bin_size), half_y), A.loc_y_scope), y_res);
        py = __fadd_rn(py, q[1]);
    } else {
        py = __fadd_rn(q[1], row[y_at]);
    }
    const float ry_norm = row[off + H + ry_bin];
    const double PI = 3.14159265358979323846;
    float ry;
    if (A.ry_fine) {
        const double apc = (PI / 2.0) / (double)H;
        const float res = __fmul_rn(ry_norm, (float)(apc / 2.0));
        ry = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn((float)ry_bin, (float)apc), (float)(apc / 2.0)), res), (float)(PI / 4.0));
    } else {
        const double apc = (2.0 * PI) / (double)H;
        const float res = __fmul_rn(ry_norm, (float)(apc / 2.0));
        const float two_pi = (float)(2.0 * PI);
        // torch's remainder: fmod, moved into the divisor's sign
        float m = fmodf(__fadd_rn(__fmul_rn((float)ry_bin, (float)apc), res), two_pi);
        if (m != 0.f && m < 0.f) m = __fadd_rn(m, two_pi);
        ry = m > (float)PI ? __fsub_rn(m, two_pi) : m;
    }
    const float* sz = row + off + 2 * H;
    float o[7];
    o[0] = px; o[1] = py; o[2] = pz;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3 + k] = __fadd_rn(__fmul_rn(sz[k], A.anchor[k]), A.anchor[k]);
    o[6] = ry;
    if (roi_width == 7) {
        const float ang = -q[6];
        const float ca = cosf(ang), sa = sinf(ang);
        const float x2 = __fsub_rn(__fmul_rn(px, ca), __fmul_rn(pz, sa));
        const float z2 = __fadd_rn(__fmul_rn(px, sa), __fmul_rn(pz, ca));
        o[0] = x2; o[2] = z2;
        o[6] = __fadd_rn(ry, q[6]);
    }
    o[0] = __fadd_rn(o[0], q[0]);
    o[2] = __fadd_rn(o[2], q[2]);
#pragma unroll
    for (int k = 0; k < 7; ++k) out[7 * r + k] = o[k];
}

// ---- proposals -------------------------------------------------------------------------------------------------------------------------
// ascending key = item, then descending score; the sort is stable and the rows arrive in ascending index, so equal scores
// keep the lower index first  (-0.0 and +0.0 are one score)
__global__ void __launch_bounds__(256)
rpn_keys(const float* __restrict__ scores, int64_t n, int64_t total, u64* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float sc = scores[i];
    keys[i] = ((u64)(i / n) << 32) | (u64)(uint32_t)(~f2ord(sc == 0.f ? 0.f : sc));
    vals[i] = (uint32_t)i;
}

constexpr float RPN_PAD = 3.0e18f;               // a zero-size box out there overlaps nothing (and nothing overlaps it)

// One workgroup per item.  cand [B, nms_pre]: on return slot s < pre_near holds the near zone's s-th row (item-local), slot
// pre_near + j the far zone's j-th candidate, -1 beyond a zone's count; counts [B, 2] the two counts; bev / nscore the padded NMS
// inputs of both zones, laid out like cand.  far [B, nms_pre] is scratch for the far zone's own rows.
__global__ void __launch_bounds__(256)
rpn_zones(const float* __restrict__ boxes, const uint32_t* __restrict__ order, int64_t n, int nms_pre, int pre_near,
          int32_t* __restrict__ cand, int32_t* __restrict__ far, int32_t* __restrict__ counts, float* __restrict__ bev,
          float* __restrict__ nscore) {
    __shared__ int wsum[2][4];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int pre_far = nms_pre - pre_near;
    const uint32_t* ord = order + b * n;
    const float* bx = boxes + b * n * 7;
    int32_t* near_list = cand + b * nms_pre;
    int32_t* far_list = far + b * nms_pre;
    int nn = 0, nf = 0;                                       // rows of either zone seen so far (uniform)
    for (int64_t p0 = 0; p0 < n; p0 += 256) {
        if (nn >= nms_pre && nf >= pre_far) break;
        const int64_t p = p0 + t;
        const bool in = p < n;
        const int src = in ? (int)((int64_t)ord[p] - b * n) : 0;
        const float z = in ? bx[(int64_t)src * 7 + 2] : 0.f;
        const bool is_near = in && z > 0.f && z <= 40.f;
        const bool is_far = in && z > 40.f && z <= 80.f;
        const u64 mn = __ballot(is_near), mf = __ballot(is_far);
        if (lane == 0) { wsum[0][wv] = __popcll(mn); wsum[1][wv] = __popcll(mf); }
        __syncthreads();
        int rn = nn, rf = nf;
        for (int w = 0; w < wv; ++w) { rn += wsum[0][w]; rf += wsum[1][w]; }
        const u64 below = (1ull << lane) - 1ull;
        rn += __popcll(mn & below);
        rf += __popcll(mf & below);
        if (is_near && rn < nms_pre) near_list[rn] = src;
        if (is_far && rf < pre_far) far_list[rf] = src;
        nn += wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        nf += wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
        __syncthreads();
    }
    // the far zone's candidates: its own rows, or -- without any -- the near zone's rows behind the first pre_near
    const int near_all = nn < nms_pre ? nn : nms_pre;
    const int cnt0 = nn < pre_near ? nn : pre_near;
    const int cnt1 = nf > 0 ? (nf < pre_far ? nf : pre_far) : (near_all > pre_near ? near_all - pre_near : 0);
    if (t == 0) { counts[2 * b] = cnt0; counts[2 * b + 1] = cnt1; }
    for (int s = t; s < nms_pre; s += 256) {
        const bool second = s >= pre_near;
        const int j = second ? s - pre_near : s;
        const bool valid = j < (second ? cnt1 : cnt0);
        int src = -1;
        if (valid) src = (second && nf > 0) ? far_list[j] : near_list[s];
        near_list[s] = src;
        float* o = bev + (b * nms_pre + s) * 5;
        if (valid) {
            // xywhr_to_xyxyr(proposals[:, [0, 2, 3, 5, 6]]): (x, z, h, l, ry)
            const float* q = bx + (int64_t)src * 7;
            const float hw = __fdiv_rn(q[3], 2.0f), hh = __fdiv_rn(q[5], 2.0f);
            o[0] = __fsub_rn(q[0], hw); o[1] = __fsub_rn(q[2], hh); o[2] = __fadd_rn(q[0], hw); o[3] = __fadd_rn(q[2], hh); o[4] = q[6];
        } else {
            o[0] = RPN_PAD; o[1] = RPN_PAD; o[2] = RPN_PAD; o[3] = RPN_PAD; o[4] = 0.f;
        }
        nscore[b * nms_pre + s] = -(float)j;                  // descending with the slot: the NMS walks the zone in score order
    }
}

// keep [B, nms_pre] (zone slices like cand) / kept [B, 2] as ml3d_nms wrote them.  The padding slots sort behind every real
// candidate, so the real survivors are a prefix of a zone's keep list.
__global__ void __launch_bounds__(256)
rpn_collect(const float* __restrict__ scores, const float* __restrict__ boxes, int64_t n, int nms_pre, int pre_near, int n_near,
            int n_far, int nms_post, int post_near, const int32_t* __restrict__ cand, const int32_t* __restrict__ counts,
            const int64_t* __restrict__ keep, const int64_t* __restrict__ kept, float* __restrict__ rois,
            float* __restrict__ roi_scores, int32_t* __restrict__ roi_index) {
    __shared__ int rows[2];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    if (t < 2) rows[t] = 0;
    __syncthreads();
    const int post[2] = {post_near, nms_post - post_near};
    const int off[2] = {0, pre_near};
    const int cap[2] = {n_near, n_far};
    for (int zone = 0; zone < 2; ++zone) {
        if (cap[zone] == 0) continue;
        const int64_t k = kept[2 * b + zone];
        const int lim = (int)(k < post[zone] ? k : post[zone]);
        const int cnt = counts[2 * b + zone];
        const int64_t* kp = keep + b * nms_pre + off[zone];
        int mine = 0;
        for (int s = t; s < lim; s += 256) mine += kp[s] < cnt ? 1 : 0;
        if (mine) atomicAdd(&rows[zone], mine);
    }
    __syncthreads();
    const int r0 = rows[0], r1 = rows[1];
    for (int s = t; s < nms_post; s += 256) {
        float* o = rois + (b * nms_post + s) * 7;
        if (s < r0 + r1) {
            const int zone = s < r0 ? 0 : 1;
            const int slot = off[zone] + (int)keep[b * nms_pre + off[zone] + (s - (zone ? r0 : 0))];
            const int src = cand[b * nms_pre + slot];
            const float* q = boxes + (b * n + src) * 7;
            o[0] = q[0];
            o[1] = __fadd_rn(q[1], __fdiv_rn(q[3], 2.0f));    // y: the centre of the bottom face
#pragma unroll
            for (int c = 2; c < 7; ++c) o[c] = q[c];
            roi_scores[b * nms_post + s] = scores[b * n + src];
            roi_index[b * nms_post + s] = src;
        } else {
#pragma unroll
            for (int c = 0; c < 7; ++c) o[c] = 0.f;
            roi_scores[b * nms_post + s] = 0.f;
            roi_index[b * nms_post + s] = -1;
        }
    }
}

// ---- RoI pooling (stage 2's input) ----------------------------------------------------------------------------------------------------
// One workgroup per (item, roi), the box in uniform registers.  Phase 1 walks the item's points 256 at a time: a point's slot is
// the running count + the hits of the waves before + the hits of the lanes below (ballot / popcount, as rpn_zones ranks its zones),
// so the list comes out in ascending point index without an atomic; the walk ends once S hits are known.  The list lives in the
// output pool_idx itself.  Phase 2: a wave per output row; slot k reads the hit k % cnt (the wheel's wrap), every lane forms the
// five leading columns (uniform work), lanes copy the feature row with consecutive addresses on both sides.
struct RoiPoolArgs {
    int64_t n, m, ld_feat;
    int c, s;
    float score_thres, extra_width;
};

__global__ void __launch_bounds__(256)
roi_pool_rows(const float* __restrict__ xyz, const float* __restrict__ feat, const float* __restrict__ scores,
              const float* __restrict__ rois, RoiPoolArgs A, float* __restrict__ out, int32_t* pool_idx, int32_t* __restrict__ empty) {
    __shared__ int wsum[4];
    const int64_t r = blockIdx.x;                             // b * m + roi
    const int64_t b = r / A.m;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* q = rois + r * 7;
    const float x = q[0], y = q[1], z = q[2], ry = q[6];
    // enlarge_box3d: one float32 add each
    const float wide = 2.0f * A.extra_width;
    const float h = q[3] + wide, w = q[4] + wide, l = q[5] + wide, ye = y + A.extra_width;
    const float hh = h / 2.0f, hw = w / 2.0f, hl = l / 2.0f;
    const float cy = ye - hh;
    const float ca = cosf(ry), sa = sinf(ry);
    const float* pts = xyz + b * A.n * 3;
    int32_t* list = pool_idx + r * A.s;
    int cnt = 0;                                              // hits so far (uniform)
    for (int64_t p0 = 0; p0 < A.n && cnt < A.s; p0 += 256) {
        const int64_t p = p0 + t;
        bool in = false;
        if (p < A.n) {
            const float dx = pts[3 * p] - x, dy = pts[3 * p + 1] - cy, dz = pts[3 * p + 2] - z;
            if (!(fabsf(dx) > 10.0f || fabsf(dy) > hh || fabsf(dz) > 10.0f)) {
                const float xr = dx * ca + dz * (-sa);
                const float zr = dx * sa + dz * ca;
                in = xr >= -hl && xr <= hl && zr >= -hw && zr <= hw;
            }
        }
        const u64 mask = __ballot(in);
        if (lane == 0) wsum[wv] = __popcll(mask);
        __syncthreads();
        int rank = cnt;
        for (int k = 0; k < wv; ++k) rank += wsum[k];
        rank += __popcll(mask & ((1ull << lane) - 1ull));
        if (in && rank < A.s) list[rank] = (int32_t)p;
        cnt += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();                                      // (also: the list entries are visible to the whole workgroup)
    }
    if (cnt > A.s) cnt = A.s;
    if (t == 0) empty[r] = cnt == 0 ? 1 : 0;
    const int width = 5 + A.c;
    for (int k = wv; k < A.s; k += 4) {
        float* o = out + (r * A.s + k) * width;
        float px = 0.f, py = 0.f, pz = 0.f, seg = 0.f, depth = 0.f;
        int64_t src = -1;
        if (cnt > 0) {
            src = list[k % cnt];                              // slots below cnt are never written in this phase
            px = pts[3 * src]; py = pts[3 * src + 1]; pz = pts[3 * src + 2];
            const float sc = scores[b * A.n + src];
            seg = 1.0f / (1.0f + expf(-sc)) > A.score_thres ? 1.0f : 0.f;
            depth = sqrtf((px * px + py * py) + pz * pz) / 70.0f - 0.5f;
        }
        if (lane == 0 && k >= cnt) list[k] = (int32_t)src;
        // the canonical transform, on the roi as given (not the enlarged box)
        const float dx = px - x, dy = py - y, dz = pz - z;
        const float xc = dx * ca - dz * sa, zc = dx * sa + dz * ca;
        const float lead = lane == 0 ? xc : lane == 1 ? dy : lane == 2 ? zc : lane == 3 ? seg : depth;
        const float* f = feat + (b * A.n + (src < 0 ? 0 : src)) * A.ld_feat;
        for (int c = lane; c < width; c += 64) o[c] = c < 5 ? lead : (src < 0 ? 0.f : f[c - 5]);
    }
}

}  // namespace ml3d

using namespace ml3d;

static int bins_of(float scope, float bin_size) { return (int)((double)scope / (double)bin_size) * 2; }

extern "C" int ml3d_bin_decode(const float* roi, int roi_width, const float* pred_reg, int64_t ld_reg, int channels, int64_t n,
                               const float* anchor_size_host, float loc_scope, float loc_bin_size, int num_head_bin,
                               float loc_y_scope, float loc_y_bin_size, int get_xz_fine, int get_y_by_bin, int get_ry_fine,
                               float* out_boxes, void* stream) {
    if (n < 0 || (roi_width != 3 && roi_width != 7) || !anchor_size_host || num_head_bin < 1 || !(loc_bin_size > 0.f) ||
        !(loc_scope > 0.f) || channels < 1 || ld_reg < channels)
        return ML3D_E_INVALID;
    DecodeArgs A;
    for (int k = 0; k < 3; ++k) A.anchor[k] = anchor_size_host[k];
    A.loc_scope = loc_scope; A.loc_bin_size = loc_bin_size; A.loc_y_scope = loc_y_scope; A.loc_y_bin_size = loc_y_bin_size;
    A.per_loc_bin_num = bins_of(loc_scope, loc_bin_size);
    A.loc_y_bin_num = 0;
    if (get_y_by_bin) {
        if (!(loc_y_bin_size > 0.f) || !(loc_y_scope > 0.f)) return ML3D_E_INVALID;
        A.loc_y_bin_num = bins_of(loc_y_scope, loc_y_bin_size);
        if (A.loc_y_bin_num < 1) return ML3D_E_INVALID;
    }
    A.num_head_bin = num_head_bin;
    A.xz_fine = get_xz_fine ? 1 : 0; A.y_by_bin = get_y_by_bin ? 1 : 0; A.ry_fine = get_ry_fine ? 1 : 0;
    if (A.per_loc_bin_num < 1) return ML3D_E_INVALID;
    const int64_t want = (int64_t)A.per_loc_bin_num * (get_xz_fine ? 4 : 2) + (get_y_by_bin ? 2 * (int64_t)A.loc_y_bin_num : 1) +
                         2 * (int64_t)num_head_bin + 3;
    if (want != channels) return ML3D_E_INVALID;
    if (n == 0) return 0;
    if (!roi || !pred_reg || !out_boxes) return ML3D_E_INVALID;
    const int64_t blocks = (n + DEC_ROWS - 1) / DEC_ROWS;
    if (blocks > 0x7fffffffll) return ML3D_E_UNSUPPORTED;
    hipLaunchKernelGGL(bin_decode_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, roi, roi_width, pred_reg, ld_reg, n,
                       A, out_boxes);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_rpn_proposals(const float* scores, const float* boxes, int64_t batch, int64_t n, int64_t nms_pre,
                                  int64_t nms_post, float nms_thres, float* out_rois, float* out_roi_scores,
                                  int32_t* out_roi_index, uint64_t* sort_keys, uint32_t* sort_vals, int32_t* sort_hist,
                                  int32_t* lists, float* nms_boxes, int64_t* nms_keep, void* nms_workspace,
                                  size_t nms_workspace_bytes, void* stream) {
    if (batch < 0 || n < 0 || nms_pre < 0 || nms_post < 0) return ML3D_E_INVALID;
    if (nms_pre > 65536 || nms_post > 0x7fffffffll / 8 || batch > 65536 || batch * n > 0x7fffffffll) return ML3D_E_UNSUPPORTED;
    if (batch == 0 || nms_post == 0) return 0;
    if (!out_rois || !out_roi_scores || !out_roi_index) return ML3D_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int pre = (int)nms_pre, pre_near = (int)((double)nms_pre * 0.7), post_near = (int)((double)nms_post * 0.7);
    // a zone never holds more candidates than the item has points: the NMS problems are sized by that
    const int n_near = (int)(pre_near < n ? pre_near : n), n_far = (int)(pre - pre_near < n ? pre - pre_near : n);
    int32_t* cand = lists;
    int32_t* far = lists + batch * pre;
    int32_t* counts = lists + 2 * batch * pre;
    float* bev = nms_boxes;
    float* nscore = nms_boxes + 5 * batch * pre;
    int64_t* kept = nms_keep + batch * pre;
    if (n > 0 && pre > 0) {
        if (!scores || !boxes || !sort_keys || !sort_vals || !sort_hist || !lists || !nms_boxes || !nms_keep) return ML3D_E_INVALID;
        const int64_t total = batch * n;
        int key_bits = 32;
        while (key_bits < 48 && ((int64_t)1 << (key_bits - 32)) < batch) ++key_bits;
        hipLaunchKernelGGL(rpn_keys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, scores, n, total, (u64*)sort_keys, sort_vals);
        if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
        SortWs S;
        const int64_t nb = (total + 1023) / 1024;
        S.keys_alt = (u64*)sort_keys + total;
        S.vals_alt = sort_vals + total;
        S.hist = sort_hist;
        S.block_sums = sort_hist + 1 + 256 * nb;
        S.n = total;
        if (sort_pairs_u64((u64*)sort_keys, sort_vals, total, key_bits, S, st, true)) return ML3D_E_LAUNCH;
        const uint32_t* order = sort_result_in_alt(total, key_bits) ? S.vals_alt : sort_vals;
        hipLaunchKernelGGL(rpn_zones, dim3((unsigned)batch), dim3(256), 0, st, boxes, order, n, pre, pre_near, cand, far, counts, bev, nscore);
        if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
        for (int64_t b = 0; b < batch; ++b) {
            for (int zone = 0; zone < 2; ++zone) {
                const int64_t at = b * pre + (zone ? pre_near : 0);
                const int64_t m = zone ? n_far : n_near;
                if (m == 0) continue;
                const int rc = ml3d_nms(bev + 5 * at, nscore + at, m, nms_thres, nms_keep + at, kept + 2 * b + zone, nms_workspace,
                                        nms_workspace_bytes, stream);
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL(rpn_collect, dim3((unsigned)batch), dim3(256), 0, st, scores, boxes, n, pre, pre_near, n_near, n_far,
                           (int)nms_post, post_near, cand, counts, nms_keep, kept, out_rois, out_roi_scores, out_roi_index);
    } else {
        // no point or no candidate slot: every row is padding
        hipLaunchKernelGGL(rpn_collect, dim3((unsigned)batch), dim3(256), 0, st, scores, boxes, n, pre, pre_near, 0, 0, (int)nms_post,
                           post_near, cand, counts, nms_keep, kept, out_rois, out_roi_scores, out_roi_index);
    }
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_roi_pool(const float* xyz, const float* feat, int64_t ld_feat, int channels, const float* scores,
                             const float* rois, int64_t batch, int64_t n, int64_t m, int num_points, float score_thres,
                             float extra_width, float* out_pts_input, int32_t* out_pool_idx, int32_t* out_empty, void* stream) {
    if (batch < 0 || n < 0 || m < 0 || channels < 0 || num_points < 1 || ld_feat < channels) return ML3D_E_INVALID;
    if (batch * n > 0x7fffffffll || batch * m > 0x7fffffffll || batch * m * (int64_t)num_points > 0x7fffffffll) return ML3D_E_UNSUPPORTED;
    if (batch == 0 || m == 0) return 0;
    if (!rois || !out_pts_input || !out_pool_idx || !out_empty || (n > 0 && (!xyz || !scores || (channels > 0 && !feat))))
        return ML3D_E_INVALID;
    RoiPoolArgs A;
    A.n = n; A.m = m; A.ld_feat = ld_feat; A.c = channels; A.s = num_points; A.score_thres = score_thres; A.extra_width = extra_width;
    hipLaunchKernelGGL(roi_pool_rows, dim3((unsigned)(batch * m)), dim3(256), 0, (hipStream_t)stream, xyz, feat, scores, rois, A,
                       out_pts_input, out_pool_idx, out_empty);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
