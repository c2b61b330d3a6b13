// PointTransformer inference (ml3d/torch/models/point_transformer.py of the reference): furthest point sampling, the fused
// vector self-attention layer and the two transition kernels.  Contracts: include/ml3d_hip.h.  gfx950 only; the same source
// builds under tests/hipemu.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ml3d_hip.h"
#include "workspace.h"

typedef float pt_f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// (a) furthest point sampling: ONE workgroup per batch item.  Thread t owns points t, t + T, t + 2T, ... of the item and keeps
// their running minimum distances in registers (PER of them; PER == 0: any item length, the minima live in the workspace).
// Per pick: every thread updates its minima against the picked point and proposes its best (distance bits, inverted index)
// key -- d2 >= 0, so the float bits order like the values, and the inverted index makes the LOWEST index win a tie --, the
// wave reduces with shuffles, the 16 waves meet in LDS once (two alternating slots: one barrier per pick).  The first JL
// points of every thread (JL * 1024 of the item) are read from LDS, the rest from L2.  The sweep is branch-free so that the
// loads of several points are in flight at once (a branch per point makes every point wait for its own L2 round trip):
// slots past the item's end start at -2 and can never beat a real minimum (>= 0), their loads are clamped to the last point.
// ---------------------------------------------------------------------------------------------------------------------------
#define FPS_T 1024
#define FPS_WAVES (FPS_T / 64)
#define FPS_LDS_J 12           // 12 288 points = 144 KB of coordinates (x[], y[], z[])
#define FPS_CHUNK 8            // points whose loads are issued together

__device__ __forceinline__ float fps_d2(float x, float y, float z, float px, float py, float pz) {
    const float dx = __fsub_rn(x, px), dy = __fsub_rn(y, py), dz = __fsub_rn(z, pz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

template <int PER, int JL>
__global__ __launch_bounds__(FPS_T) void fps_kernel(const float* __restrict__ pts, const int64_t* __restrict__ rs,
                                                    const int64_t* __restrict__ nrs, int32_t* __restrict__ out,
                                                    float* __restrict__ mind_g) {
    HIP_DYNAMIC_SHARED(float, sm)
    __shared__ unsigned long long s_key[2][FPS_WAVES];
    constexpr int CAP = JL * FPS_T;
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int64_t base = rs[b], obase = nrs[b];
    const int n = (int)(rs[b + 1] - base), m = (int)(nrs[b + 1] - obase);
    if (m <= 0 || n <= 0) return;      // (uniform for the workgroup)
    const float* P = pts + 3 * base;
    const int nl = n < CAP ? n : CAP;
    float* sx = sm;
    float* sy = sm + CAP;
    float* sz = sm + 2 * CAP;
    for (int i = t; i < CAP; i += FPS_T) {
        const int ic = i < nl ? i : nl - 1;
        sx[i] = P[3 * ic];
        sy[i] = P[3 * ic + 1];
        sz[i] = P[3 * ic + 2];
    }
    constexpr int NREG = PER > 0 ? PER : 1;
    float mind[NREG];
    const float inf = __uint_as_float(0x7f800000u);
    if constexpr (PER > 0) {
#pragma unroll
        for (int j = 0; j < PER; ++j) mind[j] = t + j * FPS_T < n ? inf : -2.f;
    } else {
        mind[0] = 0.f;
        for (int i = t; i < n; i += FPS_T) mind_g[base + i] = inf;      // (each thread re-reads only what it wrote)
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < m; ++s) {
        if (t == 0) out[obase + s] = (int32_t)(base + cur);
        if (s == m - 1) break;
        float px, py, pz;
        if (cur < nl) { px = sx[cur]; py = sy[cur]; pz = sz[cur]; }
        else { px = P[3 * cur]; py = P[3 * cur + 1]; pz = P[3 * cur + 2]; }
        float bd = -1.f;
        int bi = 0;
        // the minima take PER of the 128 registers a 16-wave workgroup leaves each lane; the point addresses must not join
        // them: an opaque copy of the thread index per pick keeps the PER address computations inside the pick loop
        int tt = t;
#ifndef ML3D_HIPEMU
        asm volatile("" : "+v"(tt));
#endif
        if constexpr (PER > 0) {
#pragma unroll
            for (int j0 = 0; j0 < PER; j0 += FPS_CHUNK) {
                float x[FPS_CHUNK], y[FPS_CHUNK], z[FPS_CHUNK];
#pragma unroll
                for (int u = 0; u < FPS_CHUNK; ++u) {
                    const int j = j0 + u;
                    if (j < PER) {
                        const int i = tt + j * FPS_T;
                        if (j < JL) { x[u] = sx[i]; y[u] = sy[i]; z[u] = sz[i]; }
                        else {
                            const int ic = i < n ? i : n - 1;
                            x[u] = P[3 * ic]; y[u] = P[3 * ic + 1]; z[u] = P[3 * ic + 2];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < FPS_CHUNK; ++u) {
                    const int j = j0 + u;
                    if (j < PER) {
                        const float mm = fminf(mind[j], fps_d2(x[u], y[u], z[u], px, py, pz));
                        mind[j] = mm;
                        if (mm > bd) { bd = mm; bi = tt + j * FPS_T; }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // (one chunk's loads at a time: registers)
            }
        } else {
            for (int i = t; i < n; i += FPS_T) {
                float x, y, z;
                if (i < nl) { x = sx[i]; y = sy[i]; z = sz[i]; }
                else { x = P[3 * i]; y = P[3 * i + 1]; z = P[3 * i + 2]; }
                const float mm = fminf(mind_g[base + i], fps_d2(x, y, z, px, py, pz));
                mind_g[base + i] = mm;
                if (mm > bd) { bd = mm; bi = i; }
            }
        }
        unsigned long long key = bd < 0.f ? 0ull : (((unsigned long long)__float_as_uint(bd) << 32) | (0xffffffffu - (unsigned)bi));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off, 64);
            key = o > key ? o : key;
        }
        if ((t & 63) == 0) s_key[s & 1][t >> 6] = key;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < FPS_WAVES; ++w) {
            const unsigned long long o = s_key[s & 1][w];
            key = o > key ? o : key;
        }
        cur = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    }
}

extern "C" size_t ml3d_fps_workspace_bytes(int64_t n_points, int64_t batch) {
    if (n_points < 0 || batch < 0) return 0;
    return (size_t)n_points * 4 + 256;
}

template <int PER, int JL>
static int fps_launch(const float* points, const int64_t* rs, const int64_t* nrs, int64_t batch, int32_t* out, float* mind,
                      hipStream_t st) {
    const size_t smb = (size_t)JL * FPS_T * 12;
    auto kern = fps_kernel<PER, JL>;
    if (smb > 48 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smb) != hipSuccess)
        return ML3D_E_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(FPS_T), smb, st, points, rs, nrs, out, mind);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

extern "C" int ml3d_furthest_point_sampling(const float* points, const int64_t* row_splits, const int64_t* new_row_splits,
                                            const int64_t* row_splits_host, const int64_t* new_row_splits_host,
                                            int64_t batch, int64_t n_points, int32_t* out_index, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (batch < 0 || batch > 65535 || n_points < 0 || !row_splits_host || !new_row_splits_host) return ML3D_E_INVALID;
    if (row_splits_host[0] != 0 || new_row_splits_host[0] != 0 || row_splits_host[batch] != n_points) return ML3D_E_INVALID;
    int64_t longest = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = row_splits_host[b + 1] - row_splits_host[b], m = new_row_splits_host[b + 1] - new_row_splits_host[b];
        if (n < 0 || m < 0 || m > n || n > 0x7fffffff / 4) return ML3D_E_INVALID;
        if (m > 0 && n > longest) longest = n;
    }
    if (batch == 0 || new_row_splits_host[batch] == 0) return 0;
    if (!points || !row_splits || !new_row_splits || !out_index) return ML3D_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
#define FPS_CLASS(PER_, JL_) \
    if (longest <= PER_ * FPS_T) return fps_launch<PER_, JL_>(points, row_splits, new_row_splits, batch, out_index, nullptr, st);
    FPS_CLASS(4, 4)
    FPS_CLASS(12, 12)
    FPS_CLASS(24, 12)
    FPS_CLASS(48, 12)
    FPS_CLASS(64, 12)
#undef FPS_CLASS
    if (!workspace || workspace_bytes < ml3d_fps_workspace_bytes(n_points, batch)) return ML3D_E_WORKSPACE;
    float* mind = (float*)ml3d::ws_align(workspace);
    return fps_launch<0, FPS_LDS_J>(points, row_splits, new_row_splits, batch, out_index, mind, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
// (b) vector self-attention.  One wave works on 16 (query, neighbour) ROWS at a time: one query with 16 neighbours or two with
// 8.  Lane l = (row l % 16, quarter l / 16) builds the input of linear_w for its row and 4 of every 16 channels in registers
// and feeds it to v_mfma_f32_16x16x4_f32 as the A operand (the contraction index of the instruction is the quarter; four
// instructions walk the lane's 4 channels); B = the folded c -> c/8 weights, rows padded to 16 NT.  The small c/8 -> c/8
// Linear, the softmax over the neighbours and the grouped weighted sum go through 8 KB of LDS; nothing [n, nsample, c]
// leaves the CU.
// ---------------------------------------------------------------------------------------------------------------------------
struct PtAttnParams {
    const float *pw1, *pb1;      // linear_p[0] + BN folded: [3][3] (out, in), [3]
    const float *pw2t, *pb2;     // linear_p[3]: transposed [3][c], [c]
    const float *s0, *t0;        // linear_w[0] (BN) as scale / shift [c]
    const float *w1, *b1;        // linear_w[2] + BN folded: [16 NT][c] (rows >= c/8 zero), [16 NT]
    const float *w2, *b2;        // linear_w[5]: [c/8][c/8] (out, in), [c/8]
    const float *es, *et;        // epilogue scale / shift [c] + ReLU, or NULL
};

template <int NS, int NT>
__global__ __launch_bounds__(64) void pt_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ pts,
                                                     const int32_t* __restrict__ idx, int64_t n, int C, PtAttnParams p,
                                                     float* __restrict__ out, int64_t groups) {
    constexpr int QW = 16 / NS;
    constexpr int CSP = 16 * NT;
    __shared__ float s_hid[16][CSP + 1];
    __shared__ float s_w[16][CSP + 1];
    __shared__ float s_h[16][4];
    __shared__ int s_nb[16];
    const int lane = (int)threadIdx.x, row = lane & 15, kq = lane >> 4;
    const int cs = C >> 3;
    float W1[9], B1[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) W1[i] = p.pw1[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) B1[i] = p.pb1[i];
    const int64_t ld = 3 * (int64_t)C;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        int64_t q = g * QW + row / NS;
        if (q >= n) q = n - 1;
        int64_t nb = idx[q * NS + row % NS];
        nb = nb < 0 ? 0 : (nb >= n ? n - 1 : nb);
        const float dx = pts[3 * nb] - pts[3 * q], dy = pts[3 * nb + 1] - pts[3 * q + 1], dz = pts[3 * nb + 2] - pts[3 * q + 2];
        const float h0 = fmaxf(((W1[0] * dx + W1[1] * dy) + W1[2] * dz) + B1[0], 0.f);
        const float h1 = fmaxf(((W1[3] * dx + W1[4] * dy) + W1[5] * dz) + B1[1], 0.f);
        const float h2 = fmaxf(((W1[6] * dx + W1[7] * dy) + W1[8] * dz) + B1[2], 0.f);
        if (kq == 0) {
            s_h[row][0] = h0; s_h[row][1] = h1; s_h[row][2] = h2;
            s_nb[row] = (int)nb;
        }
        const float* krow = qkv + nb * ld + C;
        const float* qrow = qkv + q * ld;
        pt_f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (pt_f32x4){0.f, 0.f, 0.f, 0.f};
        for (int cb = 0; cb < C; cb += 16) {
            const int ch0 = cb + 4 * kq;
            const float4 k4 = *(const float4*)(krow + ch0), q4 = *(const float4*)(qrow + ch0);
            const float4 wa = *(const float4*)(p.pw2t + ch0), wb = *(const float4*)(p.pw2t + C + ch0),
                         wc = *(const float4*)(p.pw2t + 2 * C + ch0), bb = *(const float4*)(p.pb2 + ch0);
            const float4 sc = *(const float4*)(p.s0 + ch0), sh = *(const float4*)(p.t0 + ch0);
            float a[4];
            a[0] = fmaxf(sc.x * ((k4.x - q4.x) + (((wa.x * h0 + wb.x * h1) + wc.x * h2) + bb.x)) + sh.x, 0.f);
            a[1] = fmaxf(sc.y * ((k4.y - q4.y) + (((wa.y * h0 + wb.y * h1) + wc.y * h2) + bb.y)) + sh.y, 0.f);
            a[2] = fmaxf(sc.z * ((k4.z - q4.z) + (((wa.z * h0 + wb.z * h1) + wc.z * h2) + bb.z)) + sh.z, 0.f);
            a[3] = fmaxf(sc.w * ((k4.w - q4.w) + (((wa.w * h0 + wb.w * h1) + wc.w * h2) + bb.w)) + sh.w, 0.f);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 B = *(const float4*)(p.w1 + (size_t)(16 * nt + row) * C + ch0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], B.x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], B.y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], B.z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], B.w, acc[nt], 0, 0, 0);
            }
        }
        // D[i = 4 (l / 16) + r][j = l % 16]: hidden of row 4 kq + r, column 16 nt + (l % 16)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float b = p.b1[16 * nt + row];
#pragma unroll
            for (int r = 0; r < 4; ++r) s_hid[4 * kq + r][16 * nt + row] = fmaxf(acc[nt][r] + b, 0.f);
        }
        __syncthreads();
        for (int o = kq; o < cs; o += 4) {
            float s = 0.f;
            for (int k = 0; k < cs; ++k) s += p.w2[o * cs + k] * s_hid[row][k];
            s_w[row][o] = s + p.b2[o];
        }
        __syncthreads();
        for (int o = lane; o < QW * cs; o += 64) {      // softmax over the NS neighbours of (query o / cs, column o % cs)
            const int r0 = (o / cs) * NS, col = o % cs;
            float mx = s_w[r0][col];
#pragma unroll
            for (int j = 1; j < NS; ++j) mx = fmaxf(mx, s_w[r0 + j][col]);
            float e[NS], sum = 0.f;
#pragma unroll
            for (int j = 0; j < NS; ++j) { e[j] = expf(s_w[r0 + j][col] - mx); sum += e[j]; }
#pragma unroll
            for (int j = 0; j < NS; ++j) s_w[r0 + j][col] = e[j] / sum;
        }
        __syncthreads();
        for (int o = lane; o < QW * C; o += 64) {
            const int qs = o / C, ch = o % C;
            const int64_t qq = g * QW + qs;
            if (qq < n) {
                const float wa = p.pw2t[ch], wb = p.pw2t[C + ch], wc = p.pw2t[2 * C + ch], bb = p.pb2[ch];
                const int col = ch % cs;
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int rr = qs * NS + j;
                    const float v = qkv[(int64_t)s_nb[rr] * ld + 2 * C + ch];
                    const float r = ((wa * s_h[rr][0] + wb * s_h[rr][1]) + wc * s_h[rr][2]) + bb;
                    sum += (v + r) * s_w[rr][col];
                }
                if (p.es) sum = fmaxf(sum * p.es[ch] + p.et[ch], 0.f);
                out[qq * C + ch] = sum;
            }
        }
        __syncthreads();
    }
}

extern "C" int ml3d_pt_attention(const float* qkv, const float* points, const int32_t* neighbor_idx, int64_t n, int c,
                                 int nsample, const float* p_w1, const float* p_b1, const float* p_w2t, const float* p_b2,
                                 const float* w_scale0, const float* w_shift0, const float* w_w1, const float* w_b1,
                                 const float* w_w2, const float* w_b2, const float* ep_scale, const float* ep_shift,
                                 float* out, void* stream) {
    if (n < 0 || c < 16 || c > 512 || (c & 15) || (nsample != 8 && nsample != 16) || (ep_scale != nullptr) != (ep_shift != nullptr))
        return ML3D_E_INVALID;
    if (n == 0) return 0;
    if (!qkv || !points || !neighbor_idx || !p_w1 || !p_b1 || !p_w2t || !p_b2 || !w_scale0 || !w_shift0 || !w_w1 || !w_b1 ||
        !w_w2 || !w_b2 || !out)
        return ML3D_E_INVALID;
    if ((((uintptr_t)qkv | (uintptr_t)p_w2t | (uintptr_t)p_b2 | (uintptr_t)w_scale0 | (uintptr_t)w_shift0 | (uintptr_t)w_w1) & 15) != 0)
        return ML3D_E_INVALID;
    PtAttnParams p = {p_w1, p_b1, p_w2t, p_b2, w_scale0, w_shift0, w_w1, w_b1, w_w2, w_b2, ep_scale, ep_shift};
    const int nt = (c / 8 + 15) / 16;      // 1 (c <= 128), 2 (c <= 256), 3 or 4
    const int qw = 16 / nsample;
    const int64_t groups = (n + qw - 1) / qw;
    const unsigned nb = (unsigned)(groups < 256 * 24 ? groups : 256 * 24);
    hipStream_t st = (hipStream_t)stream;
#define PT_ATTN(NS_, NT_) hipLaunchKernelGGL((pt_attn_kernel<NS_, NT_>), dim3(nb), dim3(64), 0, st, qkv, points, neighbor_idx, n, c, p, out, groups)
    if (nsample == 8) {
        if (nt == 1) PT_ATTN(8, 1); else if (nt == 2) PT_ATTN(8, 2); else PT_ATTN(8, 4);
    } else {
        if (nt == 1) PT_ATTN(16, 1); else if (nt == 2) PT_ATTN(16, 2); else PT_ATTN(16, 4);
    }
#undef PT_ATTN
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------------
// (c) TransitionDown, stride != 1, after the per-SOURCE-point product y = feat . W_f (ml3d_linear): one thread per (sampled
// point, output channel) adds the position part W_x (p_j - p_i) of the Linear, applies the folded BN + ReLU and takes the
// maximum over the neighbours (after the affine step: the BN scale may be negative).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_down_kernel(const float* __restrict__ y, const float* __restrict__ pts, int64_t n_src,
                                                      const int32_t* __restrict__ sample, const int32_t* __restrict__ idx,
                                                      int64_t m, int ns, int C, const float* __restrict__ wx,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ out, float* __restrict__ out_pts) {
    const int64_t total = m * C;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t i = o / C;
        const int ch = (int)(o - i * C);
        int64_t qi = sample[i];
        qi = qi < 0 ? 0 : (qi >= n_src ? n_src - 1 : qi);
        const float qx = pts[3 * qi], qy = pts[3 * qi + 1], qz = pts[3 * qi + 2];
        if (out_pts && ch < 3) out_pts[3 * i + ch] = ch == 0 ? qx : (ch == 1 ? qy : qz);
        const float w0 = wx[ch], w1 = wx[C + ch], w2 = wx[2 * C + ch], sc = scale[ch], sh = shift[ch];
        float mx = 0.f;      // (every candidate is a ReLU output)
        for (int j = 0; j < ns; ++j) {
            int64_t nb = idx[i * ns + j];
            nb = nb < 0 ? 0 : (nb >= n_src ? n_src - 1 : nb);
            const float dx = pts[3 * nb] - qx, dy = pts[3 * nb + 1] - qy, dz = pts[3 * nb + 2] - qz;
            const float v = ((w0 * dx + w1 * dy) + w2 * dz) + y[nb * C + ch];
            mx = fmaxf(mx, sc * v + sh);
        }
        out[o] = mx;
    }
}

extern "C" int ml3d_pt_transition_down(const float* y, const float* points, int64_t n_src, const int32_t* sample_idx,
                                       const int32_t* neighbor_idx, int64_t m, int nsample, int c_out, const float* w_x,
                                       const float* scale, const float* shift, float* out, float* out_points, void* stream) {
    if (n_src < 0 || m < 0 || nsample <= 0 || nsample > 64 || c_out < 3 || c_out > 4096 || (m > 0 && n_src == 0)) return ML3D_E_INVALID;
    if (m == 0) return 0;
    if (!y || !points || !sample_idx || !neighbor_idx || !w_x || !scale || !shift || !out) return ML3D_E_INVALID;
    const int64_t total = m * c_out;
    const unsigned nb = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(pt_down_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, y, points, n_src, sample_idx, neighbor_idx, m,
                       nsample, c_out, w_x, scale, shift, out, out_points);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------------------
// (d) 3-NN inverse-distance interpolation + the add of TransitionUp: out[i] = a[i] + sum_t w_t b[idx[i, t]].
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_interp_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n_src,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ d2, int64_t n,
                                                        int k, int C, float* __restrict__ out) {
    const int64_t total = n * C;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t i = o / C;
        const int ch = (int)(o - i * C);
        float norm = 0.f;
        for (int t = 0; t < k; ++t) norm += 1.0f / (d2[i * k + t] + 1e-8f);
        float acc = 0.f;
        for (int t = 0; t < k; ++t) {
            int64_t nb = idx[i * k + t];
            nb = nb < 0 ? 0 : (nb >= n_src ? n_src - 1 : nb);
            const float w = (1.0f / (d2[i * k + t] + 1e-8f)) / norm;
            acc += b[nb * C + ch] * w;
        }
        out[o] = a ? a[o] + acc : acc;
    }
}

extern "C" int ml3d_pt_interpolate(const float* a, const float* b, int64_t n_src, const int32_t* idx, const float* dist2,
                                   int64_t n, int k, int c, float* out, void* stream) {
    if (n < 0 || n_src < 0 || k <= 0 || k > 16 || c <= 0 || (n > 0 && n_src == 0)) return ML3D_E_INVALID;
    if (n == 0) return 0;
    if (!b || !idx || !dist2 || !out) return ML3D_E_INVALID;
    const int64_t total = n * c;
    const unsigned nb = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(pt_interp_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, b, n_src, idx, dist2, n, k, c, out);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}
