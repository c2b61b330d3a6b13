// gemm.hip — tiled f32 MFMA GEMM with loader-templated A operand and fused epilogue (see gemm.h).
#include "gemm.h"

#include <stdlib.h>

#include <type_traits>

#include <gfx950_ops.h>

#include "grid.h"
#include "ml3d_hip.h"

namespace ml3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int GM_BM = 64;        // rows of C per workgroup
constexpr int GM_BN = 64;        // columns of C per workgroup
constexpr int GM_KC = 32;        // K chunk
constexpr int GM_AP = GM_KC + 4; // LDS pitch of the A tile (b128 reads without bank conflicts)
constexpr int GM_BP = GM_BN + 4;

__device__ __forceinline__ int mfma32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ float gm_act(float v, int act, float slope) {
    if (act == 1) return v > 0.f ? v : v * slope;
    if (act == 2) return v > 0.f ? v : 0.f;
    return v;
}

// ---- epilogue slow path: the pieces gemm_tile, tile2_epilogue and gemm_reduce share --------------------------------------
// pixel-shuffle store (Epilogue::ps): column col = (dy, dx, co), row m = input pixel (b, y, x) -> element offset of (output pixel,
// co) in C.  The column's part is split off so that the tile kernels pay its divisions once per column, not per element
struct PsCol { int co, dy, dx; };
__device__ __forceinline__ PsCol ps_col(int col, const Epilogue& ep) {
    PsCol c;
    c.co = col % ep.ps_cout;
    const int dd = col / ep.ps_cout;
    c.dy = dd / ep.ps; c.dx = dd % ep.ps;
    return c;
}
__device__ __forceinline__ int64_t ps_offset(int64_t m, const PsCol& c, const Epilogue& ep, int64_t ldc) {
    const int x = (int)(m % ep.ps_w);
    const int64_t t = m / ep.ps_w;
    const int y = (int)(t % ep.ps_h);
    const int64_t bi = t / ep.ps_h;
    const int64_t opix = (bi * ep.ps_h * ep.ps + (int64_t)y * ep.ps + c.dy) * ((int64_t)ep.ps_w * ep.ps) + (int64_t)x * ep.ps + c.dx;
    return opix * ldc + c.co;
}

// v + the residual of output element (m, col), gathered when ep.res_gather is set.  The item of row m comes from the caller: the
// tile kernels fix it once per tile (rg_base = source row base of the tile's FIRST row's item, rg_l = m's distance from that item's
// first row; a tile crosses items at most once), gemm_reduce passes the row's own item base and rg_l = 0
__device__ __forceinline__ float add_residual(float v, const Epilogue& ep, int64_t m, int col, int64_t rg_base, int64_t rg_l) {
    if (ep.residual) {
        int64_t rr = m;
        bool take = true;
        if (ep.res_gather) {
            const int64_t g = ep.res_gather[ep.rg_stride ? m * ep.rg_stride : m];
            take = g >= 0 && g < ep.rg_limit;
            rr = rg_base + (rg_l >= ep.rg_rows_per_item ? ep.rg_src_rows_per_item : 0) + g;
        }
        if (take) v += ep.residual[rr * ep.ldr + col];
    }
    return v;
}

// ---- epilogue fast path -------------------------------------------------------------------------------------------------
// The plain epilogue (bias [+ bias2] [+ residual] + activation, row-major C) is the whole kernel for shallow K: RandLA's and
// KPConv's Linears have K = 32 .. 128 (1-4 chunks), and the generic store -- a 64-bit m * ldc + col, a bounds test and the
// activation switch per element -- spent ~15 VALU instructions per output, which the f32 MFMAs cannot overlap.  When the output
// is addressable with 32-bit offsets the row base is a SCALAR pointer (tile row origin + r-dependent row, uniform) and the
// lane's contribution (its column + its half's 4 rows) one 32-bit offset computed once: a store is the bias add, the
// activation and a global_store with scalar base.  ACT is resolved outside the element loops.
template <int ACT>
__device__ __forceinline__ float gm_act_t(float v, float slope) {
    if (ACT == 1) return v > 0.f ? v : v * slope;
    if (ACT == 2) return v > 0.f ? v : 0.f;
    return v;
}

// one 32 x 32 accumulator block whose first row is `mrow0` (uniform): rows mrow0 + mfma32_row(r, hi), column `col`
template <int ACT, bool FULL, bool RES>
__device__ __forceinline__ void store_block32(const f32x16& acc, float b, float slope, float* __restrict__ C, int64_t ldc,
                                              const float* __restrict__ R, int64_t ldr, int64_t mrow0, int64_t M, int col,
                                              int hi) {
    // the lane's pointer to (row mrow0 + 4 hi, column col), once; every store adds a UNIFORM row offset (scalar multiply)
    float* cp = C + (mrow0 + 4 * hi) * ldc + col;
    const float* rp = RES ? R + (mrow0 + 4 * hi) * ldr + col : nullptr;
    const int rows_left = (int)(M - mrow0 < 32 ? M - mrow0 : 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ur = (r & 3) + 8 * (r >> 2);                // uniform part of the row; the lane's half adds 4 * hi
        // (the scalar offsets come BEFORE the row predicate: every lane takes part in every readfirstlane)
        const int so_c = __builtin_amdgcn_readfirstlane(ur * (int)ldc);
        const int so_r = RES ? __builtin_amdgcn_readfirstlane(ur * (int)ldr) : 0;
        if (!FULL && ur + 4 * hi >= rows_left) continue;
        float v = acc[r] + b;
        if (RES) v += rp[so_r];
        cp[so_c] = gm_act_t<ACT>(v, slope);
    }
}

// ACT and FULL are resolved ONCE per kernel, outside the block loops (the loops stay small enough to unroll: the accumulators
// must never be indexed dynamically)
template <class F>
__device__ __forceinline__ void dispatch_act_full(int act, bool full, F&& f) {
    using T = std::integral_constant<bool, true>;
    using N = std::integral_constant<bool, false>;
    if (act == 1) { if (full) f(std::integral_constant<int, 1>{}, T{}); else f(std::integral_constant<int, 1>{}, N{}); }
    else if (act == 2) { if (full) f(std::integral_constant<int, 2>{}, T{}); else f(std::integral_constant<int, 2>{}, N{}); }
    else { if (full) f(std::integral_constant<int, 0>{}, T{}); else f(std::integral_constant<int, 0>{}, N{}); }
}

// 32-bit offsets inside a 36-row window of C / the residual (a block's rows + the lane's 4 * hi)
__device__ __forceinline__ bool fast_store_ok(const Epilogue& ep, int64_t ldc, int N) {
    return ep.ps == 0 && !ep.residual && 36 * ldc + N < 0x7fffffffll;
}

// ---- A loaders ---------------------------------------------------------------------------------------
struct RowsLoader {
    RowsA A;
    int64_t M;
    int K;
    int vec;   // 1: every block is float4-addressable (k1, k2, lda, lda2 multiples of 4, 16-byte aligned bases)
    struct Ctx { const float* p1; const float* p2; };
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c; c.p1 = nullptr; c.p2 = nullptr;
        if (m < M) {
            int64_t r = m;
            bool ok = true;
            if (A.gather) {
                r = A.gather[m * A.gather_stride];
                ok = r >= 0 && r < A.a_rows;
                if (A.g_rows_per_item > 0) r += (m / A.g_rows_per_item) * A.g_src_rows_per_item;
            }
            if (!A.gather_on_a2) {
                if (ok) c.p1 = A.a + r * A.lda;
                if (A.a2) c.p2 = A.a2 + m * A.lda2;
            } else {
                c.p1 = A.a + m * A.lda;
                if (A.a2 && ok) c.p2 = A.a2 + r * A.lda2;
            }
        }
        return c;
    }
    __device__ __forceinline__ float at(const Ctx& c, int k) const {
        if (k < A.k1) return c.p1 ? c.p1[k] : 0.f;
        if (k < K) return c.p2 ? c.p2[k - A.k1] : 0.f;
        return 0.f;
    }
    // k0 = the K chunk's first column (wave-uniform), kq = this thread's offset inside the chunk
    __device__ __forceinline__ float4 load4(const Ctx& c, int k0, int kq) const {
        const int k = k0 + kq;
        if (vec) {
            if (k < A.k1) return c.p1 ? *reinterpret_cast<const float4*>(c.p1 + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < K) return c.p2 ? *reinterpret_cast<const float4*>(c.p2 + (k - A.k1)) : make_float4(0.f, 0.f, 0.f, 0.f);
            return make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return make_float4(at(c, k), at(c, k + 1), at(c, k + 2), at(c, k + 3));
    }
};

struct ConvLoader {
    ConvA A;
    int64_t M;
    int K;
    int chunk_uniform;   // 1: C % 32 == 0, so a 32-wide K chunk lies inside ONE (ky, kx) tap and the tap is wave-uniform
    struct Ctx { const float* img; int iy0, ix0; };
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c; c.img = nullptr; c.iy0 = 0; c.ix0 = 0;
        if (m < M) {
            int ox, oy, b;
            if (M <= 0x7fffffffll) {        // (uniform) 32-bit divisions: ~20 instructions each instead of ~100 for int64
                const unsigned mu = (unsigned)m, t = mu / (unsigned)A.OW;
                ox = (int)(mu - t * (unsigned)A.OW);
                b = (int)(t / (unsigned)A.OH);
                oy = (int)(t - (unsigned)b * (unsigned)A.OH);
            } else {
                ox = (int)(m % A.OW);
                const int64_t t = m / A.OW;
                oy = (int)(t % A.OH);
                b = (int)(t / A.OH);
            }
            c.img = A.in + (int64_t)b * A.H * A.W * A.C;
            c.iy0 = oy * A.stride - A.pad;
            c.ix0 = ox * A.stride - A.pad;
        }
        return c;
    }
    // C % 4 == 0: the 4 consecutive k share (ky, kx)
    __device__ __forceinline__ float4 load4(const Ctx& c, int k0, int kq) const {
        const int k = k0 + kq;
        if (!c.img || k >= K) return make_float4(0.f, 0.f, 0.f, 0.f);
        int ci, kk;
        if (chunk_uniform) {          // tap from the chunk origin only: scalar arithmetic, no per-lane divisions
            kk = k0 / A.C;
            ci = k0 - kk * A.C + kq;
        } else {
            ci = k % A.C;
            kk = k / A.C;
        }
        int kx = kk % A.KW, ky = kk / A.KW;
        int iy = c.iy0 + ky, ix = c.ix0 + kx;
        if (iy < 0 || iy >= A.H || ix < 0 || ix >= A.W) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(c.img + ((int64_t)iy * A.W + ix) * A.C + ci);
    }
};

// ---- tile kernel -------------------------------------------------------------------------------------
// PLAIN (RowsLoader only): one or two dense float4-addressable column blocks of A with chunk-aligned widths, float4-addressable B --
// the staging loads are running pointers (no per-chunk predicates, no loader branches).  The generic fetch below is ~170 VALU / 365
// SALU instructions of control flow per chunk of 16 MFMAs in the listing; the Linears of RandLA-Net and KPConv (K = 32 .. 1024,
// almost all plain) spent more time in it than in the matrix unit.
template <class Loader, bool PLAIN = false, int DEPTH = 2>
__global__ void __launch_bounds__(256)
gemm_tile(Loader L, const float* __restrict__ Bm, int N, int bvec, Epilogue ep, float* __restrict__ C, int64_t ldc,
          int k_per_split, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float As[GM_BM * GM_AP];
    __shared__ __attribute__((aligned(16))) float Bs[GM_KC * GM_BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, cl = lane & 31;
    const int rt = wave & 1, ctw = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM_BM;
    const int n0 = blockIdx.y * GM_BN;
    const int kb = blockIdx.z * k_per_split;
    const int ke = (kb + k_per_split < L.K) ? kb + k_per_split : L.K;

    // this thread stages A rows (tid >> 3) and 32 + (tid >> 3), k offset 4 * (tid & 7);
    // B rows (tid >> 4) and 16 + (tid >> 4), column offset 4 * (tid & 15)
    const int ar = tid >> 3, aq = (tid & 7) * 4;
    const int br = tid >> 4, bq = (tid & 15) * 4;
    const typename Loader::Ctx c0 = L.prepare(m0 + ar), c1 = L.prepare(m0 + 32 + ar);

    // TWO register sets: the global loads of chunks k + 1 and k + 2 are in flight while chunk k is multiplied.  A workgroup walks
    // its chunks serially and one chunk's loads take 1-2.5 us against 0.43 us of MFMAs: with one chunk in flight (rounds 1-2) every
    // iteration waited for memory, and the small-M / deep-K GEMMs of KPConv's coarse layers (one round of workgroups: the
    // kernel takes as long as ONE workgroup) ran at ~2.6 us per chunk (profiles/r03_kp_kernel_stats.csv: 34 launches of 70-120 us).
    float4 ra0, ra1, rb0, rb1;       // set 0
    float4 sa0, sa1, sb0, sb1;       // set 1
    // PLAIN: rows past M re-read row M - 1 and columns past N re-read column 0 (their products are never stored)
    const float* pa0 = nullptr; const float* pa1 = nullptr; const float* pb0 = nullptr; const float* pb1 = nullptr;
    const float* qa0 = nullptr; const float* qa1 = nullptr;      // the second column block ([a | a2] concatenated, chunk-aligned)
    if constexpr (PLAIN) {
        const int64_t r0 = m0 + ar < L.M ? m0 + ar : L.M - 1, r1 = m0 + 32 + ar < L.M ? m0 + 32 + ar : L.M - 1;
        pa0 = L.A.a + r0 * L.A.lda + kb + aq;
        pa1 = L.A.a + r1 * L.A.lda + kb + aq;
        if (L.A.k2 > 0) {
            const int k2b = kb > L.A.k1 ? kb - L.A.k1 : 0;
            qa0 = L.A.a2 + r0 * L.A.lda2 + k2b + aq;
            qa1 = L.A.a2 + r1 * L.A.lda2 + k2b + aq;
        }
        const int colb = n0 + bq + 3 < N ? n0 + bq : 0;
        pb0 = Bm + (int64_t)(kb + br) * N + colb;
        pb1 = pb0 + (int64_t)16 * N;
    }
    auto load_b = [&](int k) -> float4 {
        const int col = n0 + bq;
        if (k >= ke) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = Bm + (int64_t)k * N + col;
        if (bvec && col + 3 < N) return *reinterpret_cast<const float4*>(p);
        float4 v;
        v.x = col + 0 < N ? p[0] : 0.f;
        v.y = col + 1 < N ? p[1] : 0.f;
        v.z = col + 2 < N ? p[2] : 0.f;
        v.w = col + 3 < N ? p[3] : 0.f;
        return v;
    };
    // (plain lambdas over named registers: passing a register struct by reference left it in scratch memory)
#define ML3D_GM_FETCH(A0, A1, B0, B1, K0)                                                            \
    do {                                                                                             \
        const int k0_ = (K0);                                                                        \
        if constexpr (PLAIN) {                                                                       \
            if (k0_ < L.A.k1) { /* (uniform: block boundaries are chunk-aligned) */                  \
                A0 = *reinterpret_cast<const float4*>(pa0);                                          \
                A1 = *reinterpret_cast<const float4*>(pa1);                                          \
                pa0 += GM_KC; pa1 += GM_KC;                                                          \
            } else {                                                                                 \
                A0 = *reinterpret_cast<const float4*>(qa0);                                          \
                A1 = *reinterpret_cast<const float4*>(qa1);                                          \
                qa0 += GM_KC; qa1 += GM_KC;                                                          \
            }                                                                                        \
            B0 = *reinterpret_cast<const float4*>(pb0);                                              \
            B1 = *reinterpret_cast<const float4*>(pb1);                                              \
            pb0 += (int64_t)GM_KC * N; pb1 += (int64_t)GM_KC * N;                                    \
        } else {                                                                                     \
            const int ka_ = k0_ + aq;                                                                \
            A0 = ka_ < ke ? L.load4(c0, k0_, aq) : make_float4(0.f, 0.f, 0.f, 0.f);                   \
            A1 = ka_ < ke ? L.load4(c1, k0_, aq) : make_float4(0.f, 0.f, 0.f, 0.f);                   \
            B0 = load_b(k0_ + br);                                                                   \
            B1 = load_b(k0_ + 16 + br);                                                              \
        }                                                                                            \
    } while (0)
#define ML3D_GM_STASH(A0, A1, B0, B1)                                                                \
    do {                                                                                             \
        *reinterpret_cast<float4*>(As + ar * GM_AP + aq) = A0;                                       \
        *reinterpret_cast<float4*>(As + (32 + ar) * GM_AP + aq) = A1;                                \
        *reinterpret_cast<float4*>(Bs + br * GM_BP + bq) = B0;                                       \
        *reinterpret_cast<float4*>(Bs + (16 + br) * GM_BP + bq) = B1;                                \
    } while (0)
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    auto multiply = [&]() {
        const float* arow = As + (rt * 32 + cl) * GM_AP + hi * (GM_KC / 2);
        const float* brow = Bs + (hi * (GM_KC / 2)) * GM_BP + ctw * 32 + cl;
#pragma unroll
        for (int s4 = 0; s4 < GM_KC / 8; ++s4) {
            const float4 a = *reinterpret_cast<const float4*>(arow + 4 * s4);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, brow[(4 * s4 + 0) * GM_BP], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, brow[(4 * s4 + 1) * GM_BP], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, brow[(4 * s4 + 2) * GM_BP], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, brow[(4 * s4 + 3) * GM_BP], acc, 0, 0, 0);
        }
    };


    if constexpr (DEPTH == 1) {              // one chunk in flight (rounds 1-2): 36 registers, eight waves per SIMD
        if (kb < ke) {
            ML3D_GM_FETCH(ra0, ra1, rb0, rb1, kb);
            ML3D_GM_STASH(ra0, ra1, rb0, rb1);
            block_sync_lds();
            for (int k0 = kb; k0 < ke; k0 += GM_KC) {
                const bool more = k0 + GM_KC < ke;
                if (more) ML3D_GM_FETCH(ra0, ra1, rb0, rb1, k0 + GM_KC);
                multiply();
                block_sync_lds();
                if (more) {
                    ML3D_GM_STASH(ra0, ra1, rb0, rb1);
                    block_sync_lds();
                }
            }
        }
    } else if (kb < ke) {
        ML3D_GM_FETCH(ra0, ra1, rb0, rb1, kb);
        if (kb + GM_KC < ke) ML3D_GM_FETCH(sa0, sa1, sb0, sb1, kb + GM_KC);
        ML3D_GM_STASH(ra0, ra1, rb0, rb1);
        block_sync_lds();
        // LDS holds chunk k0; the loop body is unrolled by two so that the register sets alternate statically
        for (int k0 = kb; k0 < ke; k0 += 2 * GM_KC) {
            if (k0 + 2 * GM_KC < ke) ML3D_GM_FETCH(ra0, ra1, rb0, rb1, k0 + 2 * GM_KC);      // set 1 (chunk k0 + 1) is in flight or landed
            multiply();
            // (LDS-only barriers: the outstanding global loads stay in flight across them)
            block_sync_lds();
            if (!(k0 + GM_KC < ke)) break;
            ML3D_GM_STASH(sa0, sa1, sb0, sb1);
            block_sync_lds();
            if (k0 + 3 * GM_KC < ke) ML3D_GM_FETCH(sa0, sa1, sb0, sb1, k0 + 3 * GM_KC);
            multiply();
            block_sync_lds();
            if (k0 + 2 * GM_KC < ke) {
                ML3D_GM_STASH(ra0, ra1, rb0, rb1);
                block_sync_lds();
            }
        }
    }
    // ---- epilogue ------------------------------------------------------------------------------------
    const int col = n0 + ctw * 32 + cl;
    if (col >= N) return;
    if (partial) {
        float* P = partial + (int64_t)blockIdx.z * L.M * N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + rt * 32 + mfma32_row(r, hi);
            if (m < L.M) P[m * N + col] = acc[r];
        }
        return;
    }
    if (ep.ps > 0) {
        const PsCol pc = ps_col(col, ep);
        const float b = ep.bias ? ep.bias[pc.co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + rt * 32 + mfma32_row(r, hi);
            if (m < L.M) C[ps_offset(m, pc, ep, ldc)] = gm_act(acc[r] + b, ep.act, ep.slope);
        }
        return;
    }
    float b = ep.bias ? ep.bias[col] : 0.f;
    if (ep.bias2) b += ep.bias2[col];
    if (fast_store_ok(ep, ldc, N)) {
        const int64_t mrow0 = m0 + __builtin_amdgcn_readfirstlane(rt) * 32;      // (scalar: uniform row offsets below)
        dispatch_act_full(ep.act, mrow0 + 32 <= L.M, [&](auto act_c, auto full_c) {
            store_block32<decltype(act_c)::value, decltype(full_c)::value, false>(acc, b, ep.slope, C, ldc, nullptr, 0, mrow0, L.M,
                                                                                  col, hi);
        });
        return;
    }
    // gathered residual: the tile's first row fixes the item (scalar division); a 64-row tile crosses items at most once
    int64_t rg_base = 0, rg_l0 = 0;
    if (ep.res_gather) {
        const int64_t item0 = m0 / ep.rg_rows_per_item;
        rg_l0 = m0 - item0 * ep.rg_rows_per_item;
        rg_base = item0 * ep.rg_src_rows_per_item;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = rt * 32 + mfma32_row(r, hi);
        const int64_t m = m0 + lr;
        if (m < L.M) C[m * ldc + col] = gm_act(add_residual(acc[r] + b, ep, m, col, rg_base, rg_l0 + lr), ep.act, ep.slope);
    }
}

constexpr int G2_BM = 128;

// ---- epilogue of the 128-row kernels (bias + residual + activation, or the pixel-shuffle store) -------------------------
// a wave's RT x CT blocks of 32 x 32: rows m0 + 64 wr + 32 i + mfma32_row(r, hi), columns n0 + 32 CT wc + 32 j + cl
template <int RT, int CT>
__device__ __forceinline__ void tile2_epilogue(f32x16 (&acc)[RT][CT], const Epilogue& ep, float* __restrict__ C, int64_t ldc,
                                               int64_t M, int N, int64_t m0, int n0, int wr, int wc, int hi, int cl) {
    if (fast_store_ok(ep, ldc, N)) {
        const int64_t mw0 = m0 + __builtin_amdgcn_readfirstlane(wr) * 64;        // (scalar: uniform row offsets below)
        dispatch_act_full(ep.act, m0 + G2_BM <= M, [&](auto act_c, auto full_c) {
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const int col = n0 + wc * (32 * CT) + 32 * j + cl;
                if (col < N) {
                    float b = ep.bias ? ep.bias[col] : 0.f;
                    if (ep.bias2) b += ep.bias2[col];
#pragma unroll
                    for (int i = 0; i < RT; ++i)
                        store_block32<decltype(act_c)::value, decltype(full_c)::value, false>(acc[i][j], b, ep.slope, C, ldc, nullptr,
                                                                                              0, mw0 + i * 32, M, col, hi);
                }
            }
        });
        return;
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int col = n0 + wc * (32 * CT) + 32 * j + cl;
        if (col >= N) continue;
        if (ep.ps > 0) {
            const PsCol pc = ps_col(col, ep);
            const float b = ep.bias ? ep.bias[pc.co] : 0.f;
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = m0 + wr * 64 + i * 32 + mfma32_row(r, hi);
                    if (m < M) C[ps_offset(m, pc, ep, ldc)] = gm_act(acc[i][j][r] + b, ep.act, ep.slope);
                }
            continue;
        }
        float b = ep.bias ? ep.bias[col] : 0.f;
        if (ep.bias2) b += ep.bias2[col];
        // gathered residual (round 6: the decoder step split by linearity on the bf16 pipe as well): the tile's first row fixes the
        // item with ONE scalar division; a 128-row tile crosses items at most once (the host checks rg_rows_per_item >= 128)
        int64_t rg_base = 0, rg_l0 = 0;
        if (ep.res_gather) {
            const int64_t item0 = m0 / ep.rg_rows_per_item;
            rg_l0 = m0 - item0 * ep.rg_rows_per_item;
            rg_base = item0 * ep.rg_src_rows_per_item;
        }
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wr * 64 + i * 32 + mfma32_row(r, hi);
                const int64_t m = m0 + lr;
                if (m < M) C[m * ldc + col] = gm_act(add_residual(acc[i][j][r] + b, ep, m, col, rg_base, rg_l0 + lr), ep.act, ep.slope);
            }
    }
}

// ---- 128-row tile kernel: register-blocked MFMA ----------------------------------------------------------------------
// The 64 x 64 kernel above gives every wave ONE 32 x 32 accumulator: each MFMA needs its own A and B value from LDS and the
// loader's address arithmetic is paid per 16 MFMAs.  On gfx950 the f32 MFMAs do not overlap VALU / LDS issue
// (tools/micro/mfma_valu_overlap.hip), so those instructions are lost matrix time: 0.5 of peak.  Here a workgroup owns
// 128 rows x BN columns and a wave a 2 x 2 (BN = 128) or 2 x 1 (BN = 64) block of 32 x 32 accumulators: an A value feeds
// two MFMAs, a B value two more, and the per-chunk loader work (same per staged element) is spread over 4x / 2x the
// MFMAs.  The conv loader keeps ONE int per staged row (element offset of the receptive field's corner) and a 9-bit mask
// of the taps that fall inside the image; a K chunk lies inside one tap (C % 32 == 0), so per chunk a staged float4
// costs a bit test and an add.  Interior rows never see a branch.
struct ConvLoader2 {
    ConvA A;
    int64_t M;
    int K;
    struct Ctx { int off; unsigned taps; };     // off: element offset of (b, iy0, ix0, 0) (may be negative); taps: valid (ky, kx)
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c; c.off = 0; c.taps = 0u;
        if (m < M) {
            // (M = B * OH * OW < 2^31 is a precondition of this loader: 32-bit divisions, ~20 instructions each instead of ~100)
            const unsigned mu = (unsigned)m;
            const unsigned t = mu / (unsigned)A.OW;
            const int ox = (int)(mu - t * (unsigned)A.OW);
            const int b = (int)(t / (unsigned)A.OH);
            const int oy = (int)(t - (unsigned)b * (unsigned)A.OH);
            const int iy0 = oy * A.stride - A.pad, ix0 = ox * A.stride - A.pad;
            c.off = ((b * A.H + iy0) * A.W + ix0) * A.C;
            for (int ky = 0; ky < A.KH; ++ky)
                for (int kx = 0; kx < A.KW; ++kx)
                    if (iy0 + ky >= 0 && iy0 + ky < A.H && ix0 + kx >= 0 && ix0 + kx < A.W) c.taps |= 1u << (ky * A.KW + kx);
        }
        return c;
    }
    // k0: the chunk's first column (uniform) -> tap and channel origin on the scalar unit
    __device__ __forceinline__ float4 load4(const Ctx& c, int k0, int kq) const {
        const int tap = k0 / A.C;
        const int ci = k0 - tap * A.C + kq;
        const int ky = tap / A.KW, kx = tap - ky * A.KW;
        if (!((c.taps >> tap) & 1u)) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(A.in + (c.off + (ky * A.W + kx) * A.C + ci));
    }
    // the same walk over K without the per-chunk divisions: (tap, element offset of the tap + channel origin) carried from chunk to
    // chunk on the scalar unit (~100 SALU instructions per chunk less than load4's k0 / C, tap / KW)
    struct Walk { int tap, kx, ci, toff; };
    __device__ __forceinline__ Walk walk_begin(int /* k0 == 0: convolutions are never split along K */) const { Walk w; w.tap = 0; w.kx = 0; w.ci = 0; w.toff = 0; return w; }
    __device__ __forceinline__ void walk_next(Walk& w, int kc) const {
        w.ci += kc;
        w.toff += kc;
        if (w.ci >= A.C) {                       // next tap: the pixel to the right (contiguous with this one's channels), or the
                                                 // first pixel of the next image row
            w.ci = 0;
            ++w.tap;
            ++w.kx;
            if (w.kx == A.KW) { w.kx = 0; w.toff += (A.W - A.KW) * A.C; }
        }
    }
    __device__ __forceinline__ float4 load4w(const Ctx& c, const Walk& w, int kq) const {
        if (!((c.taps >> w.tap) & 1u)) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(A.in + (c.off + w.toff + kq));
    }
};

// dense rows [M, k1 | k2] (one or two column blocks, each float4-addressable, k1 % 32 == 0 so that a chunk lies inside one block) for
// the 128-row kernels: Linears, "unary2 + shortcut" over concatenated inputs, KPConv's contraction, deconvolutions as GEMMs
struct RowsLoader2 {
    const float* a;
    int64_t lda;
    const float* a2;        // second block (columns k1 ..) or null
    int64_t lda2;
    int k1;
    int64_t M;
    int K;
    struct Ctx { const float* p1; const float* p2; };
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c;
        c.p1 = m < M ? a + m * lda : nullptr;
        c.p2 = (m < M && a2) ? a2 + m * lda2 - k1 : nullptr;      // (indexed by the global column k >= k1)
        return c;
    }
    struct Walk { int k; };
    __device__ __forceinline__ Walk walk_begin(int k0) const { Walk w; w.k = k0; return w; }
    __device__ __forceinline__ void walk_next(Walk& w, int kc) const { w.k += kc; }
    __device__ __forceinline__ float4 load4w(const Ctx& c, const Walk& w, int kq) const {
        const float* p = w.k < k1 ? c.p1 : c.p2;                   // (uniform choice: the chunk's block)
        return p ? *reinterpret_cast<const float4*>(p + w.k + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// implicit im2col of a channels-last VOLUME [B, D, H, W, C] for the 3 x 3 x 3 / stride 1 / pad 1 convolution (PVCNN's voxel branch):
// ConvLoader2 with one more axis.  Row m = (b, z, y, x); k = ((kd * 3 + kh) * 3 + kw) * C + ci.  The 27 taps fit the 32-bit mask; a
// 32-deep chunk lies inside one tap (C % 32 == 0); the walk carries (tap, element offset of the tap) on the scalar unit: + C per tap
// (the voxel to the right is contiguous), + (W - 3) C at the end of a kw run, + (H - 3) W C at the end of a kh run.  A tap the zero
// padding removes is never dereferenced (its float4 is zero), so `off` may point in front of the volume.
struct Conv3dLoader {
    Conv3dA A;
    int64_t M;
    int K;
    struct Ctx { int off; unsigned taps; };
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c; c.off = 0; c.taps = 0u;
        if (m < M) {
            const unsigned mu = (unsigned)m;                 // (M = B D H W < 2^31: checked on the host)
            const unsigned t1 = mu / (unsigned)A.W;
            const int x = (int)(mu - t1 * (unsigned)A.W);
            const unsigned t2 = t1 / (unsigned)A.H;
            const int y = (int)(t1 - t2 * (unsigned)A.H);
            const int b = (int)(t2 / (unsigned)A.D);
            const int z = (int)(t2 - (unsigned)b * (unsigned)A.D);
            c.off = (((b * A.D + z - 1) * A.H + y - 1) * A.W + x - 1) * A.C;
            for (int kd = 0; kd < 3; ++kd)
                for (int kh = 0; kh < 3; ++kh)
                    for (int kw = 0; kw < 3; ++kw)
                        if (z + kd >= 1 && z + kd <= A.D && y + kh >= 1 && y + kh <= A.H && x + kw >= 1 && x + kw <= A.W)
                            c.taps |= 1u << ((kd * 3 + kh) * 3 + kw);
        }
        return c;
    }
    struct Walk { int tap, kw, kh, ci, toff; };
    __device__ __forceinline__ Walk walk_begin(int /* k0 == 0: never split along K */) const {
        Walk w; w.tap = 0; w.kw = 0; w.kh = 0; w.ci = 0; w.toff = 0; return w;
    }
    __device__ __forceinline__ void walk_next(Walk& w, int kc) const {
        w.ci += kc;
        w.toff += kc;
        if (w.ci >= A.C) {
            w.ci = 0;
            ++w.tap;
            if (++w.kw == 3) {
                w.kw = 0;
                w.toff += (A.W - 3) * A.C;
                if (++w.kh == 3) { w.kh = 0; w.toff += (A.H - 3) * A.W * A.C; }
            }
        }
    }
    __device__ __forceinline__ float4 load4w(const Ctx& c, const Walk& w, int kq) const {
        if (!((c.taps >> w.tap) & 1u)) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(A.in + (c.off + w.toff + kq));
    }
};

// rulebook gather of a sparse voxel set (SparseConvUnet's submanifold 3 x 3 x 3, strided 2 x 2 x 2 and transposed convolutions and
// the final Linear gathered through index_map): row m, tap t reads input row rule[m * taps + t]; k = t * cp + ci, so a 32-deep
// chunk lies inside one tap (cp % 32 == 0) and the walk carries (tap, channel origin) on the scalar unit.  Conv3dLoader's mask in a
// register does not apply -- the rule row IS the mask: a staged row reads its ONE rule entry of the chunk (4 bytes beside the 16 of
// the float4 it fetches; the 8 lanes that stage a row's 32 channels read the same word, one request), and an entry outside
// [0, in_rows) -- the -1 of an absent neighbour -- gives a zero float4 without a dereference.  Past the taps an optional dense
// block a2 [M, k2] supplies further columns (RowsLoader2's second block).
struct SparseConvLoader {
    SparseConvA A;
    int64_t M;
    int K;
    struct Ctx { const int32_t* r; const float* p2; };
    __device__ __forceinline__ Ctx prepare(int64_t m) const {
        Ctx c;
        c.r = m < M ? A.rule + m * A.taps : nullptr;
        c.p2 = (m < M && A.a2) ? A.a2 + m * A.lda2 : nullptr;
        return c;
    }
    struct Walk { int tap, ci; };
    __device__ __forceinline__ Walk walk_begin(int k0) const {
        Walk w;
        w.tap = k0 / A.cp;
        if (w.tap > A.taps) w.tap = A.taps;
        w.ci = k0 - w.tap * A.cp;
        return w;
    }
    __device__ __forceinline__ void walk_next(Walk& w, int kc) const {
        w.ci += kc;
        if (w.tap < A.taps && w.ci >= A.cp) { w.ci = 0; ++w.tap; }
    }
    __device__ __forceinline__ float4 load4w(const Ctx& c, const Walk& w, int kq) const {
        if (w.tap < A.taps) {                                        // (uniform)
            if (!c.r) return make_float4(0.f, 0.f, 0.f, 0.f);
            const int e = c.r[w.tap];
            if ((unsigned)e >= (unsigned)A.in_rows) return make_float4(0.f, 0.f, 0.f, 0.f);
            return *reinterpret_cast<const float4*>(A.in + (int64_t)e * A.ldi + w.ci + kq);
        }
        return c.p2 ? *reinterpret_cast<const float4*>(c.p2 + w.ci + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// XCD-aware tile order.  Workgroups are dealt to the 8 XCDs round-robin by their linear id, and every XCD has its own L2: with
// the identity mapping the 128-row tiles that share input rows (the 3 x 3 taps of neighbouring pixels) sit on 8 different L2s
// and each XCD streams nearly the whole image.  Here XCD x owns a CONTIGUOUS run of tiles (the column tiles of one row tile
// adjacent), so concurrently running neighbours hit one L2: SECOND's convolutions at 16 sweeps, f32 kernel, 0.691 -> 0.612, 0.643 ->
// 0.586, 0.622 -> 0.590, 0.670 -> 0.641 ms (profiles/r05_bf16x3_conv.log).
__device__ __forceinline__ void xcd_tile(int& bx, int& by) {
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy;
    const unsigned lin = blockIdx.x + gx * blockIdx.y;
    const unsigned xcd = lin & 7u, slot = lin >> 3;
    const unsigned base = total >> 3, rem = total & 7u;
    const unsigned t = xcd * base + (xcd < rem ? xcd : rem) + slot;
    bx = (int)(t / gy);
    by = (int)(t - (unsigned)bx * gy);
}

template <class Loader, int BN, int KC>
__global__ void __launch_bounds__(256)
gemm_tile2(Loader L, const float* __restrict__ Bm, int N, Epilogue ep, float* __restrict__ C, int64_t ldc) {
    constexpr int BP = BN + 4;
    constexpr int RT = 2;                       // 32-row tiles per wave
    constexpr int CT = BN / 64;                 // 32-column tiles per wave (BN = 128: 2, BN = 64: 1)
    constexpr int AP = KC + 4;                  // LDS pitch of the A tile
    constexpr int NA4 = KC / 8;                 // A float4 per thread and chunk (128 rows x KC / 256 threads / 4)
    constexpr int NB4 = KC * BN / 1024;         // B float4 per thread and chunk
    __shared__ __attribute__((aligned(16))) float As[G2_BM * AP];
    __shared__ __attribute__((aligned(16))) float Bs[KC * BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, cl = lane & 31;
    const int wr = wave & 1, wc = wave >> 1;     // wave's 64-row half / column half
    int tbx, tby;
    xcd_tile(tbx, tby);
    const int64_t m0 = (int64_t)tbx * G2_BM;
    const int n0 = tby * BN;
    const int K = L.K;

    // staging: A rows (tid / (KC / 4)) + (1024 / KC) j, k offset 4 (tid % (KC / 4));  B rows (tid / (BN / 4)) + (1024 / BN) j,
    // column 4 (tid % (BN / 4))
    constexpr int ATH = KC / 4;                  // threads per A row
    constexpr int ARS = 256 / ATH;               // A rows per pass
    const int ar = tid / ATH, aq = (tid % ATH) * 4;
    constexpr int BTH = BN / 4;                  // threads per B row
    const int br = tid / BTH, bq = (tid % BTH) * 4;
    constexpr int NROW = 128 / ARS;              // staged A rows per thread
    static_assert(NROW == NA4, "A staging");
    typename Loader::Ctx cx[NROW];
#pragma unroll
    for (int j = 0; j < NROW; ++j) cx[j] = L.prepare(m0 + ar + ARS * j);
    const bool bcol_ok = n0 + bq + 3 < N;

    // ONE register set for the staged chunk (a second set, chunk c + 2 requested before the MFMAs of chunk c, measured slower on
    // SECOND's 3x3 64 -> 64 conv: 0.353 against 0.328 ms -- the extra registers cost more than the latency they hide)
    float4 ra[NA4], rb[NB4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA4; ++j) ra[j] = L.load4(cx[j], k0, aq);
#pragma unroll
        for (int j = 0; j < NB4; ++j) {
            const int k = k0 + br + (256 / BTH) * j;
            rb[j] = (bcol_ok && k < K) ? *reinterpret_cast<const float4*>(Bm + (int64_t)k * N + n0 + bq) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < NA4; ++j) *reinterpret_cast<float4*>(As + (ar + ARS * j) * AP + aq) = ra[j];
#pragma unroll
        for (int j = 0; j < NB4; ++j) *reinterpret_cast<float4*>(Bs + (br + (256 / BTH) * j) * BP + bq) = rb[j];
    };

    f32x16 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const float* arow = As + (wr * 64 + cl) * AP + hi * (KC / 2);
    const float* brow = Bs + (hi * (KC / 2)) * BP + wc * (32 * CT) + cl;
    auto mfma_chunk = [&]() {
#pragma unroll
        for (int s4 = 0; s4 < KC / 8; ++s4) {
            float4 a[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) a[i] = *reinterpret_cast<const float4*>(arow + i * 32 * AP + 4 * s4);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                float b[CT];
#pragma unroll
                for (int j = 0; j < CT; ++j) b[j] = brow[(4 * s4 + kk) * BP + 32 * j];
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const float av = kk == 0 ? a[i].x : (kk == 1 ? a[i].y : (kk == 2 ? a[i].z : a[i].w));
#pragma unroll
                    for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[j], acc[i][j], 0, 0, 0);
                }
            }
        }
    };

    fetch(0);
    stash();
    block_sync_lds();
    for (int k0 = 0; k0 < K; k0 += KC) {
        const bool more = k0 + KC < K;
        if (more) fetch(k0 + KC);           // global loads in flight under the MFMAs
        mfma_chunk();
        block_sync_lds();
        if (more) {
            stash();
            block_sync_lds();
        }
    }
    tile2_epilogue<RT, CT>(acc, ep, C, ldc, L.M, N, m0, n0, wr, wc, hi, cl);
}

// ---- 128-row tile kernel on the bf16 matrix pipe: float32 products from three-way bf16 splits ---------------------------
// v_mfma_f32_32x32x16_bf16 does 16x the multiply-adds per cycle of the f32 MFMA above.  A float x is EXACTLY h + m + l with
// h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (8 + 8 + 8 mantissa bits), and a product of two bf16 is exact in the
// float accumulator, so
//      a b  =  ah bh + (ah bm + am bh) + (am bm + ah bl + al bh)  +  O(2^-25 |a b|)
// -- six bf16 MFMAs per 16-deep step against eight f32 MFMAs of the same duration each: 2.7x the matrix rate, at an error
// below float32's own rounding of the sum (tests/test_emulated_api.py and tests/test_gpu_prims.py measure it against a float64
// product beside the f32 kernel; non-finite inputs give NaN where the f32 kernel gives inf).  B (the weights) is split ONCE by
// gemm_pack_bf16x3 into chunk-major planes [K / 32][3][Npad][32] bf16, so a workgroup's B tile of a chunk is one contiguous
// run per plane; A is split on its way from the staging registers to LDS (22 VALU per float4, under the MFMAs of the chunk
// before).  LDS rows are 32 bf16 + 8 of padding (80 bytes: the 16 lanes of one ds_read_b128 phase hit 64 distinct banks).
constexpr int BF_KC = 32;                       // K chunk: two MFMA steps of 16
constexpr int BF_P = BF_KC;                     // LDS row pitch in bf16: 64 bytes = four 16-byte granules, XOR-swizzled (below)
// LDS layout of a plane: row-major [rows][32 bf16], the 16-byte granule g of row r stored at granule g ^ ((r >> 2) & 3).  The 16
// lanes of one ds_read_b128 service group ({0-3, 12-15, 20-27}, ... of the wave: MI355X_MICROARCH.md, LDS) read one granule of 16
// rows whose (r & 3, (r >> 2) & 3) pairs are all different -> 16 distinct 4-bank slots; a ds_write_b64 / b128 group covers two
// whole rows 16 dwords apart -> the 32 write banks once.  (Rows padded to 80 bytes read conflict-free too but every store group
// hit 4 banks twice: SQ_LDS_BANK_CONFLICT 34.7 M cycles per launch of the 64 -> 64 layer = 72 per wave and chunk, all stores.)
__device__ __forceinline__ int bf_swz(int row) { return (row >> 2) & 3; }

__device__ __forceinline__ void bf16_split3(float4 v, uint2& h, uint2& m, uint2& l) {
    // (sub_f32: single v_sub_f32 -- the compiler pairs adjacent float subtractions into v_pk_add_f32, which costs ~13 cycles more
    //  than two plain ones beside MFMAs: MI355X_MICROARCH.md, "price of one filler")
    h.x = bf16_pack2(v.x, v.y); h.y = bf16_pack2(v.z, v.w);
    const float r0 = sub_f32(v.x, __uint_as_float(h.x << 16)), r1 = sub_f32(v.y, __uint_as_float(h.x & 0xffff0000u));
    const float r2 = sub_f32(v.z, __uint_as_float(h.y << 16)), r3 = sub_f32(v.w, __uint_as_float(h.y & 0xffff0000u));
    m.x = bf16_pack2(r0, r1); m.y = bf16_pack2(r2, r3);
    l.x = bf16_pack2(sub_f32(r0, __uint_as_float(m.x << 16)), sub_f32(r1, __uint_as_float(m.x & 0xffff0000u)));
    l.y = bf16_pack2(sub_f32(r2, __uint_as_float(m.y << 16)), sub_f32(r3, __uint_as_float(m.y & 0xffff0000u)));
}

template <class Loader, int BN>
__global__ void __launch_bounds__(256)
gemm_tile_bf3(Loader L, const u32x4* __restrict__ Bp, int N, int Npad, Epilogue ep, float* __restrict__ C, int64_t ldc, int kper,
              float* __restrict__ partial) {
    constexpr int RT = 2, CT = BN / 64;
    constexpr int NA4 = BF_KC / 8;              // A float4 per thread and chunk
    constexpr int NB = 3 * BN * 4 / 256;        // B uint4 (8 bf16) per thread and chunk
    constexpr int APL = G2_BM * BF_P, BPL = BN * BF_P;      // bf16 per plane
    __shared__ __attribute__((aligned(16))) uint16_t As[3 * APL];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[3 * BPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, cl = lane & 31;
    const int wr = wave & 1, wc = wave >> 1;
    int tbx, tby;
    xcd_tile(tbx, tby);
    const int64_t m0 = (int64_t)tbx * G2_BM;
    const int n0 = tby * BN;
    // split K: blockIdx.z owns [kb, ke) and, when `partial` is set, stores its raw sums to partial[z] (gemm_reduce adds the
    // slices and applies the epilogue)
    const int kb = blockIdx.z * kper;
    const int ke = kb + kper < L.K ? kb + kper : L.K;

    constexpr int ATH = BF_KC / 4, ARS = 256 / ATH;
    const int ar = tid / ATH, aq = (tid % ATH) * 4;
    const int asw = (((aq >> 3) ^ bf_swz(ar)) << 3) + (aq & 4);          // (ARS = 32: every staged row of the thread has ar's swizzle)
    static_assert(ARS % 16 == 0, "staged rows share the swizzle");
    typename Loader::Ctx cx[NA4];
#pragma unroll
    for (int j = 0; j < NA4; ++j) cx[j] = L.prepare(m0 + ar + ARS * j);
    // B item t = tid + 256 j: 16-byte quarter t & 3 of column (t >> 2) % BN of plane t / (4 BN)
    const u32x4* bsrc[NB];
    int bdst[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int t = tid + 256 * j, q = t & 3, col = (t >> 2) % BN, pl = t / (4 * BN);
        bsrc[j] = Bp + ((int64_t)pl * Npad + n0 + col) * 4 + q;
        bdst[j] = pl * BPL + col * BF_P + (q ^ bf_swz(col)) * 8;
    }
    const int64_t bstep = (int64_t)3 * Npad * 4;          // uint4 per chunk

    float4 ra[NA4];
    u32x4 rb[NB];            // (a native vector, not HIP's uint4 struct: the array of structs went through scratch)
    typename Loader::Walk wk = L.walk_begin(kb);
    int64_t bo = (int64_t)(kb / BF_KC) * bstep;
    auto fetch = [&]() {                          // the next chunk, in K order
#pragma unroll
        for (int j = 0; j < NA4; ++j) ra[j] = L.load4w(cx[j], wk, aq);
#pragma unroll
        for (int j = 0; j < NB; ++j) rb[j] = bsrc[j][bo];
        L.walk_next(wk, BF_KC);
        bo += bstep;
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < NA4; ++j) {
            uint2 h, m, l;
            bf16_split3(ra[j], h, m, l);
            uint16_t* d = As + (ar + ARS * j) * BF_P + asw;
            *reinterpret_cast<uint2*>(d) = h;
            *reinterpret_cast<uint2*>(d + APL) = m;
            *reinterpret_cast<uint2*>(d + 2 * APL) = l;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(Bs + bdst[j]) = rb[j];
    };

    f32x16 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the lane's row of the A / B tile (row offsets 32 i, 32 j keep cl's swizzle); granule 2 s + hi of MFMA step s
    const uint16_t* arow = As + (wr * 64 + cl) * BF_P;
    const uint16_t* brow = Bs + (wc * (32 * CT) + cl) * BF_P;
    const int gs[2] = {(hi ^ bf_swz(cl)) * 8, ((2 + hi) ^ bf_swz(cl)) * 8};
    auto mfma_chunk = [&]() {
#pragma unroll
        for (int s = 0; s < BF_KC / 16; ++s) {
            u32x4 a[RT][3], b[CT][3];
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) a[i][p] = *reinterpret_cast<const u32x4*>(arow + p * APL + i * 32 * BF_P + gs[s]);
#pragma unroll
            for (int j = 0; j < CT; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p) b[j][p] = *reinterpret_cast<const u32x4*>(brow + p * BPL + j * 32 * BF_P + gs[s]);
            // smallest terms first; a term's RT x CT MFMAs are independent, so back-to-back issues never wait on an accumulator
            constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int j = 0; j < CT; ++j) acc[i][j] = mfma_bf16_32x32x16(a[i][TA[t]], b[j][TB[t]], acc[i][j]);
        }
    };

    fetch();
    stash();
    block_sync_lds();
    for (int k0 = kb; k0 < ke; k0 += BF_KC) {
        const bool more = k0 + BF_KC < ke;
        if (more) fetch();
        mfma_chunk();
        block_sync_lds();
        if (more) {
            stash();
            block_sync_lds();
        }
    }
    if (partial) {
        tile2_epilogue<RT, CT>(acc, Epilogue{}, partial + (int64_t)blockIdx.z * L.M * N, N, L.M, N, m0, n0, wr, wc, hi, cl);
        return;
    }
    tile2_epilogue<RT, CT>(acc, ep, C, ldc, L.M, N, m0, n0, wr, wc, hi, cl);
}

// ---- 3 x 3 / stride 1 / pad 1 convolution on the bf16x3 path, the input WINDOW staged once per channel chunk --------------------
// gemm_tile_bf3 stages a 128-row A tile per (tap, 32 channels): every input value is loaded, split and stored to LDS once per tap
// that uses it -- 9 times.  With stride 1 and pad 1 output row m (flattened (b, oy, ox)) reads the input pixels
// m + (ky - 1) W + (kx - 1): the 9 taps of 128 consecutive rows lie in THREE runs of 130 consecutive pixels.  Here a workgroup stages
// those 3 x 130 pixels of one 16-channel chunk once (a third of the loads, splits and LDS stores per MFMA), and the 9 taps read them
// at shifted pixel offsets; the weights of a (tap, chunk) stream through a double-buffered LDS tile, one barrier per tap.  What the
// zero padding removes (image borders; the flattened runs wrap into the neighbouring image row there) is read from a ZERO pixel of
// the window instead: one address select per lane, 32-row block and tap.
// LDS: pixels / weight columns are 32 bytes (16 bf16) apart, the 16-byte granule g of pixel p stored at g ^ ((p >> 3) & 1): the 16
// lanes of a ds_read_b128 service group read pixels {x .. x+3, x+12 .. x+15, x+20 .. x+27} -> 16 distinct slots for every shift x.
constexpr int W3_KC = 16;                       // channels per chunk = one MFMA step
constexpr int W3_PX = G2_BM + 2;                // window pixels per tap row
constexpr int W3_PP = 132;                      // pixel pitch of a tap row in LDS
struct Conv3Args { const float* in; int H, W, C; int64_t M; };

template <int BN>
__global__ void __launch_bounds__(256)
conv3x3s1_bf3(Conv3Args A, const u32x4* __restrict__ Bp, int N, int Npad, Epilogue ep, float* __restrict__ C, int64_t ldc) {
    constexpr int RT = 2, CT = BN / 64;
    constexpr int KYS = W3_PP * W3_KC;          // bf16 per tap row
    constexpr int APL = 3 * KYS;                // bf16 per plane of the window
    constexpr int BPL = BN * W3_KC;             // bf16 per plane of a weight tile
    constexpr int BBUF = 3 * BPL;
    constexpr int NAI = (3 * W3_PX * 4 + 255) / 256;     // window float4 per thread (7; the last pass partly filled)
    constexpr int NBT = 6 * BN;                          // weight u32x4 per (tap, chunk) tile
    constexpr int NBI = (NBT + 255) / 256;
    __shared__ __attribute__((aligned(16))) uint16_t Aw[3 * APL];
    __shared__ __attribute__((aligned(16))) uint16_t Bw[2 * BBUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, cl = lane & 31;
    const int wr = wave & 1, wc = wave >> 1;
    int tbx, tby;
    xcd_tile(tbx, tby);
    const int64_t m0 = (int64_t)tbx * G2_BM;
    const int n0 = tby * BN;

    // ---- window staging slots of this thread: item = (pixel of the 3 x 130 window, float4 of its 16 channels)
    int goff[NAI], ldst[NAI];
#pragma unroll
    for (int j = 0; j < NAI; ++j) {
        const int item = tid + 256 * j;
        const int wpx = item >> 2, q = item & 3;
        const int ky = wpx / W3_PX, wp = wpx - ky * W3_PX;
        const int64_t gp = m0 - 1 + wp + (int64_t)(ky - 1) * A.W;
        goff[j] = (item < 3 * W3_PX * 4 && gp >= 0 && gp < A.M) ? (int)gp * A.C + q * 4 : -1;
        ldst[j] = (256 * (j + 1) <= 3 * W3_PX * 4 || item < 3 * W3_PX * 4) ? ky * KYS + wp * W3_KC + ((((q >> 1) ^ ((wp >> 3) & 1))) << 3) + (q & 1) * 4 : -1;
    }
    const u32x4* bsrc[NBI];
    int bdst[NBI];
#pragma unroll
    for (int j = 0; j < NBI; ++j) {
        const int t = tid + 256 * j;
        const int g = t & 1, col = (t >> 1) % BN, pl = (t / (2 * BN)) % 3;
        bsrc[j] = Bp + ((int64_t)pl * Npad + n0 + col) * 4 + g;
        bdst[j] = (256 * (j + 1) <= NBT || t < NBT) ? pl * BPL + col * W3_KC + ((g ^ ((col >> 3) & 1)) << 3) : -1;
    }
    const int64_t bstep = (int64_t)3 * Npad * 4;          // u32x4 per 32-deep chunk of the packed weights

    // ---- the wave's rows: taps the zero padding removes
    unsigned taps[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int64_t m = m0 + wr * 64 + i * 32 + cl;
        taps[i] = 0x1ffu;                  // (rows past M: nothing of theirs is stored)
        if (m < A.M) {
            const unsigned mu = (unsigned)m, t = mu / (unsigned)A.W;
            const int ox = (int)(mu - t * (unsigned)A.W), oy = (int)(t % (unsigned)A.H);
            taps[i] = 0u;
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                    if (oy + ky - 1 >= 0 && oy + ky - 1 < A.H && ox + kx - 1 >= 0 && ox + kx - 1 < A.W) taps[i] |= 1u << (ky * 3 + kx);
        }
    }
    // the zero pixel: pixel W3_PP - 1 of each of the 9 (plane, tap row) runs
    if (tid < 9 * 2) *reinterpret_cast<u32x4*>(Aw + (tid >> 1) * KYS + (W3_PP - 1) * W3_KC + (tid & 1) * 8) = u32x4{0u, 0u, 0u, 0u};
    const int zrow = (W3_PP - 1) * W3_KC + hi * 8;

    float4 ra[NAI];
    u32x4 rb[NBI];
    auto fetch_a = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NAI; ++j)
            ra[j] = goff[j] >= 0 ? *reinterpret_cast<const float4*>(A.in + (goff[j] + c0)) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto stash_a = [&]() {
#pragma unroll
        for (int j = 0; j < NAI; ++j) {
            if (256 * (j + 1) > 3 * W3_PX * 4 && ldst[j] < 0) continue;
            uint2 h, m, l;
            bf16_split3(ra[j], h, m, l);
            uint16_t* d = Aw + ldst[j];
            *reinterpret_cast<uint2*>(d) = h;
            *reinterpret_cast<uint2*>(d + APL) = m;
            *reinterpret_cast<uint2*>(d + 2 * APL) = l;
        }
    };
    auto fetch_b = [&](int kk) {                          // kk = tap * C + c0: first of the 16 k of the tile
        const int64_t o = (int64_t)(kk >> 5) * bstep + ((kk >> 4) & 1) * 2;
#pragma unroll
        for (int j = 0; j < NBI; ++j)
            if (256 * (j + 1) <= NBT || bdst[j] >= 0) rb[j] = bsrc[j][o];
    };
    auto stash_b = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NBI; ++j)
            if (256 * (j + 1) <= NBT || bdst[j] >= 0) *reinterpret_cast<u32x4*>(Bw + buf * BBUF + bdst[j]) = rb[j];
    };

    f32x16 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the lane's window pixel for kx = 0 (row r of the tile reads window pixel r + kx) and its weight column, bf16 offsets
    int arow[RT][3], brow[CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int wp = wr * 64 + i * 32 + cl + kx;
            arow[i][kx] = wp * W3_KC + ((hi ^ ((wp >> 3) & 1)) << 3);
        }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int c = wc * (32 * CT) + j * 32 + cl;
        brow[j] = c * W3_KC + ((hi ^ ((c >> 3) & 1)) << 3);
    }

    // Schedule per 16-channel chunk: window -> LDS, barrier, request the next chunk's window (lands under the nine taps); per tap:
    // request the next tap's weights, multiply out of weight buffer tap & 1, store the requested weights to the other buffer, one
    // barrier.  (Requesting the weights TWO taps ahead into a second register set measured the same: profiles/r05_conv_window_ab.log.)
    const int nc = A.C / W3_KC;
    fetch_a(0);
    fetch_b(0);
    for (int ci = 0; ci < nc; ++ci) {
        const int c0 = ci * W3_KC;
        stash_a();
        stash_b(0);
        block_sync_lds();
        if (ci + 1 < nc) fetch_a(c0 + W3_KC);
        auto tap_step = [&](auto tap_c) {                  // (one instantiation per tap: tap, ky, kx are constants)
            constexpr int tap = decltype(tap_c)::value;
            constexpr int ky = tap / 3, kx = tap - 3 * ky;
            const bool last = tap == 8 && ci + 1 == nc;
            if (!last) fetch_b(tap < 8 ? (tap + 1) * A.C + c0 : c0 + W3_KC);
            // rows that lose this tap to the zero padding read the window's ZERO pixel instead (pixel 131 of every tap row: never
            // staged, cleared once): one address select per 32-row block and tap, no branch around the MFMAs
            u32x4 a[RT][3], b[CT][3];
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const int ar = (tap == 4 || ((taps[i] >> tap) & 1u)) ? arow[i][kx] : zrow;
#pragma unroll
                for (int p = 0; p < 3; ++p) a[i][p] = *reinterpret_cast<const u32x4*>(Aw + p * APL + ky * KYS + ar);
            }
#pragma unroll
            for (int j = 0; j < CT; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p) b[j][p] = *reinterpret_cast<const u32x4*>(Bw + (tap & 1) * BBUF + p * BPL + brow[j]);
            constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int j = 0; j < CT; ++j) acc[i][j] = mfma_bf16_32x32x16(a[i][TA[t]], b[j][TB[t]], acc[i][j]);
            if (tap < 8) stash_b((tap + 1) & 1);           // the buffer tap - 1 read: every wave is past that barrier
            block_sync_lds();
        };
        tap_step(std::integral_constant<int, 0>{}); tap_step(std::integral_constant<int, 1>{}); tap_step(std::integral_constant<int, 2>{});
        tap_step(std::integral_constant<int, 3>{}); tap_step(std::integral_constant<int, 4>{}); tap_step(std::integral_constant<int, 5>{});
        tap_step(std::integral_constant<int, 6>{}); tap_step(std::integral_constant<int, 7>{}); tap_step(std::integral_constant<int, 8>{});
    }
    tile2_epilogue<RT, CT>(acc, ep, C, ldc, A.M, N, m0, n0, wr, wc, hi, cl);
}

// B [K, N] float (row-major) -> chunk-major bf16 planes [K / 32][3][Npad][32]; columns N .. Npad - 1 are zero
__global__ void gemm_pack_bf16x3_kernel(const float* __restrict__ Bm, int K, int N, int Npad, uint16_t* __restrict__ out) {
    const int64_t total = (int64_t)K * Npad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i % Npad), k = (int)(i / Npad);
        const float x = n < N ? Bm[(int64_t)k * N + n] : 0.f;
        const uint32_t h = bf16_pack2(x, 0.f) & 0xffffu;
        const float r = x - __uint_as_float(h << 16);
        const uint32_t m = bf16_pack2(r, 0.f) & 0xffffu;
        const uint32_t l = bf16_pack2(r - __uint_as_float(m << 16), 0.f) & 0xffffu;
        const int64_t base = ((int64_t)(k / BF_KC) * 3 * Npad + n) * BF_KC + (k % BF_KC);
        out[base] = (uint16_t)h;
        out[base + (int64_t)Npad * BF_KC] = (uint16_t)m;
        out[base + (int64_t)2 * Npad * BF_KC] = (uint16_t)l;
    }
}

__global__ void gemm_reduce(const float* __restrict__ partial, int splits, int64_t M, int N, Epilogue ep,
                            float* __restrict__ C, int64_t ldc) {
    const int64_t total = M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        // (32-bit index arithmetic whenever it fits: a 64-bit i / N is a ~100-instruction software division in front of `splits` loads)
        int64_t m;
        if (total < 0x7fffffffll) m = (int64_t)((unsigned)i / (unsigned)N); else m = i / N;
        const int col = (int)(i - m * N);
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += partial[(int64_t)z * total + i];
        if (ep.ps > 0) {
            const PsCol pc = ps_col(col, ep);
            if (ep.bias) v += ep.bias[pc.co];
            C[ps_offset(m, pc, ep, ldc)] = gm_act(v, ep.act, ep.slope);
            continue;
        }
        // (the tile kernels' rule and order: bias, then bias2, each if set)
        float b = ep.bias ? ep.bias[col] : 0.f;
        if (ep.bias2) b += ep.bias2[col];
        const int64_t rg_base = ep.res_gather ? (m < ep.rg_rows_per_item ? 0 : m / ep.rg_rows_per_item) * ep.rg_src_rows_per_item : 0;
        C[m * ldc + col] = gm_act(add_residual(v + b, ep, m, col, rg_base, 0), ep.act, ep.slope);
    }
}

// ---- host side ---------------------------------------------------------------------------------------
// Split-K.  A workgroup walks its K chunks serially at ~2-4 us per chunk (global latency of one prefetch stage), so a deep-K
// problem with about one workgroup per CU is latency-bound however few flops it has -- measured (KPConv, one MI355X): M = 4.6k,
// K = 1920, N = 128 as 288 workgroups took 257 us = 9 TFLOP/s.  Problems with K >= 512 are split until ~4 workgroups per CU are
// resident (partials summed by gemm_reduce).
static int pick_splits(int64_t M, int N, int K) {
    const int64_t tiles = ((M + GM_BM - 1) / GM_BM) * ((N + GM_BN - 1) / GM_BN);
    // (K in [512, 768) -- RandLA's decoder and 512-wide Linears -- keeps round 1's numbers: measured 0.4 % faster there)
    const int64_t thr = K >= 768 ? 1024 : 256;
    const int64_t aim = K >= 768 ? 1024 : 512;
    if (tiles >= thr || K < 512 || tiles <= 0) return 1;    // (tiles == 0: an empty problem, sized before it is refused)
    int64_t want = (aim + tiles - 1) / tiles;
    int64_t maxs = K / 128;                              // at least 4 chunks per split
    int64_t s = want < maxs ? want : maxs;
    if (s > 32) s = 32;
    return s < 1 ? 1 : (int)s;
}

size_t gemm_partial_bytes(int64_t M, int N, int K) {
    int s = pick_splits(M, N, K);
    return s > 1 ? sizeof(float) * (size_t)s * (size_t)M * (size_t)N : 0;
}

// The register-blocked kernel takes the problems it is built for: no split-K, float4-addressable operands, no gathered
// residual, and enough 128-row tiles to fill the 256 CUs -- medium problems (the 62 x 54 and 31 x 27 maps of SECOND's deeper
// blocks at 8 sweeps) fill the chip better with the 64 x 64 tiles of gemm_tile.  Returns the column-tile width to use, 0 = no.
static int big_bn(int64_t M, int N, int K, const float* Bm, const Epilogue& ep) {
    // workgroups below which gemm_tile keeps the problem.  A constant in the product library (no environment reads, no process-wide
    // state: SURVEY.md §8b); only the HOST EMULATOR build of the tests (-DML3D_TEST_HOOKS, tests/hipemu/build_emu.sh) reads
    // ML3D_GEMM_BIG_MIN_TILES, once, so that its suites can push small problems (of any depth) through this kernel.  Shallow K
    // (RandLA's per-point Linears, K = 32 .. 128: one or two chunks, nothing to pipeline) stays on gemm_tile.
#ifdef ML3D_TEST_HOOKS
    static const int64_t min_tiles = [] { const char* e = getenv("ML3D_GEMM_BIG_MIN_TILES"); return e ? (int64_t)atoll(e) : (int64_t)256; }();
#else
    constexpr int64_t min_tiles = 256;
#endif
    const int min_k = min_tiles <= 1 ? 0 : 256;
    if ((N & 3) || (K % GM_KC) != 0 || K < min_k || (((uintptr_t)Bm) & 15) != 0 || ep.res_gather) return 0;
    const int64_t rows = (M + G2_BM - 1) / G2_BM;
    if (N > 64 && rows * ((N + 127) / 128) >= 2 * min_tiles) return 128;
    if (rows * ((N + 63) / 64) >= min_tiles) return (N > 64 && rows * ((N + 127) / 128) >= min_tiles) ? 128 : 64;
    return 0;
}

// sum the split-K partials and apply the epilogue (the f32 and the bf16x3 path)
static int launch_reduce(const float* partial, int splits, int64_t M, int N, const Epilogue& ep, float* C, int64_t ldc,
                         hipStream_t st) {
    const int64_t total = M * N;
    const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(gemm_reduce, dim3(nb), dim3(256), 0, st, partial, splits, M, N, ep, C, ldc);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

template <class L2>
static void launch_big(const L2& L, const float* Bm, int N, int bn, int kc, const Epilogue& ep, float* C, int64_t ldc,
                       hipStream_t st) {
    const unsigned gm = (unsigned)((L.M + G2_BM - 1) / G2_BM);
    if (bn == 128) {
        const dim3 g(gm, (unsigned)((N + 127) / 128));
        if (kc == 64) hipLaunchKernelGGL((gemm_tile2<L2, 128, 64>), g, dim3(256), 0, st, L, Bm, N, ep, C, ldc);
        else hipLaunchKernelGGL((gemm_tile2<L2, 128, 32>), g, dim3(256), 0, st, L, Bm, N, ep, C, ldc);
    } else {
        const dim3 g(gm, (unsigned)((N + 63) / 64));
        if (kc == 64) hipLaunchKernelGGL((gemm_tile2<L2, 64, 64>), g, dim3(256), 0, st, L, Bm, N, ep, C, ldc);
        else hipLaunchKernelGGL((gemm_tile2<L2, 64, 32>), g, dim3(256), 0, st, L, Bm, N, ep, C, ldc);
    }
}

// K chunk: 64 for the 128-column tiles when the operands allow it (half the barriers per MFMA, twice the matrix time to
// hide the next chunk's global loads under: SECOND's 128- and 256-channel convs), 32 for the 64-column tiles (measured:
// 3x3 64 -> 64 conv 0.328 ms at 32 vs 0.362 ms at 64).
static int big_kc(int K, int c_or_zero, int bn) {
    const bool ok64 = (K % 64) == 0 && (c_or_zero == 0 || (c_or_zero % 64) == 0);
    return (ok64 && bn == 128) ? 64 : 32;
}

static bool gemm_launch_big(const ConvLoader& L, const float* Bm, int N, const Epilogue& ep, float* C, int64_t ldc,
                            hipStream_t st) {
    const ConvA& A = L.A;
    const int bn = big_bn(L.M, N, L.K, Bm, ep);
    if (!bn || (A.C % GM_KC) != 0 || A.KH * A.KW > 32 ||
        (int64_t)A.B * A.H * A.W * A.C >= 0x7fffffffll - (int64_t)(A.pad + 1) * (A.W + 1) * A.C)
        return false;
    ConvLoader2 L2;
    L2.A = A; L2.M = L.M; L2.K = L.K;
    launch_big(L2, Bm, N, bn, big_kc(L.K, A.C, bn), ep, C, ldc, st);
    return true;
}

// Row-major (Linear) problems stay on gemm_tile: measured on all three workloads (profiles/r02_gemm_ab.log, again in round 3) the
// 128-row kernel LOSES there -- RandLA 5657 vs 5787 frames/s, KPConv 2753 vs 2796 spheres/s, PointPillars 1137 vs 1165 frames/s:
// the Linears have K <= 1024 with an A operand that is read once (no 9-tap reuse out of L2 as in the convolutions), so the deeper
// register block buys nothing and its lower occupancy costs.
static bool gemm_launch_big(const RowsLoader&, const float*, int, const Epilogue&, float*, int64_t, hipStream_t) { return false; }

// Chunks in flight per workgroup of gemm_tile.  Two chunks cost 32 more registers (66 -> 98: four waves per SIMD instead of
// seven): they pay where the kernel lasts as long as ONE workgroup's serial walk over K -- the small-M / deep-K problems that
// fit the chip in a round or two (KPConv's coarse layers: +2.5 % spheres/s) -- and lose where many rounds of workgroups hide
// each other's latency anyway (RandLA's and PointPillars' 10^5 .. 10^6-row Linears: -1 %), measured in one call on one box
// (gpurun_out/r3k).  Rule: two chunks up to 12 288 workgroups (KPConv's 2 200-row-tile layer included, RandLA's / PointPillars'
// 13 000+-tile Linears not).
static int gemm_depth(const dim3& grid) { return (long long)grid.x * grid.y * grid.z <= 12288ll ? 2 : 1; }

// the streamlined K loop of gemm_tile takes: one dense float4-addressable row block, whole chunks, float4-addressable B
static bool plain_rows(const RowsLoader& L, int kper, int bvec) {
    const bool one = L.A.k2 == 0 && L.A.k1 == L.K;
    const bool two = L.A.k2 > 0 && L.A.a2 && (L.A.k1 % GM_KC) == 0 && L.A.k1 + L.A.k2 == L.K;
    return L.vec && bvec && !L.A.gather && (one || two) && (L.K % GM_KC) == 0 && (kper % GM_KC) == 0 && L.M > 0;
}
static bool plain_rows(const ConvLoader&, int, int) { return false; }
static void launch_plain(const RowsLoader& L, dim3 grid, const float* Bm, int N, int bvec, const Epilogue& ep, float* C,
                         int64_t ldc, int kper, float* partial, hipStream_t st) {
    if (gemm_depth(grid) == 1) hipLaunchKernelGGL((gemm_tile<RowsLoader, true, 1>), grid, dim3(256), 0, st, L, Bm, N, bvec, ep, C, ldc, kper, partial);
    else hipLaunchKernelGGL((gemm_tile<RowsLoader, true, 2>), grid, dim3(256), 0, st, L, Bm, N, bvec, ep, C, ldc, kper, partial);
}
static void launch_plain(const ConvLoader&, dim3, const float*, int, int, const Epilogue&, float*, int64_t, int, float*,
                         hipStream_t) {}

template <class Loader>
static int gemm_launch(const Loader& L, const float* Bm, int N, const Epilogue& ep, float* C, int64_t ldc,
                       void* partial_ws, size_t partial_bytes, hipStream_t st) {
    const int64_t M = L.M;
    const int K = L.K;
    if (M <= 0 || N <= 0) return 0;
    if (K <= 0 || !Bm || !C) return ML3D_E_INVALID;
    int splits = pick_splits(M, N, K);
    if (splits > 1 && (!partial_ws || partial_bytes < sizeof(float) * (size_t)splits * (size_t)M * (size_t)N)) splits = 1;
    if (splits == 1 && gemm_launch_big(L, Bm, N, ep, C, ldc, st)) return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
    // split boundaries are multiples of the K chunk (so also of 4: float4 loads never straddle one)
    int kper = ((K + splits - 1) / splits + GM_KC - 1) / GM_KC * GM_KC;
    splits = (K + kper - 1) / kper;
    const int bvec = ((N & 3) == 0 && (((uintptr_t)Bm) & 15) == 0) ? 1 : 0;
    dim3 grid((unsigned)((M + GM_BM - 1) / GM_BM), (unsigned)((N + GM_BN - 1) / GM_BN), (unsigned)splits);
    float* partial = splits > 1 ? (float*)partial_ws : nullptr;
    if (plain_rows(L, kper, bvec)) launch_plain(L, grid, Bm, N, bvec, ep, C, ldc, kper, partial, st);
    else if (gemm_depth(grid) == 1) hipLaunchKernelGGL((gemm_tile<Loader, false, 1>), grid, dim3(256), 0, st, L, Bm, N, bvec, ep, C, ldc, kper, partial);
    else hipLaunchKernelGGL((gemm_tile<Loader, false, 2>), grid, dim3(256), 0, st, L, Bm, N, bvec, ep, C, ldc, kper, partial);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    return splits > 1 ? launch_reduce(partial, splits, M, N, ep, C, ldc, st) : 0;
}

// ---- bf16x3 convolution ------------------------------------------------------------------------------------------------
static int bf3_npad(int N) { return (N + 127) / 128 * 128; }

size_t gemm_pack_bf16x3_bytes(int K, int N) {
    if (K <= 0 || N <= 0 || (K % BF_KC) != 0) return 0;
    return (size_t)3 * (size_t)bf3_npad(N) * (size_t)K * sizeof(uint16_t);
}

int gemm_pack_bf16x3(const float* Bm, int K, int N, void* packed, hipStream_t st) {
    if (!Bm || !packed || K <= 0 || N <= 0 || (K % BF_KC) != 0 || (((uintptr_t)packed) & 15) != 0) return ML3D_E_INVALID;
    const int Npad = bf3_npad(N);
    const int64_t total = (int64_t)K * Npad;
    const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(gemm_pack_bf16x3_kernel, dim3(nb), dim3(256), 0, st, Bm, K, N, Npad, (uint16_t*)packed);
    return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
}

// the convolutions the bf16x3 kernel takes: whole 32-deep chunks inside one tap, 32-bit image offsets, at most 32 taps.
// Every eligible problem runs there whatever its size (a 128-row tile per workgroup; narrow outputs take 64-column tiles).
bool gemm_conv_bf16x3_ok(const ConvA& A) {
    const int64_t M = (int64_t)A.B * A.OH * A.OW;
    return A.in && (A.C % BF_KC) == 0 && A.KH * A.KW <= 32 && M < 0x7fffffffll &&
           (int64_t)A.B * A.H * A.W * A.C < 0x7fffffffll - (int64_t)(A.pad + 1) * (A.W + 1) * A.C;
}

// split-K of the dense-row problems: with fewer 128-row tiles than workgroup slots (2 per CU) and a deep K, K is cut so that ~1.5
// rounds of workgroups are in flight, at least 4 chunks per slice (KPConv's contractions at the coarse layers: M = 2 400 .. 35 000
// rows, K = 15 Cin = 1 920 .. 7 680)
static int bf3_splits(int64_t M, int N, int K) {
    const int64_t tiles = ((M + G2_BM - 1) / G2_BM) * (N > 64 ? (N + 127) / 128 : 1);
    const int64_t slots = 256 * (N > 64 ? 2 : 4);          // resident workgroups: LDS 49 KB / 37 KB, 174 / 116 registers
    if (K < 512 || tiles >= 3 * slots) return 1;
    if (tiles >= 512) {
        // one to three rounds of workgroups: a last round that is mostly empty costs as much as a full one (1 101 tiles on 1 024
        // slots = 2 rounds).  Cut K into s <= 4 slices where that shortens the schedule: cost = rounds(s) / s + the reduce pass
        int best = 1;
        double best_cost = (double)((tiles + slots - 1) / slots);
        for (int c = 2; c <= 4 && c <= K / 128; ++c) {
            const double cost = (double)((tiles * c + slots - 1) / slots) / c + 0.1;
            if (cost < best_cost - 1e-9) { best_cost = cost; best = c; }
        }
        return best;
    }
    int64_t s = (768 + tiles - 1) / tiles;
    if (s > K / 128) s = K / 128;
    if (s > 32) s = 32;
    return s < 1 ? 1 : (int)s;
}

// The one launch of gemm_tile_bf3: 128-row tiles, 128- or 64-column tiles by N, K cut into `splits` slices of whole chunks whose
// partials (partial_ws: splits * M * N floats) gemm_reduce sums; splits == 1 applies the epilogue in the kernel
template <class Loader>
static int launch_bf3(const Loader& L, const void* packed, int N, const Epilogue& ep, float* C, int64_t ldc, int splits,
                      void* partial_ws, hipStream_t st) {
    const int kper = ((L.K + splits - 1) / splits + BF_KC - 1) / BF_KC * BF_KC;
    splits = (L.K + kper - 1) / kper;
    float* partial = splits > 1 ? (float*)partial_ws : nullptr;
    const int bn = N > 64 ? 128 : 64;
    const dim3 grid((unsigned)((L.M + G2_BM - 1) / G2_BM), (unsigned)((N + bn - 1) / bn), (unsigned)splits);
    hipLaunchKernelGGL((N > 64 ? gemm_tile_bf3<Loader, 128> : gemm_tile_bf3<Loader, 64>), grid, dim3(256), 0, st, L,
                       (const u32x4*)packed, N, bf3_npad(N), ep, C, ldc, kper, partial);
    if (hipGetLastError() != hipSuccess) return ML3D_E_LAUNCH;
    return splits > 1 ? launch_reduce(partial, splits, L.M, N, ep, C, ldc, st) : 0;
}

size_t gemm_partial_bytes_bf16x3(int64_t M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int s = bf3_splits(M, N, K);
    return s > 1 ? sizeof(float) * (size_t)s * (size_t)M * (size_t)N : 0;
}

// dense rows: Linears, KPConv's contraction over (kernel point, channel), the transposed convolutions of PointPillars
// (kernel == stride: a GEMM + pixel-shuffle store)
int gemm_rows_bf16x3(const float* a, int64_t lda, int k1, const float* a2, int64_t lda2, int k2, int64_t M, const void* packed,
                     int N, const Epilogue& ep, float* C, int64_t ldc, void* partial_ws, size_t partial_bytes, hipStream_t st) {
    const int K = k1 + k2;
    if (!a || !packed || !C || N <= 0 || k1 <= 0 || k2 < 0 || (k2 > 0 && !a2) || M < 0) return ML3D_E_INVALID;
    if ((ep.res_gather && ep.rg_rows_per_item < G2_BM) || (K % BF_KC) != 0 || (k1 % BF_KC) != 0 || (lda & 3) != 0 || (((uintptr_t)a) & 15) != 0 ||
        (k2 > 0 && ((lda2 & 3) != 0 || (((uintptr_t)a2) & 15) != 0)))
        return ML3D_E_UNSUPPORTED;
    if (M == 0) return 0;
    RowsLoader2 L;
    L.a = a; L.lda = lda; L.a2 = k2 > 0 ? a2 : nullptr; L.lda2 = lda2; L.k1 = k1; L.M = M; L.K = K;
    int splits = bf3_splits(M, N, K);
    if (splits > 1 && (!partial_ws || partial_bytes < sizeof(float) * (size_t)splits * (size_t)M * (size_t)N)) splits = 1;
    return launch_bf3(L, packed, N, ep, C, ldc, splits, partial_ws, st);
}

int gemm_conv_bf16x3(const ConvA& A, const void* packed, int N, const Epilogue& ep, float* C, int64_t ldc, hipStream_t st) {
    if (!gemm_conv_bf16x3_ok(A) || !packed || !C || N <= 0 || ep.res_gather) return ML3D_E_INVALID;
    ConvLoader2 L2;
    L2.A = A; L2.M = (int64_t)A.B * A.OH * A.OW; L2.K = A.KH * A.KW * A.C;
    if (L2.M <= 0) return 0;
    // 3 x 3 / stride 1 / pad 1 (13 of SECOND's 16 convolutions): the window-staged kernel.  (Only the HOST EMULATOR build of the tests
    // reads ML3D_CONV_WINDOW, once, so that its suites can push these shapes through the general kernel as well.)
#ifdef ML3D_TEST_HOOKS
    static const bool window = [] { const char* e = getenv("ML3D_CONV_WINDOW"); return !e || atoi(e) != 0; }();
#else
    constexpr bool window = true;
#endif
    if (window && A.KH == 3 && A.KW == 3 && A.stride == 1 && A.pad == 1 && A.OH == A.H && A.OW == A.W &&
        (int64_t)A.B * A.H * A.W * A.C < 0x7fffffffll) {
        const Conv3Args a3 = {A.in, A.H, A.W, A.C, L2.M};
        const int bn = N > 64 ? 128 : 64;
        const dim3 grid((unsigned)((L2.M + G2_BM - 1) / G2_BM), (unsigned)((N + bn - 1) / bn));
        hipLaunchKernelGGL((N > 64 ? conv3x3s1_bf3<128> : conv3x3s1_bf3<64>), grid, dim3(256), 0, st, a3, (const u32x4*)packed, N,
                           bf3_npad(N), ep, C, ldc);
        return hipGetLastError() == hipSuccess ? 0 : ML3D_E_LAUNCH;
    }
    return launch_bf3(L2, packed, N, ep, C, ldc, 1, nullptr, st);
}

// 3 x 3 x 3 / stride 1 / pad 1 on a channels-last volume (gemm.h): the general bf16x3 tile kernel behind Conv3dLoader
bool gemm_conv3d_bf16x3_ok(const Conv3dA& A) {
    if (!A.in || A.B <= 0 || A.D <= 0 || A.H <= 0 || A.W <= 0 || A.C <= 0 || (A.C % BF_KC) != 0 || (((uintptr_t)A.in) & 15) != 0) return false;
    const int64_t M = (int64_t)A.B * A.D * A.H * A.W;
    // 32-bit element offsets, the corner one voxel outside on every axis included
    return M < 0x7fffffffll && M * A.C < 0x7fffffffll - ((int64_t)A.H * A.W + A.W + 1) * A.C;
}

int gemm_conv3d_bf16x3(const Conv3dA& A, const void* packed, int N, const Epilogue& ep, float* C, int64_t ldc, hipStream_t st) {
    if (!gemm_conv3d_bf16x3_ok(A) || !packed || !C || N <= 0 || ep.res_gather || ep.ps) return ML3D_E_INVALID;
    Conv3dLoader L;
    L.A = A; L.M = (int64_t)A.B * A.D * A.H * A.W; L.K = 27 * A.C;
    return launch_bf3(L, packed, N, ep, C, ldc, 1, nullptr, st);
}

// sparse convolution by rulebook (gemm.h): the general bf16x3 tile kernel behind SparseConvLoader
int gemm_sparse_conv_bf16x3(const SparseConvA& A, int64_t M, const void* packed, int N, const Epilogue& ep, float* C, int64_t ldc,
                            hipStream_t st) {
    if (!A.in || !A.rule || !packed || !C || N <= 0 || M < 0 || A.taps <= 0 || A.taps > 64 || A.cp <= 0 || A.k2 < 0 ||
        (A.k2 > 0 && !A.a2) || A.in_rows < 0 || A.in_rows > 0x7fffffffll || ep.res_gather || ep.ps)
        return ML3D_E_INVALID;
    if ((A.cp % BF_KC) != 0 || (A.k2 % BF_KC) != 0 || A.ldi < A.cp || (A.ldi & 3) != 0 || (((uintptr_t)A.in) & 15) != 0 ||
        (A.k2 > 0 && (A.lda2 < A.k2 || (A.lda2 & 3) != 0 || (((uintptr_t)A.a2) & 15) != 0)))
        return ML3D_E_UNSUPPORTED;
    if (M == 0) return 0;
    SparseConvLoader L;
    L.A = A; L.M = M; L.K = A.taps * A.cp + A.k2;
    if (A.k2 == 0) L.A.a2 = nullptr;
    return launch_bf3(L, packed, N, ep, C, ldc, 1, nullptr, st);
}

int gemm_rows(const RowsA& A, const float* Bm, int64_t M, int N, int K, const Epilogue& ep, float* C, int64_t ldc,
              void* partial_ws, size_t partial_bytes, hipStream_t stream) {
    if (A.k1 + A.k2 != K || (A.k1 > 0 && !A.a) || (A.k2 > 0 && !A.a2)) return ML3D_E_INVALID;
    RowsLoader L;
    L.A = A; L.M = M; L.K = K;
    bool v = (A.k1 & 3) == 0 && (A.lda & 3) == 0 && (((uintptr_t)A.a) & 15) == 0;
    if (A.k2 > 0) v = v && (A.k2 & 3) == 0 && (A.lda2 & 3) == 0 && (((uintptr_t)A.a2) & 15) == 0;
    L.vec = v ? 1 : 0;
    return gemm_launch(L, Bm, N, ep, C, ldc, partial_ws, partial_bytes, stream);
}

// (A cut of the batch at the last full round of tiles -- the tail images on the 64 x 64 kernel -- was measured in round 3 and
//  was slower: 0.672 / 0.639 against 0.628 / 0.623 ms for SECOND's 3x3 64 -> 64 at 16 sweeps; PointPillars' two lanes fill the
//  partly filled last rounds instead, ml3d/engine.py.)
int gemm_conv(const ConvA& A, const float* Bm, int N, const Epilogue& ep, float* C, int64_t ldc, void* partial_ws,
              size_t partial_bytes, hipStream_t stream) {
    if (!A.in || (A.C & 3) || A.KH <= 0 || A.KW <= 0 || A.stride <= 0) return ML3D_E_INVALID;
    ConvLoader L;
    L.A = A;
    L.M = (int64_t)A.B * A.OH * A.OW;
    L.K = A.KH * A.KW * A.C;
    L.chunk_uniform = (A.C % GM_KC) == 0 ? 1 : 0;
    return gemm_launch(L, Bm, N, ep, C, ldc, partial_ws, partial_bytes, stream);
}

}  // namespace ml3d
