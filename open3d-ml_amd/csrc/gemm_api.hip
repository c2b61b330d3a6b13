// gemm_api.hip — the C entry points of the shared GEMM that belong to no model (include/ml3d_hip.h): packing a weight matrix
// for the bf16x3 kernels and the Linears on the f32 and the bf16x3 path.  Every model's forward calls them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "grid.h"
#include "ml3d_hip.h"

using namespace ml3d;

extern "C" size_t ml3d_gemm_pack_bf16x3_bytes(int k, int n) { return gemm_pack_bf16x3_bytes(k, n); }

extern "C" int ml3d_gemm_pack_bf16x3(const float* weights, int k, int n, void* packed, size_t packed_bytes, void* stream) {
    if (!weights || !packed || k <= 0 || n <= 0) return ML3D_E_INVALID;
    if (k % 32) return ML3D_E_UNSUPPORTED;
    if (packed_bytes < gemm_pack_bf16x3_bytes(k, n)) return ML3D_E_WORKSPACE;
    return gemm_pack_bf16x3(weights, k, n, packed, (hipStream_t)stream);
}

extern "C" size_t ml3d_linear_bf16x3_workspace_bytes(int64_t rows, int n, int k) { return gemm_partial_bytes_bf16x3(rows, n, k) + 512; }

extern "C" int ml3d_linear_bf16x3(const float* a, int64_t lda, int k1, const float* a2, int64_t lda2, int k2, int64_t rows,
                                  const void* packed, const float* bias, const float* residual, int64_t ldr, int n, int act,
                                  float slope, float* out, int64_t ldc, void* workspace, size_t workspace_bytes, void* stream) {
    // (zero rows is a no-op before any pointer is looked at, as in ml3d_linear: an empty tensor has no address)
    if (rows == 0 && k1 > 0 && k2 >= 0 && n > 0 && act >= 0 && act <= 2) return 0;
    if (rows < 0 || k1 <= 0 || k2 < 0 || n <= 0 || lda < k1 || (k2 > 0 && (!a2 || lda2 < k2)) || ldc < n || !a || !packed || !out ||
        act < 0 || act > 2 || (residual && ldr < n))
        return ML3D_E_INVALID;
    const Epilogue ep = Epilogue::of(bias, act, slope).residual_rows(residual, ldr);
    return gemm_rows_bf16x3(a, lda, k1, a2, lda2, k2, rows, packed, n, ep, out, ldc, ws_align(workspace),
                            ws_avail(workspace, workspace_bytes), (hipStream_t)stream);
}

// the same with a GATHERED residual (ABI 12): residual row of output row m = residual_gather[m * stride] (a global row index; rows
// outside [0, residual_rows) add nothing) -- KPFCNN's decoder step split by linearity, (x W_x)[up[:, 0]] + skip W_skip (kpconv.py:283-286)
extern "C" int ml3d_linear_bf16x3_gathered(const float* a, int64_t lda, int k1, const float* a2, int64_t lda2, int k2, int64_t rows,
                                           const void* packed, const float* bias, const float* residual, int64_t ldr,
                                           const int32_t* residual_gather, int64_t residual_gather_stride, int64_t residual_rows, int n,
                                           int act, float slope, float* out, int64_t ldc, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    if (rows == 0 && k1 > 0 && k2 >= 0 && n > 0 && act >= 0 && act <= 2) return 0;
    if (rows < 0 || k1 <= 0 || k2 < 0 || n <= 0 || lda < k1 || (k2 > 0 && (!a2 || lda2 < k2)) || ldc < n || !a || !packed || !out ||
        act < 0 || act > 2 || (residual && ldr < n) || (residual_gather && (!residual || residual_gather_stride < 1 || residual_rows < 0)))
        return ML3D_E_INVALID;
    Epilogue ep = Epilogue::of(bias, act, slope).residual_rows(residual, ldr);
    if (residual_gather) ep.gathered_residual(residual_gather, residual_gather_stride, residual_rows);
    return gemm_rows_bf16x3(a, lda, k1, a2, lda2, k2, rows, packed, n, ep, out, ldc, ws_align(workspace),
                            ws_avail(workspace, workspace_bytes), (hipStream_t)stream);
}

extern "C" size_t ml3d_linear_workspace_bytes(int64_t m, int n, int k) {
    if (m < 0 || n <= 0 || k <= 0) return 0;
    return gemm_partial_bytes(m, n, k) + 512;
}

extern "C" int ml3d_linear(const float* a, int64_t lda, int k1, const int32_t* a_gather, int64_t a_gather_stride,
                           int64_t a_rows, const float* a2, int64_t lda2, int k2, const float* weights_t,
                           const float* bias, const float* residual, int64_t ldr, const int32_t* residual_gather,
                           int64_t residual_gather_stride, int64_t residual_rows, int act, float slope, float* out,
                           int64_t ldc, int64_t m, int n, void* workspace, size_t workspace_bytes, void* stream) {
    if (m < 0 || n <= 0 || k1 < 0 || k2 < 0 || k1 + k2 <= 0 || act < 0 || act > 2) return ML3D_E_INVALID;
    if (m == 0) return 0;
    if (!weights_t || !out || (k1 > 0 && !a) || (k2 > 0 && !a2) || lda < k1 || (k2 > 0 && lda2 < k2) || ldc < n ||
        (residual && ldr < n) || (residual_gather && (!residual || residual_gather_stride < 1 || residual_rows < 0)))
        return ML3D_E_INVALID;
    RowsA A;
    A.a = a; A.lda = lda; A.k1 = k1;
    A.gather = a_gather; A.gather_stride = a_gather_stride; A.a_rows = a_rows;
    A.a2 = a2; A.lda2 = lda2; A.k2 = k2;
    A.gather_on_a2 = 0; A.g_rows_per_item = 0; A.g_src_rows_per_item = 0;
    Epilogue ep = Epilogue::of(bias, act, slope).residual_rows(residual, ldr);
    if (residual_gather) ep.gathered_residual(residual_gather, residual_gather_stride, residual_rows);
    return gemm_rows(A, weights_t, m, n, k1 + k2, ep, out, ldc, ws_align(workspace), ws_avail(workspace, workspace_bytes),
                     (hipStream_t)stream);
}
