// Small host-side helpers of the ABI translation units (api.hip, enc_api.hip, dec_api.hip, head_api.hip): the stream cast, fills / copies as kernels and the
// dense-product shorthands of the forward, data-gradient and weight-gradient layouts.
#pragma once
#include "kernels.h"

#define S_(x) reinterpret_cast<hipStream_t>(x)
// an fp16 operand (2-byte storage mode) where a launch function's argument list says float: the launch is told so separately
static inline const float* as_f(const vag_half* p) { return reinterpret_cast<const float*>(p); }

// Fills and copies are kernels (not hipMemset/hipMemcpy nodes) so a captured step is a pure chain of kernel nodes.
static inline int zero_async(void* p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return VAG_OK;
    return vag_axpy_launch(0.f, reinterpret_cast<const float*>(p), reinterpret_cast<float*>(p), (int64_t)(bytes / 4), 2, s);
}
static inline int copy_async(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return VAG_OK;
    return vag_axpy_launch(1.f, reinterpret_cast<const float*>(src), reinterpret_cast<float*>(dst), (int64_t)(bytes / 4), 0, s);
}
// y = act(x W^T + b): small-M kernel for a single time step, tiled kernel otherwise.
static inline int linear_fwd(int64_t M, int64_t N, int64_t K, const float* x, int64_t ldx, const float* W, const float* bias,
                             int act, float* y, int64_t ldy, hipStream_t s) {
    if (M <= 256) return vag_skinny_launch(M, N, K, x, ldx, W, K, bias, nullptr, 0, y, ldy, act, s);
    return vag_gemm_launch(M, N, K, 1.f, x, ldx, 1, W, 1, K, 0.f, y, ldy, bias, act, s);
}
// C (+)= A^T B with A (R,M) lda, B (R,N) ldb: weight gradients  g_W[m,n] += sum_r dY[r,m] X[r,n]
// g_bias (optional): += sum_r A[r,:], the bias gradient that goes with this weight gradient -- taken from the A tiles inside the
// product (GemmArgs::rowsum), no second pass over dY
static inline int gemm_tn_acc(int64_t M, int64_t N, int64_t R, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                              int64_t ldc, hipStream_t s, float* g_bias = nullptr) {
    if (R == 0) return VAG_OK;
    return vag_gemm_launch(M, N, R, 1.f, A, 1, lda, B, ldb, 1, 1.f, C, ldc, nullptr, VAG_ACT_NONE, s, 0, g_bias);
}
// C = beta*C + A B with A (M,K) lda, B (K,N) ldb: data gradients  dX = dY W
static inline int gemm_nn(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb, float beta,
                          float* C, int64_t ldc, hipStream_t s) {
    if (M <= 128 && (beta == 0.f || beta == 1.f)) return vag_skinny_nn_launch(M, N, K, A, lda, B, ldb, beta, C, ldc, s);
    return vag_gemm_launch(M, N, K, 1.f, A, lda, 1, B, ldb, 1, beta, C, ldc, nullptr, VAG_ACT_NONE, s);
}
