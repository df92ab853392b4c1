// Word-level knowledge distillation (Kim & Rush 2016; include/vag_nmt.h: vag_kd_targets, vag_kd_head_ce_seq_fwd): a SPARSE teacher
// distribution per target position -- its K <= 64 best words, renormalised -- mixed into the head's loss.
//   targets   one workgroup per row reads the M members' logits rows once, scores s_j = ens_combine_m(logits_m[j] - lse_m)
//             (select.h), keeps the K best under (value desc, word asc) with select.h's radix top-k -- each wave a running ranked
//             top-K of the 512-word slices it walks, wave 0 merges the four lists -- and writes idx best first with
//             q_k = exp((s_k - s_0) / T) / sum.
//   nll       after lse_nll on the same rows: nll[row] = w (lse - (1 - lambda) x[y] - lambda sum_k q_k x[idx_k]), K + 1 gathers.
//   d(logits) after ce_bwd / ce_bwd_colsum on the same rows, before anything reads d(logits): those kernels have written
//             coef (softmax_j - [j == y]); the soft loss differs from it by +coef lambda at y and -coef lambda q_k at idx_k.
// The soft part of the loss and of its gradient touches K + 1 logits of a row, not V: two small launches beside the V-wide
// kernels of head.hip, which stay as they are.  One wave per row in both.
#include "kernels.h"
#include "select.h"

namespace {

constexpr int KD_EPT = 8;                   // words per lane and round: a wave walks slices of 64 * KD_EPT words
constexpr int KD_SLICE = 64 * KD_EPT;

// the teacher's score of word w in row `row`: the members' log-probabilities logit - lse (one IEEE subtraction each), combined
template <int M>
__device__ __forceinline__ float kd_score(const EnsLogp<M>& L, const float (&lse)[M], int64_t row, int w) {
    float x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = L.p[m][row * L.ld[m] + w];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = __fsub_rn(x[m], lse[m]);
    return ens_combine<M>(x);
}

template <int M>
__global__ __launch_bounds__(256) void kd_targets_kernel(EnsLogp<M> L, EnsRows<M> S, int V, int K, float T, int32_t* __restrict__ idx,
                                                         float* __restrict__ q) {
    __shared__ float wv[4 * 64], sv[4 * 64];
    __shared__ int wi[4 * 64], si[4 * 64];
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lse[M];
#pragma unroll
    for (int m = 0; m < M; ++m) lse[m] = S.p[m][row];
    float* ov = wv + wave * 64;
    int* oi = wi + wave * 64;
    int cnt = 0;                                                                // ranked entries in (ov, oi), uniform over the wave
    for (int base = wave * KD_SLICE; base < V; base += 4 * KD_SLICE) {
        float val[KD_EPT + 1];
        int ix[KD_EPT + 1];
#pragma unroll
        for (int e = 0; e < KD_EPT; ++e) {                                      // all M * KD_EPT loads in flight together (index clamped)
            const int w = base + e * 64 + lane;
            const float s = kd_score<M>(L, lse, row, min(w, V - 1));
            val[e] = w < V ? s : -INFINITY;
            ix[e] = w < V ? w : 0x7fffffff;
        }
        val[KD_EPT] = lane < cnt ? ov[lane] : -INFINITY;
        ix[KD_EPT] = lane < cnt ? oi[lane] : 0x7fffffff;
        wave_lds_fence();
        cnt = wave_topk<KD_EPT + 1>(val, ix, K, sv + wave * 64, si + wave * 64, ov, oi);
        wave_lds_fence();
    }
    if (lane >= cnt) { ov[lane] = -INFINITY; oi[lane] = 0x7fffffff; }
    __syncthreads();
    if (wave != 0) return;
    float v2[4];
    int i2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v2[e] = wv[e * 64 + lane]; i2[e] = wi[e * 64 + lane]; }
    wave_lds_fence();
    const int nc = wave_topk<4>(v2, i2, K, sv, si, wv, wi);                     // ranked, best first, in wv / wi[0, nc); nc == K (K <= V)
    wave_lds_fence();
    const bool in = lane < nc;
    const float s = in ? wv[lane] : 0.f, s0 = wv[0];
    const float e = in ? expf((s - s0) / T) : 0.f;                              // the largest exponent is 0
    const float sum = wave_sum(e);                                              // one fixed tree: the same bits on every run
    if (lane < K) {
        idx[row * K + lane] = in ? wi[lane] : 0;
        q[row * K + lane] = in ? e / sum : 0.f;
    }
}

// rows of a chunk of whole time steps: row r = t*B + b of the chunk, tgt / lse / nll / idx / q offset to the chunk by the caller
__global__ __launch_bounds__(256) void kd_nll_kernel(const float* __restrict__ logits, int64_t ldl, int rows, int V,
                                                     const int64_t* __restrict__ tgt, int B, int Tt, const float* __restrict__ vw,
                                                     const float* __restrict__ lse, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ q, int K, float lambda, float* __restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                    // (uniform over the wave)
    const int t = row / B, b = row - t * B;
    const int64_t y = tgt[(int64_t)b * Tt + t];
    const float* x = logits + (int64_t)row * ldl;
    float part = 0.f;
    if (lane < K) {
        const int j = idx[(int64_t)row * K + lane];
        part = q[(int64_t)row * K + lane] * ((unsigned)j < (unsigned)V ? x[j] : NAN);       // a word outside [0, V): NaN, never a stray read
    }
    const float soft = wave_sum(part);                                          // lanes in a fixed tree: reproducible
    if (lane == 0) nll[row] = vw[y] * (lse[row] - (1.f - lambda) * x[y] - lambda * soft);
}

// lane k owns idx_k and folds the gold word's term in when idx_k == y; when no idx_k is y, lane 0 owns y as well (K may be 64:
// there is no spare lane).  The words of a row are distinct, so no two updates of a launch meet in d(logits); in g_bias rows meet,
// through the same fp32 atomics ce_bwd_colsum_kernel adds its column sums with.
__global__ __launch_bounds__(256) void kd_dlogits_kernel(float* __restrict__ dlogits, int64_t ldl, int rows, int V,
                                                         const int64_t* __restrict__ tgt, int B, int Tt,
                                                         const float* __restrict__ vw, const float* __restrict__ inv_cnt,
                                                         const float* __restrict__ d_loss, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ q, int K, float lambda,
                                                         float* __restrict__ g_bias) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                    // (uniform over the wave)
    const int t = row / B, b = row - t * B;
    const int64_t y = tgt[(int64_t)b * Tt + t];
    const float coef = d_loss[0] * inv_cnt[b] / (float)B * vw[y];               // ce_bwd_kernel's
    if (coef == 0.f) return;                                                    // PAD rows: nothing is written
    const float cl = coef * lambda;
    float* x = dlogits + (int64_t)row * ldl;
    int j = -1;
    float amount = 0.f;
    if (lane < K) {
        j = idx[(int64_t)row * K + lane];
        amount = cl * ((j == y ? 1.f : 0.f) - q[(int64_t)row * K + lane]);
    }
    const bool has_y = __ballot(lane < K && j == y) != 0ull;
    if ((unsigned)j < (unsigned)V) {
        x[j] += amount;
        if (g_bias) atomicAdd(g_bias + j, amount);
    }
    if (!has_y && lane == 0 && (uint64_t)y < (uint64_t)V) {
        x[y] += cl;
        if (g_bias) atomicAdd(g_bias + y, cl);
    }
}

bool kd_rows_ok(int64_t rows, int64_t V, int64_t B, int64_t Tt, int64_t K, float lambda) {
    return rows >= 0 && rows < (1ll << 31) && V > 0 && V < (1ll << 31) && B > 0 && B < (1ll << 31) && Tt > 0 && Tt < (1ll << 31) &&
           vag_kd_ok(K, lambda, V);
}

}  // namespace

int vag_kd_nll_launch(const float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                      const float* vw, const float* lse, const int32_t* idx, const float* q, int64_t K, float lambda, float* nll,
                      hipStream_t s) {
    VAG_CHECK_ARG(logits && tgt && vw && lse && idx && q && nll && ldl >= V && kd_rows_ok(rows, V, B, Tt, K, lambda));
    if (rows == 0) return VAG_OK;
    hipLaunchKernelGGL(kd_nll_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, logits, ldl, (int)rows, (int)V, tgt, (int)B,
                       (int)Tt, vw, lse, idx, q, (int)K, lambda, nll);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_kd_dlogits_launch(float* dlogits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                          const float* vw, const float* inv_cnt, const float* d_loss, const int32_t* idx, const float* q, int64_t K,
                          float lambda, float* g_bias, hipStream_t s) {
    VAG_CHECK_ARG(dlogits && tgt && vw && inv_cnt && d_loss && idx && q && ldl >= V && kd_rows_ok(rows, V, B, Tt, K, lambda));
    if (rows == 0) return VAG_OK;
    hipLaunchKernelGGL(kd_dlogits_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, dlogits, ldl, (int)rows, (int)V, tgt,
                       (int)B, (int)Tt, vw, inv_cnt, d_loss, idx, q, (int)K, lambda, g_bias);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

extern "C" {

int vag_kd_targets(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, int64_t R, int64_t V,
                   int64_t K, float temperature, int32_t* idx, float* q, vag_stream_t stream) {
    VAG_CHECK_ARG(K >= 1 && K <= 64 && K <= V && V < (1ll << 24));             // (the radix keys hold 24 index bits)
    VAG_CHECK_ARG(temperature > 0.f && temperature < INFINITY);                // (NaN fails both)
    EnsHost a;
    VAG_TRY(ens_logp_args(logits, ldl, M, V, a));                              // NULL array or entry, M outside [1, VAG_ENS_MAX], ldl[m] < V
    VAG_CHECK_ARG(lse && idx && q && R >= 0 && R < (1ll << 31));
    for (int m = 0; m < (int)M; ++m) VAG_CHECK_ARG(lse[m] != nullptr);
    if (R == 0) return VAG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL(kd_targets_kernel<MM>, dim3((unsigned)R), dim3(256), 0, s, ens_logp<MM>(a), ens_rows<MM>(lse), (int)V,
                           (int)K, temperature, idx, q);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

}  // extern "C"
