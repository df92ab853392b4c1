// R-Drop (Liang et al. 2021, "R-Drop: Regularized Dropout for Neural Networks"; include/vag_nmt.h: vag_rdrop_head_ce_seq_fwd): every
// sentence sits twice in the batch, in adjacent rows, under two dropout masks; the two predicted distributions of every target
// position are pulled together by a symmetric KL term.  Head rows are time-major, r = t*B + b with B even: the twin of r is r ^ 1.
//   forward   after lse_nll on the same rows: one workgroup per PAIR streams both rows once, given their lse, and forms
//             kl[r] = sum_j p_r[j] (lp_r[j] - lp_twin[j]) for both directions; nll[r] += w_r (alpha / 4) (kl[r] + kl[twin]).
//             Each thread's sum runs in index order, the threads meet in one fixed tree: no atomics, the same bits on every run.
//   backward  in place of ce_bwd_colsum on the same rows: elementwise in (x_r[j], x_twin[j]) given lse and kl of both rows,
//             d x_r[j] = coef_r (p_r - (1 - eps) [j == y_r] - eps / V)
//                        + (alpha / 4) (coef_r + coef_twin) (p_r ((lp_r - lp_twin) - kl[r]) + p_r - p_twin),
//             a thread owning four columns over a strip of row pairs: both rows are read before either is written, the strip's
//             column sums (g(out.bias)) meet in registers and leave as one atomic per column and strip, as ce_bwd_colsum's do.
// Unlike distillation's K + 1 logits per row the term is dense over the vocabulary: both kernels are V-wide and stream the rows
// (a pair is 75 KB at V = 9391, 320 KB at V = 40000: nothing is held in LDS).
#include "kernels.h"

namespace {

__device__ __forceinline__ float rd_block_sum(float v, float* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// one 256-thread workgroup per pair (rows 2 p, 2 p + 1 of the chunk).  16-byte loads over the whole groups of four columns below V,
// the V % 4 columns behind them one by one: the padding columns [V, ldl) are never read.
__global__ __launch_bounds__(256) void rdrop_pair_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                         const int64_t* __restrict__ tgt, int B, int Tt, const float* __restrict__ vw,
                                                         const float* __restrict__ lse, float qalpha, float* __restrict__ kl,
                                                         float* __restrict__ nll) {
    __shared__ float sh[4];
    const int64_t ra = 2 * (int64_t)blockIdx.x, rb = ra + 1;
    const float* xa = logits + ra * ldl;
    const float* xb = logits + rb * ldl;
    const float la = lse[ra], lb = lse[rb];
    float ka = 0.f, kb = 0.f;
    const int n4 = V >> 2;
    const float4* xa4 = reinterpret_cast<const float4*>(xa);
    const float4* xb4 = reinterpret_cast<const float4*>(xb);
    for (int i0 = threadIdx.x; i0 < n4; i0 += 512) {
        float4 a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {                           // four 16-byte loads in flight per thread (index clamped, use masked)
            const int i4 = min(i0 + 256 * u, n4 - 1);
            a[u] = xa4[i4];
            b[u] = xb4[i4];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (i0 + 256 * u < n4) {
                const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, bv[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float lpa = av[q] - la, lpb = bv[q] - lb, d = lpa - lpb;
                    ka += __expf(lpa) * d;
                    kb -= __expf(lpb) * d;
                }
            }
        }
    }
    {
        const int j = 4 * n4 + (int)threadIdx.x;                // the last V % 4 columns
        if (j < V) {
            const float lpa = xa[j] - la, lpb = xb[j] - lb, d = lpa - lpb;
            ka += __expf(lpa) * d;
            kb -= __expf(lpb) * d;
        }
    }
    ka = rd_block_sum(ka, sh);
    kb = rd_block_sum(kb, sh);
    if (threadIdx.x == 0) {
        const int t = (int)(ra / B), b0 = (int)(ra - (int64_t)t * B);
        const float wa = vw[tgt[(int64_t)b0 * Tt + t]], wb = vw[tgt[(int64_t)(b0 + 1) * Tt + t]];
        const float both = qalpha * (ka + kb);                  // (not clamped: the gradient is this sum's, a few ulp below 0 included)
        kl[ra] = ka;
        kl[rb] = kb;
        nll[ra] += wa * both;
        nll[rb] += wb * both;
    }
}

// grid (ceil(ldl / 1024), ceil(rows / rows_per)), rows_per even: a thread owns four consecutive columns over a strip of row pairs,
// two pairs (four 16-byte loads) in flight -- ce_bwd_colsum_kernel's tiling, with the twin's row where that kernel has the next row.
template <bool LS>
__global__ __launch_bounds__(256) void rdrop_bwd_colsum_kernel(float* __restrict__ logits, int64_t ldl, int V,
                                                               const int64_t* __restrict__ tgt, int B, int Tt,
                                                               const float* __restrict__ vw, const float* __restrict__ lse,
                                                               const float* __restrict__ kl, const float* __restrict__ inv_cnt,
                                                               const float* __restrict__ d_loss, int rows, int rows_per, float qalpha,
                                                               float* __restrict__ g_bias, float eps) {
    const float hit = LS ? 1.f - eps : 1.f, uni = LS ? eps / (float)V : 0.f;
    const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int r0 = blockIdx.y * rows_per, r1 = j < ldl ? min(rows, r0 + rows_per) : r0;      // columns past ldl: no rows, zero sums
    const float dl = d_loss[0] / (float)B;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += 4) {                          // r0, r1 and rows are even: rows r + 2 p, r + 2 p + 1 are twins
        float4 x[4];
        float coef[4], l[4], k[4];
        int tg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = r + u < r1 ? r + u : r + (u & 1);      // uniform over the block; past the strip: the first pair again
            const int t = row / B, b = row - t * B;
            const int64_t g = tgt[(int64_t)b * Tt + t];
            tg[u] = (int)g;
            coef[u] = dl * inv_cnt[b] * vw[g];
            l[u] = lse[row];
            k[u] = kl[row];
            x[u] = *reinterpret_cast<const float4*>(logits + (int64_t)row * ldl + j);
        }
#pragma unroll
        for (int p = 0; p < 4; p += 2) {
            if (r + p < r1) {
                const float c2 = qalpha * (coef[p] + coef[p + 1]);
                const bool live = coef[p] + coef[p + 1] != 0.f;
                const float xa[4] = {x[p].x, x[p].y, x[p].z, x[p].w}, xb[4] = {x[p + 1].x, x[p + 1].y, x[p + 1].z, x[p + 1].w};
                float ga[4], gb[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float lpa = xa[q] - l[p], lpb = xb[q] - l[p + 1], d = lpa - lpb;
                    const float pa = __expf(lpa), pb = __expf(lpb);
                    const float va = coef[p] * (pa - (j + q == tg[p] ? hit : 0.f) - uni) + c2 * (pa * (d - k[p]) + (pa - pb));
                    const float vb = coef[p + 1] * (pb - (j + q == tg[p + 1] ? hit : 0.f) - uni) + c2 * (pb * (-d - k[p + 1]) + (pb - pa));
                    ga[q] = (live && j + q < V) ? va : 0.f;
                    gb[q] = (live && j + q < V) ? vb : 0.f;
                    acc[q] += ga[q] + gb[q];
                }
                *reinterpret_cast<float4*>(logits + (int64_t)(r + p) * ldl + j) = make_float4(ga[0], ga[1], ga[2], ga[3]);
                *reinterpret_cast<float4*>(logits + (int64_t)(r + p + 1) * ldl + j) = make_float4(gb[0], gb[1], gb[2], gb[3]);
            }
        }
    }
    // the strip's column sums through LDS: every atomic wave-instruction adds 64 consecutive columns (see ce_bwd_colsum_kernel)
    __shared__ float cs[1024];
#pragma unroll
    for (int q = 0; q < 4; ++q) cs[4 * threadIdx.x + q] = acc[q];
    __syncthreads();
    const int jb = blockIdx.x * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = jb + q * 256 + threadIdx.x;
        if (c < V) atomicAdd(g_bias + c, cs[q * 256 + threadIdx.x]);
    }
}

bool rd_rows_ok(const float* logits, int64_t ldl, int64_t rows, int64_t V, int64_t B, int64_t Tt, float alpha) {
    return vag_rdrop_ok(alpha) && rows >= 0 && rows < (1ll << 31) && V > 0 && V < (1ll << 31) && ldl >= V && ldl % 4 == 0 &&
           ldl < (1ll << 31) && aligned16(logits) && B > 0 && B % 2 == 0 && B < (1ll << 31) && Tt > 0 && Tt < (1ll << 31) &&
           rows % B == 0 && rows <= B * Tt;
}

}  // namespace

int vag_rdrop_pair_launch(const float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                          const float* vw, const float* lse, float alpha, float* kl, float* nll, hipStream_t s) {
    VAG_CHECK_ARG(logits && tgt && vw && lse && kl && nll && rd_rows_ok(logits, ldl, rows, V, B, Tt, alpha));
    if (rows == 0) return VAG_OK;
    hipLaunchKernelGGL(rdrop_pair_kernel, dim3((unsigned)(rows / 2)), dim3(256), 0, s, logits, ldl, (int)V, tgt, (int)B, (int)Tt, vw,
                       lse, alpha * 0.25f, kl, nll);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_rdrop_bwd_colsum_launch(float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                                const float* vw, const float* lse, const float* kl, const float* inv_cnt, const float* d_loss,
                                float alpha, float* g_bias, hipStream_t s, float eps) {
    VAG_CHECK_ARG(logits && tgt && vw && lse && kl && inv_cnt && d_loss && g_bias && rd_rows_ok(logits, ldl, rows, V, B, Tt, alpha));
    VAG_CHECK_ARG(vag_label_smoothing_ok(eps));
    if (rows == 0) return VAG_OK;
    const int64_t nbx = cdiv64(ldl, 1024);
    int64_t splits = cdiv64(1024, nbx);                  // ~1024 blocks: every strip costs ldl atomics (vag_ce_bwd_colsum_launch)
    if (splits > cdiv64(rows, 8)) splits = cdiv64(rows, 8);
    const int rows_per = (int)((cdiv64(rows, splits) + 1) / 2 * 2);      // whole pairs
    dim3 grid((unsigned)nbx, (unsigned)cdiv64(rows, rows_per));
    if (eps > 0.f)
        hipLaunchKernelGGL(rdrop_bwd_colsum_kernel<true>, grid, dim3(256), 0, s, logits, ldl, (int)V, tgt, (int)B, (int)Tt, vw, lse, kl,
                           inv_cnt, d_loss, (int)rows, rows_per, alpha * 0.25f, g_bias, eps);
    else
        hipLaunchKernelGGL(rdrop_bwd_colsum_kernel<false>, grid, dim3(256), 0, s, logits, ldl, (int)V, tgt, (int)B, (int)Tt, vw, lse, kl,
                           inv_cnt, d_loss, (int)rows, rows_per, alpha * 0.25f, g_bias, eps);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
