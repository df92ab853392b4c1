// Minimum-Bayes-risk selection: the pairwise utility of B x Nh candidates against B x Nr pseudo-references (segment-level smooth
// BLEU or an n-gram F score over clipped 1..4-gram matches), each candidate's expected utility and the first arg-max per sentence.
// Two launches (include/vag_nmt.h: vag_mbr_select):
//   mbr_pairs_kernel   one workgroup of 4 waves per candidate (b, i); the waves split the references
//   mbr_best_kernel    one wave per sentence: the lowest i whose expected utility is maximal
//
// Matching without hashing or sorting.  Lane l of a wave owns position p = 64 c + l of the candidate (chunks c = 0, 1, ..) and
// keeps the four tokens that END at p in registers (h[p], h[p-1], h[p-2], h[p-3]; slots outside the span hold -1).  The wave
// walks q over the reference's span with a sliding window of ITS last four tokens (wave-uniform LDS reads, four tokens per
// ds_read_b128; slots outside the span hold -2, so the two sentinels never match anything, each other included).  The n-gram
// that ends at p equals the one that ends at q iff the leading n of the four token compares hold, which gives, per position,
//     cnt_n(p) = #{q : the n-gram ending at q in r equals the one ending at p in h}  =  count_r(g),  g the n-gram at p.
// Clipping: once per workgroup the same walk of the candidate against ITSELF, restricted to q < p, gives
//     rank_n(p) = the number of earlier positions of h that carry the same n-gram,
// so the positions of an n-gram g that occurs a times in h have ranks 0 .. a-1, and "rank_n(p) < cnt_n(p)" holds for exactly
// min(a, count_r(g)) of them.  Summing that predicate over p (ballot + popcount) is sum_g min(count_h(g), count_r(g)) = m_n.
// No cross-lane traffic inside the walk; integers only, so the counts do not depend on the order of anything.
#include "mbr_shared.h"                  // the span load, the tail and the walk (shared with corpus.hip), the sentinels and limits

constexpr int MBR_MAX_N = 1024;          // rows per sentence (LDS: one utility per reference)

__device__ __forceinline__ float mbr_utility(int utility, const int (&m)[4], int lh, int lr) {
    if (utility == 0) {                                                       // smooth BLEU of the segment
        if (lh == 0) return 0.f;
        float s = 0.f;
#pragma unroll
        for (int n = 1; n <= 4; ++n) s += logf((float)(m[n - 1] + 1) / (float)(max(0, lh - n + 1) + 1));
        const float bp = lh > lr ? 1.f : expf(1.f - (float)lr / (float)lh);
        return bp * expf(0.25f * s);
    }
    float s = 0.f;                                                            // n-gram F: the mean of 2 m_n / (T_n(h) + T_n(r))
    int orders = 0;
#pragma unroll
    for (int n = 1; n <= 4; ++n) {
        const int tot = max(0, lh - n + 1) + max(0, lr - n + 1);
        if (tot > 0) { s += (float)(2 * m[n - 1]) / (float)tot; ++orders; }
    }
    return orders ? s / (float)orders : 0.f;
}

__global__ __launch_bounds__(64 * MBR_WAVES) void mbr_pairs_kernel(const int64_t* __restrict__ hyps, const int64_t* __restrict__ refs,
                                                                  const float* __restrict__ weights, float uniform_w, int Nh, int Lh,
                                                                  int Nr, int Lr, int utility, int32_t* __restrict__ matches,
                                                                  float* __restrict__ util, float* __restrict__ expected) {
    __shared__ __attribute__((aligned(16))) int hbuf[MBR_MAX_L];
    __shared__ __attribute__((aligned(16))) int rbuf[MBR_WAVES][MBR_MAX_L];
    __shared__ uint2 rank[MBR_MAX_L];                                         // four 16-bit ranks per position (each < MBR_MAX_L)
    __shared__ float us[MBR_MAX_N];
    __shared__ int lh_s;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t bi = blockIdx.x;                                            // b * Nh + i
    const int64_t b = bi / Nh;

    if (wave == 0) {
        const int l = mbr_load_span(hyps + bi * Lh, Lh, hbuf, lane);
        if (lane == 0) lh_s = l;
    }
    __syncthreads();
    const int lh = lh_s;
    const int chunks = (lh + 63) >> 6;
    for (int c = wave; c < chunks; c += MBR_WAVES) {                          // the ranks: the candidate against itself
        const int p = c * 64 + lane;
        int h0, h1, h2, h3;
        mbr_tail(hbuf, lh, p, h0, h1, h2, h3);
        int cnt[4] = {0, 0, 0, 0};
        mbr_walk<true>(hbuf, min(lh, c * 64 + 64), p, h0, h1, h2, h3, cnt);  // (q < p: nothing to find past the chunk's end)
        rank[p] = make_uint2((unsigned)cnt[0] | ((unsigned)cnt[1] << 16), (unsigned)cnt[2] | ((unsigned)cnt[3] << 16));
    }
    __syncthreads();

    int* rb = rbuf[wave];
    for (int j = wave; j < Nr; j += MBR_WAVES) {
        mbr_wave_fence();                                                     // the previous reference's reads are done
        const int lr = mbr_load_span(refs + (b * Nr + j) * Lr, Lr, rb, lane);
        mbr_wave_fence();
        int m[4] = {0, 0, 0, 0};
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            int h0, h1, h2, h3;
            mbr_tail(hbuf, lh, p, h0, h1, h2, h3);
            int cnt[4] = {0, 0, 0, 0};
            mbr_walk<false>(rb, lr, p, h0, h1, h2, h3, cnt);
            const uint2 rk = rank[p];                                         // (p < 64 chunks: written above)
            m[0] += __popcll(__ballot((int)(rk.x & 0xffffu) < cnt[0]));
            m[1] += __popcll(__ballot((int)(rk.x >> 16) < cnt[1]));
            m[2] += __popcll(__ballot((int)(rk.y & 0xffffu) < cnt[2]));
            m[3] += __popcll(__ballot((int)(rk.y >> 16) < cnt[3]));
        }
        const float u = mbr_utility(utility, m, lh, lr);                      // (uniform over the wave)
        if (lane == 0) {
            const int64_t o = bi * Nr + j;
            us[j] = u;
            if (util) util[o] = u;
            if (matches) {
#pragma unroll
                for (int n = 0; n < 4; ++n) matches[o * 4 + n] = m[n];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                   // E_i: fp32, j = 0 .. Nr-1 in order, product and sum
        float e = 0.f;                                                        // rounded separately
        for (int j = 0; j < Nr; ++j) e = __fadd_rn(e, __fmul_rn(weights ? weights[b * Nr + j] : uniform_w, us[j]));
        expected[bi] = e;
    }
}

// best[b] = the lowest i with expected[b, i] >= every other (a NaN is never chosen over a number; all NaN: 0)
__global__ __launch_bounds__(64) void mbr_best_kernel(const float* __restrict__ expected, int Nh, int64_t* __restrict__ best) {
    const int lane = threadIdx.x;
    const float* e = expected + (int64_t)blockIdx.x * Nh;
    float bv = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = lane; i < Nh; i += 64) {
        const float v = e[i];
        if (v > bv || (v == bv && i < bidx)) { bv = v; bidx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ov > bv || (ov == bv && oi < bidx)) { bv = ov; bidx = oi; }
    }
    if (lane == 0) best[blockIdx.x] = bidx == 0x7fffffff ? 0 : bidx;
}

// the arg-max launch alone (checked operands): vag_chrf_select_launch (chrf.hip) ends in it too
int vag_mbr_best_launch(const float* expected, int64_t B, int64_t Nh, int64_t* best, hipStream_t s) {
    hipLaunchKernelGGL(mbr_best_kernel, dim3((unsigned)B), dim3(64), 0, s, expected, (int)Nh, best);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_mbr_supported_host(int64_t Nh, int64_t Lh, int64_t Nr, int64_t Lr) {
    return Nh >= 1 && Nh <= MBR_MAX_N && Nr >= 1 && Nr <= MBR_MAX_N && Lh >= 1 && Lh <= MBR_MAX_L && Lr >= 1 && Lr <= MBR_MAX_L;
}

int vag_mbr_select_launch(const int64_t* hyps, const int64_t* refs, const float* weights, int64_t B, int64_t Nh, int64_t Lh,
                          int64_t Nr, int64_t Lr, int utility, int32_t* matches, float* util, float* expected, int64_t* best,
                          hipStream_t s) {
    VAG_CHECK_ARG(hyps && expected && best);
    VAG_CHECK_ARG(B >= 1 && Nh >= 1 && Lh >= 1 && Nr >= 1 && Lr >= 1 && (utility == 0 || utility == 1));
    VAG_CHECK_ARG(vag_mbr_supported_host(Nh, Lh, Nr, Lr) && B < (1ll << 31) / MBR_MAX_N);
    VAG_CHECK_ARG(refs || (Nr == Nh && Lr == Lh));
    hipLaunchKernelGGL(mbr_pairs_kernel, dim3((unsigned)(B * Nh)), dim3(64 * MBR_WAVES), 0, s, hyps, refs ? refs : hyps, weights,
                       1.0f / (float)Nr, (int)Nh, (int)Lh, (int)Nr, (int)Lr, utility, matches, util, expected);
    VAG_LAUNCH_CHECK();
    return vag_mbr_best_launch(expected, B, Nh, best, s);
}
