// Corpus BLEU statistics on the device: per sentence the clipped 1..4-gram matches of a hypothesis against the MERGED counts of
// its references, the n-gram totals and the two lengths, written per sentence and added to one running total
// (include/vag_nmt.h: vag_corpus_bleu_stats).  One launch:
//   corpus_bleu_kernel   one workgroup of 4 waves per sentence; the waves split the references
//
// The matching is mbr_pairs_kernel's (mbr.hip has the derivation; the device functions are mbr_shared.h's): the hypothesis span in
// LDS, rank_n(p) = the number of earlier positions of h with the n-gram that ends at p (the self-walk, once per workgroup), and
// per reference j the walk that gives cnt_{n,j}(p) = count_{r_j}(that n-gram).  What the pairwise kernel cannot express is the
// clipping against several references at once: bleu.py clips by the per-n-gram MAXIMUM of the references' counts.  So every
// wave keeps, per position and order, the running maximum over ITS references (its own LDS slice: lane l reads and writes only
// the positions it owns, so nothing crosses lanes), the workgroup takes the maximum over the waves,
//     C_n(p) = max_j cnt_{n,j}(p),
// and m_n = #{p : rank_n(p) < C_n(p)} = sum_g min(count_h(g), max_j count_{r_j}(g)) by the same counting argument.
// Integers only: no floating point anywhere, and the totals are integer atomics, so their values do not depend on any order.
#include "mbr_shared.h"

constexpr int CORPUS_MAX_R = 64;         // references per sentence

// LDS of one workgroup, in bytes:  hbuf 2048 + rbuf 4 x 2048 + rank 4096 + cmax 4 x 4096 + 36 = 30756 (five workgroups per CU)
__global__ __launch_bounds__(64 * MBR_WAVES) void corpus_bleu_kernel(const int64_t* __restrict__ hyps, const int64_t* __restrict__ refs,
                                                                    const int32_t* __restrict__ n_refs, int Lh, int R, int Lr,
                                                                    int32_t* __restrict__ per_sentence,
                                                                    unsigned long long* __restrict__ totals) {
    __shared__ __attribute__((aligned(16))) int hbuf[MBR_MAX_L];
    __shared__ __attribute__((aligned(16))) int rbuf[MBR_WAVES][MBR_MAX_L];
    __shared__ uint2 rank[MBR_MAX_L];                                         // four 16-bit ranks per position (each < MBR_MAX_L)
    __shared__ uint2 cmax[MBR_WAVES][MBR_MAX_L];                              // four 16-bit counts per position (each <= MBR_MAX_L)
    __shared__ int lh_s, m_s[4], lr_s[MBR_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = blockIdx.x;

    if (wave == 0) {
        const int l = mbr_load_span(hyps + b * Lh, Lh, hbuf, lane);
        if (lane == 0) lh_s = l;
    }
    if (threadIdx.x < 4) m_s[threadIdx.x] = 0;
    __syncthreads();
    const int lh = lh_s;
    const int chunks = (lh + 63) >> 6;
    for (int c = wave; c < chunks; c += MBR_WAVES) {                          // the ranks: the hypothesis against itself
        const int p = c * 64 + lane;
        int h0, h1, h2, h3;
        mbr_tail(hbuf, lh, p, h0, h1, h2, h3);
        int cnt[4] = {0, 0, 0, 0};
        mbr_walk<true>(hbuf, min(lh, c * 64 + 64), p, h0, h1, h2, h3, cnt);  // (q < p: nothing to find past the chunk's end)
        rank[p] = make_uint2((unsigned)cnt[0] | ((unsigned)cnt[1] << 16), (unsigned)cnt[2] | ((unsigned)cnt[3] << 16));
    }
    uint2* cm = cmax[wave];
    for (int c = 0; c < chunks; ++c) cm[c * 64 + lane] = make_uint2(0u, 0u);  // a wave without a reference contributes 0
    __syncthreads();

    int nr = n_refs ? n_refs[b] : R;
    nr = min(max(nr, 1), R);                                                  // rows j >= nr are never read
    int* rb = rbuf[wave];
    int lr_min = 0x7fffffff;
    for (int j = wave; j < nr; j += MBR_WAVES) {
        mbr_wave_fence();                                                     // the previous reference's reads are done
        const int lr = mbr_load_span(refs + (b * R + j) * Lr, Lr, rb, lane);
        mbr_wave_fence();
        lr_min = min(lr_min, lr);
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            int h0, h1, h2, h3;
            mbr_tail(hbuf, lh, p, h0, h1, h2, h3);
            int cnt[4] = {0, 0, 0, 0};
            mbr_walk<false>(rb, lr, p, h0, h1, h2, h3, cnt);
            const uint2 o = cm[p];                                            // (this lane's own word: written above or by itself)
            cm[p] = make_uint2((unsigned)max((int)(o.x & 0xffffu), cnt[0]) | ((unsigned)max((int)(o.x >> 16), cnt[1]) << 16),
                               (unsigned)max((int)(o.y & 0xffffu), cnt[2]) | ((unsigned)max((int)(o.y >> 16), cnt[3]) << 16));
        }
    }
    if (lane == 0) lr_s[wave] = lr_min;
    __syncthreads();

    int m[4] = {0, 0, 0, 0};
    for (int p = threadIdx.x; p < chunks * 64; p += 64 * MBR_WAVES) {        // (whole waves: chunks * 64 is a multiple of 64)
        int C[4] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < MBR_WAVES; ++w) {
            const uint2 o = cmax[w][p];
            C[0] = max(C[0], (int)(o.x & 0xffffu)); C[1] = max(C[1], (int)(o.x >> 16));
            C[2] = max(C[2], (int)(o.y & 0xffffu)); C[3] = max(C[3], (int)(o.y >> 16));
        }
        const uint2 rk = rank[p];
        m[0] += __popcll(__ballot((int)(rk.x & 0xffffu) < C[0]));
        m[1] += __popcll(__ballot((int)(rk.x >> 16) < C[1]));
        m[2] += __popcll(__ballot((int)(rk.y & 0xffffu) < C[2]));
        m[3] += __popcll(__ballot((int)(rk.y >> 16) < C[3]));
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (m[n]) atomicAdd(&m_s[n], m[n]);
    }
    __syncthreads();
    if (threadIdx.x < 10) {                                                   // m_1..m_4, T_1..T_4, l_h, l_r
        const int i = threadIdx.x;
        int lr = lr_s[0];
#pragma unroll
        for (int w = 1; w < MBR_WAVES; ++w) lr = min(lr, lr_s[w]);           // (wave 0 always has reference 0: nr >= 1)
        const int v = i < 4 ? m_s[i] : i < 8 ? max(0, lh - (i - 4)) : i == 8 ? lh : lr;
        if (per_sentence) per_sentence[b * 10 + i] = v;
        if (v) atomicAdd(totals + i, (unsigned long long)v);
    }
}

int vag_corpus_bleu_supported_host(int64_t Lh, int64_t R, int64_t Lr) {
    return Lh >= 1 && Lh <= MBR_MAX_L && Lr >= 1 && Lr <= MBR_MAX_L && R >= 1 && R <= CORPUS_MAX_R;
}

int vag_corpus_bleu_stats_launch(const int64_t* hyps, const int64_t* refs, const int32_t* n_refs, int64_t N, int64_t Lh, int64_t R,
                                 int64_t Lr, int32_t* per_sentence, int64_t* totals, hipStream_t s) {
    VAG_CHECK_ARG(hyps && refs && totals);
    VAG_CHECK_ARG(N >= 1 && Lh >= 1 && R >= 1 && Lr >= 1);
    VAG_CHECK_ARG(vag_corpus_bleu_supported_host(Lh, R, Lr) && N < (1ll << 31));
    hipLaunchKernelGGL(corpus_bleu_kernel, dim3((unsigned)N), dim3(64 * MBR_WAVES), 0, s, hyps, refs, n_refs, (int)Lh, (int)R, (int)Lr,
                       per_sentence, reinterpret_cast<unsigned long long*>(totals));
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
