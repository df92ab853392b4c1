// chrF on surface characters: the utility of minimum-Bayes-risk selection and minimum-risk training computed on the characters
// that the vocabulary ids spell, not on the ids (include/vag_nmt.h: vag_surface_expand, vag_chrf_select).
//   surface_expand_kernel   one wave per token row: the span's tokens -> their code points, concatenated
//   chrf_pairs_kernel       one workgroup of 4 waves per candidate (b, i); the waves split the references
//   mbr_best_kernel         (mbr.hip) one wave per sentence: the lowest i whose expected utility is maximal
//
// The pairs kernel is mbr_pairs_kernel's matching scheme (mbr.hip has the derivation) on character rows with six orders: lane l
// owns position p = 64 c + l of the candidate and keeps the six characters that END at p in registers (slots outside the row
// hold -1); the wave walks q over the reference with a sliding window of its last six characters (wave-uniform LDS reads, four
// characters per ds_read_b128; slots outside the row hold -2).  Code points are masked to 31 bits, so neither sentinel matches
// anything.  cnt_n(p) = count_r(the n-gram ending at p), rank_n(p) = the number of earlier positions of h with the same n-gram
// (the same walk of the candidate against itself, once per workgroup), and m_n = #{p : rank_n(p) < cnt_n(p)} by ballot + popcount.
// Integers only inside the walk; the kernel is written apart from mbr_pairs_kernel so that nothing of the BLEU path is rebuilt.
#include "kernels.h"

// "Every product and sum rounded on its own" is a property of the generated code, not of the spelling: __fmul_rn / __fadd_rn are
// plain * and + to the compiler, which fuses a product into the sum that follows it (v_fmac_f32) under its default contraction
// mode.  The empty asm makes the rounded product a value of its own that nothing can be fused into.
__device__ __forceinline__ float chrf_mul(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

constexpr int64_t CHRF_EOS = 3;
constexpr int CHRF_ORDER = 6;
constexpr int CHRF_MAX_L = 512;          // tokens per row that surface_expand_kernel takes (vag_mbr_select's limit)
constexpr int CHRF_MAX_N = 1024;         // rows per sentence (LDS: one utility per reference)
constexpr int CHRF_WAVES = 4;
// Characters per row.  LDS of one workgroup, in bytes, at C = CHRF_MAX_C:
//     candidate row    4 C            4096
//     its ranks        6 x 2 C       12288      (six 16-bit ranks per position, each < C <= 65535)
//     reference rows   4 waves x 4 C 16384
//     utilities        4 CHRF_MAX_N   4096
//     the length                         4      = 36868 B
// so four workgroups share a CU's 160 KiB: 16 waves per CU, 4 per SIMD, which is what the walk wants (its LDS reads are
// broadcasts with nothing else to overlap them than the other waves of the SIMD).  C = 2048 would need 69636 B and leave 2
// workgroups, 2 waves per SIMD; a 40-token sentence has about 200 characters, and a row beyond C is cut, not refused.
constexpr int CHRF_MAX_C = 1024;
constexpr int CHRF_PAD_H = -1, CHRF_PAD_R = -2;

__device__ __forceinline__ void chrf_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// ---- token rows -> character rows ----
// One wave per row.  Per chunk of 64 tokens: the span's end (ballot), every token's surface length, an inclusive scan over the
// wave (shifts by 1, 2, .., 32) for its offset, then every lane copies its token's characters.  An id outside [0, V) is the
// caller's to exclude; it is taken as an empty surface here, so nothing is read out of the table's bounds.
__global__ __launch_bounds__(64 * CHRF_WAVES) void surface_expand_kernel(const int64_t* __restrict__ rows, int64_t R, int L,
                                                                         const int32_t* __restrict__ off,
                                                                         const int32_t* __restrict__ chars, int64_t V,
                                                                         int32_t* __restrict__ out, int C, int32_t* __restrict__ lens) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * CHRF_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                                                       // (uniform over the wave)
    const int64_t* row = rows + r * L;
    int32_t* o = out + r * C;
    int total = 0;                                                            // characters before this chunk (uniform)
    for (int base = 0; base < L; base += 64) {
        const int p = base + lane;
        const int64_t t = p < L ? row[p] : CHRF_EOS;
        const unsigned long long stop = __ballot(p < L && t == CHRF_EOS);
        const int end = stop ? base + (__ffsll(stop) - 1) : L;
        const bool in = p < end && t >= 0 && t < V;
        const int first = in ? off[t] : 0;
        const int n = in ? max(0, off[t + 1] - first) : 0;
        int incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int at = total + incl - n;
        for (int k = 0; k < n && at + k < C; ++k) o[at + k] = chars[first + k];
        total += __shfl(incl, 63, 64);
        if (stop) break;
    }
    if (lane == 0) lens[r] = total;
}

// ---- the pairs ----
// One wave copies the first l = min(len, C) characters of a row into dst and pads it with CHRF_PAD_R to the end of the 64-character
// chunk that holds the row's end (so a reader may run to the next multiple of four).  Returns l.
__device__ __forceinline__ int chrf_load_row(const int32_t* __restrict__ row, int len, int C, int* dst, int lane) {
    const int l = min(max(len, 0), C);
    const int end = (l + 63) & ~63;                                           // <= CHRF_MAX_C: C <= CHRF_MAX_C, a multiple of 64
    for (int p = lane; p < end; p += 64) dst[p] = p < l ? (row[p] & 0x7fffffff) : CHRF_PAD_R;
    return l;
}

// cnt[n-1] += #{q < lr (SELF: and q < p) : the n-gram ending at q in r equals (h[0], h[1], .., h[n-1]) read backwards from p}.
template <bool SELF>
__device__ __forceinline__ void chrf_walk(const int* r, int lr, int p, const int (&h)[CHRF_ORDER], int (&cnt)[CHRF_ORDER]) {
    int w[CHRF_ORDER];
#pragma unroll
    for (int n = 1; n < CHRF_ORDER; ++n) w[n] = CHRF_PAD_R;
    for (int q = 0; q < lr; q += 4) {
        const int4 t = *reinterpret_cast<const int4*>(r + q);                 // wave-uniform address: a broadcast read
        const int c4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[0] = c4[e];
            bool eq = (h[0] == w[0]) && (!SELF || q + e < p);
            cnt[0] += eq;
#pragma unroll
            for (int n = 1; n < CHRF_ORDER; ++n) {
                eq = eq && h[n] == w[n];
                cnt[n] += eq;
            }
#pragma unroll
            for (int n = CHRF_ORDER - 1; n > 0; --n) w[n] = w[n - 1];
        }
    }
}

// the six characters that end at position p of the candidate in hbuf (length lh)
__device__ __forceinline__ void chrf_tail(const int* hbuf, int lh, int p, int (&h)[CHRF_ORDER]) {
#pragma unroll
    for (int n = 0; n < CHRF_ORDER; ++n) h[n] = (p < lh && p >= n) ? hbuf[p - n] : CHRF_PAD_H;
}

// u of include/vag_nmt.h: every operation rounded on its own
__device__ __forceinline__ float chrf_utility(const int (&m)[CHRF_ORDER], int lh, int lr) {
    float sp = 0.f, sr = 0.f;
    int orders = 0;
#pragma unroll
    for (int n = 1; n <= CHRF_ORDER; ++n) {
        const int th = lh - n + 1, tr = lr - n + 1;
        if (th > 0 && tr > 0) {
            sp = __fadd_rn(sp, __fdiv_rn((float)m[n - 1], (float)th));
            sr = __fadd_rn(sr, __fdiv_rn((float)m[n - 1], (float)tr));
            ++orders;
        }
    }
    if (orders == 0) return 0.f;
    const float P = __fdiv_rn(sp, (float)orders), R = __fdiv_rn(sr, (float)orders);
    if (__fadd_rn(P, R) == 0.f) return 0.f;
    return __fdiv_rn(chrf_mul(chrf_mul(5.f, P), R), __fadd_rn(chrf_mul(4.f, P), R));
}

__global__ __launch_bounds__(64 * CHRF_WAVES) void chrf_pairs_kernel(const int32_t* __restrict__ hchars, const int32_t* __restrict__ hlens,
                                                                     const int32_t* __restrict__ rchars, const int32_t* __restrict__ rlens,
                                                                     const float* __restrict__ weights, float uniform_w, int Nh, int Ch,
                                                                     int Nr, int Cr, int32_t* __restrict__ matches,
                                                                     float* __restrict__ util, float* __restrict__ expected) {
    __shared__ __attribute__((aligned(16))) int hbuf[CHRF_MAX_C];
    __shared__ __attribute__((aligned(16))) int rbuf[CHRF_WAVES][CHRF_MAX_C];
    __shared__ unsigned rank[CHRF_ORDER / 2][CHRF_MAX_C];                     // two 16-bit ranks per word: orders 2k+1, 2k+2
    __shared__ float us[CHRF_MAX_N];
    __shared__ int lh_s;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t bi = blockIdx.x;                                            // b * Nh + i
    const int64_t b = bi / Nh;

    if (wave == 0) {
        const int l = chrf_load_row(hchars + bi * Ch, hlens[bi], Ch, hbuf, lane);
        if (lane == 0) lh_s = l;
    }
    __syncthreads();
    const int lh = lh_s;
    const int chunks = (lh + 63) >> 6;
    for (int c = wave; c < chunks; c += CHRF_WAVES) {                         // the ranks: the candidate against itself
        const int p = c * 64 + lane;
        int h[CHRF_ORDER], cnt[CHRF_ORDER] = {0, 0, 0, 0, 0, 0};
        chrf_tail(hbuf, lh, p, h);
        chrf_walk<true>(hbuf, min(lh, c * 64 + 64), p, h, cnt);              // (q < p: nothing to find past the chunk's end)
#pragma unroll
        for (int k = 0; k < CHRF_ORDER / 2; ++k) rank[k][p] = (unsigned)cnt[2 * k] | ((unsigned)cnt[2 * k + 1] << 16);
    }
    __syncthreads();

    int* rb = rbuf[wave];
    for (int j = wave; j < Nr; j += CHRF_WAVES) {
        chrf_wave_fence();                                                    // the previous reference's reads are done
        const int64_t rj = b * Nr + j;
        const int lr = chrf_load_row(rchars + rj * Cr, rlens[rj], Cr, rb, lane);
        chrf_wave_fence();
        int m[CHRF_ORDER] = {0, 0, 0, 0, 0, 0};
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            int h[CHRF_ORDER], cnt[CHRF_ORDER] = {0, 0, 0, 0, 0, 0};
            chrf_tail(hbuf, lh, p, h);
            chrf_walk<false>(rb, lr, p, h, cnt);
#pragma unroll
            for (int k = 0; k < CHRF_ORDER / 2; ++k) {
                const unsigned rk = rank[k][p];                               // (p < 64 chunks: written above)
                m[2 * k] += __popcll(__ballot((int)(rk & 0xffffu) < cnt[2 * k]));
                m[2 * k + 1] += __popcll(__ballot((int)(rk >> 16) < cnt[2 * k + 1]));
            }
        }
        const float u = chrf_utility(m, lh, lr);                              // (uniform over the wave)
        if (lane == 0) {
            const int64_t o = bi * Nr + j;
            us[j] = u;
            if (util) util[o] = u;
            if (matches) {
#pragma unroll
                for (int n = 0; n < CHRF_ORDER; ++n) matches[o * CHRF_ORDER + n] = m[n];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                   // E_i: fp32, j = 0 .. Nr-1 in order, product and sum
        float e = 0.f;                                                        // rounded separately
        for (int j = 0; j < Nr; ++j) e = __fadd_rn(e, chrf_mul(weights ? weights[b * Nr + j] : uniform_w, us[j]));
        expected[bi] = e;
    }
}

int vag_chrf_supported_host(int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr) {
    return Nh >= 1 && Nh <= CHRF_MAX_N && Nr >= 1 && Nr <= CHRF_MAX_N && Ch >= 1 && Ch <= CHRF_MAX_C && Cr >= 1 && Cr <= CHRF_MAX_C;
}

int vag_chrf_max_chars_host() { return CHRF_MAX_C; }

int vag_surface_expand_launch(const int64_t* rows, int64_t R, int64_t L, const int32_t* off, const int32_t* chars, int64_t V,
                              int32_t* out, int64_t C, int32_t* lens, hipStream_t s) {
    VAG_CHECK_ARG(rows && off && chars && out && lens);
    VAG_CHECK_ARG(R >= 1 && L >= 1 && V >= 1 && C >= 1 && L <= CHRF_MAX_L);
    VAG_CHECK_ARG(R < (1ll << 31) && C < (1ll << 31) && V < (1ll << 31));
    hipLaunchKernelGGL(surface_expand_kernel, dim3((unsigned)((R + CHRF_WAVES - 1) / CHRF_WAVES)), dim3(64 * CHRF_WAVES), 0, s, rows,
                       R, (int)L, off, chars, V, out, (int)C, lens);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_chrf_select_launch(const int32_t* hchars, const int32_t* hlens, const int32_t* rchars, const int32_t* rlens,
                           const float* weights, int64_t B, int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr, int32_t* matches,
                           float* util, float* expected, int64_t* best, hipStream_t s) {
    VAG_CHECK_ARG(hchars && hlens && expected && best);
    VAG_CHECK_ARG(B >= 1 && Nh >= 1 && Ch >= 1 && Nr >= 1 && Cr >= 1);
    VAG_CHECK_ARG(vag_chrf_supported_host(Nh, Ch, Nr, Cr) && B < (1ll << 31) / CHRF_MAX_N);
    VAG_CHECK_ARG((rchars != nullptr) == (rlens != nullptr));
    VAG_CHECK_ARG(rchars || (Nr == Nh && Cr == Ch));
    hipLaunchKernelGGL(chrf_pairs_kernel, dim3((unsigned)(B * Nh)), dim3(64 * CHRF_WAVES), 0, s, hchars, hlens,
                       rchars ? rchars : hchars, rchars ? rlens : hlens, weights, 1.0f / (float)Nr, (int)Nh, (int)Ch, (int)Nr, (int)Cr,
                       matches, util, expected);
    VAG_LAUNCH_CHECK();
    return vag_mbr_best_launch(expected, B, Nh, best, s);
}
