// Word-level confidence from forced decoding (include/vag_nmt.h: vag_token_conf): what the model thought of every word of a
// GIVEN translation -- the softmax entropy of the position, the rank of the given word, the two best words and their scores --
// and the sentence's quality-estimation features (Fomicheva et al. 2020) reduced from them.  The inputs are vag_forced_score's:
// M members' teacher-forced raw logits and their rows' log-sum-exp.
//   rows       one workgroup per (t, b) row.  A row outside its sentence's span writes the "outside" values and leaves.  The
//              others gather s_y, then read the M members' rows ONCE: word j scores s_j = ens_combine_m(logits_m[j] - lse_m)
//              (select.h), and every lane keeps, over the words it meets in column order, the partial sum of p_j s_j
//              (p_j = expf(s_j); a word of probability 0 adds exactly 0), the count of words ahead of the given one under the
//              total order (score desc, word asc) and its two best words.  Lanes are combined in a fixed wave tree, the four
//              waves in wave order through LDS: two runs give the same bits, no atomics.  16-byte loads where every member's
//              row is 16-byte aligned (a scalar tail for V % 4 words), scalar loads where one is not.
//   sentences  one wave per sentence reduces the positions' values in position order (logp and score exactly as
//              forced_score_kernel forms them: the same additions in the same order on the same numbers).
#include "kernels.h"
#include "select.h"

namespace {

constexpr int CONF_NONE = 0x7fffffff;       // the word of an empty top-2 slot: loses to every word of [0, V) under better()

// what a lane, then a wave, then the row knows: sum_j p_j s_j, #{j ahead of the given word}, the best two words seen
struct ConfAcc {
    float ps;
    int ahead;
    Cand t1, t2;
};

__device__ __forceinline__ void conf_push(ConfAcc& a, float s, int j) {
    if (better(s, j, a.t1.v, a.t1.idx)) { a.t2 = a.t1; a.t1 = {s, j}; }
    else if (better(s, j, a.t2.v, a.t2.idx)) a.t2 = {s, j};
}

// one word: its term of the entropy, whether it is ahead of the given word (sy, y), its place among the best two
__device__ __forceinline__ void conf_word(ConfAcc& a, float s, int j, float sy, int y) {
    const float p = expf(s);
    a.ps += p == 0.f ? 0.f : p * s;                                             // s == -inf: p == 0, the term is 0 (not 0 * inf)
    a.ahead += better(s, j, sy, y) ? 1 : 0;
    conf_push(a, s, j);
}

// b's words join a's (the two hold disjoint sets of words)
__device__ __forceinline__ void conf_merge_top(ConfAcc& a, const Cand& b1, const Cand& b2) {
    conf_push(a, b1.v, b1.idx);
    conf_push(a, b2.v, b2.idx);                                                 // (b2 is no better than b1: pushing b1 first is right)
}

template <int M>
__device__ __forceinline__ float conf_score(const float (&x)[M], const float (&lse)[M]) {
    float d[M];
#pragma unroll
    for (int m = 0; m < M; ++m) d[m] = __fsub_rn(x[m], lse[m]);
    return ens_combine<M>(d);
}

// VEC: every member's row starts 16-byte aligned (base aligned, ldl[m] % 4 == 0).  Output index g = b * Tt + t (sentence-major).
template <int M, bool VEC>
__global__ __launch_bounds__(256) void conf_rows_kernel(EnsLogp<M> L, EnsRows<M> S, const int64_t* __restrict__ tgt, int B, int Tt,
                                                        int V, float* __restrict__ token_logp, float* __restrict__ entropy,
                                                        int32_t* __restrict__ rank, int32_t* __restrict__ top,
                                                        float* __restrict__ top_logp) {
    __shared__ ConfAcc sh[4];
    const int64_t row = blockIdx.x;
    const int t = (int)(row / B), b = (int)(row - (int64_t)t * B);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* yrow = tgt + (int64_t)b * Tt;
    const int end = span_end(yrow, Tt);                                         // (every wave scans the sentence: no exchange)
    const int64_t y64 = yrow[t];
    const int64_t g = (int64_t)b * Tt + t;
    const bool in = t <= end && y64 != 0;
    if (!in || y64 < 0 || y64 >= V) {                                           // uniform over the workgroup
        if (tid == 0) {
            const float f = in ? NAN : 0.f;                                     // a word outside [0, V): NaN / -1, never a stray read
            token_logp[g] = f; entropy[g] = f; rank[g] = -1;
            top[2 * g] = -1; top[2 * g + 1] = -1; top_logp[2 * g] = f; top_logp[2 * g + 1] = f;
        }
        return;
    }
    const int y = (int)y64;
    float lse[M];
    const float* base[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { lse[m] = S.p[m][row]; base[m] = L.p[m] + row * L.ld[m]; }
    float sy;
    {
        float x[M];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = base[m][y];
        sy = conf_score<M>(x, lse);
    }
    ConfAcc a = {0.f, 0, {-INFINITY, CONF_NONE}, {-INFINITY, CONF_NONE}};
    if constexpr (VEC) {
        const int nv = V >> 2;                                                  // whole groups of four words
        for (int q = tid; q < nv; q += 256) {
            float4 x4[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x4[m] = reinterpret_cast<const float4*>(base[m])[q];    // all M loads before the first use
            float x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = x4[m].x;
            conf_word(a, conf_score<M>(x, lse), 4 * q, sy, y);
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = x4[m].y;
            conf_word(a, conf_score<M>(x, lse), 4 * q + 1, sy, y);
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = x4[m].z;
            conf_word(a, conf_score<M>(x, lse), 4 * q + 2, sy, y);
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = x4[m].w;
            conf_word(a, conf_score<M>(x, lse), 4 * q + 3, sy, y);
        }
        const int j = 4 * nv + tid;                                             // the tail: V % 4 words, after every lane's groups
        if (j < V) {
            float x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = base[m][j];
            conf_word(a, conf_score<M>(x, lse), j, sy, y);
        }
    } else {
        for (int j = tid; j < V; j += 256) {
            float x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = base[m][j];
            conf_word(a, conf_score<M>(x, lse), j, sy, y);
        }
    }
    // the wave: the sum in wave_sum's fixed tree, the count in integers, the best two by a butterfly of better()
    a.ps = wave_sum(a.ps);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.ahead += __shfl_xor(a.ahead, o, 64);
        const Cand b1 = {__shfl_xor(a.t1.v, o, 64), __shfl_xor(a.t1.idx, o, 64)};
        const Cand b2 = {__shfl_xor(a.t2.v, o, 64), __shfl_xor(a.t2.idx, o, 64)};
        conf_merge_top(a, b1, b2);
    }
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (tid != 0) return;
    ConfAcc r = sh[0];
    for (int w = 1; w < 4; ++w) {                                               // waves in wave order
        r.ps += sh[w].ps;
        r.ahead += sh[w].ahead;
        conf_merge_top(r, sh[w].t1, sh[w].t2);
    }
    token_logp[g] = sy;
    entropy[g] = -r.ps;
    rank[g] = r.ahead;
    top[2 * g] = r.t1.idx; top[2 * g + 1] = r.t2.idx;                           // V >= 2: both slots hold a word
    top_logp[2 * g] = r.t1.v; top_logp[2 * g + 1] = r.t2.v;
}

// acc += v of lanes 0 .. 63, in lane order (forced_score_kernel's sum over a chunk of 64 positions)
__device__ __forceinline__ float lane_order_add(float acc, float v) {
    for (int i = 0; i < 64; ++i) acc += __shfl(v, i, 64);
    return acc;
}

// One wave per sentence over what the row kernel wrote.  sent (B, VAG_CONF_SENT): logp, score (forced_score_kernel's, bit for
// bit), n, the population standard deviation of the span's token_logp (two passes), its minimum, the mean and the maximum of the
// entropy, the share of positions whose word is the model's first choice.
__global__ __launch_bounds__(64) void conf_sent_kernel(const int64_t* __restrict__ tgt, int Tt, const float* __restrict__ token_logp,
                                                       const float* __restrict__ entropy, const int32_t* __restrict__ rank,
                                                       float* __restrict__ sent) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* y = tgt + (int64_t)b * Tt;
    const float* lp = token_logp + (int64_t)b * Tt;
    const float* en = entropy + (int64_t)b * Tt;
    const int32_t* rk = rank + (int64_t)b * Tt;
    const int end = span_end(y, Tt);
    float acc = 0.f, esum = 0.f, lmin = INFINITY, emax = -INFINITY;
    int words = 0, n = 0, first = 0;
    for (int t0 = 0; t0 <= end; t0 += 64) {
        const int t = t0 + lane;
        const int64_t w = t < Tt ? y[t] : 0;
        const bool in = t <= end && w != 0;
        const float v = in ? lp[t] : 0.f, h = in ? en[t] : 0.f;
        words += __popcll(__ballot(in && w > 3));
        n += __popcll(__ballot(in));
        first += __popcll(__ballot(in && rk[t] == 0));
        acc = lane_order_add(acc, v);                                            // in t order (positions past the span add 0)
        esum = lane_order_add(esum, h);
        if (in) { lmin = fminf(lmin, v); emax = fmaxf(emax, h); }
    }
    float dev2 = 0.f;
    const float mean = acc / (float)(n < 1 ? 1 : n);
    for (int t0 = 0; t0 <= end; t0 += 64) {                                     // second pass: squared deviations from the mean
        const int t = t0 + lane;
        const bool in = t <= end && (t < Tt ? y[t] : 0) != 0;
        const float d = in ? lp[t] - mean : 0.f;
        dev2 = lane_order_add(dev2, d * d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lmin = fminf(lmin, __shfl_xor(lmin, o, 64));
        emax = fmaxf(emax, __shfl_xor(emax, o, 64));
    }
    if (lane != 0) return;
    float* o = sent + (int64_t)b * VAG_CONF_SENT;
    const float fn = (float)n;
    o[0] = acc;
    o[1] = acc / (float)(words < 1 ? 1 : words);
    o[2] = fn;
    o[3] = n ? sqrtf(dev2 / fn) : 0.f;
    o[4] = n ? lmin : 0.f;
    o[5] = n ? esum / fn : 0.f;
    o[6] = n ? emax : 0.f;
    o[7] = n ? (float)first / fn : 0.f;
}

}  // namespace

int vag_token_conf_launch(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, const int64_t* tgt,
                          int64_t B, int64_t Tt, int64_t V, float* token_logp, float* entropy, int32_t* rank, int32_t* top,
                          float* top_logp, float* sent, hipStream_t s) {
    EnsHost a;
    VAG_TRY(ens_logp_args(logits, ldl, M, V, a));                               // NULL array or entry, M outside [1, VAG_ENS_MAX], ldl[m] < V
    VAG_CHECK_ARG(lse && tgt && token_logp && entropy && rank && top && top_logp && sent);
    VAG_CHECK_ARG(B > 0 && Tt > 0 && V >= 2 && V < (1ll << 24));                // two best words exist; vag_kd_targets' bound on V
    VAG_CHECK_ARG(B < (1ll << 31) && Tt < (1ll << 31) && B * Tt < (1ll << 31)); // one workgroup per row
    bool vec = true;
    for (int m = 0; m < (int)M; ++m) {
        VAG_CHECK_ARG(lse[m] != nullptr);
        vec = vec && aligned16(logits[m]) && (ldl[m] & 3) == 0;
    }
    VAG_TRY(ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        if (vec)
            hipLaunchKernelGGL((conf_rows_kernel<MM, true>), dim3((unsigned)(B * Tt)), dim3(256), 0, s, ens_logp<MM>(a),
                               ens_rows<MM>(lse), tgt, (int)B, (int)Tt, (int)V, token_logp, entropy, rank, top, top_logp);
        else
            hipLaunchKernelGGL((conf_rows_kernel<MM, false>), dim3((unsigned)(B * Tt)), dim3(256), 0, s, ens_logp<MM>(a),
                               ens_rows<MM>(lse), tgt, (int)B, (int)Tt, (int)V, token_logp, entropy, rank, top, top_logp);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }));
    hipLaunchKernelGGL(conf_sent_kernel, dim3((unsigned)B), dim3(64), 0, s, tgt, (int)Tt, token_logp, entropy, rank, sent);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
