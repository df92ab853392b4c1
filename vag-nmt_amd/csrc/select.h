// Shared by beam.hip and sample.hip: the by-value kernel arguments of M ensemble members and the dispatch from the runtime M to
// the template parameter, the ensemble score of a word, the step index of a (replayed) launch, the total order (value desc,
// index asc), the exact radix top-k of the candidates a wave holds in registers and the sampler's counter-based Gumbel noise.
#pragma once
#include <type_traits>
#include "kernels.h"

struct Cand { float v; int idx; };

// The M models' inputs, by value (a captured graph holds them), sized by M: at M = 1 the kernel arguments are the single
// model's (pointer, leading dimension) and (h_in, h_out, H).  EnsRows: one row-major matrix per member with a common row
// length (log-sum-exp vectors, attention rows).  The host gathers them in EnsHost.
template <int M> struct EnsLogp { const float* p[M]; int64_t ld[M]; };
template <int M> struct EnsHid { const float* in[M]; float* out[M]; int H[M]; };
template <int M> struct EnsRows { const float* p[M]; };
struct EnsHost { const float* p[VAG_ENS_MAX]; int64_t ld[VAG_ENS_MAX]; const float* in[VAG_ENS_MAX]; float* out[VAG_ENS_MAX]; int H[VAG_ENS_MAX]; };

// The ensemble's score from the members' log-probabilities x.  M = 1: x itself.  M > 1: the mean of the M probabilities in log
// space, in the form mx + log(sum / M) -- M identical values give sum == M exactly and return x bit for bit.
template <int M>
__device__ __forceinline__ float ens_combine(const float (&x)[M]) {
    if constexpr (M == 1) {
        return x[0];
    } else {
        float mx = x[0];
#pragma unroll
        for (int m = 1; m < M; ++m) mx = fmaxf(mx, x[m]);
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) sum += expf(x[m] - mx);
        return mx == -INFINITY ? -INFINITY : mx + logf(sum / (float)M);
    }
}

// Score of word w for hypothesis row n: ens_combine of the members' rows.  All M loads are issued before the first use.
template <int M>
__device__ __forceinline__ float ens_score(const EnsLogp<M>& L, int64_t n, int w) {
    float x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = L.p[m][n * L.ld[m] + w];
    return ens_combine<M>(x);
}

// The step index of a launch: from the host (di_host) or, for launches replayed from a HIP graph, from device memory
// (di_state[0], advanced by the kernel that closes the step; such launches are always steps >= 1).  False when there is
// nothing to do: the graph was replayed past the end.
__device__ __forceinline__ bool step_index(const int32_t* di_state, int di_host, int max_len, int& di) {
    di = di_state ? __atomic_load_n(di_state, __ATOMIC_RELAXED) : di_host;
    return !(di >= max_len || (di_state && di < 1));
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// ---- forced decoding (beam.hip: scores and attention of given translations; conf.hip: word-level confidence) ----
constexpr int64_t SPAN_EOS = 3;
// The scored span of a target row y (Tt words) is [0, end]: end = the first EOS, or the last non-pad position if there is none
// (-1 for an all-pad row).  Called by whole waves; every lane returns end.
__device__ __forceinline__ int span_end(const int64_t* __restrict__ y, int Tt) {
    const int lane = threadIdx.x & 63;
    int first_eos = -1, last_nz = -1;
    for (int t0 = 0; t0 < Tt; t0 += 64) {
        const int t = t0 + lane;
        const int64_t w = t < Tt ? y[t] : 0;
        const unsigned long long me = __ballot(t < Tt && w == SPAN_EOS);
        const unsigned long long mn = __ballot(t < Tt && w != 0);
        if (me && first_eos < 0) first_eos = t0 + __ffsll((long long)me) - 1;
        if (mn) last_nz = t0 + 63 - __clzll((long long)mn);
    }
    return first_eos >= 0 ? first_eos : last_nz;
}

// block-wide argmax under the (value desc, index asc) order; result valid in all threads
__device__ __forceinline__ Cand block_best(Cand c, Cand* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(c.v, o, 64);
        const int oi = __shfl_xor(c.idx, o, 64);
        if (better(ov, oi, c.v, c.idx)) { c.v = ov; c.idx = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = c;
    __syncthreads();
    Cand r = sh[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i)
        if (better(sh[i].v, sh[i].idx, r.v, r.idx)) r = sh[i];
    __syncthreads();
    return r;
}

// ---- selection by radix search (round 2; 56-bit unique keys: round 5) ----
// The k best of the candidates one WAVE holds in registers (E per lane), under the total order (value desc, flat index asc),
// without any cross-lane data movement.  A candidate's KEY is its order-preserving value bits followed by its inverted flat
// index (indices are below 2^24: vag_beam_step_launch checks k V < 2^24): keys are unique, a larger key is a better candidate,
// and ties on the value need no handling of their own.  That matters: every continuation of a FINISHED hypothesis except EOS
// carries the same value (its score - 1e5, V11.py:291-294), so once hypotheses have ended whole 2048-candidate slices tie.  With
// 32-bit value keys such slices fell through to an exact search plus a tie loop in every wave: the expansion took 25-32 us
// instead of 12, a beam step of a trained model 120 us instead of 94 (profiles/r05_exp_beam.txt).
__device__ __forceinline__ unsigned fkey(float v) {       // order-preserving float -> uint (larger float, larger key)
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// A key in two words: hi = value bits (0 = hole; fkey(-inf) = 0x007fffff > 0, so a real candidate beats a hole), lo = inverted flat
// index.  The searches below run over the 32 value bits and go on into the 24 index bits only when the k-th value is tied.
struct Key2 { unsigned hi, lo; };
__device__ __forceinline__ Key2 ckey(float v, int idx) {
    Key2 q;
    q.hi = idx == 0x7fffffff ? 0u : fkey(v);
    q.lo = 0xffffffu - ((unsigned)idx & 0xffffffu);
    return q;
}
__device__ __forceinline__ bool key_ge(Key2 a, Key2 t) { return a.hi > t.hi || (a.hi == t.hi && a.lo >= t.lo); }
// the k-th largest of one key per lane (at least k lanes hold a valid key), found bit by bit from ballots
__device__ __forceinline__ Key2 wave_kth_largest(Key2 x, int k) {
    unsigned prefix = 0;
    int need = k;
    for (int b = 31; b >= 0; --b) {
        const unsigned test = prefix | (1u << b);
        const int c = __popcll(__ballot((x.hi >> b) == (test >> b)));
        if (c >= need) prefix = test;
        else need -= c;
    }
    Key2 t = {prefix, 0u};
    if (__popcll(__ballot(x.hi == prefix)) == need) return t;          // no tie on the k-th value: every key of that value counts
    for (int b = 23; b >= 0; --b) {                                     // tie: the `need` smallest indices among the tied lanes
        const unsigned test = t.lo | (1u << b);
        const int c = __popcll(__ballot(x.hi == prefix && (x.lo >> b) == (test >> b)));
        if (c >= need) t.lo = test;
        else need -= c;
    }
    return t;
}
// exact search over all E keys per lane (rare: the bound of wave_topk let more than 64 candidates through)
template <int E>
__device__ __forceinline__ void wave_select(const Key2 (&key)[E], int k, bool (&sel)[E]) {
    int nvalid = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) { nvalid += __popcll(__ballot(key[e].hi != 0u)); sel[e] = false; }
    const int kk = min(k, nvalid);
    if (kk == 0) return;
    unsigned prefix = 0;
    int need = kk;
    for (int b = 31; b >= 0; --b) {
        const unsigned test = prefix | (1u << b);
        int c = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) c += __popcll(__ballot((key[e].hi >> b) == (test >> b)));
        if (c >= need) prefix = test;
        else need -= c;
    }
    Key2 t = {prefix, 0u};
    int neq = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) neq += __popcll(__ballot(key[e].hi == prefix));
    if (neq != need) {
        for (int b = 23; b >= 0; --b) {
            const unsigned test = t.lo | (1u << b);
            int c = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) c += __popcll(__ballot(key[e].hi == prefix && (key[e].lo >> b) == (test >> b)));
            if (c >= need) t.lo = test;
            else need -= c;
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) sel[e] = key[e].hi != 0u && key_ge(key[e], t);      // (keys are unique: exactly kk)
}
// Writes the selected candidates of a wave densely to (ov, oi)[0 .. count): returns count (uniform over the wave).
template <int E>
__device__ __forceinline__ int wave_compact(const float (&val)[E], const int (&idx)[E], const bool (&sel)[E], float* ov, int* oi) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int n = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned long long m = __ballot(sel[e]);
        if (sel[e]) {
            const int pos = n + __popcll(m & lt);
            ov[pos] = val[e]; oi[pos] = idx[e];
        }
        n += __popcll(m);
    }
    return n;
}

// The k best of a wave's candidates, RANKED (ov/oi[0..n): best first), n = min(k, #valid) returned.  Most candidates are
// discarded by a bound that costs 32 ballots whatever E is: the k-th largest of the 64 lane-local maxima is a lower
// bound of the k-th largest overall (those k lane maxima are k distinct candidates), so only candidates >= it can be
// winners -- typically k to 2k survive.  Survivors (<= 64: one per lane) are ranked by counting who beats them; with more
// survivors (heavy ties) the exact radix search over all E takes over.  sv/si: 64 entries of LDS scratch of this wave.
__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
template <int E>
__device__ __forceinline__ int wave_topk(const float (&val)[E], const int (&idx)[E], int k, float* sv, int* si, float* ov, int* oi) {
    const int lane = threadIdx.x & 63;
    Key2 key[E], kb = {0u, 0u};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        key[e] = ckey(val[e], idx[e]);
        if (key[e].hi != 0u && (kb.hi == 0u || !key_ge(kb, key[e]))) kb = key[e];
    }
    Key2 t0 = {1u, 0u};                                 // every valid key has hi > 1
    if (__popcll(__ballot(kb.hi != 0u)) >= k) t0 = wave_kth_largest(kb, k);     // k-th largest of the lane maxima
    bool sel[E];
    int n = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        sel[e] = key[e].hi != 0u && key_ge(key[e], t0);
        n += __popcll(__ballot(sel[e]));
    }
    if (n > 64) {                                       // more than one per lane got through: exact search over everything
        wave_select<E>(key, k, sel);
    }
    n = wave_compact<E>(val, idx, sel, sv, si);
    wave_lds_fence();
    if (lane < n) {
        const float mv = sv[lane];
        const int mi = si[lane];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += better(sv[j], si[j], mv, mi) ? 1 : 0;
        if (rank < k) { ov[rank] = mv; oi[rank] = mi; }
    }
    return min(n, k);
}

// ---- the counter-based Gumbel noise of the sampling decoder (sample.hip) and of the stochastic beam expansion (beam.hip) ----
// The noise of word w under a row's key: g = -log(-log(u)), u = (r + 0.5) 2^-23 with r 23 bits of vag_mix64(key + w); the key is
// mixed from the generator's (seed, call counter), the step index and the row.  vag_sample_noise writes exactly this.
__device__ __forceinline__ uint64_t sample_key(const uint64_t* rng, int di, int64_t row) {
    const uint64_t base = vag_mix64(rng[0] ^ (rng[1] * 0xD1342543DE82EF95ull) ^ (0x53ull << 56));
    return vag_mix64(base ^ (((uint64_t)(uint32_t)di << 32) | (uint64_t)(uint32_t)row));
}
__device__ __forceinline__ float sample_gumbel(uint64_t key, int w) {
    const uint64_t r = vag_mix64(key + (uint64_t)w) >> 41;                              // 23 bits
    const float u = __fmul_rn(__fadd_rn((float)r, 0.5f), 1.0f / 8388608.0f);           // exact: in [2^-24, 1 - 2^-24]
    return -logf(-logf(u));
}

// host arrays of M entries -> the by-value kernel arguments; every entry is checked before anything is enqueued
static int ens_logp_args(const float* const* logp, const int64_t* ldl, int64_t M, int64_t V, EnsHost& a) {
    VAG_CHECK_ARG(logp && ldl && M >= 1 && M <= VAG_ENS_MAX && V > 0);
    a = EnsHost{};
    for (int m = 0; m < (int)M; ++m) {
        VAG_CHECK_ARG(logp[m] && ldl[m] >= V);
        a.p[m] = logp[m]; a.ld[m] = ldl[m];
    }
    return VAG_OK;
}

template <int M>
static EnsLogp<M> ens_logp(const EnsHost& a) {
    EnsLogp<M> in;
    for (int m = 0; m < M; ++m) { in.p[m] = a.p[m]; in.ld[m] = a.ld[m]; }
    return in;
}
template <int M>
static EnsHid<M> ens_hid(const EnsHost& a) {
    EnsHid<M> hid;
    for (int m = 0; m < M; ++m) { hid.in[m] = a.in[m]; hid.out[m] = a.out[m]; hid.H[m] = a.H[m]; }
    return hid;
}
template <int M>
static EnsRows<M> ens_rows(const float* const* p) {
    EnsRows<M> r;
    for (int m = 0; m < M; ++m) r.p[m] = p[m];
    return r;
}

// The runtime M (checked: 1 .. VAG_ENS_MAX) as a compile-time constant: returns f(std::integral_constant<int, M>{}), which
// instantiates f for every M the interface admits.
template <int N = VAG_ENS_MAX, class F>
static int ens_dispatch(int M, F&& f) {
    static_assert(N >= 1 && N <= VAG_ENS_MAX, "ens_dispatch walks M = VAG_ENS_MAX .. 1");
    if (M == N) return f(std::integral_constant<int, N>{});
    if constexpr (N > 1) return ens_dispatch<N - 1>(M, f);
    else return VAG_EINVAL;
}
