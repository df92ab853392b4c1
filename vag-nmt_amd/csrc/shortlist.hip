// Lexical shortlists (vag_nmt.h: vag_shortlist_*): the per-batch compact target vocabulary and what moves a decoder onto it.
//   select: ONE 1024-thread workgroup.  A bitmap over the V target words lives in LDS (V <= 131 072: 4096 words, 16 KB).  The
//           `always` ids are marked with LDS atomic ORs, then the lexicon's ranks one after another: rank r of every source word
//           inside its sentence's length goes into a second bitmap of that rank's NEW words, counted as they are claimed (the
//           atomic OR's return value says who claimed a bit, so a duplicate counts once).  A rank whose new words would push the
//           count over `cap` is dropped with every later rank -- the decision reads a count, never an order, so the result is
//           the same whatever the lanes' timing.  The words' popcounts are then scanned (each lane its run of words, a
//           Hillis-Steele scan over the lanes' sums) and every target id looks its compact id up: ids ascending, full2short
//           monotone.  Integer LDS atomics only; nothing is read back by the host.
//   gather: row j < n of the output is row ids[j] of the source, bit for bit; rows n .. cap-1 take the pad value, at every call
//           (n moves from batch to batch).  16-byte loads and stores where the width, the stride and both addresses allow.
//   map:    an int64 token tensor through ids (compact -> full) or full2short (full -> compact; an absent word becomes UNK and
//           counts: one LDS atomic per absent word, one global integer atomic per workgroup that met any).
#include "kernels.h"

constexpr int SL_THREADS = 1024;
constexpr int64_t SL_MAX_V = 131072;
constexpr int SL_MAX_WORDS = (int)(SL_MAX_V / 32);
constexpr int64_t SL_MAX_K = 256;
constexpr int64_t SL_UNK = 1;

__global__ __launch_bounds__(SL_THREADS) void shortlist_select_kernel(
    const int64_t* __restrict__ src, const int32_t* __restrict__ lengths, int B, int Ts, const int32_t* __restrict__ lex, int Vs,
    int K, int best, const int32_t* __restrict__ always, int A, int V, int cap, int32_t* __restrict__ ids,
    int32_t* __restrict__ n_out, int32_t* __restrict__ rank_out, int32_t* __restrict__ full2short) {
    __shared__ unsigned bits[SL_MAX_WORDS];       // the chosen words
    __shared__ unsigned pend[SL_MAX_WORDS];       // a rank's new words; after the ranks: every word's exclusive prefix count
    __shared__ int part[SL_THREADS];
    __shared__ int s_count, s_new;
    const int tid = threadIdx.x;
    const int W = (V + 31) >> 5;
    for (int w = tid; w < W; w += SL_THREADS) { bits[w] = 0u; pend[w] = 0u; }
    if (tid == 0) { s_count = 0; s_new = 0; }
    __syncthreads();
    for (int i = tid; i < A; i += SL_THREADS) {
        const int w = always[i];
        if (w < 0 || w >= V) continue;
        const unsigned m = 1u << (w & 31);
        if (!(atomicOr(&bits[w >> 5], m) & m)) atomicAdd(&s_count, 1);
    }
    __syncthreads();
    int count = s_count, used = 0;
    const int BT = B * Ts;
    for (int r = 0; r < best; ++r) {
        for (int i = tid; i < BT; i += SL_THREADS) {
            const int b = i / Ts;
            if (i - b * Ts >= lengths[b]) continue;                    // padding positions do not count, whatever they hold
            const int64_t s = src[i];
            if (s < 0 || s >= Vs) continue;
            const int w = lex[s * K + r];
            if (w < 0 || w >= V) continue;
            const unsigned m = 1u << (w & 31);
            if (bits[w >> 5] & m) continue;
            if (!(atomicOr(&pend[w >> 5], m) & m)) atomicAdd(&s_new, 1);
        }
        __syncthreads();
        const int add = s_new;
        __syncthreads();                                               // (everyone has read it before lane 0 clears it)
        if (count + add > cap) break;                                  // the same for every lane: this rank and the later ones drop
        for (int w = tid; w < W; w += SL_THREADS) {
            const unsigned p = pend[w];
            if (p) { bits[w] |= p; pend[w] = 0u; }
        }
        if (tid == 0) s_new = 0;
        count += add;
        used = r + 1;
        __syncthreads();
    }
    // every lane its run of CH consecutive words, then the lanes' sums
    const int CH = (W + SL_THREADS - 1) / SL_THREADS;
    const int w0 = tid * CH;
    int local = 0;
    for (int j = 0; j < CH; ++j)
        if (w0 + j < W) local += __popc(bits[w0 + j]);
    part[tid] = local;
    __syncthreads();
    for (int off = 1; off < SL_THREADS; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - local;
    for (int j = 0; j < CH; ++j)
        if (w0 + j < W) { pend[w0 + j] = (unsigned)run; run += __popc(bits[w0 + j]); }
    __syncthreads();
    for (int v = tid; v < V; v += SL_THREADS) {
        const unsigned wd = bits[v >> 5], m = 1u << (v & 31);
        int idx = -1;
        if (wd & m) {
            idx = (int)pend[v >> 5] + __popc(wd & (m - 1u));
            if (idx < cap) ids[idx] = v;                               // (count <= cap by construction; never past the buffer)
        }
        full2short[v] = idx;
    }
    for (int j = count + tid; j < cap; j += SL_THREADS) ids[j] = -1;
    if (tid == 0) { n_out[0] = count; rank_out[0] = used; }
}

template <bool VEC>
__global__ __launch_bounds__(256) void shortlist_gather_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ n_ptr,
                                                               int cap, const float* __restrict__ src, int V, int W, int64_t ld,
                                                               float pad, float* __restrict__ out) {
    const int n = min(max(n_ptr[0], 0), cap);
    const int Wc = VEC ? W / 4 : W;                                    // columns in units of one access
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)cap * Wc) return;
    const int row = (int)(i / Wc), c = (int)(i - (int64_t)row * Wc);
    const int id = row < n ? ids[row] : -1;
    const bool live = id >= 0 && id < V;
    if (VEC) {
        f32x4 v = {pad, pad, pad, pad};
        if (live) v = reinterpret_cast<const f32x4*>(src + (int64_t)id * ld)[c];
        reinterpret_cast<f32x4*>(out)[i] = v;
    } else {
        out[i] = live ? src[(int64_t)id * ld + c] : pad;
    }
}

__global__ __launch_bounds__(256) void shortlist_map_kernel(const int64_t* __restrict__ x, int64_t N,
                                                            const int32_t* __restrict__ table, int len, int to_short,
                                                            int64_t* __restrict__ out, int32_t* absent) {
    __shared__ int s_absent;
    if (threadIdx.x == 0) s_absent = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        const int64_t v = x[i];
        int64_t o = -1;
        if (v >= 0 && v < len) o = table[v];
        if (o < 0) {
            o = SL_UNK;
            if (to_short) atomicAdd(&s_absent, 1);
        }
        out[i] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_absent > 0 && absent) atomicAdd(absent, s_absent);
}

extern "C" {

int vag_shortlist_supported(int64_t V, int64_t Vs, int64_t K, int64_t cap) {
    return (V >= 8 && V <= SL_MAX_V && Vs >= 1 && Vs < (1ll << 31) / SL_MAX_K && K >= 1 && K <= SL_MAX_K && cap >= 8 && cap <= V)
               ? 1 : 0;
}

int vag_shortlist_select(const int64_t* src, const int32_t* lengths, int64_t B, int64_t Ts, const int32_t* lex, int64_t Vs,
                         int64_t K, int64_t best, const int32_t* always, int64_t A, int64_t V, int64_t cap, int32_t* ids,
                         int32_t* n, int32_t* rank_used, int32_t* full2short, vag_stream_t stream) {
    VAG_CHECK_ARG(src && lengths && lex && ids && n && rank_used && full2short);
    VAG_CHECK_ARG(vag_shortlist_supported(V, Vs, K, cap));
    VAG_CHECK_ARG(B >= 1 && Ts >= 1 && B * Ts < (1ll << 31) && B < (1ll << 31) && Ts < (1ll << 31));
    VAG_CHECK_ARG(best >= 0 && best <= K);
    VAG_CHECK_ARG(A >= 0 && A <= cap && (A == 0 || always));
    hipLaunchKernelGGL(shortlist_select_kernel, dim3(1), dim3(SL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, lengths,
                       (int)B, (int)Ts, lex, (int)Vs, (int)K, (int)best, always, (int)A, (int)V, (int)cap, ids, n, rank_used,
                       full2short);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_shortlist_gather(const int32_t* ids, const int32_t* n, int64_t cap, const float* src, int64_t V, int64_t W, int64_t ld,
                         float pad, float* out, vag_stream_t stream) {
    VAG_CHECK_ARG(ids && n && src && out);
    VAG_CHECK_ARG(V >= 1 && V <= SL_MAX_V && cap >= 1 && cap <= SL_MAX_V && W >= 1 && W < (1ll << 24) && ld >= W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool vec = W % 4 == 0 && ld % 4 == 0 && aligned16(src) && aligned16(out);
    const int64_t items = cap * (vec ? W / 4 : W);
    const unsigned grid = (unsigned)cdiv64(items, 256);
    if (vec)
        hipLaunchKernelGGL(shortlist_gather_kernel<true>, dim3(grid), dim3(256), 0, s, ids, n, (int)cap, src, (int)V, (int)W, ld,
                           pad, out);
    else
        hipLaunchKernelGGL(shortlist_gather_kernel<false>, dim3(grid), dim3(256), 0, s, ids, n, (int)cap, src, (int)V, (int)W, ld,
                           pad, out);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_shortlist_map(const int64_t* x, int64_t N, const int32_t* table, int64_t len, int to_short, int64_t* out, int32_t* absent,
                      vag_stream_t stream) {
    VAG_CHECK_ARG(N >= 0 && N < (1ll << 39) && table && len >= 1 && len <= SL_MAX_V && (to_short == 0 || to_short == 1));
    if (N == 0) return VAG_OK;
    VAG_CHECK_ARG(x && out);
    hipLaunchKernelGGL(shortlist_map_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                       N, table, (int)len, to_short, out, absent);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

}  // extern "C"
