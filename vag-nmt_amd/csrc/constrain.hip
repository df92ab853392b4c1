// Constrained beam search (vag_nmt.h: vag_beam_constrain): target prefixes, banned phrases and no-repeat n-grams as a mask over
// the members' log-probability rows, written BEFORE the step's expansion reads them.  A launch of its own, not a variant of
// stage 1: the expansions (plain, diverse) keep their code objects and every one of them can take the mask.
//   one 256-thread workgroup per hypothesis row (b, j); N = B rows at step 0, B k afterwards.
//   history: lane 0 walks the row's back-pointers from step di-1 down to 0 -- a chain of dependent loads, a hop's word and
//            parent issued together -- and stages the words in LDS as int32 (max_len <= 1024).
//   forced:  a row whose prefix still has a word f for this step is a block-stride fill of -1e5 over [0, V) that skips f: no
//            read-keep-write, nothing to order inside the block.  Bans are not looked at.
//   bans:    otherwise the lanes split the phrase list and the history positions between them; a ban is a store of -1e5 into
//            every member's row.  The stores are idempotent, so lanes that ban the same word need no arbitration.
// Columns [V, ldl) are never written, a finished row (previous word EOS) is left to the expansion's own rule.
#include "kernels.h"
#include "select.h"

constexpr float CON_NEG_PEN = -1e5f;     // the reference's "inf" (V11.py:257): what the expansions' own penalties write
constexpr int64_t CON_EOS = 3;
constexpr int CON_MAX_HIST = 1024;       // words of history staged in LDS

// the M members' rows, writable, by value (a captured graph holds them)
template <int M> struct ConRows { float* p[M]; int64_t ld[M]; };

template <int M>
__device__ __forceinline__ void con_ban(const ConRows<M>& L, int64_t n, int64_t w, int V) {
    if (w < 0 || w >= V) return;
#pragma unroll
    for (int m = 0; m < M; ++m) L.p[m][n * L.ld[m] + w] = CON_NEG_PEN;
}

template <int M>
__global__ __launch_bounds__(256) void beam_constrain_kernel(ConRows<M> L, const int64_t* __restrict__ beam,
                                                             const int32_t* di_state, int di_host, int max_len, int B, int k,
                                                             int V, const int64_t* __restrict__ prefix, int Lp,
                                                             const int64_t* __restrict__ phrases,
                                                             const int32_t* __restrict__ phrase_sent, int P, int ngram) {
    __shared__ int h[CON_MAX_HIST];
    // the step index the expansion that follows will read (it advances it; this launch only reads)
    const int di = di_state ? __atomic_load_n(di_state, __ATOMIC_RELAXED) : di_host;
    if (di < 0 || di >= max_len) return;
    const int k_in = di == 0 ? 1 : k;
    const int64_t n = blockIdx.x;                                  // hypothesis row b * k_in + j
    if (n >= (int64_t)B * k_in) return;                            // (a device-side step 0: the grid is sized for B k rows)
    const int b = (int)(n / k_in);
    if (threadIdx.x == 0) {
        int s = (int)(n - (int64_t)b * k_in);
        for (int t = di - 1; t >= 0; --t) {
            const int64_t o = ((int64_t)t * B + b) * k + s;
            const int64_t w = beam[o];
            const int64_t p = beam[o + (int64_t)max_len * B * k];
            h[t] = (int)w;
            s = min(max((int)p, 0), k - 1);                        // (a back-pointer is a slot; never index outside the row)
        }
    }
    __syncthreads();
    if (di >= 1 && h[di - 1] == CON_EOS) return;                   // finished: the expansion's rule (:291-294) overrides anyway
    if (di < Lp) {
        const int64_t f = prefix[(int64_t)b * Lp + di];
        if (f >= 1 && f < V) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float* __restrict__ row = L.p[m] + n * L.ld[m];
                for (int w = threadIdx.x; w < V; w += 256)
                    if (w != (int)f) row[w] = CON_NEG_PEN;
            }
            return;
        }
    }
    for (int p = threadIdx.x; p < P; p += 256) {
        const int sent = phrase_sent[p];
        if (sent != -1 && sent != b) continue;
        int64_t ph[VAG_CONSTRAIN_MAX_LEN];
        int len = VAG_CONSTRAIN_MAX_LEN;
#pragma unroll
        for (int i = 0; i < VAG_CONSTRAIN_MAX_LEN; ++i) ph[i] = phrases[(int64_t)p * VAG_CONSTRAIN_MAX_LEN + i];
#pragma unroll
        for (int i = VAG_CONSTRAIN_MAX_LEN - 1; i >= 0; --i)
            if (ph[i] == 0) len = i;                               // leading non-zero words
        if (len == 0 || len - 1 > di) continue;
        bool hit = true;
        int64_t last = ph[0];
#pragma unroll
        for (int i = 0; i < VAG_CONSTRAIN_MAX_LEN; ++i) {
            if (i < len - 1) hit = hit && (int64_t)h[di - len + 1 + i] == ph[i];
            if (i == len - 1) last = ph[i];
        }
        if (hit) con_ban<M>(L, n, last, V);
    }
    if (ngram >= 1) {
        const int c = ngram - 1;                                   // context words; the current context is h[di-c .. di-1]
        for (int t = threadIdx.x; t + ngram <= di; t += 256) {
            bool hit = true;
            for (int i = 0; i < c; ++i) hit = hit && h[t + i] == h[di - c + i];
            if (hit) con_ban<M>(L, n, (int64_t)h[t + c], V);
        }
    }
}

int vag_beam_constrain_launch(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di,
                              const int32_t* di_state, bool dev_form, int64_t max_len, int64_t B, int64_t k, int64_t V,
                              const int64_t* prefix, int64_t Lp, const int64_t* phrases, const int32_t* phrase_sent, int64_t P,
                              int64_t ngram, hipStream_t s) {
    VAG_CHECK_ARG(logp && ldl && M >= 1 && M <= VAG_ENS_MAX);
    VAG_CHECK_ARG(B > 0 && k > 0 && k <= 64 && V > 0 && max_len > 0 && max_len <= CON_MAX_HIST);
    VAG_CHECK_ARG(V < (1ll << 31) && B * k < (1ll << 31));
    for (int m = 0; m < (int)M; ++m) VAG_CHECK_ARG(logp[m] && ldl[m] >= V);
    VAG_CHECK_ARG(beam != nullptr);
    if (dev_form) VAG_CHECK_ARG(di_state != nullptr);
    else VAG_CHECK_ARG(di >= 0 && di < max_len);
    VAG_CHECK_ARG(Lp >= 0 && Lp < (1ll << 31) && (Lp == 0 || prefix));
    VAG_CHECK_ARG(P >= 0 && P <= VAG_CONSTRAIN_MAX_PHRASES && (P == 0 || (phrases && phrase_sent)));
    VAG_CHECK_ARG(ngram >= 0 && ngram <= VAG_CONSTRAIN_MAX_LEN);
    if (Lp == 0 && P == 0 && ngram == 0) return VAG_OK;           // nothing to rule out: no launch
    const int64_t rows = (!dev_form && di == 0) ? B : B * k;
    return ens_dispatch((int)M, [&](auto mm) -> int {
        constexpr int MM = decltype(mm)::value;
        ConRows<MM> L;
        for (int m = 0; m < MM; ++m) { L.p[m] = logp[m]; L.ld[m] = ldl[m]; }
        hipLaunchKernelGGL(beam_constrain_kernel<MM>, dim3((unsigned)rows), dim3(256), 0, s, L, beam,
                           dev_form ? di_state : nullptr, (int)di, (int)max_len, (int)B, (int)k, (int)V, prefix, (int)Lp, phrases,
                           phrase_sent, (int)P, (int)ngram);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}
