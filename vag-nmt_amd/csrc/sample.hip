// Sampling decoder step: draws every hypothesis row's next word from the (ensemble's) distribution, tempered and optionally cut to
// its top_k best words, without host syncs.  One launch per decoder step, one block of 256 threads per OUTPUT row.
//   score       s[n,w] = ens_score (select.h): the row itself at M = 1, the mean of the members' probabilities in log space else
//   candidates  top_k = 0: every word; else the top_k best words under (s desc, word asc), by select.h's exact radix top-k: each
//               wave keeps a running ranked top-k of the 512-word slices it walks, wave 0 merges the four lists
//   draw        Gumbel-max: tok = argmax_w ( s[n,w] * inv_T + g(n,w) ), the product and the sum rounded separately, ties to the
//               lowest word; g = -log(-log(u)), u = (r + 0.5) 2^-23 with r 23 bits of vag_mix64(key + w), key mixed from the
//               generator's (seed, call counter), the step index and the output row.  23 bits, not 24: u = 1 - 2^-25 would round
//               to 1.0f and g to +inf.
// The row is read once: the thread that owns the winner has kept its untempered score, which is the step's token_logp.
// A row whose previous word is EOS emits EOS at log-probability 0 (the rule of a finished beam hypothesis, V11.py:291-294).
// Step 0 fans every source row out to n samples (its n output rows read the same input row and draw with their own keys) and
// replicates the members' hidden states; at later steps rows map one to one and the hidden states are not touched: the state a
// member's decoder step wrote IS the next step's input.
// The history (words and their log-probabilities, (max_len, B n) each) is indexed by the step (select.h's step_index; the
// last block to finish advances di_state[0]).
// Nucleus (top-p) sampling is a kernel of its own (sample_step_p_kernel, below) with the same launch shape: the draw restricted
// to the smallest set of best words, whole tie groups, that carries top_p of the candidates' tempered mass.
#include "kernels.h"
#include "select.h"

constexpr int64_t EOS = 3;
constexpr int SEPT = 8;                  // words per lane and round of the top-k path (a wave walks slices of 64 * SEPT words)
constexpr int SLICE = 64 * SEPT;

// the noise itself (sample_key, sample_gumbel): select.h, shared with the stochastic beam expansion
__device__ __forceinline__ float sample_perturb(float s, float inv_T, float g) { return __fadd_rn(__fmul_rn(s, inv_T), g); }

// step 0: the members' states, replicated by source row
template <int M>
__device__ __forceinline__ void sample_replicate(const EnsHid<M>& hid, int64_t row, int64_t n_in) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int H = hid.H[m];
        for (int c = threadIdx.x; c < H; c += 256) hid.out[m][row * H + c] = hid.in[m][n_in * H + c];
    }
}

// The top_k best words of input row n_in, ranked, in wv / wi[0, nc): each wave keeps a running ranked top-k of the slices it
// walks, wave 0 merges the four lists.  Returns nc in wave 0 and -1 in the other waves, which have nothing left to do.
// wv, sv, wi, si: stage 1 of the beam expansion's LDS, four arrays of 4 x 64 words.
template <int M>
__device__ __forceinline__ int sample_pool(const EnsLogp<M>& L, int64_t n_in, int V, int top_k, float* wv, float* sv, int* wi, int* si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ov = wv + wave * 64;
    int* oi = wi + wave * 64;
    int cnt = 0;                                                                // ranked entries in (ov, oi), uniform over the wave
    for (int base = wave * SLICE; base < V; base += 4 * SLICE) {
        float val[SEPT + 1];
        int idx[SEPT + 1];
#pragma unroll
        for (int e = 0; e < SEPT; ++e) {                                        // all M * SEPT loads in flight together (index clamped)
            const int w = base + e * 64 + lane;
            const float s = ens_score<M>(L, n_in, min(w, V - 1));
            val[e] = w < V ? s : -INFINITY;
            idx[e] = w < V ? w : 0x7fffffff;
        }
        val[SEPT] = lane < cnt ? ov[lane] : -INFINITY;
        idx[SEPT] = lane < cnt ? oi[lane] : 0x7fffffff;
        wave_lds_fence();
        cnt = wave_topk<SEPT + 1>(val, idx, top_k, sv + wave * 64, si + wave * 64, ov, oi);
        wave_lds_fence();
    }
    if (lane >= cnt) { ov[lane] = -INFINITY; oi[lane] = 0x7fffffff; }
    __syncthreads();
    if (wave != 0) return -1;
    float v2[4];
    int i2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v2[e] = wv[e * 64 + lane]; i2[e] = wi[e * 64 + lane]; }
    wave_lds_fence();
    const int nc = wave_topk<4>(v2, i2, top_k, sv, si, wv, wi);                 // the candidate set, ranked, in wv / wi[0, nc)
    wave_lds_fence();
    return nc;
}

// Gumbel-max over the lanes of wave 0 that are `in` (lane l holds candidate word idx with score s): the winner's word and
// score in every lane; word 0x7fffffff if no lane's perturbed value compares (no candidate, or NaN scores only).
__device__ __forceinline__ Cand sample_wave_draw(bool in, float s, int idx, float inv_T, uint64_t key, float& bs) {
    bs = s;
    Cand c = {-INFINITY, 0x7fffffff};
    if (in) { c.idx = idx; c.v = sample_perturb(s, inv_T, sample_gumbel(key, c.idx)); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov2 = __shfl_xor(c.v, o, 64);
        const int oi2 = __shfl_xor(c.idx, o, 64);
        const float os = __shfl_xor(bs, o, 64);
        if (better(ov2, oi2, c.v, c.idx)) { c.v = ov2; c.idx = oi2; bs = os; }
    }
    return c;
}

// A row's one writer thread: the history, the next step's input word and the alive count; the last block to arrive publishes the
// count and advances the step (every block has read di_state[0] before it arrives here).
__device__ __forceinline__ void sample_commit(int64_t* __restrict__ toks, float* __restrict__ lps, int64_t* __restrict__ tok_out,
                                              int32_t* __restrict__ n_alive, int32_t* di_state, int di, int N, int64_t row,
                                              int64_t tok, float lp) {
    toks[(int64_t)di * N + row] = tok;
    lps[(int64_t)di * N + row] = lp;
    if (tok_out) tok_out[row] = tok;                                            // next step's input words
    if (tok != EOS) atomicAdd(&n_alive[1], 1);
    __threadfence();
    if (atomicAdd(&n_alive[2], 1) == N - 1) {
        n_alive[0] = atomicExch(&n_alive[1], 0);
        n_alive[2] = 0;
        if (di_state) __atomic_store_n(di_state, di + 1, __ATOMIC_RELAXED);
    }
}

// n_alive: int32[3] = {rows of the last step whose word is not EOS, the running count, the ticket of finished blocks}; the last
// two are zero between launches.
template <int M, bool TOPK>
__global__ __launch_bounds__(256) void sample_step_kernel(EnsLogp<M> L, EnsHid<M> hid, int64_t* __restrict__ toks,
                                                          float* __restrict__ lps, int32_t* di_state, int di_host, int max_len,
                                                          int B, int n, int V, float inv_T, int top_k,
                                                          const uint64_t* __restrict__ rng, int64_t* __restrict__ tok_out,
                                                          int32_t* __restrict__ n_alive) {
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    // stage 1 of the beam expansion's LDS: four arrays of 4 x 64 words
    __shared__ float wv[4 * 64], sv[4 * 64];
    __shared__ int wi[4 * 64], si[4 * 64];
    const int N = B * n;
    const int64_t row = blockIdx.x;
    const int64_t n_in = di == 0 ? row / n : row;
    const int lane = threadIdx.x & 63;
    if (di == 0) sample_replicate<M>(hid, row, n_in);
    const int64_t prev = di > 0 ? toks[(int64_t)(di - 1) * N + row] : (int64_t)-1;
    bool writer = false;
    int64_t tok = EOS;
    float lp = 0.f;
    if (prev == EOS) {                                                          // (uniform over the block)
        writer = threadIdx.x == 0;
    } else {
        const uint64_t key = sample_key(rng, di, row);
        if (!TOPK) {
            Cand c = {-INFINITY, 0x7fffffff};
            float cs = 0.f;
#pragma unroll 4
            for (int w = threadIdx.x; w < V; w += 256) {
                const float s = ens_score<M>(L, n_in, w);
                const float v = sample_perturb(s, inv_T, sample_gumbel(key, w));
                if (better(v, w, c.v, c.idx)) { c.v = v; c.idx = w; cs = s; }
            }
            const Cand r = block_best(c, reinterpret_cast<Cand*>(sv));
            if (r.idx == 0x7fffffff) {                                          // an all-NaN row: the padding word, never out of range
                writer = threadIdx.x == 0; tok = 0; lp = NAN;
            } else if (c.idx == r.idx) {                                        // (word indices are unique: one owner)
                writer = true; tok = r.idx; lp = cs;
            }
        } else {
            const int nc = sample_pool<M>(L, n_in, V, top_k, wv, sv, wi, si);
            if (nc < 0) return;
            float bs;
            const Cand c = sample_wave_draw(lane < nc, lane < nc ? wv[lane] : 0.f, lane < nc ? wi[lane] : 0x7fffffff, inv_T, key, bs);
            writer = lane == 0;
            if (c.idx == 0x7fffffff) { tok = 0; lp = NAN; }
            else { tok = c.idx; lp = bs; }
        }
    }
    if (writer) sample_commit(toks, lps, tok_out, n_alive, di_state, di, N, row, tok, lp);
}

// ---- nucleus (top-p) sampling ----
// The candidate pool P is the whole row (top_k = 0) or its ranked top_k.  With t[w] = fl(s[w] * inv_T), m = max_P t, e[w] =
// expf(t[w] - m) and Z = sum_P e, the nucleus is { w in P : s[w] >= s* }, s* the largest score in P whose words at or above it
// carry at least fl(top_p * Z): a value threshold, so words of equal score are in or out together.  The draw is the plain
// kernel's, restricted to the nucleus; top_p >= 1 takes the whole pool without looking at the masses (the plain kernel's draw bit
// for bit).  set_size (may be NULL): the nucleus' words, 0 for a finished or an all-NaN row.  NaN scores carry no mass and are
// never drawn.
//
// top_k = 0: the threshold is searched on the order-preserving key of s (select.h's fkey; -0 counts as +0), NUC_BITS bits per
// pass over the row, most significant first: a pass sums, per thread, e over the words at or above each of the 2^NUC_BITS
// candidate thresholds that extend the bits found so far, and keeps the largest candidate whose mass reaches top_p Z (the first
// pass's candidate 0 is the whole row: Z).  32 / NUC_BITS passes, whatever the data.  Every mass is summed in the same fixed
// tree -- a thread's words in index order, a xor butterfly over the wave, the four waves left to right -- in which a word always
// sits at the same leaf and a word below the threshold adds an exact 0: the mass is ONE monotone function of the threshold, the
// search finds its exact crossing, and a decode stays a pure function of (inputs, generator state).  No floating-point atomics.
constexpr int NUC_BITS = 4;
constexpr int NUC_CAND = 1 << NUC_BITS;

__device__ __forceinline__ unsigned nucleus_key(float s) { return fkey(s + 0.f); }
__device__ __forceinline__ float nucleus_weight(float s, float inv_T, float m) {
    return s == s ? expf(__fmul_rn(s, inv_T) - m) : 0.f;
}

template <int M, bool TOPK>
__global__ __launch_bounds__(256) void sample_step_p_kernel(EnsLogp<M> L, EnsHid<M> hid, int64_t* __restrict__ toks,
                                                            float* __restrict__ lps, int32_t* di_state, int di_host, int max_len,
                                                            int B, int n, int V, float inv_T, int top_k, float top_p,
                                                            const uint64_t* __restrict__ rng, int64_t* __restrict__ tok_out,
                                                            int32_t* __restrict__ n_alive, int32_t* __restrict__ set_size) {
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    __shared__ float wv[4 * 64], sv[4 * 64];
    __shared__ int wi[4 * 64], si[4 * 64];
    const int N = B * n;
    const int64_t row = blockIdx.x;
    const int64_t n_in = di == 0 ? row / n : row;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (di == 0) sample_replicate<M>(hid, row, n_in);
    const int64_t prev = di > 0 ? toks[(int64_t)(di - 1) * N + row] : (int64_t)-1;
    bool writer = false;
    int64_t tok = EOS;
    float lp = 0.f;
    int size = 0;
    if (prev == EOS) {                                                          // (uniform over the block)
        writer = threadIdx.x == 0;
    } else {
        const uint64_t key = sample_key(rng, di, row);
        if (!TOPK) {
            unsigned thr_key = 0;                                               // the nucleus: nucleus_key(s) >= thr_key
            if (top_p < 1.f) {
                float m = -INFINITY;
#pragma unroll 8
                for (int w = threadIdx.x; w < V; w += 256) m = fmaxf(m, __fmul_rn(ens_score<M>(L, n_in, w), inv_T));
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                if (lane == 0) sv[wave] = m;
                __syncthreads();
                m = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
                float need = 0.f;                                               // fl(top_p * Z), known after the first pass
                for (int b = 32 - NUC_BITS; b >= 0; b -= NUC_BITS) {
                    const unsigned p0 = thr_key >> b;                           // (its low NUC_BITS bits are still 0)
                    float acc[NUC_CAND];
#pragma unroll
                    for (int j = 0; j < NUC_CAND; ++j) acc[j] = 0.f;
#pragma unroll 4
                    for (int w = threadIdx.x; w < V; w += 256) {
                        const float s = ens_score<M>(L, n_in, w);
                        const float e = nucleus_weight(s, inv_T, m);
                        const unsigned kb = nucleus_key(s) >> b;
#pragma unroll
                        for (int j = 0; j < NUC_CAND; ++j) acc[j] += kb >= p0 + j ? e : 0.f;
                    }
                    float* red = wv + ((b / NUC_BITS) & 1) * (4 * NUC_CAND);    // two buffers: one barrier per pass
#pragma unroll
                    for (int j = 0; j < NUC_CAND; ++j) {
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
                        if (lane == 0) red[wave * NUC_CAND + j] = acc[j];
                    }
                    __syncthreads();
                    const int j = lane & (NUC_CAND - 1);                        // lane j of every wave: candidate j's mass
                    const float mass = ((red[j] + red[NUC_CAND + j]) + red[2 * NUC_CAND + j]) + red[3 * NUC_CAND + j];
                    if (b == 32 - NUC_BITS) need = __fmul_rn(top_p, __shfl(mass, 0, 64));
                    const unsigned ok = (unsigned)__ballot(mass >= need) & ((1u << NUC_CAND) - 2u);        // candidates 1 .. NUC_CAND - 1
                    if (ok) thr_key |= (unsigned)(31 - __clz(ok)) << b;
                }
            }
            Cand c = {-INFINITY, 0x7fffffff};
            float cs = 0.f;
#pragma unroll 4
            for (int w = threadIdx.x; w < V; w += 256) {
                const float s = ens_score<M>(L, n_in, w);
                if (nucleus_key(s) >= thr_key) {
                    size += s == s ? 1 : 0;
                    const float v = sample_perturb(s, inv_T, sample_gumbel(key, w));
                    if (better(v, w, c.v, c.idx)) { c.v = v; c.idx = w; cs = s; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) size += __shfl_xor(size, o, 64);
            if (lane == 0) si[wave] = size;
            const Cand r = block_best(c, reinterpret_cast<Cand*>(sv));          // (its barrier also publishes si)
            size = si[0] + si[1] + si[2] + si[3];
            if (r.idx == 0x7fffffff) {                                          // an all-NaN row: the padding word, never out of range
                writer = threadIdx.x == 0; tok = 0; lp = NAN; size = 0;
            } else if (c.idx == r.idx) {                                        // (word indices are unique: one owner)
                writer = true; tok = r.idx; lp = cs;
            }
        } else {
            const int nc = sample_pool<M>(L, n_in, V, top_k, wv, sv, wi, si);
            if (nc < 0) return;
            const float s = lane < nc ? wv[lane] : 0.f;
            bool in = lane < nc;
            if (top_p < 1.f) {                                                  // a prefix of the ranked pool, extended over equal scores
                const float t = __fmul_rn(s, inv_T);
                float m = in ? t : -INFINITY;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                float cum = in && s == s ? expf(t - m) : 0.f;                   // the inclusive scan of e in rank order
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float up = __shfl_up(cum, o, 64);
                    if (lane >= o) cum += up;
                }
                const float need = __fmul_rn(top_p, __shfl(cum, nc - 1, 64));   // Z: the scan's value at the pool's last word
                const unsigned long long hit = __ballot(in && cum >= need);
                const float s_star = __shfl(s, hit ? __ffsll(hit) - 1 : nc - 1, 64);
                in = in && s >= s_star;
            }
            size = __popcll(__ballot(in && s == s));
            float bs;
            const Cand c = sample_wave_draw(in, s, lane < nc ? wi[lane] : 0x7fffffff, inv_T, key, bs);
            writer = lane == 0;
            if (c.idx == 0x7fffffff) { tok = 0; lp = NAN; size = 0; }
            else { tok = c.idx; lp = bs; }
        }
    }
    if (!writer) return;
    if (set_size) set_size[(int64_t)di * N + row] = size;
    sample_commit(toks, lps, tok_out, n_alive, di_state, di, N, row, tok, lp);
}

// top_p < 0: the plain kernels (vag_sample_step*); else the nucleus kernels (vag_sample_step_p*)
static int sample_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                         int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                         int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                         int32_t* n_alive, float top_p, int32_t* set_size, hipStream_t s) {
    EnsHost a;
    VAG_TRY(ens_logp_args(logp, ldl, M, V, a));
    VAG_CHECK_ARG(toks && token_logp && rng && n_alive);
    VAG_CHECK_ARG(temperature > 0.f && temperature < INFINITY && top_k >= 0 && top_k <= 64);
    VAG_CHECK_ARG(B > 0 && n > 0 && B < (1ll << 31) && n < (1ll << 31) && B * n < (1ll << 31) && max_len > 0 && max_len < (1ll << 31));
    VAG_CHECK_ARG(V < (top_k > 0 ? (1ll << 24) : (1ll << 31)));              // (the radix keys hold 24 index bits)
    VAG_CHECK_ARG(di_state || (di >= 0 && di < max_len));
    if (!di_state && di == 0) {                                                // the one step that touches the hidden states
        VAG_CHECK_ARG(h_in && h_out && H);
        for (int m = 0; m < (int)M; ++m) {
            VAG_CHECK_ARG(h_in[m] && h_out[m] && H[m] > 0 && H[m] < (1ll << 31));
            a.in[m] = h_in[m]; a.out[m] = h_out[m]; a.H[m] = (int)H[m];
        }
    }
    const float inv_T = 1.0f / temperature;
    const dim3 grid((unsigned)(B * n));
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        if (top_p >= 0.f) {
            if (top_k > 0)
                hipLaunchKernelGGL((sample_step_p_kernel<MM, true>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks,
                                   token_logp, di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, (int)top_k, top_p, rng,
                                   tok_out, n_alive, set_size);
            else
                hipLaunchKernelGGL((sample_step_p_kernel<MM, false>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks,
                                   token_logp, di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, 0, top_p, rng, tok_out,
                                   n_alive, set_size);
        } else if (top_k > 0)
            hipLaunchKernelGGL((sample_step_kernel<MM, true>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks, token_logp,
                               di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, (int)top_k, rng, tok_out, n_alive);
        else
            hipLaunchKernelGGL((sample_step_kernel<MM, false>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks, token_logp,
                               di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, 0, rng, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

int vag_sample_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                           int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                           int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                           int32_t* n_alive, hipStream_t s) {
    return sample_launch(logp, ldl, M, toks, token_logp, di, di_state, max_len, h_in, h_out, H, tok_out, B, n, V, temperature, top_k,
                         rng, n_alive, -1.f, nullptr, s);
}

int vag_sample_step_p_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                             int32_t* n_alive, float top_p, int32_t* set_size, hipStream_t s) {
    VAG_CHECK_ARG(top_p > 0.f && top_p <= 1.f);                                // (NaN fails both)
    return sample_launch(logp, ldl, M, toks, token_logp, di, di_state, max_len, h_in, h_out, H, tok_out, B, n, V, temperature, top_k,
                         rng, n_alive, top_p, set_size, s);
}

// out (N, V): the noise g(n, w) step di's launch adds under this generator state.  Not on the hot path: for tests and audits.
__global__ __launch_bounds__(256) void sample_noise_kernel(const uint64_t* __restrict__ rng, int di, int V, float* __restrict__ out) {
    const int64_t row = blockIdx.x;
    const uint64_t key = sample_key(rng, di, row);
    for (int w = threadIdx.x; w < V; w += 256) out[row * V + w] = sample_gumbel(key, w);
}

int vag_sample_noise_launch(const uint64_t* rng, int64_t di, int64_t N, int64_t V, float* out, hipStream_t s) {
    VAG_CHECK_ARG(rng && out && di >= 0 && di < (1ll << 31) && N > 0 && N < (1ll << 31) && V > 0 && V < (1ll << 31));
    hipLaunchKernelGGL(sample_noise_kernel, dim3((unsigned)N), dim3(256), 0, s, rng, (int)di, (int)V, out);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
