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
#include "kernels.h"
#include "select.h"

constexpr int64_t EOS = 3;
constexpr int SEPT = 8;                  // words per lane and round of the top-k path (a wave walks slices of 64 * SEPT words)
constexpr int SLICE = 64 * SEPT;

// the Gumbel noise of word w under a row's key: vag_sample_noise writes exactly this
__device__ __forceinline__ uint64_t sample_key(const uint64_t* rng, int di, int64_t row) {
    const uint64_t base = vag_mix64(rng[0] ^ (rng[1] * 0xD1342543DE82EF95ull) ^ (0x53ull << 56));
    return vag_mix64(base ^ (((uint64_t)(uint32_t)di << 32) | (uint64_t)(uint32_t)row));
}
__device__ __forceinline__ float sample_gumbel(uint64_t key, int w) {
    const uint64_t r = vag_mix64(key + (uint64_t)w) >> 41;                              // 23 bits
    const float u = __fmul_rn(__fadd_rn((float)r, 0.5f), 1.0f / 8388608.0f);           // exact: in [2^-24, 1 - 2^-24]
    return -logf(-logf(u));
}
__device__ __forceinline__ float sample_perturb(float s, float inv_T, float g) { return __fadd_rn(__fmul_rn(s, inv_T), g); }

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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (di == 0) {                                                              // the members' states, replicated by source row
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int H = hid.H[m];
            for (int c = threadIdx.x; c < H; c += 256) hid.out[m][row * H + c] = hid.in[m][n_in * H + c];
        }
    }
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
            float* ov = wv + wave * 64;
            int* oi = wi + wave * 64;
            int cnt = 0;                                                        // ranked entries in (ov, oi), uniform over the wave
            for (int base = wave * SLICE; base < V; base += 4 * SLICE) {
                float val[SEPT + 1];
                int idx[SEPT + 1];
#pragma unroll
                for (int e = 0; e < SEPT; ++e) {                                // all M * SEPT loads in flight together (index clamped)
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
            if (wave != 0) return;
            float v2[4];
            int i2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v2[e] = wv[e * 64 + lane]; i2[e] = wi[e * 64 + lane]; }
            wave_lds_fence();
            const int nc = wave_topk<4>(v2, i2, top_k, sv, si, wv, wi);         // the candidate set, ranked, in wv / wi[0, nc)
            wave_lds_fence();
            const float s = lane < nc ? wv[lane] : 0.f;
            float bs = s;
            Cand c = {-INFINITY, 0x7fffffff};
            if (lane < nc) { c.idx = wi[lane]; c.v = sample_perturb(s, inv_T, sample_gumbel(key, c.idx)); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov2 = __shfl_xor(c.v, o, 64);
                const int oi2 = __shfl_xor(c.idx, o, 64);
                const float os = __shfl_xor(bs, o, 64);
                if (better(ov2, oi2, c.v, c.idx)) { c.v = ov2; c.idx = oi2; bs = os; }
            }
            writer = lane == 0;
            if (c.idx == 0x7fffffff) { tok = 0; lp = NAN; }
            else { tok = c.idx; lp = bs; }
        }
    }
    if (!writer) return;
    toks[(int64_t)di * N + row] = tok;
    lps[(int64_t)di * N + row] = lp;
    if (tok_out) tok_out[row] = tok;                                            // next step's input words
    if (tok != EOS) atomicAdd(&n_alive[1], 1);
    // every block has read di_state[0] before it arrives here; the last one to arrive publishes the count and advances the step
    __threadfence();
    if (atomicAdd(&n_alive[2], 1) == N - 1) {
        n_alive[0] = atomicExch(&n_alive[1], 0);
        n_alive[2] = 0;
        if (di_state) __atomic_store_n(di_state, di + 1, __ATOMIC_RELAXED);
    }
}

int vag_sample_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                           int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                           int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                           int32_t* n_alive, hipStream_t s) {
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
        if (top_k > 0)
            hipLaunchKernelGGL((sample_step_kernel<MM, true>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks, token_logp,
                               di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, (int)top_k, rng, tok_out, n_alive);
        else
            hipLaunchKernelGGL((sample_step_kernel<MM, false>), grid, dim3(256), 0, s, ens_logp<MM>(a), ens_hid<MM>(a), toks, token_logp,
                               di_state, (int)di, (int)max_len, (int)B, (int)n, (int)V, inv_T, 0, rng, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
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
