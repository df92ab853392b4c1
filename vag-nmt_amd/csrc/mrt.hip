// Minimum-risk training (Shen et al. 2016, "Minimum Risk Training for Neural Machine Translation"; Edunov et al. 2018, "Classical
// Structured Prediction Losses for Sequence to Sequence Learning"): the expected sentence-level cost of a set of candidate
// translations under the model's own renormalised distribution, in place of the token-level loss of models/...V11.py:162-166.
// Two kernels (include/vag_nmt.h: vag_mrt_weights, vag_mrt_pack):
//   mrt_weights_kernel   between the head's forward and backward: turns the step's per-row nll into the per-sentence factors
//                        inv_cnt[b] the cross-entropy backward multiplies every row of sentence b with, and the risk itself
//   mrt_pack_kernel      candidates in the samplers' format (+ the gold sentence) -> forced targets in the training format, with the
//                        rows that must not take part (repeats, spans holding the padding word) marked invalid
//
// Why the existing backward serves.  It forms (head.hip: ce_bwd_kernel)   d logits[t, b] = d_loss * inv_cnt[b] / B * w * (softmax - onehot),
// i.e. the gradient of   sum_b inv_cnt[b] / B * sum_t nll[t, b]  =  - sum_b inv_cnt[b] / B * s_b,   s_b = log p(y_b | x) = - sum_t nll[t, b].
// The risk of a call with G groups of N candidates, R = scale / G * sum_g sum_i Q_i c_i with Q = softmax_i(alpha s_i), has
//   dR / d s_i = scale / G * alpha Q_i (c_i - R_g),
// so the two agree for   - inv_cnt[b_i] / B = scale / G * alpha Q_i (c_i - R_g),   and with B = G N:
//   inv_cnt[b_i] = - scale * N * alpha * Q_i * (c_i - R_g).
// The sign: the backward differentiates +nll = -s.  The factor N: it divides by the B = G N rows of the call, the risk by its G groups.
#include "kernels.h"

constexpr int MRT_MAX_N = 256;           // candidates per source sentence (a lane owns at most MRT_MAX_N / 64 of them)
constexpr int MRT_PER_LANE = MRT_MAX_N / 64;
constexpr int MRT_WAVES = 4;
constexpr int MRT_MAX_L = 512;           // tokens per candidate row (vag_mbr_select's limit: the cost comes from there)
constexpr int64_t MRT_EOS = 3;

__device__ __forceinline__ double mrt_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double mrt_wave_sum(double v) {                 // a butterfly: the same order, so the same bits, in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ONE workgroup; wave w takes the groups w, w + 4, ..., lane l of it the candidates l, l + 64, ... of the group.  Every sum has a fixed
// order (a lane's candidates ascending, the wave's butterfly, a wave's groups ascending, the four waves ascending): the same bits from
// run to run.  Only the exponential is fp32; everything around it is double, for two cancellations that fp32 loses at the 1e-4 level:
// alpha * s - max at alpha * s of a few hundred (the rounding of s alone is 1e-7 relative), and c - R of the best row when Q is nearly
// one-hot (R is then that row's own cost up to a few 1e-4, so fp32's 6e-8 c is 2e-4 of the difference).  A handful of candidates per
// lane: the double arithmetic costs nothing that can be measured.
__global__ __launch_bounds__(64 * MRT_WAVES) void mrt_weights_kernel(const float* __restrict__ nll, const float* __restrict__ cost,
                                                                    const float* __restrict__ valid, int B, int Tt, int N,
                                                                    float alpha, float scale, float* __restrict__ inv_cnt,
                                                                    float* __restrict__ q, float* __restrict__ risk,
                                                                    float* __restrict__ losses, float w_mt, int ring) {
    __shared__ double rsum[MRT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = B / N;
    double racc = 0.0;
    for (int g = wave; g < G; g += MRT_WAVES) {
        double x[MRT_PER_LANE], c[MRT_PER_LANE];
        bool ok[MRT_PER_LANE];
        double mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < MRT_PER_LANE; ++u) {
            const int i = lane + 64 * u;
            const int b = g * N + i;
            ok[u] = i < N && (!valid || valid[b] != 0.f);
            x[u] = 0.0;
            c[u] = 0.0;
            if (ok[u]) {
                double s = 0.0;
                for (int t = 0; t < Tt; ++t) s -= (double)nll[(int64_t)t * B + b];
                x[u] = (double)alpha * s;
                c[u] = (double)cost[b];
                mx = fmax(mx, x[u]);
            }
        }
        mx = mrt_wave_max(mx);
        double e[MRT_PER_LANE];
        double z = 0.0;
#pragma unroll
        for (int u = 0; u < MRT_PER_LANE; ++u) {
            e[u] = ok[u] ? (double)expf((float)(x[u] - mx)) : 0.0;     // <= 1; the best row gives exactly 1, so Z >= 1
            z += e[u];
        }
        z = mrt_wave_sum(z);
        const double rz = z > 0.0 ? 1.0 / z : 0.0;                     // (a group without a valid row: every Q = 0, R_g = 0)
        double r = 0.0;
#pragma unroll
        for (int u = 0; u < MRT_PER_LANE; ++u) {
            e[u] *= rz;
            r += e[u] * c[u];
        }
        r = mrt_wave_sum(r);
#pragma unroll
        for (int u = 0; u < MRT_PER_LANE; ++u) {
            const int i = lane + 64 * u;
            if (i < N) {
                const int b = g * N + i;
                inv_cnt[b] = ok[u] ? (float)(-(double)scale * (double)N * (double)alpha * e[u] * (c[u] - r)) : 0.f;
                if (q) q[b] = (float)e[u];
            }
        }
        racc += r;
    }
    if (lane == 0) rsum[wave] = racc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < MRT_WAVES; ++w) tot += rsum[w];
        const float R = (float)((double)scale / (double)G * tot);
        if (risk) risk[0] = R;
        if (losses) {                           // the fused step's results, as loss_mt_body (head.hip) leaves them: no ranking loss here
            const float total = w_mt * R;
            losses[0] = total; losses[1] = R; losses[2] = 0.f;
            if (ring > 0) {
                const unsigned n = __float_as_uint(losses[3]);
                float* o = losses + 4 + 4 * (n % (unsigned)ring);
                o[0] = total; o[1] = R; o[2] = 0.f;
                losses[3] = __uint_as_float(n + 1u);
            }
        }
    }
}

int vag_mrt_cfg_ok(int64_t B, int64_t N, float alpha, float scale) {
    return N >= 2 && N <= MRT_MAX_N && B >= N && B % N == 0 && B < (1ll << 31) && alpha > 0.f && alpha < INFINITY && scale > 0.f &&
           scale < INFINITY;
}

int vag_mrt_weights_launch(const float* nll, const float* cost, const float* valid, int64_t B, int64_t Tt, int64_t N, float alpha,
                           float scale, float* inv_cnt, float* q, float* risk, float* losses, float w_mt, int ring, hipStream_t s) {
    VAG_CHECK_ARG(nll && cost && inv_cnt && (risk || losses));
    VAG_CHECK_ARG(Tt >= 1 && Tt < (1ll << 31) / (B > 0 ? B : 1) && vag_mrt_cfg_ok(B, N, alpha, scale));
    hipLaunchKernelGGL(mrt_weights_kernel, dim3(1), dim3(64 * MRT_WAVES), 0, s, nll, cost, valid, (int)B, (int)Tt, (int)N, alpha, scale,
                       inv_cnt, q, risk, losses, w_mt, ring);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// One workgroup per source sentence g; wave w writes the rows w, w + 4, ... of the group, then decides the validity of the same rows.
// Spans are compared on the input rows (nothing this launch wrote is read back).  "An earlier VALID row" needs no sequential pass:
// equal spans hold the padding word together, and a repeat of a repeat repeats the first, so row i is valid iff its span holds no 0
// and NO earlier row of the group has the same span.
__device__ __forceinline__ const int64_t* mrt_src_row(const int64_t* cand, int Nc, int L, const int64_t* gold, int Tg, int include_gold,
                                                      int64_t g, int i) {
    return include_gold && i == 0 ? gold + g * Tg : cand + (g * Nc + (i - include_gold)) * L;
}
__global__ __launch_bounds__(64 * MRT_WAVES) void mrt_pack_kernel(const int64_t* __restrict__ cand, int Nc, int L,
                                                                 const int64_t* __restrict__ gold, int Tg, int include_gold,
                                                                 int64_t* __restrict__ tgt, int Tt, float* __restrict__ valid) {
    __shared__ int lens[MRT_MAX_N];
    __shared__ int zero[MRT_MAX_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = Nc + include_gold;
    const int64_t g = blockIdx.x;
    for (int i = wave; i < N; i += MRT_WAVES) {
        const bool is_gold = include_gold && i == 0;
        const int64_t* row = mrt_src_row(cand, Nc, L, gold, Tg, include_gold, g, i);
        const int n = is_gold ? Tg : L;
        int len = n;
        for (int base = 0; base < n; base += 64) {                   // the span: what precedes the first EOS, or the whole row
            const int p = base + lane;
            const unsigned long long stop = __ballot(p < n && row[p] == MRT_EOS);
            if (stop) { len = base + (__ffsll(stop) - 1); break; }   // (uniform over the wave)
        }
        len = min(len, Tt - 1);                                       // (only a gold row without EOS at Tg = Tt: cut, never past the row)
        int64_t* out = tgt + (g * N + i) * Tt;
        bool z = false;
        for (int base = 0; base < Tt; base += 64) {
            const int p = base + lane;
            const int64_t t = p < len ? row[p] : (p == len ? MRT_EOS : 0);
            if (p < Tt) out[p] = t;
            z = z || __ballot(p < len && t == 0) != 0ull;
        }
        if (lane == 0) { lens[i] = len; zero[i] = z ? 1 : 0; }
    }
    __syncthreads();
    for (int i = wave; i < N; i += MRT_WAVES) {                      // a wave per row: 64 positions per comparison step
        bool ok = zero[i] == 0;
        const int len = lens[i];
        const int64_t* a = mrt_src_row(cand, Nc, L, gold, Tg, include_gold, g, i);
        for (int j = 0; ok && j < i; ++j) {                           // (everything here is uniform over the wave)
            if (lens[j] != len) continue;
            const int64_t* b = mrt_src_row(cand, Nc, L, gold, Tg, include_gold, g, j);
            bool same = true;                                         // (two empty spans are the same span)
            for (int base = 0; same && base < len; base += 64) {
                const int p = base + lane;
                same = __ballot(p < len && a[p] != b[p]) == 0ull;
            }
            ok = !same;
        }
        if (lane == 0) valid[g * N + i] = ok ? 1.f : 0.f;
    }
}

int vag_mrt_pack_launch(const int64_t* cand, int64_t G, int64_t Nc, int64_t L, const int64_t* gold, int64_t Tg, int include_gold,
                        int64_t* tgt, int64_t Tt, float* valid, hipStream_t s) {
    VAG_CHECK_ARG(cand && tgt && valid && (include_gold == 0 || include_gold == 1) && (!include_gold || gold));
    VAG_CHECK_ARG(G >= 1 && Nc >= 1 && Nc + include_gold <= MRT_MAX_N && L >= 1 && L <= MRT_MAX_L && Tg >= 0 && Tg <= MRT_MAX_L + 1);
    VAG_CHECK_ARG(!include_gold || Tg >= 1);
    VAG_CHECK_ARG(Tt >= L + 1 && (!include_gold || Tt >= Tg) && G < (1ll << 31) / (MRT_MAX_N * (MRT_MAX_L + 1)));
    hipLaunchKernelGGL(mrt_pack_kernel, dim3((unsigned)G), dim3(64 * MRT_WAVES), 0, s, cand, (int)Nc, (int)L, gold, (int)Tg,
                       include_gold, tgt, (int)Tt, valid);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
