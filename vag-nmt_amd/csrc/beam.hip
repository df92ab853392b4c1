// Batched beam-search expansion (models/NMT_AttentionImagine_Seq2Seq_Beam_V11.py:259-324) without host syncs.
//   stage 1: grid (chunks, B): each block selects the k best of a 2048-candidate slice of the k_in*V
//            continuations, applying the reference's penalties on the fly (repeat-token suppression,
//            finished hypotheses may only emit EOS at cost 0).
//   stage 2: one block per sentence merges the chunk winners, updates running scores, appends (token, parent) to the
//            history and re-orders the decoder hidden state for the next step.  The history is kept as back-pointers
//            (rows [max_len, 2 max_len) of the beam buffer) and resolved once by the finish kernel, instead of
//            permuting all earlier rows at every step as the reference does (V11.py:309) -- same hypotheses.
//   finish:  one kernel ranks the k final hypotheses of a sentence and resolves the n best (n = 1: the search's result);
//            its aligning form also resolves their attention rows from the per-step record.
// Selection uses the total order (score desc, flat index asc), so results are deterministic; the reference's
// topk(sorted=False) leaves the order of equal-score candidates unspecified.
// Ensembles (vag_beam_ens_step*, vag_ens_argmax): stage 1 and the greedy arg-max read M <= VAG_ENS_MAX log-probability matrices
// and score every candidate by select.h's ens_score; stage 2 re-orders M hidden states by the same back-pointers.  M is a
// template parameter (select.h: ens_dispatch): M = 1 is the single-model code.
// Search options (the reference's avoid_double / avoid_unk, V11.py:233,279-284): `flags`, a by-value argument of stage 1;
// 0 is the reference's defaults.  Forced decoding (scores and attention of given translations): the end of this file.
// Expansions with a selection rule of their own: the diverse search's groups (vag_beam_div_step), required phrases
// (vag_beam_req_step), stochastic beams (vag_beam_sbs_step), length and coverage penalties (vag_beam_pen_step, with
// vag_beam_cover before it and vag_beam_finish_pen after the search).  They share ONE row-aligned stage 1, a kernel template
// over the search's rule (beam_row_stage1_kernel), and each has a stage 2 of its own, one workgroup per sentence, built from
// the shared selections (block_scan_select, wave_rank_select) where its rule allows.  Every stage 2, the plain one included,
// ends in beam_step_tail.
#include "kernels.h"
#include "select.h"

constexpr int EPT = 8;                   // candidates per thread in stage 1 (a rescan after each pick walks these)
constexpr int CHUNK = 256 * EPT;
constexpr float NEG_PEN = -1e5f;         // the reference's "inf" (V11.py:257)
constexpr int64_t EOS = 3;
constexpr int64_t UNK = 1;               // NMT_Seq2Seq_Beam_V2.py:15, preprocessing.py:18 (V11.py uses it without defining it)


// Selection in both stages (fallback path): every thread caches the best of the candidates it owns; a round is one block-wide argmax
// of the cached bests, and only the winner's owner rescans its (register- or LDS-resident) candidates.
// The step index: select.h's step_index (stage 2 advances di_state[0]; launches that read it have k_in == k).
// M > 1: an ensemble (the raw-logits form, parts != NULL, is single-model only).
// flags (steps >= 1 only; step 0 applies no penalty, V11.py:261-264): VAG_BEAM_ALLOW_REPEAT lifts the repeat-token penalty
// (avoid_double=False), VAG_BEAM_AVOID_UNK gives UNK the penalty (avoid_unk=True, :283-284).  Values are replaced, not added,
// and a finished hypothesis's rule (:291-294) overrides both.  OPT = false (flags == 0) compiles the option tests away: the
// default search runs the kernel it ran before the options existed.
template <int M, bool OPT>
__global__ __launch_bounds__(256) void beam_stage1_kernel(EnsLogp<M> L,
                                                          const float* __restrict__ nll_in, const int64_t* __restrict__ beam,
                                                          const int32_t* di_state, int di_host, int max_len, int B,
                                                          int k_in, int k, int V, float* __restrict__ cval,
                                                          int* __restrict__ cidx, int32_t* __restrict__ n_alive,
                                                          const float* __restrict__ parts, int nparts, int flags) {
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    // parts != NULL (M = 1): the matrix holds raw logits and parts (nparts, rows, 2) the (max, sum exp) pieces of every row's log-sum-exp
    // (the vocabulary product's epilogue wrote them: skinny.hip, TallArgs::parts).  A chunk of 2048 candidates touches at most
    // ceil(2048 / V) + 1 rows; waves 0..3 combine the pieces of the first four of them (V >= 683 whenever pieces exist).
    __shared__ float lse_s[4];
    const int jfirst = (int)(((int64_t)blockIdx.x * CHUNK) / V);
    if (M == 1 && parts) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int j = min(jfirst + wave, k_in - 1);
        const int64_t rows = (int64_t)B * k_in;                    // pieces are laid out [piece][row]
        const float* pr = parts + ((int64_t)blockIdx.y * k_in + j) * 2;
        float m = -INFINITY;
        for (int x = lane; x < nparts; x += 64) m = fmaxf(m, pr[2 * x * rows]);
        m = wave_max(m);
        float sm = 0.f;
        for (int x = lane; x < nparts; x += 64) sm += pr[2 * x * rows + 1] * __expf(pr[2 * x * rows] - m);
        sm = wave_sum(sm);
        if (lane == 0) lse_s[wave] = m + __logf(sm);
        __syncthreads();
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *n_alive = 0;   // stage 2 (next launch) counts into it
    const int penal = di > 0;
    const float* nll = di > 0 ? nll_in : nullptr;
    const int64_t* prev_tok = di > 0 ? beam + (int64_t)(di - 1) * B * k : beam;
    const int b = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
    const int total = k_in * V;
    const int f0 = chunk * CHUNK + threadIdx.x;
    const float rV = 1.f / (float)V;
    // branch-free so that all (M+2)*EPT loads of a thread are in flight together (indices clamped, result selected)
    float val[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int f = f0 + e * 256;                               // flat index j*V + w
        const int fc = min(f, total - 1);
        int j = (int)((float)fc * rV);                            // fc < 2^24: exact up to one unit
        if (j * V > fc) --j;
        else if ((j + 1) * V <= fc) ++j;
        const int w = fc - j * V;
        const int64_t n = (int64_t)b * k_in + j;
        float lp = ens_score<M>(L, n, w);
        if (M == 1 && parts) lp -= lse_s[min(j - jfirst, 3)];
        const int64_t pt = penal ? prev_tok[n] : (int64_t)-1;
        const float base = nll ? nll[n] : 0.f;
        if (pt == EOS) lp = (w == EOS) ? 0.f : NEG_PEN;           // V11.py:291-294
        else if (!OPT && w == pt) lp = NEG_PEN;                 // V11.py:279-280
        else if (OPT && ((w == pt && !(flags & VAG_BEAM_ALLOW_REPEAT)) ||                  // V11.py:279-280
                         (penal && w == UNK && (flags & VAG_BEAM_AVOID_UNK)))) lp = NEG_PEN;   // V11.py:283-284
        val[e] = f < total ? base + lp : -INFINITY;               // V11.py:297
    }
    // each wave ranks the k best of its 512 candidates; wave 0 then ranks the k best of those 4k
    __shared__ float wv[4 * 64], sv[4 * 64];
    __shared__ int wi[4 * 64], si[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int idx[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) idx[e] = (f0 + e * 256 < total) ? f0 + e * 256 : 0x7fffffff;
    wv[wave * 64 + lane] = -INFINITY; wi[wave * 64 + lane] = 0x7fffffff;
    wave_lds_fence();
    wave_topk<EPT>(val, idx, k, sv + wave * 64, si + wave * 64, wv + wave * 64, wi + wave * 64);
    __syncthreads();
    if (wave != 0) return;
    float v2[4];
    int i2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v2[e] = wv[e * 64 + lane]; i2[e] = wi[e * 64 + lane]; }
    const int64_t o = ((int64_t)b * chunks + chunk) * k;
    const int n = wave_topk<4>(v2, i2, k, sv, si, cval + o, cidx + o);
    for (int r = n + lane; r < k; r += 64) { cval[o + r] = -INFINITY; cidx[o + r] = 0x7fffffff; }
}

// The end of every stage 2: once a sentence's k selections (flat index j V + w, score; slot r = r-th entry) are in LDS, the
// history row, the running scores, the next step's input words, the alive count, the hidden-state re-tiling of every member
// and, for a device-side step index, its advance.  Called by the whole workgroup after a barrier.
template <int M>
__device__ __forceinline__ void beam_step_tail(const int* sel_idx, const float* sel_val, int b, int k_in, int k, int V,
                                               const EnsHid<M>& hid, float* __restrict__ nll, int64_t* __restrict__ beam,
                                               int32_t* di_state, int di, int max_len, int B, int64_t* __restrict__ tok_out,
                                               int32_t* __restrict__ n_alive) {
    if (threadIdx.x < k) {
        const int j = threadIdx.x;
        const int f = sel_idx[j];
        const int64_t w = f % V;
        beam[((int64_t)di * B + b) * k + j] = w;                                // V11.py:306
        beam[((int64_t)(max_len + di) * B + b) * k + j] = f / V;                // parent hypothesis (V11.py:303,309)
        if (tok_out) tok_out[(int64_t)b * k + j] = w;                           // next step's input words
        nll[(int64_t)b * k + j] = sel_val[j];
        if (w != EOS) atomicAdd(n_alive, 1);
    }
    // hidden-state re-tiling for the next step (V11.py:273,:313): every model's state by the same back-pointers
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int H = hid.H[m];
        const float* __restrict__ h_in = hid.in[m];
        float* __restrict__ h_out = hid.out[m];
        if ((H & 3) == 0) {
            const int H4 = H >> 2;
            for (int e = threadIdx.x; e < k * H4; e += 256) {
                const int j = e / H4, c = e - j * H4;
                const int src = sel_idx[j] / V;
                reinterpret_cast<float4*>(h_out + ((int64_t)b * k + j) * H)[c] =
                    reinterpret_cast<const float4*>(h_in + ((int64_t)b * k_in + src) * H)[c];
            }
        } else {
            for (int e = threadIdx.x; e < k * H; e += 256) {
                const int j = e / H, c = e - j * H;
                const int src = sel_idx[j] / V;
                h_out[((int64_t)b * k + j) * H + c] = h_in[((int64_t)b * k_in + src) * H + c];
            }
        }
    }
    if (di_state && threadIdx.x == 0) {
        // every block has read di_state[0] before it arrives here; the last one to arrive advances the step
        __threadfence();
        if (atomicAdd(&di_state[1], 1) == B - 1) {
            di_state[1] = 0;
            __atomic_store_n(di_state, di + 1, __ATOMIC_RELAXED);
        }
    }
}

constexpr int S2_LDS = 4096;             // candidates kept in LDS by stage 2 (more: selection works on the scratch copy)

template <int M>
__global__ __launch_bounds__(256) void beam_stage2_kernel(float* __restrict__ cval, int* __restrict__ cidx,
                                                          int chunks, int k_in, int k, int V, EnsHid<M> hid,
                                                          float* __restrict__ nll, int64_t* __restrict__ beam,
                                                          int32_t* di_state, int di_host, int max_len, int B,
                                                          int64_t* __restrict__ tok_out, int32_t* __restrict__ n_alive) {
    __shared__ Cand sh[4];
    __shared__ int sel_idx[64];
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    __shared__ float sel_val[64];
    __shared__ float lv[S2_LDS];
    __shared__ int li[S2_LDS];
    const int b = blockIdx.x;
    const int ncand = chunks * k;
    float* pv = cval + (int64_t)b * ncand;
    int* pi = cidx + (int64_t)b * ncand;
    if (ncand <= S2_LDS) {
        for (int e = threadIdx.x; e < ncand; e += 256) { lv[e] = pv[e]; li[e] = pi[e]; }
        pv = lv; pi = li;
        __syncthreads();
    }
    constexpr int E2 = 16;                     // fast path: up to 1024 chunk winners, held by ONE wave (16 per lane)
    if (ncand <= 64 * E2) {
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            float v2[E2];
            int i2[E2];
#pragma unroll
            for (int e = 0; e < E2; ++e) {
                const int c = e * 64 + lane;
                v2[e] = c < ncand ? pv[c] : -INFINITY;
                i2[e] = c < ncand ? pi[c] : 0x7fffffff;
            }
            __shared__ float tv[64];
            __shared__ int ti[64];
            const int n = wave_topk<E2>(v2, i2, k, tv, ti, sel_val, sel_idx);       // ranked: slot j = j-th best
            for (int r = n + lane; r < k; r += 64) { sel_idx[r] = 0x7fffffff; sel_val[r] = -INFINITY; }
        }
    } else {
    int mine_e = -1;
    auto scan = [&]() {
        Cand c = {-INFINITY, 0x7fffffff};
        mine_e = -1;
        for (int e = threadIdx.x; e < ncand; e += 256) {
            const int f = pi[e];
            if (f != 0x7fffffff && better(pv[e], f, c.v, c.idx)) { c.v = pv[e]; c.idx = f; mine_e = e; }
        }
        return c;
    };
    Cand mine = scan();
    for (int r = 0; r < k; ++r) {
        const Cand c = block_best(mine, sh);
        if (threadIdx.x == 0) { sel_idx[r] = c.idx; sel_val[r] = c.v; }
        if (c.idx != 0x7fffffff && mine.idx == c.idx) {
            pi[mine_e] = 0x7fffffff;                               // taken (only its owner reads this slot again)
            mine = scan();
        }
    }
    }
    __syncthreads();
    beam_step_tail<M>(sel_idx, sel_val, b, k_in, k, V, hid, nll, beam, di_state, di, max_len, B, tok_out, n_alive);
}

int64_t vag_beam_scratch_bytes_impl(int64_t B, int64_t k, int64_t V) {
    const int64_t chunks = cdiv64(k * V, CHUNK);
    return B * chunks * k * 8 + 64;
}

// One expansion of M models' scores (M = 1: the single model); `a` holds entries [0, M).
static int beam_step_common(const EnsHost& a, int M, float* nll, int64_t* beam, int64_t di,
                            int32_t* di_state, int64_t max_len, int64_t* tok_out, int64_t B, int64_t k, int64_t V,
                            int32_t* n_alive, void* scratch, hipStream_t s, const float* parts, int64_t nparts, int flags) {
    VAG_CHECK_ARG(nll && beam && n_alive && scratch);
    VAG_CHECK_ARG((flags & ~(VAG_BEAM_ALLOW_REPEAT | VAG_BEAM_AVOID_UNK)) == 0);
    VAG_CHECK_ARG(!parts || (M == 1 && nparts > 0 && V >= CHUNK));    // (a chunk then spans at most two rows)
    VAG_CHECK_ARG(B > 0 && k > 0 && k <= 64 && V > 0 && max_len > 0);
    VAG_CHECK_ARG(di_state || (di >= 0 && di < max_len));
    const int k_in = (!di_state && di == 0) ? 1 : (int)k;
    const int64_t total = (int64_t)k_in * V;
    VAG_CHECK_ARG(total < (1ll << 24) && total >= k);          // stage 1 splits flat indices with a float reciprocal
    const int chunks = (int)cdiv64(total, CHUNK);
    float* cval = reinterpret_cast<float*>(scratch);
    int* cidx = reinterpret_cast<int*>(cval + B * cdiv64(k * V, CHUNK) * k);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    return ens_dispatch(M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        if (flags)
            hipLaunchKernelGGL((beam_stage1_kernel<MM, true>), grid, dim3(256), 0, s, ens_logp<MM>(a), nll, beam, di_state, (int)di,
                               (int)max_len, (int)B, k_in, (int)k, (int)V, cval, cidx, n_alive, parts, (int)nparts, flags);
        else
            hipLaunchKernelGGL((beam_stage1_kernel<MM, false>), grid, dim3(256), 0, s, ens_logp<MM>(a), nll, beam, di_state, (int)di,
                               (int)max_len, (int)B, k_in, (int)k, (int)V, cval, cidx, n_alive, parts, (int)nparts, 0);
        VAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(beam_stage2_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, cval, cidx, chunks, k_in, (int)k, (int)V,
                           ens_hid<MM>(a), nll, beam, di_state, (int)di, (int)max_len, (int)B, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

int vag_beam_step_launch(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int32_t* di_state,
                         int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k,
                         int64_t V, int64_t H, int32_t* n_alive, void* scratch, hipStream_t s, const float* parts, int64_t nparts,
                         int flags) {
    VAG_CHECK_ARG(logp && h_in && h_out && H > 0 && H < (1ll << 31) && ldl >= V);
    EnsHost a = {};
    a.p[0] = logp; a.ld[0] = ldl;
    a.in[0] = h_in; a.out[0] = h_out; a.H[0] = (int)H;
    return beam_step_common(a, 1, nll, beam, di, di_state, max_len, tok_out, B, k, V, n_alive, scratch, s, parts, nparts, flags);
}


// host arrays of M hidden states -> `a` (after ens_logp_args, which checks M); every entry is checked before anything is enqueued
static int ens_hid_args(const float* const* h_in, float* const* h_out, const int64_t* H, int64_t M, EnsHost& a) {
    VAG_CHECK_ARG(h_in && h_out && H);
    for (int m = 0; m < (int)M; ++m) {
        VAG_CHECK_ARG(h_in[m] && h_out[m] && H[m] > 0 && H[m] < (1ll << 31));
        a.in[m] = h_in[m]; a.out[m] = h_out[m]; a.H[m] = (int)H[m];
    }
    return VAG_OK;
}

int vag_beam_ens_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, hipStream_t s,
                             int flags) {
    EnsHost a;
    VAG_TRY(ens_logp_args(logp, ldl, M, V, a));
    VAG_TRY(ens_hid_args(h_in, h_out, H, M, a));
    return beam_step_common(a, (int)M, nll, beam, di, di_state, max_len, tok_out, B, k, V, n_alive, scratch, s, nullptr, 0, flags);
}

// ---- row-aligned expansions: what the searches with a selection rule of their own share ---------------------------------
// Diverse groups, required phrases, stochastic beams and the penalised search each need more than the sentence's k best by c,
// so their stage 1 is row-aligned -- grid (ceil(V / 2048), B k_in), each block ranks the k best of one 2048-word slice of ONE
// row, winners in scratch (B, k_in, slices, k) -- and one workgroup per sentence selects among the winners by the search's own
// rule and ends in beam_step_tail.  Shared here: the candidate's value, the stage 1 kernel over a rule type, the two selections a
// stage 2 can use, and the launchers' common checks.

// c(j,w): the plain search's value (same loads, ens_score, penalties and fp32 operations as beam_stage1_kernel), with EOS
// ruled out when `open` (the required search: the row still has a phrase open).  A function, so that a candidate has one value
// whoever computes it: every stage 1 rule and stage 2 of the required search call it.
// wc: w clamped into the row (stage 1 loads past-the-end lanes too); pt: the row's previous word (-1 at step 0).
template <int M>
__device__ __forceinline__ float req_value(const EnsLogp<M>& L, int64_t n, int w, int wc, int64_t pt, float base, int penal,
                                           int flags, bool open) {
    float lp = ens_score<M>(L, n, wc);
    if (pt == EOS) lp = (w == EOS) ? 0.f : NEG_PEN;           // V11.py:291-294
    else if ((w == pt && !(flags & VAG_BEAM_ALLOW_REPEAT)) ||                          // V11.py:279-280
             (penal && w == UNK && (flags & VAG_BEAM_AVOID_UNK)) ||                    // V11.py:283-284
             (open && w == EOS)) lp = NEG_PEN;                                         // phrases open: the hypothesis may not end
    return base + lp;                                         // V11.py:297
}

// After wave_topk ranked (ov, oi)[0, n) from the wave's (val, idx): oc[r] = the companion value of the r-th winner, stored by the
// lane that holds it (flat indices are unique).  Call behind a wave_lds_fence; n is uniform over the wave.  Winner by winner, every
// lane comparing its E indices in registers: one LDS read per winner, the same address in all lanes, and no branch around it
// (holder by holder with a search inside, the reads were dependent LDS round trips under divergent branches).
template <int E>
__device__ __forceinline__ void wave_companion(const int (&idx)[E], const float (&comp)[E], int n, const int* __restrict__ oi,
                                               float* __restrict__ oc) {
    for (int r = 0; r < n; ++r) {
        const int w = oi[r];
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (idx[e] == w && w != 0x7fffffff) oc[r] = comp[e];
    }
}

// Stage 1 over a rule.  Every thread forms eight candidates (c, key) of its row; the block ranks the k best of the slice under
// (key desc, flat index asc), each wave its 512 and wave 0 the 4k of those, and writes them ranked: keys to cval (no companion)
// or keys to gval and c to cval (Rule::companion: c follows its key through wave_topk, its holder stores it).  A rule has
//   companion   c travels beside a key of the rule's own (else the key is c, and neither the LDS nor the passes are paid for);
//   fin_branch  a finished row (previous word EOS; uniform over the block) has the one candidate (j, EOS) with c = base and
//               key fin_key(row, c), and reads no scores;
//   row(di, n, k_in, max_len)   the per-row set-up, called by the whole block: what key() needs, and `open` for req_value;
//   key(row, c, w, wc)          the selection key of candidate w (wc: w clamped into the row).
template <int M, class Rule>
__global__ __launch_bounds__(256) void beam_row_stage1_kernel(EnsLogp<M> L, const float* __restrict__ nll_in,
                                                              const int64_t* __restrict__ beam, const int32_t* di_state,
                                                              int di_host, int max_len, int B, int k_in, int k, int V, Rule rule,
                                                              float* __restrict__ gval, float* __restrict__ cval,
                                                              int* __restrict__ cidx, int32_t* __restrict__ n_alive, int flags) {
    constexpr bool COMP = Rule::companion;
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *n_alive = 0;   // stage 2 (next launch) counts into it
    const int penal = di > 0;                                    // (then k_in == k)
    const int64_t n = blockIdx.y;                                // hypothesis row b * k_in + j
    const int j = (int)(n % k_in);
    const int slice = blockIdx.x, slices = gridDim.x;
    const int64_t pt = penal ? beam[(int64_t)(di - 1) * B * k + n] : (int64_t)-1;
    const float base = penal ? nll_in[n] : 0.f;
    const auto row = rule.row(di, n, k_in, max_len);
    const bool open = row.open != 0;
    const int w0 = slice * CHUNK + threadIdx.x;
    float val[EPT], cv[EPT];
    int idx[EPT];
    if (Rule::fin_branch && pt == EOS) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int w = w0 + e * 256;
            const bool cand = w == EOS && w < V;
            cv[e] = base + 0.f;                                   // V11.py:291-294, :297
            val[e] = cand ? rule.fin_key(row, cv[e]) : -INFINITY;
            idx[e] = cand ? j * V + w : 0x7fffffff;
        }
    } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int w = w0 + e * 256;
            const int wc = min(w, V - 1);                         // (index clamped, result selected: all loads in flight together)
            cv[e] = req_value<M>(L, n, w, wc, pt, base, penal, flags, open);
            val[e] = w < V ? rule.key(row, cv[e], w, wc) : -INFINITY;
            idx[e] = w < V ? j * V + w : 0x7fffffff;
        }
    }
    // each wave ranks the k best of its 512 candidates by key; wave 0 then ranks the k best of those 4k
    __shared__ float wv[4 * 64], sv[4 * 64], wc_[COMP ? 4 * 64 : 1];
    __shared__ int wi[4 * 64], si[4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wv[wave * 64 + lane] = -INFINITY; wi[wave * 64 + lane] = 0x7fffffff;
    if constexpr (COMP) wc_[wave * 64 + lane] = -INFINITY;
    wave_lds_fence();
    [[maybe_unused]] const int n1 = wave_topk<EPT>(val, idx, k, sv + wave * 64, si + wave * 64, wv + wave * 64, wi + wave * 64);
    if constexpr (COMP) {
        wave_lds_fence();
        wave_companion<EPT>(idx, cv, n1, wi + wave * 64, wc_ + wave * 64);
    }
    __syncthreads();
    if (wave != 0) return;
    float v2[4];
    int i2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v2[e] = wv[e * 64 + lane]; i2[e] = wi[e * 64 + lane]; }
    const int64_t o = (n * slices + slice) * k;
    if constexpr (!COMP) {
        const int nw = wave_topk<4>(v2, i2, k, sv, si, cval + o, cidx + o);
        for (int r = nw + lane; r < k; r += 64) { cval[o + r] = -INFINITY; cidx[o + r] = 0x7fffffff; }
    } else {
        float c2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) c2[e] = wc_[e * 64 + lane];
        // (the other waves are gone: their parts of sv / si hold the ranked result and its companions)
        float* fv = sv + 64;
        float* fc = sv + 128;
        int* fi = si + 64;
        const int nw = wave_topk<4>(v2, i2, k, sv, si, fv, fi);
        wave_lds_fence();
        wave_companion<4>(i2, c2, nw, fi, fc);
        wave_lds_fence();
        for (int r = lane; r < k; r += 64) {
            const bool ok = r < nw;
            gval[o + r] = ok ? fv[r] : -INFINITY;
            cval[o + r] = ok ? fc[r] : -INFINITY;
            cidx[o + r] = ok ? fi[r] : 0x7fffffff;
        }
    }
}

// Stage 2, block-scan selection (any number of winners): the nsel best of the n entries (ps: keys in global scratch, pf: flat
// indices, pc: companion scores) under (key desc, flat index asc), best first, by block-wide arg-max rounds; every thread
// caches the best of the entries it owns and only a winner's owner rescans.  The owner stores the winner's flat index and
// companion score (and its key, where sel_key is given) and marks the entry taken with NaN, which no comparison selects -- an
// entry is read and marked by its owner only.  Called by the whole workgroup; sh: block_best's LDS.
__device__ __forceinline__ void block_scan_select(float* ps, const int* pf, const float* pc, int n, int nsel, int* sel_idx,
                                                  float* sel_val, float* sel_key, Cand* sh) {
    int mine_e = -1;
    auto scan = [&]() {
        Cand c = {-INFINITY, 0x7fffffff};
        mine_e = -1;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int f = pf[e];
            const float v = ps[e];
            if (f != 0x7fffffff && v == v && better(v, f, c.v, c.idx)) { c.v = v; c.idx = f; mine_e = e; }
        }
        return c;
    };
    Cand mine = scan();
    for (int r = 0; r < nsel; ++r) {
        const Cand c = block_best(mine, sh);
        if (c.idx == 0x7fffffff) {                                 // (nothing left: c.v is -inf)
            if (threadIdx.x == 0) { sel_idx[r] = c.idx; sel_val[r] = c.v; if (sel_key) sel_key[r] = c.v; }
        } else if (mine.idx == c.idx) {
            sel_idx[r] = c.idx;
            sel_val[r] = pc[mine_e];
            if (sel_key) sel_key[r] = c.v;
            ps[mine_e] = NAN;                                      // taken
            mine = scan();
        }
    }
}

// Stage 2, one-wave selection (at most 1024 winners): wave 0 ranks the n keys (pk, pf: LDS or global; 16 per lane) into
// (sel_key, sel_idx)[0, k), best first; then every thread looks for the winners it holds in registers (mf: flat indices, mc: their
// scores; entries threadIdx.x + 256 q) among the k chosen and stores their scores -- one LDS read per slot, the same address
// in all threads.  Called by the whole workgroup, with pk / pf visible to wave 0; tv / ti: 64 entries of LDS scratch.
constexpr int S2_WAVE = 1024;
template <int E4>
__device__ __forceinline__ void wave_rank_select(const float* pk, const int* pf, int n, int k, const int (&mf)[E4],
                                                 const float (&mc)[E4], float* tv, int* ti, float* sel_key, int* sel_idx,
                                                 float* sel_val) {
    constexpr int E2 = S2_WAVE / 64;
    static_assert(E4 * 256 == S2_WAVE, "every winner is held by one thread");
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        float s2[E2];
        int i2[E2];
#pragma unroll
        for (int e = 0; e < E2; ++e) {
            const int c = e * 64 + lane;
            s2[e] = c < n ? pk[c] : -INFINITY;
            i2[e] = c < n ? pf[c] : 0x7fffffff;
        }
        const int nsel = wave_topk<E2>(s2, i2, k, tv, ti, sel_key, sel_idx);       // ranked: slot r = r-th best
        for (int r = nsel + lane; r < k; r += 64) { sel_idx[r] = 0x7fffffff; sel_key[r] = -INFINITY; sel_val[r] = -INFINITY; }
    }
    __syncthreads();
    for (int r = 0; r < k; ++r) {
        const int w = sel_idx[r];
#pragma unroll
        for (int q = 0; q < E4; ++q)
            if (mf[q] == w && w != 0x7fffffff) sel_val[r] = mc[q];
    }
}

// What the four row-aligned launchers check alike, and the shape of their step: the members' arrays into `a`, k_in (1 at a
// host-side step 0), the slices of a row and nwin, the winners of a full step -- the scratch layout, whatever k_in is.
struct RowStep { EnsHost a; int k_in, slices; int64_t nwin; };
static int row_step_args(const float* const* logp, const int64_t* ldl, int64_t M, const float* nll, const int64_t* beam, int64_t di,
                         const int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                         int64_t B, int64_t k, int64_t V, const int32_t* n_alive, const void* scratch, int flags, RowStep& r) {
    VAG_TRY(ens_logp_args(logp, ldl, M, V, r.a));
    VAG_TRY(ens_hid_args(h_in, h_out, H, M, r.a));
    VAG_CHECK_ARG(nll && beam && n_alive && scratch);
    VAG_CHECK_ARG((flags & ~(VAG_BEAM_ALLOW_REPEAT | VAG_BEAM_AVOID_UNK)) == 0);
    VAG_CHECK_ARG(B > 0 && k > 0 && k <= 64 && V >= k && max_len > 0 && B * k <= 65535);
    VAG_CHECK_ARG(k * V < (1ll << 24));                        // select.h's keys hold 24 bits of flat index
    VAG_CHECK_ARG(di_state || (di >= 0 && di < max_len));
    r.k_in = (!di_state && di == 0) ? 1 : (int)k;
    r.slices = (int)cdiv64(V, CHUNK);
    r.nwin = B * k * r.slices * k;
    return VAG_OK;
}

// ---- diverse beam search (vag_nmt.h: vag_beam_div_step): grouped beams with a Hamming diversity penalty --------------------
// The k slots of a sentence form G groups of g = k / G consecutive slots, expanded one after another inside the step; a group
// pays `strength` for every slot of an earlier group that chose the same word at this step.  The penalty depends on what the
// earlier groups chose, so the selection is sequential over groups -- but not the candidate set:
//   stage 1 (beam_row_stage1_kernel under DivRule): each block ranks the k best of one 2048-word slice of ONE row under
//            (c desc, flat index asc), c = req_value, the plain search's value.  It takes k per slice, not g: the words earlier groups penalise number at most k - g, so a
//            row's k best by c hold at least g unpenalised words, and since penalties only lower scores nothing outside them
//            can enter the group's g best.  Winners: scratch (B, k_in, slices, k) -- a group's rows are one contiguous span.
//   stage 2: one block per sentence; for groups in order, key s = fma(-strength, cnt[w], c) over the span of the group's rows
//            (step 0: every group reads the one row), the g best under (s desc, flat index asc), appended to the list of words
//            chosen at this step.  The stored score is c, not s.  Then beam_step_tail.
// The chosen words are kept as a plain list (at most k - g <= 63 entries, one per counted slot) and cnt[w] is the number of
// entries equal to w: the append is one ballot, no search for an existing entry.
struct DivRule {                           // stage 1 of the diverse search: the key is c
    static constexpr bool companion = false, fin_branch = false;
    struct Row { static constexpr bool open = false; };
    __device__ __forceinline__ Row row(int, int64_t, int, int) const { return {}; }
    __device__ __forceinline__ float key(Row, float c, int, int) const { return c; }
    __device__ __forceinline__ float fin_key(Row, float c) const { return c; }
};

// skey: scratch of the block-scan path, one key per stage 1 winner (the owner of a winner marks it taken there with NaN, which
// no comparison selects; a NaN score is never selected by the plain search either).
template <int M>
__global__ __launch_bounds__(256) void beam_div_stage2_kernel(const float* __restrict__ cval, const int* __restrict__ cidx,
                                                              float* __restrict__ skey, int slices, int k_in, int k, int V,
                                                              int G, float strength, EnsHid<M> hid, float* __restrict__ nll,
                                                              int64_t* __restrict__ beam, int32_t* di_state, int di_host,
                                                              int max_len, int B, int64_t* __restrict__ tok_out,
                                                              int32_t* __restrict__ n_alive) {
    __shared__ Cand sh[4];
    __shared__ int sel_idx[64], chosen[64], fin[64];
    __shared__ float sel_val[64], sel_key[64];
    __shared__ float tv[64];
    __shared__ int ti[64];
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int g = k / G;
    const int per_row = slices * k;                       // stage 1 winners of one row
    const int span = (k_in == 1 ? 1 : g) * per_row;       // candidates of one group
    if (threadIdx.x < 64)                                 // finished rows (previous word EOS): neither pay nor cause penalties
        fin[threadIdx.x] = di > 0 && threadIdx.x < k && beam[((int64_t)(di - 1) * B + b) * k + threadIdx.x] == EOS;
    __syncthreads();
    int nchosen = 0;                                      // words in chosen[] (uniform over the workgroup)
    // the key of candidate (c, flat index f) for the group at hand
    auto key = [&](float c, int f) {
        if (f == 0x7fffffff || nchosen == 0) return c;
        const int j = f / V, w = f - j * V;
        if (fin[j]) return c;
        int cnt = 0;
        for (int q = 0; q < nchosen; ++q) cnt += chosen[q] == w;
        return cnt ? __fmaf_rn(-strength, (float)cnt, c) : c;
    };
    constexpr int E2 = 16;                                // one-wave path: the sentence's winners number at most 1024
    const bool one_wave = k_in * per_row <= 64 * E2;
    for (int i = 0; i < G; ++i) {
        const int64_t o = ((int64_t)b * k_in + (k_in == 1 ? 0 : i * g)) * per_row;
        const float* pv = cval + o;
        const int* pi = cidx + o;
        if (one_wave) {
            if (threadIdx.x < 64) {
                float c2[E2], s2[E2];
                int i2[E2];
#pragma unroll
                for (int e = 0; e < E2; ++e) {
                    const int c = e * 64 + lane;
                    c2[e] = c < span ? pv[c] : -INFINITY;
                    i2[e] = c < span ? pi[c] : 0x7fffffff;
                    s2[e] = key(c2[e], i2[e]);
                }
                const int nsel = wave_topk<E2>(s2, i2, g, tv, ti, sel_key + i * g, sel_idx + i * g);   // ranked: best first
                for (int r = nsel + lane; r < g; r += 64) { sel_idx[i * g + r] = 0x7fffffff; sel_val[i * g + r] = -INFINITY; }
                wave_lds_fence();
                // the model's score of every winner (flat indices are unique): its holder stores it
                const float last = nsel ? sel_key[i * g + nsel - 1] : INFINITY;
#pragma unroll
                for (int e = 0; e < E2; ++e) {
                    if (i2[e] == 0x7fffffff || s2[e] < last) continue;
                    for (int r = 0; r < nsel; ++r)
                        if (sel_idx[i * g + r] == i2[e]) sel_val[i * g + r] = c2[e];
                }
            }
        } else {
            float* ps = skey + o;
            for (int e = threadIdx.x; e < span; e += 256) ps[e] = key(pv[e], pi[e]);    // (read back by this thread only)
            block_scan_select(ps, pi, pv, span, g, sel_idx + i * g, sel_val + i * g, nullptr, sh);
        }
        __syncthreads();
        if (i + 1 < G) {
            // this group's words join the list: every wave forms the same ballot, wave 0 writes
            const int f = lane < g ? sel_idx[i * g + lane] : 0x7fffffff;
            const bool counts = f != 0x7fffffff && !fin[f / V];
            const unsigned long long m = __ballot(counts);
            if (counts && threadIdx.x < 64) chosen[nchosen + __popcll(m & ((1ull << lane) - 1ull))] = f % V;
            nchosen += __popcll(m);
            __syncthreads();
        }
    }
    beam_step_tail<M>(sel_idx, sel_val, b, k_in, k, V, hid, nll, beam, di_state, di, max_len, B, tok_out, n_alive);
}

int64_t vag_beam_div_scratch_bytes_impl(int64_t B, int64_t k, int64_t V) {
    return B * k * cdiv64(V, CHUNK) * k * 12 + 64;             // (value, flat index, key) per stage 1 winner
}

int vag_beam_div_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             int64_t groups, float strength, hipStream_t s) {
    RowStep r;
    VAG_TRY(row_step_args(logp, ldl, M, nll, beam, di, di_state, max_len, h_in, h_out, H, B, k, V, n_alive, scratch, flags, r));
    VAG_CHECK_ARG(groups >= 1 && k % groups == 0);
    VAG_CHECK_ARG(strength >= 0.f && strength <= 3.4e38f);      // (false for NaN)
    float* cval = reinterpret_cast<float*>(scratch);
    int* cidx = reinterpret_cast<int*>(cval + r.nwin);
    float* skey = cval + 2 * r.nwin;
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL((beam_row_stage1_kernel<MM, DivRule>), dim3((unsigned)r.slices, (unsigned)(B * r.k_in)), dim3(256), 0, s,
                           ens_logp<MM>(r.a), nll, beam, di_state, (int)di, (int)max_len, (int)B, r.k_in, (int)k, (int)V, DivRule{},
                           (float*)nullptr, cval, cidx, n_alive, flags);
        VAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(beam_div_stage2_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, cval, cidx, skey, r.slices, r.k_in, (int)k,
                           (int)V, (int)groups, strength, ens_hid<MM>(r.a), nll, beam, di_state, (int)di, (int)max_len, (int)B,
                           tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// ---- required phrases (vag_nmt.h: vag_beam_req_step): dynamic beam allocation (Post & Vilar 2018; Hu et al. 2019) -----------
// Every hypothesis carries {met, prog_lo, prog_hi, n}: which of its sentence's phrases it has produced, how far it is into each
// of the others, and the sum of both in words, its bank.  The k slots of a step are dealt round-robin over the banks, highest
// first, so that hypotheses further along with their phrases survive a worse score.
//   stage 1: beam_row_stage1_kernel under ReqRule: the k best of every 2048-word slice of every row by c, with one more
//            penalty: EOS is ruled out for a row that still has a phrase open.
//   stage 2: one workgroup per sentence.  The parents' states, finished flags, words, scores and the phrase table go to LDS
//            first (the state is updated in place).  The pool, by flat index j V + w: (a) the k best of all stage 1 winners,
//            (c) every row's best word (the first winner of its best slice), (b) for every open phrase of every unfinished row
//            the word that advances it, read from the members' rows through req_value -- the expression stage 1 evaluates, so
//            a candidate has one value whoever produced it.  Duplicates are dropped (a (b) entry can only meet (a), its own
//            row's (c) and its own row's earlier (b) entries), every kept entry gets the bank of its child state, its rank
//            rho among the live entries of its bank, and from (rho asc, bank desc) its slot; dead entries (value <= -5e4)
//            follow under (c desc, flat index asc).  Both orders are integer keys, so the two ranking passes are branch-free
//            counting loops over LDS (with branches in them they were dependent LDS round trips: +56 us a step at k = 12).  The k chosen slots recompute their child state and store it; then
//            beam_step_tail.
// The pool holds at most 2 k + 16 k entries (k = 12: 216, one per thread); the two ranking passes compare every entry with
// every other from LDS.  Stage 2 has TWO paths by size in its (a) selection: each thread keeps its first REQ_RC winners in
// registers (up to 256 REQ_RC = 2048 winners per sentence) and reads any further ones from the scratch at every round -- a test
// needs a shape with k_in slices k > 2048 as well as the small ones.
constexpr int REQ_P = VAG_REQUIRE_MAX_PHRASES, REQ_L = VAG_CONSTRAIN_MAX_LEN;
constexpr float REQ_LIVE = -5e4f;        // a candidate at or below it took a -1e5 somewhere
constexpr int REQ_POOL = 2 * 64 + REQ_P * 64;
constexpr int REQ_RC = 8;
constexpr int REQ_DEAD = 255;            // the class of the dead entries (a bank is at most 16 * 8 = 128)
static_assert(REQ_P == 16 && REQ_L == 8, "the state packs 16 phrases' progress into two words of 4-bit fields");

struct ReqState { unsigned met, lo, hi; int n; };

// The state of the child (row state s, word w).  Phrase c not met, progress p: the largest q <= p + 1 with the last q words of
// phrase[0..p) + [w] equal to phrase[0..q) -- exact matching, a self-overlapping phrase falls back to its longest border.
// Every loop is bounded by REQ_P or REQ_L.
__device__ __forceinline__ ReqState req_child(ReqState s, bool fin, int w, const int (*ph)[REQ_L], const int* plen) {
    if (fin) return s;
    ReqState r = {s.met, 0u, 0u, 0};
    for (int c = 0; c < REQ_P; ++c) {
        const int Lc = plen[c];
        if (Lc == 0) continue;
        if ((s.met >> c) & 1u) { r.n += Lc; continue; }
        const int p = min((int)(((c < 8 ? s.lo : s.hi) >> (4 * (c & 7))) & 15u), Lc - 1);
        int q = p + 1;
        for (; q > 0; --q) {
            if (ph[c][q - 1] != w) continue;
            bool ok = true;
            for (int i = 0; i < q - 1; ++i) ok = ok && ph[c][p + 1 - q + i] == ph[c][i];
            if (ok) break;
        }
        if (q == Lc) r.met |= 1u << c;
        else if (c < 8) r.lo |= (unsigned)q << (4 * c);
        else r.hi |= (unsigned)q << (4 * (c - 8));
        r.n += q;
    }
    return r;
}

struct ReqRule {                           // stage 1 of the required search: the key is c, EOS ruled out while a phrase is open
    const int64_t* __restrict__ required;
    const int32_t* __restrict__ state;
    static constexpr bool companion = false, fin_branch = false;
    struct Row { int open; };
    // does the row have a phrase open?  (bit c of the ballot: phrase c of the sentence is in use; step 0: nothing is met)
    __device__ __forceinline__ Row row(int di, int64_t n, int k_in, int) const {
        __shared__ int open_s;
        if (threadIdx.x < 64) {
            const int c = threadIdx.x;
            const bool used = c < REQ_P && required[((n / k_in) * REQ_P + c) * REQ_L] != 0;
            const unsigned um = (unsigned)__ballot(used);
            const unsigned met = di > 0 ? (unsigned)state[n * 4] : 0u;
            if (c == 0) open_s = (um & ~met & 0xffffu) != 0u;
        }
        __syncthreads();
        return {open_s};
    }
    __device__ __forceinline__ float key(Row, float c, int, int) const { return c; }
    __device__ __forceinline__ float fin_key(Row, float c) const { return c; }
};

// the value a candidate is ordered by: a NaN ranks last (with -inf) instead of being incomparable
__device__ __forceinline__ float req_ord(float v) { return v == v ? v : -INFINITY; }

template <int M>
__global__ __launch_bounds__(256) void beam_req_stage2_kernel(EnsLogp<M> L, const float* __restrict__ cval,
                                                              const int* __restrict__ cidx, int slices, int k_in, int k, int V,
                                                              int flags, const int64_t* __restrict__ required, int32_t* state,
                                                              EnsHid<M> hid, float* __restrict__ nll, int64_t* __restrict__ beam,
                                                              int32_t* di_state, int di_host, int max_len, int B,
                                                              int64_t* __restrict__ tok_out, int32_t* __restrict__ n_alive) {
    __shared__ Cand sh[4];
    __shared__ int sel_idx[64];
    __shared__ float sel_val[64];
    __shared__ int ph[REQ_P][REQ_L], plen[REQ_P];
    __shared__ ReqState pst[64];
    __shared__ int fin[64], prevw[64];
    __shared__ float basev[64];
    __shared__ int pf[REQ_POOL], pcls[REQ_POOL], pslot[REQ_POOL];
    __shared__ float pv[REQ_POOL];
    __shared__ unsigned long long pkey[REQ_POOL];
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int penal = di > 0;
    const bool last = di == max_len - 1;       // the finish forces EOS into this row: its word is in no hypothesis, no state moves
    // ---- everything this step reads of the search's state, into LDS before anything is written
    if (tid < REQ_P * REQ_L) {
        const int64_t w = required[(int64_t)b * REQ_P * REQ_L + tid];
        ph[tid / REQ_L][tid % REQ_L] = w == 0 ? 0 : ((w > 0 && w < V) ? (int)w : -1);      // (-1: a word no candidate is)
    }
    if (tid < 64) {
        const int j = tid;
        const bool row = penal && j < k_in;
        const int64_t o = (int64_t)b * k + j;
        const int64_t pw = row ? beam[(int64_t)(di - 1) * B * k + o] : (int64_t)-1;
        prevw[j] = (int)pw;
        fin[j] = pw == EOS;
        basev[j] = row ? nll[o] : 0.f;
        ReqState s = {0u, 0u, 0u, 0};
        if (row) { s.met = (unsigned)state[o * 4]; s.lo = (unsigned)state[o * 4 + 1]; s.hi = (unsigned)state[o * 4 + 2]; s.n = state[o * 4 + 3]; }
        pst[j] = s;
        sel_idx[j] = 0; sel_val[j] = -INFINITY;                  // (never left: (a) alone fills k slots)
    }
    __syncthreads();
    if (tid < REQ_P) {
        int Lc = 0;
        while (Lc < REQ_L && ph[tid][Lc] != 0) ++Lc;
        plen[tid] = Lc;
    }
    __syncthreads();
    const int P = 2 * k + REQ_P * k_in;                          // pool: (a) [0, k) | (c) [k, 2 k), one per row, the rest empty | (b) [2 k, P)
    const int per_row = slices * k;
    const int nwin = k_in * per_row;                             // the sentence's stage 1 winners
    const float* __restrict__ wv = cval + (int64_t)b * nwin;
    const int* __restrict__ wi = cidx + (int64_t)b * nwin;
    // ---- (c): every row's best word = the best of its slices' first winners
    if (tid < k) {
        Cand c = {-INFINITY, 0x7fffffff};
        if (tid < k_in)
            for (int s = 0; s < slices; ++s) {
                const int e = (tid * slices + s) * k;
                const int f = wi[e];
                const float v = wv[e];
                if (f != 0x7fffffff && (c.idx == 0x7fffffff || better(req_ord(v), f, req_ord(c.v), c.idx))) { c.v = v; c.idx = f; }
            }
        pf[k + tid] = c.idx; pv[k + tid] = c.v;
    }
    // ---- (a): the k best of all winners, best first: round r takes the best candidate that is worse than round r-1's
    {
        float rv[REQ_RC];
        int ri[REQ_RC];
#pragma unroll
        for (int i = 0; i < REQ_RC; ++i) {
            const int e = tid + i * 256;
            ri[i] = e < nwin ? wi[e] : 0x7fffffff;
            rv[i] = e < nwin ? wv[e] : -INFINITY;
        }
        float lasto = INFINITY;
        int lasti = -1;
        for (int r = 0; r < k; ++r) {
            Cand c = {-INFINITY, 0x7fffffff};
            float co = -INFINITY;
            auto consider = [&](float v, int f) {
                const float o = req_ord(v);
                if (f != 0x7fffffff && better(lasto, lasti, o, f) && (c.idx == 0x7fffffff || better(o, f, co, c.idx))) {
                    c.v = v; c.idx = f; co = o;
                }
            };
#pragma unroll
            for (int i = 0; i < REQ_RC; ++i) consider(rv[i], ri[i]);
            for (int e = tid + REQ_RC * 256; e < nwin; e += 256) consider(wv[e], wi[e]);      // (the second path: nwin > 2048)
            // block_best orders by the raw value: hand it the ordering value and recover the raw one from its holder
            Cand q = {co, c.idx};
            q = block_best(q, sh);
            if (q.idx != 0x7fffffff && q.idx == c.idx) { pf[r] = c.idx; pv[r] = c.v; }
            else if (q.idx == 0x7fffffff && tid == 0) { pf[r] = 0x7fffffff; pv[r] = -INFINITY; }
            lasto = q.idx == 0x7fffffff ? -INFINITY : q.v; lasti = q.idx;
        }
    }
    // ---- (b): for every open phrase of every unfinished row, the word that advances it
    for (int t = tid; t < REQ_P * k_in; t += 256) {
        const int j = t / REQ_P, c = t % REQ_P;
        int f = 0x7fffffff;
        float v = -INFINITY;
        const int Lc = plen[c];
        const ReqState s = pst[j];
        if (!fin[j] && Lc > 0 && !((s.met >> c) & 1u)) {
            const int p = min((int)(((c < 8 ? s.lo : s.hi) >> (4 * (c & 7))) & 15u), Lc - 1);
            const int w = ph[c][p];
            if (w > 0) {                                            // (inside [1, V): staged so)
                f = j * V + w;
                v = req_value<M>(L, (int64_t)b * k_in + j, w, w, (int64_t)prevw[j], basev[j], penal, flags, true);
            }
        }
        pf[2 * k + t] = f; pv[2 * k + t] = v;
    }
    __syncthreads();
    // ---- duplicates out (the earlier entry stays); every kept entry's class (its child's bank, or REQ_DEAD) and its key
    //      under (c desc, flat asc) as one integer: value bits over the inverted flat index, larger = better
    for (int e = tid; e < P; e += 256) {
        const int f = pf[e];
        bool keep = f != 0x7fffffff;
        if (keep && e >= k) {
            for (int a = 0; a < k; ++a) keep = keep && pf[a] != f;
            if (e >= 2 * k) {
                const int j = (e - 2 * k) / REQ_P;
                keep = keep && pf[k + j] != f;
                for (int a = 2 * k + j * REQ_P; a < e; ++a) keep = keep && pf[a] != f;
            }
        }
        int cls = -1;
        if (keep) {
            const int j = f / V;
            cls = req_ord(pv[e]) > REQ_LIVE ? req_child(pst[j], fin[j] != 0 || last, f - j * V, ph, plen).n : REQ_DEAD;
        }
        pcls[e] = cls;
        pkey[e] = ((unsigned long long)fkey(req_ord(pv[e])) << 32) | (unsigned long long)(0xffffffffu - (unsigned)f);
        pslot[e] = 0x7fffffff;
    }
    __syncthreads();
    // ---- rho: the rank among the entries of the same class; from it the slot key: live (rho asc, bank desc), then the dead
    //      ones by rank.  The loops are branch-free (one or two LDS loads an iteration, all threads the same address).
    for (int e = tid; e < P; e += 256) {
        const int cls = pcls[e];
        if (cls < 0) continue;
        const unsigned long long key = pkey[e];
        int rho = 0;
#pragma unroll 8
        for (int a = 0; a < P; ++a) rho += (int)((pcls[a] == cls) & (pkey[a] > key));
        pslot[e] = cls == REQ_DEAD ? 0x40000000 + rho : rho * 256 + (255 - cls);
    }
    __syncthreads();
    // ---- a kept entry's slot = the number of entries with a smaller slot key (keys are unique; a live entry's slot is >= rho)
    for (int e = tid; e < P; e += 256) {
        const int sk = pslot[e];
        if (sk == 0x7fffffff || (sk < 0x40000000 && (sk >> 8) >= k)) continue;
        int pos = 0;
#pragma unroll 8
        for (int a = 0; a < P; ++a) pos += (int)(pslot[a] < sk);
        if (pos < k) { sel_idx[pos] = pf[e]; sel_val[pos] = pv[e]; }
    }
    __syncthreads();
    // ---- the chosen slots' states (every read of `state` is behind the barriers above)
    if (tid < k) {
        const int f = sel_idx[tid];
        const int j = f / V;
        const ReqState s = req_child(pst[j], fin[j] != 0 || last, f - j * V, ph, plen);
        int32_t* o = state + ((int64_t)b * k + tid) * 4;
        o[0] = (int32_t)s.met; o[1] = (int32_t)s.lo; o[2] = (int32_t)s.hi; o[3] = s.n;
    }
    beam_step_tail<M>(sel_idx, sel_val, b, k_in, k, V, hid, nll, beam, di_state, di, max_len, B, tok_out, n_alive);
}

int64_t vag_beam_req_scratch_bytes_impl(int64_t B, int64_t k, int64_t V) {
    return B * k * cdiv64(V, CHUNK) * k * 8 + 64;              // (value, flat index) per stage 1 winner
}

int vag_beam_req_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             const int64_t* required, int32_t* state, hipStream_t s) {
    RowStep r;
    VAG_TRY(row_step_args(logp, ldl, M, nll, beam, di, di_state, max_len, h_in, h_out, H, B, k, V, n_alive, scratch, flags, r));
    VAG_CHECK_ARG(required && state);
    float* cval = reinterpret_cast<float*>(scratch);
    int* cidx = reinterpret_cast<int*>(cval + r.nwin);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL((beam_row_stage1_kernel<MM, ReqRule>), dim3((unsigned)r.slices, (unsigned)(B * r.k_in)), dim3(256), 0, s,
                           ens_logp<MM>(r.a), nll, beam, di_state, (int)di, (int)max_len, (int)B, r.k_in, (int)k, (int)V,
                           ReqRule{required, state}, (float*)nullptr, cval, cidx, n_alive, flags);
        VAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(beam_req_stage2_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, ens_logp<MM>(r.a), cval, cidx, r.slices,
                           r.k_in, (int)k, (int)V, flags, required, state, ens_hid<MM>(r.a), nll, beam, di_state, (int)di,
                           (int)max_len, (int)B, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// ---- stochastic beam search (vag_nmt.h: vag_beam_sbs_step): sampling without replacement (Kool, van Hoof, Welling 2019) ------
// A beam search over Gumbel-perturbed scores.  Every slot carries G, the perturbed score of its hypothesis (`gum`, in/out like
// nll; the root has G = 0).  A child (j,w) draws g = fl(c(j,w) + noise(j,w)), noise = select.h's sample_gumbel under the key of
// input row b k_in + j -- what vag_sample_noise writes -- and is conditioned on its parent: with Z_j = max_w g(j,w),
//     d = fl(g - Z_j);   l = -inf (d == 0), logf(-expm1f(d)) (d > -ln 2), log1pf(-expf(d)) (else);   v = fl(fl(G_j - g) + l)
//     G~(j,w) = G_j - fmaxf(v, 0) - log1pf(expf(-fabsf(v)))            (the numerically stable truncated-Gumbel form)
// so that the row's best child inherits G_j exactly and G~ is non-decreasing in g inside a row.  A finished row (previous word
// EOS) has the one candidate (j, EOS) with c = base_j and G~ = G_j, no noise read.  The step keeps the k best of all candidates
// under (G~ desc, flat index asc); the stored score is c, the model's own.  fp32, one rounding per operation, no fma.
//   stage 1 (beam_row_stage1_kernel under SbsRule): each block ranks the k best of one 2048-word slice of ONE row under
//            (g desc, flat index asc), c = req_value, the plain search's value.  G~ is monotone in g inside a row, so a row's k best by g hold everything the sentence can
//            select, and the best of them is Z_j.  Winners: scratch (B, k_in, slices, k) of (g, c, flat index), ranked per slice.
//   stage 2: one block per sentence; Z_j = the best of row j's slice winners (each slice's first entry), every winner's G~, the k
//            best under (G~ desc, flat index asc), best first; gum and, through beam_step_tail, everything else.  TWO paths by
//            size: up to 1024 winners are transformed by the whole workgroup into LDS and ranked by one wave (wave_rank_select),
//            more are ranked by block-wide arg-max rounds over their keys in the scratch (block_scan_select) -- a test needs a
//            shape with k_in slices k > 1024 (k = 12: V > 14336).
// A winner's companion value (c beside g, c beside G~) follows it through wave_topk: its holder stores it (wave_companion).
// No floating-point atomics anywhere: a decode is a pure function of (inputs, rng).
constexpr float SBS_LN2 = 0.6931472f;

__device__ __forceinline__ float sbs_condition(float G, float g, float Z) {
    const float d = __fsub_rn(g, Z);
    const float l = d == 0.f ? -INFINITY : (d > -SBS_LN2 ? logf(-expm1f(d)) : log1pf(-expf(d)));
    const float v = __fadd_rn(__fsub_rn(G, g), l);
    return __fsub_rn(__fsub_rn(G, fmaxf(v, 0.f)), log1pf(expf(-fabsf(v))));
}

struct SbsRule {                           // stage 1 of the stochastic search: key g = fl(c + noise), c beside it
    const uint64_t* __restrict__ rng;
    static constexpr bool companion = true, fin_branch = true;
    struct Row { uint64_t key; static constexpr bool open = false; };
    __device__ __forceinline__ Row row(int di, int64_t n, int, int) const { return {sample_key(rng, di, n)}; }
    __device__ __forceinline__ float key(Row r, float c, int, int wc) const { return __fadd_rn(c, sample_gumbel(r.key, wc)); }
    __device__ __forceinline__ float fin_key(Row, float c) const { return c; }      // (stage 2 gives it G_j whatever this is; no noise read)
};

// skey: scratch of the block-scan path, one key (G~) per stage 1 winner; the owner of a winner marks it taken there with NaN.
template <int M>
__global__ __launch_bounds__(256) void beam_sbs_stage2_kernel(const float* __restrict__ gval, const float* __restrict__ cval,
                                                              const int* __restrict__ cidx, float* __restrict__ skey, int slices,
                                                              int k_in, int k, int V, EnsHid<M> hid, float* __restrict__ nll,
                                                              float* __restrict__ gum, int64_t* __restrict__ beam,
                                                              int32_t* di_state, int di_host, int max_len, int B,
                                                              int64_t* __restrict__ tok_out, int32_t* __restrict__ n_alive) {
    __shared__ Cand sh[4];
    __shared__ int sel_idx[64], fin[64], ti[64];
    __shared__ float sel_val[64], sel_gum[64], Gp[64], Zr[64], tv[64];
    __shared__ float lk[S2_WAVE];                         // the one-wave path's keys and flat indices
    __shared__ int li[S2_WAVE];
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int b = blockIdx.x;
    const int per_row = slices * k;                       // stage 1 winners of one row
    const int nwin = k_in * per_row;                      // ... of the sentence
    const float* __restrict__ pg = gval + (int64_t)b * nwin;
    const float* __restrict__ pc = cval + (int64_t)b * nwin;
    const int* __restrict__ pi = cidx + (int64_t)b * nwin;
    // the parents: G_j, finished flags and Z_j = the best g of the row (every slice's first winner is its best), before anything is written
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;
        const bool row = j < k_in;
        fin[j] = di > 0 && row && beam[((int64_t)(di - 1) * B + b) * k + j] == EOS;
        Gp[j] = (di > 0 && row) ? gum[(int64_t)b * k + j] : 0.f;
        float z = -INFINITY;
        if (row)
            for (int s = 0; s < slices; ++s) z = fmaxf(z, pg[(j * slices + s) * k]);
        Zr[j] = z;
    }
    __syncthreads();
    // G~ of winner (g, flat index f)
    auto key = [&](float g, int f) {
        if (f == 0x7fffffff) return -INFINITY;
        const int j = f / V;
        return fin[j] ? Gp[j] : sbs_condition(Gp[j], g, Zr[j]);
    };
    if (nwin <= S2_WAVE) {
        // every thread transforms its (at most four) winners into LDS and keeps their flat indices and scores in registers
        constexpr int E4 = S2_WAVE / 256;
        int mf[E4];
        float mc[E4];
#pragma unroll
        for (int q = 0; q < E4; ++q) {
            const int e = threadIdx.x + q * 256;
            const bool ok = e < nwin;
            mf[q] = ok ? pi[e] : 0x7fffffff;
            mc[q] = ok ? pc[e] : -INFINITY;
            const float g = ok ? pg[e] : -INFINITY;
            if (ok) { li[e] = mf[q]; lk[e] = key(g, mf[q]); }
        }
        __syncthreads();
        wave_rank_select<E4>(lk, li, nwin, k, mf, mc, tv, ti, sel_gum, sel_idx, sel_val);
    } else {
        float* ps = skey + (int64_t)b * nwin;
        for (int e = threadIdx.x; e < nwin; e += 256) ps[e] = key(pg[e], pi[e]);       // (read back by this thread only)
        block_scan_select(ps, pi, pc, nwin, k, sel_idx, sel_val, sel_gum, sh);
    }
    __syncthreads();
    if (threadIdx.x < k) {
        if (sel_idx[threadIdx.x] == 0x7fffffff) sel_idx[threadIdx.x] = 0;       // (fewer than k candidates: cannot happen with V >= k; never out of range)
        gum[(int64_t)b * k + threadIdx.x] = sel_gum[threadIdx.x];
    }
    __syncthreads();
    beam_step_tail<M>(sel_idx, sel_val, b, k_in, k, V, hid, nll, beam, di_state, di, max_len, B, tok_out, n_alive);
}

int64_t vag_beam_sbs_scratch_bytes_impl(int64_t B, int64_t k, int64_t V) {
    return B * k * cdiv64(V, CHUNK) * k * 16 + 64;             // (g, c, flat index, G~) per stage 1 winner
}

int vag_beam_sbs_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             const uint64_t* rng, float* gum, hipStream_t s) {
    RowStep r;
    VAG_TRY(row_step_args(logp, ldl, M, nll, beam, di, di_state, max_len, h_in, h_out, H, B, k, V, n_alive, scratch, flags, r));
    VAG_CHECK_ARG(rng && gum);
    float* gval = reinterpret_cast<float*>(scratch);
    float* cval = gval + r.nwin;
    int* cidx = reinterpret_cast<int*>(gval + 2 * r.nwin);
    float* skey = gval + 3 * r.nwin;
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL((beam_row_stage1_kernel<MM, SbsRule>), dim3((unsigned)r.slices, (unsigned)(B * r.k_in)), dim3(256), 0, s,
                           ens_logp<MM>(r.a), nll, beam, di_state, (int)di, (int)max_len, (int)B, r.k_in, (int)k, (int)V, SbsRule{rng},
                           gval, cval, cidx, n_alive, flags);
        VAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(beam_sbs_stage2_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, gval, cval, cidx, skey, r.slices, r.k_in,
                           (int)k, (int)V, ens_hid<MM>(r.a), nll, gum, beam, di_state, (int)di, (int)max_len, (int)B, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// Greedy form (V11.py:207-226 on the ensemble's scores): one block per hypothesis row, the arg-max of the combined row under
// (score desc, index asc) -- the rule of the single model's arg-max (head.hip, lse_nll_kernel).  One pass over the M rows.
template <int M>
__global__ __launch_bounds__(256) void ens_argmax_kernel(EnsLogp<M> L, int V, int64_t* __restrict__ out) {
    __shared__ Cand sh[4];
    const int64_t n = blockIdx.x;
    Cand c = {-INFINITY, 0x7fffffff};
#pragma unroll 4
    for (int w = threadIdx.x; w < V; w += 256) {
        const float v = ens_score<M>(L, n, w);
        if (better(v, w, c.v, c.idx)) { c.v = v; c.idx = w; }
    }
    const Cand r = block_best(c, sh);
    if (threadIdx.x == 0) out[n] = r.idx == 0x7fffffff ? 0 : r.idx;      // (an all-NaN row: the padding word, never out of range)
}


int vag_ens_argmax_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t N, int64_t V, int64_t* out,
                          hipStream_t s) {
    EnsHost a;
    VAG_TRY(ens_logp_args(logp, ldl, M, V, a));
    VAG_CHECK_ARG(out && N > 0 && N < (1ll << 31) && V < (1ll << 31));
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL(ens_argmax_kernel<MM>, dim3((unsigned)N), dim3(256), 0, s, ens_logp<MM>(a), (int)V, out);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// ---- attention rows of the search and of forced decoding ----------------------------------------------------------------
// The decoder steps write their Bahdanau attention alpha (N, Tp) (layers/NMT_Decoder.py:27-51, :124); the search keeps it per
// step in attn_hist (max_len, B k, Tp) and the finish resolves it through the same back-pointers as the words.  M members are
// combined by the mean of their rows, sum_m a_m / M in member order: M = 1 copies the row bit for bit, two identical rows give
// (a + a) / 2 == a exactly.  "Soft attention of the chosen path", not a trained aligner.
template <int M>
__device__ __forceinline__ float4 alpha_mean4(const EnsRows<M>& A, int64_t off) {
    float4 v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = *reinterpret_cast<const float4*>(A.p[m] + off);
    if constexpr (M == 1) {
        return v[0];
    } else {
        float4 r = v[0];
#pragma unroll
        for (int m = 1; m < M; ++m) { r.x += v[m].x; r.y += v[m].y; r.z += v[m].z; r.w += v[m].w; }
        r.x /= (float)M; r.y /= (float)M; r.z /= (float)M; r.w /= (float)M;
        return r;
    }
}
template <int M>
__device__ __forceinline__ float alpha_mean1(const EnsRows<M>& A, int64_t off) {
    float v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = A.p[m][off];
    if constexpr (M == 1) {
        return v[0];
    } else {
        float r = v[0];
#pragma unroll
        for (int m = 1; m < M; ++m) r += v[m];
        return r / (float)M;
    }
}

// Step di's rows into attn_hist[di]: N = B rows at step 0 (one hypothesis per sentence), B k afterwards; the rows of one step
// are contiguous on both sides, so the copy is flat.  The step index is the one the captured expansions read (this launch
// precedes the expansion that advances it).  VEC: 16-byte loads and stores.
template <int M, bool VEC>
__global__ __launch_bounds__(256) void beam_attn_record_kernel(EnsRows<M> A, float* __restrict__ hist, const int32_t* di_state,
                                                               int di_host, int max_len, int B, int k, int Tp) {
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int64_t slab = (int64_t)B * k * Tp;
    const int64_t total = di == 0 ? (int64_t)B * Tp : slab;
    float* __restrict__ out = hist + (int64_t)di * slab;
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i * 4 < total; i += stride)
            *reinterpret_cast<float4*>(out + i * 4) = alpha_mean4<M>(A, i * 4);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) out[i] = alpha_mean1<M>(A, i);
    }
}

// a host array of M attention matrices: every entry is checked before anything is enqueued; al = all are 16-byte aligned
static int ens_alpha_args(const float* const* alpha, int64_t M, bool& al) {
    VAG_CHECK_ARG(alpha && M >= 1 && M <= VAG_ENS_MAX);
    al = true;
    for (int m = 0; m < (int)M; ++m) {
        VAG_CHECK_ARG(alpha[m] != nullptr);
        al = al && aligned16(alpha[m]);
    }
    return VAG_OK;
}

int vag_beam_attn_record_launch(const float* const* alpha, int64_t M, float* attn_hist, int64_t di, const int32_t* di_state,
                                int64_t max_len, int64_t B, int64_t k, int64_t Tp, hipStream_t s) {
    bool al;
    VAG_TRY(ens_alpha_args(alpha, M, al));
    VAG_CHECK_ARG(attn_hist && B > 0 && k > 0 && k <= 64 && Tp > 0 && max_len > 0);
    VAG_CHECK_ARG(B < (1ll << 31) && Tp < (1ll << 31) && max_len < (1ll << 31) && B * k * Tp < (1ll << 40));
    VAG_CHECK_ARG(di_state || (di >= 0 && di < max_len));
    const int64_t rows = (!di_state && di == 0) ? B : B * k;
    const bool vec = al && aligned16(attn_hist) && (Tp & 3) == 0;
    const int64_t work = vec ? rows * Tp / 4 : rows * Tp;
    const int64_t nb = cdiv64(work, 256);
    const dim3 grid((unsigned)(nb < 4096 ? nb : 4096));
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        if (vec)
            hipLaunchKernelGGL((beam_attn_record_kernel<MM, true>), grid, dim3(256), 0, s, ens_rows<MM>(alpha), attn_hist, di_state,
                               (int)di, (int)max_len, (int)B, (int)k, (int)Tp);
        else
            hipLaunchKernelGGL((beam_attn_record_kernel<MM, false>), grid, dim3(256), 0, s, ens_rows<MM>(alpha), attn_hist, di_state,
                               (int)di, (int)max_len, (int)B, (int)k, (int)Tp);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// One output row of attention and its arg-max, by a group of 16 lanes (four rows per wave): the mean of the M source rows at
// float offset `off` (live) or zeros, columns [0, Ts) of it; pos = the arg-max column, lowest index among equal values, -1 for a
// zeroed row.  vin / vout: the source rows / the output row take 16-byte accesses.
constexpr int ROW_LANES = 16;
template <int M>
__device__ __forceinline__ void attn_row(const EnsRows<M>& A, int64_t off, bool live, int Ts, bool vin, bool vout,
                                         float* __restrict__ out, int64_t* pos) {
    const int l = threadIdx.x & (ROW_LANES - 1);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c0 = l * 4; c0 < Ts; c0 += ROW_LANES * 4) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            if (vin) {                                   // (the source row is padded to a multiple of 4 columns: c0 + 3 is inside)
                const float4 q = alpha_mean4<M>(A, off + c0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c0 + i < Ts) v[i] = alpha_mean1<M>(A, off + c0 + i);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < Ts && better(v[i], c0 + i, bv, bi)) { bv = v[i]; bi = c0 + i; }
        }
        if (vout) {
            *reinterpret_cast<float4*>(out + c0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < Ts) out[c0 + i] = v[i];
        }
    }
#pragma unroll
    for (int o = ROW_LANES / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (l == 0) *pos = !live ? -1 : (bi == 0x7fffffff ? 0 : bi);          // (a live all-NaN row: column 0, never out of range)
}

// The finish (V11.py:315-324): force EOS in the last row, normalise each of the k final hypotheses' scores by its number of
// tokens > 3, rank them under (score desc, slot asc) and resolve the n best into out (B, n, max_len), each row with EOS forced
// in its last position and 0 past the written rows; scores (B, n; may be NULL) in descending order.  n = 1 is the search's
// result (the reference's final top-1).  `steps` rows of history were written (fewer than max_len after an early stop).
// Lane j < k of wave 0 owns final hypothesis j: it walks the back-pointers once for the length (steps dependent reads, once per
// decode), ranks itself by counting the hypotheses that beat it (k <= 64: one wave holds every score), and, if among the n
// best, walks them again into its row.  No de-duplication: a hypothesis that took a -1e5 step can cut to the token list of a
// finished one; its score is below -1e4.
// ALIGN (256 threads, else 64) also resolves the attention: while lane j writes its row it leaves, in src_pos (b, rank, t), the
// attn_hist row that produced word t: step t's row of the ancestor slot after step t-1 (the parent of the slot that holds word
// t), sentence b's single row at t = 0, -1 past the first EOS and from row `steps` on.  After a barrier the whole workgroup
// copies rows, 16 lanes each with 16-byte accesses, cropping Tp to Ts, and replaces each src_pos entry by its row's arg-max.
constexpr int FIN_LDS = 4096;            // (word, parent) pairs of one sentence's history kept in LDS: steps * k <= 4096
template <bool ALIGN>
__global__ __launch_bounds__(ALIGN ? 256 : 64) void beam_finish_kernel(const float* __restrict__ nll, const int64_t* __restrict__ beam,
                                                                       const float* __restrict__ hist, int max_len, int steps, int B,
                                                                       int k, int n, int Tp, int Ts, bool vin, bool vout,
                                                                       int64_t* __restrict__ out, float* __restrict__ scores,
                                                                       float* __restrict__ attention, int64_t* src_pos,
                                                                       int64_t* __restrict__ slots) {
    const int b = blockIdx.x, j = threadIdx.x;
    const int64_t* par = beam + (int64_t)max_len * B * k;
    // the sentence's history into LDS first (coalesced rows of k words / k parents per step): the walks below are chains of
    // `steps` dependent reads -- from global memory 80 steps took ~52 us per call (a memory round trip each), from LDS ~5
    __shared__ int hw[FIN_LDS], hp[FIN_LDS];
    const bool lds = steps * k <= FIN_LDS;
    if (lds) {
        for (int e = j; e < steps * k; e += (ALIGN ? 256 : 64)) {
            const int t = e / k, p = e - t * k;
            const int64_t o = ((int64_t)t * B + b) * k + p;
            hw[e] = (int)beam[o];
            hp[e] = (int)par[o];
        }
        __syncthreads();
    }
    // one step back along a hypothesis: the word slot p holds in row t; p becomes the slot it extends
    auto back = [&](int t, int& p) {
        const int64_t o = ((int64_t)t * B + b) * k + p;
        const int w = lds ? hw[t * k + p] : (int)beam[o];
        p = lds ? hp[t * k + p] : (int)par[o];
        return w;
    };
    if (!ALIGN || j < 64) {
        float sc = -INFINITY;
        int first_eos = max_len;                       // first row whose word is EOS (row max_len-1 is forced to EOS)
        if (j < k) {
            int len = 0, p = j;
            for (int t = steps - 1; t >= 0; --t) {
                const int w = back(t, p);
                if (t < max_len - 1) len += w > 3;         // row max_len-1 is forced to EOS (= 3), which never counts
                if (ALIGN && (w == EOS || t == max_len - 1)) first_eos = t;
            }
            if (len < 1) len = 1;
            sc = nll[(int64_t)b * k + j] / (float)len;
        }
        int rank = 0;
        for (int i = 0; i < k; ++i) {
            const float ov = __shfl(sc, i, 64);
            rank += better(ov, i, sc, j) ? 1 : 0;
        }
        if (j < k && rank < n) {
            int64_t* row = out + ((int64_t)b * n + rank) * max_len;
            int64_t* arow = ALIGN ? src_pos + ((int64_t)b * n + rank) * max_len : nullptr;
            for (int t = steps; t < max_len; ++t) {
                row[t] = 0;
                if (ALIGN) arow[t] = -1;
            }
            int p = j;
            for (int t = steps - 1; t >= 0; --t) {
                row[t] = back(t, p);
                if (ALIGN) arow[t] = t > first_eos ? -1 : (int64_t)t * B * k + (t > 0 ? (int64_t)b * k + p : (int64_t)b);
            }
            row[max_len - 1] = EOS;
            if (scores) scores[(int64_t)b * n + rank] = sc;
            if (slots) slots[(int64_t)b * n + rank] = j;           // (vag_beam_finish_nbest_slots: the hypothesis's final slot)
        }
    }
    if constexpr (ALIGN) {
        __syncthreads();                                // the rows' sources are in src_pos (written and read by this workgroup)
        EnsRows<1> A;
        A.p[0] = hist;
        const int nrows = n * max_len;
        for (int r = j / ROW_LANES; r < nrows; r += 256 / ROW_LANES) {
            const int64_t g = (int64_t)b * nrows + r;
            const int64_t srow = __atomic_load_n(src_pos + g, __ATOMIC_RELAXED);
            // (lane 0 replaces the entry its group has just read: what it stores depends on the value loaded)
            attn_row<1>(A, srow * Tp, srow >= 0, Ts, vin, vout, attention + g * Ts, src_pos + g);
        }
    }
}

// what the three forms of the finish check alike
static bool finish_args(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                        const int64_t* out) {
    return nll && beam && out && max_len > 0 && steps > 0 && steps <= max_len && B > 0 && k > 0 && k <= 64;
}

int vag_beam_finish_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                           int64_t* out, float* best, hipStream_t s) {
    VAG_CHECK_ARG(finish_args(nll, beam, max_len, steps, B, k, out));
    hipLaunchKernelGGL(beam_finish_kernel<false>, dim3((unsigned)B), dim3(64), 0, s, nll, beam, nullptr, (int)max_len, (int)steps,
                       (int)B, (int)k, 1, 0, 0, false, false, out, best, nullptr, nullptr, nullptr);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// slots: NULL, or (B, n) that receives every ranked hypothesis's final slot (vag_beam_finish_nbest_slots)
static int finish_nbest(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n,
                        int64_t* out, float* scores, int64_t* slots, hipStream_t s) {
    VAG_CHECK_ARG(finish_args(nll, beam, max_len, steps, B, k, out) && scores);
    VAG_CHECK_ARG(n >= 1 && n <= k && B < (1ll << 31));
    hipLaunchKernelGGL(beam_finish_kernel<false>, dim3((unsigned)B), dim3(64), 0, s, nll, beam, nullptr, (int)max_len, (int)steps,
                       (int)B, (int)k, (int)n, 0, 0, false, false, out, scores, nullptr, nullptr, slots);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_beam_finish_nbest_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                 int64_t n, int64_t* out, float* scores, hipStream_t s) {
    return finish_nbest(nll, beam, max_len, steps, B, k, n, out, scores, nullptr, s);
}

int vag_beam_finish_nbest_slots_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                       int64_t n, int64_t* out, float* scores, int64_t* slots, hipStream_t s) {
    VAG_CHECK_ARG(slots != nullptr);
    return finish_nbest(nll, beam, max_len, steps, B, k, n, out, scores, slots, s);
}

int vag_beam_finish_align_launch(const float* nll, const int64_t* beam, const float* attn_hist, int64_t max_len, int64_t steps,
                                 int64_t B, int64_t k, int64_t n, int64_t Tp, int64_t Ts, int64_t* out, float* scores,
                                 float* attention, int64_t* src_pos, hipStream_t s) {
    VAG_CHECK_ARG(finish_args(nll, beam, max_len, steps, B, k, out) && scores);
    VAG_CHECK_ARG(n >= 1 && n <= k && B < (1ll << 31));
    VAG_CHECK_ARG(attn_hist && attention && src_pos && Ts > 0 && Ts <= Tp && Tp < (1ll << 31) && max_len < (1ll << 31));
    VAG_CHECK_ARG(B * k * Tp < (1ll << 40));
    const bool vin = (Tp & 3) == 0 && aligned16(attn_hist);
    const bool vout = (Ts & 3) == 0 && aligned16(attention);
    hipLaunchKernelGGL(beam_finish_kernel<true>, dim3((unsigned)B), dim3(256), 0, s, nll, beam, attn_hist, (int)max_len, (int)steps,
                       (int)B, (int)k, (int)n, (int)Tp, (int)Ts, vin, vout, out, scores, attention, src_pos, nullptr);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// ---- penalised beam search (vag_nmt.h: vag_beam_cover, vag_beam_pen_step, vag_beam_finish_pen): GNMT length and coverage
// penalties (Wu et al. 2016, section 7), applied at the finish or, stepwise, while hypotheses compete for slots ---------------
// Every slot carries len (its words > 3), cov (Tp floats: the summed attention rows of its words up to its first EOS) and
// cp (the coverage penalty of cov); the host supplies the divisor lp[L] and the reward bonus[L], L = max(len, 1), as tables, so
// the device evaluates no powf.  s = fl(fl(fl(c + bonus[L]) / lp[L]) + cp), one rounding per operation.
//   cover:   one wave per hypothesis row: cov_row = cov + a (a = the members' mean attention row; cov alone for a finished row,
//            a alone at step 0) and cp_row = beta * sum over unmasked columns of logf(min(max(cov_row, 1e-10), 1)).
//   stage 1: beam_row_stage1_kernel under PenRule: each block ranks the k best of one 2048-word slice of
//            ONE row under (key desc, flat index asc) and keeps c beside the key.  The key is the FINAL one -- s(c, len', cp_row[j])
//            with len' = len_j + (w > 3), or c when not stepwise -- so the sentence's k best under that order are among the
//            slices' k best, whatever the class (w <= 3 or w > 3) of a word: nothing has to be monotone in c.
//   stage 2: one block per sentence ranks the k best of all slice winners (one wave up to 1024 winners, block-wide arg-max rounds
//            beyond), stores len', cp_row[parent] and cov_row[parent] by slot; then beam_step_tail.
//   finish:  beam_finish_kernel's ranking by s from the carried (nll, lens, cpen): no length walk.
__device__ __forceinline__ float pen_score(float c, int len, float cp, const float* __restrict__ lp, const float* __restrict__ bonus,
                                           int max_len) {
    const int L = min(max(len, 1), max_len);              // (the tables hold max_len + 1 entries: never out of range)
    return __fadd_rn(__fadd_rn(c, bonus[L]) / lp[L], cp);
}

// Columns are dealt to the 64 lanes in quads: lane l owns columns i with (i / 4) % 64 == l.  cp's sum: every lane adds its
// unmasked columns' terms in increasing column order from +0, then the 64 partial sums are combined by the xor butterfly
// o = 32, 16, .. 1 (p_l += p_{l ^ o}; the same value in every lane), and cp = fl(beta * sum).
template <int M>
__global__ __launch_bounds__(64) void beam_cover_kernel(EnsRows<M> A, const float* __restrict__ mask, const float* __restrict__ cov,
                                                        const int64_t* __restrict__ beam, const int32_t* di_state, int di_host,
                                                        int max_len, int B, int k, int Tp, float beta, bool vec,
                                                        float* __restrict__ cov_row, float* __restrict__ cp_row) {
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int k_in = di == 0 ? 1 : k;
    const int64_t n = blockIdx.x;                                // hypothesis row b * k_in + j
    if (n >= (int64_t)B * k_in) return;
    const int lane = threadIdx.x;
    if (beta == 0.f) {                                           // no coverage term: cp is +0 and nothing else is touched
        if (lane == 0) cp_row[n] = 0.f;
        return;
    }
    const int b = (int)(n / k_in);
    const bool first = di == 0;
    const bool fin = !first && beam[(int64_t)(di - 1) * B * k + n] == EOS;
    const float* __restrict__ mrow = mask + (int64_t)b * Tp;
    const int64_t off = n * Tp;
    float part = 0.f;
    for (int c0 = lane * 4; c0 < Tp; c0 += 256) {
        float a[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f}, mk[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {                                               // (Tp is a multiple of 4: c0 + 3 is inside the row)
            if (!fin) { const float4 q = alpha_mean4<M>(A, off + c0); a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w; }
            if (!first) { const float4 q = *reinterpret_cast<const float4*>(cov + off + c0); c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w; }
            const float4 q = *reinterpret_cast<const float4*>(mrow + c0);
            mk[0] = q.x; mk[1] = q.y; mk[2] = q.z; mk[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < Tp) {
                    if (!fin) a[i] = alpha_mean1<M>(A, off + c0 + i);
                    if (!first) c[i] = cov[off + c0 + i];
                    mk[i] = mrow[c0 + i];
                }
        }
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = first ? a[i] : (fin ? c[i] : __fadd_rn(c[i], a[i]));
            if (c0 + i < Tp && mk[i] != 0.f) part = __fadd_rn(part, logf(fminf(fmaxf(v[i], 1e-10f), 1.f)));
        }
        if (vec) {
            *reinterpret_cast<float4*>(cov_row + off + c0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < Tp) cov_row[off + c0 + i] = v[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part = __fadd_rn(part, __shfl_xor(part, o, 64));
    if (lane == 0) cp_row[n] = __fmul_rn(beta, part);
}

int vag_beam_cover_launch(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam, int64_t di,
                          const int32_t* di_state, int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row,
                          float* cp_row, hipStream_t s) {
    VAG_CHECK_ARG(beta >= 0.f && beta <= 3.4e38f);               // (false for NaN)
    VAG_CHECK_ARG(cp_row && beam && B > 0 && k > 0 && k <= 64 && Tp > 0 && max_len > 0 && B * k <= 65535);
    VAG_CHECK_ARG(Tp < (1ll << 31) && max_len < (1ll << 31) && B * k * Tp < (1ll << 40));
    VAG_CHECK_ARG(di_state || (di >= 0 && di < max_len));
    const int64_t rows = (!di_state && di == 0) ? B : B * k;
    if (beta == 0.f) {
        VAG_CHECK_ARG(M >= 1 && M <= VAG_ENS_MAX);
        hipLaunchKernelGGL(beam_cover_kernel<1>, dim3((unsigned)rows), dim3(64), 0, s, EnsRows<1>{}, mask, cov, beam, di_state, (int)di,
                           (int)max_len, (int)B, (int)k, (int)Tp, beta, false, cov_row, cp_row);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    bool al;
    VAG_TRY(ens_alpha_args(alpha, M, al));
    VAG_CHECK_ARG(mask && cov && cov_row);
    const bool vec = al && (Tp & 3) == 0 && aligned16(mask) && aligned16(cov) && aligned16(cov_row);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL(beam_cover_kernel<MM>, dim3((unsigned)rows), dim3(64), 0, s, ens_rows<MM>(alpha), mask, cov, beam, di_state,
                           (int)di, (int)max_len, (int)B, (int)k, (int)Tp, beta, vec, cov_row, cp_row);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

struct PenRule {                           // stage 1 of the penalised search: key s(c, len', cp_row) when stepwise (else c), c beside it
    const int32_t* __restrict__ lens;
    const float* __restrict__ cp_row;
    const float* __restrict__ lp_tab;
    const float* __restrict__ bonus;
    int stepwise;
    static constexpr bool companion = true, fin_branch = true;
    struct Row { int len0, len1, max_len; float cp; static constexpr bool open = false; };
    __device__ __forceinline__ Row row(int di, int64_t n, int, int max_len) const {
        const int len0 = di > 0 ? lens[n] : 0;                       // the row's words > 3 (step 0 ignores the buffer)
        const int len1 = len0 + (di < max_len - 1 ? 1 : 0);          // ... with one more (the last row's word never counts)
        return {len0, len1, max_len, stepwise ? cp_row[n] : 0.f};
    }
    __device__ __forceinline__ float key(Row r, float c, int w, int) const {
        return stepwise ? pen_score(c, w > 3 ? r.len1 : r.len0, r.cp, lp_tab, bonus, r.max_len) : c;
    }
    __device__ __forceinline__ float fin_key(Row r, float c) const {      // (a finished row: frozen length)
        return stepwise ? pen_score(c, r.len0, r.cp, lp_tab, bonus, r.max_len) : c;
    }
};

// gval: the winners' keys; the block-scan path marks a taken winner there with NaN, which no comparison selects.
template <int M>
__global__ __launch_bounds__(256) void beam_pen_stage2_kernel(float* __restrict__ gval, const float* __restrict__ cval,
                                                              const int* __restrict__ cidx, int slices, int k_in, int k, int V,
                                                              EnsHid<M> hid, float* __restrict__ nll, int32_t* __restrict__ lens,
                                                              const float* __restrict__ cp_row, float* __restrict__ cpen,
                                                              const float* __restrict__ cov_row, float* __restrict__ cov, int Tp,
                                                              bool vcov, int64_t* __restrict__ beam, int32_t* di_state, int di_host,
                                                              int max_len, int B, int64_t* __restrict__ tok_out,
                                                              int32_t* __restrict__ n_alive) {
    __shared__ Cand sh[4];
    __shared__ int sel_idx[64], fin[64], plen[64], ti[64];
    __shared__ float sel_val[64], sel_key[64], tv[64];
    int di;
    if (!step_index(di_state, di_host, max_len, di)) return;
    const int b = blockIdx.x;
    const int per_row = slices * k;                       // stage 1 winners of one row
    const int nwin = k_in * per_row;                      // ... of the sentence
    float* __restrict__ pg = gval + (int64_t)b * nwin;
    const float* __restrict__ pc = cval + (int64_t)b * nwin;
    const int* __restrict__ pi = cidx + (int64_t)b * nwin;
    // the parents' finished flags and lengths, before anything is written
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;
        const bool row = di > 0 && j < k_in;
        fin[j] = row && beam[((int64_t)(di - 1) * B + b) * k + j] == EOS;
        plen[j] = row ? lens[(int64_t)b * k + j] : 0;
    }
    if (nwin <= S2_WAVE) {
        // every thread keeps its (at most four) winners' flat indices and scores in registers
        constexpr int E4 = S2_WAVE / 256;
        int mf[E4];
        float mc[E4];
#pragma unroll
        for (int q = 0; q < E4; ++q) {
            const int e = threadIdx.x + q * 256;
            const bool ok = e < nwin;
            mf[q] = ok ? pi[e] : 0x7fffffff;
            mc[q] = ok ? pc[e] : -INFINITY;
        }
        wave_rank_select<E4>(pg, pi, nwin, k, mf, mc, tv, ti, sel_key, sel_idx, sel_val);
    } else {
        block_scan_select(pg, pi, pc, nwin, k, sel_idx, sel_val, nullptr, sh);
    }
    __syncthreads();
    if (threadIdx.x < k) {
        if (sel_idx[threadIdx.x] == 0x7fffffff) sel_idx[threadIdx.x] = 0;       // (fewer than k candidates: cannot happen with V >= k; never out of range)
        const int f = sel_idx[threadIdx.x];
        const int j = f / V, w = f - j * V;
        lens[(int64_t)b * k + threadIdx.x] = plen[j] + ((w > 3 && !fin[j] && di < max_len - 1) ? 1 : 0);
        cpen[(int64_t)b * k + threadIdx.x] = cp_row[(int64_t)b * k_in + j];
    }
    __syncthreads();
    if (cov) {                                            // the chosen parents' coverage rows, by slot
        if (vcov) {
            const int T4 = Tp >> 2;
            for (int e = threadIdx.x; e < k * T4; e += 256) {
                const int r = e / T4, c = e - r * T4;
                reinterpret_cast<float4*>(cov + ((int64_t)b * k + r) * Tp)[c] =
                    reinterpret_cast<const float4*>(cov_row + ((int64_t)b * k_in + sel_idx[r] / V) * Tp)[c];
            }
        } else {
            for (int e = threadIdx.x; e < k * Tp; e += 256) {
                const int r = e / Tp, c = e - r * Tp;
                cov[((int64_t)b * k + r) * Tp + c] = cov_row[((int64_t)b * k_in + sel_idx[r] / V) * Tp + c];
            }
        }
    }
    beam_step_tail<M>(sel_idx, sel_val, b, k_in, k, V, hid, nll, beam, di_state, di, max_len, B, tok_out, n_alive);
}

int64_t vag_beam_pen_scratch_bytes_impl(int64_t B, int64_t k, int64_t V) {
    return B * k * cdiv64(V, CHUNK) * k * 12 + 64;             // (key, c, flat index) per stage 1 winner
}

int vag_beam_pen_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             int32_t* lens, const float* cp_row, float* cpen, const float* cov_row, float* cov, int64_t Tp,
                             const float* lp, const float* bonus, int stepwise, hipStream_t s) {
    RowStep r;
    VAG_TRY(row_step_args(logp, ldl, M, nll, beam, di, di_state, max_len, h_in, h_out, H, B, k, V, n_alive, scratch, flags, r));
    VAG_CHECK_ARG(lens && cp_row && cpen && lp && bonus);
    VAG_CHECK_ARG((cov == nullptr) == (cov_row == nullptr));
    VAG_CHECK_ARG(stepwise == 0 || stepwise == 1);
    VAG_CHECK_ARG(Tp >= 1 && Tp < (1ll << 31) && B * k * Tp < (1ll << 40) && max_len < (1ll << 31));
    float* gval = reinterpret_cast<float*>(scratch);
    float* cval = gval + r.nwin;
    int* cidx = reinterpret_cast<int*>(gval + 2 * r.nwin);
    const bool vcov = cov && (Tp & 3) == 0 && aligned16(cov) && aligned16(cov_row);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL((beam_row_stage1_kernel<MM, PenRule>), dim3((unsigned)r.slices, (unsigned)(B * r.k_in)), dim3(256), 0, s,
                           ens_logp<MM>(r.a), nll, beam, di_state, (int)di, (int)max_len, (int)B, r.k_in, (int)k, (int)V,
                           PenRule{lens, cp_row, lp, bonus, stepwise}, gval, cval, cidx, n_alive, flags);
        VAG_LAUNCH_CHECK();
        hipLaunchKernelGGL(beam_pen_stage2_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, gval, cval, cidx, r.slices, r.k_in, (int)k,
                           (int)V, ens_hid<MM>(r.a), nll, lens, cp_row, cpen, cov_row, cov, (int)Tp, vcov, beam, di_state, (int)di,
                           (int)max_len, (int)B, tok_out, n_alive);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// The finish of a penalised search: beam_finish_kernel's resolution of the n best, ranked under (s desc, slot asc) with
// s = pen_score(nll, lens, cpen) of the carried values.  Lane j < k owns final hypothesis j.
__global__ __launch_bounds__(64) void beam_finish_pen_kernel(const float* __restrict__ nll, const int64_t* __restrict__ beam,
                                                             const int32_t* __restrict__ lens, const float* __restrict__ cpen,
                                                             const float* __restrict__ lp_tab, const float* __restrict__ bonus,
                                                             int max_len, int steps, int B, int k, int n, int64_t* __restrict__ out,
                                                             float* __restrict__ scores, int64_t* __restrict__ slots,
                                                             float* __restrict__ logp, int32_t* __restrict__ length,
                                                             float* __restrict__ cp) {
    const int b = blockIdx.x, j = threadIdx.x;
    const int64_t* par = beam + (int64_t)max_len * B * k;
    float sc = -INFINITY, c = 0.f, pen = 0.f;
    int len = 0;
    if (j < k) {
        c = nll[(int64_t)b * k + j];
        len = lens[(int64_t)b * k + j];
        pen = cpen[(int64_t)b * k + j];
        sc = pen_score(c, len, pen, lp_tab, bonus, max_len);
    }
    int rank = 0;
    for (int i = 0; i < k; ++i) {
        const float ov = __shfl(sc, i, 64);
        rank += better(ov, i, sc, j) ? 1 : 0;
    }
    if (j < k && rank < n) {
        int64_t* row = out + ((int64_t)b * n + rank) * max_len;
        for (int t = steps; t < max_len; ++t) row[t] = 0;
        int p = j;
        for (int t = steps - 1; t >= 0; --t) {
            const int64_t o = ((int64_t)t * B + b) * k + p;
            row[t] = beam[o];
            p = (int)par[o];
        }
        row[max_len - 1] = EOS;
        const int64_t o = (int64_t)b * n + rank;
        scores[o] = sc; slots[o] = j; logp[o] = c; length[o] = len; cp[o] = pen;
    }
}

int vag_beam_finish_pen_launch(const float* nll, const int64_t* beam, const int32_t* lens, const float* cpen, const float* lp,
                               const float* bonus, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n, int64_t* out,
                               float* scores, int64_t* slots, float* logp, int32_t* length, float* cp, hipStream_t s) {
    VAG_CHECK_ARG(finish_args(nll, beam, max_len, steps, B, k, out) && scores && slots && logp && length && cp);
    VAG_CHECK_ARG(lens && cpen && lp && bonus);
    VAG_CHECK_ARG(n >= 1 && n <= k && B < (1ll << 31) && max_len < (1ll << 31));
    hipLaunchKernelGGL(beam_finish_pen_kernel, dim3((unsigned)B), dim3(64), 0, s, nll, beam, lens, cpen, lp, bonus, (int)max_len,
                       (int)steps, (int)B, (int)k, (int)n, out, scores, slots, logp, length, cp);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// ---- forced decoding: scores and attention of given translations --------------------------------------------------------
// The scored span of a target row: select.h's span_end.
// Log-probability of target word y_t under M models, read from each model's raw logits row and its log-sum-exp (x_m = logit -
// lse, the teacher-forced head's outputs; no (rows, V) log-probability matrix is written) and combined by ens_combine -- so M
// identical members give the single model's value bit for bit.  One wave per sentence b.
// token_logp (B, Tt): x at the span's non-pad positions, 0 elsewhere (NaN for a word outside [0, V)); logp (B): their sum, added
// in t order as the beam search accumulates its running score; score (B): logp / max(1, #words > 3 in the span), the
// normalisation of the finish.  Rows of logits / lse are time-major: row = t * B + b.
template <int M>
__global__ __launch_bounds__(64) void forced_score_kernel(EnsLogp<M> L, EnsRows<M> S, const int64_t* __restrict__ tgt, int B,
                                                          int Tt, int V, float* __restrict__ token_logp, float* __restrict__ logp,
                                                          float* __restrict__ score) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* y = tgt + (int64_t)b * Tt;
    const int end = span_end(y, Tt);
    float acc = 0.f;
    int words = 0;
    for (int t0 = 0; t0 < Tt; t0 += 64) {
        const int t = t0 + lane;
        const int64_t w = t < Tt ? y[t] : 0;
        const bool in = t <= end && w != 0;
        float v = 0.f;
        if (in) {
            if (w < 0 || w >= V) {
                v = NAN;
            } else {
                const int64_t row = (int64_t)t * B + b;
                float x[M];
#pragma unroll
                for (int m = 0; m < M; ++m) x[m] = L.p[m][row * L.ld[m] + w];
#pragma unroll
                for (int m = 0; m < M; ++m) x[m] -= S.p[m][row];
                v = ens_combine<M>(x);
            }
        }
        if (t < Tt) token_logp[(int64_t)b * Tt + t] = v;
        words += __popcll(__ballot(in && w > 3));
        if (t0 <= end) {
            for (int i = 0; i < 64; ++i) acc += __shfl(v, i, 64);     // in t order (positions past the span add 0)
        }
    }
    if (lane == 0) {
        logp[b] = acc;
        score[b] = acc / (float)(words < 1 ? 1 : words);
    }
}

int vag_forced_score_launch(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M,
                            const int64_t* tgt, int64_t B, int64_t Tt, int64_t V, float* token_logp, float* logp, float* score,
                            hipStream_t s) {
    EnsHost a;
    VAG_TRY(ens_logp_args(logits, ldl, M, V, a));
    VAG_CHECK_ARG(lse && tgt && token_logp && logp && score && B > 0 && Tt > 0 && V < (1ll << 31));
    VAG_CHECK_ARG(B < (1ll << 31) && Tt < (1ll << 31) && B * Tt < (1ll << 40));
    for (int m = 0; m < (int)M; ++m) VAG_CHECK_ARG(lse[m] != nullptr);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL(forced_score_kernel<MM>, dim3((unsigned)B), dim3(64), 0, s, ens_logp<MM>(a), ens_rows<MM>(lse), tgt,
                           (int)B, (int)Tt, (int)V, token_logp, logp, score);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

// Forced decoding's attention: the mean of M models' saved teacher-forced alpha (Tt, B, Ts) (the workspace slot
// vag_cgru_ws_offset(.., 0) names) inside the scored span and zeros outside it.  One workgroup per sentence (every wave scans
// the sentence: no exchange needed); rows as in the finish.
template <int M>
__global__ __launch_bounds__(256) void forced_align_kernel(EnsRows<M> A, const int64_t* __restrict__ tgt, int B, int Tt, int Ts,
                                                           bool vin, bool vout, float* __restrict__ attention,
                                                           int64_t* __restrict__ src_pos) {
    const int b = blockIdx.x;
    const int end = span_end(tgt + (int64_t)b * Tt, Tt);
    for (int t = threadIdx.x / ROW_LANES; t < Tt; t += 256 / ROW_LANES) {
        const int64_t g = (int64_t)b * Tt + t;
        attn_row<M>(A, ((int64_t)t * B + b) * Ts, t <= end, Ts, vin, vout, attention + g * Ts, src_pos + g);
    }
}

int vag_forced_align_launch(const float* const* alpha, int64_t M, const int64_t* tgt, int64_t B, int64_t Tt, int64_t Ts,
                            float* attention, int64_t* src_pos, hipStream_t s) {
    bool al;
    VAG_TRY(ens_alpha_args(alpha, M, al));
    VAG_CHECK_ARG(tgt && attention && src_pos && B > 0 && Tt > 0 && Ts > 0);
    VAG_CHECK_ARG(B < (1ll << 31) && Tt < (1ll << 31) && Ts < (1ll << 31) && B * Tt < (1ll << 40));
    const bool vin = al && (Ts & 3) == 0, vout = (Ts & 3) == 0 && aligned16(attention);
    return ens_dispatch((int)M, [&](auto m) -> int {
        constexpr int MM = decltype(m)::value;
        hipLaunchKernelGGL(forced_align_kernel<MM>, dim3((unsigned)B), dim3(256), 0, s, ens_rows<MM>(alpha), tgt, (int)B, (int)Tt,
                           (int)Ts, vin, vout, attention, src_pos);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}
