// Shallow fusion with a back-off n-gram language model (vag_nmt.h: vag_lm_fuse_rows, vag_lm_fuse_beam(_dev), vag_lm_query).
// The model is a forward trie in flat arrays (vag_lm); ARPA semantics: lm(w | c_L..c_1) is logp(c_L..c_1 w) where that n-gram is
// stored, otherwise bo(c_L..c_1) -- 0 for a context that is not stored -- plus lm(w | c_{L-1}..c_1), down to the unigrams.
//   dense form: one 256-thread workgroup per hypothesis row evaluates the model over the whole vocabulary.
//     contexts: lane j-1 resolves the suffix of j words (j = 1 .. order-1) to its trie node by binary searches from the unigram of
//               the suffix's oldest word and leaves (exists, node, bo) in LDS.  Bsum[j] is the sum of the back-offs of the existing
//               contexts longer than j, formed from the longest down.
//     claimed:  from the longest existing context down to one word the threads stride over the node's successors; a successor w
//               that no longer context has claimed is written as x + beta (logp + Bsum[j]) and claimed in an LDS bitmap.  The
//               successors of one node are distinct, so inside one order nobody else wants w; the claim is an integer atomicOr
//               only because neighbours share a bitmap word.  A barrier separates the orders.
//     dense:    one pass over [0, V) adds beta (uni[w] + Bsum[0]) to every unclaimed word: float4 where the row allows and the
//               four words are all unclaimed, element by element otherwise.
//   Every element of [0, V) is read once and written once, whatever the thread timing; columns [V, ld) are never touched.
//   The beam form reads the context from the search buffer: at most order-1 hops back from step di-1, a hop's word and parent
//   issued together; SOS follows the word of step 0, nothing follows SOS.  A row whose previous word is EOS is left as it is.
//   No loop runs longer than `order` or an array's length; nothing waits on another workgroup; no float atomics.
// The arithmetic is spelled with __fadd_rn / __fmul_rn (no contraction): tests/lm_ref.py restates it operation for operation.
#include "kernels.h"
#include "select.h"

constexpr int LM_CTX = VAG_LM_MAX_ORDER - 1;         // longest context
constexpr int LM_BITMAP_WORDS = VAG_LM_MAX_V / 32;   // claimed-word bitmap: 16 KB of LDS
constexpr int64_t LM_SOS = 2;
constexpr int64_t LM_EOS = 3;

template <int M> struct LmRows { float* p[M]; int64_t ld[M]; };

// index of w in word[lo, hi) (ascending, distinct), or -1.  At most 32 halvings.
__device__ __forceinline__ int lm_find(const int32_t* __restrict__ word, int lo, int hi, int w) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int x = word[mid];
        if (x == w) return mid;
        if (x < w) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// number of usable context words: the leading ones (most recent first) that are words of the vocabulary
__device__ __forceinline__ int lm_ctx_len(const int (&c)[LM_CTX], int order, int V) {
    int len = 0;
    bool open = true;
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) {
        open = open && i < order - 1 && c[i] >= 0 && c[i] < V;
        if (open) len = i + 1;
    }
    return len;
}

// The trie node of the context's suffix of j words c[j-1] .. c[0] (c[0] the most recent), 1 <= j <= len: its index in level j
// (level 1 = unigrams), or -1 where it is not stored.  bo receives its back-off weight (0 where it is not stored).
__device__ __forceinline__ int lm_resolve(const vag_lm& lm, const int (&c)[LM_CTX], int j, float& bo) {
    int first = 0;
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i)
        if (i == j - 1) first = c[i];
    int node = first;                                  // level 1 is indexed by the word
#pragma unroll
    for (int d = 1; d < LM_CTX; ++d) {                 // step d: from level d to level d+1 by the word c[j-1-d]
        if (d < j && node >= 0) {
            int w = 0;
#pragma unroll
            for (int i = 0; i < LM_CTX; ++i)
                if (i == j - 1 - d) w = c[i];
            const int cnt = (int)lm.count[d];
            const int lo = max(lm.child[d - 1][node], 0);
            const int hi = min(lm.child[d - 1][node + 1], cnt);
            node = lm_find(lm.word[d], lo, hi, w);
        }
    }
    bo = 0.f;
#pragma unroll
    for (int l = 0; l < LM_CTX; ++l)
        if (l == j - 1 && node >= 0) bo = lm.bo[l][node];
    return node;
}

// rows[m][n * ld[m] + w] += beta * lm(w | c) for every w < V: the body of both dense forms.  c: most recent word first, -1 = none.
template <int M>
__device__ __forceinline__ void lm_fuse_row(const LmRows<M>& L, int64_t n, const vag_lm& lm, const int (&c)[LM_CTX], float beta) {
    __shared__ unsigned bm[LM_BITMAP_WORDS + 1];
    __shared__ int s_node[LM_CTX];
    __shared__ float s_bo[LM_CTX];
    const int tid = threadIdx.x;
    const int V = lm.V;
    const int len = lm_ctx_len(c, lm.order, V);
    for (int i = tid; i < ((V + 31) >> 5) + 1; i += 256) bm[i] = 0u;
    if (tid < LM_CTX) {
        float bo = 0.f;
        int node = -1;
        if (tid < len) node = lm_resolve(lm, c, tid + 1, bo);
        s_node[tid] = node;
        s_bo[tid] = bo;
    }
    __syncthreads();
    // bsum[j]: the back-offs of the existing contexts longer than j words, summed from the longest down
    float bsum[LM_CTX + 1];
    float acc = 0.f;
#pragma unroll
    for (int j = LM_CTX; j >= 1; --j) {
        bsum[j] = acc;
        if (s_node[j - 1] >= 0) acc = __fadd_rn(acc, s_bo[j - 1]);
    }
    bsum[0] = acc;
    // claimed first: the successors of the context of j words are the (j+1)-grams; level j+1 has index j
#pragma unroll
    for (int j = LM_CTX; j >= 1; --j) {
        const int node = s_node[j - 1];
        if (node >= 0) {
            const int cnt = (int)lm.count[j];
            const int lo = max(lm.child[j - 1][node], 0);
            const int hi = min(lm.child[j - 1][node + 1], cnt);
            const int32_t* __restrict__ word = lm.word[j];
            const float* __restrict__ lp = lm.logp[j];
            for (int i = lo + tid; i < hi; i += 256) {
                const int w = word[i];
                if (w < 0 || w >= V) continue;
                const unsigned bit = 1u << (w & 31);
                const unsigned old = atomicOr(&bm[w >> 5], bit);
                if (old & bit) continue;               // a longer context has it
                const float t = __fmul_rn(beta, __fadd_rn(lp[i], bsum[j]));
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float* q = L.p[m] + n * L.ld[m] + w;
                    *q = __fadd_rn(*q, t);
                }
            }
        }
        __syncthreads();
    }
    // the rest of the vocabulary: unigrams under the whole back-off sum
    const float* __restrict__ uni = lm.logp[0];
    const float b0 = bsum[0];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        float* __restrict__ row = L.p[m] + n * L.ld[m];
        const int head = min((int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2), V);
        const int nvec = (V - head) >> 2;
        const bool uni_vec = (((uintptr_t)(uni + head)) & 15u) == 0;
        for (int w = tid; w < head; w += 256)
            if (!((bm[w >> 5] >> (w & 31)) & 1u)) row[w] = __fadd_rn(row[w], __fmul_rn(beta, __fadd_rn(uni[w], b0)));
        for (int i = tid; i < nvec; i += 256) {
            const int w = head + 4 * i;
            const unsigned long long two = ((unsigned long long)bm[(w >> 5) + 1] << 32) | bm[w >> 5];
            const unsigned four = (unsigned)(two >> (w & 31)) & 15u;
            if (four == 0u) {
                float4 x = *reinterpret_cast<const float4*>(row + w);
                float4 u;
                if (uni_vec) u = *reinterpret_cast<const float4*>(uni + w);
                else u = make_float4(uni[w], uni[w + 1], uni[w + 2], uni[w + 3]);
                x.x = __fadd_rn(x.x, __fmul_rn(beta, __fadd_rn(u.x, b0)));
                x.y = __fadd_rn(x.y, __fmul_rn(beta, __fadd_rn(u.y, b0)));
                x.z = __fadd_rn(x.z, __fmul_rn(beta, __fadd_rn(u.z, b0)));
                x.w = __fadd_rn(x.w, __fmul_rn(beta, __fadd_rn(u.w, b0)));
                *reinterpret_cast<float4*>(row + w) = x;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (!((four >> e) & 1u)) row[w + e] = __fadd_rn(row[w + e], __fmul_rn(beta, __fadd_rn(uni[w + e], b0)));
            }
        }
        for (int w = head + 4 * nvec + tid; w < V; w += 256)
            if (!((bm[w >> 5] >> (w & 31)) & 1u)) row[w] = __fadd_rn(row[w], __fmul_rn(beta, __fadd_rn(uni[w], b0)));
    }
}

template <int M>
__global__ __launch_bounds__(256) void lm_fuse_rows_kernel(LmRows<M> L, vag_lm lm, const int32_t* __restrict__ ctx, float beta) {
    const int64_t n = blockIdx.x;
    const int nc = lm.order - 1;
    int c[LM_CTX];
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) c[i] = i < nc ? ctx[n * nc + (nc - 1 - i)] : -1;       // (the most recent word is last)
    lm_fuse_row<M>(L, n, lm, c, beta);
}

template <int M>
__global__ __launch_bounds__(256) void lm_fuse_beam_kernel(LmRows<M> L, vag_lm lm, const int64_t* __restrict__ beam,
                                                           const int32_t* di_state, int di_host, int max_len, int B, int k,
                                                           float beta) {
    __shared__ int s_c[LM_CTX];
    // the step index the expansion that follows will read (it advances it; this launch only reads)
    const int di = di_state ? __atomic_load_n(di_state, __ATOMIC_RELAXED) : di_host;
    if (di < 0 || di >= max_len) return;
    const int k_in = di == 0 ? 1 : k;
    const int64_t n = blockIdx.x;                                  // hypothesis row b * k_in + j
    if (n >= (int64_t)B * k_in) return;                            // (a device-side step 0: the grid is sized for B k rows)
    const int b = (int)(n / k_in);
    if (threadIdx.x == 0) {
        int s = (int)(n - (int64_t)b * k_in);
        int t = di - 1;
#pragma unroll
        for (int i = 0; i < LM_CTX; ++i) {
            int w = -1;
            if (i < lm.order - 1) {
                if (t >= 0) {
                    const int64_t o = ((int64_t)t * B + b) * k + s;
                    const int64_t ww = beam[o];
                    const int64_t p = beam[o + (int64_t)max_len * B * k];
                    w = (ww >= 0 && ww < lm.V) ? (int)ww : -1;
                    s = min(max((int)p, 0), k - 1);                // (a back-pointer is a slot; never index outside the row)
                } else if (t == -1) {
                    w = (int)LM_SOS;
                }
                --t;
            }
            s_c[i] = w;
        }
    }
    __syncthreads();
    int c[LM_CTX];
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) c[i] = s_c[i];
    if (di >= 1 && c[0] == (int)LM_EOS) return;                    // finished: the expansion's own rule covers the row
    lm_fuse_row<M>(L, n, lm, c, beta);
}

// the sparse form: one lane per (context, word) pair
__global__ __launch_bounds__(256) void lm_query_kernel(vag_lm lm, const int32_t* __restrict__ ctx, const int32_t* __restrict__ word,
                                                       int R, float* __restrict__ logp_out, int32_t* __restrict__ order_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int nc = lm.order - 1;
    const int V = lm.V;
    int c[LM_CTX];
#pragma unroll
    for (int i = 0; i < LM_CTX; ++i) c[i] = i < nc ? ctx[(int64_t)r * nc + (nc - 1 - i)] : -1;
    const int w = word[r];
    if (w < 0 || w >= V) {                                         // no word of the vocabulary: order 0
        logp_out[r] = -INFINITY;
        order_out[r] = 0;
        return;
    }
    const int len = lm_ctx_len(c, lm.order, V);
    int node[LM_CTX];
    float bo[LM_CTX];
#pragma unroll
    for (int j = 1; j <= LM_CTX; ++j) {
        node[j - 1] = -1;
        bo[j - 1] = 0.f;
        if (j <= len) node[j - 1] = lm_resolve(lm, c, j, bo[j - 1]);
    }
    float acc = 0.f;                                               // the back-offs of the existing longer contexts, longest first
    float val = 0.f;
    int matched = 0;
#pragma unroll
    for (int j = LM_CTX; j >= 1; --j) {
        if (matched == 0 && node[j - 1] >= 0) {
            const int cnt = (int)lm.count[j];
            const int lo = max(lm.child[j - 1][node[j - 1]], 0);
            const int hi = min(lm.child[j - 1][node[j - 1] + 1], cnt);
            const int i = lm_find(lm.word[j], lo, hi, w);
            if (i >= 0) {
                val = __fadd_rn(lm.logp[j][i], acc);
                matched = j + 1;
            } else {
                acc = __fadd_rn(acc, bo[j - 1]);
            }
        }
    }
    if (matched == 0) {
        val = __fadd_rn(lm.logp[0][w], acc);
        matched = 1;
    }
    logp_out[r] = val;
    order_out[r] = matched;
}

// the model as the kernels may trust it: every level the order uses has its arrays
static int lm_check(const vag_lm* lm) {
    VAG_CHECK_ARG(lm != nullptr);
    VAG_CHECK_ARG(lm->order >= 2 && lm->order <= VAG_LM_MAX_ORDER);
    VAG_CHECK_ARG(lm->V >= 1 && lm->V <= VAG_LM_MAX_V && lm->count[0] == lm->V);
    for (int l = 0; l < lm->order; ++l) {
        VAG_CHECK_ARG(lm->count[l] >= 0 && lm->count[l] < (1ll << 31) && lm->logp[l]);
        if (l >= 1) VAG_CHECK_ARG(lm->word[l]);
        if (l < lm->order - 1) VAG_CHECK_ARG(lm->bo[l] && lm->child[l]);
    }
    return VAG_OK;
}

template <int MM>
static LmRows<MM> lm_rows(float* const* rows, const int64_t* ld) {
    LmRows<MM> L;
    for (int m = 0; m < MM; ++m) { L.p[m] = rows[m]; L.ld[m] = ld[m]; }
    return L;
}

int vag_lm_fuse_rows_launch(float* const* rows, const int64_t* ld, int64_t M, int64_t R, int64_t V, const vag_lm* lm,
                            const int32_t* ctx, float beta, hipStream_t s) {
    VAG_CHECK_ARG(rows && ld && M >= 1 && M <= VAG_ENS_MAX);
    VAG_TRY(lm_check(lm));
    VAG_CHECK_ARG(V == lm->V && R >= 1 && R < (1ll << 31) && ctx && std::isfinite(beta));
    for (int m = 0; m < (int)M; ++m) VAG_CHECK_ARG(rows[m] && ld[m] >= V);
    if (beta == 0.f) return VAG_OK;                               // nothing to add: no launch
    return ens_dispatch((int)M, [&](auto mm) -> int {
        constexpr int MM = decltype(mm)::value;
        hipLaunchKernelGGL(lm_fuse_rows_kernel<MM>, dim3((unsigned)R), dim3(256), 0, s, lm_rows<MM>(rows, ld), *lm, ctx, beta);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

int vag_lm_fuse_beam_launch(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di,
                            const int32_t* di_state, bool dev_form, int64_t max_len, int64_t B, int64_t k, int64_t V,
                            const vag_lm* lm, float beta, hipStream_t s) {
    VAG_CHECK_ARG(logp && ldl && M >= 1 && M <= VAG_ENS_MAX);
    VAG_TRY(lm_check(lm));
    VAG_CHECK_ARG(V == lm->V && B > 0 && k > 0 && k <= 64 && max_len > 0 && max_len <= 1024 && B * k < (1ll << 31));
    for (int m = 0; m < (int)M; ++m) VAG_CHECK_ARG(logp[m] && ldl[m] >= V);
    VAG_CHECK_ARG(beam != nullptr && std::isfinite(beta));
    if (dev_form) VAG_CHECK_ARG(di_state != nullptr);
    else VAG_CHECK_ARG(di >= 0 && di < max_len);
    if (beta == 0.f) return VAG_OK;
    const int64_t rows = (!dev_form && di == 0) ? B : B * k;
    return ens_dispatch((int)M, [&](auto mm) -> int {
        constexpr int MM = decltype(mm)::value;
        hipLaunchKernelGGL(lm_fuse_beam_kernel<MM>, dim3((unsigned)rows), dim3(256), 0, s, lm_rows<MM>(logp, ldl), *lm, beam,
                           dev_form ? di_state : nullptr, (int)di, (int)max_len, (int)B, (int)k, beta);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}

int vag_lm_query_launch(const vag_lm* lm, const int32_t* ctx, const int32_t* word, int64_t R, float* logp_out, int32_t* order_out,
                        hipStream_t s) {
    VAG_TRY(lm_check(lm));
    VAG_CHECK_ARG(ctx && word && logp_out && order_out && R >= 1 && R < (1ll << 31));
    hipLaunchKernelGGL(lm_query_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, *lm, ctx, word, (int)R, logp_out,
                       order_out);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
