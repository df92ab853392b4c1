// kNN-MT (vag_nmt.h: vag_knn_store_rows, vag_knn_search, vag_knn_mix): a datastore of (decoder state h2 -> next word) pairs and
// its nearest neighbours mixed into the members' rows before a step's expansion or before the forced score.
//
//   store:   one 256-thread workgroup per sentence.  Its offset in the dense output is the sum of the spans (select.h: span_end) of
//            the sentences before it, recounted by every workgroup (B^2 Tt / 4 word reads in all: nothing next to the rows);
//            a wave per row rounds the row to bf16 (round to nearest even) and sums the squares of the ROUNDED values in a fixed
//            order (lane-strided fmaf chain, xor tree).  Integer sums only between workgroups; nothing is atomic.
//   search:  stage 1, one workgroup per (slice of KNN_SLICE keys, tile of rt query rows).  The tile's queries are split into three
//            bf16 planes (q = q1 + q2 + q3 up to 2^-27 |q|) once, into an LDS image in MFMA-fragment order.  A pass takes 256 keys:
//            each of the 4 waves holds two 32-key tiles as the A operand straight from global memory (16 bytes per lane and
//            k-step, the next eight k-steps in flight behind the current MFMAs, across passes too) and runs
//            v_mfma_f32_32x32x16_bf16 over the depth, three planes per k-step, into two 32 x 32 accumulators (keys on the rows, queries on the columns).  s = 2 acc - norm goes to an
//            LDS tile S[query][key of the pass]; then every wave keeps the K best of ITS eight queries in registers, one list
//            entry per lane, ranked: the first pass through select.h's wave_topk, later passes by a ballot against the K-th score
//            and one ranked insertion per survivor (a handful per pass).  The (R, N) matrix never exists.
//            A score depends on (query row, key) alone: the same planes, the same k order, the same instructions whatever the
//            slice, the pass, the wave, the tile column -- a key past N is a clamped load whose score becomes -inf, the depth past
//            D meets the planes' exact zeros -- so identical stored keys score bit-identically and the index decides (total order:
//            score descending, index ascending).
//            stage 2, one wave per row: the slices' lists (ranked, holes last) are merged by the same ranked insertion.
//   mix:     one workgroup per row, the members one after the other.  The K' neighbours' weights exp((s - s_max) / T), their sum and
//            the per-word sums are formed by serial loops in index order (reproducible); the words' own values are read BEFORE the
//            pass that rewrites the row as (x - lse) + log1p(-lam), and written after it.  Columns [V, ldl) are never touched.
#include <atomic>
#include "kernels.h"
#include "select.h"
#include "gemm_shared.h"

constexpr int KNN_SLICE = VAG_KNN_SLICE;  // keys of one stage-1 workgroup
constexpr int KNN_PASS = 256;             // keys of one pass: 4 waves x 2 tiles x 32
constexpr int KNN_S_LD = KNN_PASS + 4;    // floats per row of the score tile (the +4 spreads the float4 stores over the banks)
constexpr int KNN_GROUP = 8;              // k-steps of keys in flight ahead of the MFMAs
constexpr int KNN_HOLE = 0x7fffffff;      // index of an empty list entry (its score is -inf): worse than every real entry
constexpr int KNN_LDS_MAX = 160 * 1024;

// rows of a query tile: 32 where the three planes of 32 rows fit the LDS beside the score tile, 16 beyond (depth 656 .. 1024)
static int knn_row_tile(int64_t D) {
    const int64_t Dp = (D + 15) / 16 * 16;
    return Dp <= 640 ? 32 : 16;
}
static size_t knn_q_bytes(int64_t D, int rt) { return (size_t)3 * ((D + 15) / 16) * 2 * rt * 16; }
static size_t knn_lds_bytes(int64_t D, int rt) { return knn_q_bytes(D, rt) + (size_t)32 * KNN_S_LD * 4 + 4 * 192 * 4; }

int64_t vag_knn_row_tile_host(int64_t D) { return (D >= 8 && D <= 1024 && D % 8 == 0) ? knn_row_tile(D) : 0; }
int64_t vag_knn_scratch_bytes_host(int64_t R, int64_t N, int64_t K) {
    if (R < 1 || N < 1 || N >= (1ll << 31) || K < 1 || K > VAG_KNN_MAX_K) return 0;
    const int64_t ns = (N + KNN_SLICE - 1) / KNN_SLICE;
    return R * ns * K * 8;
}

// ---------------------------------------------------------------------------------------------------------------- store
__global__ __launch_bounds__(256) void knn_store_kernel(const float* __restrict__ h2, const int64_t* __restrict__ tgt, int B, int Tt,
                                                        int H, int sent_base, int64_t cap, unsigned* __restrict__ keys,
                                                        float* __restrict__ norm, int32_t* __restrict__ value,
                                                        int32_t* __restrict__ sentence, int32_t* __restrict__ position,
                                                        int32_t* __restrict__ count) {
    __shared__ int part[4];
    __shared__ int my_end;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sum = 0;
    for (int bb = wave; bb <= b; bb += 4) {
        const int e = span_end(tgt + (int64_t)bb * Tt, Tt);
        if (bb < b) sum += e + 1;
        else if (lane == 0) my_end = e;
    }
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    const int64_t off = (int64_t)part[0] + part[1] + part[2] + part[3];
    const int len = my_end + 1;
    if (b == B - 1 && threadIdx.x == 0) *count = (int32_t)(off + len);
    for (int t = wave; t < len; t += 4) {
        const int64_t dst = off + t;
        if (dst >= cap) break;
        const float* __restrict__ src = h2 + ((int64_t)t * B + b) * H;
        float acc = 0.f;
        for (int c = lane * 2; c < H; c += 128) {
            const unsigned u = pack_bf16(src[c], src[c + 1]);
            keys[(dst * H + c) >> 1] = u;
            const float k0 = __builtin_bit_cast(float, u << 16), k1 = __builtin_bit_cast(float, u & 0xffff0000u);
            acc = __fmaf_rn(k0, k0, acc);
            acc = __fmaf_rn(k1, k1, acc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o, 64));
        if (lane == 0) {
            norm[dst] = acc;
            value[dst] = (int32_t)tgt[(int64_t)b * Tt + t];
            sentence[dst] = sent_base + b;
            position[dst] = t;
        }
    }
}

int vag_knn_store_rows_launch(const float* h2, const int64_t* tgt, int64_t B, int64_t Tt, int64_t H, int64_t sent_base, int64_t cap,
                              void* keys, float* norm, int32_t* value, int32_t* sentence, int32_t* position, int32_t* count,
                              hipStream_t s) {
    VAG_CHECK_ARG(h2 && tgt && keys && norm && value && sentence && position && count);
    VAG_CHECK_ARG(B >= 1 && B < 65536 && Tt >= 1 && Tt < (1ll << 24) && H >= 8 && H <= 1024 && H % 8 == 0);
    VAG_CHECK_ARG(sent_base >= 0 && sent_base + B < (1ll << 31) && cap >= 0 && B * Tt < (1ll << 31));
    hipLaunchKernelGGL(knn_store_kernel, dim3((unsigned)B), dim3(256), 0, s, h2, tgt, (int)B, (int)Tt, (int)H, (int)sent_base, cap,
                       reinterpret_cast<unsigned*>(keys), norm, value, sentence, position, count);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// --------------------------------------------------------------------------------------------------------------- search
// One ranked insertion into a wave's list (entry `lane` in (lv, li), best first): the candidate takes the place of the first entry it
// beats, the entries behind it move down one lane, the last one falls off.
__device__ __forceinline__ void knn_insert(float& lv, int& li, float cv, int ci, int lane) {
    const int rank = __popcll(__ballot(better(lv, li, cv, ci)));
    const float uv = __shfl_up(lv, 1, 64);
    const int ui = __shfl_up(li, 1, 64);
    if (lane > rank) { lv = uv; li = ui; }
    else if (lane == rank) { lv = cv; li = ci; }
}

// the A fragments (two key tiles) of up to KNN_GROUP k-steps from ks0 on.  Rows are clamped to N - 1 and columns past D to 0, so
// every load is in bounds and NOTHING is done to the loaded values (a select on them would make the wave wait for the loads where
// they are issued and undo the prefetch): a row past N computes a score that is replaced by -inf, and the depth past D meets the
// query planes' exact zeros there (finite x 0 = 0).
struct KnnFrag { bf16x8 a[KNN_GROUP][2]; };
__device__ __forceinline__ void knn_load_group(KnnFrag& f, const __bf16* __restrict__ keys, const int64_t (&rowoff)[2], int ks0, int D,
                                               int h) {
#pragma unroll
    for (int j = 0; j < KNN_GROUP; ++j) {
        const int col = 16 * (ks0 + j) + 8 * h;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 v = *reinterpret_cast<const uint4*>(keys + rowoff[t] + (col < D ? col : 0));
            const u32x4 q = {v.x, v.y, v.z, v.w};
            f.a[j][t] = __builtin_bit_cast(bf16x8, q);
        }
    }
}
__device__ __forceinline__ void knn_mfma_group(const KnnFrag& f, f32x16 (&acc)[2], const char* qfrag, int ks0, int KS, int plane_stride,
                                               int ks_stride) {
#pragma unroll
    for (int j = 0; j < KNN_GROUP; ++j) {
        if (ks0 + j < KS) {
            const char* qp = qfrag + (size_t)(ks0 + j) * ks_stride;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const bf16x8 bq = sp_frag(reinterpret_cast<const __bf16*>(qp + (size_t)p * plane_stride));
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[j][0], bq, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[j][1], bq, acc[1], 0, 0, 0);
            }
        }
    }
}

__global__ __launch_bounds__(256) void knn_search_kernel(const float* __restrict__ q, int64_t ldq, int R, int D,
                                                         const __bf16* __restrict__ keys, const float* __restrict__ norm, int N, int K,
                                                         int rt, int ntiles, int nslices, float* __restrict__ part_v,
                                                         int* __restrict__ part_i) {
    extern __shared__ __attribute__((aligned(16))) char knn_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int KS = (D + 15) / 16;
    const int ks_stride = 2 * rt * 16, plane_stride = KS * ks_stride;          // bytes
    float* S = reinterpret_cast<float*>(knn_smem + 3 * (size_t)plane_stride);
    float* tk = S + 32 * KNN_S_LD + wave * 192;                                // wave_topk's scratch: sv[64] si[64] ov[32] oi[32]
    // the row tiles of one slice are neighbours in the grid, so they run at about the same time.  (Measured: placing them on one
    // XCD as well, by blockIdx.x % 8, changed nothing -- 845 against 850 us at N = 400 000 -- and was not kept.)
    const int slice = blockIdx.x / ntiles;
    const int row0 = (blockIdx.x - slice * ntiles) * rt;
    const int s0 = slice * KNN_SLICE;
    const int send = min(N, s0 + KNN_SLICE);

    // the tile's queries as three bf16 planes, image [plane][k-step][half][row][8]: a (plane, k-step) is lane-linear for the reads
    for (int i = threadIdx.x; i < rt * KS * 2; i += 256) {
        const int r = i % rt, ch = i / rt;                                     // ch: chunk of 8 depth values
        const int64_t row = row0 + r;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = 8 * ch + j;
            x[j] = (row < R && d < D) ? q[row * ldq + d] : 0.f;
        }
        unsigned p1[4], p2[4], p3[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split3(x[2 * j], x[2 * j + 1], p1[j], p2[j], p3[j]);
        char* dst = knn_smem + (size_t)(ch >> 1) * ks_stride + ((ch & 1) * rt + r) * 16;
        *reinterpret_cast<uint4*>(dst) = make_uint4(p1[0], p1[1], p1[2], p1[3]);
        *reinterpret_cast<uint4*>(dst + plane_stride) = make_uint4(p2[0], p2[1], p2[2], p2[3]);
        *reinterpret_cast<uint4*>(dst + 2 * (size_t)plane_stride) = make_uint4(p3[0], p3[1], p3[2], p3[3]);
    }
    __syncthreads();
    // (a 16-row tile: columns 16 .. 31 of the MFMA repeat rows 0 .. 15; their scores are never looked at)
    const char* qfrag = knn_smem + (h * rt + (c & (rt - 1))) * 16;

    float lv[8];
    int li[8];
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) { lv[qq] = -INFINITY; li[qq] = KNN_HOLE; }

    KnnFrag fa, fb;
    {
        const int64_t first[2] = {(int64_t)min(s0 + wave * 64 + c, N - 1) * D, (int64_t)min(s0 + wave * 64 + 32 + c, N - 1) * D};
        knn_load_group(fa, keys, first, 0, D, h);
    }
    for (int p0 = s0; p0 < send; p0 += KNN_PASS) {
        // (fa holds this pass's first group: loaded before the loop, or by the previous pass behind its last MFMAs)
        int64_t rowoff[2], rownext[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            rowoff[t] = (int64_t)min(p0 + wave * 64 + t * 32 + c, N - 1) * D;
            rownext[t] = (int64_t)min(p0 + KNN_PASS + wave * 64 + t * 32 + c, N - 1) * D;
        }
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        // the pass's norms, issued ahead of the MFMAs that hide them (clamped: past N the score becomes -inf anyway)
        float nr[2][16];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                nr[t][r] = norm[min(p0 + wave * 64 + t * 32 + 8 * (r >> 2) + 4 * h + (r & 3), N - 1)];
        // Every load below is unconditional (a group past the depth re-reads column 0 and is never multiplied): with a branch
        // around a load the compiler cannot count the loads in flight and waits for all of them before every MFMA group.
        for (int ks0 = 0; ks0 < KS; ks0 += 2 * KNN_GROUP) {
            knn_load_group(fb, keys, rowoff, ks0 + KNN_GROUP, D, h);
            knn_mfma_group(fa, acc, qfrag, ks0, KS, plane_stride, ks_stride);
            const bool more = ks0 + 2 * KNN_GROUP < KS;                        // else: the next pass's first group, behind fb's MFMAs
            const int64_t ro[2] = {more ? rowoff[0] : rownext[0], more ? rowoff[1] : rownext[1]};
            knn_load_group(fa, keys, ro, more ? ks0 + 2 * KNN_GROUP : 0, D, h);
            knn_mfma_group(fb, acc, qfrag, ks0 + KNN_GROUP, KS, plane_stride, ks_stride);
        }
        // s = 2 acc - norm (2 acc is exact: one rounding), -inf past the last key; S[query c][key of the pass]
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int kl = wave * 64 + t * 32 + 8 * g + 4 * h;
                float4 o;
                float* op = reinterpret_cast<float*>(&o);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kidx = p0 + kl + r;
                    op[r] = kidx < N ? __fmaf_rn(2.f, acc[t][4 * g + r], -nr[t][4 * g + r]) : -INFINITY;
                }
                *reinterpret_cast<float4*>(S + c * KNN_S_LD + kl) = o;
            }
        __syncthreads();
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) {
            const int qc = wave * 8 + qq;
            if (qc >= rt || row0 + qc >= R) continue;                          // (uniform over the wave)
            float sv[4];
            int si[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sv[j] = S[qc * KNN_S_LD + lane + 64 * j];
                si[j] = p0 + lane + 64 * j < N ? lane + 64 * j : KNN_HOLE;
            }
            if (p0 == s0) {
                float* tv = tk;
                int* ti = reinterpret_cast<int*>(tk + 64);
                float* ov = tk + 128;
                int* oi = reinterpret_cast<int*>(tk + 160);
                const int n = wave_topk<4>(sv, si, K, tv, ti, ov, oi);
                wave_lds_fence();
                lv[qq] = lane < n ? ov[lane] : -INFINITY;
                li[qq] = lane < n ? p0 + oi[lane] : KNN_HOLE;
                wave_lds_fence();
            } else {
                // later keys have larger indices: only a strictly larger score than the K-th can enter
                const float thr = __shfl(lv[qq], K - 1, 64);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned long long m = __ballot(sv[j] > thr);
                    while (m) {
                        const int bl = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        knn_insert(lv[qq], li[qq], __shfl(sv[j], bl, 64), p0 + 64 * j + bl, lane);
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
        const int qc = wave * 8 + qq;
        if (qc >= rt || row0 + qc >= R) continue;
        if (lane < K) {
            const int64_t o = (((int64_t)(row0 + qc)) * nslices + slice) * K + lane;
            part_v[o] = lv[qq];
            part_i[o] = li[qq];
        }
    }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int R, int K,
                                                        int nslices, float* __restrict__ out_v, int* __restrict__ out_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= R) return;
    const int64_t total = (int64_t)nslices * K;
    const float* pv = part_v + row * total;
    const int* pi = part_i + row * total;
    float lv = -INFINITY;
    int li = KNN_HOLE;
    for (int64_t c0 = 0; c0 < total; c0 += 64) {
        const bool in = c0 + lane < total;
        const float cv = in ? pv[c0 + lane] : -INFINITY;
        const int ci = in ? pi[c0 + lane] : KNN_HOLE;
        const float tv = __shfl(lv, K - 1, 64);
        const int ti = __shfl(li, K - 1, 64);
        unsigned long long m = __ballot(ci != KNN_HOLE && better(cv, ci, tv, ti));
        while (m) {
            const int bl = __ffsll((long long)m) - 1;
            m &= m - 1;
            knn_insert(lv, li, __shfl(cv, bl, 64), __shfl(ci, bl, 64), lane);
        }
    }
    if (lane < K) {
        out_v[row * K + lane] = lv;
        out_i[row * K + lane] = li == KNN_HOLE ? -1 : li;
    }
}

static bool knn_lds_attr() {            // dynamic LDS above 64 KB: the attribute once per device
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done.load(std::memory_order_acquire) & (1ull << dev)) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            KNN_LDS_MAX) != hipSuccess)
        return false;
    done.fetch_or(1ull << dev, std::memory_order_release);
    return true;
}

int vag_knn_search_launch(const float* q, int64_t ldq, int64_t R, int64_t D, const void* keys, const float* norm, int64_t N, int64_t K,
                          float* out_score, int32_t* out_index, void* scratch, hipStream_t s) {
    VAG_CHECK_ARG(q && keys && norm && out_score && out_index && scratch);
    VAG_CHECK_ARG(D >= 8 && D <= 1024 && D % 8 == 0 && ldq >= D && N >= 1 && N < (1ll << 31) && K >= 1 && K <= VAG_KNN_MAX_K);
    VAG_CHECK_ARG(aligned16(keys) && aligned16(scratch));
    const int rt = knn_row_tile(D);
    const int64_t tiles = (R + rt - 1) / rt, ns = (N + KNN_SLICE - 1) / KNN_SLICE;
    VAG_CHECK_ARG(R >= 1 && R * ns < (1ll << 31) / VAG_KNN_MAX_K);                // (so ns * tiles < 2^26: a one-dimensional grid)
    const size_t lds = knn_lds_bytes(D, rt);
    VAG_CHECK_ARG(lds <= (size_t)KNN_LDS_MAX);
    if (!knn_lds_attr()) return VAG_EINVAL;
    float* part_v = reinterpret_cast<float*>(scratch);
    int* part_i = reinterpret_cast<int*>(part_v + R * ns * K);
    hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)(ns * tiles)), dim3(256), lds, s, q, ldq, (int)R, (int)D,
                       reinterpret_cast<const __bf16*>(keys), norm, (int)N, (int)K, rt, (int)tiles, (int)ns, part_v, part_i);
    VAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, part_v, part_i, (int)R, (int)K, (int)ns,
                       out_score, out_index);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// ------------------------------------------------------------------------------------------------------------------ mix
template <int M> struct KnnMix {
    float* p[M]; int64_t ld[M];
    const float* nv[M]; const int32_t* ni[M]; const int32_t* val[M]; int64_t nval[M]; const float* lse[M];
};

template <int M>
__global__ __launch_bounds__(256) void knn_mix_kernel(KnnMix<M> a, int V, int K, float inv_T, float log_lam, float log1m) {
    __shared__ float w[VAG_KNN_MAX_K];
    __shared__ int word[VAG_KNN_MAX_K];
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        float* __restrict__ row = a.p[m] + n * a.ld[m];
        const float l = a.lse[m] ? a.lse[m][n] : 0.f;
        if (tid < 64) {
            bool ok = false;
            int wd = -1;
            float s = -INFINITY;
            if (tid < K) {
                const int idx = a.ni[m][n * K + tid];
                if (idx >= 0 && idx < a.nval[m]) {
                    wd = a.val[m][idx];
                    ok = wd >= 0 && wd < V;
                    s = a.nv[m][n * K + tid];
                }
            }
            float smax = ok ? s : -INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) smax = fmaxf(smax, __shfl_xor(smax, o, 64));
            if (tid < K) {
                w[tid] = ok ? expf(__fmul_rn(__fsub_rn(s, smax), inv_T)) : 0.f;
                word[tid] = ok ? wd : -1;
            }
        }
        __syncthreads();
        bool lead = false;
        int wd = -1;
        float out = 0.f;
        if (tid < K && word[tid] >= 0) {
            wd = word[tid];
            float Z = 0.f, agg = 0.f;
            lead = true;
            for (int i = 0; i < K; ++i) {                                      // index order: reproducible
                Z = __fadd_rn(Z, w[i]);
                if (word[i] == wd) {
                    agg = __fadd_rn(agg, w[i]);
                    if (i < tid) lead = false;
                }
            }
            const float x = __fadd_rn(__fsub_rn(row[wd], l), log1m);           // log((1 - lam) p_model)
            const float y = __fadd_rn(log_lam, logf(agg / Z));                 // log(lam p_knn)
            const float hi = fmaxf(x, y), lo = fminf(x, y);
            out = __fadd_rn(hi, log1pf(expf(__fsub_rn(lo, hi))));
        }
        __syncthreads();                                                       // the words' own values are read: rewrite the row
        for (int v = tid; v < V; v += 256) row[v] = __fadd_rn(__fsub_rn(row[v], l), log1m);
        __syncthreads();
        if (lead) row[wd] = out;
        __syncthreads();
    }
}

int vag_knn_mix_launch(float* const* logp, const int64_t* ldl, int64_t M, int64_t R, int64_t V, const float* const* nb_score,
                       const int32_t* const* nb_index, int64_t K, const int32_t* const* values, const int64_t* n_values,
                       const float* const* lse, float inv_T, float log_lam, float log1m_lam, hipStream_t s) {
    VAG_CHECK_ARG(logp && ldl && nb_score && nb_index && values && n_values && M >= 1 && M <= VAG_ENS_MAX);
    VAG_CHECK_ARG(R >= 1 && R < (1ll << 31) && V >= 1 && V < (1ll << 31) && K >= 1 && K <= VAG_KNN_MAX_K);
    VAG_CHECK_ARG(inv_T > 0.f && inv_T < INFINITY && log_lam < 0.f && log_lam > -INFINITY && log1m_lam <= 0.f && log1m_lam > -INFINITY);
    for (int m = 0; m < (int)M; ++m)
        VAG_CHECK_ARG(logp[m] && ldl[m] >= V && nb_score[m] && nb_index[m] && values[m] && n_values[m] >= 1 && n_values[m] < (1ll << 31));
    return ens_dispatch((int)M, [&](auto mm) -> int {
        constexpr int MM = decltype(mm)::value;
        KnnMix<MM> a;
        for (int m = 0; m < MM; ++m) {
            a.p[m] = logp[m]; a.ld[m] = ldl[m]; a.nv[m] = nb_score[m]; a.ni[m] = nb_index[m]; a.val[m] = values[m];
            a.nval[m] = n_values[m]; a.lse[m] = lse ? lse[m] : nullptr;
        }
        hipLaunchKernelGGL(knn_mix_kernel<MM>, dim3((unsigned)R), dim3(256), 0, s, a, (int)V, (int)K, inv_T, log_lam, log1m_lam);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    });
}
