// Products with few rows (one recurrence time step, a beam's hypotheses, an attention side) for gfx950: operands go straight
// from L2 into MFMA fragment layout, no LDS staging, K split across the waves of a workgroup, LDS only for the cross-wave sum.
//
//  * skinny_plain / skinny_plain_mn : out = A W^T with bias / addend / tanh epilogues (vag_skinny_launch and its gather, NN and
//                                     batched forms), skinny3 (three products summed in one launch), skinny_bt (out = A B, k outer)
//  * attn_dot_side*                 : the attention side products of the decoder backward
//  * gru_step* / gru_bwd_step       : the hidden-side product fused with the GRU cell, forward and backward
//  * skinny_tall                    : M <= 256 rows against a vocabulary-sized W (logits of a decode step)
//
// The LDS-tiled products, their planner and queues are gemm.hip; the declarations of every launcher here are in common.h.
#include "gemm_shared.h"
#include "call_ctx.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
int vag_copy2d_launch(const float* in, int64_t ldi, float* out, int64_t ldo, int64_t rows, int64_t cols, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// skinny GEMM  out[m,n] = sum_k A[m,k] W[n,k]   (both k-contiguous), fused epilogues
//
// These launches are bound by bytes fetched per CU (each CU pulls ~33 GB/s out of the Infinity Cache; L2 is dropped
// at every kernel boundary), so the workgroup tile is chosen to (a) put one workgroup on every one of the 256 CUs
// and (b) minimise (A rows + W rows) * K per workgroup: see pick_plain_tile().
// ------------------------------------------------------------------------------------------------
struct SkinnyArgs {
    const float* A; const float* W; int64_t lda, ldw;
    int M, N, K;
    const float* bias; const float* addend; int64_t ldadd; float* out; int64_t ldo; int act;
    int64_t bsA = 0, bsW = 0, bsO = 0;     // batched launches (blockIdx.z): element strides of A, W and out/addend
    // A rows taken through an index (A = embedding table, row m = A[row_idx[m]]); the column-tile-0 workgroups also write
    // the gathered rows out (the embedded inputs are needed again by the head and by the backward pass)
    const int64_t* row_idx = nullptr; float* gather_out = nullptr; int64_t ld_gather = 0;
    float a_scale = 1.f;                   // fp16-weight products only: power of two applied to A before its fp16 rounding (gradients)
    float* out2 = nullptr; int64_t ldo2 = 0; float scale2 = 0.f; int acc2 = 0;      // skinny_bt_kernel: out2 (+)= scale2 * result as well
};

// Load pattern.  The MFMA wants lane l to hold row l&15, k-group l>>4, but a wave request whose lane QUADS each touch
// a different row is processed at about half the rate of one whose quads read 64 contiguous bytes (measured,
// tools/skinny_probe.hip: 11.5 -> 6.5 us for 64x512x2560).  So lane l LOADS row skinny_ldrow(l), 16-byte segment
// l&3 (every quad = 64 contiguous bytes of one row), and the float4s are then moved to the MFMA's lanes with a fixed
// permutation through ds_bpermute (no LDS storage; it swaps lane bits {0,1} with {4,5}).
__device__ __forceinline__ int skinny_ldrow(int lane) { return 4 * ((lane >> 2) & 3) + (lane >> 4); }
__device__ __forceinline__ int skinny_ldseg(int lane) { return lane & 3; }
__device__ __forceinline__ float4 skinny_xpose(float4 v, int src4) {
    float4 o;
    o.x = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(v.x)));
    o.y = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(v.y)));
    o.z = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(v.z)));
    o.w = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(v.w)));
    return o;
}

// MT 16-row m-tiles x NT 16-col n-tiles per workgroup; K split over the WAVES waves.  ap/wp are this lane's LOAD
// pointers (row skinny_ldrow(lane) of each tile, already offset by 4*skinny_ldseg(lane) floats).  Partial sums of all
// waves end up in red[wave][tile][lane][4] (C/D map of the 16x16 MFMA: col = lane&15, row = 4*(lane>>4)+i).
template <int WAVES, int MT, int NT, int U = 4>
__device__ __forceinline__ void skinny_mma(const float* const (&ap)[MT], const float* const (&wp)[NT], int K, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = skinny_ldseg(lane);
    // MFMA lane (k-group G = lane>>4, row 4a+j = lane&15) takes the float4 loaded by lane 16j + 4a + G
    const int src4 = 4 * (16 * (lane & 3) + (lane & 12) + (lane >> 4));
    const int kper = ((K + WAVES - 1) / WAVES + 15) & ~15;
    const int kbeg = wave * kper;
    const int kend = min(K, kbeg + kper);
    f32x4 acc[MT][NT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[i][j][0] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc[i][j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    // U chunks (16 of K each) in flight per wave.  Chosen by the caller so that a wave's whole K share is requested at
    // once where it fits the registers: a second trip of the loop is a second dependent round of memory latency.
    for (int c0 = kbeg; c0 < kend; c0 += 16 * U) {
        float4 av[MT][U], wv[NT][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = c0 + 16 * u + 4 * g;
            const bool ok = k < kend;
#pragma unroll
            for (int i = 0; i < MT; ++i)
                av[i][u] = ok ? *reinterpret_cast<const float4*>(ap[i] + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < NT; ++j)      // a null row pointer = this lane's row of the tile is unused: zeros, no request
                wv[j][u] = (ok && wp[j]) ? *reinterpret_cast<const float4*>(wp[j] + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < MT; ++i) av[i][u] = skinny_xpose(av[i][u], src4);
#pragma unroll
            for (int j = 0; j < NT; ++j) wv[j][u] = skinny_xpose(wv[j][u], src4);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    // lane group g supplies k = 4g+e to MFMA e; A and W use the same k order, so the sum is exact.
                    acc[i][j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u].x, wv[j][u].x, acc[i][j][0], 0, 0, 0);
                    acc[i][j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u].y, wv[j][u].y, acc[i][j][1], 0, 0, 0);
                    acc[i][j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u].z, wv[j][u].z, acc[i][j][0], 0, 0, 0);
                    acc[i][j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u].w, wv[j][u].w, acc[i][j][1], 0, 0, 0);
                }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            f32x4 s = acc[i][j][0] + acc[i][j][1];
            *reinterpret_cast<f32x4*>(&red[((wave * (MT * NT) + i * NT + j) * 64 + lane) * 4]) = s;
        }
    __syncthreads();
}

// The same product with the W operand stored as fp16 (the 2-byte storage mode: weights the recurrences re-read at every
// time step).  Chunks are 32 of K: lane (row r, segment g) loads 8 consecutive halves of W (one 16-byte request: quads
// still read 64 contiguous bytes) and the matching 8 floats of A as two float4 (k = 8g..8g+3, 8g+4..8g+7); both go through
// the same lane permutation, which leaves MFMA lane (row, k-group G) with k = 8G..8G+7 of its row -- exactly the operand
// layout of v_mfma_f32_16x16x32_f16.  Round 3: ONE fp16 MFMA per chunk (A rounded to fp16 in registers, fp32 accumulation)
// instead of eight v_mfma_f32_16x16x4_f32 on fp32 A x converted W: at configs[4] (M = 256, K = 1024..3072) the per-step
// kernels were bound by the f32 matrix pipe (1.6 GFLOP in 15-26 us = 60-110 TF/s of its 157), and the fp16 pipe runs the
// same chunk in 1/16 of the cycles.  a_scale (a power of two): gradients are small -- backward kernels pass 2^12 so that
// entries down to 1.5e-8 stay normal fp16 numbers and up to 16 stay finite; the sum is scaled back in fp32.  ap/wp are
// already offset by 8*skinny_ldseg(lane) elements.  K % 8 == 0.
typedef _Float16 sk_f16x8 __attribute__((ext_vector_type(8)));
template <int WAVES, int MT, int NT, int U = 2>
__device__ __forceinline__ void skinny_mma_h16(const float* const (&ap)[MT], const vag_half* const (&wp)[NT], int K, float* red,
                                               float a_scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = skinny_ldseg(lane);
    const int src4 = 4 * (16 * (lane & 3) + (lane & 12) + (lane >> 4));
    const int kper = ((K + WAVES - 1) / WAVES + 31) & ~31;
    const int kbeg = wave * kper;
    const int kend = min(K, kbeg + kper);
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = kbeg; c0 < kend; c0 += 32 * U) {
        float4 a0[MT][U], a1[MT][U];
        uint4 wq[NT][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = c0 + 32 * u + 8 * g;
            const bool ok = k < kend;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                a0[i][u] = ok ? *reinterpret_cast<const float4*>(ap[i] + c0 + 32 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
                a1[i][u] = ok ? *reinterpret_cast<const float4*>(ap[i] + c0 + 32 * u + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j)
                wq[j][u] = (ok && wp[j]) ? *reinterpret_cast<const uint4*>(wp[j] + c0 + 32 * u) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            sk_f16x8 af[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float4 x = skinny_xpose(a0[i][u], src4), y = skinny_xpose(a1[i][u], src4);
                const u32x4 q = {pack_f16(x.x * a_scale, x.y * a_scale), pack_f16(x.z * a_scale, x.w * a_scale),
                                 pack_f16(y.x * a_scale, y.y * a_scale), pack_f16(y.z * a_scale, y.w * a_scale)};
                af[i] = __builtin_bit_cast(sk_f16x8, q);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                uint4 q = wq[j][u];
                q.x = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)q.x);
                q.y = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)q.y);
                q.z = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)q.z);
                q.w = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)q.w);
                const u32x4 t = {q.x, q.y, q.z, q.w};
                const sk_f16x8 wf = __builtin_bit_cast(sk_f16x8, t);
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], wf, acc[i][j], 0, 0, 0);
            }
        }
    }
    const float inv = 1.f / a_scale;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const f32x4 s = acc[i][j] * inv;
            *reinterpret_cast<f32x4*>(&red[((wave * (MT * NT) + i * NT + j) * 64 + lane) * 4]) = s;
        }
    __syncthreads();
}
// Dispatch on the W storage type.  koff = this lane's element offset inside a chunk (4g for fp32 W, 8g for fp16 W).
template <bool WH> __device__ __forceinline__ int skinny_koff(int g) { return WH ? 8 * g : 4 * g; }
template <int WAVES, int MT, int NT, int U, bool WH>
__device__ __forceinline__ void skinny_mma_any(const float* const (&ap)[MT], const float* const (&wp)[NT], int K, float* red,
                                               float a_scale = 1.f) {
    if constexpr (WH) {
        const vag_half* wh[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) wh[j] = reinterpret_cast<const vag_half*>(wp[j]);
        skinny_mma_h16<WAVES, MT, NT, (U + 1) / 2>(ap, wh, K, red, a_scale);
    } else {
        skinny_mma<WAVES, MT, NT, U>(ap, wp, K, red);
    }
}
// address of element (row, col) of a W matrix stored as fp32 or fp16 (returned as const float* either way: the half
// version is re-cast inside skinny_mma_any)
template <bool WH> __device__ __forceinline__ const float* skinny_wptr(const float* W, int64_t row, int64_t ldw, int col) {
    if (WH) return reinterpret_cast<const float*>(reinterpret_cast<const vag_half*>(W) + row * ldw + col);
    return W + row * ldw + col;
}

// sum over the waves of tile `tile`, for this lane's 4 accumulator rows
template <int WAVES, int TILES>
__device__ __forceinline__ f32x4 skinny_sum(const float* red, int tile, int lane) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += *reinterpret_cast<const f32x4*>(&red[((w * TILES + tile) * 64 + lane) * 4]);
    return s;
}
// sum over the waves of ONE element (row mrow in [0,16), col in [0,16)) of tile `tile`
template <int WAVES, int TILES>
__device__ __forceinline__ float skinny_sum1(const float* red, int tile, int mrow, int col) {
    const int lane = (mrow >> 2) * 16 + col, i = mrow & 3;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[((w * TILES + tile) * 64 + lane) * 4 + i];
    return s;
}

// One 16x16 output tile per workgroup; the 256 outputs are finished by the first 256 threads (bias / addend requested
// before the product).
template <int WAVES, int U = 4, bool WH = false>
__device__ __forceinline__ void skinny_plain_body(const SkinnyArgs& a, float* red, int bx, int by) {
    const int lane = threadIdx.x & 63;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = by * 16, nb = bx * 16;
    const int erow = (threadIdx.x >> 4) & 15, ecol = threadIdx.x & 15;
    const int em = m0 + erow, ej = nb + ecol;
    const bool eok = threadIdx.x < 256 && em < a.M && ej < a.N;
    float pre = 0.f;
    if (eok) {
        if (a.bias) pre = a.bias[ej];
        if (a.addend) pre += a.addend[(int64_t)em * a.ldadd + ej];
    }
    const float* ap[1];
    const float* wp[1];
    const int64_t arow = a.row_idx ? a.row_idx[min(m0 + r, a.M - 1)] : (int64_t)min(m0 + r, a.M - 1);
    ap[0] = a.A + arow * a.lda + skinny_koff<WH>(g);
    wp[0] = skinny_wptr<WH>(a.W, min(nb + r, a.N - 1), a.ldw, skinny_koff<WH>(g));
    if (a.gather_out && bx == 0) {
        const int k4 = a.K >> 2;
        for (int i = threadIdx.x; i < 16 * k4; i += WAVES * 64) {
            const int row = i / k4, c4 = i - row * k4;
            if (m0 + row < a.M)
                reinterpret_cast<float4*>(a.gather_out + (int64_t)(m0 + row) * a.ld_gather)[c4] =
                    reinterpret_cast<const float4*>(a.A + a.row_idx[m0 + row] * a.lda)[c4];
        }
    }
    skinny_mma_any<WAVES, 1, 1, U, WH>(ap, wp, a.K, red, a.a_scale);
    if (!eok) return;
    float v = skinny_sum1<WAVES, 1>(red, 0, erow, ecol) + pre;
    if (a.act == VAG_ACT_TANH) v = vag_tanh(v);
    a.out[(int64_t)em * a.ldo + ej] = v;
}
// MT x NT 16 x 16 tiles per workgroup (round 4, for M >= 128 rows: configs[4]'s per-step products have 256).  A 16 x 16 tile
// requests 16 rows of each operand; at M = 256, N = 3072, K = 1024 that is 295 MB per product, and the launch runs at the
// chip's aggregate request rate (~6-8 TB/s), not at anything the product itself needs: 2 x 4 tiles request 98 MB.
// red: WAVES x MT NT KB.  No row gather (the decoding-step forms keep the 16 x 16 body).
template <int WAVES, int MT, int NT, int U, bool WH>
__device__ __forceinline__ void skinny_plain_body_mn(const SkinnyArgs& a, float* red, int bx, int by) {
    const int lane = threadIdx.x & 63;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = by * 16 * MT, nb = bx * 16 * NT;
    const float* ap[MT];
    const float* wp[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) ap[i] = a.A + (int64_t)min(m0 + 16 * i + r, a.M - 1) * a.lda + skinny_koff<WH>(g);
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = skinny_wptr<WH>(a.W, min(nb + 16 * j + r, a.N - 1), a.ldw, skinny_koff<WH>(g));
    skinny_mma_any<WAVES, MT, NT, U, WH>(ap, wp, a.K, red, a.a_scale);
    for (int o = threadIdx.x; o < 256 * MT * NT; o += WAVES * 64) {
        const int tile = o >> 8, erow = (o >> 4) & 15, ecol = o & 15;
        const int em = m0 + 16 * (tile / NT) + erow, ej = nb + 16 * (tile % NT) + ecol;
        if (em >= a.M || ej >= a.N) continue;
        float v = skinny_sum1<WAVES, MT * NT>(red, tile, erow, ecol);
        if (a.bias) v += a.bias[ej];
        if (a.addend) v += a.addend[(int64_t)em * a.ldadd + ej];
        if (a.act == VAG_ACT_TANH) v = vag_tanh(v);
        a.out[(int64_t)em * a.ldo + ej] = v;
    }
}
// WH: the W operand is stored as fp16 (batched launches, blockIdx.z, are fp32-only)
template <int WAVES, bool WH = false>
__global__ __launch_bounds__(WAVES * 64) void skinny_plain_kernel(SkinnyArgs a) {
    __shared__ __attribute__((aligned(16))) float red[WAVES * 64 * 4];
    if (blockIdx.z) {
        a.A += blockIdx.z * a.bsA; a.W += blockIdx.z * a.bsW; a.out += blockIdx.z * a.bsO;
        if (a.addend) a.addend += blockIdx.z * a.bsO;
    }
    skinny_plain_body<WAVES, 4, WH>(a, red, blockIdx.x, blockIdx.y);
}

// out (M,N) = act(A1 W1^T + A2 W2^T + A3 W3^T + b1 + b2 + b3) [* dropout]: the pre-activation of the output head for one
// decoding step (NMT_Decoder.py:137-141) in ONE launch instead of three products and a dropout pass.  16x16 tile per
// workgroup; every wave takes its share of each segment's K and keeps accumulating in registers, one reduction at the end.
struct Skinny3Args {
    const float* A[3]; const float* W[3]; const float* bias[3];
    int64_t lda[3], ldw[3];
    int K[3];
    int M, N;
    float* out; int64_t ldo; int act;
    const uint64_t* rng; int sid; float p; int64_t drop_idx0;      // dropout multiplier of element (m,n): index drop_idx0 + m*N + n
    const float* addend = nullptr; int64_t ldadd = 0;              // optional (M,N) term added before the activation
    const float* addend2 = nullptr; const int64_t* idx2 = nullptr; int64_t ldadd2 = 0;     // ... and a second one, row m from line idx2[m]
};
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void skinny3_kernel(Skinny3Args a) {
    __shared__ __attribute__((aligned(16))) float red[WAVES * 64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = blockIdx.y * 16, nb = blockIdx.x * 16;
    const int erow = (threadIdx.x >> 4) & 15, ecol = threadIdx.x & 15;
    const int em = m0 + erow, ej = nb + ecol;
    const bool eok = threadIdx.x < 256 && em < a.M && ej < a.N;
    float pre = 0.f;
    if (eok) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (a.bias[q]) pre += a.bias[q][ej];
        if (a.addend) pre += a.addend[(int64_t)em * a.ldadd + ej];
        if (a.addend2) pre += a.addend2[a.idx2[em] * a.ldadd2 + ej];
    }
    const int src4 = 4 * (16 * (lane & 3) + (lane & 12) + (lane >> 4));
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int K = a.K[q];
        if (K <= 0) continue;
        const float* ap = a.A[q] + (int64_t)min(m0 + r, a.M - 1) * a.lda[q] + 4 * g;
        const float* wp = a.W[q] + (int64_t)min(nb + r, a.N - 1) * a.ldw[q] + 4 * g;
        const int kper = ((K + WAVES - 1) / WAVES + 15) & ~15;
        const int kbeg = wave * kper, kend = min(K, kbeg + kper);
        constexpr int U = 4;
        for (int c0 = kbeg; c0 < kend; c0 += 16 * U) {
            float4 av[U], wv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = c0 + 16 * u + 4 * g < kend;
                av[u] = ok ? *reinterpret_cast<const float4*>(ap + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
                wv[u] = ok ? *reinterpret_cast<const float4*>(wp + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { av[u] = skinny_xpose(av[u], src4); wv[u] = skinny_xpose(wv[u], src4); }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].x, wv[u].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].y, wv[u].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].z, wv[u].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].w, wv[u].w, acc1, 0, 0, 0);
            }
        }
    }
    *reinterpret_cast<f32x4*>(&red[(wave * 64 + lane) * 4]) = acc0 + acc1;
    __syncthreads();
    if (!eok) return;
    float v = skinny_sum1<WAVES, 1>(red, 0, erow, ecol) + pre;
    if (a.act == VAG_ACT_TANH) v = vag_tanh(v);
    if (a.rng && a.p > 0.f) v *= vag_drop_mul(a.rng, a.sid, (uint64_t)(a.drop_idx0 + (int64_t)em * a.N + ej), a.p);
    a.out[(int64_t)em * a.ldo + ej] = v;
}
static bool skinny_ok(const float* A, int64_t lda, const float* W, int64_t ldw, int64_t K);
// Three-segment product; every (A_q, W_q, K_q) must satisfy the skinny alignment rules, M <= 256.
int vag_skinny3_launch(int64_t M, int64_t N, const float* const* A, const int64_t* lda, const float* const* W, const int64_t* ldw,
                       const int64_t* K, const float* const* bias, float* out, int64_t ldo, int act, const uint64_t* rng, int sid,
                       float p, int64_t drop_idx0, hipStream_t stream, const float* addend, int64_t ldadd, const float* addend2,
                       const int64_t* idx2, int64_t ldadd2) {
    VAG_CHECK_ARG(M > 0 && M <= 256 && N > 0 && out);
    Skinny3Args a;
    for (int q = 0; q < 3; ++q) {
        VAG_CHECK_ARG(K[q] == 0 || (A[q] && W[q] && skinny_ok(A[q], lda[q], W[q], ldw[q], K[q])));      // K = 0: the segment is skipped (its bias still counts)
        a.A[q] = A[q]; a.W[q] = W[q]; a.bias[q] = bias[q]; a.lda[q] = lda[q]; a.ldw[q] = ldw[q]; a.K[q] = (int)K[q];
    }
    a.M = (int)M; a.N = (int)N; a.out = out; a.ldo = ldo; a.act = act;
    a.rng = rng; a.sid = sid; a.p = p; a.drop_idx0 = drop_idx0; a.addend = addend; a.ldadd = ldadd;
    VAG_CHECK_ARG(!addend2 || idx2);
    a.addend2 = addend2; a.idx2 = idx2; a.ldadd2 = ldadd2;
    const dim3 grid((unsigned)cdiv64(N, 16), (unsigned)cdiv64(M, 16));
    hipLaunchKernelGGL(skinny3_kernel<8>, grid, dim3(512), 0, stream, a);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// Horizontal fusion for the decoder steps: an attention dot-product pass (a streaming dot per (row, position), latency
// bound, most CUs half idle) and an INDEPENDENT skinny product in one grid.  Backward: the hidden-side part dgh2 W_hh2
// (+ carry) of the next launch's dh1 = [dq | dgh2] [attn_h; W_hh2] -- its operand is known one launch earlier than dq, so
// it runs beside d alpha instead of lengthening the critical path (K 2560 -> 1024 there).  Forward: W_hh2 h1, which the
// scores do not need (they only need attn_h h1), runs beside them instead of in front of them.
// Blocks [0, nscore) are (position chunk, row) pairs of the dot product, the rest are 16x16 tiles of the product.
static bool skinny_ok(const float* A, int64_t lda, const float* W, int64_t ldw, int64_t K);
struct DotArgs {
    const float* x; const float* q; const float* addend; float* out;      // x (B,Ts,W), q (N,ldq), addend/out (N,Ts)
    const float* v; const float* mask;                                     // MODE 0: out = v . tanh(x + q), masked to -inf
    int64_t ldq;
    int Ts, W, gx, nscore;
};
// DS_WAVES waves per block: that many (row, position) pairs, or the K split of one product tile
// S16: 2-byte storage mode -- the streamed operand x (attention keys / projected keys) and the side product's weights
// are fp16 in memory
template <int MODE, int DS_WAVES, bool S16 = false>
__global__ __launch_bounds__(64 * DS_WAVES) void attn_dot_side_kernel(DotArgs d, SkinnyArgs a, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float red[DS_WAVES * 64 * 4];
    // the side product's blocks come FIRST in the grid: each is one long K loop, the reduction's blocks are many and short -- behind
    // them (round 2-3 order) the side product was the kernel's tail: 35.5 / 42.6 us at configs[4] whatever the reduction cost
    const int nside = gridDim.x - d.nscore;
    if ((int)blockIdx.x < nside) {
        const int t = blockIdx.x;
        skinny_plain_body<DS_WAVES, (MODE == 1 ? 6 : 4), S16>(a, red, t % tiles_x, t / tiles_x);
        return;
    }
    const int id = blockIdx.x - nside;
    const int lane = threadIdx.x & 63;
    const int s = (id % d.gx) * DS_WAVES + (threadIdx.x >> 6);
    if (s >= d.Ts) return;
    const int64_t n = id / d.gx;
    const int64_t xrow = (n * d.Ts + s) * d.W;
    const float* qr = d.q + n * d.ldq;
    float acc = 0.f;
    for (int c = lane * 4; c < d.W; c += 256) {
        const float4 pv = ld4_any<S16>(d.x, xrow + c);
        const float4 qv = *reinterpret_cast<const float4*>(qr + c);
        if (MODE == 0) {
            const float4 vv = *reinterpret_cast<const float4*>(d.v + c);
            acc += vv.x * vag_tanh(pv.x + qv.x);
            acc += vv.y * vag_tanh(pv.y + qv.y);
            acc += vv.z * vag_tanh(pv.z + qv.z);
            acc += vv.w * vag_tanh(pv.w + qv.w);
        } else {
            acc += pv.x * qv.x + pv.y * qv.y + pv.z * qv.z + pv.w * qv.w;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (d.addend) acc += d.addend[n * d.Ts + s];
        if (MODE == 0 && d.mask && d.mask[n * d.Ts + s] == 0.f) acc = -INFINITY;
        d.out[n * d.Ts + s] = acc;
    }
}
// Round 4: the same two reductions with the row-constant operands in REGISTERS.  The kernel above re-reads q (and v) for every
// position -- 16 + 16 bytes out of L1 per 8 streamed bytes in the 2-byte mode: the L1, not HBM, set its pace (2.4 / 3.0 TB/s on
// configs[4]'s 84 / 126 MB per step, against 4.1-5.6 TB/s of the neighbouring streaming kernels).  Here a wave owns positions
// s0 + wave, + DS_WAVES, ... of ONE query row and keeps its 8 NJ-float share of q (and v) -- elements 512 j + 8 lane + e -- for all
// of them; a position is NJ 16-byte (fp16 keys) or 2 NJ 16-byte (fp32) loads per lane and nothing else from memory, two positions
// in flight.  W = 512 NJ, NJ in {2, 3, 4, 6} (C = 2H and 3H at H = 512 / 1024); other widths keep the kernel above.
template <bool S16> __device__ __forceinline__ void ld8_any(const float* base, int64_t elem, float (&o)[8]) {
    if (S16) {
        const uint4 p = *reinterpret_cast<const uint4*>(reinterpret_cast<const vag_half*>(base) + elem);
        o[0] = h16_lo(p.x); o[1] = h16_hi(p.x); o[2] = h16_lo(p.y); o[3] = h16_hi(p.y);
        o[4] = h16_lo(p.z); o[5] = h16_hi(p.z); o[6] = h16_lo(p.w); o[7] = h16_hi(p.w);
    } else {
        const float4 a = *reinterpret_cast<const float4*>(base + elem), b = *reinterpret_cast<const float4*>(base + elem + 4);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    }
}
// WIDE: the side product on 2 x 4 tiles per workgroup (M >= 128 rows; 8 waves)
template <int MODE, int DS_WAVES, bool S16, int NJ, bool WIDE>
__global__ __launch_bounds__(64 * DS_WAVES) void attn_dot_side_reg_kernel(DotArgs d, SkinnyArgs a, int tiles_x) {
    constexpr int SMT = WIDE ? 2 : 1, SNT = WIDE ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float red[DS_WAVES * 64 * 4 * SMT * SNT];
    // the side product's blocks come first in the grid (each is one long K loop, the reduction's blocks are many and short).
    // At configs[4] the side product IS the kernel's duration: 35.5 / 42.6 us whatever the reduction costs, until its tiles grew
    const int nside = gridDim.x - d.nscore;
    if ((int)blockIdx.x < nside) {
        const int t = blockIdx.x;
        if (WIDE) skinny_plain_body_mn<DS_WAVES, SMT, SNT, (MODE == 1 ? 4 : 4), S16>(a, red, t % tiles_x, t / tiles_x);
        else skinny_plain_body<DS_WAVES, (MODE == 1 ? 6 : 4), S16>(a, red, t % tiles_x, t / tiles_x);
        return;
    }
    const int id = blockIdx.x - nside;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = id / d.gx;
    const int ppb = (d.Ts + d.gx - 1) / d.gx;                       // positions of this block: [s0, s1)
    const int s0 = (id % d.gx) * ppb, s1 = min(d.Ts, s0 + ppb);
    const float* qr = d.q + n * d.ldq + 8 * lane;
    float q[NJ][8], v[MODE == 0 ? NJ : 1][8];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        ld8_any<false>(qr, 512 * j, q[j]);
        if (MODE == 0) ld8_any<false>(d.v + 8 * lane, 512 * j, v[j]);
    }
    auto dot = [&](const float (&x)[NJ][8]) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += MODE == 0 ? v[j][e] * vag_tanh(x[j][e] + q[j][e]) : x[j][e] * q[j][e];
        return wave_sum(acc);
    };
    auto put = [&](int s, float acc) {
        if (lane == 0) {
            if (d.addend) acc += d.addend[n * d.Ts + s];
            if (MODE == 0 && d.mask && d.mask[n * d.Ts + s] == 0.f) acc = -INFINITY;
            d.out[n * d.Ts + s] = acc;
        }
    };
    const int64_t xbase = n * d.Ts * (int64_t)d.W + 8 * lane;
    int s = s0 + wave;
    for (; s + DS_WAVES < s1; s += 2 * DS_WAVES) {                   // two positions in flight
        float x0[NJ][8], x1[NJ][8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            ld8_any<S16>(d.x, xbase + (int64_t)s * d.W + 512 * j, x0[j]);
            ld8_any<S16>(d.x, xbase + (int64_t)(s + DS_WAVES) * d.W + 512 * j, x1[j]);
        }
        put(s, dot(x0));
        put(s + DS_WAVES, dot(x1));
    }
    if (s < s1) {
        float x0[NJ][8];
#pragma unroll
        for (int j = 0; j < NJ; ++j) ld8_any<S16>(d.x, xbase + (int64_t)s * d.W + 512 * j, x0[j]);
        put(s, dot(x0));
    }
}
// mode 1: out (N,Ts) = x[n,s,:] . q[n,:] + addend;  mode 0: out = v . tanh(x[n,s,:] + q[n,:]), -inf where mask (N,Ts) == 0.
// One source row per query row (training: N = B).  Side product in the same grid:
// P (M,Np) = A (M,K) Wt^T + pbias + padd;  A row stride lda, Wt (Np,K) row stride ldw, padd (M,Np) contiguous, P row stride ldp.
int vag_attn_dot_side_launch(int mode, const float* x, const float* q, int64_t ldq, const float* v, const float* mask,
                             const float* addend, int64_t N, int64_t Ts, int64_t W, float* out, int64_t M, int64_t Np,
                             int64_t K, const float* A, int64_t lda, const float* Wt, int64_t ldw, const float* pbias,
                             const float* padd, float* P, int64_t ldp, hipStream_t stream, bool s16) {
    VAG_CHECK_ARG(x && q && out && N > 0 && Ts > 0 && W > 0 && W % 4 == 0 && ldq % 4 == 0 && aligned16(x) && aligned16(q));
    VAG_CHECK_ARG((mode == 1 || (mode == 0 && v && aligned16(v))) && A && Wt && P && M > 0 && Np > 0 &&
                  skinny_ok(A, lda, Wt, ldw, K));
    DotArgs d;
    d.x = x; d.q = q; d.addend = addend; d.out = out; d.v = v; d.mask = mask; d.ldq = ldq; d.Ts = (int)Ts; d.W = (int)W;
    const int DS_WAVES = mode == 0 ? 8 : 16;        // measured: forward side product K = H, backward K = 3H
    d.gx = (int)cdiv64(Ts, DS_WAVES);
    VAG_CHECK_ARG((int64_t)d.gx * N < (1ll << 30));
    d.nscore = (int)(d.gx * N);
    SkinnyArgs a;
    a.A = A; a.W = Wt; a.lda = lda; a.ldw = ldw; a.M = (int)M; a.N = (int)Np; a.K = (int)K;
    a.bias = pbias; a.addend = padd; a.ldadd = Np; a.out = P; a.ldo = ldp; a.act = VAG_ACT_NONE;
    a.a_scale = mode == 1 ? 4096.f : 1.f;           // backward: the riding product's A operand is a gate gradient
    const int tiles_x = (int)cdiv64(Np, 16), tiles_y = (int)cdiv64(M, 16);
    if (W % 512 == 0 && (W == 1024 || W == 1536 || W == 2048 || W == 3072) && aligned16(v ? v : q) && (!s16 || K % 8 == 0) &&
        vag_opt().attn_dot_reg != 0) {
        // row-constant operands in registers (attn_dot_side_reg_kernel): a block = positions [g ppb, (g + 1) ppb) of one row
        const bool wide = M >= 128;                 // the side product on 32 x 64 tiles (skinny_plain_body_mn), 8 waves either way
        const int WV = (mode == 0 || wide) ? 8 : 16;
        int64_t gx = cdiv64(512, N);
        const int64_t gmax = Ts / (2 * WV) > 1 ? Ts / (2 * WV) : 1;
        if (gx > gmax) gx = gmax;
        d.gx = (int)gx;
        d.nscore = (int)(gx * N);
        const int stx = wide ? (int)cdiv64(Np, 64) : tiles_x, sty = wide ? (int)cdiv64(M, 32) : tiles_y;
        const dim3 grid2((unsigned)(d.nscore + stx * sty));
#define VAG_DOTREG(MODE_, WV, S16_, NJ_)                                                                                        \
        { if (wide) hipLaunchKernelGGL((attn_dot_side_reg_kernel<MODE_, WV, S16_, NJ_, true>), grid2, dim3(64 * WV), 0, stream, d, a, stx); \
          else hipLaunchKernelGGL((attn_dot_side_reg_kernel<MODE_, WV, S16_, NJ_, false>), grid2, dim3(64 * WV), 0, stream, d, a, stx); }
#define VAG_DOTREG_NJ(MODE_, WV, S16_)                                                      \
        switch (W / 512) {                                                                  \
            case 2: VAG_DOTREG(MODE_, WV, S16_, 2); break;                                  \
            case 3: VAG_DOTREG(MODE_, WV, S16_, 3); break;                                  \
            case 4: VAG_DOTREG(MODE_, WV, S16_, 4); break;                                  \
            default: VAG_DOTREG(MODE_, WV, S16_, 6); break;                                 \
        }
        if (s16) { if (mode == 0) { VAG_DOTREG_NJ(0, 8, true) } else if (wide) { VAG_DOTREG_NJ(1, 8, true) } else { VAG_DOTREG_NJ(1, 16, true) } }
        else { if (mode == 0) { VAG_DOTREG_NJ(0, 8, false) } else if (wide) { VAG_DOTREG_NJ(1, 8, false) } else { VAG_DOTREG_NJ(1, 16, false) } }
#undef VAG_DOTREG_NJ
#undef VAG_DOTREG
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    const dim3 grid((unsigned)(d.nscore + tiles_x * tiles_y));
    if (s16) {
        VAG_CHECK_ARG(K % 8 == 0 && W % 4 == 0);
        if (mode == 0) hipLaunchKernelGGL((attn_dot_side_kernel<0, 8, true>), grid, dim3(512), 0, stream, d, a, tiles_x);
        else hipLaunchKernelGGL((attn_dot_side_kernel<1, 16, true>), grid, dim3(1024), 0, stream, d, a, tiles_x);
    } else {
        if (mode == 0) hipLaunchKernelGGL((attn_dot_side_kernel<0, 8>), grid, dim3(512), 0, stream, d, a, tiles_x);
        else hipLaunchKernelGGL((attn_dot_side_kernel<1, 16>), grid, dim3(1024), 0, stream, d, a, tiles_x);
    }
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// out[m,n] = sum_k A[m,k] B[k,n] with B stored (K,N) row-major (data gradients dX = dY W of the once-per-batch
// M <= 128-row operators: the LDS-tiled kernels need ~14 us for these however small they are).  A is loaded as in
// skinny_mma; B is read directly in MFMA layout, one dword per lane and k (16 consecutive n = 64 contiguous bytes).
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void skinny_bt_kernel(SkinnyArgs a) {
    __shared__ __attribute__((aligned(16))) float red[WAVES * 64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 16, nb = blockIdx.x * 16;
    const int erow = (threadIdx.x >> 4) & 15, ecol = threadIdx.x & 15;
    const int em = m0 + erow, ej = nb + ecol;
    const bool eok = threadIdx.x < 256 && em < a.M && ej < a.N;
    const float* ap = a.A + (int64_t)min(m0 + skinny_ldrow(lane), a.M - 1) * a.lda + 4 * skinny_ldseg(lane);
    const int src4 = 4 * (16 * (lane & 3) + (lane & 12) + (lane >> 4));
    const int g = lane >> 4;
    const float* bp = a.W + min(nb + (lane & 15), a.N - 1);
    const int kper = ((a.K + WAVES - 1) / WAVES + 15) & ~15;
    const int kbeg = wave * kper;
    const int kend = min(a.K, kbeg + kper);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 2;
    for (int c0 = kbeg; c0 < kend; c0 += 16 * U) {
        float4 av[U];
        float bv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ka = c0 + 16 * u + 4 * skinny_ldseg(lane);
            av[u] = ka < kend ? *reinterpret_cast<const float4*>(ap + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
            const int kb = c0 + 16 * u + 4 * g;
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[u][e] = kb < kend ? bp[(int64_t)(kb + e) * a.ldw] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 x = skinny_xpose(av[u], src4);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, bv[u][0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, bv[u][1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, bv[u][2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, bv[u][3], acc1, 0, 0, 0);
        }
    }
    *reinterpret_cast<f32x4*>(&red[(wave * 64 + lane) * 4]) = acc0 + acc1;
    __syncthreads();
    if (!eok) return;
    float v = skinny_sum1<WAVES, 1>(red, 0, erow, ecol);
    if (a.bias) v += a.bias[ej];
    if (a.addend) v += a.addend[(int64_t)em * a.ldadd + ej];
    a.out[(int64_t)em * a.ldo + ej] = v;
    if (a.out2) {
        float* o2 = a.out2 + (int64_t)em * a.ldo2 + ej;
        *o2 = (a.acc2 ? *o2 : 0.f) + a.scale2 * v;
    }
}

// Fused GRU cell: 16 rows x 16 hidden units x 3 gates per workgroup.  The 256 (row, unit) outputs are finished by the
// first 256 threads, one each; their epilogue operands (the other projection, h_prev, bias) are requested BEFORE the
// product so that they arrive under it instead of costing a second memory round trip.
// MT 16-row tiles per workgroup (2 for wide batches: the three gate rows of W are then re-read by half as many workgroups).
template <int WAVES, bool WH = false, int MT = 1>
__global__ __launch_bounds__(WAVES * 64) void gru_step_kernel(GruStepArgs a) {
    constexpr int NT = 3;
    __shared__ __attribute__((aligned(16))) float red[WAVES * MT * NT * 64 * 4];
    const GruSide& sd = a.s[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = blockIdx.y * 16 * MT, u0 = blockIdx.x * 16;
    const int H = a.H;
    // epilogue operands: output q of thread t is (row m0 + 16*(t'/256) + (t'%256)/16, unit u0 + t'%16), t' = t + q*threads
    constexpr int OUTS = (MT * 256 + WAVES * 64 - 1) / (WAVES * 64);
    float o_r[OUTS], o_z[OUTS], o_n[OUTS], hp[OUTS], b_r[OUTS], b_z[OUTS], b_n[OUTS];
    bool active[OUTS], eok[OUTS];
#pragma unroll
    for (int q = 0; q < OUTS; ++q) {
        const int t = threadIdx.x + q * WAVES * 64;
        const int em = m0 + 16 * (t >> 8) + ((t >> 4) & 15), ej = u0 + (t & 15);
        eok[q] = t < MT * 256 && em < a.M && ej < H;
        o_r[q] = o_z[q] = o_n[q] = hp[q] = b_r[q] = b_z[q] = b_n[q] = 0.f;
        active[q] = true;
        if (eok[q]) {
            const float* op = sd.other + (sd.other_idx ? sd.other_idx[em] : (int64_t)em) * a.ldother + ej;
            o_r[q] = op[0]; o_z[q] = op[H]; o_n[q] = op[2 * H];
            hp[q] = sd.hprev[(int64_t)em * a.ldh + ej];
            if (sd.bias) { b_r[q] = sd.bias[ej]; b_z[q] = sd.bias[H + ej]; b_n[q] = sd.bias[2 * H + ej]; }
            if (a.lengths) active[q] = sd.t < a.lengths[em];
        }
    }
    const float* ap[MT];
    const float* wp[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) ap[i] = sd.A + (int64_t)min(m0 + 16 * i + r, a.M - 1) * a.lda + skinny_koff<WH>(g);
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = skinny_wptr<WH>(sd.W, min(j * H + u0 + r, 3 * H - 1), a.ldw, skinny_koff<WH>(g));
    skinny_mma_any<WAVES, MT, NT, 4, WH>(ap, wp, a.K, red);
#pragma unroll
    for (int q = 0; q < OUTS; ++q) {
        if (!eok[q]) continue;
        const int t = threadIdx.x + q * WAVES * 64;
        const int mt = t >> 8, erow = (t >> 4) & 15, ecol = t & 15;
        const int em = m0 + 16 * mt + erow, ej = u0 + ecol;
        const float c_r = skinny_sum1<WAVES, MT * NT>(red, mt * NT + 0, erow, ecol) + b_r[q];
        const float c_z = skinny_sum1<WAVES, MT * NT>(red, mt * NT + 1, erow, ecol) + b_z[q];
        const float c_n = skinny_sum1<WAVES, MT * NT>(red, mt * NT + 2, erow, ecol) + b_n[q];
        const float gi_n = a.comp_hidden ? o_n[q] : c_n;
        const float gh_n = a.comp_hidden ? c_n : o_n[q];
        const float rr = vag_sigmoid(c_r + o_r[q]);
        const float zz = vag_sigmoid(c_z + o_z[q]);
        const float nn = vag_tanh(gi_n + rr * gh_n);
        const float hn = (1.f - zz) * nn + zz * hp[q];
        const int64_t o = (int64_t)em * H + ej;
        if (sd.save) {
            const int64_t MH = (int64_t)a.M * H;
            sd.save[o] = rr; sd.save[MH + o] = zz; sd.save[2 * MH + o] = nn; sd.save[3 * MH + o] = gh_n;
        }
        sd.hout[o] = active[q] ? hn : hp[q];
        if (sd.out2) sd.out2[(int64_t)em * a.ld2 + ej] = active[q] ? hn : 0.f;
    }
}

// The same cell with 8 or 4 hidden units per workgroup (2x / 4x the workgroups).  UNITS = 8: tile 0 holds [r | z] of
// the 8 units, tile 1 [n | unused]; UNITS = 4: one tile [r | z | n | unused].  For single-direction launches with
// M <= 64 rows this puts a workgroup on every CU instead of every other one, with less MFMA time and fewer bytes per
// workgroup (unused tile rows issue no loads).
template <int WAVES, int UNITS, bool WH = false>
__global__ __launch_bounds__(WAVES * 64) void gru_step_small_kernel(GruStepArgs a) {
    constexpr int NT = UNITS == 8 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float red[WAVES * NT * 64 * 4];
    const GruSide& sd = a.s[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = blockIdx.y * 16, u0 = blockIdx.x * UNITS;
    const int H = a.H;
    // epilogue operands of thread t < 16*UNITS: output (row m0 + t/UNITS, unit u0 + t%UNITS)
    const int erow = (threadIdx.x / UNITS) & 15, ecol = threadIdx.x % UNITS;
    const int em = m0 + erow, ej = u0 + ecol;
    const bool eok = threadIdx.x < 16 * UNITS && em < a.M && ej < H;
    float o_r = 0.f, o_z = 0.f, o_n = 0.f, hp = 0.f, b_r = 0.f, b_z = 0.f, b_n = 0.f;
    bool active = true;
    if (eok) {
        const float* op = sd.other + (sd.other_idx ? sd.other_idx[em] : (int64_t)em) * a.ldother + ej;
        o_r = op[0]; o_z = op[H]; o_n = op[2 * H];
        hp = sd.hprev[(int64_t)em * a.ldh + ej];
        if (sd.bias) { b_r = sd.bias[ej]; b_z = sd.bias[H + ej]; b_n = sd.bias[2 * H + ej]; }
        if (a.lengths) active = sd.t < a.lengths[em];
    }
    const float* ap[1];
    const float* wp[NT];
    ap[0] = sd.A + (int64_t)min(m0 + r, a.M - 1) * a.lda + skinny_koff<WH>(g);
    const int unit = min(u0 + (r % UNITS), H - 1);
    const int gate = r / UNITS;                                   // gate of tile 0's row r
    const int ko = skinny_koff<WH>(g);
    if (UNITS == 8) {
        wp[0] = skinny_wptr<WH>(sd.W, gate * H + unit, a.ldw, ko);                                  // r | z
        wp[NT - 1] = r < 8 ? skinny_wptr<WH>(sd.W, 2 * H + unit, a.ldw, ko) : nullptr;              // n | -
    } else {
        wp[0] = gate < 3 ? skinny_wptr<WH>(sd.W, gate * H + unit, a.ldw, ko) : nullptr;             // r | z | n | -
    }
    skinny_mma_any<WAVES, 1, NT, 4, WH>(ap, wp, a.K, red);
    if (!eok) return;
    const float c_r = skinny_sum1<WAVES, NT>(red, 0, erow, ecol) + b_r;
    const float c_z = skinny_sum1<WAVES, NT>(red, 0, erow, UNITS + ecol) + b_z;
    const float c_n = (UNITS == 8 ? skinny_sum1<WAVES, NT>(red, NT - 1, erow, ecol)
                                  : skinny_sum1<WAVES, NT>(red, 0, erow, 2 * UNITS + ecol)) + b_n;
    const float gi_n = a.comp_hidden ? o_n : c_n;
    const float gh_n = a.comp_hidden ? c_n : o_n;
    const float rr = vag_sigmoid(c_r + o_r);
    const float zz = vag_sigmoid(c_z + o_z);
    const float nn = vag_tanh(gi_n + rr * gh_n);
    const float hn = (1.f - zz) * nn + zz * hp;
    const int64_t o = (int64_t)em * H + ej;
    if (sd.save) {
        const int64_t MH = (int64_t)a.M * H;
        sd.save[o] = rr; sd.save[MH + o] = zz; sd.save[2 * MH + o] = nn; sd.save[3 * MH + o] = gh_n;
    }
    sd.hout[o] = active ? hn : hp;
    if (sd.out2) sd.out2[(int64_t)em * a.ld2 + ej] = active ? hn : 0.f;
}

// dh = A WT^T + addend, then the GRU cell backward (elementwise) that consumes dh -- see common.h.
// Same structure: 256 outputs finished by 256 threads, epilogue operands prefetched under the product.
// (A half-tile variant -- 8 output columns per workgroup on twice the workgroups, as gru_step_small_kernel does for the
// forward cell -- measured no gain here: the MFMA count per workgroup stays that of a full tile.)
// MT x NT 16x16 tiles per workgroup (1 x 1 for M <= 64 rows: one workgroup per CU matters more there; 2 x 2 for the wide
// configuration, where each launch is bound by operand re-reads out of L2: 300 MB -> 150 MB at M = 256, H = 1024).
template <int WAVES, int U, bool WH = false, int MT = 1, int NT = 1>
__global__ __launch_bounds__(WAVES * 64) void gru_bwd_step_kernel(GruBwdStepArgs a) {
    constexpr int TILES = MT * NT;
    __shared__ __attribute__((aligned(16))) float red[WAVES * TILES * 64 * 4];
    const GruBwdStepSide& sd = a.s[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int r = skinny_ldrow(lane), g = skinny_ldseg(lane);
    const int m0 = blockIdx.y * 16 * MT, nb = blockIdx.x * 16 * NT;
    const int H = a.H;
    const int64_t MH = (int64_t)a.M * H;
    constexpr int OUTS = (TILES * 256 + WAVES * 64 - 1) / (WAVES * 64);      // outputs per thread
    float add[OUTS], e[OUTS], rr[OUTS], zz[OUTS], nn[OUTS], hn[OUTS], hp[OUTS];
    bool active[OUTS], eok[OUTS];
    int64_t oo[OUTS];
#pragma unroll
    for (int q = 0; q < OUTS; ++q) {
        const int t = threadIdx.x + q * WAVES * 64;
        const int tile = t >> 8, erow = (t >> 4) & 15, ecol = t & 15;
        const int em = m0 + 16 * (tile / NT) + erow, ej = nb + 16 * (tile % NT) + ecol;
        eok[q] = tile < TILES && em < a.M && ej < H;
        oo[q] = (int64_t)em * H + ej;
        add[q] = e[q] = rr[q] = zz[q] = nn[q] = hn[q] = hp[q] = 0.f;
        active[q] = true;
        if (eok[q]) {
            if (sd.addend) add[q] = sd.addend[oo[q]];
            if (a.has_cell) {
                if (a.lengths) active[q] = sd.t < a.lengths[em];
                if (sd.dh_add) {
                    e[q] = sd.dh_add[(int64_t)em * a.ld_add + ej];
                    if (a.rng && a.p > 0.f) e[q] *= vag_drop_mul(a.rng, a.sid, (uint64_t)em * a.ld_add + sd.drop_idx0 + ej, a.p);
                }
                rr[q] = sd.save[oo[q]]; zz[q] = sd.save[MH + oo[q]]; nn[q] = sd.save[2 * MH + oo[q]]; hn[q] = sd.save[3 * MH + oo[q]];
                hp[q] = sd.hprev[(int64_t)em * a.ldh + ej];
            }
        }
    }
    const float* ap[MT];
    const float* wp[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) ap[i] = sd.A + (int64_t)min(m0 + 16 * i + r, a.M - 1) * a.lda + skinny_koff<WH>(g);
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = skinny_wptr<WH>(sd.WT, min(nb + 16 * j + r, H - 1), a.ldw, skinny_koff<WH>(g));
    skinny_mma_any<WAVES, MT, NT, U, WH>(ap, wp, a.K, red, 4096.f);       // A = gate gradients: scaled into fp16's range
#pragma unroll
    for (int q = 0; q < OUTS; ++q) {
        if (!eok[q]) continue;
        const int t = threadIdx.x + q * WAVES * 64;
        const int tile = t >> 8, erow = (t >> 4) & 15, ecol = t & 15;
        const int em = m0 + 16 * (tile / NT) + erow, ej = nb + 16 * (tile % NT) + ecol;
        const int64_t o = oo[q];
        float dh = skinny_sum1<WAVES, TILES>(red, tile, erow, ecol) + add[q];
        if (!a.has_cell) {
            sd.dh_out[o] = dh;
            continue;
        }
        float* gi = sd.dgi + (int64_t)em * a.ldgi + ej;
        float* gh = sd.dgh + (int64_t)em * a.ldgh + ej;
        if (!active[q]) {
            gi[0] = 0.f; gi[H] = 0.f; gi[2 * H] = 0.f;
            gh[0] = 0.f; gh[H] = 0.f; gh[2 * H] = 0.f;
            sd.dh_direct[o] = dh;
            continue;
        }
        dh += e[q];
        const float dn_pre = dh * (1.f - zz[q]) * (1.f - nn[q] * nn[q]);
        const float dz_pre = dh * (hp[q] - nn[q]) * zz[q] * (1.f - zz[q]);
        const float dr_pre = dn_pre * hn[q] * rr[q] * (1.f - rr[q]);
        gi[0] = dr_pre; gi[H] = dz_pre; gi[2 * H] = dn_pre;
        gh[0] = dr_pre; gh[H] = dz_pre; gh[2 * H] = dn_pre * rr[q];
        sd.dh_direct[o] = dh * zz[q];
    }
}

static bool skinny_ok(const float* A, int64_t lda, const float* W, int64_t ldw, int64_t K) {
    return aligned16(A) && aligned16(W) && lda % 4 == 0 && ldw % 4 == 0 && K % 4 == 0 && K >= 4;
}

// 32 x 64 outputs per workgroup (skinny_plain_body_mn): wide batches
template <int WAVES, bool WH>
__global__ __launch_bounds__(WAVES * 64) void skinny_plain_mn_kernel(SkinnyArgs a) {
    __shared__ __attribute__((aligned(16))) float red[WAVES * 64 * 4 * 8];
    skinny_plain_body_mn<WAVES, 2, 4, 4, WH>(a, red, blockIdx.x, blockIdx.y);
}
static void skinny_plain_go(const SkinnyArgs& a, hipStream_t stream, bool w16 = false) {
    // wide batches (configs[4]: 256 rows): 32 x 64 tiles request a third of the operand bytes; as long as >= 192 workgroups remain (beam decoding has 192 rows)
    if (a.M >= 128 && a.K > 256 && a.K <= 1024 && !a.row_idx && !a.gather_out && cdiv64(a.N, 64) * cdiv64(a.M, 32) >= 192) {
        dim3 gw((unsigned)cdiv64(a.N, 64), (unsigned)cdiv64(a.M, 32), 1);
        if (w16) hipLaunchKernelGGL((skinny_plain_mn_kernel<8, true>), gw, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((skinny_plain_mn_kernel<8, false>), gw, dim3(512), 0, stream, a);
        return;
    }
    dim3 grid((unsigned)cdiv64(a.N, 16), (unsigned)cdiv64(a.M, 16), 1);
    if (w16) {
        if (a.K <= 256) hipLaunchKernelGGL((skinny_plain_kernel<4, true>), grid, dim3(256), 0, stream, a);
        else if (a.K <= 1024) hipLaunchKernelGGL((skinny_plain_kernel<8, true>), grid, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((skinny_plain_kernel<16, true>), grid, dim3(1024), 0, stream, a);
        return;
    }
    if (a.K <= 256) hipLaunchKernelGGL((skinny_plain_kernel<4>), grid, dim3(256), 0, stream, a);
    else if (a.K <= 1024) hipLaunchKernelGGL((skinny_plain_kernel<8>), grid, dim3(512), 0, stream, a);
    else hipLaunchKernelGGL((skinny_plain_kernel<16>), grid, dim3(1024), 0, stream, a);
}

// out (M,N) = table[idx[m], :] W^T + bias, and gathered (M,K) = table[idx[m], :]: embedding lookup and input projection of one
// decoding step in one launch.  M <= 256, K % 4 == 0.
int vag_skinny_gather_launch(int64_t M, int64_t N, int64_t K, const float* table, int64_t ldt, const int64_t* idx, const float* W,
                             int64_t ldw, const float* bias, float* out, int64_t ldo, float* gathered, int64_t ldg,
                             hipStream_t stream) {
    VAG_CHECK_ARG(M > 0 && M <= 256 && N > 0 && table && idx && W && out && gathered && skinny_ok(table, ldt, W, ldw, K) &&
                  aligned16(gathered) && ldg % 4 == 0);
    SkinnyArgs a;
    a.A = table; a.W = W; a.lda = ldt; a.ldw = ldw; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.bias = bias; a.addend = nullptr; a.ldadd = 0; a.out = out; a.ldo = ldo; a.act = VAG_ACT_NONE;
    a.row_idx = idx; a.gather_out = gathered; a.ld_gather = ldg;
    skinny_plain_go(a, stream);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// ------------------------------------------------------------------------------------------------
// Tall-skinny product for the per-step vocabulary head of decoding and of free-running training steps (round 4):
// out[M, N] = A[M, K] W[N, K]^T + bias, M <= 256 rows (B*k hypotheses, or the batch), N = V large, K = E small.
// (NMT_Decoder.py:143 at one time step: models/...V11.py:148-160 free running, :259-313 beam search.)
// The 16x16-tile skinny kernel requests M*N*K/2 bytes chip-wide (230 MB at 192 x 9391 x 256: 38 us) and the 64x64 LDS-tiled f32
// kernel took 17.5 us in the beam step / 16 us in the greedy step (profiles/r04_decode_kernel_stats.csv): both pay for
// re-reading operands, W above all.  Here a workgroup owns 64 columns for ALL rows: its W tile is read once, split exactly into
// three bf16 planes and kept in LDS (K chunks of 256: 99 KB), wave (row tile, k split) streams its 32 rows of A straight from
// memory in MFMA operand layout, splits them in registers and runs the six products (bf16x6, fp32-grade: the arithmetic of the
// training step's logits product, gemm.hip).  Requested bytes: N/64 x (M + 64) x K x 4 (38 MB instead of 230).
struct TallArgs {
    const float* A; const float* W; const float* bias; float* out;
    float* parts;              // NULL, or (gridDim.x, M, 2): per row the (max, sum of exp(. - max)) of this workgroup's 64 columns -- the
                               // pieces of the row's log-sum-exp, so that decoding needs no pass over the logits to normalise them
    int64_t lda, ldw, ldo;
    int M, N, K, RT, KS;       // RT = ceil(M / 32) row tiles, KS = k splits: RT * KS <= 8 waves
};
constexpr int TALL_KC = 256;                       // K chunk staged in LDS
constexpr int TALL_LD = TALL_KC + 8;               // bf16 elements per LDS row: 528 B = 132 dwords = 4 mod 64 banks: conflict-free b128 reads
constexpr int TALL_PLANE = 64 * TALL_LD;
constexpr int TALL_LDS_BYTES = 3 * TALL_PLANE * 2; // 101376
__global__ __launch_bounds__(512, 2) void skinny_tall_kernel(TallArgs a) {
    extern __shared__ __attribute__((aligned(16))) __bf16 tall_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 64;
    const int rt = wave / a.KS, ks = wave % a.KS;
    const bool active = rt < a.RT;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int arow = min(rt * 32 + (lane & 31), a.M - 1);
    const float* Ap = a.A + (int64_t)arow * a.lda + 8 * (lane >> 5);
    // staging map: thread -> (W row = tid >> 3, 32 consecutive k at (tid & 7) * 32)
    const int srow = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 32;
    const float* Wp = a.W + (int64_t)min(n0 + srow, a.N - 1) * a.ldw + sk;
    for (int kc = 0; kc < a.K; kc += TALL_KC) {
        const int klen = min(TALL_KC, a.K - kc);              // multiple of 32 (launcher)
        if (kc > 0) __syncthreads();
        if (sk < klen) {
            float4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float4*>(Wp + kc + 4 * i);
#pragma unroll
            for (int i = 0; i < 4; ++i) {                      // 8 consecutive k -> one 16-byte store per plane
                unsigned p[3][4];
                split3(v[2 * i].x, v[2 * i].y, p[0][0], p[1][0], p[2][0]);
                split3(v[2 * i].z, v[2 * i].w, p[0][1], p[1][1], p[2][1]);
                split3(v[2 * i + 1].x, v[2 * i + 1].y, p[0][2], p[1][2], p[2][2]);
                split3(v[2 * i + 1].z, v[2 * i + 1].w, p[0][3], p[1][3], p[2][3]);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    *reinterpret_cast<uint4*>(tall_smem + q * TALL_PLANE + srow * TALL_LD + sk + 8 * i) =
                        make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
            }
        }
        __syncthreads();
        if (active) {
            const int per = klen / a.KS;                       // k range of this wave inside the chunk: 64, 128 or 256 (launcher)
            const int kb = ks * per;
            const __bf16* Bf = tall_smem + (lane & 31) * TALL_LD + 8 * (lane >> 5);
            // the wave's rows of A in groups of 64 k (8 x 16-byte loads per lane), the next group in flight under the current
            // one's MFMAs: a k-step that waited for its own two loads cost a memory round trip each (16 us at 16 k-steps)
            const int ng = per >> 6;
            float4 xa[2][8];
            auto load_group = [&](int g, float4 (&x)[8]) {
                const float* src = Ap + kc + kb + 64 * g;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    x[2 * i] = *reinterpret_cast<const float4*>(src + 16 * i);
                    x[2 * i + 1] = *reinterpret_cast<const float4*>(src + 16 * i + 4);
                }
            };
            auto compute_group = [&](int g, const float4 (&x)[8]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k0 = kb + 64 * g + 16 * i;
                    const float4 x0 = x[2 * i], x1 = x[2 * i + 1];
                    unsigned q[3][4];
                    split3(x0.x, x0.y, q[0][0], q[1][0], q[2][0]);
                    split3(x0.z, x0.w, q[0][1], q[1][1], q[2][1]);
                    split3(x1.x, x1.y, q[0][2], q[1][2], q[2][2]);
                    split3(x1.z, x1.w, q[0][3], q[1][3], q[2][3]);
                    bf16x8 af[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const u32x4 t = {q[p][0], q[p][1], q[p][2], q[p][3]};
                        af[p] = __builtin_bit_cast(bf16x8, t);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        bf16x8 bf[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p) bf[p] = sp_frag(Bf + p * TALL_PLANE + j * 32 * TALL_LD + k0);
                        // smallest terms first (the order of sp_compute)
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[2], acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bf[1], acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], bf[0], acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[1], acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bf[0], acc[j], 0, 0, 0);
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[0], acc[j], 0, 0, 0);
                    }
                }
            };
            load_group(0, xa[0]);
            for (int g = 0; g < ng; g += 2) {
                if (g + 1 < ng) load_group(g + 1, xa[1]);
                compute_group(g, xa[0]);
                if (g + 1 < ng) {
                    if (g + 2 < ng) load_group(g + 2, xa[0]);
                    compute_group(g + 1, xa[1]);
                }
            }
        }
    }
    // the k splits of a row tile meet in LDS (the W planes are done with)
    if (a.KS > 1) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(tall_smem);      // [wave][j][r][lane]
        if (active && ks > 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((wave * 2 + j) * 16 + r) * 64 + lane] = acc[j][r];
        }
        __syncthreads();
        if (active && ks == 0) {
            for (int o = 1; o < a.KS; ++o)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[j][r] += red[(((wave + o) * 2 + j) * 16 + r) * 64 + lane];
        }
    }
    if (a.parts) __syncthreads();      // the epilogue below transposes through the LDS the other waves' MFMAs may still be reading
    if (!active || ks != 0) return;
    const int row0 = rt * 32 + 4 * (lane >> 5);
    float bvj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + j * 32 + (lane & 31);
        bvj[j] = (a.bias && col < a.N) ? a.bias[col] : 0.f;
        if (col >= a.N) continue;
        gemm_epilogue16(acc[j], a.out + (int64_t)row0 * a.ldo + col, a.ldo, a.M - row0, 1.f, 0.f, bvj[j], 0, false);
    }
    if (a.parts) {
        // A row's 64 values sit in the 32 lanes of one half of the wave.  Through LDS (the W planes are done with; 4.2 KB per wave
        // beyond the k-split reduction area, row stride 33) so that lane l owns row l & 31, columns 16 (l >> 5) .. + 15 of a 32-column
        // half, serially; the two column halves and the two lane halves are merged as (max, sum) pairs.  Layout [workgroup][row]:
        // a wave's 32 results are 256 contiguous bytes.
        float* T = reinterpret_cast<float*>(tall_smem) + 16384 + wave * (32 * 33);
        const int rl = lane & 31, ch = lane >> 5;
        float m = -INFINITY, sm = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool cok = n0 + j * 32 + rl < a.N;
#pragma unroll
            for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * ch) * 33 + rl] = cok ? acc[j][r] + bvj[j] : -INFINITY;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = T[rl * 33 + 16 * ch + e];
            float mj = v[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mj = fmaxf(mj, v[e]);
            float sj = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) sj += v[e] == -INFINITY ? 0.f : __expf(v[e] - mj);
            const float mn = fmaxf(m, mj);
            sm = (m == -INFINITY ? 0.f : sm * __expf(m - mn)) + (mj == -INFINITY ? 0.f : sj * __expf(mj - mn));
            m = mn;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        const float mo = __shfl_xor(m, 32, 64), so = __shfl_xor(sm, 32, 64);
        const float mn = fmaxf(m, mo);
        sm = (m == -INFINITY ? 0.f : sm * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
        const int row = rt * 32 + rl;
        if (ch == 0 && row < a.M) *reinterpret_cast<float2*>(a.parts + ((int64_t)blockIdx.x * a.M + row) * 2) = make_float2(mn, sm);
    }
}
static bool skinny_tall_ok(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw) {
    // measured (tools/exp_tall.py, 20 launches per graph; us): M = 192: V = 9391 16.2 vs 18.3 on the LDS-tiled f32 kernel, V = 40000 45 vs 49;
    // M = 16: 7.1 vs 4.1 on the 16x16 skinny kernel -- one workgroup per CU is a chain of memory round trips, so only the wide cases come here
    return M > 96 && M <= 256 && N >= 4096 && K >= 256 && K % 256 == 0 && K <= 4096 && lda % 4 == 0 && ldw % 4 == 0 && aligned16(A) &&
           aligned16(W);
}
static int skinny_tall_launch(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
                              const float* bias, float* out, int64_t ldo, hipStream_t stream, float* parts = nullptr) {
    TallArgs a;
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.parts = parts; a.lda = lda; a.ldw = ldw; a.ldo = ldo;
    a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.RT = (int)cdiv64(M, 32);
    a.KS = a.RT <= 2 ? 4 : (a.RT <= 4 ? 2 : 1);     // k range per wave and chunk: a multiple of 64 (K % 256 == 0, skinny_tall_ok)
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return VAG_EINVAL;
    if (!(done.load(std::memory_order_acquire) & (1ull << dev))) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(skinny_tall_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                TALL_LDS_BYTES) != hipSuccess) return VAG_EINVAL;
        done.fetch_or(1ull << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL(skinny_tall_kernel, dim3((unsigned)cdiv64(N, 64)), dim3(512), TALL_LDS_BYTES, stream, a);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// The vocabulary product of a decoding step with the pieces of every row's log-sum-exp (TallArgs::parts): number of pieces per
// row (= workgroups), or 0 when the tall-skinny kernel does not take the shape (the caller then normalises with lse_nll_kernel).
int64_t vag_logits_parts_count(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw) {
    return vag_opt().gemm_f32mfma == 0 && skinny_tall_ok(M, N, K, A, lda, W, ldw) ? cdiv64(N, 64) : 0;
}
int vag_logits_parts_launch(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
                            const float* bias, float* out, int64_t ldo, float* parts, hipStream_t stream) {
    VAG_CHECK_ARG(A && W && out && parts && vag_logits_parts_count(M, N, K, A, lda, W, ldw) > 0);
    return skinny_tall_launch(M, N, K, A, lda, W, ldw, bias, out, ldo, stream, parts);
}

int vag_skinny_launch(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
                      const float* bias, const float* addend, int64_t ldadd, float* out, int64_t ldo, int act,
                      hipStream_t stream, bool w16) {
    VAG_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && A && W && out);
    if (M == 0 || N == 0) return VAG_OK;
    if (w16) {      // W stored as fp16: skinny kernels only (the per-time-step products of the 2-byte storage mode)
        VAG_CHECK_ARG(M <= 256 && K % 8 == 0 && lda % 4 == 0 && ldw % 8 == 0 && aligned16(A) && aligned16(W));
        SkinnyArgs a;
        a.A = A; a.W = W; a.lda = lda; a.ldw = ldw; a.M = (int)M; a.N = (int)N; a.K = (int)K;
        a.bias = bias; a.addend = addend; a.ldadd = ldadd; a.out = out; a.ldo = ldo; a.act = act;
        skinny_plain_go(a, stream, true);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    // vocabulary-sized products of one decoding / free-running step: the tall-skinny bf16x6 kernel above
    if (!addend && act == 0 && vag_opt().gemm_f32mfma == 0 && skinny_tall_ok(M, N, K, A, lda, W, ldw))
        return skinny_tall_launch(M, N, K, A, lda, W, ldw, bias, out, ldo, stream);
    // every 16x16 output tile re-reads its operand rows: M*N*K/2 bytes requested in all.  Measured at the beam-decode
    // shape (B*k = 192 rows): the 192x2560x512 query/gate product (126 MB) is still faster here (5 vs 16 us), the
    // 192x9391x256 vocabulary product (230 MB) is faster on the LDS-tiled kernel (19 vs 38 us).
    if (!skinny_ok(A, lda, W, ldw, K) || M > 256 || (M > 64 && (double)M * (double)N * (double)K > 350e6)) {
        // generic path through the tiled kernel; an addend is folded in with beta = 1
        if (addend) {
            if (addend != out) VAG_TRY(vag_copy2d_launch(addend, ldadd, out, ldo, M, N, stream));
            return vag_gemm_launch(M, N, K, 1.f, A, lda, 1, W, 1, ldw, 1.f, out, ldo, bias, act, stream);
        }
        return vag_gemm_launch(M, N, K, 1.f, A, lda, 1, W, 1, ldw, 0.f, out, ldo, bias, act, stream);
    }
    SkinnyArgs a;
    a.A = A; a.W = W; a.lda = lda; a.ldw = ldw; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.bias = bias; a.addend = addend; a.ldadd = ldadd; a.out = out; a.ldo = ldo; a.act = act;
    // Tile choice, from measurements (tools/exp_tiles.py, tools/skinny_probe.hip): these launches are bound by the bytes
    // REQUESTED chip-wide (L2 is dropped at every kernel boundary; ~6.3 TB/s aggregate, ~50 GB/s per CU), duplicates
    // included, so wider/taller tiles or half tiles do not pay at M <= 128; 16x16 with K split over the waves it is.
    skinny_plain_go(a, stream);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_axpy_launch(float a, const float* x, float* y, int64_t n, int accumulate, hipStream_t s);      // elem.hip
static int vag_axpy2d_launch(float a, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t cols, int accumulate, hipStream_t s) {
    if (ldx == cols && ldy == cols) return vag_axpy_launch(a, x, y, rows * cols, accumulate, s);
    for (int64_t r = 0; r < rows; ++r) VAG_TRY(vag_axpy_launch(a, x + r * ldx, y + r * ldy, cols, accumulate, s));     // (not a shape of this library)
    return VAG_OK;
}

// C (M,N) = beta C + A (M,K) B (K,N), B row-major with row stride ldb; M <= 128 (skinny path), else the tiled kernels.
// out2 (optional): a second destination, out2 (M,N) (+)= scale2 * (A B) -- an axpy launch saved (the initial state's backward:
// d_ctx += split * dx beside dx itself), whatever path the product takes.
int vag_skinny_nn_launch(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                         float beta, float* C, int64_t ldc, hipStream_t stream, float* out2, int64_t ldo2, float scale2, int acc2) {
    VAG_CHECK_ARG(M >= 0 && N >= 0 && K > 0 && A && B && C && (beta == 0.f || beta == 1.f));
    if (M == 0 || N == 0) return VAG_OK;
    if (M > 128 || !aligned16(A) || lda % 4 != 0 || K % 4 != 0 || (double)M * (double)N * (double)K > 350e6) {
        VAG_TRY(vag_gemm_launch(M, N, K, 1.f, A, lda, 1, B, ldb, 1, beta, C, ldc, nullptr, VAG_ACT_NONE, stream));
        if (out2) return vag_axpy2d_launch(scale2, C, ldc, out2, ldo2, M, N, acc2, stream);
        return VAG_OK;
    }
    SkinnyArgs a;
    a.out2 = out2; a.ldo2 = ldo2; a.scale2 = scale2; a.acc2 = acc2;
    a.A = A; a.W = B; a.lda = lda; a.ldw = ldb; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.bias = nullptr; a.addend = beta != 0.f ? C : nullptr; a.ldadd = ldc; a.out = C; a.ldo = ldc; a.act = VAG_ACT_NONE;
    dim3 grid((unsigned)cdiv64(N, 16), (unsigned)cdiv64(M, 16), 1);
    if (K <= 256) hipLaunchKernelGGL((skinny_bt_kernel<4>), grid, dim3(256), 0, stream, a);
    else if (K <= 1024) hipLaunchKernelGGL((skinny_bt_kernel<8>), grid, dim3(512), 0, stream, a);
    else hipLaunchKernelGGL((skinny_bt_kernel<16>), grid, dim3(1024), 0, stream, a);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// nb independent products out_z (M,N) = A_z (M,K) W_z^T, operands and outputs at fixed element strides (one launch)
int vag_skinny_batched_launch(int64_t nb, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, int64_t bsA,
                              const float* W, int64_t ldw, int64_t bsW, float* out, int64_t ldo, int64_t bsO,
                              hipStream_t stream) {
    VAG_CHECK_ARG(nb > 0 && nb < 65536 && M > 0 && N > 0 && K > 0 && A && W && out && skinny_ok(A, lda, W, ldw, K));
    VAG_CHECK_ARG(bsA % 4 == 0 && bsW % 4 == 0);
    SkinnyArgs a;
    a.A = A; a.W = W; a.lda = lda; a.ldw = ldw; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.bias = nullptr; a.addend = nullptr; a.ldadd = 0; a.out = out; a.ldo = ldo; a.act = VAG_ACT_NONE;
    a.bsA = bsA; a.bsW = bsW; a.bsO = bsO;
    dim3 grid((unsigned)cdiv64(N, 16), (unsigned)cdiv64(M, 16), (unsigned)nb);
    if (K <= 256) hipLaunchKernelGGL((skinny_plain_kernel<4>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((skinny_plain_kernel<8>), grid, dim3(512), 0, stream, a);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_gru_step_launch(const GruStepArgs& a, int nz, hipStream_t stream, bool w16) {
    VAG_CHECK_ARG(a.H > 0 && a.M > 0 && a.K > 0 && (nz == 1 || nz == 2));
    for (int z = 0; z < nz; ++z) {
        VAG_CHECK_ARG(a.s[z].A && a.s[z].W && a.s[z].other && a.s[z].hprev && a.s[z].hout);
        VAG_CHECK_ARG(skinny_ok(a.s[z].A, a.lda, a.s[z].W, a.ldw, a.K));
    }
    VAG_CHECK_ARG(!w16 || (a.K % 8 == 0 && a.ldw % 8 == 0));
    // tile choice from measurements (tools/exp_tiles.py, tools/skinny_probe.hip): 16 units x 16 rows; half tiles on
    // twice the CUs were no faster (the launch is paced by load requests issued chip-wide, duplicates included).
    dim3 grid((unsigned)cdiv64(a.H, 16), (unsigned)cdiv64(a.M, 16), (unsigned)nz);
    const int64_t wgs = (int64_t)grid.x * grid.y * grid.z;
    constexpr int64_t maxwg = 160;
    if (a.K > 256 && wgs <= maxwg) {
        // fewer than ~2/3 of the CUs would get a workgroup: 8 units each on twice the workgroups
        const dim3 g8((unsigned)cdiv64(a.H, 8), grid.y, grid.z);
        if (w16) hipLaunchKernelGGL((gru_step_small_kernel<8, 8, true>), g8, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((gru_step_small_kernel<8, 8>), g8, dim3(512), 0, stream, a);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    // wide batches: two row tiles per workgroup (half the W re-reads) as long as >= 192 workgroups remain (beam decoding has 192 rows)
    if (a.M >= 128 && a.K > 256 && (int64_t)grid.x * cdiv64(a.M, 32) * nz >= 192) {
        const dim3 gw(grid.x, (unsigned)cdiv64(a.M, 32), grid.z);
        if (w16) hipLaunchKernelGGL((gru_step_kernel<8, true, 2>), gw, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((gru_step_kernel<8, false, 2>), gw, dim3(512), 0, stream, a);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    if (w16) {
        if (a.K <= 256) hipLaunchKernelGGL((gru_step_kernel<4, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((gru_step_kernel<8, true>), grid, dim3(512), 0, stream, a);
    } else {
        if (a.K <= 256) hipLaunchKernelGGL((gru_step_kernel<4>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((gru_step_kernel<8>), grid, dim3(512), 0, stream, a);
    }
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

int vag_gru_bwd_step_launch(const GruBwdStepArgs& a, int nz, hipStream_t stream, bool w16) {
    VAG_CHECK_ARG(a.H > 0 && a.M > 0 && a.K > 0 && (nz == 1 || nz == 2));
    for (int z = 0; z < nz; ++z) {
        VAG_CHECK_ARG(a.s[z].A && a.s[z].WT && skinny_ok(a.s[z].A, a.lda, a.s[z].WT, a.ldw, a.K));
        if (a.has_cell) VAG_CHECK_ARG(a.s[z].save && a.s[z].hprev && a.s[z].dgi && a.s[z].dgh && a.s[z].dh_direct);
        else VAG_CHECK_ARG(a.s[z].dh_out != nullptr);
    }
    VAG_CHECK_ARG(!w16 || (a.K % 8 == 0 && a.ldw % 8 == 0));
    // wide shapes (M >= 128 rows and still >= 256 workgroups): 2 x 2 tiles per workgroup halve the operand re-reads
    if (a.M >= 128 && a.K > 1024 && cdiv64(a.H, 32) * cdiv64(a.M, 32) * nz >= 256) {
        dim3 gw((unsigned)cdiv64(a.H, 32), (unsigned)cdiv64(a.M, 32), (unsigned)nz);
        if (w16) hipLaunchKernelGGL((gru_bwd_step_kernel<16, 4, true, 2, 2>), gw, dim3(1024), 0, stream, a);
        else hipLaunchKernelGGL((gru_bwd_step_kernel<16, 2, false, 2, 2>), gw, dim3(1024), 0, stream, a);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    dim3 grid((unsigned)cdiv64(a.H, 16), (unsigned)cdiv64(a.M, 16), (unsigned)nz);
    // waves by K; chunks in flight so that a wave's K share (K / waves, in 16s) is one round of requests when it fits
#define VAG_BWD_GO(WH)                                                                                                \
    if (a.K <= 256) hipLaunchKernelGGL((gru_bwd_step_kernel<4, 4, WH>), grid, dim3(256), 0, stream, a);               \
    else if (a.K <= 512) hipLaunchKernelGGL((gru_bwd_step_kernel<8, 4, WH>), grid, dim3(512), 0, stream, a);          \
    else if (a.K <= 1024) hipLaunchKernelGGL((gru_bwd_step_kernel<8, 8, WH>), grid, dim3(512), 0, stream, a);         \
    else if (a.K <= 1536) hipLaunchKernelGGL((gru_bwd_step_kernel<16, 6, WH>), grid, dim3(1024), 0, stream, a);       \
    else hipLaunchKernelGGL((gru_bwd_step_kernel<16, 4, WH>), grid, dim3(1024), 0, stream, a);
    if (w16) { VAG_BWD_GO(true) } else { VAG_BWD_GO(false) }
#undef VAG_BWD_GO
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

