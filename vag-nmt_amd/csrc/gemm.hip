// Dense fp32 products C = alpha A B (+ beta C, bias, tanh) for gfx950 through LDS-staged block tiles, and the host layer that plans
// and launches them.  (Products with few rows -- a recurrence step, a beam -- are skinny.hip.)
//
// Kernels
//  * gemm_tiled_kernel        exact f32-input MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 (4 waves) or 128 x 128 (8 waves) tiles,
//                             double-buffered LDS; gemm_tiled_multi_kernel: several small weight-gradient products in one grid
//  * gemm_split_kernel        fp32 operands split into 3 / 2 / 1 bf16 planes (or one fp16 plane) on their way into LDS, bf16 MFMA,
//                             128 x 128 tiles; row sums of A and split-K through slabs on the three-plane form; _group_: several
//                             products of one operand layout in one grid
//  * gemm_big_kernel          one plane, 256 x 256 tiles (the 2-byte storage mode's large products); _group_ likewise
//  * fill2d, colsum, colsum_multi, transpose
// Host layer, in file order
//  * gemm_kernel_for / gemm_group_kernel_for   plan -> kernel: the one list of template instantiations
//  * gemm_plan_single                          pure planner of one product (vag_gemm_plan is its host-only ABI view);
//    group_plan                                split-K and block order of a grouped launch (vag_gemm_group_plan)
//  * gemm_prepare_output                       slabs / prezeroed mark / fill, for single products and group members alike
//  * gemm_launch_single                        one planned product: row-sum fallback, output preparation, kernel
//  * GemmQueues                                the calling thread's group bracket, leaf list and column-sum queue
//  * vag_gemm_launch, vag_gemm_launch_planes, vag_colsum*_launch, vag_transpose_launch
#include "gemm_shared.h"
#include "call_ctx.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// tiled GEMM
// ------------------------------------------------------------------------------------------------
// Load a (BT outer) x (BK k) operand tile into registers.  KC: k is the contiguous dimension.  NTH threads.
template <int BT, bool KC, bool VEC, int NTH>
__device__ __forceinline__ void tile_load(const float* __restrict__ P, int64_t so, int64_t sk, int o0, int k0,
                                          int OUT, int KEND, float4 (&r)[BT * (BK / 4) / NTH]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < BT * (BK / 4) / NTH; ++i) {
        const int idx = tid + i * NTH;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KC) {
            const int o = o0 + idx / (BK / 4), k = k0 + ((idx % (BK / 4)) << 2);
            if (o < OUT) {
                const float* p = P + (int64_t)o * so + k;
                if (VEC && k + 3 < KEND) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (k + 0 < KEND) v.x = p[0];
                    if (k + 1 < KEND) v.y = p[1];
                    if (k + 2 < KEND) v.z = p[2];
                    if (k + 3 < KEND) v.w = p[3];
                }
            }
        } else {
            const int k = k0 + idx / (BT / 4), o = o0 + ((idx % (BT / 4)) << 2);
            if (k < KEND) {
                const float* p = P + (int64_t)k * sk + o;
                if (VEC && o + 3 < OUT) {
                    v = *reinterpret_cast<const float4*>(p);
                } else {
                    if (o + 0 < OUT) v.x = p[0];
                    if (o + 1 < OUT) v.y = p[1];
                    if (o + 2 < OUT) v.z = p[2];
                    if (o + 3 < OUT) v.w = p[3];
                }
            }
        }
        r[i] = v;
    }
}

// LDS image: S[k][o], row stride BT+4 floats (MFMA operand reads are 32 consecutive floats -> conflict free).
template <int BT, bool KC, int NTH>
__device__ __forceinline__ void tile_store(float* __restrict__ S, const float4 (&r)[BT * (BK / 4) / NTH]) {
    const int tid = threadIdx.x;
    constexpr int LD = BT + 4;
#pragma unroll
    for (int i = 0; i < BT * (BK / 4) / NTH; ++i) {
        const int idx = tid + i * NTH;
        if (KC) {
            const int o = idx / (BK / 4), k = (idx % (BK / 4)) << 2;
            S[(k + 0) * LD + o] = r[i].x;
            S[(k + 1) * LD + o] = r[i].y;
            S[(k + 2) * LD + o] = r[i].z;
            S[(k + 3) * LD + o] = r[i].w;
        } else {
            const int k = idx / (BT / 4), o = (idx % (BT / 4)) << 2;
            *reinterpret_cast<float4*>(&S[k * LD + o]) = r[i];
        }
    }
}

// NTH = 256: 4 waves as 2x2, each (BM/2)x(BN/2).  NTH = 512: 8 waves as 2x4, each (BM/2)x(BN/4): two waves per SIMD,
// so one workgroup alone on a CU (the usual case for this model's mid-size products) still overlaps LDS reads with MFMAs.
template <int BM, int BN, bool AKC, bool BKC, bool VEC, int NTH>
__device__ __forceinline__ void gemm_tiled_body(const GemmArgs& a, float* smem, int bx, int by, int bz) {
    constexpr int WN = NTH / 128;                 // waves along N
    constexpr int TM = BM / 64, TN = BN / (32 * WN);
    constexpr int LDA = BM + 4, LDB = BN + 4;
    float* As = smem;
    float* Bs = smem + 2 * BK * LDA;

    const int m0 = by * BM, n0 = bx * BN;
    const int kbeg = bz * a.kchunk;
    const int kend = min(a.K, kbeg + a.kchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[BM * (BK / 4) / NTH], rb[BN * (BK / 4) / NTH];
    tile_load<BM, AKC, VEC, NTH>(a.A, a.sa_o, a.sa_k, m0, kbeg, a.M, kend, ra);
    tile_load<BN, BKC, VEC, NTH>(a.B, a.sb_o, a.sb_k, n0, kbeg, a.N, kend, rb);
    tile_store<BM, AKC, NTH>(As, ra);
    tile_store<BN, BKC, NTH>(Bs, rb);
    __syncthreads();

    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        const bool more = (k0 + BK) < kend;
        if (more) {
            tile_load<BM, AKC, VEC, NTH>(a.A, a.sa_o, a.sa_k, m0, k0 + BK, a.M, kend, ra);
            tile_load<BN, BKC, VEC, NTH>(a.B, a.sb_o, a.sb_k, n0, k0 + BK, a.N, kend, rb);
        }
        const float* Ac = As + cur * BK * LDA + wm * (BM / 2) + (lane & 31);
        const float* Bc = Bs + cur * BK * LDB + wn * (BN / WN) + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const int kr = kk + (lane >> 5);
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = Ac[kr * LDA + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bc[kr * LDB + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            tile_store<BM, AKC, NTH>(As + (cur ^ 1) * BK * LDA, ra);
            tile_store<BN, BKC, NTH>(Bs + (cur ^ 1) * BK * LDB, rb);
        }
        __syncthreads();
        cur ^= 1;
    }

    // epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    const bool atomic = a.splitk > 1;
    const bool first = bz == 0;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
            if (col >= a.N) continue;
            const float bv = (a.bias && first) ? a.bias[col] : 0.f;
            const int row0 = m0 + wm * (BM / 2) + i * 32 + 4 * (lane >> 5);
            float* cbase = a.C + (int64_t)row0 * a.ldc + col;
            if (a.c_half) gemm_epilogue16(acc[i][j], a.C, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, false, 1, (int64_t)row0 * a.ldc + col);
            else gemm_epilogue16(acc[i][j], cbase, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, atomic);
        }
}
template <int BM, int BN, bool AKC, bool BKC, bool VEC, int NTH>
__global__ __launch_bounds__(NTH) void gemm_tiled_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (BM + 4) + 2 * BK * (BN + 4)];
    gemm_tiled_body<BM, BN, AKC, BKC, VEC, NTH>(a, smem, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Several small weight-gradient products g_W += dY^T X of ONE launch (the leaf queue below): 64 x 64 tiles of the exact f32 kernel,
// both operands outer-contiguous, tiles of all tasks numbered through (tile0[k] = first tile of task k).  A task's optional
// rowsum (the bias gradient sum_r dY[r,:] that goes with it) is taken by the task's first column of tiles straight from memory.
constexpr int LEAF_MAX = 8;
struct LeafTasks {
    GemmArgs g[LEAF_MAX];
    int tile0[LEAF_MAX + 1];
    int tiles_x[LEAF_MAX];
    int n;
};
__global__ __launch_bounds__(256) void gemm_tiled_multi_kernel(LeafTasks T) {
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * 68 + 2 * BK * 68];
    int k = 0;
    while (k + 1 < T.n && (int)blockIdx.x >= T.tile0[k + 1]) ++k;
    const int t = blockIdx.x - T.tile0[k];
    const GemmArgs& a = T.g[k];
    const int bx = t % T.tiles_x[k], by = t / T.tiles_x[k];
    if (a.rowsum && bx == 0 && threadIdx.x < 64) {
        const int m = by * 64 + threadIdx.x;
        if (m < a.M) {
            float s0 = 0.f, s1 = 0.f;
            int r = 0;
            for (; r + 1 < a.K; r += 2) { s0 += a.A[(int64_t)r * a.sa_k + m]; s1 += a.A[(int64_t)(r + 1) * a.sa_k + m]; }
            if (r < a.K) s0 += a.A[(int64_t)r * a.sa_k + m];
            a.rowsum[m] += s0 + s1;
        }
    }
    gemm_tiled_body<64, 64, false, false, true, 256>(a, smem, bx, by, 0);
}

// ------------------------------------------------------------------------------------------------
// fp32 GEMM on the bf16 matrix pipes: 3-way operand split, 6 products ("bf16x6")
//
// gfx950's f32-input MFMA runs at 1/16 of the bf16 MFMA rate.  Every fp32 value is the exact sum of three bf16 numbers
// x = x1 + x2 + x3 (8 significand bits each: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); the residual is
// below 2^-24 |x|), so a*b = sum_{i+j<=4} a_i b_j up to 2^-24 relative: the six bf16 x bf16 products are exact in fp32
// and are accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  That is fp32-grade arithmetic (same error class as a
// reassociated fp32 sum) at 6/16 of the f32-MFMA instruction time.  The split is done once per element on its way from
// global memory into LDS (three bf16 planes per operand), so global traffic is unchanged.
// Block 128x128x32, 8 waves (2x4, 64x32 each), LDS single-staged (61 KB: two blocks per CU), register prefetch.
// ------------------------------------------------------------------------------------------------
// (operand loaders, the split + LDS store and the fragment reads / MFMA step live in gemm_shared.h)
template <bool AKC, bool BKC, bool VEC, int PL = 3, bool F16 = false, bool ABF = false>
__device__ __forceinline__ void gemm_split_body(const GemmArgs& a, __bf16* smem, int bx, int by, int bz) {
    __bf16* As = smem;
    __bf16* Bs = smem + PL * SP_PLANE;
    const int m0 = by * 128, n0 = bx * 128;
    const int kbeg = bz * a.kchunk;
    const int kend = min(a.K, kbeg + a.kchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 2, wn = wave & 3;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    // fragment addresses: lane (r = lane&31, h = lane>>5) holds 8 consecutive k (8h..8h+7) of row r
    const __bf16* Af = As + (wm * 64 + (lane & 31)) * SP_LD + 8 * (lane >> 5);
    const __bf16* Bf = Bs + (wn * 32 + (lane & 31)) * SP_LD + 8 * (lane >> 5);

    SpRegs ra, rb;
    // full k-tiles through the precomputed-offset loads (sp_fast_*), a last partial one (and unaligned operands) through sp_load
    constexpr bool FAST = VEC && !ABF;
    const int nt = (kend - kbeg + SP_BK - 1) / SP_BK;
    const int nfull = FAST ? (kend - kbeg) / SP_BK : 0;
    SpFast<AKC> fa;
    SpFast<BKC> fb;
    if (FAST) {
        sp_fast_init<AKC>(fa, a.A, a.sa_o, a.sa_k, m0, kbeg, a.M);
        sp_fast_init<BKC>(fb, a.B, a.sb_o, a.sb_k, n0, kbeg, a.N);
    }
    auto load_tile = [&](int t) {
        if (FAST && t < nfull) {
            sp_fast_load<AKC>(fa, ra);
            sp_fast_load<BKC>(fb, rb);
        } else {
            const int k0 = kbeg + t * SP_BK;
            if (ABF) sp_load_bf16<AKC>(reinterpret_cast<const unsigned short*>(a.A), a.sa_o, a.sa_k, m0, k0, a.M, kend, ra);
            else sp_load<AKC, VEC>(a.A, a.sa_o, a.sa_k, m0, k0, a.M, kend, ra);
            sp_load<BKC, VEC>(a.B, a.sb_o, a.sb_k, n0, k0, a.N, kend, rb);
        }
    };
    load_tile(0);
    // row sums of A for the first column tile's blocks (outer-contiguous A: this thread's two items of a k-tile are the same
    // four rows m at two k): the bias gradient of a weight-gradient product without a second pass over dY
    // (three-plane kernels only: at the one-plane kernels' 80-VGPR cap the extra state spills; the launcher sends those
    // products' row sums to a column-sum launch instead)
    const bool do_rs = !AKC && PL == 3 && a.rowsum != nullptr && bx == 0;
    float4 rs = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < nt; ++t) {
        if (!AKC && PL == 3 && do_rs) {
            rs.x += ra.v[0] + ra.v[4]; rs.y += ra.v[1] + ra.v[5]; rs.z += ra.v[2] + ra.v[6]; rs.w += ra.v[3] + ra.v[7];
        }
        sp_store<AKC, PL, F16, ABF>(As, ra);
        sp_store<BKC, PL, F16>(Bs, rb);
        __syncthreads();
        if (t + 1 < nt) load_tile(t + 1);
        sp_compute<PL, AKC, BKC, F16>(Af, Bf, As, Bs, wm * 64, wn * 32, acc);
        __syncthreads();
    }
    if (!AKC && PL == 3 && do_rs) {           // (uniform over the block) 16 threads hold partial sums of the same four rows: meet in LDS
        float4* rs_s = reinterpret_cast<float4*>(smem);
        rs_s[threadIdx.x] = rs;
        __syncthreads();
        if (threadIdx.x < 32) {
            float4 t = rs_s[threadIdx.x];
#pragma unroll
            for (int q = 1; q < 16; ++q) {
                const float4 o = rs_s[threadIdx.x + 32 * q];
                t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
            }
            const int m = m0 + 4 * threadIdx.x;
            if (m + 0 < a.M) atomicAdd(a.rowsum + m + 0, t.x);
            if (m + 1 < a.M) atomicAdd(a.rowsum + m + 1, t.y);
            if (m + 2 < a.M) atomicAdd(a.rowsum + m + 2, t.z);
            if (m + 3 < a.M) atomicAdd(a.rowsum + m + 3, t.w);
        }
    }

    // epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    bool atomic = a.splitk > 1;
    bool first = bz == 0;
    if (PL == 3 && !F16 && !ABF && a.slab != nullptr && a.nslices > 1) {      // (three-plane kernels only: the one-plane ones sit at an 80-register cap)
        // ---- split-K through slabs (GemmArgs::slab).  Atomics execute at the memory side at ~1.3 TB/s chip-wide (MI355X_MICROARCH.md,
        // global float atomics): a 2560 x 512 output in six slices is 31 MB of them, 24 us -- more than the slices' MFMA work -- and
        // they arrive in one burst when the launch is a single round of blocks.  Here a slice stores its 128 x 128 accumulators as they
        // lie in the registers (16 bytes per lane and store, write-through), drains, and one lane takes the tile's ticket; whoever
        // draws the last ticket loads ALL slabs of the tile in slice order (its own included: the sum then does not depend on who was
        // last -- bitwise reproducible, unlike the atomics) and finishes the tile alone.  Hand-off as persist.hip's (sc1 stores,
        // vmcnt(0), barrier, one agent-scope add whose RETURN value names the last arriver, sc1 loads): no fences, and no block
        // ever waits for another, so the scheme holds whatever part of the grid is resident.
        const int tile = by * ((a.N + 127) >> 7) + bx;
        float4* mine = reinterpret_cast<float4*>(a.slab) + ((int64_t)tile * a.nslices + bz) * 4096 + (wave * 8) * 64 + lane;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]};
                // (s_nop: a store of more than 64 bits must not be followed at once by a write of its data registers -- the compiler
                // knows that hazard for its own stores, not for inline asm)
                asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(mine + (i * 4 + q) * 64), "v"(v) : "memory");
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                          // (also: every wave is done with the LDS planes)
        int* flag = reinterpret_cast<int*>(smem);
        if (threadIdx.x == 0) {
            const unsigned t = __hip_atomic_fetch_add(a.ticket + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = t == (unsigned)(a.nslices - 1);
            if (last) __hip_atomic_store(a.ticket + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
            flag[0] = last ? 1 : 0;
        }
        __syncthreads();
        if (flag[0] == 0) return;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        const float4* all = reinterpret_cast<const float4*>(a.slab) + (int64_t)tile * a.nslices * 4096 + (wave * 8) * 64 + lane;
        // (One slice per round trip.  Two in flight -- loads of slice z + 1 issued before slice z is waited for -- was tried: at the
        // kernels' 128-register cap the second buffer spills, scratch traffic then counts in vmcnt and the compiler saves load
        // targets before their data has arrived: wrong sums.  The tail this leaves is nslices x ~1.5 us on the last block of a tile.)
        for (int z = 0; z < a.nslices; ++z) {
            f32x4 v[8];
            const float4* p = all + (int64_t)z * 4096;
            asm volatile("global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %8, off offset:1024 sc1\n\t"
                         "global_load_dwordx4 %2, %8, off offset:2048 sc1\n\tglobal_load_dwordx4 %3, %8, off offset:3072 sc1\n\t"
                         "global_load_dwordx4 %4, %9, off sc1\n\tglobal_load_dwordx4 %5, %9, off offset:1024 sc1\n\t"
                         "global_load_dwordx4 %6, %9, off offset:2048 sc1\n\tglobal_load_dwordx4 %7, %9, off offset:3072 sc1\n\t"
                         "s_waitcnt vmcnt(0)"
                         : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                         : "v"(p), "v"(p + 256) : "memory");
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][4 * q + e] += v[i * 4 + q][e];
        }
        // an accumulating product still ADDS its one result atomically.  (A plain read-modify-write where no other product of the
        // launch targets the same C was measured: +11 us per step -- the block then waits for sixteen loads per lane before it can
        // store, while the atomics are fire-and-forget and overlap the next blocks' work.)
        atomic = a.beta != 0.f;
        first = true;                      // (the bias rides with the one epilogue)
    }
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= a.N) return;
    const float bv = (a.bias && first) ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row0 = m0 + wm * 64 + i * 32 + 4 * (lane >> 5);
        if (a.c_half) gemm_epilogue16(acc[i], a.C, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, atomic, 1, (int64_t)row0 * a.ldc + col);
        else gemm_epilogue16(acc[i], a.C + (int64_t)row0 * a.ldc + col, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, atomic);
    }
}

// (Round 3, measured and dropped: an XCD-contiguous, panel-ordered block -> tile mapping (T1 + 8-column panels).  Single
// products: no change on hot operands (4096^3 NT 705 -> 710 us); grouped launches: SLOWER in the step (weight-gradient group
// 150 -> 174 us, logits/keys group 67 -> 86 us) because an XCD then works through one product's blocks and the products'
// K differ by 10x -- the round-robin dealing of blocks over the XCDs is what balances a group.)
// Waves per SIMD asked of the compiler: 4 (two 8-wave blocks per CU: <= 128 VGPRs -- without the bound the forward group kernel
// took 134 and two single-product layouts 130, i.e. ONE block per CU), 6 for the one-plane kernels of the 2-byte mode (20 KB of
// LDS: three blocks per CU at <= 80 VGPRs, a few spills; configs[4] 33.3 -> 32.8 ms; 8 spills everything: 122 ms).
template <bool AKC, bool BKC, bool VEC, int PL = 3, bool F16 = false, bool ABF = false>
__global__ __launch_bounds__(512, PL == 1 ? 6 : 4) void gemm_split_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * PL * SP_PLANE];      // 60 / 40 / 20 KB
    gemm_split_body<AKC, BKC, VEC, PL, F16, ABF>(a, smem, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Grouped launch: the blocks of up to GROUP_MAX independent products of one operand layout (e.g. all "TN": both operands
// outer-contiguous, the weight gradients g_W += dY^T X of one operator) in ONE grid.  Each of these products alone is a few dozen 128x128 tiles
// with K = Tt*B: launched one by one they need split-K by 5-10 (atomics) to fill the chip and still pay a ramp and a
// partial last wave each; together they fill it with split-K 1-2.
template <bool AKC, bool BKC, int PL = 3, bool F16 = false>
__global__ __launch_bounds__(512, PL == 1 ? 6 : 4) void gemm_split_group_kernel(GemmGroupArgs G) {
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * PL * SP_PLANE];
    int p = 0;
    while (p + 1 < G.n && (int)blockIdx.x >= G.start[p + 1]) ++p;
    const GemmArgs& a = G.p[p];
    const int id = blockIdx.x - G.start[p];
    const int tn = (a.N + 127) / 128, tm = (a.M + 127) / 128;
    const int bx = id % tn, by = (id / tn) % tm, bz = id / (tn * tm);
    gemm_split_body<AKC, BKC, true, PL, F16>(a, smem, bx, by, bz);
}

// ---- round 4: 256 x 256 block tile for the ONE-plane products of the 2-byte storage mode (configs[4]) ----------------------
// With one plane per operand a 128 x 128 x 32 k-tile is 8 MFMAs per wave (256 matrix-pipe cycles per SIMD and block) behind 32 KB of
// fp32 operands: at the ~70 GB/s a CU draws from its L2 that is 0.46 us of ingest per 0.11 us of MFMA work -- the kernel above runs at
// 280-560 TF/s on configs[4]'s shapes (11-22 % of the bf16 peak; tools/exp_gemm_oneplane.py), bound by operand BYTES, as DESIGN
// section 9 already said of the large products in that mode.  A 256 x 256 tile does four times the MFMA work per k-tile on twice
// the bytes.  Eight waves (2 x 4, 128 x 64 outputs each: 8 accumulators), operands still fp32 in memory and rounded on their way
// into LDS (sp_load / sp_store, one plane; an operand's 256 rows are two of the 128-row images), two LDS stages of 40 KB, the loads of
// k-tile t + 2 and the store of t + 1 issued around the MFMAs of t, ONE barrier per k-tile.
constexpr int BIG_STAGE = 4 * SP_PLANE;                 // bf16 elements per stage: A halves 0,1 then B halves 0,1 (4 x 10 KB)
constexpr int BIG_LDS_BYTES = 2 * BIG_STAGE * 2;        // 81920
__device__ __forceinline__ void big_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <bool AKC, bool BKC, bool F16, bool ABF>
__device__ __forceinline__ void gemm_big_body(const GemmArgs& a, __bf16* smem, int bx, int by, int bz) {
    const int m0 = by * 256, n0 = bx * 256;
    const int kbeg = bz * a.kchunk;
    const int kend = min(a.K, kbeg + a.kchunk);
    const int nt = (kend - kbeg + SP_BK - 1) / SP_BK;
    const int nfull = (kend - kbeg) / SP_BK;               // full k-tiles: precomputed-offset loads (a bf16-stored A keeps its own loader)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 2, wn = wave & 3;               // rows wm * 128 .. +128 (= A half wm), columns wn * 64 .. +64 (B half wn >> 1)
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // fragment bases inside a stage (k-contiguous operands) / first outer index inside the half (outer-contiguous ones)
    const int foff_a = wm * SP_PLANE + (lane & 31) * SP_LD + 8 * (lane >> 5);
    const int foff_b = (2 + (wn >> 1)) * SP_PLANE + ((wn & 1) * 64 + (lane & 31)) * SP_LD + 8 * (lane >> 5);
    SpRegs ra[2], rb[2];                                   // halves of the k-tile in flight
    SpFast<AKC> fa[2];
    SpFastH<AKC> fah[2];
    SpFast<BKC> fb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // a half that lies entirely outside the operand is clamped onto its last valid row / group like any other out-of-range row
        if (!ABF) sp_fast_init<AKC>(fa[h], a.A, a.sa_o, a.sa_k, min(m0 + 128 * h, AKC ? a.M - 1 : ((a.M - 1) & ~3)), kbeg, a.M);
        else sp_fast_init_bf16<AKC>(fah[h], reinterpret_cast<const unsigned short*>(a.A), a.sa_o, a.sa_k,
                                    min(m0 + 128 * h, AKC ? a.M - 1 : ((a.M - 1) & ~3)), kbeg, a.M);
        sp_fast_init<BKC>(fb[h], a.B, a.sb_o, a.sb_k, min(n0 + 128 * h, BKC ? a.N - 1 : ((a.N - 1) & ~3)), kbeg, a.N);
    }
    auto load_tile = [&](int t) {
        const int k0 = kbeg + t * SP_BK;
        if (t < nfull) {            // ONE branch around all of a k-tile's loads: a select per load makes hipcc wait for each load in turn
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (ABF) sp_fast_load_bf16<AKC>(fah[h], ra[h]);
                else sp_fast_load<AKC>(fa[h], ra[h]);
                sp_fast_load<BKC>(fb[h], rb[h]);
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (ABF) sp_load_bf16<AKC>(reinterpret_cast<const unsigned short*>(a.A), a.sa_o, a.sa_k, m0 + 128 * h, k0, a.M, kend, ra[h]);
                else sp_load<AKC, true>(a.A, a.sa_o, a.sa_k, m0 + 128 * h, k0, a.M, kend, ra[h]);
                sp_load<BKC, true>(a.B, a.sb_o, a.sb_k, n0 + 128 * h, k0, a.N, kend, rb[h]);
            }
        }
    };
    // row sums of an outer-contiguous fp32 A (the bias gradient of a weight-gradient product g_W += dY^T X), taken from the tiles on
    // their way into LDS by the first column of blocks, as the 128 x 128 three-plane kernel does (round 6: the 2-byte mode's products
    // ran a separate column-sum pass over dY for them, 0.45 ms per step at configs[4])
    const bool do_rs = !AKC && !ABF && a.rowsum != nullptr && bx == 0;
    float4 rs[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    auto store_tile = [&](int stage) {
        __bf16* S = smem + stage * BIG_STAGE;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!AKC && !ABF && do_rs) {
                rs[h].x += ra[h].v[0] + ra[h].v[4]; rs[h].y += ra[h].v[1] + ra[h].v[5];
                rs[h].z += ra[h].v[2] + ra[h].v[6]; rs[h].w += ra[h].v[3] + ra[h].v[7];
            }
            sp_store<AKC, 1, F16, ABF>(S + h * SP_PLANE, ra[h]);
            sp_store<BKC, 1, F16>(S + (2 + h) * SP_PLANE, rb[h]);
        }
    };
    auto compute = [&](int stage) {
        const __bf16* S = smem + stage * BIG_STAGE;
        const __bf16* Ah = S + wm * SP_PLANE;                       // this wave's A half (outer-contiguous image base)
        const __bf16* Bh = S + (2 + (wn >> 1)) * SP_PLANE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bf[j] = BKC ? sp_frag(S + foff_b + j * 32 * SP_LD + ks * 16) : sp_frag_tr(Bh, (wn & 1) * 64 + 32 * j, ks);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                af[i] = AKC ? sp_frag(S + foff_a + i * 32 * SP_LD + ks * 16) : sp_frag_tr(Ah, 32 * i, ks);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (F16)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[i]), __builtin_bit_cast(f16x8, bf[j]),
                                                                           acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
                }
        }
    };
    load_tile(0);
    store_tile(0);
    if (nt > 1) load_tile(1);
    big_barrier();
    for (int t = 0; t < nt; ++t) {
        const int st = t & 1;
        if (t + 1 < nt) store_tile(st ^ 1);           // k-tile t + 1 (in registers since the previous iteration)
        if (t + 2 < nt) load_tile(t + 2);
        compute(st);
        big_barrier();
    }
    if (!AKC && !ABF && do_rs) {      // (uniform over the block) 16 threads hold partial sums of the same four rows of a half: meet in LDS
        float4* rs_s = reinterpret_cast<float4*>(smem);
        __syncthreads();
        rs_s[threadIdx.x] = rs[0];
        rs_s[512 + threadIdx.x] = rs[1];
        __syncthreads();
        if (threadIdx.x < 64) {
            const int h = threadIdx.x >> 5, g = threadIdx.x & 31;
            float4 t = rs_s[h * 512 + g];
#pragma unroll
            for (int q = 1; q < 16; ++q) {
                const float4 o = rs_s[h * 512 + g + 32 * q];
                t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
            }
            const int m = m0 + 128 * h + 4 * g;
            if (m + 0 < a.M) atomicAdd(a.rowsum + m + 0, t.x);
            if (m + 1 < a.M) atomicAdd(a.rowsum + m + 1, t.y);
            if (m + 2 < a.M) atomicAdd(a.rowsum + m + 2, t.z);
            if (m + 3 < a.M) atomicAdd(a.rowsum + m + 3, t.w);
        }
    }
    const bool atomic = a.splitk > 1;
    const bool first = bz == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + j * 32 + (lane & 31);
        if (col >= a.N) continue;
        const float bv = (a.bias && first) ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row0 = m0 + wm * 128 + i * 32 + 4 * (lane >> 5);
            if (a.c_half) gemm_epilogue16(acc[i][j], a.C, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, atomic, 1, (int64_t)row0 * a.ldc + col);
            else gemm_epilogue16(acc[i][j], a.C + (int64_t)row0 * a.ldc + col, a.ldc, a.M - row0, a.alpha, a.beta, bv, a.act, atomic);
        }
    }
}
template <bool AKC, bool BKC, bool F16, bool ABF>
__global__ __launch_bounds__(512, 2) void gemm_big_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) __bf16 big_smem[];
    gemm_big_body<AKC, BKC, F16, ABF>(a, big_smem, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC, bool F16>
__global__ __launch_bounds__(512, 2) void gemm_big_group_kernel(GemmGroupArgs G) {
    extern __shared__ __attribute__((aligned(16))) __bf16 big_smem[];
    int p = 0;
    while (p + 1 < G.n && (int)blockIdx.x >= G.start[p + 1]) ++p;
    const GemmArgs& a = G.p[p];
    const int id = blockIdx.x - G.start[p];
    const int tn = (a.N + 255) / 256, tm = (a.M + 255) / 256;
    const int bx = id % tn, by = (id / tn) % tm, bz = id / (tn * tm);
    gemm_big_body<AKC, BKC, F16, false>(a, big_smem, bx, by, bz);
}
template <typename K> static bool big_attr(K kernel) {          // dynamic LDS above 64 KB: the attribute once per kernel and device
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done.load(std::memory_order_acquire) & (1ull << dev)) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, BIG_LDS_BYTES) != hipSuccess)
        return false;
    done.fetch_or(1ull << dev, std::memory_order_release);
    return true;
}

// (Round 4, measured and dropped -- profiles/r04_exp_gemm_waves4.txt, _pp.txt, _swp.txt, _big3.txt: a four-wave block with 64 x 64 wave tiles;
// 256 x 256 tiles for the three-plane products (+8-10 % at 4096^3, 0.5-0.8x at configs[1]'s M = 2560 shapes);
// a ping-pong of the two wave halves between MFMA and split intervals; one software-pipelined MFMA + split stream per wave.  All within
// +-10 % of this kernel: two waves per SIMD carrying 24 MFMAs + ~90 vector instructions + 30 LDS accesses per k-tile saturate the SIMD's
// issue port at ~75 % matrix-pipe occupancy whatever the order.)
// (A double-buffered variant -- 110 KB of LDS, one block per CU, split/store of tile t+1 issued between the k-halves of
// tile t -- measured 6-9 % slower than this single-stage kernel at two blocks per CU, and was dropped.  So was a
// wave-specialised one -- 4 producer waves splitting into a second LDS stage while 4 consumer waves run 64x64 MFMA
// tiles: 128 vs 138 TFLOP/s at 4096^3, up to 35 % slower at K = 256 -- and a 3-tile register prefetch (154 VGPRs, one
// block per CU).  Reference points: PMC on this kernel shows MFMA 31 %, LDS 39 %, VALU 26 % busy; a pure MFMA loop
// (tools/mfma_probe.hip) sustains 1.9-2.1 PFLOP/s bf16, i.e. 315-350 TFLOP/s fp32-equivalent at six products.)
// Planes per operand of the bf16 split: VagCallCtx::gemm_planes (3, 2, 1 or 11: see there).

// plan -> kernel: the ONLY place that names instantiations of the product kernels (a variant not listed here is not in the library).
// Families as in include/vag_nmt.h (VAG_GEMM_*: tiled 64 x 64 f32, tiled 128 x 128 f32, bf16 planes 128 x 128, one plane 256 x 256).
enum GemmFamily { GEMM_NONE = -1 /* no kernel takes the product */, GEMM_TILED64 = VAG_GEMM_TILED64, GEMM_TILED128_F32 = VAG_GEMM_TILED128_F32,
                  GEMM_SPLIT128 = VAG_GEMM_SPLIT128, GEMM_BIG256 = VAG_GEMM_BIG256 };
static inline int gemm_family_tile(GemmFamily f) { return f == GEMM_TILED64 ? 64 : f == GEMM_BIG256 ? 256 : 128; }
using GemmKernel = void (*)(GemmArgs);
using GemmGroupKernel = void (*)(GemmGroupArgs);
template <class F> static auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> static auto with_layout(bool akc, bool bkc, F&& f) {
    return with_bool(akc, [&](auto ak) { return with_bool(bkc, [&](auto bk) { return f(ak, bk); }); });      // flags -> template arguments
}
static GemmKernel gemm_kernel_for(GemmFamily fam, bool akc, bool bkc, bool vec, int planes, bool a_bf16) {       // nullptr: no such variant
    if (a_bf16) {       // a bf16-stored A (the head's two vocabulary-sized gradient products over a bf16 d(logits) chunk): one bf16 plane only
        if (planes != 1 || bkc || !vec) return nullptr;
        if (fam == GEMM_BIG256) return akc ? gemm_big_kernel<true, false, false, true> : gemm_big_kernel<false, false, false, true>;
        if (fam == GEMM_SPLIT128) return akc ? gemm_split_kernel<true, false, true, 1, false, true> : gemm_split_kernel<false, false, true, 1, false, true>;
        return nullptr;
    }
    return with_layout(akc, bkc, [&](auto ak, auto bk) -> GemmKernel {
        constexpr bool AK = decltype(ak)::value, BKc = decltype(bk)::value;
        if (fam == GEMM_BIG256) return planes == 11 ? gemm_big_kernel<AK, BKc, true, false> : gemm_big_kernel<AK, BKc, false, false>;
        return with_bool(vec, [&](auto v) -> GemmKernel {
            constexpr bool V = decltype(v)::value;
            switch (fam) {
            case GEMM_TILED64: return gemm_tiled_kernel<64, 64, AK, BKc, V, 256>;
            case GEMM_TILED128_F32: return gemm_tiled_kernel<128, 128, AK, BKc, V, 512>;       // 8 waves (2 per SIMD)
            case GEMM_SPLIT128:
                return planes == 2 ? gemm_split_kernel<AK, BKc, V, 2> : planes == 1 ? gemm_split_kernel<AK, BKc, V, 1>
                     : planes == 11 ? gemm_split_kernel<AK, BKc, V, 1, true> : gemm_split_kernel<AK, BKc, V, 3>;
            default: return nullptr;
            }
        });
    });
}
// grouped launches: vectorised loads only (the queue takes nothing else), 128 x 128 by planes or 256 x 256 one-plane
static GemmGroupKernel gemm_group_kernel_for(bool big, bool akc, bool bkc, int planes) {
    return with_layout(akc, bkc, [&](auto ak, auto bk) -> GemmGroupKernel {
        constexpr bool AK = decltype(ak)::value, BKc = decltype(bk)::value;
        if (big) return planes == 11 ? gemm_big_group_kernel<AK, BKc, true> : gemm_big_group_kernel<AK, BKc, false>;
        return planes == 11 ? gemm_split_group_kernel<AK, BKc, 1, true> : planes == 1 ? gemm_split_group_kernel<AK, BKc, 1, false>
             : planes == 2 ? gemm_split_group_kernel<AK, BKc, 2, false> : gemm_split_group_kernel<AK, BKc, 3, false>;
    });
}

__global__ __launch_bounds__(256) void fill2d_kernel(float* __restrict__ C, int64_t ldc, int64_t rows, int64_t cols) {
    const int64_t total = rows * cols;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        C[r * ldc + (i - r * cols)] = 0.f;
    }
}

// ---- column sums (bias gradients): the kernels (their launchers and queue follow the products' below) ----
// out (and, when given, out2 / out3: parameters whose gradients are the same column sums) += column sums of X
// (The two kernels keep a copy of the loop each: through one shared __forceinline__ body both compiled to other instructions.)
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int M, int N, int64_t ld,
                                                     int rows_per, float* __restrict__ out, float* __restrict__ out2,
                                                     float* __restrict__ out3) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int m0 = blockIdx.y * rows_per, m1 = min(M, m0 + rows_per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int m = m0;
    for (; m + 3 < m1; m += 4) {
        s0 += X[(int64_t)m * ld + n];
        s1 += X[(int64_t)(m + 1) * ld + n];
        s2 += X[(int64_t)(m + 2) * ld + n];
        s3 += X[(int64_t)(m + 3) * ld + n];
    }
    for (; m < m1; ++m) s0 += X[(int64_t)m * ld + n];
    const float t = (s0 + s1) + (s2 + s3);
    atomicAdd(out + n, t);
    if (out2) atomicAdd(out2 + n, t);
    if (out3) atomicAdd(out3 + n, t);
}
// Several column sums in one grid (blockIdx.z = task): inside a vag_gemm_group_begin/end bracket the bias-gradient sums
// of an operator are queued like its weight-gradient products and go out together.
constexpr int COLSUM_MAX = 8;
struct ColsumTasks {
    const float* X[COLSUM_MAX]; float* out[COLSUM_MAX]; float* out2[COLSUM_MAX]; float* out3[COLSUM_MAX];
    int64_t ld[COLSUM_MAX];
    int M[COLSUM_MAX], N[COLSUM_MAX], rows_per[COLSUM_MAX];
};
__global__ __launch_bounds__(256) void colsum_multi_kernel(ColsumTasks T) {
    const int k = blockIdx.z;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int M = T.M[k], N = T.N[k], rows_per = T.rows_per[k];
    const int m0 = blockIdx.y * rows_per;
    if (n >= N || m0 >= M) return;
    const int m1 = min(M, m0 + rows_per);
    const float* X = T.X[k];
    const int64_t ld = T.ld[k];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int m = m0;
    for (; m + 3 < m1; m += 4) {
        s0 += X[(int64_t)m * ld + n];
        s1 += X[(int64_t)(m + 1) * ld + n];
        s2 += X[(int64_t)(m + 2) * ld + n];
        s3 += X[(int64_t)(m + 3) * ld + n];
    }
    for (; m < m1; ++m) s0 += X[(int64_t)m * ld + n];
    const float t = (s0 + s1) + (s2 + s3);
    atomicAdd(T.out[k] + n, t);
    if (T.out2[k]) atomicAdd(T.out2[k] + n, t);
    if (T.out3[k]) atomicAdd(T.out3[k] + n, t);
}

// ---- the plan of ONE product: kernel family, split-K, whether its row sum rides.  Pure: no HIP call, no context read. ----
struct GemmPlanIn {
    int64_t M, N, K;
    bool akc, bkc, vec;            // A / B k-contiguous; both operands 16-byte aligned with leading dimensions % 4 == 0
    float beta; int act;
    bool c_half, a_bf16, rowsum;   // rowsum: the caller wants A's row sums
    int planes;                    // VagCallCtx::gemm_planes
    bool f32mfma, big_on; int force_tile, force_splitk;      // vag_opt(): gemm_f32mfma, gemm_big, gemm_force_tile / _splitk
    bool slabs;                    // a slab scratch is at hand on the launch's stream (gemm_slabs_usable)
};
struct GemmPlan {
    GemmFamily family;
    int T, splitk; double model_us;      // the cost model's choice (the force hook applied): what "gemm_debug" prints
    int slices, kchunk;                  // what is launched: grid z and the k-length of a slice
    bool rowsum_rides;                   // the kernel takes the row sums along; false with rowsum wanted: a column-sum launch first
};
// the 2-byte storage mode's one-plane products take 256 x 256 tiles (gemm_big_kernel) from this size on
static bool gemm_big_fits(int planes, int64_t M, int64_t N, bool big_on) { return (planes == 1 || planes == 11) && big_on && M >= 192 && N >= 192; }
// row sums ride on outer-contiguous A tiles of the three-plane 128 x 128 kernels (at the one-plane kernels' 80-VGPR cap the extra
// state spills) and of the 256 x 256 one-plane kernel over an fp32 A; every other kernel leaves them to a column-sum pass over A
static bool gemm_rowsum_rides(GemmFamily f, int planes, bool akc, bool a_bf16) {
    return (f == GEMM_SPLIT128 && planes == 3) || (f == GEMM_BIG256 && !akc && !a_bf16);
}
// Tile / split-K choice.  One 128x128 block keeps a CU's four MFMA pipes busy for 128*k cycles, so a launch is only
// efficient with >= 2 blocks per CU in flight (latency hiding across co-resident blocks) and every CU busy: small-output,
// deep-K products (every weight gradient: K = Tt*B) are split along K and accumulated with fp32 atomics.
static GemmPlan gemm_plan_single(const GemmPlanIn& in) {
    const int64_t M = in.M, N = in.N, K = in.K;
    const float beta = in.beta;
    // cost model (microseconds) over tile in {64,128} x split-K: MFMA time of the busiest CU + output traffic
    // (split-K partial sums as fp32 atomics ~3 TB/s chip-wide, plain stores ~4 TB/s) -- constants fitted to measured launches.
    const bool can_split = (in.act == VAG_ACT_NONE) && (beta == 0.f || beta == 1.f) && !in.c_half;
    double best = 1e30;
    int64_t T = 64, splitk = 1;
    // bytes/us of split-K partial sums landing as fp32 atomics (fitted: tools/exp_gemm_sweep.py; 1e6 was too pessimistic)
    const double atomic_rate = 3.0e6;
    for (int64_t t = 64; t <= 128; t *= 2) {
        if (t == 128 && (M <= 64 || N <= 64)) continue;
        if (t == 64 && in.a_bf16 && M > 64 && N > 64) continue;       // a bf16-stored operand: the 128 x 128 one-plane kernel only
        const double eff = (t == 128) ? (in.f32mfma ? 0.62 : 0.64) : 0.42;   // fraction of the f32-MFMA peak
        const int64_t base = cdiv64(M, t) * cdiv64(N, t);
        for (int64_t sp = 1; sp <= 64; sp += (sp < 16 ? 1 : sp < 32 ? 4 : 8)) {      // few tiles, long K (a row chunk of d(tmid)): up to 64
            if (sp > 1 && (!can_split || K / sp < 128)) break;
            const int64_t kper = cdiv64(cdiv64(K, sp), BK) * BK;
            const int64_t blocks = base * sp;
            // a CU holds two 128x128 blocks, and a pair advances ~1.33x faster than two blocks one after the other:
            // full waves of 512 blocks count 1.5 "single-block rounds", a remainder of <= 256 blocks counts 1
            double rounds;
            if (t == 128 && !in.f32mfma) {
                const int64_t full = blocks / 512, rem = blocks % 512;
                rounds = 1.5 * (double)full + (rem == 0 ? 0.0 : (rem <= 256 ? 1.0 : 1.5));
            } else {
                rounds = (double)cdiv64(blocks, 256);
            }
            const double t_mfma = rounds * (double)kper * (double)(t * t) * 2.0 / (256.0 * eff) / 2400.0;
            const double bytes = (double)M * (double)N * 4.0;
            // (slab form of split-K, when the caller's scratch is at hand: the slices' slabs as plain stores, then the last block
            // of a tile reads them back one round trip per slice, plus the one result)
            const bool slabs_on = in.slabs && t == 128 && in.planes == 3 && !in.f32mfma;
            const double t_out = sp > 1 ? (slabs_on ? sp * bytes / 4.0e6 + 1.5 * sp + bytes / (beta != 0.f ? atomic_rate : 4.0e6)
                                                    : sp * bytes / atomic_rate + (beta == 0.f ? bytes / 4.0e6 + 2.0 : 0.0))
                                        : bytes * (beta != 0.f ? 2.0 : 1.0) / 4.0e6;
            const double cost = t_mfma + t_out;
            if (cost < best) { best = cost; T = t; splitk = sp; }
        }
    }
    // tuning hook: vag_set_option("gemm_force_tile" / "gemm_force_splitk")
    if ((in.force_tile == 64 || in.force_tile == 128) && in.force_splitk >= 1 && (in.force_splitk == 1 || can_split)) {
        T = in.force_tile; splitk = in.force_splitk;
    }
    GemmPlan p;
    p.T = (int)T; p.splitk = (int)splitk; p.model_us = best;
    if (T == 128 && gemm_big_fits(in.planes, M, N, in.big_on) && in.vec && !in.f32mfma && (!in.a_bf16 || !in.bkc) && in.force_tile == 0) {
        // the 2-byte storage mode's one-plane products on 256 x 256 tiles: split-K so that tiles x slices fill the 256 CUs about
        // once; a bf16-stored A (d(logits) chunks) included.  (Only where the cost model chose the 128 x 128 one-plane kernel:
        // products it sends to the exact f32 64 x 64 kernel stay there.)
        p.family = GEMM_BIG256;
        const int64_t tiles = cdiv64(M, 256) * cdiv64(N, 256);
        splitk = 1;
        if (can_split) while (tiles * splitk < 208 && K / (splitk + 1) >= 512 && splitk < 32) ++splitk;
    } else {
        p.family = T == 64 ? GEMM_TILED64 : in.f32mfma ? GEMM_TILED128_F32 : GEMM_SPLIT128;
    }
    p.kchunk = (int)(cdiv64(cdiv64(K, splitk), BK) * BK);
    p.slices = (int)cdiv64(K, p.kchunk);
    // a bf16-stored operand exists for the one-plane kernels only (gemm_kernel_for)
    if (in.a_bf16 && !(p.family == GEMM_BIG256 || (p.family == GEMM_SPLIT128 && in.planes == 1 && !in.bkc && in.vec))) p.family = GEMM_NONE;
    p.rowsum_rides = in.rowsum && gemm_rowsum_rides(p.family, in.planes, in.akc, in.a_bf16);
    return p;
}

// ---- the plan of a grouped launch ----
// Split-K and block order of one grouped launch.  The chip runs 512 of these blocks at a time (two per CU) and hands out
// blocks in index order to whichever slot frees first, i.e. list scheduling: with the longest blocks first the launch ends
// on short ones.  A common target slice length L (k-steps of SP_BK) is tried over the slice lengths the products can have;
// products are cut into round(K / L) slices (never shorter than 256; one that overwrites its output needs a fill launch first).  Each candidate is
// priced by simulating that schedule (block cost = slice length + a fixed prologue / epilogue share) plus the extra atomic
// traffic of the slices.  (The first version aimed at ~512 blocks with one common split: totals of 528 / 576 blocks -- the
// decoder / encoder weight-gradient groups -- ran a full second round for 16 / 64 blocks: 204 and 108 us.)
struct GroupPlanEntry { int n, tile; bool slabs; int m[GROUP_MAX], nn[GROUP_MAX], k[GROUP_MAX]; bool acc[GROUP_MAX], half[GROUP_MAX]; int split[GROUP_MAX], order[GROUP_MAX]; };
static void group_plan_compute(const GemmArgs* q, int n, int* split, int* order, int tile, bool slabs = false);
// plans are remembered per list of shapes (a training run repeats a handful of them; the simulation costs ~1 ms of host time)
static void group_plan(const GemmArgs* q, int n, int* split, int* order, int tile = 128, bool slabs = false) {
    constexpr int CACHE = 64;
    static thread_local GroupPlanEntry cache[CACHE];
    static thread_local int used = 0, next = 0;
    for (int e = 0; e < used; ++e) {
        const GroupPlanEntry& c = cache[e];
        bool same = c.n == n && c.tile == tile && c.slabs == slabs;
        for (int i = 0; same && i < n; ++i)
            same = c.m[i] == q[i].M && c.nn[i] == q[i].N && c.k[i] == q[i].K && c.acc[i] == (q[i].beta != 0.f) &&
                   c.half[i] == (q[i].c_half != 0);
        if (same) {
            for (int i = 0; i < n; ++i) { split[i] = c.split[i]; order[i] = c.order[i]; }
            return;
        }
    }
    group_plan_compute(q, n, split, order, tile, slabs);
    GroupPlanEntry& c = cache[next];
    next = (next + 1) % CACHE;
    if (used < CACHE) ++used;
    c.n = n; c.tile = tile; c.slabs = slabs;
    for (int i = 0; i < n; ++i) {
        c.m[i] = q[i].M; c.nn[i] = q[i].N; c.k[i] = q[i].K; c.acc[i] = q[i].beta != 0.f; c.half[i] = q[i].c_half != 0;
        c.split[i] = split[i]; c.order[i] = order[i];
    }
}
static void group_plan_compute(const GemmArgs* q, int n, int* split, int* order, int tile, bool slabs) {
    constexpr int MAXSLOTS = 512;
    const int SLOTS = tile == 256 ? 256 : 512;  // 256 x 256 one-plane blocks (gemm_big_kernel): one per CU
    const double C0 = tile == 256 ? 8.0 : 4.0;  // k-steps a block spends outside its main loop
    const double US_PER_KSTEP = tile == 256 ? 1.0 : 2.5;        // one 128x128x32 step of a block sharing its CU / one 256x256x32 one-plane step
    int cand[GROUP_MAX * 10 + 1], nc = 0;
    for (int i = 0; i < n; ++i) {
        const int ks = (int)cdiv64(q[i].K, SP_BK);
        const int smax = q[i].c_half ? 1 : std::max(1, std::min(10, q[i].K / 256));      // fp16 outputs are stored whole
        for (int j = 1; j <= smax; ++j) {
            const int L = (ks + j - 1) / j;
            bool seen = false;
            for (int c = 0; c < nc; ++c) seen = seen || cand[c] == L;
            if (!seen) cand[nc++] = L;
        }
    }
    double best = 1e30;
    double load[MAXSLOTS];
    for (int c = 0; c < nc; ++c) {
        const int L = cand[c];
        int sp[GROUP_MAX], len[GROUP_MAX], ord[GROUP_MAX];
        double atomic_us = 0.0;
        for (int i = 0; i < n; ++i) {
            const int ks = (int)cdiv64(q[i].K, SP_BK);
            int s_i = (ks + L / 2) / L;
            const int smax = q[i].c_half ? 1 : std::max(1, q[i].K / 256);
            s_i = std::max(1, std::min(s_i, smax));
            const double out_bytes = (double)q[i].M * (double)q[i].N * 4.0;
            if (slabs && s_i > 1) atomic_us += (double)s_i * out_bytes / 4.0e6 + 1.5 * s_i / 4.0 + out_bytes / (q[i].beta != 0.f ? 3.0e6 : 4.0e6);
            else if (q[i].beta != 0.f) atomic_us += (double)s_i * out_bytes / 3.0e6;
            else if (s_i > 1) atomic_us += (double)s_i * out_bytes / 3.0e6 + 4.0 + out_bytes / 4.0e6;   // + a fill launch first
            sp[i] = s_i;
            len[i] = (ks + s_i - 1) / s_i;
            ord[i] = i;
        }
        std::stable_sort(ord, ord + n, [&](int a, int b) { return len[a] > len[b]; });
        // list scheduling of equal-cost batches onto the slots: a min-heap of slot loads
        for (int k = 0; k < SLOTS; ++k) load[k] = 0.0;
        std::make_heap(load, load + SLOTS, std::greater<double>());
        double makespan = 0.0;
        for (int j = 0; j < n; ++j) {
            const int i = ord[j];
            const int64_t blocks = cdiv64(q[i].M, tile) * cdiv64(q[i].N, tile) * sp[i];
            const double cost = (double)len[i] + C0;
            for (int64_t b = 0; b < blocks; ++b) {
                std::pop_heap(load, load + SLOTS, std::greater<double>());
                load[SLOTS - 1] += cost;
                makespan = std::max(makespan, load[SLOTS - 1]);
                std::push_heap(load, load + SLOTS, std::greater<double>());
            }
        }
        const double us = makespan * US_PER_KSTEP + atomic_us;
        if (us < best) {
            best = us;
            for (int i = 0; i < n; ++i) { split[i] = sp[i]; order[i] = ord[i]; }
        }
    }
}
// Host-only view of the plan (include/vag_nmt.h: vag_gemm_group_plan): tests and tuning scripts
int vag_gemm_group_plan_host(int n, const int64_t* M, const int64_t* N, const int64_t* K, const int* accumulate, int* split,
                             int* order) {
    VAG_CHECK_ARG(n >= 1 && n <= GROUP_MAX && M && N && K && accumulate && split && order);
    GemmArgs q[GROUP_MAX] = {};
    for (int i = 0; i < n; ++i) {
        VAG_CHECK_ARG(M[i] > 0 && N[i] > 0 && K[i] > 0 && M[i] < (1ll << 30) && N[i] < (1ll << 30) && K[i] < (1ll << 30));
        q[i].M = (int)M[i]; q[i].N = (int)N[i]; q[i].K = (int)K[i]; q[i].beta = accumulate[i] ? 1.f : 0.f; q[i].c_half = 0;
    }
    group_plan_compute(q, n, split, order, 128);
    return VAG_OK;
}
// ... and of one product (include/vag_nmt.h: vag_gemm_plan): no slab scratch, options from vag_set_option, planes 0 = the calling thread's
int vag_gemm_plan_host(int64_t M, int64_t N, int64_t K, int a_kc, int b_kc, int vec, float beta, int act, int c_half, int a_bf16,
                       int rowsum, int planes, int* plan) {
    VAG_CHECK_ARG(plan && M > 0 && N > 0 && K > 0 && M < (1ll << 30) && N < (1ll << 30) && K < (1ll << 30));
    VAG_CHECK_ARG((planes == 0 || planes == 1 || planes == 2 || planes == 3 || planes == 11) && (act == VAG_ACT_NONE || act == VAG_ACT_TANH));
    if (planes == 0) planes = vag_ctx().gemm_planes;
    VAG_CHECK_ARG((!a_bf16 || (planes == 1 && !rowsum)) && (!c_half || beta == 0.f) && (!rowsum || !a_kc));      // the rules of vag_gemm_launch
    const VagOptions& o = vag_opt();
    const GemmPlanIn in = {M, N, K, a_kc != 0, b_kc != 0, vec != 0, beta, act, c_half != 0, a_bf16 != 0, rowsum != 0, planes,
                           o.gemm_f32mfma != 0, o.gemm_big != 0, o.gemm_force_tile, o.gemm_force_splitk, false};
    const GemmPlan p = gemm_plan_single(in);
    VAG_CHECK_ARG(p.family != GEMM_NONE);
    plan[0] = p.family; plan[1] = p.T; plan[2] = p.splitk; plan[3] = p.slices; plan[4] = p.kchunk; plan[5] = p.rowsum_rides ? 1 : 0;
    return VAG_OK;
}

// ---- output preparation: slabs, prezeroed marks, fill ----
// Scratch of the slab form of split-K (GemmArgs::slab): VagCallCtx::gemm_scratch, the step driver's workspace (step.hip).
static bool gemm_slabs_usable(hipStream_t stream) {
    const VagCallCtx::GemmScratch& sc = vag_ctx().gemm_scratch;
    return sc.slab && sc.tickets && stream == sc.stream && vag_opt().gemm_slabs != 0;
}
// slabs and tickets for a product of `tiles` output tiles in `slices` k-slices on `stream`, from running offsets; false: does not
// fit, another stream's launch, or off
static bool gemm_take_slabs(GemmArgs& a, int64_t tiles, int slices, int64_t& used_f, int64_t& used_t, hipStream_t stream) {
    a.slab = nullptr; a.ticket = nullptr; a.nslices = slices;
    const VagCallCtx::GemmScratch& sc = vag_ctx().gemm_scratch;
    if (slices <= 1 || !gemm_slabs_usable(stream)) return false;
    const int64_t need = tiles * slices * 16384;
    if (used_f + need > sc.floats || used_t + tiles > sc.ntickets) return false;
    a.slab = sc.slab + used_f; a.ticket = sc.tickets + used_t;
    used_f += need; used_t += tiles;
    return true;
}
static bool gemm_take_prezeroed(const float* C) {          // VagCallCtx::gemm_prezeroed: an entry is used once
    for (auto& q : vag_ctx().gemm_prezeroed)
        if (q && q == C) { q = nullptr; return true; }
    return false;
}
// Before the kernel of a product in `slices` k-slices: slabs where the kernel has that form (slabs_ok) and the scratch has room past
// the running offsets, else a zeroed output for an overwriting product's slices: a prezeroed mark (spent either way) or a fill launch.
static int gemm_prepare_output(GemmArgs& a, int T, int slices, bool slabs_ok, int64_t& slab_used, int64_t& ticket_used, hipStream_t stream) {
    const bool slabs = slabs_ok && gemm_take_slabs(a, cdiv64(a.M, T) * cdiv64(a.N, T), slices, slab_used, ticket_used, stream);
    if (!slabs) { a.slab = nullptr; a.ticket = nullptr; a.nslices = slices; }
    if (slabs && a.beta == 0.f) (void)gemm_take_prezeroed(a.C);
    if (a.beta == 0.f && slices > 1 && !slabs && !gemm_take_prezeroed(a.C)) {
        int64_t nb = cdiv64((int64_t)a.M * a.N, 256 * 8);
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(fill2d_kernel, dim3((unsigned)nb), dim3(256), 0, stream, a.C, a.ldc, (int64_t)a.M, (int64_t)a.N);
        VAG_LAUNCH_CHECK();
    }
    return VAG_OK;
}

// ---- one planned product: row-sum fallback, output preparation, kernel.  Never queues; no slabs on a stream other than
// gemm_scratch.stream (gemm_take_slabs).  g: operands, shape, epilogue; its kchunk / splitk / slab fields are set here. ----
static int gemm_launch_single(GemmArgs g, bool akc, bool bkc, bool vec, int planes, hipStream_t stream) {
    const VagOptions& o = vag_opt();
    const GemmPlanIn in = {g.M, g.N, g.K, akc, bkc, vec, g.beta, g.act, g.c_half != 0, g.a_bf16 != 0, g.rowsum != nullptr, planes,
                           o.gemm_f32mfma != 0, o.gemm_big != 0, o.gemm_force_tile, o.gemm_force_splitk, gemm_slabs_usable(stream)};
    const GemmPlan p = gemm_plan_single(in);
#ifdef VAG_LAB
    if (o.gemm_debug)
        fprintf(stderr, "[vag_gemm] M=%lld N=%lld K=%lld akc=%d bkc=%d beta=%g -> T=%lld splitk=%lld model=%.1f us\n",
                (long long)g.M, (long long)g.N, (long long)g.K, (int)akc, (int)bkc, (double)g.beta, (long long)p.T, (long long)p.splitk, p.model_us);
#endif
    const GemmKernel kernel = gemm_kernel_for(p.family, akc, bkc, vec, planes, g.a_bf16 != 0);
    VAG_CHECK_ARG(kernel != nullptr);
    if (g.rowsum && !p.rowsum_rides) {
        VAG_TRY(vag_colsum_launch(g.A, g.K, g.M, g.sa_k, g.rowsum, stream));
        g.rowsum = nullptr;
    }
    g.splitk = p.slices; g.kchunk = p.kchunk;
    const int T = gemm_family_tile(p.family);
    int64_t slab_used = 0, ticket_used = 0;
    VAG_TRY(gemm_prepare_output(g, T, p.slices, p.family == GEMM_SPLIT128 && planes == 3 && !g.a_bf16, slab_used, ticket_used, stream));
    const dim3 grid((unsigned)cdiv64(g.N, T), (unsigned)cdiv64(g.M, T), (unsigned)p.slices);
    const bool big = p.family == GEMM_BIG256;
    if (big && !big_attr(kernel)) return VAG_EINVAL;
    hipLaunchKernelGGL(kernel, grid, dim3(p.family == GEMM_TILED64 ? 256 : 512), big ? BIG_LDS_BYTES : 0, stream, g);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

// ---- the queues of a host thread: group bracket, leaf list, column sums (queued while a bracket is open, one launch per flush) ----
// Host side; thread_local: forward runs on the caller's thread, backward on the autograd engine's; a bracket never spans threads.
// Group bracket: one queue per operand layout (index akc*2 + bkc).  Brackets nest: an inner end() flushes everything queued so far
// (its caller is about to consume those results) and the outer bracket keeps collecting afterwards.
// Leaf list (step driver, backward of the VSE branch and of the initial state: VSE_Imagine_Enc.py:110-152, V11.py:118): the
// weight-gradient products of those operators are rank-B updates (K = B <= 128 rows) that nothing later in the step reads -- five
// launches of the 64 x 64 kernel and three column-sum launches, ~5 us each, strung between the kernels of a 28-launch chain.
// While VagCallCtx::leaf_on is set such products (and the column sums that go with them) are held back and go out as ONE launch
// at leaf_flush; their operands must stay untouched until then (the step driver's do: api.hip).  The list is empty whenever
// leaf_on is off: the flush and leaf_drop (an error return before the flush: the call scope's destructor) both leave it so.
struct GemmQueues {         // (an aggregate without initialisers: the thread's copy starts zeroed, no constructor runs)
    int depth;
    int qn[4];
    GemmArgs q[4][GROUP_MAX];
    LeafTasks leaf;
    bool colsum_on;
    int colsum_n;
    ColsumTasks colsum;
    unsigned colsum_gx, colsum_gy;

    void colsum_begin() { colsum_on = true; colsum_n = 0; colsum_gx = colsum_gy = 0; }
    void colsum_abort() { colsum_on = false; colsum_n = 0; }
    int colsum_flush(hipStream_t stream) {       // launches what is queued; the queue stays open
        const int n = colsum_n;
        colsum_n = 0;
        const unsigned gx = colsum_gx, gy = colsum_gy;
        colsum_gx = colsum_gy = 0;
        if (n == 0) return VAG_OK;
        hipLaunchKernelGGL(colsum_multi_kernel, dim3(gx, gy, (unsigned)n), dim3(256), 0, stream, colsum);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    void begin() {
        if (depth++ == 0) {
            for (int l = 0; l < 4; ++l) qn[l] = 0;
            colsum_begin();
        }
    }
    void abort() {        // error path: drop the queues
        depth = 0;
        for (int l = 0; l < 4; ++l) qn[l] = 0;
        colsum_abort();
    }
    int flush_layout(int lay, hipStream_t stream, bool own_stream) {
        const int n = qn[lay];
        qn[lay] = 0;
        if (n == 0) return VAG_OK;
        const int gemm_planes = vag_ctx().gemm_planes;
        const bool akc = (lay & 2) != 0, bkc = (lay & 1) != 0;
        if (n == 1) return gemm_launch_single(q[lay][0], akc, bkc, true, gemm_planes, stream);      // (on a leaf stream: no slabs)
        GemmGroupArgs G;
        G.n = n;
        int split[GROUP_MAX], order[GROUP_MAX];
        // the 2-byte storage mode's one-plane products: 256 x 256 tiles when every product of the group is large enough for them
        bool big = true;
        for (int j = 0; j < n && big; ++j) big = gemm_big_fits(gemm_planes, q[lay][j].M, q[lay][j].N, vag_opt().gemm_big != 0) && !q[lay][j].a_bf16;
        const int T = big ? 256 : 128;
        const bool rides = gemm_rowsum_rides(big ? GEMM_BIG256 : GEMM_SPLIT128, gemm_planes, akc, false);
        for (GemmArgs* r = q[lay]; r < q[lay] + n; ++r)
            if (r->rowsum && !rides) {
                VAG_TRY(vag_colsum_launch(r->A, r->K, r->M, r->sa_k, r->rowsum, stream));
                r->rowsum = nullptr;
            }
        const bool slabs_ok = !big && own_stream && gemm_planes == 3;
        group_plan(q[lay], n, split, order, T, slabs_ok && gemm_slabs_usable(stream));
        int total = 0;
        int64_t slab_used = 0, ticket_used = 0;
        for (int j = 0; j < n; ++j) {
            GemmArgs& a = G.p[j];
            a = q[lay][order[j]];
            int s_i = split[order[j]];
            const int kchunk = (int)(cdiv64(cdiv64(a.K, s_i), SP_BK) * SP_BK);
            s_i = (int)cdiv64(a.K, kchunk);
            a.kchunk = kchunk;
            // accumulating products always add atomically here (two of them may target the same gradient buffer);
            // splitk > 1 is what selects the atomic epilogue, the block count below uses the real number of k-slices
            a.splitk = a.beta != 0.f ? (s_i > 2 ? s_i : 2) : s_i;
            VAG_TRY(gemm_prepare_output(a, T, s_i, slabs_ok, slab_used, ticket_used, stream));
            G.start[j] = total;
            total += (int)(cdiv64(a.M, T) * cdiv64(a.N, T)) * s_i;
        }
        G.start[n] = total;
        const GemmGroupKernel kernel = gemm_group_kernel_for(big, akc, bkc, gemm_planes);
        if (big && !big_attr(kernel)) return VAG_EINVAL;
        hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(512), big ? BIG_LDS_BYTES : 0, stream, G);
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    int flush(hipStream_t stream) {            // a bracket's end
        if (depth <= 0) return VAG_OK;
        int rc = colsum_flush(stream);
        VagCallCtx::LeafStream& ls = vag_ctx().leaf_stream;      // the weight-gradient layout's side stream, if the step set one
        for (int lay = 0; lay < 4 && rc == VAG_OK; ++lay) {
            hipStream_t to = stream;
            if (lay == 0 && ls.stream && qn[0] > 0 && ls.stream != stream) {
                if (hipEventRecord(ls.event, stream) == hipSuccess && hipStreamWaitEvent(ls.stream, ls.event, 0) == hipSuccess) {
                    to = ls.stream;
                    ls.used = true;
                } else {
                    (void)hipGetLastError();
                }
            }
            rc = flush_layout(lay, to, to == stream);
        }
        if (--depth == 0 || rc != VAG_OK) {
            if (rc != VAG_OK) abort();
            else colsum_abort();           // bracket closed: later column sums launch at once
        }
        return rc;
    }
    // a product the leaf list can hold (rank-B weight gradient g_W += dY^T X, vectorised loads): taken (true) or left to the caller
    bool leaf_take(int64_t M, int64_t N, int64_t K, const float* A, int64_t sak, const float* B, int64_t sbk, float* C, int64_t ldc, float* rowsum) {
        if (!(vag_ctx().leaf_on && leaf.n < LEAF_MAX && M > 0 && N > 0 && K > 0 && K <= 128 && A && B && C && aligned16(A) && aligned16(B) &&
              sak % 4 == 0 && sbk % 4 == 0 && M < (1 << 20) && N < (1 << 20)))
            return false;
        const int k = leaf.n++;
        GemmArgs& g = leaf.g[k];
        g.A = A; g.B = B; g.C = C; g.bias = nullptr;
        g.sa_o = 1; g.sa_k = sak; g.sb_o = 1; g.sb_k = sbk; g.ldc = ldc;
        g.M = (int)M; g.N = (int)N; g.K = (int)K; g.kchunk = (int)(cdiv64(K, BK) * BK);
        g.alpha = 1.f; g.beta = 1.f; g.act = VAG_ACT_NONE; g.splitk = 1; g.c_half = 0; g.a_bf16 = 0; g.rowsum = rowsum;
        leaf.tiles_x[k] = (int)cdiv64(N, 64);
        leaf.tile0[k + 1] = leaf.tile0[k] + (int)(cdiv64(N, 64) * cdiv64(M, 64));
        return true;
    }
    bool leaf_attach_rowsum(const float* X, int64_t rows, int64_t N, int64_t ld, float* out) {
        if (!vag_ctx().leaf_on) return false;
        for (int k = 0; k < leaf.n; ++k) {
            GemmArgs& g = leaf.g[k];
            if (g.A == X && g.K == (int)rows && g.M == (int)N && g.sa_k == ld && !g.rowsum) { g.rowsum = out; return true; }
        }
        return false;
    }
    int leaf_flush(hipStream_t stream) {
        const bool was = vag_ctx().leaf_on;
        vag_ctx().leaf_on = false;
        const int n = leaf.n;
        if (!was || n == 0) { leaf.n = 0; return VAG_OK; }
        hipLaunchKernelGGL(gemm_tiled_multi_kernel, dim3((unsigned)leaf.tile0[n]), dim3(256), 0, stream, leaf);   // (n travels in the struct)
        leaf.n = 0;
        VAG_LAUNCH_CHECK();
        return VAG_OK;
    }
    void leaf_drop() { vag_ctx().leaf_on = false; leaf.n = 0; }
};
static thread_local GemmQueues g_queues;
void vag_gemm_group_begin() { g_queues.begin(); }
int vag_gemm_group_end(hipStream_t stream) { return g_queues.flush(stream); }
void vag_gemm_group_abort() { g_queues.abort(); }
int vag_leaf_flush(hipStream_t stream) { return g_queues.leaf_flush(stream); }
void vag_leaf_drop() { g_queues.leaf_drop(); }
bool vag_leaf_attach_rowsum(const float* X, int64_t rows, int64_t N, int64_t ld, float* out) { return g_queues.leaf_attach_rowsum(X, rows, N, ld, out); }
void vag_colsum_queue_begin() { g_queues.colsum_begin(); }
void vag_colsum_queue_abort() { g_queues.colsum_abort(); }
int vag_colsum_queue_flush(hipStream_t stream) { return g_queues.colsum_flush(stream); }

// ---- entry points: a product goes to the leaf list, into the open group bracket, or out at once ----
static int gemm_product(int planes, bool may_queue, int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t sam, int64_t sak,
                        const float* B, int64_t sbk, int64_t sbn, float beta, float* C, int64_t ldc, const float* bias, int act,
                        hipStream_t stream, int c_half, float* rowsum, int a_bf16) {
    GemmQueues& Q = g_queues;
    if (sam == 1 && sbn == 1 && alpha == 1.f && beta == 1.f && !bias && act == VAG_ACT_NONE && !c_half && !a_bf16 &&
        Q.leaf_take(M, N, K, A, sak, B, sbk, C, ldc, rowsum))
        return VAG_OK;
    VAG_CHECK_ARG(M >= 0 && N >= 0 && K >= 0 && A && B && C);
    if (M == 0 || N == 0) return VAG_OK;
    VAG_CHECK_ARG(M < (1ll << 30) && N < (1ll << 30) && K < (1ll << 30));
    VAG_CHECK_ARG(sam == 1 || sak == 1);
    VAG_CHECK_ARG(sbk == 1 || sbn == 1);
    GemmArgs g;
    g.slab = nullptr; g.ticket = nullptr; g.nslices = 1;
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    const bool akc = (sak == 1);        // A: k contiguous
    const bool bkc = (sbk == 1);        // B: k contiguous
    g.sa_o = sam; g.sa_k = sak; g.sb_o = sbn; g.sb_k = sbk;
    g.ldc = ldc; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.kchunk = (int)K; g.splitk = 1;
    g.alpha = alpha; g.beta = beta; g.act = act; g.c_half = c_half; g.rowsum = rowsum; g.a_bf16 = a_bf16;
    const bool bracket = may_queue && Q.depth > 0;
    VAG_CHECK_ARG(!a_bf16 || (planes == 1 && !bracket && !rowsum));     // one-plane bf16 kernel, launched at once
    VAG_CHECK_ARG(!c_half || beta == 0.f);      // fp16 output: plain stores only (no split-K, no accumulation)
    VAG_CHECK_ARG(!rowsum || sam == 1);         // row sums ride on outer-contiguous A tiles only
    const int64_t lda = akc ? sam : sak, ldb = bkc ? sbn : sbk;
    const bool vec = aligned16(A) && aligned16(B) && (lda % 4 == 0) && (ldb % 4 == 0);
    const VagOptions& o = vag_opt();           // vag_set_option("gemm_f32mfma"): the bf16x6 bound test flips it
    const int lay = (akc ? 2 : 0) + (bkc ? 1 : 0);
    if (bracket && Q.qn[lay] < GROUP_MAX && vec && alpha == 1.f && (beta == 0.f || beta == 1.f) && act == VAG_ACT_NONE && M > 64 && N > 64 &&
        K >= 256 && !o.gemm_f32mfma && !o.gemm_nogroup) {
        // a row sum that neither kernel the group may get would carry goes to the column-sum queue now
        const bool may_ride = gemm_rowsum_rides(GEMM_SPLIT128, planes, akc, false) ||
                              (gemm_big_fits(planes, M, N, o.gemm_big != 0) && gemm_rowsum_rides(GEMM_BIG256, planes, akc, false));
        if (g.rowsum && !may_ride) {
            VAG_TRY(vag_colsum_launch(A, K, M, sak, rowsum, stream));
            g.rowsum = nullptr;
        }
        Q.q[lay][Q.qn[lay]++] = g;
        return VAG_OK;
    }
    return gemm_launch_single(g, akc, bkc, vec, planes, stream);
}
int vag_gemm_launch(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t sam, int64_t sak,
                    const float* B, int64_t sbk, int64_t sbn, float beta, float* C, int64_t ldc,
                    const float* bias, int act, hipStream_t stream, int c_half, float* rowsum, int a_bf16) {
    return gemm_product(vag_ctx().gemm_planes, true, M, N, K, alpha, A, sam, sak, B, sbk, sbn, beta, C, ldc, bias, act, stream, c_half, rowsum,
                        a_bf16);
}
// One product launched at once (not queued into an open group bracket) with `planes` bf16 planes per operand.
int vag_gemm_launch_planes(int planes, int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t sam, int64_t sak,
                           const float* B, int64_t sbk, int64_t sbn, float beta, float* C, int64_t ldc, hipStream_t stream,
                           int a_bf16) {
    return gemm_product(planes, false, M, N, K, alpha, A, sam, sak, B, sbk, sbn, beta, C, ldc, nullptr, 0, stream, 0, nullptr, a_bf16);
}

// ---- column sums (launchers; kernels above) and transpose ----
int vag_colsum3_launch(const float* X, int64_t M, int64_t N, int64_t ld, float* out, float* out2, float* out3,
                       hipStream_t stream) {
    VAG_CHECK_ARG(X && out && M >= 0 && N >= 0);
    if (M == 0 || N == 0) return VAG_OK;
    if (!out2 && !out3 && vag_leaf_attach_rowsum(X, M, N, ld, out)) return VAG_OK;     // rides in the held-back product that reads X
    const int64_t nbx = cdiv64(N, 256);
    int64_t splits = cdiv64(1024, nbx);
    if (splits > cdiv64(M, 8)) splits = cdiv64(M, 8);
    if (splits < 1) splits = 1;
    const int rows_per = (int)cdiv64(M, splits);             // ~1024 blocks of 256 columns, none with fewer than 8 rows
    const unsigned gy = (unsigned)cdiv64(M, rows_per);
    GemmQueues& Q = g_queues;
    if (Q.colsum_on && Q.colsum_n < COLSUM_MAX && M < (1ll << 30) && N < (1ll << 30)) {
        const int k = Q.colsum_n++;
        ColsumTasks& t = Q.colsum;
        t.X[k] = X; t.out[k] = out; t.out2[k] = out2; t.out3[k] = out3; t.ld[k] = ld;
        t.M[k] = (int)M; t.N[k] = (int)N; t.rows_per[k] = rows_per;
        if ((unsigned)nbx > Q.colsum_gx) Q.colsum_gx = (unsigned)nbx;
        if (gy > Q.colsum_gy) Q.colsum_gy = gy;
        return VAG_OK;
    }
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)nbx, gy), dim3(256), 0, stream, X, (int)M, (int)N, ld, rows_per, out, out2, out3);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}
int vag_colsum_launch(const float* X, int64_t M, int64_t N, int64_t ld, float* out, hipStream_t stream) {
    return vag_colsum3_launch(X, M, N, ld, out, nullptr, nullptr, stream);
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int M, int N,
                                                        float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int m = m0 + ty + i, n = n0 + tx;
        if (m < M && n < N) tile[ty + i][tx] = in[(int64_t)m * N + n];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int n = n0 + ty + i, m = m0 + tx;
        if (m < M && n < N) out[(int64_t)n * M + m] = tile[tx][ty + i];
    }
}

int vag_transpose_launch(const float* in, int64_t M, int64_t N, float* out, hipStream_t stream) {
    VAG_CHECK_ARG(in && out && M > 0 && N > 0);
    dim3 grid((unsigned)cdiv64(N, 32), (unsigned)cdiv64(M, 32));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, stream, in, (int)M, (int)N, out);
    VAG_LAUNCH_CHECK();
    return VAG_OK;
}

