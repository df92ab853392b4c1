// The n-gram matching walk that mbr.hip (pairwise utilities) and corpus.hip (corpus BLEU statistics) share: a token row's span into
// LDS, the four tokens that end at a position, and the walk that counts, per position of the candidate, the positions of another
// row that carry the same 1..4-gram.  mbr.hip has the derivation of the scheme.
#pragma once
#include "kernels.h"

constexpr int64_t MBR_EOS = 3;
constexpr int MBR_MAX_L = 512;           // tokens per row (LDS: one candidate row, its ranks, one reference row per wave)
constexpr int MBR_WAVES = 4;
constexpr int MBR_PAD_H = -1, MBR_PAD_R = -2;

__device__ __forceinline__ void mbr_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// One wave copies a row's span (the tokens before the first EOS) into dst as int32 and pads it with MBR_PAD_R to the end of the
// 64-token chunk that holds the span's end (so a reader may run to the next multiple of four).  Returns the span's length.
// Nothing after the EOS's chunk is read; what follows the EOS inside it is loaded but never stored.
__device__ __forceinline__ int mbr_load_span(const int64_t* __restrict__ row, int L, int* dst, int lane) {
    int len = L;
    for (int base = 0; base < L; base += 64) {
        const int p = base + lane;
        const int64_t t = p < L ? row[p] : MBR_EOS;
        const unsigned long long stop = __ballot(p < L && t == MBR_EOS);
        const int end = stop ? base + (__ffsll(stop) - 1) : L;               // (uniform over the wave)
        dst[p] = p < end ? (int)t : MBR_PAD_R;                                // p < 64 ceil(L / 64) <= MBR_MAX_L
        if (stop) { len = end; break; }
    }
    return len;
}

// cnt[n-1] += #{q < lr (SELF: and q < p) : the n-gram ending at q in r equals (h0, h1, .., h_{n-1}) read backwards from p}.
template <bool SELF>
__device__ __forceinline__ void mbr_walk(const int* r, int lr, int p, int h0, int h1, int h2, int h3, int (&cnt)[4]) {
    int w1 = MBR_PAD_R, w2 = MBR_PAD_R, w3 = MBR_PAD_R;
    for (int q = 0; q < lr; q += 4) {
        const int4 t = *reinterpret_cast<const int4*>(r + q);                 // wave-uniform address: a broadcast read
        const int tok[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int w0 = tok[e];
            const bool e0 = (h0 == w0) && (!SELF || q + e < p);
            const bool e1 = e0 && h1 == w1;
            const bool e2 = e1 && h2 == w2;
            const bool e3 = e2 && h3 == w3;
            cnt[0] += e0; cnt[1] += e1; cnt[2] += e2; cnt[3] += e3;
            w3 = w2; w2 = w1; w1 = w0;
        }
    }
}

// the four tokens that end at position p of the candidate in hbuf (span length lh)
__device__ __forceinline__ void mbr_tail(const int* hbuf, int lh, int p, int& h0, int& h1, int& h2, int& h3) {
    const bool in = p < lh;
    h0 = in ? hbuf[p] : MBR_PAD_H;
    h1 = in && p >= 1 ? hbuf[p - 1] : MBR_PAD_H;
    h2 = in && p >= 2 ? hbuf[p - 2] : MBR_PAD_H;
    h3 = in && p >= 3 ? hbuf[p - 3] : MBR_PAD_H;
}
