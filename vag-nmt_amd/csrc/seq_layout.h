// Layouts of the caller-owned buffers of the sequence operators (enc_api.hip, dec_api.hip) and of what step.hip and head_api.hip
// read inside them: each a struct of region pointers and the function that carves it (kernels.h: WsCarver).  On a NULL base a
// layout yields NULL pointers and the same total: the *_floats queries of the ABI.  tests/golden/ws_layout.json pins every offset.
#pragma once
#include "kernels.h"

// ---------------- bi-GRU encoder workspace ----------------
struct BiGruWs {
    float *x, *xp, *hst, *gates, *dgh, *carry, *dx, *whhT, *gx;
    unsigned *sync, *sync_b;             // counters of the persistent recurrence kernels (persist.hip): forward, backward
    int64_t total;
};
static inline BiGruWs bigru_ws(float* ws, int64_t B, int64_t Ts, int64_t E, int64_t H) {
    BiGruWs w;
    WsCarver c(ws);
    w.x = c.take(Ts * B * E);              // embedded (+dropout) input, time-major (Ts,B,E)
    w.xp = c.take(Ts * B * 6 * H);         // input projections [fwd 3H | rev 3H]; reused as d_xp in backward
    w.hst = c.take(2 * (Ts + 1) * B * H);  // [dir][step][B][H] hidden states in processing order, step 0 = zeros
    w.gates = c.take(2 * Ts * 4 * B * H);  // [dir][step][r,z,n,hn][B][H]
    w.dgh = c.take(2 * Ts * B * 3 * H);    // backward: [dir][step][B][3H]
    w.carry = c.take(4 * B * H);           // backward: [dir][2][B][H]
    w.dx = c.take(Ts * B * E);             // backward: d(embedded input)
    w.whhT = c.take(2 * 3 * H * H);        // backward: W_hh^T per direction (H,3H)
    w.gx = c.take(3 * Ts * B * H);         // backward, 2-byte mode one-launch kernel: [dir][step][B][3H] fp16 copy of dgh for the exchange
    w.sync = c.take_as<unsigned>(vag_enc_persistent_sync_words(B, Ts));
    w.sync_b = c.take_as<unsigned>(vag_enc_persistent_sync_words(B, Ts));      // (adjacent: one range to zero)
    w.total = c.off;
    return w;
}

// ---------------- cGRU decoder: derived weights ----------------
// Per-call derived weights (vag_cgru_prepare): Wcat = [attn_h ; gru_2.w_hh] (C+3H,H) so that q = attn_h(h1) and the
// hidden projection of gru_2 come out of ONE product; bcat = [0 ; gru_2.b_hh]; Wp = gru_2.w_ih . context2hid (3H,C)
// so that gru_2's input projection is taken straight from the context (context2hid folded in; exact in real
// arithmetic, fp32 reassociation only).
struct CgruPrep {
    float *wcat, *bcat, *wp;
    int64_t total;
};
static inline CgruPrep cgru_prep(float* p, int64_t H) {
    CgruPrep w;
    const int64_t C = 2 * H, Q = C + 3 * H;
    WsCarver c(p);
    w.wcat = c.take(Q * H); w.bcat = c.take(Q); w.wp = c.take(3 * H * C);
    w.total = c.off;
    return w;
}
// Layout of the derived-weights buffer: [wcat | bcat | wp] (= CgruPrep), then the transposes the backward recurrences
// read: wcatT (H, C+3H), whh1T (H, 3H), encT (2 x (H, 3H): forward / reverse encoder W_hh^T).
struct DerivedW {
    float *prep, *wcatT, *whh1T, *encT;
    // fp16 copies for the 2-byte storage mode (element counts in halves; each region starts 256-byte aligned):
    // wcat16 (Q,H), wcatT16 (H,Q), whh1_16 (3H,H), whh1T16 (H,3H), enc16 (2 x (3H,H)), encT16 (2 x (H,3H))
    vag_half *wcat16, *wcatT16, *whh1_16, *whh1T16, *enc16, *encT16;
    int64_t total;
};
static inline DerivedW derived_layout(float* p, int64_t H) {
    DerivedW w;
    const int64_t C = 2 * H, Q = C + 3 * H;
    WsCarver c(p);
    w.prep = c.take(cgru_prep(nullptr, H).total); w.wcatT = c.take(Q * H); w.whh1T = c.take(3 * H * H); w.encT = c.take(2 * 3 * H * H);
    w.wcat16 = c.take_as<vag_half>(Q * H); w.wcatT16 = c.take_as<vag_half>(Q * H);
    w.whh1_16 = c.take_as<vag_half>(3 * H * H); w.whh1T16 = c.take_as<vag_half>(3 * H * H);
    w.enc16 = c.take_as<vag_half>(2 * 3 * H * H); w.encT16 = c.take_as<vag_half>(2 * 3 * H * H);
    w.total = c.off;
    return w;
}

// ---------------- cGRU decoder workspace ----------------
struct CgruWs {
    float *xp1, *h1, *g1, *g2, *qhp, *scores, *alpha, *tmp, *prep, *encwp;
    float* uk;                  // (B,Ts,H) enc W_c2h^T: context2hid applied to the keys once per batch (round 5: the projected keys are
                                // encwp = uk W_ih2^T -- two products through the H-wide intermediate instead of one through W_ih2 W_c2h)
    float* psc;                 // persistent decoder (persist.hip): the steps' scores as exchanged between workgroups (Tt,4,B,Ts)
    unsigned* sync;             // ... and its counters
    unsigned* sync_b;           // the backward kernel's counters ...
    float* dal;                 // ... and its d alpha accumulator (Tt,4,B,Ts)   [h1 .. dal: one range to zero]
    int64_t total;
};
static inline CgruWs cgru_ws(float* ws, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H) {
    CgruWs w;
    const int64_t C = 2 * H;
    WsCarver c(ws);
    w.xp1 = c.take(Tt * B * 3 * H);
    w.g1 = c.take(Tt * 4 * B * H);
    w.g2 = c.take(Tt * 4 * B * H);
    w.qhp = c.take(Tt * B * (C + 3 * H));     // [q | W_hh2 h1 + b_hh2] per step
    w.scores = c.take(B * Ts);
    w.alpha = c.take(Tt * B * Ts);
    w.tmp = c.take(B * E);
    w.prep = c.take(cgru_prep(nullptr, H).total);
    w.encwp = c.take(B * Ts * 3 * H);         // (W_ih2 W_c2h) enc[b,s,:]: the keys as gru_2 sees them, once per batch
    w.uk = c.take(B * Ts * H);
    w.h1 = c.take(Tt * B * H);                // (exchanged between workgroups with marked words: starts from zero, see step.hip: step_zero_ranges)
    w.psc = c.take(Tt * B * Ts * 4);          // four copies (persist.hip: ACC_SHARDS)
    w.sync = c.take_as<unsigned>(vag_dec_persistent_sync_words(B, Tt));
    w.sync_b = c.take_as<unsigned>(vag_dec_persistent_sync_words(B, Tt));
    w.dal = c.take(Tt * B * Ts * 4);
    w.total = c.off;
    return w;
}

// ---------------- cGRU decoder: backward scratch ----------------
// de: where the decoder's backward keeps d(embedded inputs) (R,E): a step driver lets the head's backward write its share straight
// there (vag_cgru_bwd_weights_chunk then adds gru_1's share without a copy)
struct CgruBwdScratch {
    float *wcatT, *wpT, *whh1T, *dgi2, *dqgh, *dalpha, *ds, *dgi1, *dgh1, *dh1d, *carry, *de, *dvp, *dwp, *dah, *dencwp, *pbuf;
    float *u_all, *du_all, *duk;          // (R,H) context2hid(c_t); (R,H) its gradient dgi2 W_ih2; (B,Ts,H) gradient of uk
    int64_t total;
};
static inline CgruBwdScratch cgru_bwd_scratch(float* p, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H) {
    CgruBwdScratch w;
    const int64_t C = 2 * H, Q = C + 3 * H, R = Tt * B;
    WsCarver c(p);
    w.wcatT = c.take(Q * H); w.wpT = c.take(3 * H * C); w.whh1T = c.take(3 * H * H);
    w.dgi2 = c.take(R * 3 * H); w.dqgh = c.take(R * Q);
    w.dalpha = c.take(B * Ts); w.ds = c.take(R * Ts);
    w.dgi1 = c.take(R * 3 * H); w.dgh1 = c.take(R * 3 * H);
    w.dh1d = c.take(B * H); w.carry = c.take(B * H); w.de = c.take(R * E); w.dvp = c.take(VAG_POST_CHUNKS(Ts) * B * C);
    w.dwp = c.take(3 * H * C);
    w.dah = c.take(R * Ts);                   // d alpha through the head's use of the context, all steps
    w.dencwp = c.take(B * Ts * 3 * H);        // gradient of the projected keys
    w.pbuf = c.take(B * H);                   // dgh2 W_hh2 + carry, computed beside the attention backward
    w.u_all = c.take(R * H); w.du_all = c.take(R * H); w.duk = c.take(B * Ts * H);
    w.total = c.off;
    return w;
}

// ---------------- decoding steps ----------------
// What the hoisted decoding step keeps per decode call (vag_cgru_decode_keys): keys = [encwp (B,Ts,3H) | encw2 (B,Ts,E)]
struct DecKeys {
    float *encwp, *encw2;
    int64_t total;
};
static inline DecKeys dec_keys(float* keys, int64_t B, int64_t Ts, int64_t E, int64_t H) {
    WsCarver c(keys);
    DecKeys k;
    k.encwp = c.take(B * Ts * 3 * H); k.encw2 = c.take(B * Ts * E);
    k.total = c.off;
    return k;
}
// ... and what a step needs of a TOKEN, for every vocabulary entry, once per call: tables = [emb W_ih1^T + b_ih1 (V,3H) | emb W3^T (V,E)]
// (the first two of the free-running recurrence kernel's tables: kernels.h, DecTables).  With them a step has no embedding / input-projection launch: gru_1 reads
// its input projection from the line its row's token picks, the head its share of the embedded token likewise.
static inline DecTables step_tables(float* tables, int64_t V, int64_t E, int64_t H) { return vag_dec_tables(tables, 0, 0, 0, E, H, V, true); }
// Scratch of one decoding step on N rows (either form): [xp1 (N,3H) | h1 (N,H) | qhp (N,C+3H) | scores (N,Ts)] back to back -- the
// one layout here that is not rounded to granules -- and 64 floats of slack in the total
struct StepScratch {
    float *xp1, *h1, *qhp, *scores;
    int64_t total;
};
static inline StepScratch step_scratch(float* p, int64_t N, int64_t Ts, int64_t H) {
    StepScratch w;
    const int64_t Q = 2 * H + 3 * H;
    int64_t off = 0;
    auto take = [&](int64_t n) { float* q = p ? p + off : nullptr; off += n; return q; };
    w.xp1 = take(N * 3 * H); w.h1 = take(N * H); w.qhp = take(N * Q); w.scores = take(N * Ts);
    w.total = off + 64;
    return w;
}
