// Host layer of the cGRU decoder (include/vag_nmt.h: vag_gru_cell_*, the stand-alone attention, vag_cgru_*, vag_derive_weights).
// Host code only: the kernels are persist.hip's, skinny.hip's, attn.hip's, gemm.hip's and elem.hip's.  A sequence entry point checks
// its arguments, makes the call's DecSeq, enqueues what every path shares and hands the recurrence to ONE path function, each a plain
// list of launches (dec_fwd_one_launch / _hoisted_chain / _free_chain, dec_bwd_one_launch / _chain).  Nothing here allocates or
// synchronises.
#include "api_shared.h"
#include "seq_layout.h"

// ---------------- single GRU cell step (torch nn.GRU on a length-1 sequence: layers/NMT_Decoder.py:121,129) ----------------
// Arguments of ONE cell on M rows: h_out = cell(gi, h_prev) with the hidden projection h_prev W_hh^T + b_hh formed in the launch
static GruStepArgs gru_cell_args(const float* gi, const float* h_prev, const float* w_hh, const float* b_hh, int64_t M, int64_t H,
                                 float* h_out, float* save) {
    GruStepArgs a = {};
    a.lda = H; a.ldw = H; a.ldother = 3 * H; a.ldh = H; a.ld2 = 0;
    a.M = (int)M; a.K = (int)H; a.H = (int)H; a.lengths = nullptr; a.comp_hidden = 1;
    a.s[0].A = h_prev; a.s[0].W = w_hh; a.s[0].bias = b_hh; a.s[0].other = gi; a.s[0].hprev = h_prev;
    a.s[0].hout = h_out; a.s[0].out2 = nullptr; a.s[0].save = save; a.s[0].t = 0;
    return a;
}
int vag_gru_cell_fwd(const float* gi, const float* h_prev, const float* w_hh, const float* b_hh, int64_t M, int64_t H,
                     float* h_out, float* save, vag_stream_t stream) {
    VAG_CHECK_ARG(gi && h_prev && w_hh && b_hh && h_out && M > 0 && H > 0 && H % 4 == 0);
    return vag_gru_step_launch(gru_cell_args(gi, h_prev, w_hh, b_hh, M, H, h_out, save), 1, S_(stream));
}

// One backward step of a GRU recurrence (what torch autograd replays per time step for nn.GRU): the hidden-state
// gradient arriving through the later step's recurrent projection, plus the carried and the direct contributions, then
// the cell backward.  save = [4][M][H] (r, z, n, W_hn h + b_hn) as written by vag_gru_cell_fwd.
int vag_gru_cell_bwd(const float* dgh_next, const float* w_hh_t, const float* carry, const float* d_out, const float* save,
                     const float* h_prev, int64_t M, int64_t H, float* dgi, float* dgh, float* carry_out,
                     vag_stream_t stream) {
    VAG_CHECK_ARG(dgh_next && w_hh_t && save && h_prev && dgi && dgh && carry_out && M > 0 && H > 0 && H % 4 == 0);
    GruBwdStepArgs f = {};
    f.lda = 3 * H; f.ldw = 3 * H; f.ld_add = H; f.ldh = H; f.ldgi = 3 * H; f.ldgh = 3 * H;
    f.M = (int)M; f.K = (int)(3 * H); f.H = (int)H; f.lengths = nullptr; f.rng = nullptr; f.sid = 0; f.p = 0.f;
    f.has_cell = 1;
    GruBwdStepSide& sd = f.s[0];
    sd.A = dgh_next; sd.WT = w_hh_t; sd.addend = carry; sd.dh_add = d_out; sd.drop_idx0 = 0; sd.save = save;
    sd.hprev = h_prev; sd.dgi = dgi; sd.dgh = dgh; sd.dh_direct = carry_out; sd.dh_out = nullptr; sd.t = 0;
    return vag_gru_bwd_step_launch(f, 1, S_(stream));
}

// ---------------- attention keys ----------------
int vag_attn_keys_proj(const float* enc, const float* attn_e, int64_t rows, int64_t C, float* pe, vag_stream_t stream) {
    VAG_CHECK_ARG(enc && attn_e && pe && rows > 0 && C > 0);
    if (vag_ctx().store16)      // 2-byte storage mode: the keys are written as fp16
        return vag_gemm_launch(rows, C, C, 1.f, enc, C, 1, attn_e, 1, C, 0.f, pe, C, nullptr, 0, S_(stream), 1);
    return linear_fwd(rows, C, C, enc, C, attn_e, nullptr, 0, pe, C, S_(stream));
}
// a4 stand-alone (inference): alpha = softmax_s(v . tanh(pe_s + q)), ctx = sum_s alpha_s enc_s
int vag_bahdanau_attn_fwd(const float* pe, const float* q, const float* v, const float* mask, const float* enc, int64_t N,
                          int64_t rows_per_src, int64_t Ts, int64_t C, float* scores, float* alpha, float* ctx,
                          vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(pe && q && v && enc && scores && alpha && ctx);
    VAG_TRY(vag_attn_scores_launch(0, pe, q, C, v, mask, N, rows_per_src, Ts, C, scores, s));
    return vag_attn_ctx_launch(1, scores, enc, N, rows_per_src, Ts, C, alpha, ctx, s);
}
int vag_attn_keys_proj_bwd(const float* enc, const float* attn_e, const float* d_pe, int64_t rows, int64_t C, float* d_enc,
                           int accumulate_enc, float* g_attn_e, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && attn_e && d_pe && rows > 0 && C > 0);
    if (d_enc) VAG_TRY(gemm_nn(rows, C, C, d_pe, C, attn_e, C, accumulate_enc ? 1.f : 0.f, d_enc, C, s));
    if (g_attn_e) VAG_TRY(gemm_tn_acc(C, C, rows, d_pe, C, enc, C, g_attn_e, C, s));
    return VAG_OK;
}

// ---------------- cGRU decoder: derived weights ----------------
int64_t vag_cgru_prep_floats(int64_t H) { return cgru_prep(nullptr, H).total; }
int64_t vag_derived_floats(int64_t H) { return derived_layout(nullptr, H).total; }

static bool dec_w_ok(const vag_dec_w& w) {
    return w.emb && w.gru1.w_ih && w.gru1.w_hh && w.gru1.b_ih && w.gru1.b_hh && w.attn_h && w.attn_v && w.c2h &&
           w.gru2.w_ih && w.gru2.w_hh && w.gru2.b_ih && w.gru2.b_hh;
}

int vag_cgru_prepare(vag_dec_w w, int64_t H, float* prep, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(dec_w_ok(w) && prep && H > 0 && H % 4 == 0 && aligned16(prep));
    const int64_t C = 2 * H;
    CgruPrep p = cgru_prep(prep, H);
    VAG_TRY(copy_async(p.wcat, w.attn_h, C * H * sizeof(float), s));
    VAG_TRY(copy_async(p.wcat + C * H, w.gru2.w_hh, 3 * H * H * sizeof(float), s));
    VAG_TRY(zero_async(p.bcat, C * sizeof(float), s));
    VAG_TRY(copy_async(p.bcat + C, w.gru2.b_hh, 3 * H * sizeof(float), s));
    return gemm_nn(3 * H, C, H, w.gru2.w_ih, H, w.c2h, C, 0.f, p.wp, C, s);
}

// Everything the recurrences read that is a function of the parameters alone, refreshed once per optimiser step by a
// step driver (the stand-alone operators rebuild their share per call): [attn_h; W_hh2] stacked and transposed, the
// folded W_ih2 W_c2h, W_hh1^T, both encoder W_hh^T.  derived: vag_derived_floats(H) floats.
int vag_derive_weights(vag_dec_w w, const float* enc_whh_fw, const float* enc_whh_bw, int64_t H, int with_fp16,
                       float* derived, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(dec_w_ok(w) && enc_whh_fw && enc_whh_bw && derived && H > 0 && H % 4 == 0 && aligned16(derived));
    VAG_CHECK_ARG(!with_fp16 || H % 8 == 0);
    const int64_t C = 2 * H, Q = C + 3 * H;
    DerivedW d = derived_layout(derived, H);
    CgruPrep p = cgru_prep(d.prep, H);      // (wp stays unwritten: the one path that wants W_ih2 W_c2h, the free-running launch chain, forms it itself)
    const VagJob jobs[9] = {
        {w.attn_h, p.wcat, C, H, H, H, 1},                                 // wcat = [attn_h ; W_hh2]
        {w.gru2.w_hh, p.wcat + C * H, 3 * H, H, H, H, 1},
        {nullptr, p.bcat, 1, C, C, C, 0},                                  // bcat = [0 ; b_hh2]
        {w.gru2.b_hh, p.bcat + C, 1, 3 * H, 3 * H, 3 * H, 1},
        {w.attn_h, d.wcatT, C, H, H, Q, 2},                                // wcatT (H, C+3H) = [attn_h^T | W_hh2^T]
        {w.gru2.w_hh, d.wcatT + C, 3 * H, H, H, Q, 2},
        {w.gru1.w_hh, d.whh1T, 3 * H, H, H, 3 * H, 2},
        {enc_whh_fw, d.encT, 3 * H, H, H, 3 * H, 2},
        {enc_whh_bw, d.encT + 3 * H * H, 3 * H, H, H, 3 * H, 2},
    };
    VAG_TRY(vag_jobs_launch(jobs, 9, s));
    if (with_fp16) {        // fp16 copies of what the recurrences re-read every time step (2-byte storage mode)
        auto h = [&](vag_half* q) { return reinterpret_cast<float*>(q); };
        const VagJob j16[10] = {
            {w.attn_h, h(d.wcat16), C, H, H, H, 3},
            {w.gru2.w_hh, h(d.wcat16 + C * H), 3 * H, H, H, H, 3},
            {w.attn_h, h(d.wcatT16), C, H, H, Q, 4},
            {w.gru2.w_hh, h(d.wcatT16 + C), 3 * H, H, H, Q, 4},
            {w.gru1.w_hh, h(d.whh1_16), 3 * H, H, H, H, 3},
            {w.gru1.w_hh, h(d.whh1T16), 3 * H, H, H, 3 * H, 4},
            {enc_whh_fw, h(d.enc16), 3 * H, H, H, H, 3},
            {enc_whh_bw, h(d.enc16 + 3 * H * H), 3 * H, H, H, H, 3},
            {enc_whh_fw, h(d.encT16), 3 * H, H, H, 3 * H, 4},
            {enc_whh_bw, h(d.encT16 + 3 * H * H), 3 * H, H, H, 3 * H, 4},
        };
        VAG_TRY(vag_jobs_launch(j16, 10, s));
    }
    return VAG_OK;
}

// ---------------- cGRU decoder: what the sequence operators share ----------------
int64_t vag_cgru_ws_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H) { return cgru_ws(nullptr, B, Ts, Tt, E, H).total; }
// float offset of a saved per-step tensor inside the workspace (parity tests read them): 0 = alpha (Tt,B,Ts),
// 1 = h1 (Tt,B,H), 2 = [q | W_hh2 h1 + b] (Tt,B,C+3H)
int64_t vag_cgru_ws_offset(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int which) {
    static float base[1];
    CgruWs k = cgru_ws(base, B, Ts, Tt, E, H);
    const float* p = which == 0 ? k.alpha : which == 1 ? k.h1 : which == 2 ? k.qhp : nullptr;
    return p ? (int64_t)(p - base) : -1;
}
int64_t vag_cgru_bwd_scratch_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H) { return cgru_bwd_scratch(nullptr, B, Ts, Tt, E, H).total; }

// One sequence-level call of the decoder, forward or backward: shapes, the carved workspace, the derived weights in force and the
// storage mode.  Host side only: dec_seq enqueues nothing.
struct DecSeq {
    int64_t B, Ts, Tt, E, H;
    CgruWs k;
    CgruPrep p;         // Wcat / bcat / Wp: the driver's derived buffer, else this workspace's (a forward fills it: vag_cgru_prepare)
    bool s16;           // 2-byte storage mode
    DerivedW dw;        // the derived buffer's regions, its fp16 copies among them; all NULL without one
};
static DecSeq dec_seq(float* ws, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H) {
    DecSeq d = {B, Ts, Tt, E, H, cgru_ws(ws, B, Ts, Tt, E, H), {}, vag_ctx().store16, {}};
    if (vag_ctx().derived) d.dw = derived_layout(const_cast<float*>(vag_ctx().derived), H);
    d.p = cgru_prep(vag_ctx().derived ? d.dw.prep : d.k.prep, H);
    return d;
}

// Buffers of one decoder step on N rows (training: step t's slices of the sequence arrays, dec_step_view; decoding: the step's own)
struct DecStep {
    float* xp1;         // (N,3H) input projection of gru_1 (bias included)
    const float* hprev; // (N,H)
    float *h1, *g1, *g2, *qhp, *scores, *alpha, *c, *h2;
};
static DecStep dec_step_view(const DecSeq& d, int64_t t, const float* h0, float* h2_all, float* c_all) {
    const CgruWs& k = d.k;
    const int64_t B = d.B, H = d.H, C = 2 * H, Q = C + 3 * H, BH = B * H;
    DecStep b;
    b.xp1 = k.xp1 + t * B * 3 * H;
    b.hprev = t == 0 ? h0 : h2_all + (t - 1) * BH;
    b.h1 = k.h1 + t * BH; b.g1 = k.g1 + t * 4 * BH; b.g2 = k.g2 + t * 4 * BH;
    b.qhp = k.qhp + t * B * Q; b.scores = k.scores; b.alpha = k.alpha + t * B * d.Ts;
    b.c = c_all ? c_all + t * B * C : nullptr; b.h2 = h2_all + t * BH;
    return b;
}

// The keys as gru_2 sees them (NMT_Decoder.py:127-129 hoisted): context2hid on the keys, then W_ih2 on the H-wide result -- 6.7
// instead of 9.6 GFLOP at configs[1] against the one product through W_ih2 W_c2h, and the per-optimiser-step product that forms
// W_ih2 W_c2h is gone (exact in real arithmetic; the reference's own order).  Two group brackets: the first closes behind uk and
// sends it out together with whatever the caller's own open bracket holds (the group is the caller's products, then uk, then -- free
// running -- the head's keys encw2 = enc W2^T); the second is encwp alone, launched at once: the recurrence reads it.
static int dec_project_keys(const DecSeq& d, const float* enc, const vag_dec_w& w, const float* w2, float* encw2, hipStream_t s) {
    const int64_t B = d.B, Ts = d.Ts, H = d.H, C = 2 * H;
    {
        VagGemmGroup grp;
        VAG_TRY(vag_gemm_launch(B * Ts, H, C, 1.f, enc, C, 1, w.c2h, 1, C, 0.f, d.k.uk, H, nullptr, 0, s));
        if (w2) VAG_TRY(vag_gemm_launch(B * Ts, d.E, C, 1.f, enc, C, 1, w2, 1, C, 0.f, encw2, d.E, nullptr, 0, s));
        VAG_TRY(grp.end(s));
    }
    VagGemmGroup grp2;
    VAG_TRY(vag_gemm_launch(B * Ts, 3 * H, H, 1.f, d.k.uk, H, 1, w.gru2.w_ih, 1, H, 0.f, d.k.encwp, 3 * H, nullptr, 0, s, d.s16 ? 1 : 0));
    return grp2.end(s);
}
// What a step needs of a token, for every vocabulary entry: the input projection of gru_1 (:118-121) and W3 e (:137).  Two products
// for the caller's open group bracket.
static int dec_token_tables(const vag_dec_w& w, const float* w3, const DecTables& tab, int64_t V, int64_t E, int64_t H, hipStream_t s) {
    VAG_TRY(vag_gemm_launch(V, 3 * H, E, 1.f, w.emb, E, 1, w.gru1.w_ih, 1, E, 0.f, tab.embp, 3 * H, w.gru1.b_ih, 0, s));
    return vag_gemm_launch(V, E, E, 1.f, w.emb, E, 1, w3, 1, E, 0.f, tab.embw3, E, nullptr, 0, s);
}

// One cGRU step for N rows (layers/NMT_Decoder.py:121-129): 5 launches.
static int cgru_step(const float* enc, const float* pe, const float* mask, int64_t rps, const vag_dec_w& w,
                     const CgruPrep& p, int64_t N, int64_t Ts, int64_t H, const DecStep& b, hipStream_t s) {
    const int64_t C = 2 * H, Q = C + 3 * H;
    GruStepArgs a = gru_cell_args(b.xp1, b.hprev, w.gru1.w_hh, w.gru1.b_hh, N, H, b.h1, b.g1);
    VAG_TRY(vag_gru_step_launch(a, 1, s));                                                         // gru_1        :121
    VAG_TRY(vag_skinny_launch(N, Q, H, b.h1, H, p.wcat, H, p.bcat, nullptr, 0, b.qhp, Q, 0, s));    // attn_h(h1) :47 | W_hh2 h1
    VAG_TRY(vag_attn_scores_launch(0, pe, b.qhp, Q, w.attn_v, mask, N, rps, Ts, C, b.scores, s));   // :47-51, :41-43
    VAG_TRY(vag_attn_ctx_launch(1, b.scores, enc, N, rps, Ts, C, b.alpha, b.c, s));                 // :44, :126
    a.lda = C; a.ldw = C; a.ldother = Q; a.K = (int)C; a.comp_hidden = 0;
    a.s[0].A = b.c; a.s[0].W = p.wp; a.s[0].bias = w.gru2.b_ih; a.s[0].other = b.qhp + C;
    a.s[0].hprev = b.h1; a.s[0].hout = b.h2; a.s[0].save = b.g2;
    VAG_TRY(vag_gru_step_launch(a, 1, s));                                                         // context2hid + gru_2 :127-129
    return VAG_OK;
}

// ---------------- cGRU decoder: forward over a sequence ----------------
// all Tt steps in ONE launch (persist.hip): weights in registers, keys in LDS, four exchanges per step
static int dec_fwd_one_launch(const DecSeq& d, const float* enc, const float* pe, const float* mask, const float* h0,
                              const vag_dec_w& w, float* h2_all, float* c_all, hipStream_t s) {
    const CgruWs& k = d.k;
    VAG_TRY(vag_dec_fwd_persistent_launch(pe, mask, h0, k.xp1, w.gru1.w_hh, w.gru1.b_hh, d.p.wcat, d.p.bcat, w.attn_v, k.encwp,
                                          w.gru2.b_ih, k.h1, k.g1, k.qhp, k.alpha, h2_all, k.g2, k.psc, k.sync, d.B, d.Ts, d.Tt, d.H,
                                          s));
    return vag_attn_wsum_launch(1, k.alpha, enc, d.B, d.Ts, d.Tt, 2 * d.H, c_all, s);                       // all contexts :126
}
// Teacher forcing, a launch chain: the step with the context projection hoisted (4 launches, see attn_ctx_gru_kernel; fp32
// and 2-byte storage): the cell only needs sum_s alpha_s (W_ih2 W_c2h enc_s), the contexts themselves are formed for all steps after the loop.
static int dec_fwd_hoisted_chain(const DecSeq& d, const float* enc, const float* pe, const float* mask, const float* h0,
                                 const vag_dec_w& w, float* h2_all, float* c_all, hipStream_t s) {
    const CgruWs& k = d.k;
    const CgruPrep& p = d.p;
    const int64_t B = d.B, Ts = d.Ts, H = d.H, C = 2 * H, Q = C + 3 * H;
    const bool s16 = d.s16;
    for (int64_t t = 0; t < d.Tt; ++t) {
        const DecStep b = dec_step_view(d, t, h0, h2_all, nullptr);
        const GruStepArgs a = gru_cell_args(b.xp1, b.hprev, s16 ? as_f(d.dw.whh1_16) : w.gru1.w_hh, w.gru1.b_hh, B, H, b.h1, b.g1);
        VAG_TRY(vag_gru_step_launch(a, 1, s, s16));                                                         // gru_1 :121
        if (s16) {
            VAG_TRY(vag_skinny_launch(B, C, H, b.h1, H, as_f(d.dw.wcat16), H, nullptr, nullptr, 0, b.qhp, Q, 0, s, true));  // :47
            VAG_TRY(vag_attn_dot_side_launch(0, pe, b.qhp, Q, w.attn_v, mask, nullptr, B, Ts, C, k.scores, B, 3 * H, H, b.h1, H,
                                             as_f(d.dw.wcat16 + C * H), H, p.bcat + C, nullptr, b.qhp + C, Q, s, true));
            VAG_TRY(vag_attn_ctx_gru_launch(k.scores, k.encwp, B, 1, Ts, H, w.gru2.b_ih, b.qhp + C, Q, b.h1, b.alpha, b.h2, b.g2, s,
                                            true));
            continue;
        }
        if (Ts * B < (1ll << 28)) {
            // q = attn_h h1, then the scores with W_hh2 h1 + b_hh2 (not needed before the cell) in the same grid
            VAG_TRY(vag_skinny_launch(B, C, H, b.h1, H, p.wcat, H, nullptr, nullptr, 0, b.qhp, Q, 0, s));                  // :47
            VAG_TRY(vag_attn_dot_side_launch(0, pe, b.qhp, Q, w.attn_v, mask, nullptr, B, Ts, C, k.scores, B, 3 * H, H, b.h1, H,
                                             p.wcat + C * H, H, p.bcat + C, nullptr, b.qhp + C, Q, s));                     // :47-51, :41-43
        } else {
            VAG_TRY(vag_skinny_launch(B, Q, H, b.h1, H, p.wcat, H, p.bcat, nullptr, 0, b.qhp, Q, 0, s));         // attn_h(h1) | W_hh2 h1
            VAG_TRY(vag_attn_scores_launch(0, pe, b.qhp, Q, w.attn_v, mask, B, 1, Ts, C, k.scores, s));         // :47-51, :41-43
        }
        VAG_TRY(vag_attn_ctx_gru_launch(k.scores, k.encwp, B, 1, Ts, H, w.gru2.b_ih, b.qhp + C, Q, b.h1, b.alpha, b.h2, b.g2, s));   // :44, :126-129
    }
    return vag_attn_wsum_launch(1, k.alpha, enc, B, Ts, d.Tt, C, c_all, s);                                 // all contexts :126
}
// Free running, a launch chain: the head needs each context at once, so the step keeps its 5 launches (cgru_step), behind the
// token's embedding and input projection and in front of the head's step and the arg-max that picks the next token
static int dec_fwd_free_chain(const DecSeq& d, const float* enc, const float* pe, const float* mask, const float* h0, int64_t* tok,
                              const vag_dec_w& w, int64_t V, float* h2_all, float* c_all, float* e_all, const vag_head_w& head,
                              float p_out, const uint64_t* rng, float* tmid, float* logits, int64_t ldl, hipStream_t s) {
    const int64_t B = d.B, E = d.E, H = d.H, C = 2 * H;
    CgruPrep p = d.p;
    if (vag_ctx().derived) {
        // the step takes gru_2's input projection from the context through the folded product Wp = W_ih2 W_c2h (cgru_step); a
        // driver's derived buffer does not carry it any more: formed here, in this call's workspace
        VagGemmGroup now;
        p.wp = cgru_prep(d.k.prep, H).wp;
        VAG_TRY(gemm_nn(3 * H, C, H, w.gru2.w_ih, H, w.c2h, C, 0.f, p.wp, C, s));
        VAG_TRY(now.end(s));
    }
    for (int64_t t = 0; t < d.Tt; ++t) {
        const DecStep b = dec_step_view(d, t, h0, h2_all, c_all);
        float* e = e_all + t * B * E;
        if (B <= 256 && aligned16(w.emb) && aligned16(w.gru1.w_ih) && aligned16(e_all)) {
            // embedding lookup + input projection of gru_1 in one launch
            VAG_TRY(vag_skinny_gather_launch(B, 3 * H, E, w.emb, E, tok + t * B, w.gru1.w_ih, E, w.gru1.b_ih, b.xp1, 3 * H, e, E, s));
        } else {
            VAG_TRY(vag_embed_gather_launch(tok + t * B, B, 1, 1, B, w.emb, E, e, nullptr, 0, 0.f, s));
            VAG_TRY(vag_skinny_launch(B, 3 * H, E, e, E, w.gru1.w_ih, E, w.gru1.b_ih, nullptr, 0, b.xp1, 3 * H, 0, s));
        }
        VAG_TRY(cgru_step(enc, pe, mask, 1, w, p, B, d.Ts, H, b, s));
        VAG_TRY(vag_head_step(b.h2, b.c, e, head, B, E, H, V, p_out, rng, t * B * E, d.k.tmp, tmid + t * B * E, logits + t * B * ldl,
                              ldl, s));
        // next input = argmax of this step's distribution (V11.py:157), written to tok row t+1
        VAG_TRY(vag_lse_nll_launch(logits + t * B * ldl, ldl, B, V, nullptr, 0, 0, nullptr, nullptr, nullptr, tok + (t + 1) * B, 1,
                                   nullptr, 0, s, 0.f));
    }
    return VAG_OK;
}

int vag_cgru_attn_decode_seq_fwd(const float* enc, const float* pe, const float* mask, const float* h0, int64_t* tok,
                                 vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V,
                                 float* h2_all, float* c_all, float* e_all, float* ws, int free_run,
                                 const vag_head_w* head, float p_out, const uint64_t* rng, float* tmid, float* logits,
                                 int64_t ldl, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && pe && mask && h0 && tok && h2_all && c_all && e_all && ws && dec_w_ok(w));
    VAG_CHECK_ARG(B > 0 && Ts > 0 && Tt > 0 && E % 4 == 0 && H % 4 == 0 && E > 0 && H > 0 && aligned16(ws));
    VAG_CHECK_ARG(!free_run || (head && tmid && logits && ldl >= V && ldl % 4 == 0));
    const DecSeq d = dec_seq(ws, B, Ts, Tt, E, H);
    // Teacher forcing runs the hoisted step; free running keeps the 5-launch step.  Backward is common to both and always works
    // on the projected keys.
    const bool hoist = !free_run;
    // 2-byte storage mode: teacher-forced (hoisted) path only, weights from the driver's derived buffer
    VAG_CHECK_ARG(!d.s16 || (hoist && vag_ctx().derived && H % 8 == 0 && Ts * B < (1ll << 28)));
    if (!vag_ctx().derived) VAG_TRY(vag_cgru_prepare(w, H, d.k.prep, stream));
    {
        VagGemmGroup grp;       // (closed by dec_project_keys' first bracket: the input projection and uk are one grouped launch)
        if (hoist) {
            // every input token is known -> embed and project all steps at once
            if (!vag_ctx().step_gathered) VAG_TRY(vag_embed_gather_launch(tok, B, 1, Tt, B, w.emb, E, e_all, nullptr, 0, 0.f, s));
            VAG_TRY(vag_gemm_launch(Tt * B, 3 * H, E, 1.f, e_all, E, 1, w.gru1.w_ih, 1, E, 0.f, d.k.xp1, 3 * H, w.gru1.b_ih, 0, s));
        }
        VAG_TRY(dec_project_keys(d, enc, w, nullptr, nullptr, s));
        VAG_TRY(grp.end(s));
    }
    if (!hoist) return dec_fwd_free_chain(d, enc, pe, mask, h0, tok, w, V, h2_all, c_all, e_all, *head, p_out, rng, tmid, logits, ldl, s);
    if (hoist && !d.s16 && vag_opt().persistent && vag_dec_persistent_ok(B, Ts, Tt, H))
        return dec_fwd_one_launch(d, enc, pe, mask, h0, w, h2_all, c_all, s);
    return dec_fwd_hoisted_chain(d, enc, pe, mask, h0, w, h2_all, c_all, s);
}

int vag_cgru_free_supported(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V) {
    return vag_opt().persistent && vag_opt().free_persistent && !vag_ctx().store16 && vag_dec_free_persistent_ok(B, Ts, Tt, E, H, V) ? 1 : 0;
}
int64_t vag_cgru_free_tables_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V) {
    return vag_dec_tables(nullptr, B, Ts, Tt, E, H, V).total;
}
int vag_cgru_attn_decode_free_fwd(const float* enc, const float* pe, const float* mask, const float* h0, int64_t* tok,
                                  vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V,
                                  float* h2_all, float* c_all, float* e_all, float* ws, const vag_head_w* head, float p_out,
                                  const uint64_t* rng, float* tmid, float* logits, int64_t ldl, float* tables,
                                  vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && pe && mask && h0 && tok && h2_all && ws && head && tmid && tables && dec_w_ok(w));
    VAG_CHECK_ARG(head->w1 && head->b1 && head->w2 && head->b2 && head->w3 && head->b3 && head->out_w && head->out_b);
    VAG_CHECK_ARG(vag_cgru_free_supported(B, Ts, Tt, E, H, V) && aligned16(ws) && aligned16(tables));
    VAG_CHECK_ARG(!logits || (ldl >= V && ldl % 4 == 0));
    const DecSeq d = dec_seq(ws, B, Ts, Tt, E, H);
    const CgruWs& k = d.k;
    if (!vag_ctx().derived) VAG_TRY(vag_cgru_prepare(w, H, k.prep, stream));
    const DecTables tab = vag_dec_tables(tables, B, Ts, Tt, E, H, V);
    {
        // what a step needs of a token or of a key, for every token and every key, as four products in one grouped launch:
        // the input projection of gru_1 (:118-121), W3 e (:137), the keys as gru_2 sees them (:127-129), W2 enc (:137)
        VagGemmGroup grp;       // (closed by dec_project_keys' first bracket)
        VAG_TRY(dec_token_tables(w, head->w3, tab, V, E, H, s));
        VAG_TRY(dec_project_keys(d, enc, w, head->w2, tab.encw2, s));
        VAG_TRY(grp.end(s));
    }
    VAG_TRY(vag_dec_free_persistent_launch(pe, mask, h0, w.gru1.w_hh, w.gru1.b_hh, d.p.wcat, d.p.bcat, w.attn_v, k.encwp, w.gru2.b_ih,
                                           k.h1, k.g1, k.qhp, k.alpha, h2_all, k.g2, k.psc, k.sync, tab, head->w1, head->b1,
                                           head->b2, head->b3, head->out_w, head->out_b, tmid, logits, ldl, tok, rng, p_out, B, Ts,
                                           Tt, E, H, V, s));
    if (c_all) VAG_TRY(vag_attn_wsum_launch(1, k.alpha, enc, B, Ts, Tt, 2 * H, c_all, s));                   // all contexts :126
    if (e_all) VAG_TRY(vag_embed_gather_launch(tok, B, 1, Tt, B, w.emb, E, e_all, nullptr, 0, 0.f, s));     // the inputs it chose
    return VAG_OK;
}

// ---------------- cGRU decoder: backward over a sequence ----------------
// What the two paths of the backward recurrence take besides the call's DecSeq and scratch: forward data, arriving gradients
struct DecBwdIo {
    const float *enc, *pe, *h0, *h2_all, *d_h2_all, *d_c_all;
    float* d_h0;
};
// The context reaches the loss through the head (d_c_all) and through gru_2's input projection.  The first part of
// d alpha does not depend on the recurrence: all steps at once, before the loop.  The second is taken on the
// projected keys, d alpha[b,s] += encwp[b,s,:] . dgi2[b,:], so no per-step product dc = dgi2 W is needed.
// per sentence b: dah[:, b, :] (Tt,Ts) = d_c_all[:, b, :] (Tt,C) enc[b]^T (C,Ts): B small products in one launch
static int dec_bwd_dah(const DecSeq& d, const CgruBwdScratch& z, const DecBwdIo& io, hipStream_t s) {
    const int64_t B = d.B, Ts = d.Ts, Tt = d.Tt, C = 2 * d.H;
    if (C % 4 == 0 && aligned16(io.enc) && aligned16(io.d_c_all) && B < 65536)
        return vag_skinny_batched_launch(B, Tt, Ts, C, io.d_c_all, B * C, C, io.enc, C, Ts * C, z.dah, B * Ts, Ts, s);
    return vag_attn_scores_ex_launch(1, io.enc, io.d_c_all, C, nullptr, nullptr, Tt * B, 1, B, Ts, C, nullptr, z.dah, s);
}
// the dah product, then the whole backward recurrence in ONE launch (persist.hip); k.dal holds d alpha
static int dec_bwd_one_launch(const DecSeq& d, const CgruBwdScratch& z, const DecBwdIo& io, const vag_dec_w& w, hipStream_t s) {
    const CgruWs& k = d.k;
    VAG_TRY(dec_bwd_dah(d, z, io, s));
    return vag_dec_bwd_persistent_launch(io.pe, k.encwp, w.attn_v, z.wcatT, z.whh1T, io.h0, io.h2_all, k.h1, k.g1, k.g2, k.qhp, k.alpha,
                                         io.d_h2_all, z.dah, z.dgi2, z.dqgh, z.ds, z.dgi1, z.dgh1, io.d_h0, k.dal,
                                         vag_ctx().handoff_planes, vag_ctx().handoff_planes ? vag_ctx().handoff_floats : 0,
                                         k.sync_b, d.B, d.Ts, d.Tt, d.H, s);      // (the launch takes the forms the buffer holds)
}
// A launch chain: gru_2's cell of the last step, the dah product, then four launches per step
static int dec_bwd_chain(const DecSeq& d, const CgruBwdScratch& z, const DecBwdIo& io, const vag_dec_w& w, hipStream_t s) {
    const CgruWs& k = d.k;
    const int64_t B = d.B, Ts = d.Ts, Tt = d.Tt, H = d.H, C = 2 * H, Q = C + 3 * H, BH = B * H;
    const bool s16 = d.s16;
    float* h2_all = const_cast<float*>(io.h2_all);       // (for the step views: read only here)
    {
        // gru_2 cell backward of the last step: nothing arrives from a later step
        GruBwdArgs a = {};
        a.ld_add = H; a.ldh = H; a.ldgi = 3 * H; a.ldgh = Q; a.M = (int)B; a.H = (int)H;
        const int64_t t = Tt - 1;
        const DecStep b = dec_step_view(d, t, io.h0, h2_all, nullptr);
        GruBwdSide& sd = a.s[0];
        sd.dh_carry = nullptr; sd.dh_add = io.d_h2_all + t * BH; sd.drop_idx0 = 0;
        sd.save = b.g2; sd.hprev = b.h1;
        sd.dgi = z.dgi2 + t * B * 3 * H; sd.dgh = z.dqgh + t * B * Q + C; sd.dh_prev = z.dh1d; sd.t = 0;
        VAG_TRY(vag_gru_bwd_elem_launch(a, 1, s));
    }
    VAG_TRY(dec_bwd_dah(d, z, io, s));
    GruBwdStepArgs f = {};
    f.ld_add = H; f.ldh = H; f.M = (int)B; f.H = (int)H; f.lengths = nullptr; f.rng = nullptr; f.sid = 0; f.p = 0.f;
    for (int64_t t = Tt - 1; t >= 0; --t) {
        const DecStep b = dec_step_view(d, t, io.h0, h2_all, nullptr);
        float* dgi2 = z.dgi2 + t * B * 3 * H;
        float* dqgh = z.dqgh + t * B * Q;
        // attention backward: d alpha ; softmax backward ; dq = sum_s ds v (1 - tanh^2)
        // ... in one grid with the hidden-side half of dh1 (dgh2 W_hh2 + z2*dh2), whose operand is already known
        const float* wside = s16 ? as_f(reinterpret_cast<const vag_half*>(z.wcatT) + C) : z.wcatT + C;
        VAG_TRY(vag_attn_dot_side_launch(1, k.encwp, dgi2, 3 * H, nullptr, nullptr, z.dah + t * B * Ts, B, Ts, 3 * H, z.dalpha,
                                         B, H, 3 * H, dqgh + C, Q, wside, Q, nullptr, z.dh1d, z.pbuf, H, s, s16));
        VAG_TRY(vag_attn_dq_launch(io.pe, b.qhp, Q, w.attn_v, b.alpha, z.dalpha, z.ds + t * B * Ts, B, Ts, C, dqgh, Q, s, s16));
        // dh1 = dq attn_h + (dgh2 W_hh2 + z2*dh2)   -> gru_1 cell backward of this step
        f.lda = Q; f.ldw = Q; f.K = (int)C; f.ldgi = 3 * H; f.ldgh = 3 * H; f.has_cell = 1;
        GruBwdStepSide& sd = f.s[0];
        sd.A = dqgh; sd.WT = z.wcatT; sd.addend = z.pbuf; sd.dh_add = nullptr; sd.drop_idx0 = 0;
        sd.save = b.g1; sd.hprev = b.hprev;
        sd.dgi = z.dgi1 + t * B * 3 * H; sd.dgh = z.dgh1 + t * B * 3 * H; sd.dh_direct = z.carry; sd.dh_out = nullptr; sd.t = 0;
        VAG_TRY(vag_gru_bwd_step_launch(f, 1, s, s16));
        // d h2[t-1] = dgh1 W_hh1 + z1*dh1 (+ head's d_h2[t-1])   -> gru_2 cell backward of step t-1 (or d_h0 at t = 0)
        f.lda = 3 * H; f.ldw = 3 * H; f.K = (int)(3 * H);
        sd.A = z.dgh1 + t * B * 3 * H; sd.WT = z.whh1T; sd.addend = z.carry;
        if (t > 0) {
            const int64_t t1 = t - 1;
            const DecStep b1 = dec_step_view(d, t1, io.h0, h2_all, nullptr);
            f.has_cell = 1; f.ldgi = 3 * H; f.ldgh = Q;
            sd.dh_add = io.d_h2_all + t1 * BH;
            sd.save = b1.g2; sd.hprev = b1.h1;
            sd.dgi = z.dgi2 + t1 * B * 3 * H; sd.dgh = z.dqgh + t1 * B * Q + C; sd.dh_direct = z.dh1d; sd.dh_out = nullptr;
        } else {
            f.has_cell = 0;
            sd.dh_add = nullptr; sd.save = nullptr; sd.hprev = nullptr; sd.dgi = nullptr; sd.dgh = nullptr;
            sd.dh_direct = nullptr; sd.dh_out = io.d_h0;
        }
        VAG_TRY(vag_gru_bwd_step_launch(f, 1, s, s16));
    }
    return VAG_OK;
}

int vag_cgru_attn_decode_seq_bwd_loop(const float* enc, const float* pe, const float* mask, const float* h0, const int64_t* tok,
                                 vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V,
                                 const float* h2_all, const float* c_all, const float* e_all, float* d_h2_all,
                                 float* d_c_all, const float* d_e_all, float* ws, float* d_enc_out, int accumulate_enc,
                                 float* d_pe, float* d_h0, float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && pe && mask && h0 && tok && h2_all && c_all && e_all && d_h2_all && d_c_all && ws && d_enc_out &&
                  d_pe && d_h0 && scratch && dec_w_ok(w));
    VAG_CHECK_ARG(B > 0 && Ts > 0 && Tt > 0 && E % 4 == 0 && H % 4 == 0 && aligned16(ws) && aligned16(scratch));
    (void)V; (void)mask; (void)d_e_all;
    const int64_t C = 2 * H, Q = C + 3 * H;
    const DecSeq d = dec_seq(ws, B, Ts, Tt, E, H);      // (without a derived buffer: Wcat / Wp from the forward call are still in the workspace)
    const CgruWs& k = d.k;
    CgruBwdScratch z = cgru_bwd_scratch(scratch, B, Ts, Tt, E, H);
    const bool s16 = d.s16;
    VAG_CHECK_ARG(!s16 || (vag_ctx().derived && H % 8 == 0));
    if (vag_ctx().derived) {
        z.wcatT = d.dw.wcatT; z.whh1T = d.dw.whh1T;
        if (s16) {      // the same two transposes as fp16 (element strides are unchanged)
            z.wcatT = const_cast<float*>(as_f(d.dw.wcatT16)); z.whh1T = const_cast<float*>(as_f(d.dw.whh1T16));
        }
    } else {
        // per-step products are written as x W^T, so transpose the (derived) weights once per call
        VAG_TRY(vag_transpose_launch(d.p.wcat, Q, H, z.wcatT, s));          // (H, C+3H) = [attn_h^T | W_hh2^T]
        VAG_TRY(vag_transpose_launch(w.gru1.w_hh, 3 * H, H, z.whh1T, s));   // (H, 3H)
    }
    const DecBwdIo io = {enc, pe, h0, h2_all, d_h2_all, d_c_all, d_h0};
    const bool persist = !s16 && vag_opt().persistent && vag_opt().persistent_dec_bwd && vag_dec_bwd_persistent_ok(B, Ts, Tt, H);
    if (persist) VAG_TRY(dec_bwd_one_launch(d, z, io, w, s));
    else VAG_TRY(dec_bwd_chain(d, z, io, w, s));
    // after the recurrence: everything that does not sit on its critical path, as large products
    VAG_TRY(vag_attn_post_bwd_launch(pe, k.qhp, Q, w.attn_v, z.ds, k.alpha, d_c_all, B, Ts, Tt, C, d_pe, z.dvp, d_enc_out,
                                     accumulate_enc, s, s16));
    // gru_2's share of d_enc, through the projected keys encwp = (enc W_c2h^T) W_ih2^T: du_t = dgi2_t W_ih2 for all steps (H wide),
    // d_uk[b,s] = sum_t alpha[t,b,s] du_t[b], d_enc += d_uk W_c2h.  (Rounds 2-4: d_enc += (sum_t alpha_t dgi2_t) (W_ih2 W_c2h), 8 GFLOP.)
    {
        VagGemmGroup now;       // du is read by the weighted sum right below: launched at once (with whatever was queued before)
        VAG_TRY(gemm_nn(Tt * B, H, 3 * H, z.dgi2, 3 * H, w.gru2.w_ih, H, 0.f, z.du_all, H, s));
        VAG_TRY(now.end(s));
    }
    // (in the same launch: u_t = sum_s alpha[t,b,s] uk[b,s] for all steps, which the weight-gradient function needs -- forward data only)
    VAG_TRY(vag_attn_wsum_pair_launch(k.alpha, z.du_all, H, z.duk, k.uk, H, z.u_all, B, Ts, Tt, s));
    vag_ctx().u_all_ready = z.u_all;      // (taken by the weight-gradient function of the same backward)
    return gemm_nn(B * Ts, C, H, z.duk, H, w.c2h, C, 1.f, d_enc_out, C, s);
}

// Parameter gradients of the decoder from the per-step tensors the loop left in `scratch` (large products; nothing
// downstream waits for them, so they may run on a side stream beside the encoder's backward recurrence).
int vag_cgru_attn_decode_seq_bwd_weights(const float* h0, const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt,
                                         int64_t E, int64_t H, const float* h2_all, const float* c_all, const float* e_all,
                                         const float* d_e_all, float* ws, vag_dec_g g, float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(h0 && tok && h2_all && c_all && e_all && ws && scratch && dec_w_ok(w));
    VAG_CHECK_ARG(g.emb && g.gru1.w_ih && g.gru1.w_hh && g.gru1.b_ih && g.gru1.b_hh && g.attn_h && g.attn_v && g.c2h &&
                  g.gru2.w_ih && g.gru2.w_hh && g.gru2.b_ih && g.gru2.b_hh);
    const int64_t C = 2 * H;
    CgruBwdScratch z = cgru_bwd_scratch(scratch, B, Ts, Tt, E, H);
    VagGemmGroup grp3;              // the independent K = Tt*B weight gradients go out as one grouped launch,
    VAG_TRY(vag_colsum_launch(z.dvp, VAG_POST_CHUNKS(Ts) * B, C, C, g.attn_v, s));      // the bias sums as another
    VAG_TRY(vag_cgru_bwd_weights_chunk(h0, tok, w, B, Ts, Tt, E, H, h2_all, c_all, e_all, d_e_all, ws, g, scratch, 0, Tt, true,
                                       s));
    VAG_TRY(grp3.end(s));      // z.dwp and z.de are complete from here on
    return vag_cgru_bwd_weights_scatter(tok, B, Ts, Tt, E, H, g, scratch, 0, Tt, s);
}

// Rows of the time steps [t0, t1).  The products are queued when the caller holds a group bracket; the embedding-gradient
// tail (d(embedded inputs) -> scatter) reads nothing the queued products write.
int vag_cgru_bwd_weights_chunk(const float* h0, const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                               int64_t H, const float* h2_all, const float* c_all, const float* e_all, const float* d_e_all,
                               float* ws, vag_dec_g g, float* scratch, int64_t t0, int64_t t1, bool first, hipStream_t s) {
    VAG_CHECK_ARG(0 <= t0 && t0 < t1 && t1 <= Tt);
    const int64_t C = 2 * H, Q = C + 3 * H, r0 = t0 * B, n = (t1 - t0) * B;
    CgruWs k = cgru_ws(ws, B, Ts, Tt, E, H);
    CgruBwdScratch z = cgru_bwd_scratch(scratch, B, Ts, Tt, E, H);
    const float* dqgh = z.dqgh + r0 * Q;
    const float* dgh2 = dqgh + C;        // (n,3H) row stride Q
    const float* dgi2 = z.dgi2 + r0 * 3 * H;
    const float* dgi1 = z.dgi1 + r0 * 3 * H;
    const float* dgh1 = z.dgh1 + r0 * 3 * H;
    const float* h1 = k.h1 + r0 * H;
    VAG_TRY(gemm_tn_acc(3 * H, H, n, dgh2, Q, h1, H, g.gru2.w_hh, H, s, g.gru2.b_hh));       // (each with its bias gradient)
    VAG_TRY(gemm_tn_acc(C, H, n, dqgh, Q, h1, H, g.attn_h, H, s));
    // gru_2's input side, gi2_t = W_ih2 u_t with u_t = W_c2h c_t = sum_s alpha[t,b,s] uk[b,s] (formed here for all steps by one
    // weighted sum): d W_ih2 += dgi2^T u (with the bias gradient), d W_c2h += du^T c  (du = dgi2 W_ih2: the loop function left it)
    if (first) {
        if (vag_ctx().u_all_ready != z.u_all) VAG_TRY(vag_attn_wsum_launch(1, k.alpha, k.uk, B, Ts, Tt, H, z.u_all, s));
        vag_ctx().u_all_ready = nullptr;        // (the loop function of the same backward left it: see there)
    }
    VAG_TRY(gemm_tn_acc(3 * H, H, n, dgi2, 3 * H, z.u_all + r0 * H, H, g.gru2.w_ih, H, s, g.gru2.b_ih));
    VAG_TRY(gemm_tn_acc(H, C, n, z.du_all + r0 * H, H, c_all + r0 * C, C, g.c2h, C, s));
    if (h0 + B * H == h2_all) {
        // caller keeps [h0, h2_all] in one buffer: the previous states of all steps are one (R,H) operand
        VAG_TRY(gemm_tn_acc(3 * H, H, n, dgh1, 3 * H, h0 + r0 * H, H, g.gru1.w_hh, H, s, g.gru1.b_hh));
    } else {
        if (t0 == 0) VAG_TRY(gemm_tn_acc(3 * H, H, B, dgh1, 3 * H, h0, H, g.gru1.w_hh, H, s, g.gru1.b_hh));
        const int64_t skip = t0 == 0 ? B : 0;
        if (n > skip)
            VAG_TRY(gemm_tn_acc(3 * H, H, n - skip, dgh1 + skip * 3 * H, 3 * H, h2_all + (r0 + skip - B) * H, H, g.gru1.w_hh, H,
                                s, g.gru1.b_hh));      // (the two row ranges add their own shares of the bias gradient)
    }
    VAG_TRY(gemm_tn_acc(3 * H, E, n, dgi1, 3 * H, e_all + r0 * E, E, g.gru1.w_ih, E, s, g.gru1.b_ih));
    // d(embedded inputs) = dgi1 W_ih1 (+ the head's W3 path), scattered into the embedding gradient
    // (z.de: the sum; a caller that hands over d_e_all with the scratch's own address -- the step driver, whose head backward
    // writes there -- saves the copy)
    float* de = z.de + r0 * E;
    if (d_e_all && d_e_all != z.de) VAG_TRY(copy_async(de, d_e_all + r0 * E, n * E * sizeof(float), s));
    VAG_TRY(gemm_nn(n, E, 3 * H, dgi1, 3 * H, w.gru1.w_ih, E, d_e_all ? 1.f : 0.f, de, E, s));
    return VAG_OK;
}
// After every chunk's products have been LAUNCHED (group brackets closed): the embedding scatter of [t0, t1)
int vag_cgru_bwd_weights_scatter(const int64_t* tok, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, vag_dec_g g,
                                 float* scratch, int64_t t0, int64_t t1, hipStream_t s) {
    CgruBwdScratch z = cgru_bwd_scratch(scratch, B, Ts, Tt, E, H);
    return vag_embed_scatter_launch(tok + t0 * B, B, 1, t1 - t0, B, z.de + t0 * B * E, E, g.emb, nullptr, 0, 0.f, s);
}

int vag_cgru_attn_decode_seq_bwd(const float* enc, const float* pe, const float* mask, const float* h0, const int64_t* tok,
                                 vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V,
                                 const float* h2_all, const float* c_all, const float* e_all, float* d_h2_all,
                                 float* d_c_all, const float* d_e_all, float* ws, float* d_enc_out, int accumulate_enc,
                                 float* d_pe, float* d_h0, vag_dec_g g, float* scratch, vag_stream_t stream) {
    VAG_TRY(vag_cgru_attn_decode_seq_bwd_loop(enc, pe, mask, h0, tok, w, B, Ts, Tt, E, H, V, h2_all, c_all, e_all, d_h2_all,
                                              d_c_all, d_e_all, ws, d_enc_out, accumulate_enc, d_pe, d_h0, scratch, stream));
    return vag_cgru_attn_decode_seq_bwd_weights(h0, tok, w, B, Ts, Tt, E, H, h2_all, c_all, e_all, d_e_all, ws, g, scratch,
                                                stream);
}

// ---------------- cGRU decoder: one decoding step ----------------
int64_t vag_cgru_step_scratch_floats(int64_t N, int64_t Ts, int64_t, int64_t H) { return step_scratch(nullptr, N, Ts, H).total; }
int vag_cgru_attn_decode_step(const float* enc, const float* pe, const float* mask, int64_t rows_per_src, const int64_t* tok,
                              const float* h_in, vag_dec_w w, const float* prep, int64_t N, int64_t Ts, int64_t E, int64_t H,
                              float* h_out, float* c, float* e, float* alpha, float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && pe && mask && tok && h_in && h_out && c && e && alpha && scratch && prep && dec_w_ok(w));
    VAG_CHECK_ARG(N > 0 && Ts > 0 && E % 4 == 0 && H % 4 == 0 && rows_per_src >= 1 && aligned16(scratch) && aligned16(prep));
    CgruPrep p = cgru_prep(const_cast<float*>(prep), H);
    const StepScratch q = step_scratch(scratch, N, Ts, H);
    if (N <= 256 && aligned16(w.emb) && aligned16(w.gru1.w_ih) && aligned16(e)) {                          // :118, one launch
        VAG_TRY(vag_skinny_gather_launch(N, 3 * H, E, w.emb, E, tok, w.gru1.w_ih, E, w.gru1.b_ih, q.xp1, 3 * H, e, E, s));
    } else {
        VAG_TRY(vag_embed_gather_launch(tok, 1, 0, N, 1, w.emb, E, e, nullptr, 0, 0.f, s));
        VAG_TRY(linear_fwd(N, 3 * H, E, e, E, w.gru1.w_ih, w.gru1.b_ih, 0, q.xp1, 3 * H, s));
    }
    DecStep b;
    b.xp1 = q.xp1; b.hprev = h_in; b.h1 = q.h1; b.g1 = nullptr; b.g2 = nullptr; b.qhp = q.qhp; b.scores = q.scores;
    b.alpha = alpha; b.c = c; b.h2 = h_out;
    return cgru_step(enc, pe, mask, rows_per_src, w, p, N, Ts, H, b, s);
}

// The decoding step in its HOISTED form (round 4): what the training chain does since round 2 -- the keys as gru_2 sees them are
// projected once per call (encwp = (W_ih2 W_c2h) enc), so the second cell has no product left and rides as the epilogue of the
// softmax + weighted-sum kernel -- plus the head's share of the context as a second weighted sum in the same launch
// (cw = alpha . (enc W2^T)): the context itself is never formed.  Four launches instead of five, and the head's product over
// C = 2H columns is gone.  vag_cgru_decode_keys: once per decode call; `keys` = [encwp (B,Ts,3H) | encw2 (B,Ts,E)] (seq_layout.h).
int64_t vag_cgru_decode_keys_floats(int64_t B, int64_t Ts, int64_t E, int64_t H) { return dec_keys(nullptr, B, Ts, E, H).total; }
int vag_cgru_decode_keys(const float* enc, const float* prep, const float* w2, int64_t B, int64_t Ts, int64_t E, int64_t H,
                         float* keys, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && prep && w2 && keys && B > 0 && Ts > 0 && E % 4 == 0 && H % 4 == 0 && aligned16(keys) && aligned16(prep));
    const int64_t C = 2 * H;
    CgruPrep p = cgru_prep(const_cast<float*>(prep), H);
    const DecKeys k = dec_keys(keys, B, Ts, E, H);
    VagGemmGroup grp;
    VAG_TRY(vag_gemm_launch(B * Ts, 3 * H, C, 1.f, enc, C, 1, p.wp, 1, C, 0.f, k.encwp, 3 * H, nullptr, 0, s));
    VAG_TRY(vag_gemm_launch(B * Ts, E, C, 1.f, enc, C, 1, w2, 1, C, 0.f, k.encw2, E, nullptr, 0, s));
    return grp.end(s);
}
// ... and the step's token tables (seq_layout.h: step_tables), once per call
int64_t vag_cgru_decode_tables_floats(int64_t V, int64_t E, int64_t H) { return step_tables(nullptr, V, E, H).total; }
int vag_cgru_decode_tables(vag_dec_w w, const float* w3, int64_t V, int64_t E, int64_t H, float* tables, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(dec_w_ok(w) && w3 && tables && V > 0 && E % 4 == 0 && H % 4 == 0 && aligned16(tables));
    VagGemmGroup grp;
    VAG_TRY(dec_token_tables(w, w3, step_tables(tables, V, E, H), V, E, H, s));
    return grp.end(s);
}
int vag_cgru_attn_decode_step_h(const float* pe, const float* mask, const float* keys, const float* tables, int64_t V,
                                int64_t rows_per_src, const int64_t* tok, const float* h_in, vag_dec_w w, const float* prep,
                                int64_t N, int64_t Ts, int64_t E, int64_t H, float* h_out, float* cw, float* e, float* alpha,
                                float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(pe && mask && keys && tok && h_in && h_out && cw && (e || tables) && alpha && scratch && prep && dec_w_ok(w));
    VAG_CHECK_ARG(!tables || (V > 0 && aligned16(tables)));
    VAG_CHECK_ARG(N > 0 && N <= 256 && Ts > 0 && E % 4 == 0 && H % 4 == 0 && rows_per_src >= 1 && N % rows_per_src == 0 &&
                  aligned16(scratch) && aligned16(prep) && aligned16(keys) && aligned16(w.emb) && aligned16(w.gru1.w_ih) && aligned16(e));
    const int64_t C = 2 * H, Q = C + 3 * H, Bs = N / rows_per_src;
    CgruPrep p = cgru_prep(const_cast<float*>(prep), H);
    const float* encw2 = dec_keys(const_cast<float*>(keys), Bs, Ts, E, H).encw2;
    const StepScratch q = step_scratch(scratch, N, Ts, H);
    float *xp1 = q.xp1, *h1 = q.h1, *qhp = q.qhp;
    if (!tables) VAG_TRY(vag_skinny_gather_launch(N, 3 * H, E, w.emb, E, tok, w.gru1.w_ih, E, w.gru1.b_ih, xp1, 3 * H, e, E, s));      // :118
    // (with tables: gru_1's input projection is the line of embp that the row's token picks)
    GruStepArgs a = gru_cell_args(tables ? tables : xp1, h_in, w.gru1.w_hh, w.gru1.b_hh, N, H, h1, nullptr);
    a.s[0].other_idx = tables ? tok : nullptr;
    VAG_TRY(vag_gru_step_launch(a, 1, s));                                                                               // gru_1 :121
    // (the training chain lets W_hh2 h1 ride in the score kernel's grid; at 192 rows the one (q | hp2) product + the plain score
    // kernel measured 3.5 us less than q + scores-with-rider: the rider is a long K loop of few workgroups)
    VAG_TRY(vag_skinny_launch(N, Q, H, h1, H, p.wcat, H, p.bcat, nullptr, 0, qhp, Q, 0, s));                  // attn_h(h1) :47 | W_hh2 h1 + b
    if (vag_attn_row_gru_ok(N, Ts, H, E) && aligned16(pe) && aligned16(w.attn_v) && aligned16(w.gru2.b_ih) && aligned16(h_out) &&
        aligned16(cw))                                                                                        // :47-51, :41-44, :126-129
        return vag_attn_row_gru_launch(pe, qhp, Q, w.attn_v, mask, keys, encw2, N, rows_per_src, Ts, H, E, w.gru2.b_ih, qhp + C, Q, h1,
                                       alpha, h_out, cw, s);
    VAG_TRY(vag_attn_scores_launch(0, pe, qhp, Q, w.attn_v, mask, N, rows_per_src, Ts, C, q.scores, s));      // :47-51, :41-43
    return vag_attn_ctx_gru_launch(q.scores, keys, N, rows_per_src, Ts, H, w.gru2.b_ih, qhp + C, Q, h1, alpha, h_out, nullptr, s,
                                   false, encw2, E, cw);                                                                 // :44, :126-129
}

// the one-launch teacher-forced recurrence on the caller's own buffers (measurement scripts and tests)
int vag_cgru_recurrence_fwd(const float* pe, const float* mask, const float* h0, const float* xp1, vag_dec_w w, const float* wcat,
                            const float* bcat, const float* encwp, int64_t B, int64_t Ts, int64_t Tt, int64_t H, float* h1,
                            float* g1, float* qhp, float* alpha, float* h2_all, float* g2, float* psc, void* sync,
                            vag_stream_t stream) {
    VAG_CHECK_ARG(dec_w_ok(w) && vag_dec_persistent_ok(B, Ts, Tt, H));
    return vag_dec_fwd_persistent_launch(pe, mask, h0, xp1, w.gru1.w_hh, w.gru1.b_hh, wcat, bcat, w.attn_v, encwp, w.gru2.b_ih, h1,
                                         g1, qhp, alpha, h2_all, g2, psc, reinterpret_cast<unsigned*>(sync), B, Ts, Tt, H,
                                         S_(stream));
}
