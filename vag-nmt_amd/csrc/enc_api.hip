// Host layer of the bi-GRU encoder (include/vag_nmt.h: vag_bigru_*).  Host code only: the kernels are persist.hip's, skinny.hip's,
// gemm.hip's and elem.hip's.  An entry point checks its arguments, enqueues what every path shares and hands the recurrence to ONE
// path: a one-launch kernel of persist.hip, or the launch chain (enc_fwd_chain, enc_bwd_chain).  Nothing here allocates or synchronises.
#include "api_shared.h"
#include "seq_layout.h"

int64_t vag_bigru_ws_floats(int64_t B, int64_t Ts, int64_t E, int64_t H) { return bigru_ws(nullptr, B, Ts, E, H).total; }

// What the recurrence paths of one call share: shapes, the carved workspace, the storage mode
struct EncSeq {
    int64_t B, Ts, H;
    BiGruWs w;
    bool s16;
};

// one launch per time step (both directions in it), then the context dropout; w16: the fp16 W_hh pair in 2-byte mode, else NULL
static int enc_fwd_chain(const EncSeq& e, const vag_half* w16, const int32_t* lengths, const vag_gru_w& fw, const vag_gru_w& bw,
                         float p_ctx, const uint64_t* rng, float* enc, hipStream_t s) {
    const BiGruWs& w = e.w;
    const int64_t B = e.B, Ts = e.Ts, H = e.H, BH = B * H;
    const bool s16 = e.s16;
    {
        const VagJob zj[2] = {{nullptr, w.hst, B, H, H, H, 0}, {nullptr, w.hst + (Ts + 1) * BH, B, H, H, H, 0}};
        VAG_TRY(vag_jobs_launch(zj, 2, s));          // initial states of both directions (the one-launch kernels write them themselves)
    }
    GruStepArgs a = {};
    a.lda = H; a.ldw = H; a.ldother = 6 * H; a.ldh = H; a.ld2 = Ts * 2 * H;
    a.M = (int)B; a.K = (int)H; a.H = (int)H; a.lengths = lengths; a.comp_hidden = 1;
    for (int64_t k = 0; k < Ts; ++k) {
        for (int d = 0; d < 2; ++d) {
            const int64_t t = d == 0 ? k : Ts - 1 - k;
            const vag_gru_w& g = d == 0 ? fw : bw;
            float* hs = w.hst + d * (Ts + 1) * BH;
            GruSide& sd = a.s[d];
            sd.A = hs + k * BH; sd.W = s16 ? as_f(w16 + d * 3 * H * H) : g.w_hh; sd.bias = g.b_hh;
            sd.other = w.xp + t * B * 6 * H + d * 3 * H;
            sd.hprev = hs + k * BH; sd.hout = hs + (k + 1) * BH;
            sd.out2 = enc + t * 2 * H + d * H;
            sd.save = w.gates + (d * Ts + k) * 4 * BH;
            sd.t = (int)t;
        }
        VAG_TRY(vag_gru_step_launch(a, 2, s, s16));
    }
    return vag_dropout_apply_launch(enc, B * Ts * 2 * H, 0, rng, VAG_DROP_ENC_CTX, p_ctx, s);
}

int vag_bigru_seq_fwd(const int64_t* src, const int32_t* lengths, const float* emb, vag_gru_w fw, vag_gru_w bw, float p_emb,
                      float p_ctx, const uint64_t* rng, int64_t B, int64_t Ts, int64_t E, int64_t H, float* enc,
                      float* mask, float* ws, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(src && lengths && emb && enc && mask && ws && B > 0 && Ts > 0 && E > 0 && H > 0);
    VAG_CHECK_ARG(E % 4 == 0 && H % 4 == 0 && aligned16(ws) && aligned16(enc));
    VAG_CHECK_ARG(fw.w_ih && fw.w_hh && fw.b_ih && fw.b_hh && bw.w_ih && bw.w_hh && bw.b_ih && bw.b_hh);
    VAG_CHECK_ARG(!vag_ctx().store16 || (vag_ctx().derived && H % 8 == 0));
    const EncSeq e = {B, Ts, H, bigru_ws(ws, B, Ts, E, H), vag_ctx().store16 && vag_ctx().derived};
    const BiGruWs& w = e.w;
    const int64_t R = Ts * B;
    VAG_TRY(vag_embed_gather_launch(src, 1, Ts, Ts, B, emb, E, w.x, rng, VAG_DROP_ENC_EMB, p_emb, s, mask));    // (+ the source mask)
    VagGemmGroup grp0;              // both directions' input projections: one grouped launch
    VAG_TRY(vag_gemm_launch(R, 3 * H, E, 1.f, w.x, E, 1, fw.w_ih, 1, E, 0.f, w.xp, 6 * H, fw.b_ih, 0, s));
    VAG_TRY(vag_gemm_launch(R, 3 * H, E, 1.f, w.x, E, 1, bw.w_ih, 1, E, 0.f, w.xp + 3 * H, 6 * H, bw.b_ih, 0, s));
    VAG_TRY(grp0.end(s));
    const bool s16 = e.s16;
    if (!s16 && vag_opt().persistent && vag_enc_persistent_ok(B, Ts, H)) {
        // the whole recurrence, both directions, in ONE launch (persist.hip): W_hh stays in registers for all Ts steps
        // (the context dropout is applied as the kernel writes enc: no separate pass)
        // (with the caller's plane buffer, if one is set -- the fused step has one -- the state rows are handed off as planes)
        return vag_enc_fwd_persistent_launch(w.xp, fw.w_hh, bw.w_hh, fw.b_hh, bw.b_hh, lengths, w.hst, w.gates, enc,
                                             vag_ctx().handoff_planes, vag_ctx().handoff_planes ? vag_ctx().handoff_floats : 0, w.sync,
                                             rng, p_ctx, B, Ts, H, s);
    }
    const vag_half* w16 = s16 ? derived_layout(const_cast<float*>(vag_ctx().derived), H).enc16 : nullptr;
    if (s16 && vag_opt().persistent && vag_enc_wide16_ok(B, Ts, H) && B >= 64) {
        // 2-byte mode, wide batches: one launch, the fp16 weight slice of a workgroup in registers, four row tiles through
        // it per step; the fp16 copy of the states that the workgroups exchange lives in the backward's (still unused) dgh
        // (the context dropout is applied as the kernel writes enc, as in the fp32 kernel: no separate pass)
        return vag_enc_fwd_wide16_launch(w.xp, w16, w16 + 3 * H * H, fw.b_hh, bw.b_hh, lengths, w.hst, w.gates, enc,
                                         reinterpret_cast<vag_half*>(w.dgh), w.sync, rng, p_ctx, B, Ts, H, s);
    }
    return enc_fwd_chain(e, w16, lengths, fw, bw, p_ctx, rng, enc, s);
}

// The caller's buffer for the backward recurrence's hand-off planes (vag_set_handoff_planes), if it holds `need` floats; else
// NULL: the launch keeps the fp32 hand-off.  Not part of the operators' workspaces: their sizes and layouts are as they were.
static float* handoff_planes(int64_t need) {
    const VagCallCtx& c = vag_ctx();
    return (need > 0 && c.handoff_planes && c.handoff_floats >= need) ? c.handoff_planes : nullptr;
}
// one launch per processed step, both directions in it; whhT: both directions' W_hh^T, fp16 in 2-byte mode
static int enc_bwd_chain(const EncSeq& e, const float* whhT, const float* d_enc, const int32_t* lengths, const uint64_t* rng, float p_ctx,
                         float* d_xp, hipStream_t s) {
    const BiGruWs& w = e.w;
    const int64_t B = e.B, Ts = e.Ts, H = e.H, BH = B * H;
    const bool s16 = e.s16;
    int cur = 0;
    // the cell of processed step k of direction d (time t): what its backward reads and writes, in either argument form
    auto cell_of = [&](auto& sd, int d, int64_t k) {
        const int64_t t = d == 0 ? k : Ts - 1 - k;
        sd.dh_add = d_enc + t * 2 * H + d * H;
        sd.drop_idx0 = t * 2 * H + d * H;
        sd.save = w.gates + (d * Ts + k) * 4 * BH;
        sd.hprev = w.hst + (d * (Ts + 1) + k) * BH;
        sd.dgi = d_xp + t * B * 6 * H + d * 3 * H;
        sd.dgh = w.dgh + (d * Ts + k) * B * 3 * H;
        sd.t = (int)t;
    };
    // last processed step: plain elementwise cell backward (no gradient arrives from a later step)
    GruBwdArgs a = {};
    a.ld_add = Ts * 2 * H; a.ldh = H; a.ldgi = 6 * H; a.ldgh = 3 * H;
    a.M = (int)B; a.H = (int)H; a.lengths = lengths; a.rng = rng; a.sid = VAG_DROP_ENC_CTX; a.p = p_ctx;
    for (int d = 0; d < 2; ++d) {
        GruBwdSide& sd = a.s[d];
        cell_of(sd, d, Ts - 1);
        sd.dh_carry = nullptr;
        sd.dh_prev = w.carry + (d * 2 + cur) * BH;
    }
    VAG_TRY(vag_gru_bwd_elem_launch(a, 2, s));
    // every other step: dh = dgh[k] W_hh + z*dh[k]  fused with the cell backward of step k-1 (both directions / launch)
    GruBwdStepArgs f = {};
    f.lda = 3 * H; f.ldw = 3 * H; f.ld_add = Ts * 2 * H; f.ldh = H; f.ldgi = 6 * H; f.ldgh = 3 * H;
    f.M = (int)B; f.K = (int)(3 * H); f.H = (int)H; f.lengths = lengths; f.rng = rng; f.sid = VAG_DROP_ENC_CTX; f.p = p_ctx;
    f.has_cell = 1;
    for (int64_t k = Ts - 1; k >= 1; --k) {
        for (int d = 0; d < 2; ++d) {
            GruBwdStepSide& sd = f.s[d];
            cell_of(sd, d, k - 1);
            sd.A = w.dgh + (d * Ts + k) * B * 3 * H;
            sd.WT = s16 ? as_f(reinterpret_cast<const vag_half*>(whhT) + d * 3 * H * H) : whhT + d * 3 * H * H;
            sd.addend = w.carry + (d * 2 + cur) * BH;
            sd.dh_direct = w.carry + (d * 2 + (cur ^ 1)) * BH;
            sd.dh_out = nullptr;
        }
        VAG_TRY(vag_gru_bwd_step_launch(f, 2, s, s16));
        cur ^= 1;
    }
    return VAG_OK;
}

int vag_bigru_seq_bwd(const int64_t* src, const int32_t* lengths, vag_gru_w fw, vag_gru_w bw, float p_emb, float p_ctx,
                      const uint64_t* rng, int64_t B, int64_t Ts, int64_t E, int64_t H, float* d_enc, float* ws,
                      float* g_emb, vag_gru_g g_fw, vag_gru_g g_bw, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(src && lengths && d_enc && ws && g_emb && B > 0 && Ts > 0 && E % 4 == 0 && H % 4 == 0);
    VAG_CHECK_ARG(!vag_ctx().store16 || (vag_ctx().derived && H % 8 == 0));
    const EncSeq e = {B, Ts, H, bigru_ws(ws, B, Ts, E, H), vag_ctx().store16 && vag_ctx().derived};
    const BiGruWs& w = e.w;
    const int64_t R = Ts * B, BH = B * H;
    const bool s16 = e.s16;
    float* d_xp = w.xp;      // forward input projections are no longer needed (gates are saved)
    const float* whhT = w.whhT;
    if (s16) {
        whhT = as_f(derived_layout(const_cast<float*>(vag_ctx().derived), H).encT16);
    } else if (vag_ctx().derived) {
        whhT = derived_layout(const_cast<float*>(vag_ctx().derived), H).encT;
    } else {
        for (int d = 0; d < 2; ++d) {
            const vag_gru_w& g = d == 0 ? fw : bw;
            VAG_TRY(vag_transpose_launch(g.w_hh, 3 * H, H, w.whhT + d * 3 * H * H, s));
        }
    }
    const bool pers_on = vag_opt().persistent && vag_opt().persistent_enc_bwd;
    const bool wide16 = s16 && pers_on && vag_enc_wide16_ok(B, Ts, H) && B >= 64;
    const bool persist = wide16 || (!s16 && pers_on && (H == 512 || H == 256) && vag_enc_persistent_ok(B, Ts, H));
    if (wide16) {
        // 2-byte mode, wide batches: the twin of the forward's one-launch kernel (fp16 W_hh^T slice in registers, gate gradients
        // exchanged as fp16 x 2^12 -- what the chain's fp16-pipe product rounds them to)
        VAG_TRY(vag_enc_bwd_wide16_launch(reinterpret_cast<const vag_half*>(whhT), d_enc, w.gates, w.hst, lengths, rng, p_ctx, d_xp,
                                          w.dgh, reinterpret_cast<vag_half*>(w.gx), w.sync_b, B, Ts, H, s));
    } else if (persist) {
        // the whole backward recurrence, both directions, in ONE launch (persist.hip)
        VAG_TRY(vag_enc_bwd_persistent_launch(whhT, d_enc, w.gates, w.hst, lengths, rng, p_ctx, d_xp, w.dgh,
                                              handoff_planes(vag_enc_bwd_planes_floats(B, Ts, H)), w.sync_b, B, Ts, H, s));
    } else {
        VAG_TRY(enc_bwd_chain(e, whhT, d_enc, lengths, rng, p_ctx, d_xp, s));
    }
    VagGemmGroup grp1;      // the four weight gradients (both directions) go out as one grouped launch
    for (int d = 0; d < 2; ++d) {
        const vag_gru_g& gg = d == 0 ? g_fw : g_bw;
        const float* dgh = w.dgh + d * Ts * B * 3 * H;
        const float* hs = w.hst + d * (Ts + 1) * BH;
        VAG_TRY(gemm_tn_acc(3 * H, H, R, dgh, 3 * H, hs, H, gg.w_hh, H, s, gg.b_hh));                    // + bias gradient
        VAG_TRY(gemm_tn_acc(3 * H, E, R, d_xp + d * 3 * H, 6 * H, w.x, E, gg.w_ih, E, s, gg.b_ih));
    }
    VAG_TRY(grp1.end(s));
    // d(embedded inputs) = sum over the directions of dgi W_ih: both products add into a zeroed buffer, one grouped launch
    if (!vag_ctx().step_zeroed) VAG_TRY(zero_async(w.dx, R * E * sizeof(float), s));
    VagGemmGroup grp2;
    for (int d = 0; d < 2; ++d)
        VAG_TRY(gemm_nn(R, E, 3 * H, d_xp + d * 3 * H, 6 * H, (d == 0 ? fw : bw).w_ih, E, 1.f, w.dx, E, s));
    VAG_TRY(grp2.end(s));
    VAG_TRY(vag_embed_scatter_launch(src, 1, Ts, Ts, B, w.dx, E, g_emb, rng, VAG_DROP_ENC_EMB, p_emb, s,
                                     vag_ctx().poison_inject ? vag_persist_guard() : nullptr));
    return VAG_OK;
}
