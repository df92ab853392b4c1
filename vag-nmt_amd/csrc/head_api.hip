// Host layer of the output head (include/vag_nmt.h: vag_head_*): tanh(W1 h2 + W2 c + W3 e + biases) -> dropout -> vocabulary
// product -> log-sum-exp / NLL -> loss, and its backward.  Host code only: the kernels are head.hip's, gemm.hip's and skinny.hip's.
// A sequence-level call is one HeadSeq (kernels.h): every ABI entry point fills one, vag_train_step fills one and hands it to the
// forward and then to the backward.  Nothing here allocates or synchronises.
#include "api_shared.h"
#include "seq_layout.h"

// ---------------------------------------------------------------------------------------------------------------------
// one decoding step (N rows)
// ---------------------------------------------------------------------------------------------------------------------
// tmid = dropout(tanh(W1 h2 + W2 c + W3 e + biases)) in one launch (NMT_Decoder.py:137-141); N <= 256, operands 16-byte aligned
static int head_pre_step(const float* h2, const float* c, const float* e, const vag_head_w& w, int64_t N, int64_t E, int64_t H,
                         float p_out, const uint64_t* rng, int64_t drop_idx0, float* tmid, hipStream_t s) {
    const int64_t C = 2 * H;
    const float* A3[3] = {h2, c, e};
    const float* W3[3] = {w.w1, w.w2, w.w3};
    const float* B3[3] = {w.b1, w.b2, w.b3};
    const int64_t ld3[3] = {H, C, E}, K3[3] = {H, C, E};
    return vag_skinny3_launch(N, E, A3, ld3, W3, ld3, K3, B3, tmid, E, VAG_ACT_TANH, rng, VAG_DROP_DEC_OUT, p_out, drop_idx0, s);
}
// tmid for a step whose context share cw (N,E) = alpha . (enc W2^T) is at hand instead of the context (hoisted decoding step)
// embw3 / tok: W3 e as a table line (vag_cgru_decode_tables) instead of a product over the embedded token e
static int head_pre_step_h(const float* h2, const float* cw, const float* e, const float* embw3, const int64_t* tok,
                           const vag_head_w& w, int64_t N, int64_t E, int64_t H, float* tmid, hipStream_t s) {
    const float* A3[3] = {h2, nullptr, embw3 ? nullptr : e};
    const float* W3[3] = {w.w1, nullptr, embw3 ? nullptr : w.w3};
    const float* B3[3] = {w.b1, w.b2, w.b3};
    const int64_t ld3[3] = {H, 0, E}, K3[3] = {H, 0, embw3 ? 0 : E};
    return vag_skinny3_launch(N, E, A3, ld3, W3, ld3, K3, B3, tmid, E, VAG_ACT_TANH, nullptr, VAG_DROP_DEC_OUT, 0.f, 0, s, cw, E,
                              embw3, tok, E);
}
// tanh(W1 h2 + W2 c + W3 e + biases) -> dropout -> logits   for N rows of one step (NMT_Decoder.py:137-143)
int vag_head_step(const float* h2, const float* c, const float* e, const vag_head_w& w, int64_t N, int64_t E, int64_t H, int64_t V,
                  float p_out, const uint64_t* rng, int64_t drop_idx0, float* tmp, float* tmid, float* logits, int64_t ldl,
                  hipStream_t s) {
    const int64_t C = 2 * H;
    if (N <= 256 && aligned16(h2) && aligned16(c) && aligned16(e) && aligned16(w.w1) && aligned16(w.w2) && aligned16(w.w3)) {
        // one launch: the three products, the biases, tanh and the dropout multiplier (round 2; was four launches)
        VAG_TRY(head_pre_step(h2, c, e, w, N, E, H, p_out, rng, drop_idx0, tmid, s));
    } else {
        VAG_TRY(vag_skinny_launch(N, E, H, h2, H, w.w1, H, w.b1, nullptr, 0, tmp, E, 0, s));
        VAG_TRY(vag_skinny_launch(N, E, C, c, C, w.w2, C, w.b2, tmp, E, tmp, E, 0, s));
        VAG_TRY(vag_skinny_launch(N, E, E, e, E, w.w3, E, w.b3, tmp, E, tmid, E, VAG_ACT_TANH, s));
        VAG_TRY(vag_dropout_apply_launch(tmid, N * E, drop_idx0, rng, VAG_DROP_DEC_OUT, p_out, s));
    }
    return linear_fwd(N, V, E, tmid, E, w.out_w, w.out_b, 0, logits, ldl, s);
}
// rows of logits -> log-probabilities in place (no target, no loss), and the row's arg-max where asked for
static int head_logp_rows(float* logp, int64_t ldl, int64_t rows, int64_t V, int64_t* argmax, hipStream_t s) {
    return vag_lse_nll_launch(logp, ldl, rows, V, /*tgt, B, Tt, vw*/ nullptr, 0, 0, nullptr, /*lse, nll*/ nullptr, nullptr, argmax,
                              argmax ? 1 : 0, logp, ldl, s, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// the bundle's validator: each condition once; `need` says what an entry point is going to touch
// ---------------------------------------------------------------------------------------------------------------------
// HS_ACT: h2, c, e.  HS_W: the four matrices of vag_head_w, HS_B: b1, b2, b3, HS_OUT_B: out.bias (whoever forms logits).
// HS_TARGET: tgt, vocab_weight, lse, inv_cnt.  HS_LOSS: nll and a loss destination.  HS_D_OUT: d_h2, d_c, d_e.
// HS_DIMS4: E % 4, H % 4, V > 0, ldl % 4 (the vectorised kernels).
enum : unsigned { HS_ACT = 1, HS_W = 2, HS_B = 4, HS_OUT_B = 8, HS_TARGET = 16, HS_LOSS = 32, HS_D_LOSS = 64, HS_D_OUT = 128,
                  HS_DT = 256, HS_G = 512, HS_DIMS4 = 1024, HS_W_ALL = HS_W | HS_B | HS_OUT_B };
static bool head_w_ok(const vag_head_w& w, unsigned need) {
    return (!(need & HS_W) || (w.w1 && w.w2 && w.w3 && w.out_w)) && (!(need & HS_B) || (w.b1 && w.b2 && w.b3)) && (!(need & HS_OUT_B) || w.out_b);
}
static bool head_g_ok(const vag_head_g& g) { return g.w1 && g.b1 && g.w2 && g.b2 && g.w3 && g.b3 && g.out_w && g.out_b; }
static int head_seq_check(const HeadSeq& a, unsigned need) {
    VAG_CHECK_ARG(vag_label_smoothing_ok(a.eps));
    VAG_CHECK_ARG(a.tmid && a.logits && head_w_ok(a.w, need) && (!(need & HS_ACT) || (a.h2 && a.c && a.e)));
    VAG_CHECK_ARG(!(need & HS_TARGET) || (a.tgt && a.vocab_weight && a.lse && a.inv_cnt));
    VAG_CHECK_ARG(!(need & HS_LOSS) || (a.nll && (a.loss_mt || a.losses)));
    VAG_CHECK_ARG((!(need & HS_D_LOSS) || a.d_loss) && (!(need & HS_D_OUT) || (a.d_h2 && a.d_c && a.d_e)) && (!(need & HS_DT) || a.dt));
    VAG_CHECK_ARG(!(need & HS_G) || head_g_ok(a.g));
    // distillation: the plain loss in fp32 storage, on logits this call forms (the bf16 d(logits) slot has no correction)
    VAG_CHECK_ARG(a.kd.k == 0 || (vag_kd_ok(a.kd.k, a.kd.lambda, a.V) && a.kd.idx && a.kd.q && a.eps == 0.f && a.mrt.n == 0 &&
                                  !a.logits_ready && !vag_ctx().store16));
    // R-Drop: pairs of adjacent rows, on logits this call forms, fp32 d(logits) in place; smoothing may be on
    VAG_CHECK_ARG(a.rd.alpha == 0.f || (vag_rdrop_ok(a.rd.alpha) && a.rd.kl && a.B % 2 == 0 && a.mrt.n == 0 && a.kd.k == 0 &&
                                        !a.logits_ready && !vag_ctx().store16));
    VAG_CHECK_ARG(a.B > 0 && a.Tt > 0 && a.ldl >= a.V && (!(need & HS_DIMS4) || (a.E % 4 == 0 && a.H % 4 == 0 && a.V > 0 && a.ldl % 4 == 0)));
    return VAG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the vocabulary-sized gradient products
// ---------------------------------------------------------------------------------------------------------------------
// d(tmid) = d(logits) out.weight and g(out.weight) += d(logits)^T tmid.  2-byte storage mode: plain bf16 operands, one MFMA
// product instead of three (fp32 accumulation) -- gradients of a softmax over V classes are sums of thousands of small terms whose
// 2^-9 rounding errors average out; the forward logits keep the two-plane product.  VAG_HEAD_BF16_GRADS=0 keeps two planes here too.
static bool head_grads_one_plane() { return vag_opt().head_bf16_grads != 0 && vag_ctx().store16; }
// dl16 (optional): the same d(logits) chunk as its producer stored it in bf16 (vag_ce_bwd_colsum_launch's out16), row stride ldl
static int head_dt_gemm(int64_t R, int64_t E, int64_t V, const float* dlogits, int64_t ldl, const float* out_w, float* dt,
                        hipStream_t s, const void* dl16 = nullptr) {
    if (dl16) return vag_gemm_launch_planes(1, R, E, V, 1.f, reinterpret_cast<const float*>(dl16), ldl, 1, out_w, E, 1, 0.f, dt, E, s, 1);
    if (head_grads_one_plane() && R > 128) return vag_gemm_launch_planes(1, R, E, V, 1.f, dlogits, ldl, 1, out_w, E, 1, 0.f, dt, E, s);
    return gemm_nn(R, E, V, dlogits, ldl, out_w, E, 0.f, dt, E, s);
}
static int head_outw_gemm(int64_t V, int64_t E, int64_t R, const float* dlogits, int64_t ldl, const float* tmid, float* g_out_w,
                          hipStream_t s, const void* dl16 = nullptr) {
    if (R == 0) return VAG_OK;
    if (dl16) return vag_gemm_launch_planes(1, V, E, R, 1.f, reinterpret_cast<const float*>(dl16), 1, ldl, tmid, E, 1, 1.f, g_out_w, E, s, 1);
    if (head_grads_one_plane() && R > 128) return vag_gemm_launch_planes(1, V, E, R, 1.f, dlogits, 1, ldl, tmid, E, 1, 1.f, g_out_w, E, s);
    return gemm_tn_acc(V, E, R, dlogits, ldl, tmid, E, g_out_w, E, s);
}
// 2-byte storage mode, chunked head: the bf16 copy of a chunk's d(logits) lives behind the chunk inside the (whole-sequence
// sized) logits buffer; NULL when the mode is off, the chunk is small, or there is no room behind it.
static void* head_dl16_slot(float* logits, int64_t ldl, int64_t R, int64_t CH, int64_t E) {
    if (!head_grads_one_plane() || CH <= 128 || vag_opt().head_bf16_dlogits == 0) return nullptr;
    // a bf16 A operand exists only for the 128 x 128 one-plane kernel (gemm.hip): narrow embeddings (the cost model then picks
    // 64-wide tiles), the f32-MFMA switch and a forced tile keep the fp32 in-place d(logits)
    if (E <= 64 || vag_opt().gemm_f32mfma != 0 || vag_opt().gemm_force_tile != 0) return nullptr;
    if (CH * 3 > R * 2) return nullptr;                      // CH * ldl floats of chunk + CH * ldl / 2 floats of bf16 must fit R * ldl
    return logits + CH * ldl;
}

// ---------------------------------------------------------------------------------------------------------------------
// the parts of a sequence-level call
// ---------------------------------------------------------------------------------------------------------------------
// What a pass over rows produces; the backward's halves are told with the same words what they find done.
// HEAD_LOGITS: the vocabulary product.  HEAD_LSE: log-sum-exp and nll of the rows.  HEAD_DLOGITS: d(logits) in place (or in the bf16
// slot) with g(out.bias), its column sums.  HEAD_DT: d(tmid) = d(logits) out.weight.  HEAD_OUT_W: g(out.weight) += d(logits)^T tmid.
enum : unsigned { HEAD_LOGITS = 1, HEAD_LSE = 2, HEAD_DLOGITS = 4, HEAD_DT = 8, HEAD_OUT_W = 16 };

// tmid (R,E) = dropout(tanh(W1 h2 + b1 + W2 c + b2 + W3 e + b3)) for all R = Tt*B rows (NMT_Decoder.py:137-141): the three
// products accumulate into a zeroed tmid from ONE grouped launch (each alone is 40 tiles), then one elementwise pass.
static int head_pre_seq(const HeadSeq& a) {
    const int64_t R = a.Tt * a.B, E = a.E, H = a.H, C = 2 * H;
    if (!vag_ctx().step_zeroed) VAG_TRY(zero_async(a.tmid, R * E * sizeof(float), a.s));
    VagGemmGroup grp4;
    VAG_TRY(vag_gemm_launch(R, E, H, 1.f, a.h2, H, 1, a.w.w1, 1, H, 1.f, a.tmid, E, a.w.b1, 0, a.s));
    VAG_TRY(vag_gemm_launch(R, E, C, 1.f, a.c, C, 1, a.w.w2, 1, C, 1.f, a.tmid, E, a.w.b2, 0, a.s));
    VAG_TRY(vag_gemm_launch(R, E, E, 1.f, a.e, E, 1, a.w.w3, 1, E, 1.f, a.tmid, E, a.w.b3, 0, a.s));
    VAG_TRY(grp4.end(a.s));
    return vag_tanh_dropout_launch(a.tmid, R * E, 0, a.rng, VAG_DROP_DEC_OUT, a.p_out, a.s);
}

// Rows per chunk of a chunked head, a whole number of time steps (row r0 = step r0 / B); 0: the whole sequence at once.  With a
// chunk the (Tt*B, V) logits are never formed as a whole: the forward computes them chunk by chunk for the log-sum-exp / NLL, the
// backward RECOMPUTES each chunk, turns it into d(logits) in place and consumes it with the two products that need it -- the chunk
// is the only logits storage that is touched (set for large Tt*B*V: configs[4]).
static int64_t head_chunk_rows(const HeadSeq& a) {
    const int64_t R = a.Tt * a.B;
    return (!a.logits_ready && a.chunk > 0 && a.chunk < R) ? (a.chunk + a.B - 1) / a.B * a.B : 0;
}
// `parts` of rows [r0, r0 + rows), the logits in the chunk buffer a.logits (CH = 0: rows are the whole sequence, in place)
static int head_rows_pass(const HeadSeq& a, int64_t r0, int64_t rows, int64_t CH, unsigned parts) {
    const int64_t B = a.B, E = a.E, V = a.V, ldl = a.ldl;
    const int64_t* tgt = a.tgt + r0 / B;
    hipStream_t s = a.s;
    if (parts & HEAD_LOGITS)
        VAG_TRY(vag_gemm_launch(rows, V, E, 1.f, a.tmid + r0 * E, E, 1, a.w.out_w, 1, E, 0.f, a.logits, ldl, a.w.out_b, 0, s));
    if (parts & HEAD_LSE)
        VAG_TRY(vag_lse_nll_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.lse + r0, a.nll + r0, /*argmax*/ nullptr, 0,
                                   /*logp_out*/ nullptr, 0, s, a.eps));
    const int64_t K = a.kd.k;           // distillation (distill.hip): the soft part of the rows' nll, and of their d(logits) below
    if ((parts & HEAD_LSE) && K > 0)
        VAG_TRY(vag_kd_nll_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.lse + r0, a.kd.idx + r0 * K, a.kd.q + r0 * K, K,
                                  a.kd.lambda, a.nll + r0, s));
    const bool rd = a.rd.alpha > 0.f;   // R-Drop (rdrop.hip): the pairs' kl and its share of nll; its own d(logits) pass below
    if ((parts & HEAD_LSE) && rd)
        VAG_TRY(vag_rdrop_pair_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.lse + r0, a.rd.alpha, a.rd.kl + r0,
                                      a.nll + r0, s));
    void* dl16 = nullptr;
    if ((parts & HEAD_DLOGITS) && rd) {
        VAG_TRY(vag_rdrop_bwd_colsum_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.lse + r0, a.rd.kl + r0, a.inv_cnt,
                                            a.d_loss, a.rd.alpha, a.g.out_b, s, a.eps));
    } else if (parts & HEAD_DLOGITS) {
        if (rows > 128) dl16 = head_dl16_slot(a.logits, ldl, a.Tt * B, CH, E);
        VAG_TRY(vag_ce_bwd_colsum_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.lse + r0, a.inv_cnt, a.d_loss,
                                         a.g.out_b, s, dl16, a.eps));
        if (K > 0)                      // before the two products below (and the weight group) read d(logits)
            VAG_TRY(vag_kd_dlogits_launch(a.logits, ldl, rows, V, tgt, B, a.Tt, a.vocab_weight, a.inv_cnt, a.d_loss, a.kd.idx + r0 * K,
                                          a.kd.q + r0 * K, K, a.kd.lambda, a.g.out_b, s));
    }
    if (parts & HEAD_DT) VAG_TRY(head_dt_gemm(rows, E, V, a.logits, ldl, a.w.out_w, a.dt + r0 * E, s, dl16));
    if (parts & HEAD_OUT_W) VAG_TRY(head_outw_gemm(V, E, rows, a.logits, ldl, a.tmid + r0 * E, a.g.out_w, s, dl16));
    return VAG_OK;
}
static int head_chunks(const HeadSeq& a, int64_t CH, unsigned parts) {
    const int64_t R = a.Tt * a.B, step = CH > 0 ? CH : R;
    for (int64_t r0 = 0; r0 < R; r0 += step) VAG_TRY(head_rows_pass(a, r0, R - r0 < step ? R - r0 : step, CH, parts));
    return VAG_OK;
}

// d(logits) (a.logits) -> d(tmid) -> through dropout+tanh -> input gradients.  a.dt (R,E) is left holding d(pre-activation).
static int head_bwd_data(const HeadSeq& a, unsigned done) {
    const int64_t R = a.Tt * a.B, E = a.E, H = a.H, C = 2 * H;
    if (!(done & HEAD_DT)) VAG_TRY(head_dt_gemm(R, E, a.V, a.logits, a.ldl, a.w.out_w, a.dt, a.s));
    VAG_TRY(vag_tanh_bwd_launch(a.tmid, a.dt, a.dt, R * E, a.rng, VAG_DROP_DEC_OUT, a.p_out, a.s));   // tmid holds tanh(.)*mul
    VagGemmGroup grp5;              // three independent products of d(pre-activation): one grouped launch
    VAG_TRY(gemm_nn(R, H, E, a.dt, E, a.w.w1, H, 0.f, a.d_h2, H, a.s));
    VAG_TRY(gemm_nn(R, C, E, a.dt, E, a.w.w2, C, 0.f, a.d_c, C, a.s));
    VAG_TRY(gemm_nn(R, E, E, a.dt, E, a.w.w3, E, 0.f, a.d_e, E, a.s));
    return grp5.end(a.s);
}
// Parameter gradients of the head from d(logits) and a.dt = d(pre-activation): nothing downstream waits for these,
// so they may run on a side stream beside the decoder's backward recurrence.
static int head_bwd_weights(const HeadSeq& a, unsigned done) {
    const int64_t R = a.Tt * a.B, E = a.E, H = a.H, C = 2 * H;
    VagGemmGroup grp6;
    if (!(done & HEAD_OUT_W)) VAG_TRY(head_outw_gemm(a.V, E, R, a.logits, a.ldl, a.tmid, a.g.out_w, a.s));
    if (!(done & HEAD_DLOGITS)) VAG_TRY(vag_colsum_launch(a.logits, R, a.V, a.ldl, a.g.out_b, a.s));
    // b1, b2, b3 enter the same sum (NMT_Decoder.py:137): each of the three products leaves sum_r dt[r,:] in one of them
    VAG_TRY(gemm_tn_acc(E, H, R, a.dt, E, a.h2, H, a.g.w1, H, a.s, a.g.b1));
    VAG_TRY(gemm_tn_acc(E, C, R, a.dt, E, a.c, C, a.g.w2, C, a.s, a.g.b2));
    VAG_TRY(gemm_tn_acc(E, E, R, a.dt, E, a.e, E, a.g.w3, E, a.s, a.g.b3));
    return grp6.end(a.s);
}

// Forward: tmid, logits (whole or by chunks), lse / nll, then the loss.  inv_cnt_ready: the caller has filled inv_cnt already (step
// prologue).  finish_in_fwd (a step whose backward follows in the same call): each chunk is finished completely while it is
// still on the die -- a row's log-sum-exp needs only that row, and d(loss)/d(loss_mt) and 1/count are known before the step starts --
// so nothing is recomputed and the backward starts at d(tmid); fwd_finished tells it so.
int vag_head_seq_fwd(HeadSeq& a) {
    VAG_TRY(head_seq_check(a, HS_ACT | HS_W_ALL | HS_TARGET | HS_LOSS | HS_DIMS4));
    if (!a.inv_cnt_ready) VAG_TRY(vag_inv_cnt_launch(a.tgt, a.B, a.Tt, a.inv_cnt, a.s));
    const int64_t CH = head_chunk_rows(a);
    if (!a.logits_ready) VAG_TRY(head_pre_seq(a));
    unsigned parts = HEAD_LSE | (a.logits_ready ? 0 : HEAD_LOGITS);
    if (CH > 0 && a.finish_in_fwd) parts |= HEAD_DLOGITS | HEAD_DT | HEAD_OUT_W;
    VAG_TRY(head_chunks(a, CH, parts));
    a.fwd_finished = (parts & HEAD_DLOGITS) != 0;
    if (a.losses && a.mrt.n > 0)        // a minimum-risk step: the coefficients and the risk in place of the loss reduction (mrt.hip)
        return vag_mrt_weights_launch(a.nll, a.mrt.cost, a.mrt.valid, a.B, a.Tt, a.mrt.n, a.mrt.alpha, a.mrt.scale, a.inv_cnt, nullptr,
                                      nullptr, a.losses, a.w_mt, a.ring, a.s);
    // losses != NULL: losses[1] = loss_mt and the weighted total losses[0] are written instead of loss_mt (V11.py:164-166)
    const LossTask t = {a.nll, a.inv_cnt, a.losses, (int)a.B, (int)a.Tt, a.has_vse, a.ring, a.w_mt, a.w_vse};
    return vag_loss_mt_launch(t, a.losses ? nullptr : a.loss_mt, a.s);
}

// Backward with the label smoothing a.eps of the forward it follows.  A chunked head whose forward already finished the chunks
// applied it there; every other form applies it to d(logits) here.
int vag_head_seq_bwd(const HeadSeq& a) {
    const int64_t CH = head_chunk_rows(a);
    VAG_TRY(head_seq_check(a, HS_ACT | HS_W | (CH > 0 ? HS_OUT_B : 0) | HS_TARGET | HS_D_LOSS | HS_D_OUT | HS_DT | HS_G | HS_DIMS4));
    // chunked: per chunk, logits again -> d(logits) (+ bias gradient) -> its share of d(tmid) and of the out.weight gradient; then
    // everything that no longer needs the logits.  Whole sequence: d(logits) and the output-bias gradient in one pass over the
    // logits; d(tmid) is head_bwd_data's, g(out.weight) joins the weight-gradient group.
    const unsigned parts = CH > 0 ? HEAD_LOGITS | HEAD_DLOGITS | HEAD_DT | HEAD_OUT_W : HEAD_DLOGITS;
    if (!(CH > 0 && a.fwd_finished)) VAG_TRY(head_chunks(a, CH, parts));
    VAG_TRY(head_bwd_data(a, parts));
    return head_bwd_weights(a, parts);
}
// ... the input gradients alone (the parameter gradients: vag_head_bwd_weights, possibly on another stream)
static int head_seq_bwd_data(const HeadSeq& a) {
    VAG_CHECK_ARG(a.rd.alpha == 0.f);   // (no entry point asks for it: an R-Drop backward is vag_head_seq_bwd's)
    VAG_TRY(head_seq_check(a, HS_W | HS_TARGET | HS_D_LOSS | HS_D_OUT | HS_DT | HS_DIMS4));
    VAG_TRY(vag_ce_bwd_launch(a.logits, a.ldl, a.Tt * a.B, a.V, a.tgt, a.B, a.Tt, a.vocab_weight, a.lse, a.inv_cnt, a.d_loss, a.s,
                              a.eps));
    if (a.kd.k > 0)                     // (g(out.bias) is vag_head_bwd_weights' column sum of the corrected d(logits))
        VAG_TRY(vag_kd_dlogits_launch(a.logits, a.ldl, a.Tt * a.B, a.V, a.tgt, a.B, a.Tt, a.vocab_weight, a.inv_cnt, a.d_loss, a.kd.idx,
                                      a.kd.q, a.kd.k, a.kd.lambda, nullptr, a.s));
    return head_bwd_data(a, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static HeadSeq head_seq(const float* h2, const float* c, const float* e, const vag_head_w& w, int64_t B, int64_t Tt, int64_t E, int64_t H,
                        int64_t V, int64_t ldl, float p_out, const uint64_t* rng, const float* tmid, float* logits, vag_stream_t stream) {
    HeadSeq a;
    a.h2 = h2; a.c = c; a.e = e; a.w = w;
    a.B = B; a.Tt = Tt; a.E = E; a.H = H; a.V = V; a.ldl = ldl;
    a.p_out = p_out; a.rng = rng; a.s = S_(stream);
    a.tmid = const_cast<float*>(tmid); a.logits = logits;
    return a;
}
// what the loss reads (d_loss: a backward's), and what a backward writes (g: all-NULL where the parameter gradients are not asked for)
static void head_seq_loss_in(HeadSeq& a, const int64_t* tgt, const float* vocab_weight, const float* lse, const float* inv_cnt, float eps,
                             const float* d_loss) {
    a.tgt = tgt; a.vocab_weight = vocab_weight; a.eps = eps; a.d_loss = d_loss;
    a.lse = const_cast<float*>(lse); a.inv_cnt = const_cast<float*>(inv_cnt);
}
static void head_seq_bwd_out(HeadSeq& a, float* d_h2, float* d_c, float* d_e, const vag_head_g& g, float* dt) {
    a.d_h2 = d_h2; a.d_c = d_c; a.d_e = d_e; a.g = g; a.dt = dt;
}

extern "C" {

// The label-smoothed loss (vag_nmt.h): eps reaches every loss launch of the call -- the plain form, the chunked form and
// logits_ready.  eps == 0 is vag_head_ce_seq_fwd.
int vag_head_ce_seq_fwd_ls(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                           const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                           const uint64_t* rng, int logits_ready, float* tmid, float* logits, int64_t ldl, float* lse,
                           float* nll, float* inv_cnt, float* loss_mt, float label_smoothing, vag_stream_t stream) {
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, label_smoothing, nullptr);
    a.logits_ready = logits_ready; a.nll = nll; a.loss_mt = loss_mt;
    return vag_head_seq_fwd(a);
}
int vag_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                        const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                        const uint64_t* rng, int logits_ready, float* tmid, float* logits, int64_t ldl, float* lse,
                        float* nll, float* inv_cnt, float* loss_mt, vag_stream_t stream) {
    return vag_head_ce_seq_fwd_ls(h2_all, c_all, e_all, w, tgt, vocab_weight, B, Tt, E, H, V, p_out, rng, logits_ready, tmid, logits,
                                  ldl, lse, nll, inv_cnt, loss_mt, 0.f, stream);
}

int vag_head_ce_seq_bwd_data_ls(vag_head_w w, const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E,
                                int64_t H, int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits,
                                int64_t ldl, const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                                float* d_c_all, float* d_e_all, float* scratch, float label_smoothing, vag_stream_t stream) {
    HeadSeq a = head_seq(nullptr, nullptr, nullptr, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, label_smoothing, d_loss);
    head_seq_bwd_out(a, d_h2_all, d_c_all, d_e_all, vag_head_g{}, scratch);
    return head_seq_bwd_data(a);
}
int vag_head_ce_seq_bwd_data(vag_head_w w, const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E,
                             int64_t H, int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits,
                             int64_t ldl, const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                             float* d_c_all, float* d_e_all, float* scratch, vag_stream_t stream) {
    return vag_head_ce_seq_bwd_data_ls(w, tgt, vocab_weight, B, Tt, E, H, V, p_out, rng, tmid, logits, ldl, lse, inv_cnt, d_loss,
                                       d_h2_all, d_c_all, d_e_all, scratch, 0.f, stream);
}

// rows R = Tt * B of any split: the products only see R
int vag_head_bwd_weights(const float* h2_all, const float* c_all, const float* e_all, int64_t R, int64_t E, int64_t H,
                         int64_t V, const float* tmid, const float* dlogits, int64_t ldl, const float* dt, vag_head_g g,
                         vag_stream_t stream) {
    HeadSeq a = head_seq(h2_all, c_all, e_all, vag_head_w{}, R, 1, E, H, V, ldl, 0.f, nullptr, tmid, const_cast<float*>(dlogits), stream);
    a.g = g; a.dt = const_cast<float*>(dt);
    VAG_TRY(head_seq_check(a, HS_ACT | HS_DT | HS_G));
    return head_bwd_weights(a, 0);
}

int vag_head_ce_seq_bwd_ls(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                           const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                           const uint64_t* rng, const float* tmid, float* logits, int64_t ldl, const float* lse,
                           const float* inv_cnt, const float* d_loss, float* d_h2_all, float* d_c_all, float* d_e_all,
                           vag_head_g g, float* scratch, float label_smoothing, vag_stream_t stream) {
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, label_smoothing, d_loss);
    head_seq_bwd_out(a, d_h2_all, d_c_all, d_e_all, g, scratch);
    return vag_head_seq_bwd(a);
}
int vag_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                        const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                        const uint64_t* rng, const float* tmid, float* logits, int64_t ldl, const float* lse,
                        const float* inv_cnt, const float* d_loss, float* d_h2_all, float* d_c_all, float* d_e_all,
                        vag_head_g g, float* scratch, vag_stream_t stream) {
    return vag_head_ce_seq_bwd_ls(h2_all, c_all, e_all, w, tgt, vocab_weight, B, Tt, E, H, V, p_out, rng, tmid, logits, ldl, lse,
                                  inv_cnt, d_loss, d_h2_all, d_c_all, d_e_all, g, scratch, 0.f, stream);
}

// Word-level distillation (vag_nmt.h): the _ls signatures with the teacher's targets in place of the smoothing.  K outside
// [1, 64] is refused here: "no distillation" is vag_head_ce_seq_fwd / _bwd, not these calls with a zero.  (Named vag_kd_*: the
// vag_head_* names are the set whose rejections tests/golden/head_rejections.json records.)
int vag_kd_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                           const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                           const uint64_t* rng, int logits_ready, float* tmid, float* logits, int64_t ldl, float* lse,
                           float* nll, float* inv_cnt, float* loss_mt, int64_t K, float lambda, const int32_t* idx, const float* q,
                           vag_stream_t stream) {
    VAG_CHECK_ARG(K >= 1 && K <= 64);
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, 0.f, nullptr);
    a.logits_ready = logits_ready; a.nll = nll; a.loss_mt = loss_mt;
    a.kd = {(int)K, lambda, idx, q};
    return vag_head_seq_fwd(a);
}
int vag_kd_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                           const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                           const uint64_t* rng, const float* tmid, float* logits, int64_t ldl, const float* lse,
                           const float* inv_cnt, const float* d_loss, float* d_h2_all, float* d_c_all, float* d_e_all,
                           vag_head_g g, float* scratch, int64_t K, float lambda, const int32_t* idx, const float* q,
                           vag_stream_t stream) {
    VAG_CHECK_ARG(K >= 1 && K <= 64);
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, 0.f, d_loss);
    head_seq_bwd_out(a, d_h2_all, d_c_all, d_e_all, g, scratch);
    a.kd = {(int)K, lambda, idx, q};
    return vag_head_seq_bwd(a);
}

// R-Drop (vag_nmt.h): the _ls signatures plus the weight alpha of the symmetric KL term and the rows' kl.  alpha <= 0 or not finite
// is refused here: "no R-Drop" is vag_head_ce_seq_fwd_ls / _bwd_ls, not these calls with a zero.  (Named vag_rdrop_*, as vag_kd_* are.)
int vag_rdrop_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                              const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                              const uint64_t* rng, int logits_ready, float* tmid, float* logits, int64_t ldl, float* lse,
                              float* nll, float* inv_cnt, float* loss_mt, float label_smoothing, float alpha, float* kl,
                              vag_stream_t stream) {
    VAG_CHECK_ARG(vag_rdrop_ok(alpha));
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, label_smoothing, nullptr);
    a.logits_ready = logits_ready; a.nll = nll; a.loss_mt = loss_mt;
    a.rd = {alpha, kl};
    return vag_head_seq_fwd(a);
}
int vag_rdrop_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w, const int64_t* tgt,
                              const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H, int64_t V, float p_out,
                              const uint64_t* rng, const float* tmid, float* logits, int64_t ldl, const float* lse,
                              const float* inv_cnt, const float* d_loss, float* d_h2_all, float* d_c_all, float* d_e_all,
                              vag_head_g g, float* scratch, float label_smoothing, float alpha, const float* kl,
                              vag_stream_t stream) {
    VAG_CHECK_ARG(vag_rdrop_ok(alpha));
    HeadSeq a = head_seq(h2_all, c_all, e_all, w, B, Tt, E, H, V, ldl, p_out, rng, tmid, logits, stream);
    head_seq_loss_in(a, tgt, vocab_weight, lse, inv_cnt, label_smoothing, d_loss);
    head_seq_bwd_out(a, d_h2_all, d_c_all, d_e_all, g, scratch);
    a.rd = {alpha, const_cast<float*>(kl)};
    return vag_head_seq_bwd(a);
}

int vag_head_logp_seq_fwd(const float* h2, const float* c, const float* e, vag_head_w w, int64_t R, int64_t E, int64_t H,
                          int64_t V, float p_out, const uint64_t* rng, float* tmid, float* logp, int64_t ldl,
                          vag_stream_t stream) {
    HeadSeq a = head_seq(h2, c, e, w, R, 1, E, H, V, ldl, p_out, rng, tmid, logp, stream);
    VAG_TRY(head_seq_check(a, HS_ACT | HS_W_ALL | HS_DIMS4));
    VAG_TRY(head_pre_seq(a));
    VAG_TRY(linear_fwd(R, V, E, tmid, E, w.out_w, w.out_b, 0, logp, ldl, a.s));
    return head_logp_rows(logp, ldl, R, V, nullptr, a.s);
}

int vag_head_logp_seq_bwd(const float* h2, const float* c, const float* e, vag_head_w w, int64_t R, int64_t E, int64_t H,
                          int64_t V, float p_out, const uint64_t* rng, const float* tmid, const float* logp, float* d_logp,
                          int64_t ldl, float* d_h2, float* d_c, float* d_e, vag_head_g g, float* scratch,
                          vag_stream_t stream) {
    HeadSeq a = head_seq(h2, c, e, w, R, 1, E, H, V, ldl, p_out, rng, tmid, d_logp, stream);      // (d_logp becomes d(logits) in place)
    head_seq_bwd_out(a, d_h2, d_c, d_e, g, scratch);
    VAG_CHECK_ARG(logp != nullptr);
    VAG_TRY(head_seq_check(a, HS_ACT | HS_W | HS_D_OUT | HS_DT | HS_G));
    VAG_TRY(vag_logsoftmax_bwd_launch(logp, ldl, d_logp, ldl, R, V, a.s));
    VAG_TRY(head_bwd_data(a, 0));
    return head_bwd_weights(a, 0);
}

int vag_head_logp_step(const float* h2, const float* c, const float* e, vag_head_w w, int64_t N, int64_t E, int64_t H,
                       int64_t V, float* logp, int64_t ldl, int64_t* argmax, float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(h2 && c && e && logp && scratch && N > 0 && E % 4 == 0 && H % 4 == 0 && V > 0 && ldl >= V && head_w_ok(w, HS_W_ALL));
    VAG_TRY(vag_head_step(h2, c, e, w, N, E, H, V, 0.f, nullptr, 0, /*tmp (N,E)*/ scratch, /*tmid (N,E)*/ scratch + N * E, logp, ldl, s));
    return head_logp_rows(logp, ldl, N, V, argmax, s);
}

// ... with the context share of a hoisted decoding step (vag_cgru_attn_decode_step_h) in place of the context.  What its two
// entry points share: the checks (out: logp or logits) and tmid (N,E), formed in the scratch's second half
static int head_tmid_step_h(const float* h2, const float* cw, const float* e, const float* tables, const int64_t* tok, const vag_head_w& w,
                            int64_t N, int64_t E, int64_t H, int64_t V, const float* out, int64_t ldl, float* scratch, hipStream_t s) {
    VAG_CHECK_ARG(h2 && cw && (tables ? tok != nullptr : e != nullptr) && out && scratch && N > 0 && N <= 256 && E % 4 == 0 &&
                  H % 4 == 0 && V > 0 && ldl >= V);
    VAG_CHECK_ARG(w.w1 && w.b1 && w.b2 && w.w3 && w.b3 && w.out_w && w.out_b && aligned16(h2) && (tables || aligned16(e)) &&
                  aligned16(w.w1) && aligned16(w.w3));
    const float* embw3 = tables ? step_tables(const_cast<float*>(tables), V, E, H).embw3 : nullptr;      // (a reader's view)
    return head_pre_step_h(h2, cw, e, embw3, tok, w, N, E, H, scratch + N * E, s);
}
int vag_head_logp_step_h(const float* h2, const float* cw, const float* e, const float* tables, const int64_t* tok, vag_head_w w,
                         int64_t N, int64_t E, int64_t H, int64_t V, float* logp, int64_t ldl, int64_t* argmax, float* scratch,
                         vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_TRY(head_tmid_step_h(h2, cw, e, tables, tok, w, N, E, H, V, logp, ldl, scratch, s));
    VAG_TRY(linear_fwd(N, V, E, scratch + N * E, E, w.out_w, w.out_b, 0, logp, ldl, s));
    return head_logp_rows(logp, ldl, N, V, argmax, s);
}
int vag_head_logits_step_h(const float* h2, const float* cw, const float* e, const float* tables, const int64_t* tok, vag_head_w w,
                           int64_t N, int64_t E, int64_t H, int64_t V, float* logits, int64_t ldl, float* parts, float* scratch,
                           vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(parts && aligned16(scratch));
    VAG_TRY(head_tmid_step_h(h2, cw, e, tables, tok, w, N, E, H, V, logits, ldl, scratch, s));
    return vag_logits_parts_launch(N, V, E, scratch + N * E, E, w.out_w, E, w.out_b, logits, ldl, parts, s);
}
// The same step for beam search without the normalising pass: raw logits plus, per row, the pieces of its log-sum-exp written by
// the vocabulary product's epilogue (skinny.hip, TallArgs::parts); vag_beam_step_logits_dev normalises on the fly.  The count is 0
// for shapes the tall-skinny kernel does not take (N = B k <= 96 rows, V < 4096, E % 256 != 0): use vag_head_logp_step there.
int64_t vag_head_logits_parts_count(vag_head_w w, int64_t N, int64_t E, int64_t V) {
    if (!w.out_w || N <= 0 || E <= 0 || V <= 0) return 0;
    alignas(16) static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};
    return vag_logits_parts_count(N, V, E, dummy, E, w.out_w, E);
}
int vag_head_logits_step(const float* h2, const float* c, const float* e, vag_head_w w, int64_t N, int64_t E, int64_t H,
                         int64_t V, float* logits, int64_t ldl, float* parts, float* scratch, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(h2 && c && e && logits && parts && scratch && N > 0 && E % 4 == 0 && H % 4 == 0 && V > 0 && ldl >= V);
    VAG_CHECK_ARG(head_w_ok(w, HS_W_ALL) && aligned16(scratch));
    VAG_CHECK_ARG(N <= 256 && aligned16(h2) && aligned16(c) && aligned16(e) && aligned16(w.w1) && aligned16(w.w2) && aligned16(w.w3));
    VAG_TRY(head_pre_step(h2, c, e, w, N, E, H, 0.f, nullptr, 0, /*tmid (N,E)*/ scratch + N * E, s));
    return vag_logits_parts_launch(N, V, E, scratch + N * E, E, w.out_w, E, w.out_b, logits, ldl, parts, s);
}

}  // extern "C"
