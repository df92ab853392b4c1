// C ABI of libvagnmt.so (include/vag_nmt.h): host-side orchestration of the kernel launches for every operator of the VAG-NMT hot
// path but the sequence operators (enc_api.hip, dec_api.hip) and the output head (head_api.hip): version, options and call context,
// dense products and embedding, grounding and initial state, the decode-time wrappers, optimiser, RNG, recurrence queries.  A
// definition takes its C linkage from the header's declaration.  No allocation, no host synchronisation: every function only enqueues
// work on the caller's stream, so whole training steps can be captured into a HIP graph.
#include "../../include/vag_nmt.h"
#include "api_shared.h"
#include <cstring>

// What a call tells its operators: one VagCallCtx per host thread (the base context) and one per vag_train_step call, reached
// through vag_ctx() -- call_ctx.h has the fields, DESIGN.md section 5a the list.
static thread_local VagCallCtx g_base_ctx;
static thread_local VagCallCtx* g_active_ctx = nullptr;
VagCallCtx& vag_ctx() { return g_active_ctx ? *g_active_ctx : g_base_ctx; }
VagCallScope::VagCallScope(VagCallCtx& c) : ctx(c), prev(g_active_ctx) { g_active_ctx = &c; }
// What must not outlive the call, in the order that matters; everything else goes with the context itself (a stack object of the
// caller): hints, requests nobody consumed, a held-back rmw record.
VagCallScope::~VagCallScope() {
    (void)vag_loss_defer_flush();       // (an error return between the head's forward and backward: the loss is still written)
    if (ctx.leaf_on) vag_leaf_drop();   // (an error return before the leaf queue's flush: its task list is gemm.hip's)
    g_active_ctx = prev;
}

VagOptions& vag_opt() {
    static VagOptions o;
    return o;
}

int vag_version(void) { return 330; }      // 330: search options, n-best finish, forced-decoding scores (vag_beam_*_opt,
                                           // vag_beam_finish_nbest, vag_forced_score); 320: ensemble decoding

// Debug / tuning options by name (common.h: VagOptions); process-wide, takes effect for calls enqueued afterwards.
int vag_set_option(const char* name, int64_t value) {
    VAG_CHECK_ARG(name != nullptr);
    VagOptions& o = vag_opt();
    const struct { const char* n; int* p; } ints[] = {
        {"gemm_f32mfma", &o.gemm_f32mfma}, {"gemm_slabs", &o.gemm_slabs}, {"gemm_nogroup", &o.gemm_nogroup}, {"gemm_big", &o.gemm_big}, {"gemm_force_tile", &o.gemm_force_tile},
        {"gemm_force_splitk", &o.gemm_force_splitk}, {"head_fuse", &o.head_fuse},
        {"head_bf16_grads", &o.head_bf16_grads}, {"persistent", &o.persistent}, {"persistent_dec_bwd", &o.persistent_dec_bwd}, {"persistent_enc_bwd", &o.persistent_enc_bwd}, {"free_persistent", &o.free_persistent}, {"attn_dot_reg", &o.attn_dot_reg},
        {"persist_timing", &o.persist_timing}, {"s16_one_plane", &o.s16_one_plane}, {"leaf_queue", &o.leaf_queue}, {"attn_row", &o.attn_row}, {"dec_xcd_map", &o.dec_xcd_map}, {"loss_ride", &o.loss_ride}, {"step_fork", &o.step_fork},
        {"head_bf16_dlogits", &o.head_bf16_dlogits}, {"handoff_planes", &o.handoff_planes}};
    for (const auto& e : ints)
        if (strcmp(name, e.n) == 0) { *e.p = (int)value; return VAG_OK; }
    if (strcmp(name, "head_chunk") == 0) { o.head_chunk = value; return VAG_OK; }
    if (strcmp(name, "persist_spin_limit") == 0) { o.persist_spin_limit = value; return VAG_OK; }
#ifdef VAG_LAB          // lab build only (make LAB=1): phase timestamps of the persistent decoder kernels, per-product choice printing
    if (strcmp(name, "dec_stamps") == 0) { o.dec_stamps = value; return VAG_OK; }
    if (strcmp(name, "dec_bwd_stamps") == 0) { o.dec_bwd_stamps = value; return VAG_OK; }
    if (strcmp(name, "gemm_debug") == 0) { o.gemm_debug = (int)value; return VAG_OK; }
    if (strcmp(name, "gemm_planes") == 0) {      // calling thread's base context: 3, 2, 1, 11
        g_base_ctx.gemm_planes = (value == 2 || value == 1 || value == 11) ? (int)value : 3;
        return VAG_OK;
    }
#endif
    return VAG_EINVAL;
}

// Operator-level access to what vag_train_step sets up for itself: the derived-weights buffer and the storage mode the
// per-operator entry points use ON THE CALLING THREAD until changed (derived NULL / storage 0 = the defaults).
int vag_set_operator_context(const float* derived, int storage) {
    VAG_CHECK_ARG(storage == 0 || (storage == 1 && derived));
    g_base_ctx.derived = derived;
    g_base_ctx.store16 = storage == 1;
    g_base_ctx.gemm_planes = storage == 1 ? 2 : 3;
    return VAG_OK;
}

int vag_gemm_f32(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t sam, int64_t sak, const float* B,
                 int64_t sbk, int64_t sbn, float beta, float* C, int64_t ldc, const float* bias, int act,
                 vag_stream_t stream) {
    return vag_gemm_launch(M, N, K, alpha, A, sam, sak, B, sbk, sbn, beta, C, ldc, bias, act, S_(stream));
}

int vag_linear_fwd(int64_t M, int64_t N, int64_t K, const float* x, const float* W, const float* bias, int act, float* y,
                   vag_stream_t stream) {
    VAG_CHECK_ARG(x && W && y && M >= 0 && N > 0 && K > 0);
    return linear_fwd(M, N, K, x, K, W, bias, act, y, N, S_(stream));
}

int vag_linear_bwd(int64_t M, int64_t N, int64_t K, const float* x, const float* W, const float* y, float* dy, int act,
                   float* d_x, int accumulate_dx, float* g_W, float* g_b, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(x && W && dy && M >= 0 && N > 0 && K > 0 && (!act || y));
    if (M == 0) return VAG_OK;
    if (act) VAG_TRY(vag_tanh_bwd_launch(y, dy, dy, M * N, nullptr, 0, 0.f, s));
    if (d_x) VAG_TRY(gemm_nn(M, K, N, dy, N, W, K, accumulate_dx ? 1.f : 0.f, d_x, K, s));
    if (g_W) VAG_TRY(gemm_tn_acc(N, K, M, dy, N, x, K, g_W, K, s));
    if (g_b) VAG_TRY(vag_colsum_launch(dy, M, N, N, g_b, s));
    return VAG_OK;
}

int vag_embed_fwd(const int64_t* idx, int64_t n, const float* W, int64_t E, float* out, vag_stream_t stream) {
    return vag_embed_gather_launch(idx, 1, 0, n, 1, W, E, out, nullptr, 0, 0.f, S_(stream));
}
int vag_embed_bwd(const int64_t* idx, int64_t n, const float* d_out, int64_t E, float* g_W, vag_stream_t stream) {
    return vag_embed_scatter_launch(idx, 1, 0, n, 1, d_out, E, g_W, nullptr, 0, 0.f, S_(stream));
}

// =====================================================================================================
// shared-space projections
// =====================================================================================================
int vag_img_proj_l2_fwd(const float* x, const float* W, const float* b, int64_t B, int64_t K, int64_t S, int act, float* y,
                        float* nrm, float* out, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(x && W && b && y && nrm && out && B > 0 && K > 0 && S > 0);
    VAG_TRY(linear_fwd(B, S, K, x, K, W, b, act ? VAG_ACT_TANH : 0, y, S, s));
    return vag_l2norm_fwd_launch(y, B, S, nrm, out, s);
}
int vag_img_proj_l2_bwd(const float* x, const float* W, const float* y, const float* nrm, const float* out, float* d_out,
                        int64_t B, int64_t K, int64_t S, int act, float* d_x, float* g_W, float* g_b, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(x && W && y && nrm && out && d_out && B > 0 && K > 0 && S > 0);
    VAG_TRY(vag_l2norm_bwd_launch(y, nrm, out, d_out, B, S, act, d_out, s));
    if (d_x) VAG_TRY(gemm_nn(B, K, S, d_out, S, W, K, 0.f, d_x, K, s));
    if (g_W) VAG_TRY(gemm_tn_acc(S, K, B, d_out, S, x, K, g_W, K, s));
    if (g_b) VAG_TRY(vag_colsum_launch(d_out, B, S, S, g_b, s));
    return VAG_OK;
}

int vag_l2norm_fwd(const float* x, int64_t B, int64_t S, float* nrm, float* out, vag_stream_t stream) {
    return vag_l2norm_fwd_launch(x, B, S, nrm, out, S_(stream));
}
int vag_l2norm_bwd(const float* x, const float* nrm, const float* out, const float* d_out, int64_t B, int64_t S, float* dx,
                   vag_stream_t stream) {
    return vag_l2norm_bwd_launch(x, nrm, out, d_out, B, S, 0, dx, S_(stream));
}

// =====================================================================================================
// image-conditioned attention
// =====================================================================================================
struct ImgWs {
    float *u, *w, *scores, *dalpha, *de, *dw, *du, *pre, *dpre, *dvp;
    int64_t total;
};
static ImgWs imagine_ws(float* p, int64_t B, int64_t Ts, int64_t C, int method) {
    ImgWs w;
    WsCarver c(p);
    w.u = c.take(B * C); w.w = c.take(B * C); w.scores = c.take(B * Ts); w.dalpha = c.take(B * Ts); w.de = c.take(B * Ts);
    w.dw = c.take(B * C); w.du = c.take(B * C); w.dvp = c.take(VAG_POST_CHUNKS(Ts) * B * C);
    w.pre = method == 1 ? c.take(B * Ts * C) : nullptr;
    w.dpre = method == 1 ? c.take(B * Ts * C) : nullptr;
    w.total = c.off;
    return w;
}
int64_t vag_imagine_ws_floats(int64_t B, int64_t Ts, int64_t C, int64_t S, int method) {
    (void)S;
    return imagine_ws(nullptr, B, Ts, C, method).total;
}

int vag_imagine_attn_ctx_fwd(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                             const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts, int64_t C,
                             int64_t S, float* alpha, float* ctx, float* ws, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(im_emb && enc && mask && ctx2ctx && emb2ctx && alpha && ctx && ws && (method == 0 || (method == 1 && mlp_w)));
    VAG_CHECK_ARG(B > 0 && Ts > 0 && C % 4 == 0 && S % 4 == 0 && aligned16(ws));
    ImgWs w = imagine_ws(ws, B, Ts, C, method);
    VAG_TRY(linear_fwd(B, C, S, im_emb, S, emb2ctx, nullptr, 0, w.u, C, s));                     // emb2ctx(image_vec) :58/:76
    if (method == 0) {
        // e[b,t] = (W_cc enc[b,t]) . u[b] = enc[b,t] . (W_cc^T u[b])                                 :57-64
        VAG_TRY(gemm_nn(B, C, C, w.u, C, ctx2ctx, C, 0.f, w.w, C, s));
        if (Ts <= 4096 && vag_opt().attn_row != 0)          // scores, softmax :46 and bmm :137 in one launch
            return vag_attn_dot_row_launch(false, enc, w.w, C, mask, nullptr, B, Ts, C, alpha, ctx, s);
        VAG_TRY(vag_attn_scores_launch(1, enc, w.w, C, nullptr, mask, B, 1, Ts, C, w.scores, s));
    } else {
        VAG_TRY(linear_fwd(B * Ts, C, C, enc, C, ctx2ctx, nullptr, 0, w.pre, C, s));              // ctx2ctx(decoder_hidden) :75
        VAG_TRY(vag_attn_scores_launch(0, w.pre, w.u, C, mlp_w, mask, B, 1, Ts, C, w.scores, s));   // mlp(tanh(ctx_+im_)) :78
    }
    return vag_attn_ctx_launch(1, w.scores, enc, B, 1, Ts, C, alpha, ctx, s);                      // softmax :46, bmm :137
}

int vag_imagine_attn_ctx_bwd(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                             const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts, int64_t C,
                             int64_t S, const float* alpha, const float* d_ctx, float* ws, float* d_enc, int accumulate_enc,
                             float* d_im_emb, float* g_ctx2ctx, float* g_emb2ctx, float* g_mlp_w, vag_stream_t stream) {
    return vag_imagine_attn_ctx_bwd_impl(im_emb, enc, mask, ctx2ctx, emb2ctx, mlp_w, method, B, Ts, C, S, alpha, d_ctx, ws,
                                         d_enc, accumulate_enc, d_im_emb, 0, g_ctx2ctx, g_emb2ctx, g_mlp_w, S_(stream));
}
int vag_imagine_attn_ctx_bwd_impl(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                                  const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts, int64_t C,
                                  int64_t S, const float* alpha, const float* d_ctx, float* ws, float* d_enc,
                                  int accumulate_enc, float* d_im_emb, int accumulate_im, float* g_ctx2ctx,
                                  float* g_emb2ctx, float* g_mlp_w, hipStream_t s) {
    VAG_CHECK_ARG(im_emb && enc && ctx2ctx && emb2ctx && alpha && d_ctx && ws && d_enc && d_im_emb && g_ctx2ctx && g_emb2ctx);
    VAG_CHECK_ARG((method == 0) || (method == 1 && mlp_w && g_mlp_w));
    VAG_CHECK_ARG(B > 0 && Ts > 0 && C % 4 == 0 && S % 4 == 0);
    (void)mask;
    ImgWs w = imagine_ws(ws, B, Ts, C, method);
    const bool row = Ts <= 4096 && vag_opt().attn_row != 0;
    if (row) {      // d alpha = d_ctx . enc, the softmax backward and (dot method) dw[b] = sum_t de enc in one launch
        VAG_TRY(vag_attn_dot_row_launch(true, enc, d_ctx, C, nullptr, alpha, B, Ts, C, w.de, method == 0 ? w.dw : nullptr, s));
    } else {
        VAG_TRY(vag_attn_scores_launch(1, enc, d_ctx, C, nullptr, nullptr, B, 1, Ts, C, w.dalpha, s));   // d alpha = d_ctx . enc
        VAG_TRY(vag_softmax_bwd_launch(alpha, w.dalpha, B, Ts, w.de, s));
    }
    if (method == 0) {
        VAG_TRY(vag_outer2_launch(alpha, d_ctx, w.de, w.w, B, Ts, C, d_enc, accumulate_enc, s));
        if (!row) VAG_TRY(vag_attn_ctx_launch(0, w.de, enc, B, 1, Ts, C, nullptr, w.dw, s));      // dw[b] = sum_t de enc
        VAG_TRY(linear_fwd(B, C, C, w.dw, C, ctx2ctx, nullptr, 0, w.du, C, s));                   // du = dw W_cc^T
        VAG_TRY(gemm_tn_acc(C, C, B, w.u, C, w.dw, C, g_ctx2ctx, C, s));                          // g_cc[i,j] += u[b,i] dw[b,j]
    } else {
        VAG_TRY(vag_outer2_launch(alpha, d_ctx, nullptr, nullptr, B, Ts, C, d_enc, accumulate_enc, s));
        VAG_TRY(vag_attn_post_bwd_launch(w.pre, w.u, C, mlp_w, w.de, alpha, nullptr, B, Ts, 1, C, w.dpre, w.dvp, nullptr, 0, s));
        VAG_TRY(vag_colsum_launch(w.dvp, VAG_POST_CHUNKS(Ts) * B, C, C, g_mlp_w, s));
        VAG_TRY(vag_attn_dq_launch(w.pre, w.u, C, mlp_w, nullptr, nullptr, w.de, B, Ts, C, w.du, C, s));
        VAG_TRY(gemm_nn(B * Ts, C, C, w.dpre, C, ctx2ctx, C, 1.f, d_enc, C, s));
        VAG_TRY(gemm_tn_acc(C, C, B * Ts, w.dpre, C, enc, C, g_ctx2ctx, C, s));
    }
    VAG_TRY(gemm_nn(B, S, C, w.du, C, emb2ctx, S, accumulate_im ? 1.f : 0.f, d_im_emb, S, s));
    VAG_TRY(gemm_tn_acc(C, S, B, w.du, C, im_emb, S, g_emb2ctx, S, s));
    return VAG_OK;
}

// =====================================================================================================
// ranking loss
// =====================================================================================================
int vag_rank_loss_fwd(const float* im, const float* sv, int64_t B, int64_t S, float margin, int kind, float* scores,
                      float* G, float* loss, vag_stream_t stream) {
    return vag_rank_loss_fwd_impl(im, sv, B, S, margin, kind, scores, G, loss, nullptr, S_(stream));
}
int vag_rank_loss_bwd(const float* im, const float* sv, const float* G, const float* d_loss, int64_t B, int64_t S,
                      float* d_im, float* d_s, vag_stream_t stream) {
    VAG_CHECK_ARG(d_loss != nullptr);
    return vag_rank_loss_bwd_impl(im, sv, G, d_loss, B, S, d_im, d_s, S_(stream));
}
int vag_rank_loss_fwd_impl(const float* im, const float* sv, int64_t B, int64_t S, float margin, int kind, float* scores,
                           float* G, float* loss, const float* g_scale, hipStream_t s, float scale) {
    VAG_CHECK_ARG(im && sv && scores && G && loss && B > 0 && S > 0);
    VAG_CHECK_ARG(kind >= 0 && kind <= 3 && (!(kind & 2) || B % 2 == 0));                          // (before the product is launched)
    VAG_TRY(linear_fwd(B, B, S, im, S, sv, nullptr, 0, scores, B, s));                             // im s^T  (:12)
    return vag_rank_loss_launch(scores, B, margin, kind, G, loss, s, g_scale, scale);
}
int vag_rank_loss_bwd_impl(const float* im, const float* sv, const float* G, const float* d_loss, int64_t B, int64_t S,
                           float* d_im, float* d_s, hipStream_t s) {
    VAG_CHECK_ARG(im && sv && G && d_im && d_s && B > 0 && S > 0);
    if (B <= 128 && B % 16 == 0 && S % 4 == 0 && aligned16(G) && aligned16(im) && aligned16(sv)) return vag_rank_bwd_launch(G, im, sv, d_loss, B, S, d_im, d_s, s);               // both products (and the scale) in one launch
    VAG_TRY(gemm_nn(B, S, B, G, B, sv, S, 0.f, d_im, S, s));                                       // d_im = G s
    VAG_TRY(vag_gemm_launch(B, S, B, 1.f, G, 1, B, im, S, 1, 0.f, d_s, S, nullptr, 0, s));        // d_s  = G^T im
    if (!d_loss) return VAG_OK;                                                                    // (G came pre-multiplied)
    VAG_TRY(vag_scale_by_dev_launch(d_im, B * S, d_loss, s));
    return vag_scale_by_dev_launch(d_s, B * S, d_loss, s);
}

// batch assembly from a device-resident corpus (preprocessing.py:308-384)
int vag_gather_rows_i64(const int64_t* in, int64_t ld, const int64_t* idx, int64_t rows, int64_t w, int64_t* out,
                        vag_stream_t stream) {
    return vag_gather_rows_i64_launch(in, ld, idx, rows, w, out, S_(stream));
}

// =====================================================================================================
// retrieval evaluation: utils/im_retrieval_eval.py:4-57
// =====================================================================================================
int vag_retrieval_ranks(const float* queries, const float* keys, int64_t N, int64_t S, float* scores, int32_t* ranks,
                        vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(queries && keys && scores && ranks && N > 0 && S > 0);
    VAG_TRY(vag_gemm_launch(N, N, S, 1.f, queries, S, 1, keys, 1, S, 0.f, scores, N, nullptr, 0, s));   // one (N,S)x(S,N) product
    return vag_retrieval_rank_launch(scores, N, ranks, s);
}

// =====================================================================================================
// decoder initial state
// =====================================================================================================
int vag_dec_init_fwd(const float* enc, const float* mask, const float* ctx, float split, const float* W, const float* b,
                     int64_t B, int64_t Ts, int64_t C, int64_t H, float* xmix, float* h0, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(enc && mask && W && b && xmix && h0 && B > 0 && Ts > 0 && C % 4 == 0 && H > 0);
    // (a step driver's visual-attention launch may already have left xmix: VagCallCtx::row_mix; asked once)
    const bool left = ctx && vag_ctx().row_mix.done == xmix;
    vag_ctx().row_mix.done = nullptr;
    if (!left) VAG_TRY(vag_meanpool_mix_launch(enc, mask, ctx, split, B, Ts, C, xmix, s));
    return linear_fwd(B, H, C, xmix, C, W, b, VAG_ACT_TANH, h0, H, s);
}
int vag_dec_init_bwd(const float* mask, const float* xmix, const float* h0, float split, const float* W, float* d_h0,
                     int64_t B, int64_t Ts, int64_t C, int64_t H, float* d_enc, int accumulate_enc, float* d_ctx, float* g_W,
                     float* g_b, float* scratch, vag_stream_t stream) {
    return vag_dec_init_bwd_impl(mask, xmix, h0, split, W, d_h0, B, Ts, C, H, d_enc, accumulate_enc, d_ctx, 0, g_W, g_b,
                                 scratch, S_(stream));
}
int vag_dec_init_bwd_impl(const float* mask, const float* xmix, const float* h0, float split, const float* W, float* d_h0,
                          int64_t B, int64_t Ts, int64_t C, int64_t H, float* d_enc, int accumulate_enc, float* d_ctx,
                          int accumulate_ctx, float* g_W, float* g_b, float* scratch, hipStream_t s) {
    VAG_CHECK_ARG(mask && xmix && h0 && W && d_h0 && d_enc && g_W && g_b && scratch && B > 0 && Ts > 0 && C % 4 == 0);
    float* dx = scratch;    // (B,C)
    // (a step driver's persistent decoder backward may already have applied the tanh's derivative: VagCallCtx::dh0_tanh; asked once)
    const bool tanh_done = vag_ctx().dh0_tanh.done == d_h0;
    vag_ctx().dh0_tanh.done = nullptr;
    if (!tanh_done) VAG_TRY(vag_tanh_bwd_launch(h0, d_h0, d_h0, B * H, nullptr, 0, 0.f, s));
    VAG_TRY(gemm_tn_acc(H, C, B, d_h0, H, xmix, C, g_W, C, s));
    VAG_TRY(vag_colsum_launch(d_h0, B, H, H, g_b, s));
    const bool ride = d_ctx && B <= 128;                       // d_ctx (+)= split * dx leaves with the product that forms dx
    if (ride) VAG_TRY(vag_skinny_nn_launch(B, C, H, d_h0, H, W, C, 0.f, dx, C, s, d_ctx, C, split, accumulate_ctx ? 1 : 0));
    else VAG_TRY(gemm_nn(B, C, H, d_h0, H, W, C, 0.f, dx, C, s));
    const float s_eff = d_ctx ? split : 0.f;
    VAG_TRY(vag_meanpool_bwd_launch(mask, dx, 1.f - s_eff, B, Ts, C, d_enc, accumulate_enc, s));
    if (d_ctx && !ride) VAG_TRY(vag_axpy_launch(split, dx, d_ctx, B * C, accumulate_ctx ? 1 : 0, s));
    return VAG_OK;
}

// =====================================================================================================
// beam search, optimiser, dropout helpers
// =====================================================================================================
int64_t vag_beam_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len) {
    (void)max_len;
    return vag_beam_scratch_bytes_impl(B, k, V);
}
int vag_beam_step(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int64_t max_len, const float* h_in,
                  float* h_out, int64_t B, int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch,
                  vag_stream_t stream) {
    return vag_beam_step_launch(logp, ldl, nll, beam, di, nullptr, max_len, h_in, h_out, nullptr, B, k, V, H, n_alive, scratch,
                                S_(stream));
}
int vag_beam_step_dev(float* logp, int64_t ldl, float* nll, int64_t* beam, int32_t* di_state, int64_t max_len,
                      const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k, int64_t V, int64_t H,
                      int32_t* n_alive, void* scratch, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_step_launch(logp, ldl, nll, beam, 0, di_state, max_len, h_in, h_out, tok_out, B, k, V, H, n_alive, scratch,
                                S_(stream));
}
int vag_beam_step_logits_dev(float* logits, int64_t ldl, const float* parts, int64_t nparts, float* nll, int64_t* beam,
                             int32_t* di_state, int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B,
                             int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr && parts != nullptr && nparts > 0);
    return vag_beam_step_launch(logits, ldl, nll, beam, 0, di_state, max_len, h_in, h_out, tok_out, B, k, V, H, n_alive, scratch,
                                S_(stream), parts, nparts);
}
int vag_beam_finish(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t* out,
                    float* best_score, vag_stream_t stream) {
    return vag_beam_finish_launch(nll, beam, max_len, steps, B, k, out, best_score, S_(stream));
}
int vag_ens_max_models(void) { return VAG_ENS_MAX; }
int vag_beam_ens_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, vag_stream_t stream) {
    return vag_beam_ens_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, S_(stream));
}
int vag_beam_ens_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_ens_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, S_(stream));
}
int vag_ens_argmax(const float* const* logp, const int64_t* ldl, int64_t M, int64_t N, int64_t V, int64_t* out,
                   vag_stream_t stream) {
    return vag_ens_argmax_launch(logp, ldl, M, N, V, out, S_(stream));
}
// the expansions above with the search options (flags: VAG_BEAM_ALLOW_REPEAT | VAG_BEAM_AVOID_UNK; 0 = the forms above)
int vag_beam_step_opt(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int64_t max_len, const float* h_in,
                      float* h_out, int64_t B, int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch, int32_t flags,
                      vag_stream_t stream) {
    return vag_beam_step_launch(logp, ldl, nll, beam, di, nullptr, max_len, h_in, h_out, nullptr, B, k, V, H, n_alive, scratch,
                                S_(stream), nullptr, 0, flags);
}
int vag_beam_step_dev_opt(float* logp, int64_t ldl, float* nll, int64_t* beam, int32_t* di_state, int64_t max_len,
                          const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k, int64_t V, int64_t H,
                          int32_t* n_alive, void* scratch, int32_t flags, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_step_launch(logp, ldl, nll, beam, 0, di_state, max_len, h_in, h_out, tok_out, B, k, V, H, n_alive, scratch,
                                S_(stream), nullptr, 0, flags);
}
int vag_beam_step_logits_dev_opt(float* logits, int64_t ldl, const float* parts, int64_t nparts, float* nll, int64_t* beam,
                                 int32_t* di_state, int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B,
                                 int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch, int32_t flags,
                                 vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr && parts != nullptr && nparts > 0);
    return vag_beam_step_launch(logits, ldl, nll, beam, 0, di_state, max_len, h_in, h_out, tok_out, B, k, V, H, n_alive, scratch,
                                S_(stream), parts, nparts, flags);
}
int vag_beam_ens_step_opt(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                          int64_t V, int32_t* n_alive, void* scratch, int32_t flags, vag_stream_t stream) {
    return vag_beam_ens_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, S_(stream), flags);
}
int vag_beam_ens_step_dev_opt(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam,
                              int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                              int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags,
                              vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_ens_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, S_(stream), flags);
}
int vag_beam_finish_nbest(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n,
                          int64_t* out, float* scores, vag_stream_t stream) {
    return vag_beam_finish_nbest_launch(nll, beam, max_len, steps, B, k, n, out, scores, S_(stream));
}
int vag_beam_finish_nbest_slots(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                int64_t n, int64_t* out, float* scores, int64_t* slots, vag_stream_t stream) {
    return vag_beam_finish_nbest_slots_launch(nll, beam, max_len, steps, B, k, n, out, scores, slots, S_(stream));
}
// diverse beam search: the grouped expansion (beam.hip)
int64_t vag_beam_div_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len) {
    (void)max_len;
    return vag_beam_div_scratch_bytes_impl(B, k, V);
}
int vag_beam_div_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int64_t groups, float strength,
                      vag_stream_t stream) {
    return vag_beam_div_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, flags, groups, strength, S_(stream));
}
int vag_beam_div_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int64_t groups,
                          float strength, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_div_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, flags, groups, strength, S_(stream));
}
// required phrases: the allotting expansion (beam.hip)
int64_t vag_beam_req_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len) {
    (void)max_len;
    return vag_beam_req_scratch_bytes_impl(B, k, V);
}
int vag_beam_req_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const int64_t* required, int32_t* state,
                      vag_stream_t stream) {
    return vag_beam_req_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, flags, required, state, S_(stream));
}
int vag_beam_req_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const int64_t* required,
                          int32_t* state, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_req_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, flags, required, state, S_(stream));
}
// stochastic beam search: the Gumbel-perturbed expansion (beam.hip)
int64_t vag_beam_sbs_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len) {
    (void)max_len;
    return vag_beam_sbs_scratch_bytes_impl(B, k, V);
}
int vag_beam_sbs_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const uint64_t* rng, float* gum,
                      vag_stream_t stream) {
    return vag_beam_sbs_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, flags, rng, gum, S_(stream));
}
int vag_beam_sbs_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const uint64_t* rng,
                          float* gum, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_sbs_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, flags, rng, gum, S_(stream));
}
// penalised beam search: coverage, the expansion that can select by the penalised score, its finish (beam.hip)
int64_t vag_beam_pen_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len) {
    if (B < 1 || k < 1 || k > 64 || V < k || max_len < 1) return VAG_EINVAL;
    return vag_beam_pen_scratch_bytes_impl(B, k, V);
}
int vag_beam_cover(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam, int64_t di,
                   int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row, float* cp_row, vag_stream_t stream) {
    return vag_beam_cover_launch(alpha, M, mask, cov, beam, di, nullptr, max_len, B, k, Tp, beta, cov_row, cp_row, S_(stream));
}
int vag_beam_cover_dev(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam,
                       const int32_t* di_state, int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row,
                       float* cp_row, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_cover_launch(alpha, M, mask, cov, beam, 0, di_state, max_len, B, k, Tp, beta, cov_row, cp_row, S_(stream));
}
int vag_beam_pen_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int32_t* lens, const float* cp_row, float* cpen,
                      const float* cov_row, float* cov, int64_t Tp, const float* lp, const float* bonus, int32_t stepwise,
                      vag_stream_t stream) {
    return vag_beam_pen_step_launch(logp, ldl, M, nll, beam, di, nullptr, max_len, h_in, h_out, H, nullptr, B, k, V, n_alive,
                                    scratch, flags, lens, cp_row, cpen, cov_row, cov, Tp, lp, bonus, stepwise, S_(stream));
}
int vag_beam_pen_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int32_t* lens,
                          const float* cp_row, float* cpen, const float* cov_row, float* cov, int64_t Tp, const float* lp,
                          const float* bonus, int32_t stepwise, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_pen_step_launch(logp, ldl, M, nll, beam, 0, di_state, max_len, h_in, h_out, H, tok_out, B, k, V, n_alive,
                                    scratch, flags, lens, cp_row, cpen, cov_row, cov, Tp, lp, bonus, stepwise, S_(stream));
}
int vag_beam_finish_pen(const float* nll, const int64_t* beam, const int32_t* lens, const float* cpen, const float* lp,
                        const float* bonus, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n, int64_t* out,
                        float* scores, int64_t* slots, float* logp, int32_t* length, float* cp, vag_stream_t stream) {
    return vag_beam_finish_pen_launch(nll, beam, lens, cpen, lp, bonus, max_len, steps, B, k, n, out, scores, slots, logp, length,
                                      cp, S_(stream));
}
// constrained beam search: the mask over the step's rows (constrain.hip)
int vag_beam_constrain(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di, int64_t max_len,
                       int64_t B, int64_t k, int64_t V, const int64_t* prefix, int64_t Lp, const int64_t* phrases,
                       const int32_t* phrase_sent, int64_t P, int64_t ngram, vag_stream_t stream) {
    return vag_beam_constrain_launch(logp, ldl, M, beam, di, nullptr, false, max_len, B, k, V, prefix, Lp, phrases, phrase_sent, P,
                                     ngram, S_(stream));
}
int vag_beam_constrain_dev(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, const int32_t* di_state,
                           int64_t max_len, int64_t B, int64_t k, int64_t V, const int64_t* prefix, int64_t Lp,
                           const int64_t* phrases, const int32_t* phrase_sent, int64_t P, int64_t ngram, vag_stream_t stream) {
    return vag_beam_constrain_launch(logp, ldl, M, beam, 0, di_state, true, max_len, B, k, V, prefix, Lp, phrases, phrase_sent, P,
                                     ngram, S_(stream));
}
// kNN-MT: the datastore's append, the nearest-neighbour search and the mix over the step's rows (knn.hip)
int64_t vag_knn_slice(void) { return VAG_KNN_SLICE; }
int64_t vag_knn_row_tile(int64_t D) { return vag_knn_row_tile_host(D); }
int64_t vag_knn_scratch_bytes(int64_t R, int64_t N, int64_t K) { return vag_knn_scratch_bytes_host(R, N, K); }
int vag_knn_store_rows(const float* h2, const int64_t* tgt, int64_t B, int64_t Tt, int64_t H, int64_t sent_base, int64_t cap,
                       void* keys, float* norm, int32_t* value, int32_t* sentence, int32_t* position, int32_t* count,
                       vag_stream_t stream) {
    return vag_knn_store_rows_launch(h2, tgt, B, Tt, H, sent_base, cap, keys, norm, value, sentence, position, count, S_(stream));
}
int vag_knn_search(const float* q, int64_t ldq, int64_t R, int64_t D, const void* keys, const float* norm, int64_t N, int64_t K,
                   float* out_score, int32_t* out_index, void* scratch, vag_stream_t stream) {
    return vag_knn_search_launch(q, ldq, R, D, keys, norm, N, K, out_score, out_index, scratch, S_(stream));
}
int vag_knn_mix(float* const* logp, const int64_t* ldl, int64_t M, int64_t R, int64_t V, const float* const* nb_score,
                const int32_t* const* nb_index, int64_t K, const int32_t* const* values, const int64_t* n_values,
                const float* const* lse, float inv_T, float log_lam, float log1m_lam, vag_stream_t stream) {
    return vag_knn_mix_launch(logp, ldl, M, R, V, nb_score, nb_index, K, values, n_values, lse, inv_T, log_lam, log1m_lam, S_(stream));
}
// shallow fusion with a back-off n-gram language model (lm.hip)
int vag_lm_fuse_rows(float* const* rows, const int64_t* ld, int64_t M, int64_t R, int64_t V, const vag_lm* lm, const int32_t* ctx,
                     float beta, vag_stream_t stream) {
    return vag_lm_fuse_rows_launch(rows, ld, M, R, V, lm, ctx, beta, S_(stream));
}
int vag_lm_fuse_beam(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di, int64_t max_len,
                     int64_t B, int64_t k, int64_t V, const vag_lm* lm, float beta, vag_stream_t stream) {
    return vag_lm_fuse_beam_launch(logp, ldl, M, beam, di, nullptr, false, max_len, B, k, V, lm, beta, S_(stream));
}
int vag_lm_fuse_beam_dev(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, const int32_t* di_state,
                         int64_t max_len, int64_t B, int64_t k, int64_t V, const vag_lm* lm, float beta, vag_stream_t stream) {
    return vag_lm_fuse_beam_launch(logp, ldl, M, beam, 0, di_state, true, max_len, B, k, V, lm, beta, S_(stream));
}
int vag_lm_query(const vag_lm* lm, const int32_t* ctx, const int32_t* word, int64_t R, float* logp_out, int32_t* order_out,
                 vag_stream_t stream) {
    return vag_lm_query_launch(lm, ctx, word, R, logp_out, order_out, S_(stream));
}
int vag_forced_score(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, const int64_t* tgt,
                     int64_t B, int64_t Tt, int64_t V, float* token_logp, float* logp, float* score, vag_stream_t stream) {
    return vag_forced_score_launch(logits, ldl, lse, M, tgt, B, Tt, V, token_logp, logp, score, S_(stream));
}
int vag_token_conf(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, const int64_t* tgt,
                   int64_t B, int64_t Tt, int64_t V, float* token_logp, float* entropy, int32_t* rank, int32_t* top, float* top_logp,
                   float* sent, vag_stream_t stream) {
    return vag_token_conf_launch(logits, ldl, lse, M, tgt, B, Tt, V, token_logp, entropy, rank, top, top_logp, sent, S_(stream));
}
int vag_beam_attn_record(const float* const* alpha, int64_t M, float* attn_hist, int64_t di, int64_t max_len, int64_t B, int64_t k,
                         int64_t Tp, vag_stream_t stream) {
    return vag_beam_attn_record_launch(alpha, M, attn_hist, di, nullptr, max_len, B, k, Tp, S_(stream));
}
int vag_beam_attn_record_dev(const float* const* alpha, int64_t M, float* attn_hist, const int32_t* di_state, int64_t max_len,
                             int64_t B, int64_t k, int64_t Tp, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_beam_attn_record_launch(alpha, M, attn_hist, 0, di_state, max_len, B, k, Tp, S_(stream));
}
int vag_beam_finish_align(const float* nll, const int64_t* beam, const float* attn_hist, int64_t max_len, int64_t steps, int64_t B,
                          int64_t k, int64_t n, int64_t Tp, int64_t Ts, int64_t* out, float* scores, float* attention,
                          int64_t* src_pos, vag_stream_t stream) {
    return vag_beam_finish_align_launch(nll, beam, attn_hist, max_len, steps, B, k, n, Tp, Ts, out, scores, attention, src_pos,
                                        S_(stream));
}
int vag_forced_align(const float* const* alpha, int64_t M, const int64_t* tgt, int64_t B, int64_t Tt, int64_t Ts, float* attention,
                     int64_t* src_pos, vag_stream_t stream) {
    return vag_forced_align_launch(alpha, M, tgt, B, Tt, Ts, attention, src_pos, S_(stream));
}

int vag_sample_step(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                    int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out, int64_t B,
                    int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng, int32_t* n_alive,
                    vag_stream_t stream) {
    return vag_sample_step_launch(logp, ldl, M, toks, token_logp, di, nullptr, max_len, h_in, h_out, H, tok_out, B, n, V, temperature,
                                  top_k, rng, n_alive, S_(stream));
}
int vag_sample_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int32_t* di_state,
                        int64_t max_len, int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k,
                        const uint64_t* rng, int32_t* n_alive, vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_sample_step_launch(logp, ldl, M, toks, token_logp, 0, di_state, max_len, nullptr, nullptr, nullptr, tok_out, B, n, V,
                                  temperature, top_k, rng, n_alive, S_(stream));
}
int vag_sample_step_p(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out, int64_t B,
                      int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng, int32_t* n_alive, float top_p,
                      int32_t* set_size, vag_stream_t stream) {
    return vag_sample_step_p_launch(logp, ldl, M, toks, token_logp, di, nullptr, max_len, h_in, h_out, H, tok_out, B, n, V,
                                    temperature, top_k, rng, n_alive, top_p, set_size, S_(stream));
}
int vag_sample_step_p_dev(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp,
                          int32_t* di_state, int64_t max_len, int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature,
                          int64_t top_k, const uint64_t* rng, int32_t* n_alive, float top_p, int32_t* set_size,
                          vag_stream_t stream) {
    VAG_CHECK_ARG(di_state != nullptr);
    return vag_sample_step_p_launch(logp, ldl, M, toks, token_logp, 0, di_state, max_len, nullptr, nullptr, nullptr, tok_out, B, n,
                                    V, temperature, top_k, rng, n_alive, top_p, set_size, S_(stream));
}
int vag_sample_noise(const uint64_t* rng, int64_t di, int64_t N, int64_t V, float* out, vag_stream_t stream) {
    return vag_sample_noise_launch(rng, di, N, V, out, S_(stream));
}

int vag_mbr_supported(int64_t Nh, int64_t Lh, int64_t Nr, int64_t Lr) { return vag_mbr_supported_host(Nh, Lh, Nr, Lr); }
int vag_mbr_select(const int64_t* hyps, const int64_t* refs, const float* weights, int64_t B, int64_t Nh, int64_t Lh, int64_t Nr,
                   int64_t Lr, int utility, int32_t* matches, float* util, float* expected, int64_t* best, vag_stream_t stream) {
    return vag_mbr_select_launch(hyps, refs, weights, B, Nh, Lh, Nr, Lr, utility, matches, util, expected, best, S_(stream));
}

int vag_corpus_bleu_supported(int64_t Lh, int64_t R, int64_t Lr) { return vag_corpus_bleu_supported_host(Lh, R, Lr); }
int vag_corpus_bleu_stats(const int64_t* hyps, const int64_t* refs, const int32_t* n_refs, int64_t N, int64_t Lh, int64_t R,
                          int64_t Lr, int32_t* per_sentence, int64_t* totals, vag_stream_t stream) {
    return vag_corpus_bleu_stats_launch(hyps, refs, n_refs, N, Lh, R, Lr, per_sentence, totals, S_(stream));
}

int vag_surface_expand(const int64_t* rows, int64_t R, int64_t L, const int32_t* off, const int32_t* chars, int64_t V, int32_t* out,
                       int64_t C, int32_t* lens, vag_stream_t stream) {
    return vag_surface_expand_launch(rows, R, L, off, chars, V, out, C, lens, S_(stream));
}
int vag_chrf_supported(int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr) { return vag_chrf_supported_host(Nh, Ch, Nr, Cr); }
int vag_chrf_max_chars(void) { return vag_chrf_max_chars_host(); }
int vag_chrf_select(const int32_t* hchars, const int32_t* hlens, const int32_t* rchars, const int32_t* rlens, const float* weights,
                    int64_t B, int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr, int32_t* matches, float* util, float* expected,
                    int64_t* best, vag_stream_t stream) {
    return vag_chrf_select_launch(hchars, hlens, rchars, rlens, weights, B, Nh, Ch, Nr, Cr, matches, util, expected, best, S_(stream));
}

int vag_mrt_weights(const float* nll, const float* cost, const float* valid, int64_t B, int64_t Tt, int64_t N, float alpha, float scale,
                    float* inv_cnt, float* q, float* risk, vag_stream_t stream) {
    VAG_CHECK_ARG(risk != nullptr);
    return vag_mrt_weights_launch(nll, cost, valid, B, Tt, N, alpha, scale, inv_cnt, q, risk, nullptr, 0.f, 0, S_(stream));
}
int vag_mrt_pack(const int64_t* cand, int64_t G, int64_t Nc, int64_t L, const int64_t* gold, int64_t Tg, int include_gold, int64_t* tgt,
                 int64_t Tt, float* valid, vag_stream_t stream) {
    return vag_mrt_pack_launch(cand, G, Nc, L, gold, Tg, include_gold, tgt, Tt, valid, S_(stream));
}

int vag_clip_adam_flat(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                       const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1, float beta2,
                       float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch, const float* lr_dev,
                       vag_stream_t stream) {
    return vag_clip_adam_launch(p, g, m, v, n, nseg, seg_off, seg_lr, seg_wd, clip, grad_scale, beta1, beta2, eps, zero_grad,
                                step, norm_out, scratch, lr_dev, S_(stream));
}

int vag_clip_adam_flat_ema(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                           const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1, float beta2,
                           float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch, const float* lr_dev,
                           float* ema, float ema_decay, int ema_warmup, vag_stream_t stream) {
    return vag_clip_adam_ema_launch(p, g, m, v, n, nseg, seg_off, seg_lr, seg_wd, clip, grad_scale, beta1, beta2, eps, zero_grad,
                                    step, norm_out, scratch, lr_dev, ema, ema_decay, ema_warmup, S_(stream));
}

int vag_swap_flat(float* a, float* b, int64_t n, vag_stream_t stream) { return vag_swap_flat_launch(a, b, n, S_(stream)); }

int vag_clip_adam_shard(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off, const float* seg_lr,
                        const float* seg_wd, float clip, float grad_scale, float beta1, float beta2, float eps, int zero_grad,
                        int32_t* step, float* norm_out, void* scratch, const float* lr_dev, int64_t lo, int64_t hi, int phase,
                        double* sumsq, vag_stream_t stream) {
    return vag_clip_adam_shard_launch(p, g, m, v, n, nseg, seg_off, seg_lr, seg_wd, clip, grad_scale, beta1, beta2, eps, zero_grad,
                                      step, norm_out, scratch, lr_dev, lo, hi, phase, sumsq, S_(stream));
}

int vag_copy4(const void* const* src, void* const* dst, const int64_t* bytes, int n, vag_stream_t stream) {
    return vag_copy4_launch(src, dst, bytes, n, S_(stream));
}

int vag_recurrence_supported(int kind, int64_t B, int64_t Ts, int64_t Tt, int64_t H) {
    if (kind == 0) return vag_enc_persistent_ok(B, Ts, H) ? 1 : 0;
    if (kind == 1) return vag_dec_persistent_ok(B, Ts, Tt, H) ? 1 : 0;
    if (kind == 2) return vag_dec_bwd_persistent_ok(B, Ts, Tt, H) ? 1 : 0;
    return 0;
}
int vag_persistent_timeouts(void) { return vag_persistent_timeouts_read(); }
int vag_attn_energy_probe(const float* a, const float* b, int64_t n, float* out, vag_stream_t stream) {
    return vag_attn_energy_probe_launch(a, b, n, out, S_(stream));
}
int64_t vag_handoff_planes_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t H) {
    // the two forward recurrences of a step hold their regions at the same time (the decoder's behind the encoder's); each backward
    // one has the buffer to itself
    const int64_t e = vag_enc_bwd_planes_floats(B, Ts, H), d = vag_dec_bwd_planes_floats(B, Tt, H);
    const int64_t f = vag_enc_fwd_planes_floats(B, Ts, H) + vag_dec_fwd_planes_floats(B, Tt, H);
    return std::max(std::max(e, d), f);
}
int vag_set_handoff_planes(float* buf, int64_t floats) {
    VAG_CHECK_ARG((buf == nullptr || (floats > 0 && aligned16(buf))));
    g_base_ctx.handoff_planes = buf;
    g_base_ctx.handoff_floats = buf ? floats : 0;
    return VAG_OK;
}
int vag_set_operator_guard(void* guard) {
    VAG_CHECK_ARG((reinterpret_cast<uintptr_t>(guard) & 3) == 0);
    g_base_ctx.guard = reinterpret_cast<unsigned*>(guard);
    return VAG_OK;
}
int vag_gemm_group_plan(int n, const int64_t* M, const int64_t* N, const int64_t* K, const int* accumulate, int* split,
                        int* order) {
    return vag_gemm_group_plan_host(n, M, N, K, accumulate, split, order);
}
int vag_gemm_plan(int64_t M, int64_t N, int64_t K, int a_kc, int b_kc, int vec, float beta, int act, int c_half, int a_bf16,
                  int rowsum, int planes, int* plan) {
    return vag_gemm_plan_host(M, N, K, a_kc, b_kc, vec, beta, act, c_half, a_bf16, rowsum, planes, plan);
}
int vag_recurrence_time(int kind, double* ms_total, int* launches) { return vag_persistent_time_read(kind, ms_total, launches); }
int64_t vag_recurrence_sync_words(int kind, int64_t B, int64_t T) {
    return kind == 0 ? vag_enc_persistent_sync_words(B, T) : vag_dec_persistent_sync_words(B, T);
}
int vag_dropout_mask(const uint64_t* rng, int which, int64_t n, float p, float* out, vag_stream_t stream) {
    VAG_CHECK_ARG(which >= 1 && which <= 3);
    return vag_dropout_mask_launch(rng, which, n, p, out, S_(stream));
}
int vag_rng_advance(uint64_t* rng, vag_stream_t stream) { return vag_rng_advance_launch(rng, S_(stream)); }
