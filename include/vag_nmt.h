/* vag_nmt.h -- C ABI of libvagnmt.so: the VAG-NMT per-step training / decode hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference (Eurus-Holmes/VAG-NMT) is pure Python on torch; the functions
 * below replace the torch-op sequences of its hot path, and each comment cites the reference code it stands
 * in for (paths relative to the reference checkout).  The Python host side in
 * vag-nmt_amd/machine_translation_vision/ mirrors the reference's module API and calls these entry points
 * through ctypes.
 *
 * Conventions
 *   - All tensors are dense row-major fp32 on the current HIP device unless stated; token ids are int64
 *     (torch.LongTensor, as in the reference); lengths are int32 on the device.
 *   - Source-side sequences are batch-major inside the library: enc/pe are (B,Ts,C), C = 2H.
 *     Decoder-side per-step tensors are time-major: (Tt,B,*).
 *   - Ownership: the caller owns every buffer, including workspaces ("ws", sizes from *_ws_floats()).  The
 *     library never allocates or frees device memory and keeps no pointer after a call returns.
 *   - All work is enqueued on `stream`; nothing synchronises with the host, so every call can be captured
 *     into a HIP graph.  Calls are re-entrant across streams.
 *   - Gradient outputs named g_* are ACCUMULATED (+=) into the caller's buffers (zero them per step);
 *     outputs named d_* are written.
 *   - Return value: 0 ok; <0 argument/shape error (-22 = EINVAL); >0 a hipError_t.
 *   - Dropout: `rng` points to two device uint64 {seed, step}; masks are a pure function of
 *     (seed, step, stream-id, element index) so backward recomputes them.  rng == NULL or p == 0: no dropout
 *     (eval mode).  vag_dropout_mask() materialises a mask for tests.
 */
#ifndef VAG_NMT_H
#define VAG_NMT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vag_stream_t; /* hipStream_t */

/* GRU parameter bundle, torch gate order (r,z,n): w_ih (3H,in), w_hh (3H,H), b_ih (3H), b_hh (3H). */
typedef struct { const float *w_ih, *w_hh, *b_ih, *b_hh; } vag_gru_w;
typedef struct { float *w_ih, *w_hh, *b_ih, *b_hh; } vag_gru_g;

/* Decoder recurrent parameters (layers/NMT_Decoder.py:78-86): embedding (V,E); gru_1 (in=E); attn_h (C,H);
 * attn.v (C); context2hid (H,C); gru_2 (in=H). */
typedef struct {
    const float* emb;
    vag_gru_w gru1;
    const float *attn_h, *attn_v, *c2h;
    vag_gru_w gru2;
} vag_dec_w;
typedef struct {
    float* emb;
    vag_gru_g gru1;
    float *attn_h, *attn_v, *c2h;
    vag_gru_g gru2;
} vag_dec_g;

/* Output-head parameters (layers/NMT_Decoder.py:89-106): W1 (E,H), W2 (E,C), W3 (E,E), out (V,E)+(V).
 * With tied embeddings `out_w` is the decoder embedding matrix. */
typedef struct { const float *w1, *b1, *w2, *b2, *w3, *b3, *out_w, *out_b; } vag_head_w;
typedef struct { float *w1, *b1, *w2, *b2, *w3, *b3, *out_w, *out_b; } vag_head_g;

int vag_version(void);

/* ---- generic dense products (torch.nn.Linear / torch.mm call sites on the path) ---------------------- */
/* C[M,N] = act(alpha * op(A) op(B) + beta*C + bias[n]).  A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn];
 * one stride of each operand must be 1.  act: 0 none, 1 tanh.  Arithmetic: fp32-grade.  Products with M,N > 64 run on
 * the bf16 matrix pipes with every fp32 operand split exactly into three bf16 parts and the six partial products with
 * i+j <= 4 accumulated in fp32 ("bf16x6": relative error of a term ~2^-24, the class of a reassociated fp32 sum;
 * bounded against the exact-f32 kernel in tests/test_gpu_kernels.py); smaller ones and VAG_GEMM_F32MFMA=1 use the
 * f32-input MFMA (exact f32 fma chains). */
int vag_gemm_f32(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t sam, int64_t sak,
                 const float* B, int64_t sbk, int64_t sbn, float beta, float* C, int64_t ldc,
                 const float* bias, int act, vag_stream_t stream);
/* y[M,N] = act(x[M,K] W[N,K]^T + bias)  -- nn.Linear forward; picks the small-M kernel for M <= 128. */
int vag_linear_fwd(int64_t M, int64_t N, int64_t K, const float* x, const float* W, const float* bias, int act,
                   float* y, vag_stream_t stream);
/* nn.Linear backward.  If act==1, dy is first multiplied in place by (1 - y^2).  d_x (may be NULL) is
 * written or, if accumulate_dx, added to; g_W, g_b (may be NULL) are accumulated. */
int vag_linear_bwd(int64_t M, int64_t N, int64_t K, const float* x, const float* W, const float* y, float* dy,
                   int act, float* d_x, int accumulate_dx, float* g_W, float* g_b, vag_stream_t stream);

/* ---- embedding (nn.Embedding(padding_idx=0), layers/Encoder.py:22,50; layers/NMT_Decoder.py:78,118) --- */
int vag_embed_fwd(const int64_t* idx, int64_t n, const float* W, int64_t E, float* out, vag_stream_t stream);
int vag_embed_bwd(const int64_t* idx, int64_t n, const float* d_out, int64_t E, float* g_W, vag_stream_t stream);

/* ---- a3: bi-GRU encoder, layers/Encoder.py:36-66 ------------------------------------------------------ */
/* src (B,Ts) int64 padded with 0; lengths int32[B] on device (descending).  Writes enc (B,Ts,2H)
 * (forward direction in [:H], reverse in [H:], zeros past each row's length) and mask (B,Ts) = (src != 0).
 * p_emb / p_ctx: dropout on the embedded input / on the output (Encoder.py:51-52,:63-64).
 * ws: vag_bigru_ws_floats(B,Ts,E,H) floats, must stay untouched until the matching backward. */
int64_t vag_bigru_ws_floats(int64_t B, int64_t Ts, int64_t E, int64_t H);
int vag_bigru_seq_fwd(const int64_t* src, const int32_t* lengths, const float* emb, vag_gru_w fwd, vag_gru_w bwd,
                      float p_emb, float p_ctx, const uint64_t* rng, int64_t B, int64_t Ts, int64_t E, int64_t H,
                      float* enc, float* mask, float* ws, vag_stream_t stream);
/* d_enc (B,Ts,2H) is consumed (overwritten).  Accumulates g_emb (Vs,E; pad row untouched) and both GRUs. */
int vag_bigru_seq_bwd(const int64_t* src, const int32_t* lengths, vag_gru_w fwd, vag_gru_w bwd, float p_emb,
                      float p_ctx, const uint64_t* rng, int64_t B, int64_t Ts, int64_t E, int64_t H, float* d_enc,
                      float* ws, float* g_emb, vag_gru_g g_fwd, vag_gru_g g_bwd, vag_stream_t stream);

/* ---- one GRU cell step (torch nn.GRU on a length-1 sequence, layers/NMT_Decoder.py:121) ------------------ */
/* gi (M,3H) = W_ih x + b_ih (already projected); computes W_hh h_prev + b_hh, the gates and the blend in one
 * launch (the kernel every recurrent step of the encoder and decoder runs).  save: NULL or [4][M][H] (r,z,n,hn). */
int vag_gru_cell_fwd(const float* gi, const float* h_prev, const float* w_hh, const float* b_hh, int64_t M,
                     int64_t H, float* h_out, float* save, vag_stream_t stream);

/* One backward step of the same recurrence (what autograd replays per time step for nn.GRU, layers/Encoder.py:58,
 * layers/NMT_Decoder.py:121,129), fused the way the sequence operators run it:
 *   dh  = dgh_next W_hh + carry + d_out        dgh_next (M,3H): gradient of the LATER step's hidden projection,
 *                                              w_hh_t (H,3H) = W_hh^T, carry / d_out (M,H) may be NULL
 *   dgi (M,3H), dgh (M,3H) = cell backward of THIS step (save [4][M][H] from vag_gru_cell_fwd, h_prev (M,H))
 *   carry_out (M,H) = z * dh                   (the part of dh that flows to the previous step directly) */
int vag_gru_cell_bwd(const float* dgh_next, const float* w_hh_t, const float* carry, const float* d_out,
                     const float* save, const float* h_prev, int64_t M, int64_t H, float* dgi, float* dgh,
                     float* carry_out, vag_stream_t stream);

/* ---- a4 (hoisted part): attention keys pe = enc W_e^T, layers/NMT_Decoder.py:47 ----------------------- */
/* The reference recomputes attn_e(encoder_outputs) at every decoder step; it does not depend on the step,
 * so it is computed once per batch.  rows = B*Ts. */
int vag_attn_keys_proj(const float* enc, const float* attn_e, int64_t rows, int64_t C, float* pe,
                       vag_stream_t stream);
/* a4 stand-alone (BahdanauAttn.forward, layers/NMT_Decoder.py:27-51), inference: q (N,C) = attn_h(hidden);
 * alpha[n,:] = softmax_s(v . tanh(pe[n/rows_per_src,s] + q[n])) with masked positions at -inf; ctx = alpha . enc. */
int vag_bahdanau_attn_fwd(const float* pe, const float* q, const float* v, const float* mask, const float* enc,
                          int64_t N, int64_t rows_per_src, int64_t Ts, int64_t C, float* scores, float* alpha,
                          float* ctx, vag_stream_t stream);
/* d_enc (+)= d_pe attn_e ; g_attn_e += d_pe^T enc */
int vag_attn_keys_proj_bwd(const float* enc, const float* attn_e, const float* d_pe, int64_t rows, int64_t C,
                           float* d_enc, int accumulate_enc, float* g_attn_e, vag_stream_t stream);

/* ---- a5: cGRU decoder with Bahdanau attention, layers/NMT_Decoder.py:109-131 -------------------------- */
/* Whole target sequence.  tok (Tt+1,B) int64: row 0 = SOS, row t+1 = input of step t+1.  Teacher forcing
 * (models/...V11.py:138-146): the caller fills every row.  Free running (V11.py:148-160, free_run=1): rows
 * 1.. are written here with the argmax of each step's output distribution, for which the head parameters,
 * `tmid` (Tt,B,E) and `logits` (Tt*B, ldl) are also produced step by step (p_out = head dropout).
 * Outputs for the head: h2_all (Tt,B,H), c_all (Tt,B,C), e_all (Tt,B,E).
 * ws: vag_cgru_ws_floats(B,Ts,Tt,E,H) floats, kept for the backward. */
int64_t vag_cgru_ws_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H);
/* float offset of a saved per-step tensor inside ws (parity tests): 0 alpha (Tt,B,Ts), 1 h1 (Tt,B,H), 2 [q | W_hh2 h1 + b] */
int64_t vag_cgru_ws_offset(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int which);
int vag_cgru_attn_decode_seq_fwd(const float* enc, const float* pe, const float* mask, const float* h0,
                                 int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                                 int64_t H, int64_t V, float* h2_all, float* c_all, float* e_all, float* ws,
                                 int free_run, const vag_head_w* head, float p_out, const uint64_t* rng,
                                 float* tmid, float* logits, int64_t ldl, vag_stream_t stream);
/* The free-running form as ONE launch (round 4; persist.hip: the recurrence kernel also forms the head's hidden layer, the
 * logits of its vocabulary tiles and the arg-max, and feeds the token back: two more hand-offs per step instead of nine
 * launches).  Same outputs and saved tensors as vag_cgru_attn_decode_seq_fwd(free_run = 1), so the backward entry points
 * are unchanged.  vag_cgru_free_supported: H = 512, E = 256, B <= 64, keys fit the LDS, every workgroup resident.
 * tables: vag_cgru_free_tables_floats floats of scratch (the input projection of every vocabulary entry, emb W3^T, enc W2^T,
 * arg-max candidates), filled here.  logits may be NULL (greedy decoding, V11.py:207-226: only tok is read); c_all / e_all
 * may be NULL then too. */
int vag_cgru_free_supported(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V);
int64_t vag_cgru_free_tables_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V);
int vag_cgru_attn_decode_free_fwd(const float* enc, const float* pe, const float* mask, const float* h0, int64_t* tok,
                                  vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V,
                                  float* h2_all, float* c_all, float* e_all, float* ws, const vag_head_w* head,
                                  float p_out, const uint64_t* rng, float* tmid, float* logits, int64_t ldl,
                                  float* tables, vag_stream_t stream);
/* Backward through time.  Inputs: gradients w.r.t. the three outputs (d_h2_all, d_c_all are consumed;
 * d_e_all may be NULL).  Writes d_enc_out (B,Ts,C) (accumulate_enc: adds), d_pe (B,Ts,C), d_h0 (B,H);
 * accumulates the parameter gradients in g (g.emb: pad row untouched). */
int vag_cgru_attn_decode_seq_bwd(const float* enc, const float* pe, const float* mask, const float* h0,
                                 const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                                 int64_t H, int64_t V, const float* h2_all, const float* c_all, const float* e_all,
                                 float* d_h2_all, float* d_c_all, const float* d_e_all, float* ws, float* d_enc_out,
                                 int accumulate_enc, float* d_pe, float* d_h0, vag_dec_g g, float* scratch,
                                 vag_stream_t stream);
int64_t vag_cgru_bwd_scratch_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H);
/* The same backward in two phases, for callers that overlap them on two streams: _loop is the recurrence (writes
 * d_enc_out, d_pe, d_h0 and leaves the per-step tensors in `scratch`); _weights turns those into the parameter
 * gradients (large products nothing downstream waits for).  ws/scratch must stay untouched in between. */
int vag_cgru_attn_decode_seq_bwd_loop(const float* enc, const float* pe, const float* mask, const float* h0,
                                      const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                                      int64_t H, int64_t V, const float* h2_all, const float* c_all,
                                      const float* e_all, float* d_h2_all, float* d_c_all, const float* d_e_all,
                                      float* ws, float* d_enc_out, int accumulate_enc, float* d_pe, float* d_h0,
                                      float* scratch, vag_stream_t stream);
int vag_cgru_attn_decode_seq_bwd_weights(const float* h0, const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts,
                                         int64_t Tt, int64_t E, int64_t H, const float* h2_all, const float* c_all,
                                         const float* e_all, const float* d_e_all, float* ws, vag_dec_g g,
                                         float* scratch, vag_stream_t stream);

/* One inference step for N hypotheses (greedy / beam search, models/...V11.py:207-226,259-313).  Hypothesis n
 * attends over source sentence n / rows_per_src (the reference tiles encoder_outputs by beam_size, :253).
 * tok int64[N]; h_in (N,H) -> h_out (N,H), c (N,C), e (N,E).  scratch: vag_cgru_step_scratch_floats(). */
/* `prep`: vag_cgru_prep_floats(H) floats filled by vag_cgru_prepare() once per decode call (derived weights:
 * [attn_h ; gru_2.w_hh] stacked so both products of h1 are one launch, and gru_2.w_ih . context2hid folded: decoding
 * steps and the free-running launch chain read it; the teacher-forced sequence operators apply context2hid and gru_2.w_ih to the
 * keys one after the other instead). */
int64_t vag_cgru_prep_floats(int64_t H);
int vag_cgru_prepare(vag_dec_w w, int64_t H, float* prep, vag_stream_t stream);
int64_t vag_cgru_step_scratch_floats(int64_t N, int64_t Ts, int64_t E, int64_t H);
int vag_cgru_attn_decode_step(const float* enc, const float* pe, const float* mask, int64_t rows_per_src,
                              const int64_t* tok, const float* h_in, vag_dec_w w, const float* prep, int64_t N,
                              int64_t Ts, int64_t E, int64_t H, float* h_out, float* c, float* e, float* alpha,
                              float* scratch, vag_stream_t stream);

/* ---- a5 (head) + a2 loss: layers/NMT_Decoder.py:137-143, models/...V11.py:140,164 --------------------- */
/* t = tanh(W1 h2 + W2 c + W3 e + b1+b2+b3); dropout p_out; logits = t out_w^T + out_b; log_softmax;
 * nll[t,b] = -weight[tgt[b,t]] * logp[tgt[b,t]]  (nn.NLLLoss(weight, reduce=False));
 * loss_mt = mean_b( sum_t nll[t,b] / #nonpad(tgt[b,:]) ).
 * rows = Tt*B time-major; tgt (B,Tt) int64; logits (rows, ldl) with ldl >= V, ldl % 4 == 0 (kept for bwd).
 * logits_ready=1: tmid/logits were already produced (free-running decode), only the loss is computed.
 * Outputs: lse (rows), nll (rows), loss_mt (1), inv_cnt (B). */
int vag_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                        const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                        int64_t V, float p_out, const uint64_t* rng, int logits_ready, float* tmid, float* logits,
                        int64_t ldl, float* lse, float* nll, float* inv_cnt, float* loss_mt, vag_stream_t stream);
/* d_loss: device scalar (gradient of loss_mt).  logits is overwritten with d(logits).  Writes d_h2_all,
 * d_c_all, d_e_all; accumulates g.  scratch: rows*E floats. */
int vag_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                        const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                        int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits, int64_t ldl,
                        const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                        float* d_c_all, float* d_e_all, vag_head_g g, float* scratch, vag_stream_t stream);
/* vag_head_ce_seq_bwd in two phases (see vag_cgru_attn_decode_seq_bwd_loop): _data writes d_h2_all/d_c_all/d_e_all and
 * leaves d(logits) in `logits` and d(pre-activation) in `scratch` (R*E floats); vag_head_bwd_weights accumulates g. */
int vag_head_ce_seq_bwd_data(vag_head_w w, const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt,
                             int64_t E, int64_t H, int64_t V, float p_out, const uint64_t* rng, const float* tmid,
                             float* logits, int64_t ldl, const float* lse, const float* inv_cnt, const float* d_loss,
                             float* d_h2_all, float* d_c_all, float* d_e_all, float* scratch, vag_stream_t stream);
int vag_head_bwd_weights(const float* h2_all, const float* c_all, const float* e_all, int64_t R, int64_t E, int64_t H,
                         int64_t V, const float* tmid, const float* dlogits, int64_t ldl, const float* dt, vag_head_g g,
                         vag_stream_t stream);
/* The same three calls with label smoothing eps = label_smoothing, 0 <= eps < 1 (else, and for NaN, -EINVAL).  With
 * y = tgt[b,t], w = vocab_weight[y], x the row's V logits and lse = logsumexp(x):
 *   nll[t,b] = w * ( lse - (1 - eps) * x[y] - eps * (1/V) * sum_{j<V} x[j] )
 *            = w * ( (1 - eps) * (-logp[y]) + eps * mean_j(-logp[j]) ),
 *   loss_mt as above;   d x[j] = coef * ( softmax(x)[j] - (1 - eps) * [j == y] - eps / V ),
 *   coef = d_loss * inv_cnt[b] / B * w  (unchanged).
 * With unit weights this is cross_entropy(label_smoothing = eps); the row weight multiplies the whole row (PAD rows give 0).
 * The padding columns V <= j < ldl are outside the mean and keep a zero gradient.  Nothing else changes: same saved tensors
 * (backward needs only lse), same scratch, every form of the head (row chunks with and without the chunk's backward inside the
 * forward, logits_ready = 1, the bf16 d(logits) of the 2-byte storage mode).  eps = 0 is exactly the function without _ls:
 * the same kernels are launched.  Backward must be given the eps of its forward. */
int vag_head_ce_seq_fwd_ls(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                           const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                           int64_t V, float p_out, const uint64_t* rng, int logits_ready, float* tmid, float* logits,
                           int64_t ldl, float* lse, float* nll, float* inv_cnt, float* loss_mt, float label_smoothing,
                           vag_stream_t stream);
int vag_head_ce_seq_bwd_ls(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                           const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                           int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits, int64_t ldl,
                           const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                           float* d_c_all, float* d_e_all, vag_head_g g, float* scratch, float label_smoothing,
                           vag_stream_t stream);
int vag_head_ce_seq_bwd_data_ls(vag_head_w w, const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt,
                                int64_t E, int64_t H, int64_t V, float p_out, const uint64_t* rng, const float* tmid,
                                float* logits, int64_t ldl, const float* lse, const float* inv_cnt, const float* d_loss,
                                float* d_h2_all, float* d_c_all, float* d_e_all, float* scratch, float label_smoothing,
                                vag_stream_t stream);
/* Word-level knowledge distillation (Kim & Rush 2016, "Sequence-Level Knowledge Distillation", section 3.1): the loss reads a
 * teacher distribution per target position, here a SPARSE one -- the teacher's K <= 64 best words of the position, renormalised
 * (vag_kd_targets writes it).  Rows are time-major, row = t*B + b, as lse and nll.  Per row, with y = tgt[b,t] the gold word,
 * w = vocab_weight[y], x the student's V logits, idx[0..K) DISTINCT words in [0, V) and q[0..K) their probabilities, sum_k q_k = 1:
 *   nll[t,b] = w * ( lse - (1 - lambda) * x[y] - lambda * sum_k q_k * x[idx_k] )
 *            = w * ( (1 - lambda) * CE(gold) + lambda * CE(teacher) ),
 *   loss_mt as in vag_head_ce_seq_fwd;
 *   d x[j] = coef * ( softmax(x)[j] - (1 - lambda) * [j == y] - lambda * sum_k q_k * [j == idx_k] ),
 *   coef = d_loss * inv_cnt[b] / B * w  (unchanged).
 * The row weight multiplies the whole row, as with label smoothing: PAD rows give exactly 0.  y may be one of the idx_k.
 * idx (Tt*B, K) int32 and q (Tt*B, K) float are device arrays the caller owns.  The V-wide kernels are those of the plain loss;
 * the soft part costs two launches per pass over rows that touch K + 1 logits of a row: one after the log-sum-exp pass rewrites
 * nll (the sum over k in a fixed order: reproducible), one after the softmax-minus-onehot pass adds + coef lambda at y and
 * - coef lambda q_k at idx_k in place (one combined update where idx_k == y; rows with coef == 0 and the padding columns
 * [V, ldl) are not touched) and the same amounts into g.out_b by fp32 atomicAdd.  g.out_b already is a sum of fp32 atomics (the
 * column sums of d(logits)), so its last bits depend on arrival order with and without distillation; everything else is
 * reproducible.  Every form of the head applies it: the whole sequence and row chunks with and without the chunk's backward
 * inside the forward.  K = 1 with idx = y, q = 1 is the plain loss for every lambda (up to the rounding of + coef lambda -
 * coef lambda).  -EINVAL before any launch: K outside [1, 64] or K > V, lambda outside (0, 1] (NaN included), NULL idx or q,
 * logits_ready != 0, a thread in the 2-byte storage mode (vag_set_operator_context: its bf16 d(logits) has no correction), and
 * whatever the namesakes refuse.  Backward must be given the K, lambda, idx, q of its forward. */
int vag_kd_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                           const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                           int64_t V, float p_out, const uint64_t* rng, int logits_ready, float* tmid, float* logits,
                           int64_t ldl, float* lse, float* nll, float* inv_cnt, float* loss_mt, int64_t K, float lambda,
                           const int32_t* idx, const float* q, vag_stream_t stream);
int vag_kd_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                           const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                           int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits, int64_t ldl,
                           const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                           float* d_c_all, float* d_e_all, vag_head_g g, float* scratch, int64_t K, float lambda,
                           const int32_t* idx, const float* q, vag_stream_t stream);
/* R-Drop (Liang et al. 2021, "R-Drop: Regularized Dropout for Neural Networks"): B is even and rows b = 2 p, 2 p + 1 of the batch
 * hold ONE sentence -- the same target, the activations of two passes under two dropout masks (the counter-based dropout is
 * indexed by element, so two copies of a sentence in one batch get different masks).  Head rows are time-major, r = t*B + b; the
 * twin of r is r ^ 1.  With x_r the row's V logits, p_r = softmax(x_r), lp_r = x_r - lse_r, y_r = tgt[b,t], w_r = vocab_weight[y_r]:
 *   kl[r]   = KL(p_r || p_twin) = sum_j p_r[j] * (lp_r[j] - lp_twin[j]),
 *   nll[r]  = w_r * ( lse_r - (1 - eps) * x_r[y_r] - eps / V * sum_j x_r[j] ) + w_r * (alpha / 4) * (kl[r] + kl[twin]),
 *   loss_mt as in vag_head_ce_seq_fwd.
 * Per sentence that is mean(CE_1, CE_2) + (alpha / 2) * sum_t w (KL_12 + KL_21) / 2 / count: half of the paper's CE_1 + CE_2 +
 * alpha * KL_sym, so alpha is the paper's (5 for translation).  Both directions carry gradient, nothing is detached:
 *   d x_r[j] = coef_r * ( p_r[j] - (1 - eps) * [j == y_r] - eps / V )
 *              + (alpha / 4) * (coef_r + coef_twin) * ( p_r[j] * ((lp_r[j] - lp_twin[j]) - kl[r]) + p_r[j] - p_twin[j] ),
 *   coef_r = d_loss * inv_cnt[b] / B * w_r  (unchanged).
 * A PAD row of a pair (w = 0) adds no loss of its own and still receives the gradient of its twin's term.  kl (Tt*B) device floats
 * the caller owns: written by the forward, read by the backward; not clamped (a few ulp below 0 are possible: the gradient is
 * that sum's).  Two identical rows give kl == 0 exactly and the plain gradient.  The forward adds one launch per pass over rows
 * behind the log-sum-exp pass: one workgroup per pair reads both rows once (never the padding columns [V, ldl)) and sums in a fixed
 * order, so kl and nll are reproducible.  The backward's d(logits) pass is a kernel of its own in place of the plain one, with its
 * tiling and traffic: both rows of a pair are read before either is overwritten, g.out_b receives the column sums by fp32 atomics
 * after a reduction over a strip of rows (as the plain pass: its last bits depend on arrival order); pairs with coef_r + coef_twin
 * == 0 and the padding columns are written as zeros.  Every form of the head applies it: the whole sequence and row chunks (whole
 * time steps, so a pair never straddles one) with and without the chunk's backward inside the forward; a backward that recomputes
 * chunks reads kl from the forward's buffer.  -EINVAL before any launch: alpha <= 0 or not finite, NULL kl, B odd, logits_ready != 0,
 * a thread in the 2-byte storage mode (vag_set_operator_context), and whatever the _ls namesakes refuse.  Backward must be given
 * the label_smoothing, alpha and kl of its forward. */
int vag_rdrop_head_ce_seq_fwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                              const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                              int64_t V, float p_out, const uint64_t* rng, int logits_ready, float* tmid, float* logits,
                              int64_t ldl, float* lse, float* nll, float* inv_cnt, float* loss_mt, float label_smoothing,
                              float alpha, float* kl, vag_stream_t stream);
int vag_rdrop_head_ce_seq_bwd(const float* h2_all, const float* c_all, const float* e_all, vag_head_w w,
                              const int64_t* tgt, const float* vocab_weight, int64_t B, int64_t Tt, int64_t E, int64_t H,
                              int64_t V, float p_out, const uint64_t* rng, const float* tmid, float* logits, int64_t ldl,
                              const float* lse, const float* inv_cnt, const float* d_loss, float* d_h2_all,
                              float* d_c_all, float* d_e_all, vag_head_g g, float* scratch, float label_smoothing,
                              float alpha, const float* kl, vag_stream_t stream);
/* Same head producing the log-probabilities themselves (R rows) with a backward from d_logp -- the form the
 * per-step layer API (NMT_Decoder.forward -> logp, layers/NMT_Decoder.py:143) and arbitrary criteria need.
 * tmid (R,E) saved; d_logp (R,ldl) is consumed.  scratch: R*E floats. */
int vag_head_logp_seq_fwd(const float* h2, const float* c, const float* e, vag_head_w w, int64_t R, int64_t E, int64_t H,
                          int64_t V, float p_out, const uint64_t* rng, float* tmid, float* logp, int64_t ldl,
                          vag_stream_t stream);
int vag_head_logp_seq_bwd(const float* h2, const float* c, const float* e, vag_head_w w, int64_t R, int64_t E, int64_t H,
                          int64_t V, float p_out, const uint64_t* rng, const float* tmid, const float* logp,
                          float* d_logp, int64_t ldl, float* d_h2, float* d_c, float* d_e, vag_head_g g, float* scratch,
                          vag_stream_t stream);
/* Single step, inference: logp (N,V) = log_softmax(out(tanh(...))) and argmax (int64[N], may be NULL).
 * scratch: N*E floats. */
int vag_head_logp_step(const float* h2, const float* c, const float* e, vag_head_w w, int64_t N, int64_t E,
                       int64_t H, int64_t V, float* logp, int64_t ldl, int64_t* argmax, float* scratch,
                       vag_stream_t stream);

/* ---- a7/a8: shared-space projections, layers/VSE_Imagine_Enc.py:123-132,138-145; utils/utils.py:6-10 - */
/* out = l2norm(act(x W^T + b)); x (B,K), W (S,K).  y (B,S) = activation output and nrm (B) are saved. */
int vag_img_proj_l2_fwd(const float* x, const float* W, const float* b, int64_t B, int64_t K, int64_t S, int act,
                        float* y, float* nrm, float* out, vag_stream_t stream);
/* d_out is consumed.  d_x may be NULL; g_W, g_b accumulated. */
int vag_img_proj_l2_bwd(const float* x, const float* W, const float* y, const float* nrm, const float* out,
                        float* d_out, int64_t B, int64_t K, int64_t S, int act, float* d_x, float* g_W, float* g_b,
                        vag_stream_t stream);

/* a8 alone: out = x / max(||x||, 1e-12) per row (utils/utils.py:6-10). */
int vag_l2norm_fwd(const float* x, int64_t B, int64_t S, float* nrm, float* out, vag_stream_t stream);
int vag_l2norm_bwd(const float* x, const float* nrm, const float* out, const float* d_out, int64_t B, int64_t S,
                   float* dx, vag_stream_t stream);

/* ---- a6: image-conditioned attention + attended context, VSE_Imagine_Enc.py:29-79,135-137 ------------- */
/* method 0 = 'dot' (score_dot), 1 = 'mlp' (score_mlp; mlp_w (C)).  im_emb (B,S), enc (B,Ts,C), mask (B,Ts).
 * Outputs alpha (B,Ts), ctx (B,C).  ws: vag_imagine_ws_floats() floats kept for backward.
 * 'dot' uses e[b,t] = enc[b,t] . (W_cc^T (W_ec im_emb[b])): identical in exact arithmetic to the reference's
 * bmm(emb2ctx(im), ctx2ctx(enc)^T) and avoids the (B*Ts,C,C) product. */
int64_t vag_imagine_ws_floats(int64_t B, int64_t Ts, int64_t C, int64_t S, int method);
int vag_imagine_attn_ctx_fwd(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                             const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts,
                             int64_t C, int64_t S, float* alpha, float* ctx, float* ws, vag_stream_t stream);
/* d_ctx (B,C) in.  d_enc (B,Ts,C) is written or added to (accumulate_enc); d_im_emb (B,S) written. */
int vag_imagine_attn_ctx_bwd(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                             const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts,
                             int64_t C, int64_t S, const float* alpha, const float* d_ctx, float* ws,
                             float* d_enc, int accumulate_enc, float* d_im_emb, float* g_ctx2ctx,
                             float* g_emb2ctx, float* g_mlp_w, vag_stream_t stream);

/* ---- a9: max-margin ranking losses, losses/PairwiseRankingLoss.py:9-24, ImageRetrievalRankingLoss.py -- */
/* kind 0 = pairwise (both directions), 1 = image retrieval (cost_s only).  im, s (B,S).
 * loss (1).  G (B,B) = d loss / d scores, kept for backward.  scores (B,B) scratch.
 * kind | 2 (B even): rows 2 p and 2 p + 1 are twins -- one sentence under two dropout masks (vag_train_step_rdrop).  A twin is
 * neither a positive nor a negative of its sibling: every entry (i, j) with i != j and i >> 1 == j >> 1 is skipped by both hinges
 * and its G is 0.  kind 0 and 1 are unchanged; anything outside 0 .. 3, or the flag with an odd B, is -EINVAL. */
int vag_rank_loss_fwd(const float* im, const float* s, int64_t B, int64_t S, float margin, int kind, float* scores,
                      float* G, float* loss, vag_stream_t stream);
int vag_rank_loss_bwd(const float* im, const float* s, const float* G, const float* d_loss, int64_t B, int64_t S,
                      float* d_im, float* d_s, vag_stream_t stream);

/* ---- next: batch assembly from a device-resident corpus, preprocessing.py:308-384 ---------- */
/* out[i, 0:w] = in[idx[i], 0:w] for int64 token matrices (in: (N, ld) padded with 0).  Image-feature rows use
 * vag_embed_fwd (a row gather of an fp32 matrix). */
int vag_gather_rows_i64(const int64_t* in, int64_t ld, const int64_t* idx, int64_t rows, int64_t w, int64_t* out,
                        vag_stream_t stream);

/* ---- next: retrieval evaluation, utils/im_retrieval_eval.py:4-57 --------------------------- */
/* The reference loops over N queries with one torch.mm + torch.sort each; here: one (N,S)x(S,N) product into
 * `scores` (N,N scratch) and one rank kernel.  ranks[i] = 0-based position of key i in the descending sort of
 * scores[i,:].  t2i: queries = caption embeddings, keys = image embeddings; i2t: the other way round. */
int vag_retrieval_ranks(const float* queries, const float* keys, int64_t N, int64_t S, float* scores, int32_t* ranks,
                        vag_stream_t stream);

/* ---- a2: decoder initial state, models/...V11.py:118 / NMT_Seq2Seq_Beam_V2.py:85 ---------------------- */
/* x = split*ctx + (1-split)*sum_t enc/sum_t mask (ctx NULL: text-only, x = mean);  h0 = tanh(W x + b).
 * xmix (B,C) is saved. */
int vag_dec_init_fwd(const float* enc, const float* mask, const float* ctx, float split, const float* W,
                     const float* b, int64_t B, int64_t Ts, int64_t C, int64_t H, float* xmix, float* h0,
                     vag_stream_t stream);
/* d_h0 consumed.  d_enc written or added; d_ctx (may be NULL) written.  scratch: B*C floats.
 * d_enc[b,t,:] (+)= coef * dx[b,:] / sum_t mask[b,:] at EVERY t (x sums enc over all Ts positions), dx = (d_h0 (1 - h0^2)) W.
 * d_ctx given: coef = 1 - split and d_ctx = split * dx.  d_ctx NULL is the backward of the text-only form (ctx NULL in the
 * forward): coef = 1 and split is ignored, as it is there. */
int vag_dec_init_bwd(const float* mask, const float* xmix, const float* h0, float split, const float* W,
                     float* d_h0, int64_t B, int64_t Ts, int64_t C, int64_t H, float* d_enc, int accumulate_enc,
                     float* d_ctx, float* g_W, float* g_b, float* scratch, vag_stream_t stream);

/* ---- a10: beam-search step, models/...V11.py:262-313 -------------------------------------------------- */
/* One expansion for B sentences x k beams over V words (step di >= 0; step 0 expands one hypothesis per sentence).
 * logp (B*k_in, ldl) is read through the reference's penalties (repeat-token suppression :279-280, finished
 * hypotheses may only emit EOS at cost 0 :291-294, inf = -1e5).  nll (B,k) running scores in/out.
 * beam (2*max_len,B,k) int64 history: row di receives the chosen words (:306) and row max_len+di the index of the
 * hypothesis each one extends (:303); the reference's per-step permutation of all earlier rows (:309) is replaced
 * by these back-pointers, resolved once in vag_beam_finish.  h_in (B*k_in,H) -> h_out (B*k,H) re-ordered by
 * back-pointer (:273,:313); n_alive (1) int32 = number of new hypotheses whose word is not EOS (host-sync-free
 * early-exit test).  scratch: vag_beam_scratch_bytes. */
int64_t vag_beam_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len);
int vag_beam_step(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int64_t max_len,
                  const float* h_in, float* h_out, int64_t B, int64_t k, int64_t V, int64_t H, int32_t* n_alive,
                  void* scratch, vag_stream_t stream);
/* The same expansion with the step index held in device memory, so that one captured HIP graph serves every step:
 * di_state int32[2] = {di (>= 1 on entry, incremented by the call), 0 (internal arrival counter)}.  A call with
 * di >= max_len does nothing.  tok_out (B*k) int64 (may be NULL) also receives row di, the next step's input words. */
int vag_beam_step_dev(float* logp, int64_t ldl, float* nll, int64_t* beam, int32_t* di_state, int64_t max_len,
                      const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k, int64_t V, int64_t H,
                      int32_t* n_alive, void* scratch, vag_stream_t stream);
/* Final selection (:315-324) after `steps` calls of vag_beam_step (steps < max_len after an early stop): follow the
 * back-pointers, force EOS in the last row, length-normalise, pick the best hypothesis.
 * out (B,max_len) int64 (0 past the written rows), best_score (B). */
/* The decoding step in its hoisted form (round 4): the keys as gru_2 sees them and the head's share of them are projected once per
 * decode call (vag_cgru_decode_keys: keys = [(W_ih2 W_c2h) enc (B,Ts,3H) | enc W2^T (B,Ts,E)], vag_cgru_decode_keys_floats floats;
 * prep from vag_cgru_prepare, w2 = head W2 (E,C)); a step is then four launches and returns cw (N,E) = W2 c instead of the
 * context c, which vag_head_logp_step_h / vag_head_logits_step_h take in its place.  N <= 256 hypotheses, rows_per_src divides N.
 * scratch: vag_cgru_step_scratch_floats. */
int64_t vag_cgru_decode_keys_floats(int64_t B, int64_t Ts, int64_t E, int64_t H);
int vag_cgru_decode_keys(const float* enc, const float* prep, const float* w2, int64_t B, int64_t Ts, int64_t E, int64_t H,
                         float* keys, vag_stream_t stream);
/* tables (optional, NULL: none): [emb W_ih1^T + b_ih1 (V,3H) | emb W3^T (V,E)] from vag_cgru_decode_tables, once per call
 * (w3 = head W3): a step then has no embedding / input-projection launch, `e` is not produced (may be NULL) and the head reads
 * its share of the embedded token from the table line `tok` picks. */
int64_t vag_cgru_decode_tables_floats(int64_t V, int64_t E, int64_t H);
int vag_cgru_decode_tables(vag_dec_w w, const float* w3, int64_t V, int64_t E, int64_t H, float* tables, vag_stream_t stream);
int vag_cgru_attn_decode_step_h(const float* pe, const float* mask, const float* keys, const float* tables, int64_t V,
                                int64_t rows_per_src, const int64_t* tok, const float* h_in, vag_dec_w w, const float* prep,
                                int64_t N, int64_t Ts, int64_t E, int64_t H, float* h_out, float* cw, float* e, float* alpha,
                                float* scratch, vag_stream_t stream);
int vag_head_logp_step_h(const float* h2, const float* cw, const float* e, const float* tables, const int64_t* tok, vag_head_w w,
                         int64_t N, int64_t E, int64_t H, int64_t V, float* logp, int64_t ldl, int64_t* argmax, float* scratch,
                         vag_stream_t stream);
int vag_head_logits_step_h(const float* h2, const float* cw, const float* e, const float* tables, const int64_t* tok, vag_head_w w,
                           int64_t N, int64_t E, int64_t H, int64_t V, float* logits, int64_t ldl, float* parts, float* scratch,
                           vag_stream_t stream);
/* Beam step on RAW logits (round 4): the vocabulary product of vag_head_logits_step leaves, per row, vag_head_logits_parts_count
 * (max, sum exp) pairs -- the pieces of the row's log-sum-exp -- in `parts` (count, N, 2); the expansion kernel normalises the
 * candidates it reads with them, so no pass over the (B k, V) logits is needed between product and selection (V11.py:276,297).
 * count = 0: the shape is not taken (use vag_head_logp_step + vag_beam_step_dev).  scratch of vag_head_logits_step: 2 N E floats. */
int64_t vag_head_logits_parts_count(vag_head_w w, int64_t N, int64_t E, int64_t V);
int vag_head_logits_step(const float* h2, const float* c, const float* e, vag_head_w w, int64_t N, int64_t E, int64_t H,
                         int64_t V, float* logits, int64_t ldl, float* parts, float* scratch, vag_stream_t stream);
int vag_beam_step_logits_dev(float* logits, int64_t ldl, const float* parts, int64_t nparts, float* nll, int64_t* beam,
                             int32_t* di_state, int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B,
                             int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch, vag_stream_t stream);
int vag_beam_finish(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                    int64_t* out, float* best_score, vag_stream_t stream);

/* ---- ensemble decoding: one search over M models (V11.py:207-226 greedy, :233-337 beam, on combined scores) ----------- */
/* M <= VAG_ENS_MAX models sharing the source and target vocabularies; model m contributes its log_softmax rows x_m
 * (logp[m] (B*k_in, ldl[m]), as vag_head_logp_step writes them).  The ensemble scores word w of hypothesis n by the mean of the
 * models' probabilities (the rule of fairseq's ensembles):
 *     s[n,w] = mx + log( (sum_m exp(x_m[n,w] - mx)) / M ),   mx = max_m x_m[n,w]
 * in exactly this form, so that M identical rows give s == x bit for bit.  vag_beam_ens_step is vag_beam_step on s in place of
 * logp -- the penalties of :279-280 / :291-294 (inf = -1e5), the selection of :297-306, the history and the scratch
 * (vag_beam_scratch_bytes) are the same -- and it re-orders the M hidden states h_in[m] (B*k_in, H[m]) -> h_out[m] (B*k, H[m])
 * by the same back-pointers (:273,:313): every hypothesis feeds its word to all M decoders.  vag_beam_finish closes the
 * search unchanged.  logp, ldl, h_in, h_out, H: host arrays of M entries, copied into the kernel arguments at the call (a
 * captured graph keeps its own copy).  -EINVAL for a NULL array or entry, M < 1, M > VAG_ENS_MAX, ldl[m] < V, H[m] < 1, and for
 * everything vag_beam_step rejects.  The raw-logits form (vag_beam_step_logits_dev) has no ensemble counterpart. */
#define VAG_ENS_MAX 8
int vag_ens_max_models(void);
int vag_beam_ens_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, vag_stream_t stream);
/* The same with the step index in device memory (di_state as in vag_beam_step_dev); tok_out (B*k) may be NULL. */
int vag_beam_ens_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, vag_stream_t stream);
/* Greedy step (V11.py:207-226 on s): out[n] (int64, N rows) = arg-max over w of s[n,w], ties to the lowest word index (the rule
 * of vag_head_logp_step's arg-max).  One launch, one block per row. */
int vag_ens_argmax(const float* const* logp, const int64_t* ldl, int64_t M, int64_t N, int64_t V, int64_t* out,
                   vag_stream_t stream);

/* ---- search options, n-best lists, forced-decoding scores (V11.py:233-337, NMT_Seq2Seq_Beam_V2.py:173-277) ---------------- */
/* The five expansions above with the reference's beamsearch options in `flags` (0 = its defaults avoid_double=True,
 * avoid_unk=False: the call is then the form without _opt).  At steps di >= 1, per hypothesis row, in this order: the row's
 * previous word gets -1e5 unless VAG_BEAM_ALLOW_REPEAT (avoid_double=False, :279-280); with VAG_BEAM_AVOID_UNK word UNK = 1 gets
 * -1e5 (avoid_unk=True, :283-284); a finished row (previous word EOS) gets -1e5 everywhere and 0 at EOS (:291-294), overriding
 * both.  Values are replaced, not added (the raw-logits form normalises first).  Step 0 applies no penalty (:261-264): UNK may be
 * picked there even with VAG_BEAM_AVOID_UNK.  V11.py never defines UNK_token (avoid_unk=True raises NameError there); 1 is the
 * text model's value (V2.py:15).  flags is a by-value kernel argument: a captured graph keeps the value it was captured with.
 * -EINVAL for any other bit, and for everything the form without _opt rejects. */
#define VAG_BEAM_ALLOW_REPEAT 1
#define VAG_BEAM_AVOID_UNK 2
int vag_beam_step_opt(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int64_t max_len,
                      const float* h_in, float* h_out, int64_t B, int64_t k, int64_t V, int64_t H, int32_t* n_alive,
                      void* scratch, int32_t flags, vag_stream_t stream);
int vag_beam_step_dev_opt(float* logp, int64_t ldl, float* nll, int64_t* beam, int32_t* di_state, int64_t max_len,
                          const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k, int64_t V, int64_t H,
                          int32_t* n_alive, void* scratch, int32_t flags, vag_stream_t stream);
int vag_beam_step_logits_dev_opt(float* logits, int64_t ldl, const float* parts, int64_t nparts, float* nll, int64_t* beam,
                                 int32_t* di_state, int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B,
                                 int64_t k, int64_t V, int64_t H, int32_t* n_alive, void* scratch, int32_t flags,
                                 vag_stream_t stream);
int vag_beam_ens_step_opt(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                          int64_t V, int32_t* n_alive, void* scratch, int32_t flags, vag_stream_t stream);
int vag_beam_ens_step_dev_opt(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam,
                              int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                              int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags,
                              vag_stream_t stream);
/* N-best finish (:315-324 without the final top-1): after `steps` expansions, rank the k final hypotheses by vag_beam_finish's
 * length-normalised score nll / max(1, #words > 3 over the written rows) under its order (score desc, slot asc) and resolve
 * the n best: out (B, n, max_len) int64, row (b, r) = the r-th best hypothesis with EOS forced in its last position and 0 past
 * the written rows; scores (B, n) float in descending order.  n = 1 writes vag_beam_finish's row and score bit for bit.
 * No de-duplication: a hypothesis that took a -1e5 step can cut at EOS to the same token list as a finished one; such entries
 * score below -1e4.  1 <= n <= k <= 64, else -EINVAL. */
int vag_beam_finish_nbest(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n,
                          int64_t* out, float* scores, vag_stream_t stream);
/* vag_beam_finish_nbest (out and scores bit for bit) that also writes slots (B, n) int64: the final slot, in [0, k), of each
 * ranked hypothesis -- after a diverse search (below) slot / (k / groups) is the group it ended in.  -EINVAL as
 * vag_beam_finish_nbest, and for slots == NULL. */
int vag_beam_finish_nbest_slots(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                int64_t n, int64_t* out, float* scores, int64_t* slots, vag_stream_t stream);

/* ---- diverse beam search: grouped beams with a Hamming diversity penalty (Vijayakumar et al. 2016) -------------------------- */
/* vag_beam_ens_step_opt with the k slots of a sentence split into `groups` groups of g = k / groups consecutive slots (group i
 * owns slots [i g, (i+1) g)) that are expanded one after another inside the step; M = 1 is the single model.
 *   rows:      at steps di >= 1 row j (slot j of the previous step) belongs to group j / g; at step 0 the sentence's one row
 *              (SOS) is expanded by every group.
 *   model:     c(j,w) = base_j + lp'(j,w): the running score (0 at step 0) plus the (ensemble) log-probability after exactly
 *              vag_beam_ens_step_opt's penalties under `flags` -- bitwise the value the plain search selects by.
 *   selection: for groups i = 0 .. groups-1 in this order, cnt[w] = the number of slots chosen by groups < i at this step whose
 *              word is w and whose parent row was not finished (at step 0 every chosen slot counts).  The key of a candidate is
 *              s(j,w) = fmaf(-strength, (float)cnt[w], c(j,w)), one rounding; s = c for a finished row (previous word EOS): a
 *              finished hypothesis neither pays nor causes a penalty.  Group i takes the g best of its rows' candidates under
 *              (s desc, flat index j V + w asc) into its slots, best first.
 *   stored:    the word in beam[di], the parent's absolute slot j in beam[max_len + di], and c(j,w) -- the model's score WITHOUT
 *              the diversity term -- in nll, so that a finished search's scores are what vag_forced_score gives for the returned
 *              words.  n_alive, tok_out, the M hidden states and di_state as in vag_beam_ens_step(_dev)_opt; vag_beam_finish* close
 *              the search unchanged.
 * groups = 1 is the plain search (words, parents and scores bit for bit); strength = 0 gives `groups` identical copies of a
 * width-g search.  Two launches: a row-aligned stage 1 (the k best of every 2048-word slice of every row by c: at most k - g
 * words are penalised for a group, so a row's k best hold everything its group can select) and one workgroup per sentence that
 * runs the groups.  scratch: vag_beam_div_scratch_bytes (larger than vag_beam_scratch_bytes).  groups, strength and flags are
 * by-value kernel arguments: a captured graph keeps the values it was captured with.  There is no raw-logits form.
 * -EINVAL for groups < 1, k % groups != 0, V < k, strength negative or not finite, B k > 65535, and for everything
 * vag_beam_ens_step_opt rejects. */
int64_t vag_beam_div_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len);
int vag_beam_div_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int64_t groups, float strength,
                      vag_stream_t stream);
int vag_beam_div_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int64_t groups,
                          float strength, vag_stream_t stream);

/* ---- constrained beam search: target prefixes, banned phrases, no-repeat n-grams --------------------------------------------- */
/* Rules words out for the expansion that follows: rewrites, in place, the M members' log-probability rows logp[m] (N, ldl[m]) of
 * step di as vag_head_logp_step wrote them (N = B at step 0, B k afterwards), one launch for all members and rows.  Enqueue it
 * after the members' steps and before vag_beam_ens_step(_opt) / vag_beam_div_step of the same step; M = 1 is the single model.
 *   history:  row (b, j) at step di is slot j of sentence b after step di-1; its words h[0 .. di-1] are what vag_beam_finish
 *             would resolve: s_{di-1} = j, h[t] = beam[t][b][s_t], s_{t-1} = beam[max_len + t][b][s_t].  Empty at step 0.
 *   finished: a row with di >= 1 and h[di-1] == EOS is left untouched (the expansion's own rule, :291-294, overrides it anyway).
 *   prefix:   prefix (B, Lp) int64, pad 0.  A row that is not finished, with di < Lp and f = prefix[b][di] in [1, V), is FORCED:
 *             every word w != f in [0, V) of every member's row becomes -1e5; f keeps each member's own value, so a finished
 *             search's score is still the model's own (what vag_forced_score gives).  Nothing else applies to a forced row: it
 *             ignores the bans.
 *   phrases:  otherwise every phrase p < P: phrases (P, VAG_CONSTRAIN_MAX_LEN) int64, L = its number of leading non-zero
 *             words (L = 0: the phrase is ignored); phrase_sent[p] = -1 (every sentence) or the one sentence index it applies to.
 *             L = 1 bans the word; L - 1 <= di and h[di-L+1 .. di-1] equal to the phrase's first L-1 words bans its last word.
 *   n-grams:  ngram = n >= 1: for every t in [0, di-n], word h[t+n-1] is banned whenever h[t .. t+n-2] equals
 *             h[di-n+1 .. di-1] (no n-gram occurs twice in a hypothesis); n = 1 bans every word of the history.  0: off.
 *   a ban:    -1e5 at that word in EVERY member's row, replaced, not added (the expansions' own "inf").  With all M values -1e5
 *             the ensemble score mx + log(sum / M) is -1e5 exactly (sum == M), so an ensemble sees a ban as the single model
 *             does.  A banned word outside [0, V) writes nothing; columns [V, ldl) are never written.
 * Step 0 is constrained as well (its first word may be forced, unigram bans apply) -- unlike `flags`, which skip step 0.  The
 * expansion's penalties under `flags` come after the mask: a forced word that repeats its predecessor (without
 * VAG_BEAM_ALLOW_REPEAT) or is UNK (with VAG_BEAM_AVOID_UNK) would be ruled out by them; the callers reject such prefixes.
 * logp, ldl: host arrays of M entries, copied into the kernel arguments at the call (a captured graph keeps its own copy);
 * Lp, P and ngram are by-value arguments too, prefix / phrases / phrase_sent are read at every launch.
 * The _dev form reads the step index from di_state[0], the word the expansions' _dev forms advance, and does not modify it:
 * enqueue it BEFORE that step's expansion; it does nothing once the index has reached max_len.
 * -EINVAL for a NULL array or entry, M outside [1, VAG_ENS_MAX], ldl[m] < V, NULL beam, empty sizes, k > 64, max_len > 1024
 * (the history is staged in LDS), di outside [0, max_len) (by-value form), NULL di_state (_dev form), Lp < 0, Lp > 0 with NULL
 * prefix, P outside [0, VAG_CONSTRAIN_MAX_PHRASES], P > 0 with either phrase array NULL, ngram outside
 * [0, VAG_CONSTRAIN_MAX_LEN].  Lp = 0, P = 0 and ngram = 0 is valid and launches nothing. */
#define VAG_CONSTRAIN_MAX_LEN     8     /* words in a banned phrase; largest no-repeat n */
#define VAG_CONSTRAIN_MAX_PHRASES 256
int vag_beam_constrain(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di, int64_t max_len,
                       int64_t B, int64_t k, int64_t V, const int64_t* prefix, int64_t Lp, const int64_t* phrases,
                       const int32_t* phrase_sent, int64_t P, int64_t ngram, vag_stream_t stream);
int vag_beam_constrain_dev(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, const int32_t* di_state,
                           int64_t max_len, int64_t B, int64_t k, int64_t V, const int64_t* prefix, int64_t Lp,
                           const int64_t* phrases, const int32_t* phrase_sent, int64_t P, int64_t ngram, vag_stream_t stream);

/* ---- kNN-MT: a nearest-neighbour datastore mixed into the rows of a step (Khandelwal et al. 2021) --------------------------- */
/* The datastore holds N entries: keys (N, D) bf16 (the decoder's second state h2 of the step that predicts the word, rounded to
 * nearest even; D = H), norm (N) fp32 = the squared length of the STORED key, value (N) int32 = the word, and the provenance
 * sentence / position (N) int32.  The stored key is the entry.
 *   score:   for a query row q (fp32) and entry i:  s_i = 2 q.k_i - norm[i]  (ranking by s descending is ranking by squared L2
 *            distance ascending; s_max - s_i = d_i - d_min).  Total order: score descending, then index ascending.  A score depends
 *            on the query row and the stored key alone and is formed by one sequence of operations everywhere, so entries with
 *            identical stored keys score bit-identically wherever they lie, and the index decides between them.
 *   weights: over the K' = min(K, N) retrieved entries w_j = exp((s_j - s_max) / T), p_knn(word) = sum_{j: value_j = word} w_j / sum_j w_j.
 *   mix:     a retrieved word gets log((1 - lam) exp(x) + lam p_knn) in the max-shifted form, every other word x + log1p(-lam),
 *            x the row's log-probability (the row's value minus the optional log-sum-exp).
 *
 * vag_knn_store_rows appends a forced batch: h2 (Tt, B, H) time-major as vag_cgru_attn_decode_seq_fwd leaves it, tgt (B, Tt) int64.
 * It takes rows t = 0 .. end of every sentence b, end as vag_forced_score's span (the first EOS, or the last non-pad word if there
 * is none; an all-pad sentence gives nothing), and writes them densely in the order (b, t) from entry 0 of the five output arrays
 * on: the rounded key, its norm (fp32 sum of the rounded values' squares in a fixed order), value = tgt[b][t], sentence =
 * sent_base + b, position = t.  count[0] receives the number of entries the batch has; entries from `cap` on are not written (the
 * caller compares count with cap).  One launch, nothing atomic.  -EINVAL: a NULL pointer, H outside [8, 1024] or not a multiple
 * of 8, B outside [1, 65535], Tt < 1, B Tt >= 2^31, sent_base < 0.
 *
 * vag_knn_search: queries q (R, D) fp32 with leading dimension ldq >= D against the N entries; out_score / out_index (R, K)
 * receive every row's K' best, ranked; places K' .. K-1 hold (-inf, -1).  Stage 1: one workgroup per (slice of VAG_KNN_SLICE keys,
 * tile of vag_knn_row_tile(D) rows) streams its keys once, forms the scores on the matrix units from the queries' three bf16
 * planes (q = q1 + q2 + q3 up to 2^-27 |q|; fp32 accumulation over 3 ceil(D / 16) products of depth 16) and keeps every row's K
 * best of the slice; stage 2 merges the slices' lists per row.  No (R, N) matrix, no atomics.  scratch: vag_knn_scratch_bytes(R,
 * N, K) bytes, 16-byte aligned; keys 16-byte aligned.  The call allocates nothing and does not wait: it can be captured.  Inputs
 * are taken as finite.  -EINVAL: a NULL pointer, D outside [8, 1024] or not a multiple of 8, ldq < D, N outside [1, 2^31), K
 * outside [1, VAG_KNN_MAX_K], R < 1, R ceil(N / VAG_KNN_SLICE) >= 2^26, misaligned keys or scratch.
 * vag_knn_scratch_bytes: 0 for sizes vag_knn_search refuses.  vag_knn_row_tile: 32 up to D = 640, 16 beyond, 0 for a D it refuses.
 *
 * vag_knn_mix rewrites, in place, rows [0, R) of the M members' matrices logp[m] (R, ldl[m]) as vag_beam_constrain takes them.
 * Member m's rows are mixed with member m's neighbours nb_score[m] / nb_index[m] (R, K) as vag_knn_search wrote them and its
 * store's values[m] (n_values[m] words); an index outside [0, n_values[m]) or a word outside [0, V) is no neighbour.  lse: NULL,
 * or M entries, each NULL or the rows' log-sum-exp (R) to subtract (raw logits; NULL for log-probabilities).  inv_T = 1 / T,
 * log_lam = log(lam) and log1m_lam = log1p(-lam) are formed by the caller in double and rounded once; lam = 0 is the caller's
 * case (nothing to launch).  Neighbours carrying one word are summed before the mix; every sum runs in index order.  Columns
 * [V, ldl) are never read or written.  One launch, one workgroup per row.  -EINVAL: a NULL array or entry, M outside
 * [1, VAG_ENS_MAX], ldl[m] < V, K outside [1, VAG_KNN_MAX_K], inv_T <= 0 or not finite, log_lam >= 0, log1m_lam > 0, either -inf. */
#define VAG_KNN_SLICE 2048      /* keys of one stage-1 workgroup */
#define VAG_KNN_MAX_K 32
int64_t vag_knn_slice(void);
int64_t vag_knn_row_tile(int64_t D);
int64_t vag_knn_scratch_bytes(int64_t R, int64_t N, int64_t K);
int vag_knn_store_rows(const float* h2, const int64_t* tgt, int64_t B, int64_t Tt, int64_t H, int64_t sent_base, int64_t cap,
                       void* keys, float* norm, int32_t* value, int32_t* sentence, int32_t* position, int32_t* count,
                       vag_stream_t stream);
int vag_knn_search(const float* q, int64_t ldq, int64_t R, int64_t D, const void* keys, const float* norm, int64_t N, int64_t K,
                   float* out_score, int32_t* out_index, void* scratch, vag_stream_t stream);
int vag_knn_mix(float* const* logp, const int64_t* ldl, int64_t M, int64_t R, int64_t V, const float* const* nb_score,
                const int32_t* const* nb_index, int64_t K, const int32_t* const* values, const int64_t* n_values,
                const float* const* lse, float inv_T, float log_lam, float log1m_lam, vag_stream_t stream);

/* ---- shallow fusion: a back-off n-gram language model added to the rows of a step (Gulcehre et al. 2015) --------------------- */
/* score(w | hyp) = logp_model(w | hyp) + beta ln p_LM(w | the last order-1 words of hyp), not renormalised.
 * The model (vag_lm) is a back-off model of order 2 .. VAG_LM_MAX_ORDER over the word ids [0, V) in ARPA's semantics, natural logs:
 * lm(w | c_L..c_1) = logp(c_L..c_1 w) where that n-gram is stored, otherwise bo(c_L..c_1) -- 0 for a context that is not stored --
 * plus lm(w | c_{L-1}..c_1); the unigrams cover every id.  It is a forward trie in flat device arrays, level n = the n-grams,
 * index l = n - 1:
 *   level 1 is indexed by the word: logp[0][V], bo[0][V], child[0][V+1]; count[0] = V;
 *   level n >= 2: word[l][count[l]] int32, ascending and distinct inside every parent's range, logp[l][count[l]], and below the
 *   top order bo[l][count[l]] and child[l][count[l]+1]; the successors of node i of level n are the entries
 *   [child[l][i], child[l][i+1]) of level n+1.  word[0], and bo / child of the top order, are not read.  Counts are below 2^31.
 * The struct is read on the host while a call enqueues; its pointers and counts travel by value into the launch (a captured graph
 * keeps its own copy, so the arrays must outlive it).  The kernels take a well-formed trie on trust -- child ranges monotone and
 * inside the next level, words in [0, V), finite values: the caller validates (vagnmt_hip.lm.NgramLM does); they clamp every
 * range to its array all the same.
 *
 * vag_lm_fuse_rows: rows[m][r ld[m] + w] += beta lm(w | ctx_r) for every member m < M, row r < R and word w < V.  ctx (R, order-1)
 * int32, the most recent word last; -1, or an id outside [0, V), means "no word" and ends the context there, so a context may
 * be shorter than order-1 or empty.  One 256-thread workgroup per row: the context's suffixes are resolved once, every element is
 * read once and written once -- the successors of the longest stored context first, each claimed in an LDS bitmap of V bits, then
 * the shorter ones' unclaimed successors, then one dense pass of the unigrams -- and the result does not depend on thread
 * timing: the same inputs give the same bits.  The term is the same for every member, which commutes with the ensemble's
 * log-mean.  Columns [V, ld) are never read or written.  A value is x + beta (logp + Bsum), Bsum the sum, longest first, of the
 * back-offs of the stored contexts longer than the matching one; every operation is rounded once (no contraction).
 *
 * vag_lm_fuse_beam(_dev): the same on the members' rows of step di of a beam search, as vag_beam_constrain takes them, with the
 * context read from the search buffer: row (b, j) walks at most order-1 hops back from step di-1 (word and back-pointer of a hop
 * loaded together, the slot clamped to [0, k)); SOS follows the word of step 0 and nothing follows SOS.  At step 0 there are B
 * rows and the context is (SOS).  A row whose previous word is EOS is left untouched (the expansion's own rule covers it).
 * Enqueue it after the members' steps and before vag_beam_constrain of the same step, so that a ban still wins.  The _dev form
 * reads the step index from di_state[0] and does not modify it; it does nothing once the index has reached max_len.
 *
 * vag_lm_query: the sparse form, one lane per pair: logp_out[r] = lm(word[r] | ctx_r), order_out[r] = the order n of the n-gram
 * that matched (1 = a unigram); a word outside [0, V) gives (-inf, 0).  The same operations in the same order as the dense form.
 *
 * beta = 0 is valid and launches nothing.  -EINVAL before any launch: a NULL array, entry or model, order outside
 * [2, VAG_LM_MAX_ORDER], model V outside [1, VAG_LM_MAX_V] or count[0] != V, V != the model's, a count outside [0, 2^31), a NULL
 * array of a level the order uses, M outside [1, VAG_ENS_MAX], ld[m] < V, R < 1, empty sizes, k > 64, max_len > 1024, di outside
 * [0, max_len) (by-value form), NULL di_state (_dev form), beta not finite. */
#define VAG_LM_MAX_ORDER 5
#define VAG_LM_MAX_V 131072     /* the claimed-word bitmap: V bits of LDS */
typedef struct {
    int32_t order;                              /* 2 .. VAG_LM_MAX_ORDER */
    int32_t V;
    int64_t count[VAG_LM_MAX_ORDER];            /* entries of level l+1; count[0] = V */
    const int32_t* word[VAG_LM_MAX_ORDER];
    const float* logp[VAG_LM_MAX_ORDER];
    const float* bo[VAG_LM_MAX_ORDER];
    const int32_t* child[VAG_LM_MAX_ORDER];
} vag_lm;
int vag_lm_fuse_rows(float* const* rows, const int64_t* ld, int64_t M, int64_t R, int64_t V, const vag_lm* lm, const int32_t* ctx,
                     float beta, vag_stream_t stream);
int vag_lm_fuse_beam(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di, int64_t max_len,
                     int64_t B, int64_t k, int64_t V, const vag_lm* lm, float beta, vag_stream_t stream);
int vag_lm_fuse_beam_dev(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, const int32_t* di_state,
                         int64_t max_len, int64_t B, int64_t k, int64_t V, const vag_lm* lm, float beta, vag_stream_t stream);
int vag_lm_query(const vag_lm* lm, const int32_t* ctx, const int32_t* word, int64_t R, float* logp_out, int32_t* order_out,
                 vag_stream_t stream);

/* ---- required phrases in beam search: dynamic beam allocation (Post & Vilar 2018; Hu et al. 2019) ---------------------------- */
/* vag_beam_ens_step_opt for a search whose hypotheses must CONTAIN given phrases; M = 1 is the single model.  A hypothesis that has
 * not produced a phrase yet is unfinished, not wrong, so nothing is masked: the step keeps slots for hypotheses that are further
 * along with their phrases even when they score worse.  The arguments are vag_beam_div_step(_dev)'s without groups / strength, plus
 *   required:  (B, VAG_REQUIRE_MAX_PHRASES, VAG_CONSTRAIN_MAX_LEN) int64, pad 0, read at every launch.  Phrase c of sentence b has
 *              L_c = its number of leading non-zero words; L_c = 0: the entry is unused.  A word outside [1, V) is a word no
 *              candidate is: such a phrase is never met.
 *   state:     (B, k, 4) int32, in/out, carried from step to step: per slot {met, prog_lo, prog_hi, n}.  met: bit c is set once
 *              phrase c occurred contiguously in the hypothesis's words.  prog_lo / prog_hi: 4 bits per phrase (phrases 0-7 / 8-15),
 *              the progress p_c in [0, L_c - 1] of every phrase that is not met, 0 for met and unused ones.  n = sum_c (met_c ? L_c :
 *              p_c), the hypothesis's bank.  Step 0 ignores the contents: its one parent row has the all-zero state.
 * Per sentence and step di, rows j < k_in (k_in = 1 at step 0):
 *   scores:      c(j,w) = base_j + lp'(j,w) exactly as the diverse block defines it -- the running score (0 at step 0) plus the
 *                (ensemble) log-probability after the expansion's penalties under `flags`, one float add -- with one more
 *                penalty, which applies at step 0 too: a row that is not finished and has a phrase with L_c > 0 not met gets
 *                lp'(j, EOS) = -1e5 (a hypothesis may not end with phrases open).  The finished-row rule (:291-294) overrides it.
 *   transition:  phrase c, not met, progress p, on word w: p' = the largest q <= min(L_c, p + 1) such that the last q words of
 *                phrase[0..p-1] + [w] equal phrase[0..q-1] (exact substring matching: `a a b` is found in `a a a b`); p' = L_c sets
 *                the met bit and clears the progress.  Phrases are tracked independently.  The child of a finished row keeps its
 *                parent's state unchanged, and so does every child of the last step, di = max_len - 1: vag_beam_finish* force EOS
 *                into that row, so its word is part of no hypothesis and the state keeps describing the words that are.
 *   candidates:  the union, by flat index j V + w, each once, of (a) the k best of all k_in V candidates under (c desc, flat asc),
 *                the plain search's selection; (b) for every row that is not finished and every phrase c of it that is not met, the
 *                candidate (j, phrase_c[p_c]), the word that advances it; (c) every row's own best word under (c desc, w asc).  A
 *                candidate's value is c(j,w), bitwise the same whichever of (a)-(c) produced it; its bank is the n of its child state.
 *   allotment:   a candidate is live iff c(j,w) > -5e4f, else dead (it took a -1e5 somewhere).  rho = a live candidate's rank among
 *                the live candidates of its bank under (c desc, flat asc), from 0.  The live candidates fill slots 0, 1, ... in the
 *                order (rho asc, bank desc): the best unseen of each bank, highest bank first, repeated.  If fewer than k are live
 *                the remaining slots take dead candidates under (c desc, flat asc); (a) alone guarantees k candidates.
 *   stored:      the word, the parent slot, c(j,w) -- the model's own score, so a finished search scores what vag_forced_score gives
 *                for the returned words -- and the child state.  n_alive, tok_out, the M hidden states and di_state as in
 *                vag_beam_ens_step(_dev)_opt.
 * With no phrases (every L_c = 0) the step writes vag_beam_ens_step_opt's words, parents and scores bit for bit.  vag_beam_finish*
 * close the search unchanged; vag_beam_finish_nbest_slots gives the slot whose `met` belongs to each ranked hypothesis.  The mask of
 * the negative constraints (vag_beam_constrain) may precede the step as it precedes any expansion.  Two launches: a row-aligned
 * stage 1 and one workgroup per sentence.  scratch: vag_beam_req_scratch_bytes.  flags is a by-value kernel argument.
 * -EINVAL for NULL required or state, and for everything vag_beam_div_step rejects with groups = 1. */
#define VAG_REQUIRE_MAX_PHRASES 16      /* phrases per sentence; each has 1 .. VAG_CONSTRAIN_MAX_LEN words */
int64_t vag_beam_req_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len);
int vag_beam_req_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const int64_t* required, int32_t* state,
                      vag_stream_t stream);
int vag_beam_req_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const int64_t* required,
                          int32_t* state, vag_stream_t stream);

/* ---- stochastic beam search: sampling translations without replacement (Kool, van Hoof, Welling 2019) ------------------------ */
/* vag_beam_ens_step_opt over Gumbel-perturbed scores: the k hypotheses of a finished search are an exact sample WITHOUT replacement
 * from the (ensemble's) sequence distribution, in sampling order, and their perturbed scores give the importance weights of
 * weighted estimates.  M = 1 is the single model.  The arguments are vag_beam_div_step(_dev)'s without groups / strength, plus
 *   rng:  the {seed, call counter} words of vag_sample_step (uint64[2] in device memory), read at every launch.
 *   gum:  (B, k) float, in/out: the perturbed score G of every slot, carried from step to step as nll is.  Step 0 ignores its
 *         contents: the root has G = 0.
 * Per sentence b and step di, rows j < k_in (k_in = 1 at step 0); all arithmetic fp32, one rounding per named operation, no fma:
 *   score:      c(j,w) = base_j + lp'(j,w), bitwise the diverse block's value: the running score (0 at step 0) plus the (ensemble)
 *               log-probability after the expansion's penalties under `flags`.
 *   perturbed:  g(j,w) = fl(c(j,w) + noise(j,w)), noise = the sampler's Gumbel noise of word w under the key of (rng, di, input
 *               row n = b k_in + j): exactly what vag_sample_noise(rng, di, B k_in, V, out) writes at out[n, w].
 *   maximum:    Z_j = max_w g(j,w).
 *   condition:  on the parent's G (the numerically stable truncated-Gumbel form): d = fl(g - Z_j); l = -inf if d == 0,
 *               logf(-expm1f(d)) if d > -ln 2, else log1pf(-expf(d)); v = fl(fl(G_j - g) + l);
 *               G~(j,w) = G_j - fmaxf(v, 0) - log1pf(expf(-fabsf(v))), the two subtractions in that order.  The row's arg-max
 *               child gets G~ = G_j exactly, and G~ is non-decreasing in g within a row.
 *   finished:   a row whose previous word is EOS contributes the single candidate (j, EOS) with c = base_j and G~ = G_j exactly,
 *               no noise read; none of its other words is a candidate.
 *   selection:  the k best of all candidates under (G~ desc, flat index j V + w asc), best first into slots 0 .. k-1.
 *   stored:     the word in beam[di], the parent slot in beam[max_len + di], c(j,w) -- the model's own score, so a finished search
 *               scores what vag_forced_score gives for the returned words -- in nll, and G~ in gum.  n_alive, tok_out, the M hidden
 *               states and di_state as in vag_beam_ens_step(_dev)_opt; vag_beam_finish* close the search unchanged
 *               (vag_beam_finish_nbest_slots gives the slot whose gum belongs to each ranked hypothesis).
 * Two launches: a row-aligned stage 1 that reads every log-probability row once and keeps, per row and 2048-word slice, the k best
 * by (g desc, flat asc) with both g and c (G~ is monotone in g inside a row, so these hold everything the sentence can select, and
 * their best is Z_j), and one workgroup per sentence that forms Z_j, transforms and selects.  No floating-point atomics: a decode
 * is a pure function of (inputs, rng).  The mask of vag_beam_constrain may precede the step as it precedes any expansion; a -1e5
 * word is an ordinary candidate that loses.  scratch: vag_beam_sbs_scratch_bytes.  flags is a by-value kernel argument.
 * -EINVAL for NULL rng or gum, and for everything vag_beam_div_step rejects with groups = 1. */
int64_t vag_beam_sbs_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len);
int vag_beam_sbs_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const uint64_t* rng, float* gum,
                      vag_stream_t stream);
int vag_beam_sbs_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, const uint64_t* rng,
                          float* gum, vag_stream_t stream);

/* ---- penalised beam search: GNMT length and coverage penalties, at the finish or stepwise (Wu et al. 2016, section 7) --------- */
/* vag_beam_ens_step_opt for a search that ranks hypotheses by a length- and coverage-penalised score -- at the finish only, or
 * (stepwise) already while they compete for slots, where the plain search compares a short finished hypothesis and a long
 * unfinished one on raw sums.  M = 1 is the single model.  All arithmetic fp32, one rounding per named operation, no contraction.
 * Per hypothesis (slot) the search carries
 *   len:  int32, the number of its words with id > 3 (UNK, EOS and pad never count, nor does the word of row max_len-1, which the
 *         finish forces to EOS): the count vag_beam_finish makes by walking the history.
 *   cov:  Tp floats, the sum of the attention rows (the mean over members, as vag_beam_attn_record forms it) that produced its
 *         words, up to and including the row that produced its first EOS: the column sum of vag_beam_finish_align's attention.
 *   cp:   beta * sum_i logf(fminf(fmaxf(cov_i, 1e-10f), 1.f)) over the source positions i whose mask is non-zero.  Summation
 *         order: the columns are dealt to 64 lanes in quads, lane l owning the columns i with (i / 4) % 64 == l; every lane adds its
 *         terms in increasing i from +0, the 64 partial sums are combined by the butterfly p_l += p_(l xor o), o = 32, 16, .. 1, and
 *         cp = fl(beta * sum).  A finished hypothesis's len, cov and cp are frozen.
 * and the host supplies two tables of max_len + 1 floats, built in fp64 and rounded once: the divisor lp[L] and the additive reward
 * bonus[L], indexed with L = max(len, 1) -- the device evaluates no powf, and every score is reproducible bit for bit on the host.
 * The penalised score of a hypothesis with running score c is  s = fl(fl(fl(c + bonus[L]) / lp[L]) + cp).  With lp[L] = L,
 * bonus = 0 and cp = +0, s is vag_beam_finish_nbest's score bit for bit.
 *
 * vag_beam_cover: one launch per step, enqueued BEFORE the expansion (the _dev form reads di_state[0] as vag_beam_attn_record_dev
 * does).  alpha[m] (N, Tp): the members' attention rows of this step, N = B at step 0 and B k afterwards; mask (B, Tp); cov
 * (B, k, Tp) the carried sums by slot (not read at step 0); beam the history (a row whose previous word is EOS has ended).
 * cov_row (N, Tp) = cov + a for a live row, cov for a finished one, a at step 0; cp_row (N) = cp of cov_row.  Any Tp >= 1: 16-byte
 * accesses when Tp % 4 == 0 and every buffer is 16-byte aligned, scalar ones otherwise (same values, same order).  beta == 0 does
 * no coverage work: it writes cp_row = +0 and touches nothing else (alpha, mask, cov, cov_row may be NULL).
 * -EINVAL for beta negative or not finite, NULL buffers, M out of range, k > 64, Tp < 1, B k > 65535, di outside [0, max_len).
 *
 * vag_beam_pen_step: vag_beam_sbs_step's arguments without rng / gum, plus lens (B, k) int32 in/out (step 0 ignores its
 * contents), cp_row (N) in, cpen (B, k) out, cov_row (N, Tp) in and cov (B, k, Tp) out (both NULL without a coverage term), Tp,
 * the tables lp and bonus, and stepwise (0 / 1, by value).  Per sentence, rows j < k_in (k_in = 1 at step 0):
 *   candidates: (j, w) with c(j,w) bitwise the diverse block's value (same loads, ens_score and penalties under `flags`); a
 *               finished row contributes (j, EOS) alone, with c = base_j.
 *   length:     len' = len_j + (w > 3 and row j is live and di < max_len - 1).
 *   key:        s(c, len', cp_row[j]) if stepwise, else c.
 *   selection:  the k best under (key desc, flat index j V + w asc) into slots 0 .. k-1, best first.
 *   stored:     word and parent in the history, c in nll, len' in lens, cp_row[parent] in cpen, cov_row[parent] in cov[slot];
 *               n_alive, tok_out, the M hidden states and di_state as in vag_beam_ens_step(_dev)_opt.
 * stepwise = 0 selects what vag_beam_ens_step_opt selects, bit for bit (as long as k candidates above the -1e5 range exist).
 * Two launches: a row-aligned stage 1 and one workgroup per sentence; no floating-point atomics.  Inside a row the key is monotone
 * in c only within a class (words 0..3 keep len_j, the others get len_j + 1), so stage 1 does NOT rank by c: every block ranks its
 * 2048-word slice of one row by the final (key, flat index) order itself, both classes together, and keeps c beside the key.  The
 * k best of the sentence under a total order are among the k best of every subset they fall into, so this is complete with no
 * assumption about the key.  scratch: vag_beam_pen_scratch_bytes (-EINVAL for sizes the step rejects).  flags and stepwise are
 * by-value kernel arguments: a captured graph keeps the values it was captured with; the tables are read at every launch.
 * The mask of vag_beam_constrain may precede the step as it precedes any expansion.
 * -EINVAL for NULL lens, cp_row, cpen, lp or bonus, cov given without cov_row or the reverse, Tp < 1, stepwise outside {0, 1}, and
 * for everything vag_beam_div_step rejects with groups = 1.
 *
 * vag_beam_finish_pen: vag_beam_finish_nbest_slots that ranks by s formed from nll, lens and cpen under (s desc, slot asc); besides
 * out, scores (= s) and slots it returns, per ranked hypothesis, logp (= nll), length (= len) and cp, all (B, n).  One launch.
 * -EINVAL as vag_beam_finish_nbest_slots, and for any NULL buffer. */
int64_t vag_beam_pen_scratch_bytes(int64_t B, int64_t k, int64_t V, int64_t max_len);
int vag_beam_cover(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam, int64_t di,
                   int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row, float* cp_row, vag_stream_t stream);
int vag_beam_cover_dev(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam,
                       const int32_t* di_state, int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row,
                       float* cp_row, vag_stream_t stream);
int vag_beam_pen_step(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t B, int64_t k,
                      int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int32_t* lens, const float* cp_row, float* cpen,
                      const float* cov_row, float* cov, int64_t Tp, const float* lp, const float* bonus, int32_t stepwise,
                      vag_stream_t stream);
int vag_beam_pen_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int32_t* di_state,
                          int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out,
                          int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int32_t flags, int32_t* lens,
                          const float* cp_row, float* cpen, const float* cov_row, float* cov, int64_t Tp, const float* lp,
                          const float* bonus, int32_t stepwise, vag_stream_t stream);
int vag_beam_finish_pen(const float* nll, const int64_t* beam, const int32_t* lens, const float* cpen, const float* lp,
                        const float* bonus, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n, int64_t* out,
                        float* scores, int64_t* slots, float* logp, int32_t* length, float* cp, vag_stream_t stream);

/* Forced decoding: the log-probability M <= VAG_ENS_MAX models assign to given targets tgt (B, Tt) int64 (pad 0).  Model m
 * contributes its teacher-forced raw logits (Tt*B, ldl[m]) and their rows' log-sum-exp lse[m] (Tt*B), time-major (row t*B+b:
 * vag_head_ce_seq_fwd's logits and lse); word y_t scores x_m = logit - lse, combined as in vag_beam_ens_step (M = 1: x itself;
 * M identical members give the single model bit for bit).  Per sentence, over the span up to and including the first EOS (to
 * the last non-pad position if there is none): token_logp (B, Tt) = the score at non-pad span positions, 0 elsewhere (NaN for a
 * word outside [0, V)); logp (B) = their sum in position order; score (B) = logp / max(1, #words > 3 in the span), the
 * normalisation of vag_beam_finish.  logits, ldl, lse: host arrays of M entries.  One launch, one wave per sentence. */
int vag_forced_score(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, const int64_t* tgt,
                     int64_t B, int64_t Tt, int64_t V, float* token_logp, float* logp, float* score, vag_stream_t stream);

/* Word-level confidence from the same inputs (M <= VAG_ENS_MAX models' teacher-forced raw logits (Tt*B, ldl[m]) and row log-sum-exp
 * lse[m] (Tt*B), time-major rows t*B+b; tgt (B, Tt) int64, pad 0): what the model thought of every word of a given translation.
 * Word j of a row scores s_j = combine_m(logits_m[j] - lse_m), one IEEE subtraction per member, combined as in vag_beam_ens_step
 * (M = 1: the subtraction itself; M identical members give the single model bit for bit in every output).  With y the given word,
 * per position of vag_forced_score's span (up to and including the first EOS, to the last non-pad position if there is none; pad
 * positions inside it are not span positions), all sentence-major (B, Tt[, 2]):
 *   token_logp  s_y, bit for bit what vag_forced_score writes;
 *   entropy     -sum_{j < V} p_j s_j, p_j = expf(s_j), in nats; a word with p_j == 0 (a logit of -inf included) contributes exactly 0;
 *               per-lane partial sums in column order, one fixed wave tree, the waves in wave order: two runs give the same bits;
 *   rank        int32, #{ j : s_j > s_y or (s_j == s_y and j < y) }: the words ahead of the given one under the total order (score
 *               descending, word ascending); 0 = the model's own first choice;
 *   top         int32 (.., 2), top_logp (.., 2): the best and the second-best word under that order and their s (the margin is
 *               top_logp[.., 0] - top_logp[.., 1]).
 * Outside the span token_logp = entropy = top_logp = 0 and rank = top = -1.  A target word outside [0, V): NaN / -1 at that
 * position, never a stray read.  The padding columns [V, ldl[m]) are never read.
 * Per sentence, sent (B, VAG_CONF_SENT), reduced in position order over the n span positions: [0] logp and [1] score, bit for bit
 * vag_forced_score's; [2] n; [3] the population standard deviation of the span's token_logp (two passes: the mean, then the squared
 * deviations); [4] the smallest token_logp; [5] the mean and [6] the largest entropy; [7] the share of positions with rank == 0.
 * n == 0: entries 3..7 are 0.
 * Two launches: one workgroup per (t, b) row, which reads the M rows once (16-byte loads where every logits[m] is 16-byte aligned
 * and ldl[m] % 4 == 0, scalar loads otherwise); one wave per sentence.  -EINVAL with nothing launched: whatever vag_forced_score
 * rejects (a NULL array or entry, M outside [1, VAG_ENS_MAX], ldl[m] < V, B < 1, Tt < 1), V < 2, V >= 2^24, B*Tt >= 2^31, a NULL
 * output. */
#define VAG_CONF_SENT 8
int vag_token_conf(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M,
                   const int64_t* tgt, int64_t B, int64_t Tt, int64_t V,
                   float* token_logp, float* entropy, int32_t* rank, int32_t* top, float* top_logp,
                   float* sent, vag_stream_t stream);

/* The teacher's targets of word-level distillation (vag_kd_head_ce_seq_fwd) from the same inputs: M <= VAG_ENS_MAX models'
 * teacher-forced raw logits (R, ldl[m]) and their rows' log-sum-exp lse[m] (R), R = Tt*B rows.  Word j of a row scores
 * s_j = combine_m(logits_m[j] - lse_m), combined as in vag_beam_ens_step (M = 1: the one IEEE subtraction itself; M identical
 * members give the single model's idx bit for bit).  idx (R, K) int32: the row's K best words under the total order (score
 * descending, word ascending), best first; q (R, K): q_k = exp((s_k - s_0) / temperature) / sum_k', the teacher's distribution at
 * that temperature cut to those words and renormalised (the sum in a fixed order: two runs give the same bits).  One launch, one
 * workgroup per row, the M rows read once.  -EINVAL with nothing launched: K outside [1, 64] or K > V, V >= 2^24, M outside
 * [1, VAG_ENS_MAX], temperature <= 0 or not finite, a NULL array or entry, ldl[m] < V. */
int vag_kd_targets(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, int64_t R, int64_t V,
                   int64_t K, float temperature, int32_t* idx, float* q, vag_stream_t stream);

/* ---- attention alignments: the Bahdanau attention (layers/NMT_Decoder.py:27-51, :124) of the search's hypotheses and of
 * forced decoding ("soft attention of the chosen path", not a trained aligner) ------------------------------------------------ */
/* Keep step di's attention in attn_hist (max_len, B*k, Tp): alpha[m] (N, Tp), m < M <= VAG_ENS_MAX, are the rows the members'
 * decode steps (vag_cgru_attn_decode_step / _step_h) wrote for this step's N hypotheses, N = B at step 0 (one hypothesis per
 * sentence, V11.py:260; they go to the first B rows of attn_hist[0]) and B*k afterwards (:275).  The stored row is the mean over
 * members, sum_m alpha_m / M in member order: M = 1 copies the row bit for bit and two identical rows give it back exactly.
 * alpha: a host array of M entries, copied into the kernel arguments at the call (a captured graph keeps its own copy).
 * The _dev form reads the step index from di_state[0], the word vag_beam_step_dev advances: enqueue it BEFORE that step's
 * expansion; such launches are steps >= 1 and do nothing once the index has reached max_len.  One launch.
 * -EINVAL for a NULL array or entry, M out of range, k > 64, di outside [0, max_len) and empty sizes. */
int vag_beam_attn_record(const float* const* alpha, int64_t M, float* attn_hist, int64_t di, int64_t max_len, int64_t B, int64_t k,
                         int64_t Tp, vag_stream_t stream);
int vag_beam_attn_record_dev(const float* const* alpha, int64_t M, float* attn_hist, const int32_t* di_state, int64_t max_len,
                             int64_t B, int64_t k, int64_t Tp, vag_stream_t stream);
/* vag_beam_finish_nbest (out and scores bit for bit) that also walks the back-pointers (:303,:309) through attn_hist:
 * attention (B, n, max_len, Ts) float, row t of hypothesis (b, r) = the attention that produced its word t -- attn_hist[t] at
 * the hypothesis's ancestor slot after step t-1, sentence b's single row at t = 0 -- with the columns cropped from Tp to
 * Ts <= Tp.  Rows after the hypothesis's first EOS (the row that produced the EOS is kept; row max_len-1 counts as EOS, :315)
 * and rows >= steps are exactly 0.  src_pos (B, n, max_len) int64 = each row's arg-max column, the lowest index among equal
 * values, -1 where the row is zeroed.  One launch, one workgroup per sentence.  -EINVAL as vag_beam_finish_nbest, and for
 * NULL buffers, Ts < 1 and Ts > Tp. */
int vag_beam_finish_align(const float* nll, const int64_t* beam, const float* attn_hist, int64_t max_len, int64_t steps, int64_t B,
                          int64_t k, int64_t n, int64_t Tp, int64_t Ts, int64_t* out, float* scores, float* attention,
                          int64_t* src_pos, vag_stream_t stream);
/* Forced decoding's attention: alpha[m] (Tt, B, Ts) is model m's saved teacher-forced attention (the workspace slot
 * vag_cgru_ws_offset(.., 0) names, written by vag_cgru_attn_decode_seq_fwd); attention (B, Tt, Ts) = the mean over members as
 * above inside vag_forced_score's span (up to and including the first EOS of tgt (B, Tt), to the last non-pad position if there
 * is none), 0 outside it; src_pos (B, Tt) as above.  One launch.  -EINVAL for a NULL array or entry, M out of range and empty
 * sizes. */
int vag_forced_align(const float* const* alpha, int64_t M, const int64_t* tgt, int64_t B, int64_t Tt, int64_t Ts, float* attention,
                     int64_t* src_pos, vag_stream_t stream);

/* ---- sampling decoder: temperature / top-k draws from the (ensemble's) distribution ------------------------------------------ */
/* One decoder step of a sampling decode over B source sentences with n samples each: logp[m] (N_in, ldl[m]), m < M <=
 * VAG_ENS_MAX, are the members' log_softmax rows of this step, N_in = B at step 0 (rows_per_src = 1: every source row fans out
 * to its n samples, output row r reads input row r / n) and B*n afterwards (rows_per_src = n, rows map one to one).  Word w of
 * a row scores s = the ensemble score of vag_beam_ens_step (M = 1: the row itself; M identical members: the row bit for bit).
 * Candidates: every word (top_k = 0), or the top_k <= 64 best under (s desc, word asc).  The draw is Gumbel-max over them,
 *     tok = argmax_w ( s[w] * inv_T + g(r, w) ),   inv_T = 1.0f / temperature (fp32, on the host),
 * the product and the sum rounded separately (no fma), ties to the lowest word; g = -log(-log(u)), u = (x + 0.5) 2^-23 with x
 * 23 bits of a counter-based generator keyed by rng = {seed, call counter} (uint64[2] in device memory, the layout of the
 * dropout generator; advance it with vag_rng_advance between decodes), the step index and the output row -- so a decode is a
 * pure function of (inputs, rng), whatever the launch order.  top_k = 1 is the arg-max of vag_ens_argmax at any temperature.
 * History: toks (max_len, B*n) int64 and token_logp (max_len, B*n) float, time-major; the step writes its row di: the drawn
 * word and its UNTEMPERED, UNTRUNCATED log-probability s[tok] (comparable with vag_forced_score).  A row whose previous word
 * toks[di-1] is EOS = 3 emits EOS at log-probability 0.  tok_out (B*n, may be NULL) also receives the words (the next step's
 * input).  n_alive: int32[3], zero before the first step; [0] = the rows of the last step whose word is not EOS, [1] and [2]
 * are the kernel's own (left zero).  Hidden states: step 0 replicates h_in[m] (B, H[m]) -> h_out[m] (B*n, H[m]) by source row;
 * later steps do not touch them (h_in, h_out, H are ignored and may be NULL): the state a member's decoder step wrote is the
 * next step's input as it is.  logp, ldl, h_in, h_out, H: host arrays of M entries, copied into the kernel arguments.
 * One launch, one workgroup per output row, every log-probability row read once, no host synchronisation.
 * -EINVAL for top_k outside [0, 64], temperature <= 0 or not finite, V >= 2^24 with top_k > 0, NULL buffers, arrays or entries,
 * di outside [0, max_len), and everything vag_ens_argmax rejects. */
int vag_sample_step(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                    int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out, int64_t B,
                    int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng, int32_t* n_alive,
                    vag_stream_t stream);
/* The same with the step index in device memory: di_state (int32[1]) holds the step this launch runs and is advanced by it, so
 * one captured graph serves every step.  Such launches are steps >= 1 (no hidden states) and do nothing once the index has
 * reached max_len. */
int vag_sample_step_dev(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int32_t* di_state,
                        int64_t max_len, int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k,
                        const uint64_t* rng, int32_t* n_alive, vag_stream_t stream);
/* Nucleus (top-p) sampling: vag_sample_step / vag_sample_step_dev with the draw restricted to the nucleus of the candidate pool
 * P (the whole row at top_k = 0, else the top_k set above; the order is temperature, top_k, then top_p on the pool's renormalised
 * mass).  With t[w] = fl(s[w] * inv_T), m = max_P t, e[w] = expf(t[w] - m), Z = sum_P e (fp32):
 *     nucleus = { w in P : s[w] >= s* },   s* = the largest score in P with  sum { e[w] : w in P, s[w] >= s* }  >=  fl(top_p * Z),
 * a value threshold: words of equal score are in or out together, the set is a prefix of the (s desc, word asc) order that ends
 * on a tie-group boundary.  The sums are fp32 in an order fixed by (V, thread layout) alone, without floating-point atomics, so a
 * decode stays a pure function of (inputs, rng).  The draw is the same arg-max of fl(fl(s * inv_T) + g) with the same key, noise
 * and tie rule over the nucleus; token_logp is still the untempered, untruncated s[tok].  top_p = 1 is the whole pool: the words
 * and log-probabilities of vag_sample_step bit for bit.  set_size (may be NULL): int32, the layout of toks; the step writes its
 * row di: the nucleus' words (NaN scores carry no mass and are not counted), 0 for a row that was finished before this step
 * and, at top_k = 0, for an all-NaN row, which gives word 0 at NaN (the top_k selection does not order NaNs: what a top_k pool
 * holds for such a row is undefined, here as in vag_sample_step).  top_k = 0 reads the row
 * 2 + 32/4 times (maximum, threshold search of 4 key bits per pass, draw); top_k > 0 reads it once.  One launch, as above.
 * -EINVAL also for top_p outside (0, 1] or NaN. */
int vag_sample_step_p(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                      int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H, int64_t* tok_out, int64_t B,
                      int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng, int32_t* n_alive, float top_p,
                      int32_t* set_size, vag_stream_t stream);
int vag_sample_step_p_dev(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp,
                          int32_t* di_state, int64_t max_len, int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature,
                          int64_t top_k, const uint64_t* rng, int32_t* n_alive, float top_p, int32_t* set_size,
                          vag_stream_t stream);
/* out (N, V) float = the noise g(r, w) that step di's launch adds under this rng state, by the step's own device function (bit
 * for bit): lets a test or an audit reproduce a draw.  Not on the hot path. */
int vag_sample_noise(const uint64_t* rng, int64_t di, int64_t N, int64_t V, float* out, vag_stream_t stream);

/* ---- minimum-Bayes-risk selection over candidate translations ------------------------------------------------------------ */
/* Chooses, per sentence, the candidate with the highest expected utility against a set of pseudo-references (usually the
 * sampler's draws).  Definitions, for a token row x of length L (int64 vocabulary ids in [0, 2^31)):
 *   span     the tokens of x before its first EOS = 3, or the whole row if it holds none; l = the span's length.  What follows
 *            the EOS is never read as content.  A padding word 0 inside the span is an ordinary token (a sampler can draw it).
 *   T_n(x)   = max(0, l - n + 1), the span's number of n-grams.
 *   m_n(h,r) = sum over n-grams g of min(count_h(g), count_r(g)), n = 1..4: the clipped match count; an integer, symmetric.
 * utility = 0, "bleu": the reference's segment-level smooth BLEU (bleu.py: compute_bleu([[r]], [h], smooth=True)[0]),
 *     u(h, r) = 0 if l_h = 0, else  bp * exp( 1/4 sum_{n=1..4} log( (m_n + 1) / (T_n(h) + 1) ) ),
 *     bp = 1 if l_h > l_r (so also for an empty reference, where bleu.py divides by zero), else exp(1 - l_r / l_h);
 * utility = 1, "ngram_f": the mean of 2 m_n / (T_n(h) + T_n(r)) over the n in 1..4 with T_n(h) + T_n(r) > 0, 0 if there is no
 *     such n; symmetric, no transcendental function.
 * Both are evaluated in fp32 with logf / expf and IEEE division.
 * Expected utility: E_i = sum_j w_j u(h_i, r_j), fp32, j = 0 .. Nr-1 in that order, each product and each sum rounded on its
 * own (no fma): bitwise reproducible.  w_j = weights[b, j] as given (not normalised here), or 1.0f / Nr with weights NULL.
 * best[b] = the lowest i whose E_i is maximal, compared on the fp32 values written to expected.
 * hyps (B, Nh, Lh) int64; refs (B, Nr, Lr) int64, or NULL: the candidates are their own references (Nr, Lr must equal Nh, Lh);
 * weights (B, Nr) or NULL; matches (B, Nh, Nr, 4) int32 or NULL: m_1..m_4 of every pair; util (B, Nh, Nr) or NULL: u of every
 * pair; expected (B, Nh); best (B,).  Ids are compared on their low 32 bits.
 * Limits (vag_mbr_supported: a pure host call, 1 or 0): 1 <= Nh, Nr <= 1024 and 1 <= Lh, Lr <= 512; B < 2^21.
 * Two launches (the pairs: one workgroup per candidate; the arg-max: one wave per sentence), no floating-point atomics, no
 * host synchronisation.  -EINVAL, before anything touches the device, for NULL hyps / expected / best, a size below 1, an
 * unknown utility, refs NULL with (Nr, Lr) != (Nh, Lh), and a shape vag_mbr_supported refuses. */
int vag_mbr_supported(int64_t Nh, int64_t Lh, int64_t Nr, int64_t Lr);
int vag_mbr_select(const int64_t* hyps, const int64_t* refs, const float* weights, int64_t B, int64_t Nh, int64_t Lh, int64_t Nr,
                   int64_t Lr, int utility, int32_t* matches, float* util, float* expected, int64_t* best, vag_stream_t stream);

/* ---- corpus BLEU statistics: what a validation pass needs, on the device ---------------------------------------------------- */
/* The sufficient statistics of the reference's corpus BLEU (bleu.py: compute_bleu(reference_corpus, translation_corpus)) for N
 * sentences, each a hypothesis and up to R references.  hyps (N, Lh) int64; refs (N, R, Lr) int64; n_refs (N,) int32, the number
 * of references of every sentence, or NULL: R everywhere.  Its values are clamped to [1, R]; rows j >= n_refs[b] are never
 * read.  Span, l and T_n as in vag_mbr_select: the tokens before the first EOS = 3, or the whole row; a padding word 0 inside
 * the span is an ordinary token; ids are compared on their low 32 bits, of which 0xFFFFFFFE and 0xFFFFFFFF are not ids (the
 * kernels of both entry points pad with them).  Per sentence, ten integers
 *   m_1..m_4, T_1..T_4, l_h, l_r
 * with T_n = max(0, l_h - n + 1), l_r = min_j l_{r_j} over the sentence's references (bleu.py:67) and
 *   m_n = sum over n-grams g of min(count_h(g), max_j count_{r_j}(g)),
 * the matches clipped by the MERGED counts of the references (bleu.py:70-83: merged_ref_ngram_counts |= ..., the per-n-gram
 * maximum) -- not the maximum over j of vag_mbr_select's m_n(h, r_j), which clips against one reference at a time ("a a b" against
 * "a a" and "b b": m_1 = 3, while either reference alone gives 2 or 1).
 * per_sentence (N, 10) int32 or NULL receives them; totals (10,) int64, which must be given, has the same ten numbers ADDED to
 * it with integer atomics.  It is not zeroed here: one buffer accumulates a dev set batch after batch with no host
 * synchronisation, and being integer sums its values do not depend on the order of anything.  The corpus score is formed from
 * the totals by the caller (vagnmt_hip/validate.py, in the reference's double arithmetic): nothing here is floating point.
 * One launch, one workgroup per sentence (the matching of vag_mbr_select's pairs kernel; the waves split the references, keep a
 * running integer maximum per position and order, and combine through LDS).
 * Limits (vag_corpus_bleu_supported: a pure host call, 1 or 0): 1 <= Lh, Lr <= 512, 1 <= R <= 64; N < 2^31.  -EINVAL, before
 * anything touches the device, for NULL hyps / refs / totals, a size below 1, and a shape vag_corpus_bleu_supported refuses. */
int vag_corpus_bleu_supported(int64_t Lh, int64_t R, int64_t Lr);
int vag_corpus_bleu_stats(const int64_t* hyps, const int64_t* refs, const int32_t* n_refs, int64_t N, int64_t Lh, int64_t R,
                          int64_t Lr, int32_t* per_sentence, int64_t* totals, vag_stream_t stream);

/* ---- chrF on surface characters: the same selection on what the ids spell -------------------------------------------------- */
/* A surface table maps every vocabulary id to the Unicode code points of its word (CSR: off (V + 1,) int32 ascending from 0,
 * chars (off[V],) int32 code points in [0, 2^31)); the host builds it (vagnmt_hip/surface.py: BPE join markers and whitespace
 * are dropped there, padding / SOS / EOS get the empty surface).
 * vag_surface_expand: rows (R, L) int64 token rows -> out (R, C) int32 character rows and lens (R,) int32.  The span of a row is
 * vag_mbr_select's (the tokens before the first EOS = 3, or the whole row; a padding word 0 inside it is an ordinary token).  The
 * character row is the concatenation of the surfaces of the span's tokens, in order; lens[r] is its TRUE length, of which only
 * the first min(lens[r], C) characters are stored.  What lies beyond them in out is unspecified and nothing here reads it.  An id
 * outside [0, V) is the caller's to exclude (it contributes no character).  One launch, one wave per row (a wave-level prefix
 * sum of the token lengths gives every token's offset), no atomics.  -EINVAL before the launch for a NULL pointer, a size below
 * 1, L > 512, or R, C or V of 2^31 and more.  The caller keeps L * (the longest surface) below 2^31.
 *
 * vag_chrf_select is vag_mbr_select on character rows: hchars (B, Nh, Ch) int32 with hlens (B, Nh); rchars (B, Nr, Cr) with rlens
 * (B, Nr), or both NULL: the candidates are their own references (Nr, Cr must equal Nh, Ch); weights (B, Nr) or NULL; matches
 * (B, Nh, Nr, 6) int32 or NULL; util (B, Nh, Nr) or NULL; expected (B, Nh); best (B,).  Characters are compared on their low 31
 * bits.  Definitions, for a character row x of stored length l = min(max(len, 0), C):
 *   T_n(x)   = max(0, l - n + 1), n = 1..6.
 *   m_n(h,r) = sum over character n-grams g of min(count_h(g), count_r(g)): an integer, symmetric.
 *   An order n is effective when T_n(h) > 0 and T_n(r) > 0; E = the number of effective orders.
 *   P = ( sum over the effective n, ascending, of m_n / T_n(h) ) / E, the sum starting from 0;  R the same with T_n(r).
 *   u(h, r) = ((5 P) R) / ((4 P) + R), the F score with beta = 2;  u = 0 when E = 0 or P + R = 0.  0 <= u <= 1.
 * All of it in fp32 (m_n, T_n and E converted exactly), every division, product and sum rounded to nearest on its own, no fma,
 * no reciprocal approximation, in the order written: IEEE float32 arithmetic on the host gives the same bits.  This is chrF
 * (Popovic 2015) as sacreBLEU computes it by default: character order 6, beta 2, whitespace removed, averaged over the effective
 * orders.  chrF++ (word n-grams) is not computed.
 * Expected utility and best are exactly vag_mbr_select's (fixed order of j, product and sum rounded separately, w_j = weights[b, j]
 * or 1.0f / Nr; the lowest index of the maximum).
 * Limits (vag_chrf_supported: a pure host call, 1 or 0): 1 <= Nh, Nr <= 1024 and 1 <= Ch, Cr <= vag_chrf_max_chars() = 1024 (set
 * by the LDS of a workgroup: csrc/chrf.hip has the budget); B < 2^21.  A longer sentence is cut to its first C characters by the
 * expansion, which lens shows.  Two launches (the pairs: one workgroup per candidate; the arg-max), integers only inside the
 * matching, no hashing, no sorting, no floating-point atomics: two runs give the same bits.  -EINVAL, before anything touches
 * the device, for NULL hchars / hlens / expected / best, rchars without rlens or the reverse, a size below 1, rchars NULL with
 * (Nr, Cr) != (Nh, Ch), and a shape vag_chrf_supported refuses. */
int vag_surface_expand(const int64_t* rows, int64_t R, int64_t L, const int32_t* off, const int32_t* chars, int64_t V, int32_t* out,
                       int64_t C, int32_t* lens, vag_stream_t stream);
int vag_chrf_supported(int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr);
int vag_chrf_max_chars(void);
int vag_chrf_select(const int32_t* hchars, const int32_t* hlens, const int32_t* rchars, const int32_t* rlens, const float* weights,
                    int64_t B, int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr, int32_t* matches, float* util, float* expected,
                    int64_t* best, vag_stream_t stream);

/* ---- minimum-risk training: sentence-level risk over candidate translations ----------------------------------------------- */
/* Shen et al. 2016 ("Minimum Risk Training for Neural Machine Translation"), Edunov et al. 2018: in place of the token-level loss of
 * models/NMT_AttentionImagine_Seq2Seq_Beam_V11.py:162-166 (loss_mt += criterion_mt(...); loss_mt / tgt_mask.sum(-1); .mean()) the
 * expected cost of N candidate translations y_i of a source sentence under the model's renormalised distribution over them:
 *   s_i = log p(y_i | x),  c_i = 1 - BLEU(y_i, gold),  Q_i = softmax_i(alpha s_i),  R = sum_i Q_i c_i,
 *   dR / d theta = sum_i alpha Q_i (c_i - R) d s_i / d theta.
 * That is a cross-entropy gradient with one coefficient per sentence, and the head's backward already has one: it multiplies every
 * row of sentence b by d_loss * inv_cnt[b] / B * w (vag_head_ce_seq_bwd), the gradient of sum_b inv_cnt[b] / B * sum_t nll[t, b] =
 * -sum_b inv_cnt[b] / B * s_b.  For the risk of a call, scale / G * sum_g R_g over its G = B / N groups, the two agree for
 *   inv_cnt[b_i] = -scale * N * alpha * Q_i * (c_i - R_g)
 * (the sign: nll = -s; the factor N: the backward divides by the B = G N rows, the risk by the G groups).
 * vag_mrt_weights: nll (Tt, B) time-major as the head writes it (0 at padded positions); rows b = g N .. g N + N - 1 are the candidates
 * of group g; cost, valid (B,) floats, valid NULL = all valid.  Per group, over its valid rows: s_i = -sum_t nll[t, b_i] (t
 * ascending; only the exponential is fp32, the sums around it are double), Q_i = exp(alpha s_i - max) / Z, R_g = sum_i Q_i c_i,
 * inv_cnt[b_i] as above; an invalid row gets inv_cnt = 0 and q = 0; risk[0] = scale / G * sum_g R_g.  q (B,) or NULL.  A group with one valid row has Q = 1 and coefficient 0; one with
 * none contributes R_g = 0.  The largest exponent is 0, so saturated inputs give neither NaN nor Inf.  One launch of one workgroup;
 * every sum has a fixed order and there is no floating-point atomic: two runs give the same bits.
 * scale: a driver may run the groups of one optimiser step in several calls with scale = groups of the call / groups of the step;
 * the risks add up to the step's and the gradients accumulate.
 * -EINVAL before any launch unless 2 <= N <= 256, B % N == 0, Tt >= 1, alpha > 0 and finite, scale > 0 and finite, and nll, cost,
 * inv_cnt, risk are not NULL. */
int vag_mrt_weights(const float* nll, const float* cost, const float* valid, int64_t B, int64_t Tt, int64_t N, float alpha, float scale,
                    float* inv_cnt, float* q, float* risk, vag_stream_t stream);
/* Candidates -> forced targets.  cand (G, Nc, L) int64 in the samplers' format (a row's span: the tokens before its first EOS = 3, or
 * the whole row); gold (G, Tg) in the training format (words, EOS, zero padding; read only with include_gold = 1).  tgt (G N, Tt)
 * with N = Nc + include_gold and Tt >= max(L + 1, Tg): every row is its span, one EOS, zeros; the gold row is candidate 0 of its group
 * when included (a gold row that holds no EOS is cut to Tt - 1 words).  valid (G N,) floats: 0 for a row whose span equals that of an
 * earlier valid row of its group (a gold sentence that was also sampled, a sampler's repeats) and for a row whose span holds the
 * padding word 0 (the loss skips that word, so s would not be the row's log-probability), else 1.  An empty span is a valid one-token
 * row.  One workgroup per source sentence.  -EINVAL before the launch for NULL cand / tgt / valid (gold with include_gold), sizes
 * below 1, N > 256, L > 512, Tg > 513, or a Tt below the bound. */
int vag_mrt_pack(const int64_t* cand, int64_t G, int64_t Nc, int64_t L, const int64_t* gold, int64_t Tg, int include_gold, int64_t* tgt,
                 int64_t Tt, float* valid, vag_stream_t stream);

/* ---- a13: optimiser step, train.py:46-49 + nmt_multimodal_beam_DE.py:303-332 -------------------------- */
/* Global-norm clip (clip_grad_norm_, eps 1e-6) fused with Adam over one flat fp32 buffer of n elements split
 * into nseg contiguous segments [seg_off[i], seg_off[i+1]) with their own lr / L2 weight decay (the reference's
 * param groups).  grad_scale multiplies every gradient first (1/world_size after a sum all-reduce).
 * seg_off (nseg+1), seg_lr, seg_wd are HOST arrays (read while enqueuing).  step: device int32 counter,
 * incremented here.  norm_out (1): total gradient norm before clipping.  scratch: VAG_ADAM_SCRATCH_BYTES, 8-byte aligned. */
#define VAG_ADAM_SCRATCH_BYTES 2048
/* A void gradient is never applied (train.py:44-49 holds for every step that IS applied): when the gradient norm is not
 * finite, or a persistent recurrence kernel launched under THIS scratch's guard pair (VAG_ADAM_SCRATCH_GUARD_OFFSET) gave up a wait
 * since the previous call (on a replica
 * of a data-parallel run the give-up reaches every rank as a non-finite entry of the all-reduced gradient), this call leaves
 * p, m, v and *step unchanged, still zeroes g (zero_grad), writes NaN to norm_out and adds one to the uint32 at byte
 * VAG_ADAM_SCRATCH_SKIPPED_OFFSET of the scratch (a host reads it from there whenever it likes; TrainStep.skipped_steps). */
#define VAG_ADAM_SCRATCH_SKIPPED_OFFSET 28
/* The driver's guard pair {void flag, give-up count} (two uint32) lives at this byte offset of the scratch: pass its address as
 * vag_step_cfg.guard (or vag_set_operator_guard) and this call skips exactly the steps whose OWN recurrence launches gave up a
 * wait; the count is the driver's to read and reset (TrainStep.check). */
#define VAG_ADAM_SCRATCH_GUARD_OFFSET 32
/* zero_grad != 0: g is left zeroed (the next step's backward accumulates into it; no separate fill pass).
 * scratch must be zero before the FIRST call; every call leaves it ready for the next one.  Three launches.
 * lr_dev: NULL, or one DEVICE float that multiplies every seg_lr when the kernels run: with seg_lr = the groups' relative
 * rates and *lr_dev = the current learning rate, a captured graph of this call serves every learning rate. */
int vag_clip_adam_flat(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                       const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1,
                       float beta2, float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch,
                       const float* lr_dev, vag_stream_t stream);

/* The same step (same three launches, scratch contract, skip rules and zero_grad) that also keeps AVERAGED weights: a Polyak /
 * exponential moving average of the parameters, which the reference does not have -- it stands beside train.py:44-49 (backward,
 * clip, optimizer.step()) as the line a recipe adds after optimizer.step().  ema: n floats, 16-byte aligned, laid out as p
 * (initialise it from p).  In the streaming pass, with p_new exactly what vag_clip_adam_flat stores,
 *     ema[k] += (1 - d_t) * (p_new[k] - ema[k])       d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay
 * in fp32, t = *step after this call's increment; 1 - d_t is formed on the device (in double) from the step counter, so a captured
 * graph of this call serves every step.  A skipped step leaves ema exactly as it was, together with p, m, v and *step.
 * -EINVAL before anything is enqueued: ema NULL or not 16-byte aligned, ema_decay not inside (0, 1) (NaN included) -- "no
 * averaging" is vag_clip_adam_flat, not this call with a zero.  There is no sharded form. */
int vag_clip_adam_flat_ema(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                           const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1,
                           float beta2, float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch,
                           const float* lr_dev, float* ema, float ema_decay, int ema_warmup, vag_stream_t stream);

/* a[0, n) <-> b[0, n) in place, one launch (the averaged weights of vag_clip_adam_flat_ema take the parameters' place for
 * validation / decoding / export and go back the same way, bit for bit: what a recipe does around the evaluation that follows
 * train.py:44-49's steps).  Both bases 16-byte aligned and the two ranges disjoint, else -EINVAL; nothing beyond n is read or
 * written; n == 0 is a no-op. */
int vag_swap_flat(float* a, float* b, int64_t n, vag_stream_t stream);

/* The same optimiser step for ONE contiguous shard [lo, hi) of the flat buffer (lo a multiple of 4): the data-parallel option of
 * SURVEY.md 8e / section 5 for train.py:46-49 -- gradient by reduce-scatter, sharded sum of squares / clip / Adam, parameters back by
 * all-gather (vagnmt_hip.trainer.TrainStep(zero1=True)).  Two calls per step with one all-reduce of ONE double in between:
 *   phase 0: sumsq[0] (device) = sum of squares of g[lo, hi)            -- the caller sums it over the ranks
 *   phase 1: clip coefficient from that global sum (norm_out: the global norm), step counter, Adam on the segments cut to [lo, hi);
 *            zero_grad: all of g[0, n) is zeroed.  Skips (non-finite norm, guard flag) as vag_clip_adam_flat; the step counter
 *            advances on every rank alike because every rank sees the same global sum. */
int vag_clip_adam_shard(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                        const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1,
                        float beta2, float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch,
                        const float* lr_dev, int64_t lo, int64_t hi, int phase, double* sumsq, vag_stream_t stream);

/* ---- a2 + a13: the whole training step (train.py:36-51 around models/...V11.py:82-168 and
 * NMT_Seq2Seq_Beam_V2.py:58-113) as ONE call: every operator above in the order autograd would run them, on one
 * caller-owned workspace.  Gradients are ACCUMULATED into g (keep it zeroed between steps: vag_clip_adam_flat with
 * zero_grad does).  The per-operator entry points stay the public API for the reference's module-level calls
 * (model.forward + loss.backward()); this is what the step driver (vagnmt_hip/trainer.py) replays from a HIP graph. */
typedef struct {
    const float* enc_emb;                 /* encoder.embedding.weight (Vs,Es) */
    vag_gru_w enc_fw, enc_bw;             /* encoder.gru.*_l0 / *_l0_reverse */
    /* vse_imagine.* -- all NULL for the text-only model (NMT_Seq2Seq_Beam_V2) */
    const float *im_w, *im_b, *txt_w, *txt_b, *ctx2ctx, *emb2ctx, *mlp_w;
    const float *ini_w, *ini_b;           /* decoderini */
    const float* attn_e;                  /* decoder.attn.attn_e.weight (C,C) */
    vag_dec_w dec;
    vag_head_w head;
} vag_model_w;
typedef struct {
    float* enc_emb;
    vag_gru_g enc_fw, enc_bw;
    float *im_w, *im_b, *txt_w, *txt_b, *ctx2ctx, *emb2ctx, *mlp_w;
    float *ini_w, *ini_b;
    float* attn_e;
    vag_dec_g dec;
    vag_head_g head;
} vag_model_g;
typedef struct {
    int64_t B, Ts, Tt, Es, Et, H, S, I, V, ldl;   /* Es/Et: source/target embedding size; ldl = ceil4(V) */
    int32_t multimodal;                   /* 1: V11 (image branch + ranking loss), 0: text-only V2 */
    int32_t attn_method;                  /* imagine attention: 0 'dot', 1 'mlp' */
    int32_t activation_vse;               /* tanh on the shared-space projections */
    int32_t rank_kind;                    /* 0 pairwise, 1 image retrieval, -1 no criterion_vse (loss_vse = 0) */
    int32_t free_run;                     /* 0 teacher forcing, 1 feed back the argmax (V11.py:148-160) */
    int32_t storage;                      /* 0: everything fp32.  1 (BASELINE configs[4], "fp16"): what the recurrences stream at
                                           * every time step -- their weights and the attention keys / projected keys -- is
                                           * kept as fp16 in HBM; accumulation, master weights, recurrent state, saved gates and
                                           * all gradients stay fp32.  Teacher-forced steps only; needs `derived` built with
                                           * with_fp16 and H % 8 == 0 */
    float margin, loss_w, init_split, p_emb, p_ctx, p_out;
    int32_t loss_ring;                    /* R > 0: `losses` holds 4 + 4 R floats; the forward phase also stores {loss, loss_mt, loss_vse}
                                           * of its n-th execution (n kept in the bit pattern of losses[3]) at losses[4 + 4 (n % R)]:
                                           * a driver that replays captured graphs hands out results that stay valid for R steps
                                           * without a copy launch per step.  0: losses is 4 floats */
    void* guard;                          /* NULL, or two caller-owned DEVICE uint32 {void flag, give-up count} (zero before the first
                                           * call): the persistent recurrence kernels of THIS call report a give-up there and nowhere
                                           * else, so several drivers on one device cannot void each other's steps.  The step driver
                                           * passes (char*)adam_scratch + VAG_ADAM_SCRATCH_GUARD_OFFSET, the words vag_clip_adam_flat
                                           * reads.  NULL: the calling thread's operator guard (vag_set_operator_guard), else the
                                           * process-wide pair no optimiser reads */
    float label_smoothing;                /* eps of the translation loss (see vag_head_ce_seq_fwd_ls): 0 <= eps < 1, else -EINVAL.
                                           * 0 (a zero-initialised struct): the reference's NLLLoss, the kernels of the plain loss */
    int32_t mrt_n;                        /* N > 0: a minimum-risk step (vag_mrt_weights).  The B rows are G = B / N groups of N forced
                                           * candidate translations of one source sentence each (rows g N .. g N + N - 1; source, length
                                           * and image repeated N times by the caller).  The forward phase runs the head as always and
                                           * then, in place of the loss reduction, vag_mrt_weights' launch on the step's nll: loss_mt =
                                           * the risk, loss = w_mt * risk, loss_vse = 0, ring slot and execution counter as ever; the
                                           * backward is unchanged and reads the coefficients that launch left in inv_cnt.  The chunked
                                           * head then always recomputes its chunks in the backward, and the loss reduction never rides
                                           * in the backward's first launch: both need coefficients known before the head's forward ends.
                                           * -EINVAL unless B % N == 0, 2 <= N <= 256, free_run == 0, label_smoothing == 0, storage == 0
                                           * and rank_kind == -1 (a ranking loss over a batch that holds every image N times means
                                           * nothing; the 2-byte mode is out of scope).
                                           * 0 (a zero-initialised struct): off -- the launches are those of the plain step, and none
                                           * of the fields below is read */
    float mrt_alpha, mrt_scale;           /* vag_mrt_weights' alpha (> 0, finite) and scale (> 0): groups of this call / groups of the
                                           * optimiser step when a driver runs a step's groups in several calls (gradients accumulate) */
    const float *mrt_cost, *mrt_valid;    /* (B,) device floats: every row's cost c = 1 - BLEU, and 1 / 0 = takes part or not (NULL: all) */
} vag_step_cfg;
/* phases: bit 0 forward (losses[0..2] = loss, loss_mt, loss_vse), bit 1 backward down to the encoder states (final for
 * every gradient except the encoder's), bit 2 the encoder's backward.  A data-parallel driver all-reduces the first
 * gradient bucket while phase 4 runs.  Phase 2 may also be called as its two halves: 16 = output head + decoder (final for
 * the head's, the decoder's and attn_e's gradients), 32 = visual grounding + initial state (final for vse_imagine.* and
 * decoderini.*), for a driver that cuts the gradient into three buckets (phases 1|16, then 32, then 4).  rng: {seed, step} (step is advanced by the forward phase) or NULL (no dropout).
 * derived: vag_derived_floats(H) floats kept current with vag_derive_weights() after every optimiser step, or NULL
 * (derived weights are then rebuilt inside the call).  ws: vag_step_ws_floats(cfg) floats, kept between phases. */
int64_t vag_step_ws_floats(const vag_step_cfg* cfg);
int64_t vag_step_ws_offset(const vag_step_cfg* cfg, int which);
int vag_train_step(const vag_step_cfg* cfg, const vag_model_w* w, const vag_model_g* g, const int64_t* src,
                   const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight, uint64_t* rng,
                   const float* derived, float* ws, float* losses, int phases, vag_stream_t stream);
/* A word-level distillation step (vag_kd_head_ce_seq_fwd): vag_train_step whose translation loss mixes the gold word with the
 * teacher's K best words of every target position.  The teacher's targets travel beside the configuration, in a struct of their
 * own, so vag_step_cfg and every caller of vag_train_step stay as they are.  The launches are the plain step's plus two small ones
 * per pass of the head over rows (whole sequence, or each chunk of a chunked head in either of its forms); the ranking loss stays
 * on; the workspace is vag_step_ws_floats(cfg), unchanged.  k and lambda are read by value while enqueuing, so a captured graph
 * holds them; idx and q are caller-owned static buffers beside the batch.
 * vag_step_kd_check: host only, 0 or -EINVAL -- what vag_train_step_kd answers for (cfg, kd) before it looks at anything else:
 * -EINVAL unless cfg is a valid configuration, kd is not NULL, 1 <= k <= 64, k <= V, 0 < lambda <= 1 (NaN refused), idx and q are
 * not NULL, and free_run == 0, label_smoothing == 0, mrt_n == 0, storage == 0.  "No distillation" is vag_train_step. */
typedef struct {
    int32_t k;                            /* K: the teacher's words per target position */
    float lambda;                         /* weight of the teacher's term: nll = w ((1 - lambda) CE(gold) + lambda CE(teacher)) */
    const int32_t* idx;                   /* (Tt*B, K) device int32, rows time-major: the teacher's words (distinct, in [0, V)) */
    const float* q;                       /* (Tt*B, K) device floats: their probabilities, each row summing to 1 (vag_kd_targets) */
} vag_kd_cfg;
int vag_step_kd_check(const vag_step_cfg* cfg, const vag_kd_cfg* kd);
int vag_train_step_kd(const vag_step_cfg* cfg, const vag_kd_cfg* kd, const vag_model_w* w, const vag_model_g* g, const int64_t* src,
                      const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight, uint64_t* rng,
                      const float* derived, float* ws, float* losses, int phases, vag_stream_t stream);
/* An R-Drop step (vag_rdrop_head_ce_seq_fwd): vag_train_step on a batch that holds every sentence twice, in adjacent rows (B even;
 * rows 2 p, 2 p + 1: the same source, lengths, target and image), whose translation loss carries the symmetric KL term between
 * the twins' distributions with weight alpha.  Label smoothing composes with it.  The ranking loss runs with the twin flag
 * (vag_rank_loss_fwd: kind | 2) and is scaled by 1/4 -- each of the B rows meets every other sentence twice -- so with all dropout
 * at 0 every loss equals the plain step's on the B / 2 sentences.  The launches are the plain step's plus one per pass of the head
 * over rows, with the head's d(logits) pass replaced by R-Drop's and the loss reduction launched on its own; the workspace is
 * vag_step_ws_floats(cfg), unchanged.  alpha is read by value while enqueuing, so a captured graph holds it; kl is a caller-owned
 * static buffer beside the batch.
 * vag_step_rdrop_check: host only, 0 or -EINVAL -- what vag_train_step_rdrop answers for (cfg, rd) before it looks at anything
 * else: -EINVAL unless cfg is a valid configuration, rd is not NULL, alpha > 0 and finite (NaN refused), kl is not NULL, B is even,
 * and free_run == 0, mrt_n == 0, storage == 0.  "No R-Drop" is vag_train_step. */
typedef struct {
    float alpha;                          /* weight of the symmetric KL term (the paper's alpha) */
    float* kl;                            /* (Tt*B) device floats, rows time-major: KL(p_r || p_twin), written by the forward */
} vag_rdrop_cfg;
int vag_step_rdrop_check(const vag_step_cfg* cfg, const vag_rdrop_cfg* rd);
int vag_train_step_rdrop(const vag_step_cfg* cfg, const vag_rdrop_cfg* rd, const vag_model_w* w, const vag_model_g* g,
                         const int64_t* src, const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight,
                         uint64_t* rng, const float* derived, float* ws, float* losses, int phases, vag_stream_t stream);
/* The per-operator entry points (vag_bigru_seq_*, vag_attn_keys_proj, vag_cgru_attn_decode_seq_*) normally rebuild the
 * derived weights inside their workspaces and use fp32 storage.  This sets, for the CALLING THREAD until changed, the
 * driver-owned derived buffer they should read instead and the storage mode (vag_step_cfg.storage); vag_train_step does the
 * same for the duration of its call.  derived = NULL, storage = 0 restores the defaults. */
int vag_set_operator_context(const float* derived, int storage);
/* Process-wide debug / tuning options by name, for the parity tests and tuning scripts (none is needed in normal use):
 * "gemm_f32mfma" (1: every product on the exact f32-input MFMA kernels), "gemm_nogroup", "gemm_force_tile" +
 * "gemm_force_splitk", "gemm_debug", "head_chunk" (rows per chunk of the output head; -1 automatic, 0 never),
 * "head_fuse", "head_bf16_grads", "head_bf16_dlogits" (2-byte mode, chunked head: d(logits) as bf16), "s16_one_plane"
 * (2-byte mode of vag_train_step: one-plane products), "persistent" / "persistent_dec_bwd" (0: launch chains instead of the
 * one-launch recurrence kernels), "persist_timing" (vag_recurrence_time), "dec_stamps" / "dec_bwd_stamps" (device address
 * for phase timestamps of the decoder kernels), "handoff_planes" (a bit mask, default 15; 0: the one-launch recurrences hand their rows
 * off as fp32, which every consumer splits again, instead of as bf16 planes split once by the producer; bit 0: the backward
 * recurrences' hand-offs; bit 1, with bit 0: the decoder backward's hidden-side product takes its dgh2 rows and its W_hh2^T slice
 * as planes too, the slice split once per launch; bit 2: the encoder forward's state rows, where the caller has set a plane
 * buffer; bit 3: the teacher-forced decoder forward's h1 and h2 rows, as planes that carry their own "written" marks, where the
 * caller's buffer holds vag_handoff_planes_floats: same results bit for bit in every form, kept for A/B timing).  Returns
 * VAG_EINVAL for an unknown name. */
int vag_set_option(const char* name, int64_t value);
/* The one-launch backward recurrences (and, given the buffer, the two forward ones) publish the rows their workgroups hand to each other as bf16 planes in a buffer of the
 * CALLER's: vag_handoff_planes_floats(B, Ts, Tt, H) floats (host only; 0 where the shape has no such kernel), 16-byte aligned,
 * contents arbitrary -- a launch reads only what it wrote, except in the decoder forward's region (vag_dec_fwd_planes_floats(B, Tt, H)
 * floats behind the encoder forward's), whose planes carry marks: the library zeroes that region itself before every launch that
 * uses it.  The need is the largest of the two forwards' regions together, the encoder's backward and the decoder's backward, which
 * use the buffer one after the other.  vag_set_handoff_planes names it for every call the CALLING THREAD makes until changed (vag_train_step and the operator
 * entry points alike; NULL, 0 = none).  Without a buffer, or with one too small for a call's shape, the kernels keep the fp32
 * hand-off (the decoder's backward: the hand-off planes alone while those still fit): same results, slower.  The buffer must stay alive while work that was enqueued (or captured) with it can run. */
int64_t vag_handoff_planes_floats(int64_t B, int64_t Ts, int64_t Tt, int64_t H);
int64_t vag_dec_fwd_planes_floats(int64_t B, int64_t Tt, int64_t H);
int vag_set_handoff_planes(float* buf, int64_t floats);
/* Up to four contiguous device byte ranges copied by one launch (src[i] -> dst[i], bytes[i]; host arrays): a batch's
 * src / lengths / tgt / image rows into the step driver's static input buffers. */
int vag_copy4(const void* const* src, void* const* dst, const int64_t* bytes, int n, vag_stream_t stream);
/* Weights derived from the parameters alone ([attn_h; gru_2.w_hh] stacked and transposed, gru_1.w_hh^T, both encoder w_hh^T;
 * until round 4 also gru_2.w_ih . context2hid, which the training step no longer reads): per optimiser step, not per training step.  with_fp16: also the fp16 copies of the
 * recurrent matrices the 2-byte storage mode reads (vag_step_cfg.storage = 1; H % 8 == 0). */
int64_t vag_derived_floats(int64_t H);
int vag_derive_weights(vag_dec_w w, const float* enc_whh_fw, const float* enc_whh_bw, int64_t H, int with_fp16,
                       float* derived, vag_stream_t stream);

/* ---- persistent recurrences (round 3, persist.hip) -------------------------------------------------------- */
/* The teacher-forced decoder recurrence (every step's gru_1 cell, attention query / scores / softmax, projected context and
 * gru_2 cell: layers/NMT_Decoder.py:121-129 x models/...V11.py:138-146) as ONE launch: recurrent weights in registers as
 * bf16x3 planes, the attention keys of a row tile in LDS, four workgroup-to-workgroup exchanges per step (write-through
 * stores + counters + sc1 loads).  vag_cgru_attn_decode_seq_fwd uses it whenever vag_recurrence_supported(1, ...) says so
 * (H = 512, B <= 64, keys fit the LDS); this entry point runs it alone (bench.py times it; parity: tests/test_gpu_round3.py).
 * kind: 0 = the bi-GRU encoder kernels (H in {256, 512, 1024}, 2 * ceil(B/16) * H/16 workgroups <= CUs), 1 = the decoder.
 * 2 = the decoder's one-launch BACKWARD: kind 1 and its own LDS carve-up (keys, transposed context projections and one
 * attn_h^T slice of a row tile) fitting as well, which ends at a smaller Ts than the forward's at H = 512.
 * xp1 (Tt,B,3H) = W_ih1 e_t + b_ih1; wcat (C+3H,H) = [attn_h; gru_2.w_hh], bcat (C+3H) = [0; gru_2.b_hh]; encwp (B,Ts,3H) =
 * (gru_2.w_ih context2hid) enc; outputs as vag_cgru_attn_decode_seq_fwd saves them: h1 (Tt,B,H), g1 / g2 (Tt,4,B,H),
 * qhp (Tt,B,C+3H), alpha (Tt,B,Ts), h2_all (Tt,B,H); psc (Tt,4,B,Ts) floats (the score accumulators, four copies) and sync (vag_recurrence_sync_words 32-bit
 * words) are scratch.
 * The hand-off mark: the one-launch decoder stores every h1 and h2 with the lowest significand bit forced to 1 (a consumer tells a
 * written word from an unwritten one by it), so wherever that kernel runs -- vag_recurrence_supported(1, ...) holds, the option
 * "persistent" is 1 (its default), storage is fp32 (not the 2-byte mode) and the call is teacher-forced -- the hidden states a caller
 * reads from h2_all (and h1 in the workspace) differ from the launch chain's by at most one unit in the last place, |h| 2^-23, each. */
int vag_recurrence_supported(int kind, int64_t B, int64_t Ts, int64_t Tt, int64_t H);
/* The persistent kernels wait on each other inside one launch, which needs every workgroup resident at once (one per CU;
 * vag_recurrence_supported checks the CU count).  Their waits are bounded: on a device where that does not hold they give
 * up after ~1 s instead of hanging, the launch's results are then void -- and never applied: the give-up sets the launch's guard
 * flag (vag_step_cfg.guard, VAG_ADAM_SCRATCH_GUARD_OFFSET), which vag_clip_adam_flat reads on the device (the optimiser step is
 * skipped, see VAG_ADAM_SCRATCH_SKIPPED_OFFSET) and which
 * the last launch of vag_train_step's backward turns into a non-finite gradient entry, so that every replica of a
 * data-parallel run skips the same step after the all-reduce.  This returns how many waits gave up PROCESS-WIDE since the last
 * call (0 in a healthy run; every driver's and every unguarded launch's) and resets the count; it synchronises the device --
 * call it at checkpoints, not per step.
 * vag_set_option("persist_spin_limit", n): polls before a wait gives up (0 = default 2^19; tests force a give-up with 1). */
int vag_persistent_timeouts(void);
/* Test probe of the attention energies' hoisted form (the one-launch decoder kernels and the attention's post-pass keep exp(2 pe)
 * and exp(2 q) and take one reciprocal per energy): out[i] = 1 - 2 / (E(a[i]) E(b[i]) + 1), E(x) = exp(2x) with a compensated
 * argument, on the device's own exponential and reciprocal.  Within 2^-20 of tanh(a[i] + b[i]) for |a|, |b| <= 39; operands beyond
 * that are clamped (the saturated regime), the result is finite and in [-1, 1] for every input.  n device floats each. */
int vag_attn_energy_probe(const float* a, const float* b, int64_t n, float* out, vag_stream_t stream);
/* Operators called one by one (the module API under torch.autograd, decoding) have no vag_step_cfg: this sets the guard pair
 * (see vag_step_cfg.guard) of every persistent launch the CALLING THREAD enqueues until changed; NULL = the process-wide pair. */
int vag_set_operator_guard(void* guard);
/* Measurement: with vag_set_option("persist_timing", 1) every EAGER launch (not inside a stream capture) of a recurrence
 * kernel is bracketed by HIP events on its stream.  This returns the accumulated kernel time and launch count of one kind
 * (0 encoder forward, 1 decoder forward, 2 encoder backward, 3 decoder backward) since the last call and resets them; it
 * waits for the last bracketed launch.  bench.py derives the per-family roofline rows from it. */
int vag_recurrence_time(int kind, double* ms_total, int* launches);
/* Host-only (no device is touched): the plan the library makes for one grouped launch of n (<= 12) large products C_i (M_i x
 * N_i) over K_i -- products an operator issues between its group brackets go out as ONE grid per operand layout.  The chip
 * runs 512 blocks of 128 x 128 at a time and hands them out in index order; the plan is split[i] = number of K slices of
 * product i (accumulate[i] != 0: the slices add into C; 0: C is overwritten, slicing costs a fill launch) and order[] = the
 * products sorted by slice length, longest first, chosen by simulating that schedule.  Exposed for tests and tuning. */
int vag_gemm_group_plan(int n, const int64_t* M, const int64_t* N, const int64_t* K, const int* accumulate, int* split, int* order);
/* Host-only (no device is touched): the plan the library makes for ONE product C (M x N) over K that is launched at once and has
 * no split-K slab scratch at hand, as vag_gemm_f32 is.  a_kc / b_kc: A / B is k-contiguous; vec: both operands 16-byte aligned with
 * leading dimensions % 4 == 0; rowsum: A's row sums are wanted (needs a_kc == 0); planes: bf16 planes per operand (3, 2, 1, 11 = one
 * fp16 plane), 0 = the calling thread's operator context.  The options of vag_set_option apply as they do to a launch.
 * plan[0] = kernel family (below); plan[1], plan[2] = tile and split-K the cost model chose (a forced pair applied);
 * plan[3], plan[4] = k-slices launched and the k-length of a slice (a multiple of 32); plan[5] = 1: the kernel takes the row sums
 * along, 0: they are not wanted or need a column-sum launch.  Exposed for tests and tuning. */
enum { VAG_GEMM_TILED64 = 0,        /* exact f32-input MFMA, 64 x 64 tiles */
       VAG_GEMM_TILED128_F32 = 1,   /* the same on 128 x 128 tiles (option "gemm_f32mfma") */
       VAG_GEMM_SPLIT128 = 2,       /* bf16 planes, 128 x 128 tiles */
       VAG_GEMM_BIG256 = 3 };       /* one plane, 256 x 256 tiles */
int vag_gemm_plan(int64_t M, int64_t N, int64_t K, int a_kc, int b_kc, int vec, float beta, int act, int c_half, int a_bf16,
                  int rowsum, int planes, int* plan);
int64_t vag_recurrence_sync_words(int kind, int64_t B, int64_t T);
int vag_cgru_recurrence_fwd(const float* pe, const float* mask, const float* h0, const float* xp1, vag_dec_w w, const float* wcat,
                            const float* bcat, const float* encwp, int64_t B, int64_t Ts, int64_t Tt, int64_t H, float* h1,
                            float* g1, float* qhp, float* alpha, float* h2_all, float* g2, float* psc, void* sync,
                            vag_stream_t stream);

/* ---- lexical shortlists: a per-batch compact target vocabulary (csrc/shortlist.hip, vagnmt_hip.shortlist) -----------------
 * A search takes everything vocabulary-sized from three tensors of the decoder (embedding.weight, out.weight, out.bias).  These
 * calls choose, per batch, the target words worth scoring and cut the three tensors down to them; every decoding kernel then
 * runs unchanged on the compact vocabulary.  Compact ids ascend with full ids, so "word ascending" tie-breaks choose the same
 * word in either numbering, and ids 0 .. 3 (PAD, UNK, SOS, EOS) keep their values when `always` holds them.
 *
 * vag_shortlist_supported: 1 for 8 <= V <= 131072, 1 <= Vs, 1 <= K <= 256, 8 <= cap <= V, else 0.  A pure host call.
 *
 * vag_shortlist_select: src (B, Ts) int64 source ids, lengths (B) int32, lex (Vs, K) int32 -- row s: the target ids of the K best
 * translations of source word s, best first, padded with -1 -- and always (A) int32.  The `always` ids are marked first; then
 * the lexicon's ranks r = 0 .. best-1 one after another, rank r of every source word at a position t < lengths[b].  A rank whose
 * NEW words would push the number of chosen words over cap is not applied, and neither are later ranks: the result does not
 * depend on thread order.  Source ids outside [0, Vs) and target ids outside [0, V) are ignored; duplicates are harmless.
 * Writes ids (cap): the chosen ids ascending, then -1; n[0]: their number; rank_used[0]: the ranks applied; full2short (V): the
 * compact id of every full id, -1 for a word not chosen.  One launch of one workgroup, a bitmap over V in LDS, integer LDS
 * atomics only; it can be captured.  -EINVAL: a NULL pointer (always may be NULL with A = 0), sizes vag_shortlist_supported
 * refuses, B < 1, Ts < 1, B Ts >= 2^31, best outside [0, K], A outside [0, cap].
 *
 * vag_shortlist_gather: out (cap, W) contiguous; row j < n[0] is row ids[j] of src (V, W) with row stride ld, bit for bit, rows
 * n[0] .. cap-1 (and a row whose id lies outside [0, V)) hold `pad` -- written at every call.  src is only read.  16-byte
 * accesses when W and ld are multiples of 4 and both addresses are 16-byte aligned, 4-byte ones otherwise.  -EINVAL: a NULL
 * pointer, V or cap outside [1, 131072], W < 1, ld < W.
 *
 * vag_shortlist_map: out[i] = table[x[i]] for N int64 words (out may be x).  to_short = 0: table = ids (len = cap), compact ->
 * full; to_short = 1: table = full2short (len = V), full -> compact.  A word outside [0, len) or with a negative entry becomes
 * UNK = 1; with to_short = 1 each such word also adds 1 to absent[0] (integer atomics; absent may be NULL).  -EINVAL: NULL table,
 * len outside [1, 131072], N < 0, NULL x or out with N > 0. */
int vag_shortlist_supported(int64_t V, int64_t Vs, int64_t K, int64_t cap);
int vag_shortlist_select(const int64_t* src, const int32_t* lengths, int64_t B, int64_t Ts, const int32_t* lex, int64_t Vs,
                         int64_t K, int64_t best, const int32_t* always, int64_t A, int64_t V, int64_t cap, int32_t* ids,
                         int32_t* n, int32_t* rank_used, int32_t* full2short, vag_stream_t stream);
int vag_shortlist_gather(const int32_t* ids, const int32_t* n, int64_t cap, const float* src, int64_t V, int64_t W, int64_t ld,
                         float pad, float* out, vag_stream_t stream);
int vag_shortlist_map(const int64_t* x, int64_t N, const int32_t* table, int64_t len, int to_short, int64_t* out, int32_t* absent,
                      vag_stream_t stream);

/* ---- data-parallel gradient exchange over RCCL (SURVEY 8b "C1", 8e) -------------------------------------------------------
 * One process per GPU, one communicator per process.  Rank 0 draws an id (128 opaque bytes) and ships it to the other
 * ranks by any channel (the Python host uses the torch.distributed store); every rank then calls vag_comm_init with the
 * same id -- a collective that binds the communicator to the CURRENT device.  vag_comm_allreduce sums `n` floats in place
 * across the ranks (ncclAllReduce, ncclSum -- the caller scales by 1/N; vag_clip_adam_flat's grad_scale does) on `stream`;
 * like every call here it only enqueues, so it can be captured with the step's kernels.  The reference has no
 * distributed backend (nmt_multimodal_beam_DE.py:277-282 leaves nn.DataParallel commented out); this is the exchange
 * SURVEY 8e adds.  librccl is loaded on the first vag_comm_* call (-38 = ENOSYS if it cannot be); RCCL's own errors come
 * back as 10000 + ncclResult_t. */
#define VAG_COMM_ID_BYTES 128
typedef struct vag_comm_s* vag_comm_t;
int vag_comm_unique_id(void* id);
int vag_comm_init(vag_comm_t* comm, int nranks, int rank, const void* id);
int vag_comm_allreduce(vag_comm_t comm, float* buf, int64_t n, vag_stream_t stream);
int vag_comm_size(vag_comm_t comm);
int vag_comm_destroy(vag_comm_t comm);

/* ---- dropout helpers ---------------------------------------------------------------------------------- */
/* which: 1 encoder-embedding (Ts,B,E), 2 encoder-context (B,Ts,2H), 3 decoder-output (Tt,B,E).  out[i] holds the MULTIPLIER of
 * element i, 0 for a dropped element and 1 / (1 - p) for a kept one (not a 0/1 keep flag); 1 everywhere for rng == NULL or p == 0. */
int vag_dropout_mask(const uint64_t* rng, int which, int64_t n, float p, float* out, vag_stream_t stream);
int vag_rng_advance(uint64_t* rng, vag_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VAG_NMT_H */
