// Internal launcher prototypes (one per kernel family).  Not part of the C ABI.
#pragma once
#include "common.h"
#include "call_ctx.h"
#include "../../include/vag_nmt.h"

// ---------------- workspace layouts (host) ----------------
// Every caller-owned workspace is carved into regions of 64-float (256-byte) granules by ONE carver: a layout function takes its
// regions in order, and called on a NULL base it yields NULL pointers and the same offsets -- that is how the *_floats queries
// of the ABI get their totals.
static inline int64_t round64(int64_t n) { return (n + 63) & ~63ll; }
struct WsCarver {
    float* base;
    int64_t off = 0;            // floats taken so far: the layout's total once every region is taken
    explicit WsCarver(float* b) : base(b) {}
    float* take(int64_t n) {
        float* q = base ? base + off : nullptr;
        off += round64(n);
        return q;
    }
    template <class T> T* take_as(int64_t n) {         // n elements of T (unsigned / int64_t / vag_half: whole floats, rounded up)
        return reinterpret_cast<T*>(take((n * (int64_t)sizeof(T) + 3) / 4));
    }
};
// Tables of the free-running recurrence kernel and of the hoisted decoding step (persist.hip has the definition):
// [embp (V,3H) emb W_ih1^T + b_ih1 | embw3 (V,E) emb W3^T | encw2 (B,Ts,E) enc W2^T | cand (Tt,B,64) 8-byte arg-max candidates].
// token_only: the first two regions alone, which are the decoding step's tables (vag_cgru_decode_tables); encw2 / cand stay NULL.
struct DecTables {
    float *embp, *embw3, *encw2;
    unsigned long long* cand;
    int64_t total;
};
DecTables vag_dec_tables(float* base, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V, bool token_only = false);

// ---------------- elem.hip ----------------
// out[(t*B+b), :] = W[idx[b*isb + t*ist], :] * dropout
// mask_out (optional, indexed like idx): 1 where the index is not the padding index 0
int vag_embed_gather_launch(const int64_t* idx, int64_t ist, int64_t isb, int64_t T, int64_t B, const float* W,
                            int64_t E, float* out, const uint64_t* rng, int sid, float p, hipStream_t s,
                            float* mask_out = nullptr);
// gW[idx, :] += g[(t*B+b), :] * dropout, skipping idx == 0 (padding_idx)
int vag_embed_scatter_launch(const int64_t* idx, int64_t ist, int64_t isb, int64_t T, int64_t B, const float* g,
                             int64_t E, float* gW, const uint64_t* rng, int sid, float p, hipStream_t s,
                             const unsigned* poison = nullptr);   // poison: see embed_scatter_kernel

struct GruBwdSide {
    const float* dh_carry;   // (M,H) gradient arriving from the later time step, or NULL
    const float* dh_add;     // optional extra gradient source, element (m,j) at dh_add[m*ld_add + j]
    int64_t drop_idx0;       // dropout index of dh_add element (m,j) = m*ld_add + drop_idx0 + j
    const float* save;       // [4][M][H] r,z,n,hn from the forward step
    const float* hprev;      // (M,H) ld = ldh
    float* dgi;              // (M,3H) ld = ldgi
    float* dgh;              // (M,3H) ld = ldgh
    float* dh_prev;          // (M,H): z * dh (the W_hh^T dgh part is added by the following GEMM)
    int t;
};
struct GruBwdArgs {
    GruBwdSide s[2];
    int64_t ld_add, ldh, ldgi, ldgh;
    int M, H;
    const int* lengths;
    const uint64_t* rng; int sid; float p;   // dropout applied to dh_add (encoder context dropout)
};
int vag_gru_bwd_elem_launch(const GruBwdArgs& a, int nz, hipStream_t s);

// dx = dy * dropout(i) * (1 - t*t)   (in place allowed).  With dropout, y is the post-dropout value t*mul;
// t is recovered from it (dropped elements have zero gradient).
int vag_tanh_bwd_launch(const float* y, const float* dy, float* dx, int64_t n, const uint64_t* rng, int sid, float p,
                        hipStream_t s, int64_t idx0 = 0);      // idx0: dropout index of element 0 (a row chunk of a larger array)
// x[i] *= dropout(idx0 + i)
int vag_dropout_apply_launch(float* x, int64_t n, int64_t idx0, const uint64_t* rng, int sid, float p, hipStream_t s);
int vag_tanh_dropout_launch(float* x, int64_t n, int64_t idx0, const uint64_t* rng, int sid, float p, hipStream_t s);
int vag_dropout_mask_launch(const uint64_t* rng, int sid, int64_t n, float p, float* out, hipStream_t s);
// y (+)= a*x
int vag_axpy_launch(float a, const float* x, float* y, int64_t n, int accumulate, hipStream_t s);
// mask[b,t] = src[b,t] != 0
int vag_src_mask_launch(const int64_t* src, int64_t n, float* mask, hipStream_t s);
// xmix[b,c] = split*ctx[b,c] + (1-split) * sum_t enc[b,t,c] / sum_t mask[b,t]   (ctx NULL -> split treated as 0)
int vag_meanpool_mix_launch(const float* enc, const float* mask, const float* ctx, float split, int64_t B, int64_t Ts,
                            int64_t C, float* xmix, hipStream_t s);
// d_enc[b,t,c] (+)= coef * dx[b,c] / sum_t mask[b,t]
int vag_meanpool_bwd_launch(const float* mask, const float* dx, float coef, int64_t B, int64_t Ts, int64_t C,
                            float* d_enc, int accumulate, hipStream_t s);
int vag_rng_advance_launch(uint64_t* rng, hipStream_t s);
// out[i*ldo + j] = in[i*ldi + j] for a (rows x cols) block
int vag_copy2d_launch(const float* in, int64_t ldi, float* out, int64_t ldo, int64_t rows, int64_t cols, hipStream_t s);

int vag_gather_rows_i64_launch(const int64_t* in, int64_t ld, const int64_t* idx, int64_t rows, int64_t w, int64_t* out,
                               hipStream_t s);

// ---------------- mrt.hip ----------------
int vag_mrt_cfg_ok(int64_t B, int64_t N, float alpha, float scale);      // the limits of vag_mrt_weights on (B, N, alpha, scale): host only
// losses != NULL (the fused step): also {loss, loss_mt, loss_vse} = {w_mt risk, risk, 0}, the ring slot and the execution counter
int vag_mrt_weights_launch(const float* nll, const float* cost, const float* valid, int64_t B, int64_t Tt, int64_t N, float alpha,
                           float scale, float* inv_cnt, float* q, float* risk, float* losses, float w_mt, int ring, hipStream_t s);
int vag_mrt_pack_launch(const int64_t* cand, int64_t G, int64_t Nc, int64_t L, const int64_t* gold, int64_t Tg, int include_gold,
                        int64_t* tgt, int64_t Tt, float* valid, hipStream_t s);

// several small fills (kind 0) / copies (1) / transposes (2) of (rows x cols) fp32 matrices in one launch
struct VagJob { const float* src; float* dst; int64_t rows, cols, ld_src, ld_dst; int kind; };
constexpr int VAG_MAXJOBS = 12;
struct VagJobs { VagJob j[VAG_MAXJOBS]; int start[VAG_MAXJOBS + 1]; int n; };
int vag_jobs_launch(const VagJob* jobs, int n, hipStream_t s);

int vag_copy4_launch(const void* const* src, void* const* dst, const int64_t* bytes, int n, hipStream_t s);

// ---------------- attn.hip ----------------
#ifndef VAG_POST_SC
#define VAG_POST_SC 8          // source positions per attn_post_bwd block
#endif
static inline int64_t VAG_POST_CHUNKS(int64_t Ts) { return (Ts + VAG_POST_SC - 1) / VAG_POST_SC; }
// mode 0: scores[n,s] = sum_c v[c] tanh(pe[b,s,c] + q[n,c]); mode 1: scores[n,s] = sum_c q[n,c] * pe[b,s,c].
// b = n / rps.  mask (Bsrc,Ts) float or NULL: masked positions get -inf.
// q row stride ldq (>= C).
int vag_attn_scores_launch(int mode, const float* pe, const float* q, int64_t ldq, const float* v, const float* mask,
                           int64_t N, int64_t rps, int64_t Ts, int64_t C, float* scores, hipStream_t s);
int vag_attn_scores_ex_launch(int mode, const float* pe, const float* q, int64_t ldq, const float* v, const float* mask,
                              int64_t N, int64_t rps, int64_t rows_mod, int64_t Ts, int64_t C, const float* addend,
                              float* scores, hipStream_t s);
int vag_attn_ctx_gru_launch(const float* scores, const float* encwp, int64_t N, int64_t rps, int64_t Ts, int64_t H,
                            const float* b_ih, const float* hp, int64_t ldhp, const float* hprev, float* alpha, float* hout,
                            float* save, hipStream_t s, bool x16 = false,       // x16: encwp is fp16
                            const float* x2 = nullptr, int64_t W2 = 0, float* out2 = nullptr);     // out2 (N,W2) = alpha . x2 (B,Ts,W2)
int vag_attn_wsum_launch(int over_src, const float* a, const float* x, int64_t B, int64_t Ts, int64_t T, int64_t W, float* out,
                         hipStream_t s);
// softmax=1: alpha[n,:] = softmax(scores[n,:]) (written to alpha), ctx[n,c] = sum_s alpha[n,s] enc[b,s,c]
// softmax=0: weights = scores as given (alpha not written)
int vag_attn_ctx_launch(int softmax, const float* scores, const float* enc, int64_t N, int64_t rps, int64_t Ts,
                        int64_t C, float* alpha, float* ctx, hipStream_t s);
// dscore[n,s] = alpha[n,s] * (dalpha[n,s] - sum_s' alpha dalpha)
int vag_softmax_bwd_launch(const float* alpha, const float* dalpha, int64_t N, int64_t Ts, float* dscore, hipStream_t s);
// dq[n,c] = sum_s dscore[n,s] * v[c] * (1 - tanh^2(pe[n,s,c] + q[n,c]))      (training: rps = 1)
// alpha/dalpha given: dscore is first computed (softmax backward) and stored; NULL: dscore is an input.
int vag_attn_dq_launch(const float* pe, const float* q, int64_t ldq, const float* v, const float* alpha,
                       const float* dalpha, float* dscore, int64_t N, int64_t Ts, int64_t C, float* dq, int64_t lddq,
                       hipStream_t s, bool x16 = false);                       // x16: pe is fp16
// After the time loop: d_pe[b,s,c] = v[c] sum_t ds[t,b,s] (1-th^2);  dvp[(z*B+b),c] = sum_{t, s in chunk z} ds*th
// (VAG_POST_CHUNKS(Ts) = ceil(Ts/8) chunk rows per batch row; column-sum all rows for dv);
// d_enc[b,s,c] (+)= sum_t alpha[t,b,s] dc[t,b,c]   (skipped when dc == NULL)
int vag_attn_post_bwd_launch(const float* pe, const float* q_all, int64_t ldq, const float* v, const float* ds_all,
                             const float* alpha_all, const float* dc_all, int64_t B, int64_t Ts, int64_t Tt,
                             int64_t C, float* d_pe, float* dvp, float* d_enc, int accumulate_enc, hipStream_t s,
                             bool x16 = false);                                // x16: pe is fp16
// out[i] = vag_energy_tanh(vag_energy_exp(a[i]), vag_energy_exp(b[i])) (common.h): the hoisted form of tanh(a + b), for the tests
int vag_attn_energy_probe_launch(const float* a, const float* b, int64_t n, float* out, hipStream_t s);
// out[b,t,c] (+)= a1[b,t]*x1[b,c] + a2[b,t]*x2[b,c]
int vag_outer2_launch(const float* a1, const float* x1, const float* a2, const float* x2, int64_t B, int64_t Ts,
                      int64_t C, float* out, int accumulate, hipStream_t s);

// ---------------- head.hip ----------------
// Label smoothing eps of the translation loss (vag_nmt.h: vag_head_ce_seq_fwd_ls): 0 <= eps < 1; NaN fails both comparisons.
// eps == 0 launches the LS = false instantiations (the kernels as they were before the option), eps > 0 the LS = true ones.
// eps has no default anywhere: a call site that computes no loss (no target) says 0.f itself, one that does cannot forget it.
inline bool vag_label_smoothing_ok(float eps) { return eps >= 0.f && eps < 1.f; }
// per row: lse, nll = -w[tgt]*(x[tgt]-lse) (tgt NULL: skipped), argmax (may be NULL), logp_out (may be NULL)
// eps > 0 (needs tgt): nll = w[tgt]*(lse - (1-eps)*x[tgt] - eps/V * sum_{j<V} x[j])
// row r = t*B + b;  tgt index = tgt[b*Tt + t]
int vag_lse_nll_launch(const float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B,
                       int64_t Tt, const float* vw, float* lse, float* nll, int64_t* argmax, int64_t argmax_stride,
                       float* logp_out, int64_t ldlp, hipStream_t s, float eps);
int vag_inv_cnt_launch(const int64_t* tgt, int64_t B, int64_t Tt, float* inv_cnt, hipStream_t s);
// The loss reduction, the one launch site of loss_mt_kernel: loss[0] = loss_mt (the stand-alone form: t.losses NULL), or t.losses[1] =
// loss_mt and the mixed total t.losses[0] = w_mt*loss_mt + w_vse*losses[2] (V11.py:166) with the ring slot t.ring asks for.  The
// second form is held back instead while VagCallCtx::loss_defer is on (vag_loss_defer_flush, or the next ce_bwd_colsum launch, does it).
int vag_loss_mt_launch(const LossTask& t, float* loss, hipStream_t s);
// in place: logits[r,j] = d_loss * inv_cnt[b]/B * w[tgt] * (softmax_j - (1-eps)*[j==tgt] - eps/V); pad columns [V,ldl) = 0
int vag_ce_bwd_launch(float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                      const float* vw, const float* lse, const float* inv_cnt, const float* d_loss, hipStream_t s,
                      float eps);
int vag_ce_bwd_colsum_launch(float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                             const float* vw, const float* lse, const float* inv_cnt, const float* d_loss, float* g_bias,
                             hipStream_t s, void* out16, float eps);

int vag_logsoftmax_bwd_launch(const float* logp, int64_t ldlp, float* d, int64_t ldd, int64_t rows, int64_t V,
                              hipStream_t s);

// ---------------- distill.hip ----------------
// Word-level distillation (vag_nmt.h: vag_kd_head_ce_seq_fwd): per row K distinct words idx (rows, K) with probabilities q (rows, K),
// sum_k q_k = 1, mixed into the loss with weight lambda.  1 <= K <= min(64, V), 0 < lambda <= 1; NaN fails both comparisons.
inline bool vag_kd_ok(int64_t K, float lambda, int64_t V) { return K >= 1 && K <= 64 && K <= V && lambda > 0.f && lambda <= 1.f; }
// After vag_lse_nll_launch on the same rows (a chunk of whole time steps: tgt, lse, nll, idx, q offset to it by the caller), the
// logits still in place: nll[row] = w[y] * (lse - (1 - lambda) x[y] - lambda sum_k q_k x[idx_k]), overwriting the plain value.  One
// wave per row, K + 1 gathers; the sum over k runs in one fixed tree, so the value is reproducible.
int vag_kd_nll_launch(const float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                      const float* vw, const float* lse, const int32_t* idx, const float* q, int64_t K, float lambda, float* nll,
                      hipStream_t s);
// After vag_ce_bwd_launch / vag_ce_bwd_colsum_launch (eps = 0, fp32 d(logits) in place) on the same rows and BEFORE anything reads
// d(logits): read-modify-write of K + 1 entries per row, + coef lambda at y and - coef lambda q_k at idx_k (one combined update
// where idx_k == y), coef as in ce_bwd_kernel.  g_bias (may be NULL): the same amounts by atomicAdd -- the sum g(out.bias) already
// meets in fp32 atomics (ce_bwd_colsum_kernel's column sums), so this adds no new source of run-to-run rounding differences.
// Rows with coef == 0 (PAD) write nothing; the padding columns [V, ldl) are never touched.
int vag_kd_dlogits_launch(float* dlogits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                          const float* vw, const float* inv_cnt, const float* d_loss, const int32_t* idx, const float* q, int64_t K,
                          float lambda, float* g_bias, hipStream_t s);

// ---------------- conf.hip ----------------
// Word-level confidence of forced decoding (vag_nmt.h: vag_token_conf): the row kernel, then the sentence kernel.
int vag_token_conf_launch(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M, const int64_t* tgt,
                          int64_t B, int64_t Tt, int64_t V, float* token_logp, float* entropy, int32_t* rank, int32_t* top,
                          float* top_logp, float* sent, hipStream_t s);

// ---------------- rdrop.hip ----------------
// R-Drop (vag_nmt.h: vag_rdrop_head_ce_seq_fwd): B even, rows 2 p and 2 p + 1 hold one sentence under two dropout masks.  alpha > 0
// and finite; NaN fails both comparisons.
inline bool vag_rdrop_ok(float alpha) { return alpha > 0.f && alpha < INFINITY; }
// After vag_lse_nll_launch on the same rows (a chunk of whole time steps: tgt, lse, kl, nll offset to it by the caller), the logits
// still in place: kl[r] = sum_j p_r[j] (lp_r[j] - lp_twin[j]) for both rows of every pair, nll[r] += w[y_r] (alpha / 4) (kl[r] +
// kl[twin]).  One workgroup per pair, one pass over both rows, a fixed summation order (reproducible); [V, ldl) is never read.
int vag_rdrop_pair_launch(const float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                          const float* vw, const float* lse, float alpha, float* kl, float* nll, hipStream_t s);
// In place of vag_ce_bwd_colsum_launch (fp32 d(logits) in place, no held-back loss reduction rides in it): the smoothed gradient plus
// (alpha / 4) (coef_r + coef_twin) (p_r ((lp_r - lp_twin) - kl[r]) + p_r - p_twin), both rows of a pair read before either is
// written; g_bias receives the column sums, reduced over a strip of rows before the atomics.  Pairs whose coefficients sum to 0
// and the padding columns [V, ldl) are written as zeros.
int vag_rdrop_bwd_colsum_launch(float* logits, int64_t ldl, int64_t rows, int64_t V, const int64_t* tgt, int64_t B, int64_t Tt,
                                const float* vw, const float* lse, const float* kl, const float* inv_cnt, const float* d_loss,
                                float alpha, float* g_bias, hipStream_t s, float eps);

// ---------------- vse.hip ----------------
int vag_l2norm_fwd_launch(const float* y, int64_t B, int64_t S, float* nrm, float* out, hipStream_t s);
// dy = l2norm backward of d_out, then (act) * (1 - y^2); written to dy (may alias d_out)
int vag_l2norm_bwd_launch(const float* y, const float* nrm, const float* out, const float* d_out, int64_t B, int64_t S,
                          int act, float* dy, hipStream_t s);
// kind | 2 (vag_nmt.h: vag_rank_loss_fwd): rows 2 p, 2 p + 1 are twins, neither a positive nor a negative of each other.  scale: a
// host factor on the loss and on G (the R-Drop step's 1/4)
int vag_rank_loss_launch(const float* scores, int64_t B, float margin, int kind, float* G, float* loss, hipStream_t s,
                         const float* g_scale = nullptr, float scale = 1.f);
int vag_retrieval_rank_launch(const float* scores, int64_t N, int* ranks, hipStream_t s);
// x[i] *= *scalar
int vag_scale_by_dev_launch(float* x, int64_t n, const float* scalar, hipStream_t s);

// ---------------- optim.hip ----------------
int vag_clip_adam_shard_launch(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                               const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1, float beta2,
                               float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch, const float* lr_dev,
                               int64_t lo, int64_t hi, int phase, double* sumsq, hipStream_t s);
int vag_clip_adam_launch(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                         const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1,
                         float beta2, float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch, const float* lr_dev,
                         hipStream_t s);
int vag_clip_adam_ema_launch(float* p, float* g, float* m, float* v, int64_t n, int nseg, const int64_t* seg_off,
                             const float* seg_lr, const float* seg_wd, float clip, float grad_scale, float beta1,
                             float beta2, float eps, int zero_grad, int32_t* step, float* norm_out, void* scratch,
                             const float* lr_dev, float* ema, float ema_decay, int ema_warmup, hipStream_t s);
int vag_swap_flat_launch(float* a, float* b, int64_t n, hipStream_t s);

// ---------------- persist.hip: whole recurrences in one launch ----------------
bool vag_enc_persistent_ok(int64_t B, int64_t Ts, int64_t H);
int64_t vag_enc_persistent_sync_words(int64_t B, int64_t Ts);
int vag_enc_fwd_persistent_launch(const float* xp, const float* w_fw, const float* w_bw, const float* b_fw, const float* b_bw,
                                  const int* lengths, float* hst, float* gates, float* enc, float* planes, int64_t planes_floats,
                                  unsigned* sync, const uint64_t* rng, float p_ctx, int64_t B, int64_t Ts, int64_t H, hipStream_t s);
int64_t vag_enc_fwd_planes_floats(int64_t B, int64_t Ts, int64_t H);     // the forward's state rows as bf16 planes (persist.hip)
int vag_enc_bwd_persistent_launch(const float* whhT, const float* d_enc, const float* gates, const float* hst, const int* lengths,
                                  const uint64_t* rng, float p_ctx, float* d_xp, float* dgh, float* planes, unsigned* sync, int64_t B,
                                  int64_t Ts, int64_t H, hipStream_t s);
int64_t vag_enc_bwd_planes_floats(int64_t B, int64_t Ts, int64_t H);     // the backward recurrences' hand-off rows as bf16 planes (persist.hip)
int64_t vag_dec_bwd_planes_floats(int64_t B, int64_t Tt, int64_t H);
bool vag_enc_wide16_ok(int64_t B, int64_t Ts, int64_t H);
int vag_enc_fwd_wide16_launch(const float* xp, const vag_half* w16_fw, const vag_half* w16_bw, const float* b_fw, const float* b_bw,
                              const int* lengths, float* hst, float* gates, float* enc, vag_half* hx, unsigned* sync, const uint64_t* rng,
                              float p_ctx, int64_t B, int64_t Ts, int64_t H, hipStream_t s);
int vag_enc_bwd_wide16_launch(const vag_half* wt16, const float* d_enc, const float* gates, const float* hst, const int* lengths,
                              const uint64_t* rng, float p_ctx, float* d_xp, float* dgh, vag_half* gx, unsigned* sync, int64_t B,
                              int64_t Ts, int64_t H, hipStream_t s);
int vag_gemm_group_plan_host(int n, const int64_t* M, const int64_t* N, const int64_t* K, const int* accumulate, int* split,
                             int* order);
int vag_gemm_plan_host(int64_t M, int64_t N, int64_t K, int a_kc, int b_kc, int vec, float beta, int act, int c_half, int a_bf16,
                       int rowsum, int planes, int* plan);
int vag_persistent_timeouts_read(void);
unsigned* vag_persist_guard(void);           // {void flag, give-up count} pair of the launches the calling thread enqueues: the context's, else the process-wide pair (persist.hip)
int vag_persistent_time_read(int kind, double* ms_total, int* launches);
bool vag_dec_bwd_persistent_ok(int64_t B, int64_t Ts, int64_t Tt, int64_t H);
int vag_dec_bwd_persistent_launch(const float* pe, const float* encwp, const float* v, const float* wcatT, const float* whh1T,
                                  const float* h0, const float* h2_all, const float* h1, const float* g1, const float* g2,
                                  const float* qhp, const float* alpha, const float* d_h2_all, const float* dah, float* dgi2,
                                  float* dqgh, float* ds, float* dgi1, float* dgh1, float* d_h0, float* dal, float* planes,
                                  int64_t planes_floats, unsigned* sync, int64_t B, int64_t Ts, int64_t Tt, int64_t H, hipStream_t s);
int vag_attn_dot_row_launch(bool bwd, const float* x, const float* q, int64_t ldq, const float* mask, const float* alpha, int64_t B,
                            int64_t Ts, int64_t C, float* wout, float* sum, hipStream_t s);      // attn.hip: one launch per dot attention
int vag_rank_bwd_launch(const float* G, const float* im, const float* sv, const float* d_loss, int64_t B, int64_t S, float* d_im,
                        float* d_s, hipStream_t s);       // vse.hip: d_im = G s and d_s = G^T im (x *d_loss) in one launch, B <= 128
int vag_attn_wsum_pair_launch(const float* a, const float* y, int64_t Wy, float* out_src, const float* x, int64_t Wx, float* out_time,
                              int64_t B, int64_t Ts, int64_t T, hipStream_t s);        // attn.hip: sum over t of a y and sum over s of a x, one grid
int vag_loss_defer_flush();                 // head.hip: launch a held-back loss reduction (VagCallCtx::loss_defer) now if no ce_bwd_colsum launch took it
bool vag_attn_row_gru_ok(int64_t N, int64_t Ts, int64_t H, int64_t W2);       // attn.hip: a decoding step's attention + gru_2 + W2 c in one launch
int vag_attn_row_gru_launch(const float* pe, const float* q, int64_t ldq, const float* v, const float* mask, const float* keys,
                            const float* x2, int64_t N, int64_t rps, int64_t Ts, int64_t H, int64_t W2, const float* b_ih,
                            const float* hp, int64_t ldhp, const float* hprev, float* alpha, float* hout, float* out2, hipStream_t s);
int vag_rmw_defer_flush(hipStream_t s);    // attn.hip: the held-back accumulations (VagCallCtx::rmw) in one pass
bool vag_rmw_defer_meanpool(const float* mask, const float* dx, float coef, int64_t B, int64_t Ts, int64_t C, float* out, int accumulate);
float* vag_dec_fwd_planes_region(int64_t B, int64_t Ts, int64_t Tt, int64_t H);       // persist.hip: the decoder forward's marked planes in the caller's buffer (NULL: fp32 hand-off)
bool vag_dec_persistent_ok(int64_t B, int64_t Ts, int64_t Tt, int64_t H);
int64_t vag_dec_persistent_sync_words(int64_t B, int64_t Tt);
int vag_dec_fwd_persistent_launch(const float* pe, const float* mask, const float* h0, const float* xp1, const float* W1,
                                  const float* b1, const float* wcat, const float* bcat, const float* v, const float* encwp,
                                  const float* b_ih2, float* h1, float* g1, float* qhp, float* alpha, float* h2_all, float* g2,
                                  float* psc, unsigned* sync, int64_t B, int64_t Ts, int64_t Tt, int64_t H, hipStream_t s);
// free-running form (the kernel feeds its own arg-max back): see persist.hip
bool vag_dec_free_persistent_ok(int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, int64_t V);
int vag_dec_free_persistent_launch(const float* pe, const float* mask, const float* h0, const float* W1, const float* b1,
                                   const float* wcat, const float* bcat, const float* v, const float* encwp, const float* b_ih2,
                                   float* h1, float* g1, float* qhp, float* alpha, float* h2_all, float* g2, float* psc,
                                   unsigned* sync, const DecTables& tab, const float* hw1, const float* hb1, const float* hb2,
                                   const float* hb3, const float* out_w, const float* out_b, float* tmid, float* logits, int64_t ldl,
                                   int64_t* tok, const uint64_t* rng, float p_out, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                                   int64_t H, int64_t V, hipStream_t s);

// ---------------- beam.hip ----------------
int64_t vag_beam_scratch_bytes_impl(int64_t B, int64_t k, int64_t V);
int vag_beam_step_launch(float* logp, int64_t ldl, float* nll, int64_t* beam, int64_t di, int32_t* di_state,
                         int64_t max_len, const float* h_in, float* h_out, int64_t* tok_out, int64_t B, int64_t k,
                         int64_t V, int64_t H, int32_t* n_alive, void* scratch, hipStream_t s, const float* parts = nullptr,
                         int64_t nparts = 0, int flags = 0);
int vag_beam_finish_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                           int64_t* out, float* best, hipStream_t s);
int vag_beam_ens_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, hipStream_t s,
                             int flags = 0);
int vag_beam_finish_nbest_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                 int64_t n, int64_t* out, float* scores, hipStream_t s);
int vag_beam_finish_nbest_slots_launch(const float* nll, const int64_t* beam, int64_t max_len, int64_t steps, int64_t B, int64_t k,
                                       int64_t n, int64_t* out, float* scores, int64_t* slots, hipStream_t s);
int64_t vag_beam_div_scratch_bytes_impl(int64_t B, int64_t k, int64_t V);
int vag_beam_div_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             int64_t groups, float strength, hipStream_t s);
int64_t vag_beam_req_scratch_bytes_impl(int64_t B, int64_t k, int64_t V);
int vag_beam_req_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             const int64_t* required, int32_t* state, hipStream_t s);
int64_t vag_beam_sbs_scratch_bytes_impl(int64_t B, int64_t k, int64_t V);
int vag_beam_sbs_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             const uint64_t* rng, float* gum, hipStream_t s);
int64_t vag_beam_pen_scratch_bytes_impl(int64_t B, int64_t k, int64_t V);
int vag_beam_cover_launch(const float* const* alpha, int64_t M, const float* mask, const float* cov, const int64_t* beam, int64_t di,
                          const int32_t* di_state, int64_t max_len, int64_t B, int64_t k, int64_t Tp, float beta, float* cov_row,
                          float* cp_row, hipStream_t s);
int vag_beam_pen_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, float* nll, int64_t* beam, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t k, int64_t V, int32_t* n_alive, void* scratch, int flags,
                             int32_t* lens, const float* cp_row, float* cpen, const float* cov_row, float* cov, int64_t Tp,
                             const float* lp, const float* bonus, int stepwise, hipStream_t s);
int vag_beam_finish_pen_launch(const float* nll, const int64_t* beam, const int32_t* lens, const float* cpen, const float* lp,
                               const float* bonus, int64_t max_len, int64_t steps, int64_t B, int64_t k, int64_t n, int64_t* out,
                               float* scores, int64_t* slots, float* logp, int32_t* length, float* cp, hipStream_t s);
int vag_beam_constrain_launch(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di,
                              const int32_t* di_state, bool dev_form, int64_t max_len, int64_t B, int64_t k, int64_t V,
                              const int64_t* prefix, int64_t Lp, const int64_t* phrases, const int32_t* phrase_sent, int64_t P,
                              int64_t ngram, hipStream_t s);
// kNN-MT (knn.hip): the datastore's append, the streaming nearest-neighbour search and the mix into the members' rows
int64_t vag_knn_row_tile_host(int64_t D);
int64_t vag_knn_scratch_bytes_host(int64_t R, int64_t N, int64_t K);
int vag_knn_store_rows_launch(const float* h2, const int64_t* tgt, int64_t B, int64_t Tt, int64_t H, int64_t sent_base, int64_t cap,
                              void* keys, float* norm, int32_t* value, int32_t* sentence, int32_t* position, int32_t* count,
                              hipStream_t s);
int vag_knn_search_launch(const float* q, int64_t ldq, int64_t R, int64_t D, const void* keys, const float* norm, int64_t N, int64_t K,
                          float* out_score, int32_t* out_index, void* scratch, hipStream_t s);
int vag_knn_mix_launch(float* const* logp, const int64_t* ldl, int64_t M, int64_t R, int64_t V, const float* const* nb_score,
                       const int32_t* const* nb_index, int64_t K, const int32_t* const* values, const int64_t* n_values,
                       const float* const* lse, float inv_T, float log_lam, float log1m_lam, hipStream_t s);
// shallow fusion (lm.hip): a back-off n-gram model evaluated densely over the members' rows, and its sparse query
int vag_lm_fuse_rows_launch(float* const* rows, const int64_t* ld, int64_t M, int64_t R, int64_t V, const vag_lm* lm,
                            const int32_t* ctx, float beta, hipStream_t s);
int vag_lm_fuse_beam_launch(float* const* logp, const int64_t* ldl, int64_t M, const int64_t* beam, int64_t di,
                            const int32_t* di_state, bool dev_form, int64_t max_len, int64_t B, int64_t k, int64_t V,
                            const vag_lm* lm, float beta, hipStream_t s);
int vag_lm_query_launch(const vag_lm* lm, const int32_t* ctx, const int32_t* word, int64_t R, float* logp_out, int32_t* order_out,
                        hipStream_t s);
int vag_forced_score_launch(const float* const* logits, const int64_t* ldl, const float* const* lse, int64_t M,
                            const int64_t* tgt, int64_t B, int64_t Tt, int64_t V, float* token_logp, float* logp, float* score,
                            hipStream_t s);
int vag_beam_attn_record_launch(const float* const* alpha, int64_t M, float* attn_hist, int64_t di, const int32_t* di_state,
                                int64_t max_len, int64_t B, int64_t k, int64_t Tp, hipStream_t s);
int vag_beam_finish_align_launch(const float* nll, const int64_t* beam, const float* attn_hist, int64_t max_len, int64_t steps,
                                 int64_t B, int64_t k, int64_t n, int64_t Tp, int64_t Ts, int64_t* out, float* scores,
                                 float* attention, int64_t* src_pos, hipStream_t s);
int vag_forced_align_launch(const float* const* alpha, int64_t M, const int64_t* tgt, int64_t B, int64_t Tt, int64_t Ts,
                            float* attention, int64_t* src_pos, hipStream_t s);
int vag_ens_argmax_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t N, int64_t V, int64_t* out,
                          hipStream_t s);

// ---------------- sample.hip ----------------
int vag_sample_step_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                           int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                           int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                           int32_t* n_alive, hipStream_t s);
int vag_sample_step_p_launch(const float* const* logp, const int64_t* ldl, int64_t M, int64_t* toks, float* token_logp, int64_t di,
                             int32_t* di_state, int64_t max_len, const float* const* h_in, float* const* h_out, const int64_t* H,
                             int64_t* tok_out, int64_t B, int64_t n, int64_t V, float temperature, int64_t top_k, const uint64_t* rng,
                             int32_t* n_alive, float top_p, int32_t* set_size, hipStream_t s);
int vag_sample_noise_launch(const uint64_t* rng, int64_t di, int64_t N, int64_t V, float* out, hipStream_t s);

// ---------------- mbr.hip ----------------
int vag_mbr_supported_host(int64_t Nh, int64_t Lh, int64_t Nr, int64_t Lr);
int vag_mbr_select_launch(const int64_t* hyps, const int64_t* refs, const float* weights, int64_t B, int64_t Nh, int64_t Lh,
                          int64_t Nr, int64_t Lr, int utility, int32_t* matches, float* util, float* expected, int64_t* best,
                          hipStream_t s);
int vag_mbr_best_launch(const float* expected, int64_t B, int64_t Nh, int64_t* best, hipStream_t s);

// ---------------- corpus.hip ----------------
int vag_corpus_bleu_supported_host(int64_t Lh, int64_t R, int64_t Lr);
int vag_corpus_bleu_stats_launch(const int64_t* hyps, const int64_t* refs, const int32_t* n_refs, int64_t N, int64_t Lh, int64_t R,
                                 int64_t Lr, int32_t* per_sentence, int64_t* totals, hipStream_t s);

// ---------------- chrf.hip ----------------
int vag_chrf_supported_host(int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr);
int vag_chrf_max_chars_host();
int vag_surface_expand_launch(const int64_t* rows, int64_t R, int64_t L, const int32_t* off, const int32_t* chars, int64_t V,
                              int32_t* out, int64_t C, int32_t* lens, hipStream_t s);
int vag_chrf_select_launch(const int32_t* hchars, const int32_t* hlens, const int32_t* rchars, const int32_t* rlens,
                           const float* weights, int64_t B, int64_t Nh, int64_t Ch, int64_t Nr, int64_t Cr, int32_t* matches,
                           float* util, float* expected, int64_t* best, hipStream_t s);

// ---------------- api.hip internals shared with step.hip ----------------
// the fused step's ranking loss: G pre-multiplied by a device scalar in the forward (g_scale), no scaling pass in the backward (d_loss NULL)
int vag_rank_loss_fwd_impl(const float* im, const float* sv, int64_t B, int64_t S, float margin, int kind, float* scores,
                           float* G, float* loss, const float* g_scale, hipStream_t s, float scale = 1.f);
int vag_rank_loss_bwd_impl(const float* im, const float* sv, const float* G, const float* d_loss, int64_t B, int64_t S,
                           float* d_im, float* d_s, hipStream_t s);
int vag_dec_init_bwd_impl(const float* mask, const float* xmix, const float* h0, float split, const float* W, float* d_h0,
                          int64_t B, int64_t Ts, int64_t C, int64_t H, float* d_enc, int accumulate_enc, float* d_ctx,
                          int accumulate_ctx, float* g_W, float* g_b, float* scratch, hipStream_t s);
int vag_imagine_attn_ctx_bwd_impl(const float* im_emb, const float* enc, const float* mask, const float* ctx2ctx,
                                  const float* emb2ctx, const float* mlp_w, int method, int64_t B, int64_t Ts, int64_t C,
                                  int64_t S, const float* alpha, const float* d_ctx, float* ws, float* d_enc,
                                  int accumulate_enc, float* d_im_emb, int accumulate_im, float* g_ctx2ctx,
                                  float* g_emb2ctx, float* g_mlp_w, hipStream_t s);

// ---------------- head_api.hip: the output head's host layer ----------------
// One sequence-level call of the head, forward or backward: R = Tt * B rows, row r = t*B + b.  The ABI entry points fill what
// their argument lists carry and leave the rest at its default, which means "stand-alone operator call"; vag_train_step fills one
// bundle and hands it to the forward and then to the backward of the same call.
struct HeadSeq {
    int64_t B = 0, Tt = 0, E = 0, H = 0, V = 0, ldl = 0;
    float p_out = 0.f, eps = 0.f;               // dropout on tmid (with the caller's generator state), label smoothing of the loss
    const uint64_t* rng = nullptr;
    const float *h2 = nullptr, *c = nullptr, *e = nullptr;      // activations (R,H), (R,2H), (R,E)
    vag_head_w w = {};
    const int64_t* tgt = nullptr;               // (B,Tt)
    const float* vocab_weight = nullptr;
    float *tmid = nullptr, *logits = nullptr, *lse = nullptr, *nll = nullptr, *inv_cnt = nullptr;
    // where the loss goes: loss_mt[0], or losses = {loss, loss_mt, loss_vse, count, ring ...} with the weights of the total and
    // vag_step_cfg.loss_ring (the n-th execution's losses stay readable for that many steps)
    float *loss_mt = nullptr, *losses = nullptr;
    float w_mt = 0.f, w_vse = 0.f;
    int has_vse = 0, ring = 0, logits_ready = 0;        // logits_ready: the caller has formed tmid and the logits (free-running decoder)
    // backward: d(loss), the input gradients, the parameter gradients, and dt (R,E): d(tmid), left holding d(pre-activation)
    const float* d_loss = nullptr;
    float *d_h2 = nullptr, *d_c = nullptr, *d_e = nullptr, *dt = nullptr;
    vag_head_g g = {};
    // What only a step sets.  inv_cnt_ready: its prologue launch has filled inv_cnt.  chunk: rows per chunk of the vocabulary product
    // (0: the whole sequence at once).  finish_in_fwd: the backward follows in the same call, the forward finishes each chunk (needs
    // d_loss, g, dt); fwd_finished, written by the forward: it did, the backward starts at d(tmid).
    int64_t chunk = 0;
    bool inv_cnt_ready = false, finish_in_fwd = false, fwd_finished = false;
    // n > 0: the forward ends in vag_mrt_weights' launch instead of the loss reduction (mrt.hip): inv_cnt becomes the minimum-risk
    // coefficients the backward reads, the losses the risk
    struct Mrt { int n = 0; float alpha = 0.f, scale = 0.f; const float* cost = nullptr; const float* valid = nullptr; } mrt;
    // k > 0: word-level distillation (distill.hip).  idx, q (R, k): the teacher's k best words of every row and their renormalised
    // probabilities; each pass over rows runs vag_kd_nll_launch behind its log-sum-exp part and vag_kd_dlogits_launch behind its
    // d(logits) part.  Only with eps == 0, mrt.n == 0, logits formed here and fp32 storage (head_seq_check)
    struct Kd { int k = 0; float lambda = 0.f; const int32_t* idx = nullptr; const float* q = nullptr; } kd;
    // alpha > 0: R-Drop (rdrop.hip), B even, rows 2 p and 2 p + 1 twins.  kl (R): each pass over rows runs vag_rdrop_pair_launch behind
    // its log-sum-exp part (writes kl) and vag_rdrop_bwd_colsum_launch as its d(logits) part (reads kl).  Any eps; only with mrt.n == 0,
    // kd.k == 0, logits formed here and fp32 storage (head_seq_check)
    struct Rd { float alpha = 0.f; float* kl = nullptr; } rd;
    hipStream_t s = nullptr;
};
int vag_head_seq_fwd(HeadSeq& a);
int vag_head_seq_bwd(const HeadSeq& a);
// one decoding step's tmid and logits for N rows (the decoder's free-running launch chain in dec_api.hip calls it too); tmp, tmid: (N,E) scratch
int vag_head_step(const float* h2, const float* c, const float* e, const vag_head_w& w, int64_t N, int64_t E, int64_t H, int64_t V,
                  float p_out, const uint64_t* rng, int64_t drop_idx0, float* tmp, float* tmid, float* logits, int64_t ldl,
                  hipStream_t s);

// dec_api.hip: decoder parameter gradients from the rows of time steps [t0, t1) (first: this chunk initialises the folded-product
// gradient instead of adding to it), and the embedding scatter of those steps once every chunk's products are launched
int vag_cgru_bwd_weights_chunk(const float* h0, const int64_t* tok, vag_dec_w w, int64_t B, int64_t Ts, int64_t Tt, int64_t E,
                               int64_t H, const float* h2_all, const float* c_all, const float* e_all, const float* d_e_all,
                               float* ws, vag_dec_g g, float* scratch, int64_t t0, int64_t t1, bool first, hipStream_t s);
int vag_cgru_bwd_weights_scatter(const int64_t* tok, int64_t B, int64_t Ts, int64_t Tt, int64_t E, int64_t H, vag_dec_g g,
                                 float* scratch, int64_t t0, int64_t t1, hipStream_t s);
