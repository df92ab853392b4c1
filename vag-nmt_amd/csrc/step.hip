// Fused training step (train.py:36-51 around models/...V11.py:82-168 / NMT_Seq2Seq_Beam_V2.py:58-113): zero-grad is the
// optimiser's job (vag_clip_adam_flat leaves the gradient buffer zeroed), so one call here enqueues the whole forward and
// backward of one mini-batch on the caller's stream -- every operator of include/vag_nmt.h in the order autograd would run
// them, on ONE caller-owned workspace, with the gradient w.r.t. the encoder states accumulated in place by its four
// consumers (decoder, attention keys, decoder initial state, image-conditioned attention) instead of summed by the host
// framework.  No allocation, no host synchronisation: a step is capturable into a HIP graph, and the `phases` mask lets a
// data-parallel driver cut it where a gradient bucket becomes final (after the decoder side: everything but the encoder's
// parameters; after the encoder's backward recurrence: the rest).
#include "../../include/vag_nmt.h"
#include <vector>
#include "kernels.h"
#include "seq_layout.h"

#define S_(x) reinterpret_cast<hipStream_t>(x)

namespace {

struct StepWs {
    float *enc, *mask, *ws_enc, *pe;
    float *y_im, *nrm_im, *im_emb, *ws_img, *alpha_v, *ctx, *y_txt, *nrm_txt, *txt_emb, *rscores, *G;
    float *xmix, *hseq, *c_all, *e_all, *ws_dec, *tmid, *logits, *lse, *nll, *inv_cnt, *consts;
    int64_t* tok;
    float *d_enc, *d_pe, *d_h2, *d_c, *d_e, *d_h0, *d_ctx, *d_im, *d_txt, *scr_dec, *scr_head, *scr_ini;
    float* free_tab;            // tables of the one-launch free-running decoder (shapes it can take only)
    float* gemm_slab;           // scratch of the slab form of split-K (gemm.hip: GemmArgs::slab), fp32 storage only
    unsigned* gemm_ticket;      // ... and its per-tile arrival counters (zeroed by the step's prologue launch)
    int64_t gemm_slab_floats, gemm_tickets;
    int64_t total;
};

StepWs step_ws(float* p, const vag_step_cfg& c) {
    StepWs w;
    const int64_t B = c.B, Ts = c.Ts, Tt = c.Tt, H = c.H, C = 2 * c.H, S = c.S, R = c.Tt * c.B;
    WsCarver cv(p);
    w.enc = cv.take(B * Ts * C); w.mask = cv.take(B * Ts); w.ws_enc = cv.take(vag_bigru_ws_floats(B, Ts, c.Es, H));
    w.pe = cv.take(B * Ts * C);
    const bool mm = c.multimodal != 0;
    w.y_im = cv.take(mm ? B * S : 0); w.nrm_im = cv.take(mm ? B : 0); w.im_emb = cv.take(mm ? B * S : 0);
    w.ws_img = cv.take(mm ? vag_imagine_ws_floats(B, Ts, C, S, c.attn_method) : 0);
    w.alpha_v = cv.take(mm ? B * Ts : 0); w.ctx = cv.take(mm ? B * C : 0);
    w.y_txt = cv.take(mm ? B * S : 0); w.nrm_txt = cv.take(mm ? B : 0); w.txt_emb = cv.take(mm ? B * S : 0);
    w.rscores = cv.take(mm ? B * B : 0); w.G = cv.take(mm ? B * B : 0);
    w.xmix = cv.take(B * C); w.hseq = cv.take((Tt + 1) * B * H); w.c_all = cv.take(R * C); w.e_all = cv.take(R * c.Et);
    w.ws_dec = cv.take(vag_cgru_ws_floats(B, Ts, Tt, c.Et, H));
    w.tmid = cv.take(R * c.Et); w.logits = cv.take(R * c.ldl); w.lse = cv.take(R); w.nll = cv.take(R); w.inv_cnt = cv.take(B);
    w.consts = cv.take(8);
    w.tok = cv.take_as<int64_t>((Tt + 1) * B);
    w.d_enc = cv.take(B * Ts * C); w.d_pe = cv.take(B * Ts * C); w.d_h2 = cv.take(R * H); w.d_c = cv.take(R * C); w.d_e = cv.take(R * c.Et);
    w.d_h0 = cv.take(B * H); w.d_ctx = cv.take(mm ? B * C : 0); w.d_im = cv.take(mm ? B * S : 0); w.d_txt = cv.take(mm ? B * S : 0);
    w.scr_dec = cv.take(vag_cgru_bwd_scratch_floats(B, Ts, Tt, c.Et, H)); w.scr_head = cv.take(R * c.Et); w.scr_ini = cv.take(B * C);
    // (by shape, not by device: a workspace size must not depend on where it is asked for)
    w.free_tab = cv.take(H == 512 && c.Et == 256 && B <= 64 ? vag_dec_tables(nullptr, B, Ts, Tt, c.Et, H, c.V).total : 0);
    // split-K slabs: the largest flush of a step parks (k-slices x its output elements) floats -- at configs[1] 17 M (the d_enc /
    // d_e group), 14 M (the decoder's weight gradients), 7.8 M (d tmid in 12 slices): twelve times the widest activation covers them;
    // a product that does not fit keeps its atomics (gemm_take_slabs).  The 2-byte mode's one-plane kernels do not use slabs.
    const int64_t widest = std::max(std::max(B * Ts * C, R * 3 * H), std::max(3 * H * C, R * c.Et));
    w.gemm_slab_floats = c.storage == 0 ? std::min<int64_t>(12 * widest, 192ll << 20) : 0;      // (at most 768 MB: configs[4] sizes in fp32)
    w.gemm_tickets = c.storage == 0 ? 16384 : 0;
    w.gemm_slab = cv.take(w.gemm_slab_floats);
    w.gemm_ticket = cv.take_as<unsigned>(w.gemm_tickets);
    w.total = cv.off;
    return w;
}

bool cfg_ok(const vag_step_cfg* c) {
    return c && c->B > 0 && c->Ts > 0 && c->Tt > 0 && c->Es > 0 && c->Et > 0 && c->H > 0 && c->V > 0 && c->Es % 4 == 0 &&
           c->Et % 4 == 0 && c->H % 4 == 0 && c->ldl >= c->V && c->ldl % 4 == 0 && c->loss_ring >= 0 && (reinterpret_cast<uintptr_t>(c->guard) & 3) == 0 &&
           vag_label_smoothing_ok(c->label_smoothing) &&
           // a minimum-risk step (mrt_n > 0): whole groups of candidates, forced targets, the plain loss, fp32 storage, no ranking loss
           (c->mrt_n == 0 || (c->mrt_n > 0 && vag_mrt_cfg_ok(c->B, c->mrt_n, c->mrt_alpha, c->mrt_scale) && c->mrt_cost && !c->free_run &&
                              c->label_smoothing == 0.f && c->storage == 0 && c->rank_kind == -1)) &&
           (!c->multimodal || (c->S > 0 && c->S % 4 == 0 && c->I > 0 && (c->attn_method == 0 || c->attn_method == 1) &&
                               c->rank_kind >= -1 && c->rank_kind <= 1));
}

// a distillation step (vag_train_step_kd): forced targets, the plain loss, fp32 storage, not a minimum-risk step; the ranking loss stays
bool kd_cfg_ok(const vag_step_cfg* c, const vag_kd_cfg* kd) {
    return cfg_ok(c) && kd && vag_kd_ok(kd->k, kd->lambda, c->V) && kd->idx && kd->q && !c->free_run && c->label_smoothing == 0.f &&
           c->mrt_n == 0 && c->storage == 0;
}

// an R-Drop step (vag_train_step_rdrop): every sentence twice in adjacent rows, forced targets, fp32 storage, not a minimum-risk step;
// label smoothing and the ranking loss (with the twin rule) stay
bool rdrop_cfg_ok(const vag_step_cfg* c, const vag_rdrop_cfg* rd) {
    return cfg_ok(c) && rd && vag_rdrop_ok(rd->alpha) && rd->kl && c->B % 2 == 0 && !c->free_run && c->mrt_n == 0 && c->storage == 0;
}

// What the recurrence kernels of one training step expect to find zeroed, as word ranges (the prologue launch zeroes them and the
// step tells the launch functions so: persist.hip, VagCallCtx::persist_prezeroed): [0] the encoder's counters, [1] the decoder's
// h1 | psc | sync | sync_b | dal as one range, [2] the encoder's d(embedded inputs), which two grouped products add into.
// dec_fwd_planes: the decoder's forward hands h1 and h2 off as marked planes in the caller's plane buffer (the step zeroes that region
// instead): h1 carries no mark that anybody reads and stays out of the range
void step_zero_ranges(float* ws_enc, float* ws_dec, int64_t B, int64_t Ts, int64_t Tt, int64_t Es, int64_t Et, int64_t H,
                      bool dec_fwd_planes, unsigned** p, int64_t* n) {
    BiGruWs e = bigru_ws(ws_enc, B, Ts, Es, H);
    p[0] = e.sync;
    n[0] = (reinterpret_cast<unsigned*>(ws_enc) + e.total) - e.sync;
    CgruWs d = cgru_ws(ws_dec, B, Ts, Tt, Et, H);
    p[2] = reinterpret_cast<unsigned*>(e.dx);
    n[2] = Ts * B * Es;
    p[1] = reinterpret_cast<unsigned*>(dec_fwd_planes ? d.psc : d.h1);
    n[1] = (reinterpret_cast<unsigned*>(ws_dec) + d.total) - p[1];
}

// rng step counter, the two loss-mix constants, the decoder's input token matrix (row 0 = SOS, row t+1 = target word t:
// V11.py:117,146), the per-sentence token counts -- one launch for the step's scalar bookkeeping.
// Also zeroes the counters and exchange buffers of the step's four recurrence kernels (two word ranges:
// step_zero_ranges): one launch instead of four.
// further ranges the prologue zeroes, in 16-byte units: the decoder's hidden states h2 (exchanged between workgroups with marked
// words, persist.hip: tag1) or, where the decoder's forward hands off marked planes, their region of the caller's plane buffer
// instead (st_planes2_marked); the head's tmid and the encoder's d(embedded inputs) (grouped products accumulate into them)
// ... and two outputs of sliced overwriting products of the backward pass (d(tmid), dgi2 W_ih2), which then skip their fill launches
struct ZeroRanges { uint4* p[6]; int64_t n[6]; };
// the decoder's embedded input tokens of every step (teacher-forced: V11.py:117,146 -> NMT_Decoder.py:118), from the target matrix itself
struct GatherTask { const float* emb; float* out; int E4; };
__global__ __launch_bounds__(256) void step_prologue_kernel(uint64_t* rng, const int64_t* __restrict__ tgt, int B, int Tt,
                                                            int64_t* __restrict__ tok, float* __restrict__ consts,
                                                            float* __restrict__ inv_cnt, float w_mt, float w_vse,
                                                            unsigned* __restrict__ z0, int64_t n0, unsigned* __restrict__ z1,
                                                            int64_t n1, ZeroRanges zr, GatherTask ga) {
    const int64_t gid = blockIdx.x * 256ll + threadIdx.x;
    for (int64_t i = gid; i < n0; i += (int64_t)gridDim.x * 256) z0[i] = 0u;
    if (ga.out) {
        const int64_t rows = (int64_t)Tt * B, tot = rows * ga.E4;
        for (int64_t i = gid; i < tot; i += (int64_t)gridDim.x * 256) {
            const int64_t row = i / ga.E4;
            const int e4 = (int)(i - row * ga.E4);
            const int t = (int)(row / B), b = (int)(row - (int64_t)t * B);
            const int64_t tk = t == 0 ? 2 : tgt[(int64_t)b * Tt + (t - 1)];
            reinterpret_cast<float4*>(ga.out)[i] = reinterpret_cast<const float4*>(ga.emb)[tk * ga.E4 + e4];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)                                                                           // (16-byte units)
        for (int64_t i = gid; i < zr.n[r]; i += (int64_t)gridDim.x * 256) zr.p[r][i] = make_uint4(0u, 0u, 0u, 0u);
    {   // the large range: 16 bytes per thread (the range starts 256-byte aligned; its tail word by word)
        const int64_t n4 = n1 >> 2;
        uint4* z4 = reinterpret_cast<uint4*>(z1);
        for (int64_t i = gid; i < n4; i += (int64_t)gridDim.x * 256) z4[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int64_t i = (n4 << 2) + gid; i < n1; i += (int64_t)gridDim.x * 256) z1[i] = 0u;
    }
    if (gid < B) {                          // inv_cnt[b] = 1 / #(tgt[b,:] != 0)   (V11.py:164)
        int c = 0;
        for (int t = 0; t < Tt; ++t) c += tgt[gid * Tt + t] != 0;
        inv_cnt[gid] = 1.f / (float)c;
    }
    if (gid == 0) {
        if (rng) rng[1] += 1;
        consts[0] = w_mt; consts[1] = w_vse; consts[2] = 0.f; consts[3] = 0.f;
    }
    const int64_t total = (int64_t)(Tt + 1) * B;
    for (int64_t i = gid; i < total; i += (int64_t)gridDim.x * 256) {
        const int t = (int)(i / B), b = (int)(i - (int64_t)t * B);
        tok[i] = t == 0 ? 2 : tgt[(int64_t)b * Tt + (t - 1)];
    }
}

}  // namespace

extern "C" {

int64_t vag_step_ws_floats(const vag_step_cfg* cfg) {
    if (!cfg_ok(cfg)) return VAG_EINVAL;
    return step_ws(nullptr, *cfg).total;
}

// float offset of a workspace tensor, for tests and diagnostics: 0 enc (B,Ts,C), 1 alpha_vse (B,Ts), 2 hseq (Tt+1,B,H),
// 3 logits (Tt*B,ldl), 4 decoder workspace (see vag_cgru_ws_offset), 5 d_enc (B,Ts,C), 6 im_emb, 7 txt_emb, 8 tok (int64)
int64_t vag_step_ws_offset(const vag_step_cfg* cfg, int which) {
    if (!cfg_ok(cfg)) return VAG_EINVAL;
    static float base[1];
    StepWs w = step_ws(base, *cfg);
    const float* p = nullptr;
    switch (which) {
        case 0: p = w.enc; break;
        case 1: p = w.alpha_v; break;
        case 2: p = w.hseq; break;
        case 3: p = w.logits; break;
        case 4: p = w.ws_dec; break;
        case 5: p = w.d_enc; break;
        case 6: p = w.im_emb; break;
        case 7: p = w.txt_emb; break;
        case 8: p = reinterpret_cast<const float*>(w.tok); break;
        default: return VAG_EINVAL;
    }
    return (int64_t)(p - base);
}

}  // extern "C"

// Side branches of a step (round 5).  What a step launches is one chain on the caller's stream, except for work that nothing on
// the chain waits for soon: the image projection of the forward pass (needs only the batch: it runs while the encoder does) and
// the held-back weight-gradient leaves of the backward pass (needed by the optimiser only: they run beside the encoder's backward
// recurrence).  Such work goes to a library-owned side stream between fork() and join(): an event recorded on the caller's
// stream, waited for by the side stream, and back.  Under stream capture both become graph edges (the side stream joins the
// capture through the event), eagerly they are two cheap runtime calls each.  One side stream and four events per host thread
// and device, created on first use, never destroyed (a handful per process).
namespace {
struct ForkState { hipStream_t side = nullptr; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; int dev = -1; };
thread_local ForkState g_fork[8];
ForkState* fork_state() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ForkState* f = nullptr;
    for (auto& x : g_fork) if (x.dev == dev) { f = &x; break; }
    if (!f) for (auto& x : g_fork) if (x.dev < 0) { f = &x; break; }
    if (!f) return nullptr;
    if (!f->side) {
        // lowest priority: what runs here is throughput work nothing waits for soon; the chain on the caller's stream goes first
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = 0; }
        if (hipStreamCreateWithPriority(&f->side, hipStreamNonBlocking, lo) != hipSuccess) { (void)hipGetLastError(); f->side = nullptr; return nullptr; }
        for (auto& e : f->ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        f->dev = dev;
    }
    return f;
}
// a branch: fork(main, slot) returns the side stream (or `main` itself when forks are off / unavailable: the work then simply
// stays on the chain); join(main, slot) makes `main` wait for everything the side stream was given since
struct StepBranch {
    ForkState* f = nullptr;
    bool open = false;
    hipStream_t fork(hipStream_t main, int slot, int bit) {
        if ((vag_opt().step_fork & bit) == 0) return main;
        f = fork_state();
        if (!f) return main;
        if (hipEventRecord(f->ev[slot], main) != hipSuccess || hipStreamWaitEvent(f->side, f->ev[slot], 0) != hipSuccess) {
            (void)hipGetLastError();
            return main;
        }
        open = true;
        return f->side;
    }
    int join(hipStream_t main, int slot) {
        if (!open) return VAG_OK;
        open = false;
        if (hipEventRecord(f->ev[slot], f->side) != hipSuccess || hipStreamWaitEvent(main, f->ev[slot], 0) != hipSuccess)
            return (int)hipGetLastError();
        return VAG_OK;
    }
};
}  // namespace

// kd: NULL (vag_train_step), or the teacher's targets of a distillation step (vag_train_step_kd; checked by the caller)
// rd: NULL, or the weight and the kl buffer of an R-Drop step (vag_train_step_rdrop; checked by the caller)
static int train_step(const vag_step_cfg* cfg, const vag_kd_cfg* kd, const vag_rdrop_cfg* rd, const vag_model_w* wp,
                      const vag_model_g* gp, const int64_t* src, const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight, uint64_t* rng,
                      const float* derived, float* ws, float* losses, int phases, vag_stream_t stream) {
    hipStream_t s = S_(stream);
    VAG_CHECK_ARG(cfg_ok(cfg) && wp && gp && src && lengths && tgt && vocab_weight && ws && losses && aligned16(ws));
    const vag_step_cfg& c = *cfg;
    const vag_model_w& w = *wp;
    const vag_model_g& g = *gp;
    const bool mm = c.multimodal != 0;
    VAG_CHECK_ARG(!mm || (im && w.im_w && w.im_b && w.txt_w && w.txt_b && w.ctx2ctx && w.emb2ctx &&
                          (c.attn_method == 0 || w.mlp_w)));
    VAG_CHECK_ARG(w.enc_emb && w.ini_w && w.ini_b && w.attn_e && (phases & 55) != 0 && (phases & ~55) == 0);
    const int64_t B = c.B, Ts = c.Ts, Tt = c.Tt, H = c.H, C = 2 * H, S = c.S, V = c.V, Et = c.Et;
    StepWs k = step_ws(ws, c);
    VAG_CHECK_ARG(c.storage == 0 || (c.storage == 1 && derived && !c.free_run && H % 8 == 0));
    // output head in row chunks once the logits would exceed 1 GiB (configs[4]: 3.3 GB): the (Tt*B, V) logits are then never
    // formed -- one chunk buffer (<= 640 MiB) is reused.  Measured at configs[4] (fp16 storage, ms per step): whole 46.80;
    // chunks finished in the forward 4096 rows 46.84, 2048 47.7, 1024 48.2, 512 (96 MB, Infinity-Cache sized) 55.7 -- the
    // head is bound by its three products, not by the logits' traffic, and short chunks make those inefficient
    // (d(tmid) = 512 x 512 x K=40000 is 16 tiles); so chunks are as long as the buffer bound allows.
    int64_t chunk = 0;
    if (!c.free_run && (double)c.Tt * (double)c.B * (double)c.ldl * 4.0 > 1073741824.0) {
        chunk = (int64_t)(671088640.0 / ((double)c.ldl * 4.0)) / c.B * c.B;
        if (chunk < c.B) chunk = c.B;
    }
    if (vag_opt().head_chunk >= 0)      // vag_set_option("head_chunk", rows): rows per chunk (0 = never chunk); tests
        chunk = c.free_run ? 0 : vag_opt().head_chunk;
    // What this call tells the operators it calls (call_ctx.h): a copy of the thread's context with the step's own fields filled in,
    // active until the call returns.  A hint that ends earlier is assigned back where it ends; an early error return (VAG_TRY) skips
    // those assignments, which is harmless: the whole context goes with the call.  The scope's destructor flushes a held-back loss
    // reduction and drops an unflushed leaf queue; what the caller had set with vag_set_operator_context / _guard ("until changed")
    // is untouched.
    VagCallCtx ctx = vag_ctx();
    ctx.derived = derived;                  // the driver's derived weights, storage mode (with its plane count)
    ctx.store16 = c.storage == 1;
    ctx.gemm_planes = ctx.store16 ? 2 : 3;
    // a minimum-risk step: the head's forward ends in vag_mrt_weights' launch (head_api.hip: vag_head_seq_fwd), which turns inv_cnt
    // into the risk's coefficients.  They exist only once every row's nll does, so neither shortcut that applies inv_cnt earlier holds
    const bool mrt = c.mrt_n > 0;
    // this call's persistent recurrence launches report a give-up to the caller's guard pair (vag_step_cfg.guard), not process-wide
    if (c.guard) ctx.guard = reinterpret_cast<unsigned*>(c.guard);
    // the recurrence kernels of this call find their counters zeroed by the step's prologue launch, the head and the encoder's
    // backward their accumulation buffers (a backward-only call relies on the forward call of the same step having run first)
    ctx.persist_prezeroed = true;
    ctx.step_zeroed = true;
    VagCallScope scope(ctx);
    // the grouped / single bf16x6 products of this call park their split-K slices in the workspace's slab region instead of adding
    // them into their outputs with one atomic per element and slice (gemm.hip: GemmArgs::slab)
    // (the caller's stream only: a launch on a step_fork side stream may run beside them, and keeps its atomics).  With the forward
    // in this call the scratch is handed over only once the prologue launch has zeroed the tickets (below): a product before it
    // -- the image projection -- keeps its atomics.  A backward-only call finds them zeroed by the forward call of its step.
    const VagCallCtx::GemmScratch slabs = {k.gemm_slab, k.gemm_slab_floats, k.gemm_ticket, k.gemm_tickets, s};
    if (!(phases & 1)) ctx.gemm_scratch = slabs;
    // forward and backward in one call: the chunked head finishes each chunk (d(logits) and its products) in the forward;
    // a backward called on its own (phases = 2 after an earlier phases = 1) recomputes the chunks instead
    // (not a minimum-risk step: a chunk's d(logits) needs coefficients that depend on every chunk's nll -- the backward recomputes)
    const bool head_finish_in_fwd = chunk > 0 && (phases & 1) && (phases & (2 | 16)) && vag_opt().head_fuse != 0 && !mrt;
    const bool has_vse = mm && c.rank_kind >= 0;
    const float w_mt = mm ? c.loss_w : 1.f, w_vse = mm ? 1.f - c.loss_w : 0.f;
    float* h0 = k.hseq;                    // [h0, h2_0 .. h2_{Tt-1}] in one buffer: the W_hh1 gradient is one product
    float* h2_all = k.hseq + B * H;
    const uint64_t* crng = rng;
    const CgruBwdScratch zdec = cgru_bwd_scratch(k.scr_dec, B, Ts, Tt, Et, H);
    float* d_e = zdec.de;                  // d(embedded target inputs): head's share + gru_1's, in place
    // the head's call (kernels.h: HeadSeq), forward (V11.py:140,164-166) and backward alike
    HeadSeq head;
    head.B = B; head.Tt = Tt; head.E = Et; head.H = H; head.V = V; head.ldl = c.ldl;
    head.p_out = c.p_out; head.rng = crng; head.eps = c.label_smoothing;
    head.h2 = h2_all; head.c = k.c_all; head.e = k.e_all; head.w = w.head;
    head.tgt = tgt; head.vocab_weight = vocab_weight; head.logits_ready = c.free_run ? 1 : 0;
    head.tmid = k.tmid; head.logits = k.logits; head.lse = k.lse; head.nll = k.nll; head.inv_cnt = k.inv_cnt;
    head.losses = losses; head.w_mt = w_mt; head.w_vse = w_vse; head.has_vse = has_vse ? 1 : 0; head.ring = c.loss_ring;
    head.d_loss = k.consts + 0; head.d_h2 = k.d_h2; head.d_c = k.d_c; head.d_e = d_e; head.g = g.head; head.dt = k.scr_head;
    head.inv_cnt_ready = true; head.chunk = chunk; head.finish_in_fwd = head_finish_in_fwd;
    if (mrt) head.mrt = {c.mrt_n, c.mrt_alpha, c.mrt_scale, c.mrt_cost, c.mrt_valid};
    // a distillation step: two small launches per pass of the head over rows (distill.hip).  Both shortcuts below stay: a chunk's
    // d(logits) needs nothing beyond the chunk, and a loss reduction that rides in the backward's first launch reads nll after the
    // launch that rewrote it, on the same stream
    if (kd) head.kd = {kd->k, kd->lambda, kd->idx, kd->q};
    // an R-Drop step: one launch behind each log-sum-exp pass and its own d(logits) pass (rdrop.hip).  A chunk is whole time steps
    // of B rows, so a pair never straddles one and finishing chunks in the forward stays; the loss reduction does not ride (below)
    if (rd) head.rd = {rd->alpha, rd->kl};
    head.s = s;
    // 2-byte storage mode: what feeds the large products carries no more than fp16 there (fp16-stored keys and weights,
    // activations the next fp16 product rounds anyway), so they run on one plane: fp16 operands forward (11 significand bits),
    // bf16 operands for every gradient product (fp16 would flush small gradients; their rounding errors average over the long sums)
    const bool one_plane = c.storage == 1 && !c.free_run && vag_opt().s16_one_plane != 0;
    StepBranch br_im, br_leaf, br_dw;
    if (phases & 1) {
        if (one_plane) ctx.gemm_planes = 11;
        if (mm) {
            // V11.py:114, VSE_Imagine_Enc.py:123-132: the image projection needs the batch only -- beside the encoder
            hipStream_t si = br_im.fork(s, 0, 1);
            VAG_TRY(vag_img_proj_l2_fwd(im, w.im_w, w.im_b, B, c.I, S, c.activation_vse, k.y_im, k.nrm_im, k.im_emb, si));
        }
        {
            unsigned* zp[3];
            int64_t zn[3];
            // the teacher-forced decoder forward hands h1 and h2 off as marked planes where the caller's plane buffer has the region: the
            // region is zeroed here (before the encoder's forward writes ITS region of the buffer) in place of the two tensors
            float* dpl = c.free_run ? nullptr : vag_dec_fwd_planes_region(B, Ts, Tt, H);
            ctx.dec_fwd_planes_zeroed = dpl;
            step_zero_ranges(k.ws_enc, k.ws_dec, B, Ts, Tt, c.Es, Et, H, dpl != nullptr, zp, zn);
            int64_t nb = cdiv64((Tt + 1) * B, 256);
            if (nb < cdiv64(zn[1], 1024)) nb = cdiv64(zn[1], 1024);
            if (nb > 1024) nb = 1024;
            ZeroRanges zr;
            zr.p[0] = reinterpret_cast<uint4*>(dpl ? dpl : h2_all); zr.n[0] = dpl ? vag_dec_fwd_planes_floats(B, Tt, H) / 4 : Tt * B * H / 4;
            zr.p[1] = reinterpret_cast<uint4*>(k.tmid); zr.n[1] = Tt * B * Et / 4;
            zr.p[2] = reinterpret_cast<uint4*>(zp[2]); zr.n[2] = zn[2] / 4;
            zr.p[3] = reinterpret_cast<uint4*>(k.scr_head); zr.n[3] = chunk > 0 ? 0 : Tt * B * Et / 4;
            zr.p[4] = reinterpret_cast<uint4*>(zdec.du_all); zr.n[4] = Tt * B * H / 4;
            // split-K tickets (gemm.hip): what the slab form's last-arriver test rests on.  The region's offset moves with (B, Ts, Tt) and
            // the workspace is not cleared between shapes, so no product of the call takes slabs before this launch (ctx.gemm_scratch); the
            // last block of a tile resetting its own ticket only spares the next launch of the same call a zeroing pass.
            zr.p[5] = reinterpret_cast<uint4*>(k.gemm_ticket); zr.n[5] = k.gemm_tickets / 4;
            GatherTask ga = {nullptr, nullptr, 0};
            if (!c.free_run) { ga.emb = w.dec.emb; ga.out = k.e_all; ga.E4 = (int)(Et / 4); }
            hipLaunchKernelGGL(step_prologue_kernel, dim3((unsigned)nb), dim3(256), 0, s, rng, tgt, (int)B, (int)Tt, k.tok,
                               k.consts, k.inv_cnt, w_mt, w_vse, zp[0], zn[0], zp[1], zn[1], zr, ga);
            VAG_LAUNCH_CHECK();
            if (ga.out) ctx.step_gathered = true;
        }
        ctx.gemm_scratch = slabs;
        VAG_TRY(vag_bigru_seq_fwd(src, lengths, w.enc_emb, w.enc_fw, w.enc_bw, c.p_emb, c.p_ctx, crng, B, Ts, c.Es, H, k.enc,
                                  k.mask, k.ws_enc, stream));                                           // V11.py:111
        if (mm) {                                                                                       // V11.py:114
            VAG_TRY(br_im.join(s, 1));
            ctx.row_mix = {k.xmix, c.init_split, nullptr};      // (consumed by the dot method's one-launch attention, else dropped)
            const int rc_att = vag_imagine_attn_ctx_fwd(k.im_emb, k.enc, k.mask, w.ctx2ctx, w.emb2ctx, w.mlp_w, c.attn_method, B, Ts, C, S,
                                                        k.alpha_v, k.ctx, k.ws_img, stream);
            ctx.row_mix.xmix = nullptr;
            VAG_TRY(rc_att);
            VAG_TRY(vag_img_proj_l2_fwd(k.ctx, w.txt_w, w.txt_b, B, C, S, c.activation_vse, k.y_txt, k.nrm_txt, k.txt_emb,
                                        stream));
            if (has_vse)
                // (G times the loss weight: no scaling pass in the backward.)  An R-Drop step: a twin is neither a positive nor a
                // negative of its sibling, and each of the B rows meets every other sentence twice -- 1/4 of the sum is the
                // plain step's loss on the B / 2 sentences
                VAG_TRY(vag_rank_loss_fwd_impl(k.im_emb, k.txt_emb, B, S, c.margin, c.rank_kind | (rd ? 2 : 0), k.rscores, k.G,
                                               losses + 2, k.consts + 1, s, rd ? 0.25f : 1.f));
        }
        VAG_TRY(vag_dec_init_fwd(k.enc, k.mask, mm ? k.ctx : nullptr, mm ? c.init_split : 0.f, w.ini_w, w.ini_b, B, Ts, C, H,
                                 k.xmix, h0, stream));                                                  // V11.py:118
        {
            // the key projection joins the decoder's per-batch products (projected keys, input projection of every step) in
            // one grouped launch: the bracket is flushed by the decoder operator's own bracket before its time loop starts.
            // (Only with the driver's derived weights: otherwise the operator first builds W_ih2 W_c2h, which the queue
            // would hold back.)
            VagGemmGroup outer(derived != nullptr);
            VAG_TRY(vag_attn_keys_proj(k.enc, w.attn_e, B * Ts, C, k.pe, stream));                      // NMT_Decoder.py:47
            if (c.free_run && vag_cgru_free_supported(B, Ts, Tt, Et, H, V))
                VAG_TRY(vag_cgru_attn_decode_free_fwd(k.enc, k.pe, k.mask, h0, k.tok, w.dec, B, Ts, Tt, Et, H, V, h2_all, k.c_all,
                                                      k.e_all, k.ws_dec, &w.head, c.p_out, crng, k.tmid, k.logits, c.ldl,
                                                      k.free_tab, stream));                             // V11.py:148-160, one launch
            else
            VAG_TRY(vag_cgru_attn_decode_seq_fwd(k.enc, k.pe, k.mask, h0, k.tok, w.dec, B, Ts, Tt, Et, H, V, h2_all, k.c_all,
                                                 k.e_all, k.ws_dec, c.free_run, &w.head, c.p_out, crng, k.tmid, k.logits,
                                                 c.ldl, stream));                                       // V11.py:138-160
            VAG_TRY(outer.end(s));
        }
        // with the head's backward in the same call the loss reduction rides in that backward's first launch
        // (a minimum-risk step has no loss reduction to hold back: the backward's first launch reads what takes its place)
        // (nor an R-Drop step: its d(logits) launch is rdrop.hip's, which carries no loss task)
        if ((phases & (2 | 16)) && chunk == 0 && vag_opt().loss_ride != 0 && !mrt && !rd) ctx.loss_defer.on = true;
        VAG_TRY(vag_head_seq_fwd(head));
    }
    if (one_plane && (phases & 54)) ctx.gemm_planes = 1;
    // phase 2 = its two halves 16 (head + decoder: final for the head's, the decoder's and attn_e's gradients) and 32 (visual grounding
    // + initial state: final for vse_imagine.* and decoderini.*): a data-parallel driver with three buckets calls them one by one
    if (phases & (2 | 16)) {
        // zeroed by this step's prologue launch (a backward-only call: by the forward call of the same step)
        if (chunk == 0) ctx.gemm_prezeroed[0] = k.scr_head;
        ctx.gemm_prezeroed[1] = zdec.du_all;
        VAG_TRY(vag_head_seq_bwd(head));
        VAG_TRY(vag_loss_defer_flush());
        {
            // after the backward recurrence: the products that add into d_enc (projected keys, attention keys) and the weight
            // gradients of the decoder and of attn_e are queued by layout and go out as two grouped launches
            VagGemmGroup outer(true);
            // step_fork bit 2 (value 4; round 6): the decoder's weight-gradient products (the TN layout of this
            // bracket's flushes: eight K = Tt*B products that only the optimiser reads) leave on the low-priority side stream and run
            // beside the VSE / initial-state backward and the encoder's backward recurrence.  Only when that backward follows in this
            // call: a data-parallel driver's phase call ends here and all-reduces these gradients next.
            ForkState* dw_side = (phases & 4) && (phases & (2 | 32)) && (vag_opt().step_fork & 4) ? fork_state() : nullptr;
            if (dw_side) ctx.leaf_stream = {dw_side->side, dw_side->ev[4], false};
            // the initial state's backward follows in this call: d_h0 leaves the recurrence kernel as the gradient of tanh's argument
            ctx.dh0_tanh.req = (phases & 2) != 0;
            VAG_TRY(vag_cgru_attn_decode_seq_bwd_loop(k.enc, k.pe, k.mask, h0, k.tok, w.dec, B, Ts, Tt, Et, H, V, h2_all, k.c_all,
                                                      k.e_all, k.d_h2, k.d_c, d_e, k.ws_dec, k.d_enc, 0, k.d_pe, k.d_h0,
                                                      k.scr_dec, stream));
            VAG_TRY(vag_attn_keys_proj_bwd(k.enc, w.attn_e, k.d_pe, B * Ts, C, k.d_enc, 1, g.attn_e, stream));
            VAG_TRY(vag_cgru_attn_decode_seq_bwd_weights(h0, k.tok, w.dec, B, Ts, Tt, Et, H, h2_all, k.c_all, k.e_all, d_e,
                                                         k.ws_dec, g.dec, k.scr_dec, stream));
            VAG_TRY(outer.end(s));
            if (dw_side && ctx.leaf_stream.used) { br_dw.f = dw_side; br_dw.open = true; }      // joined at the end of the call
            ctx.leaf_stream.stream = nullptr; ctx.leaf_stream.event = nullptr;       // (this bracket's flushes only)
            ctx.dh0_tanh.req = false;
        }
    }
    if (phases & (2 | 32)) {
        // the weight-gradient products of the VSE branch and of the initial state (rank-B updates nothing later in the step reads)
        // and their bias sums are held back and leave as ONE launch, on a side branch that joins before the optimiser
        ctx.leaf_on = vag_opt().leaf_queue != 0;
        // ... and the two accumulations into d_enc of this block (initial state: mean pool; visual attention: outer products) are one pass
        ctx.rmw = RmwDefer();
        ctx.rmw.out = k.d_enc;
        if (mm) {
            if (has_vse) {
                VAG_TRY(vag_rank_loss_bwd_impl(k.im_emb, k.txt_emb, k.G, nullptr, B, S, k.d_im, k.d_txt, s));
            } else {
                VAG_TRY(vag_axpy_launch(0.f, k.d_im, k.d_im, B * S, 2, s));
                VAG_TRY(vag_axpy_launch(0.f, k.d_txt, k.d_txt, B * S, 2, s));
            }
            VAG_TRY(vag_img_proj_l2_bwd(k.ctx, w.txt_w, k.y_txt, k.nrm_txt, k.txt_emb, k.d_txt, B, C, S, c.activation_vse,
                                        k.d_ctx, g.txt_w, g.txt_b, stream));
        }
        VAG_TRY(vag_dec_init_bwd_impl(k.mask, k.xmix, h0, mm ? c.init_split : 0.f, w.ini_w, k.d_h0, B, Ts, C, H, k.d_enc, 1,
                                      mm ? k.d_ctx : nullptr, 1, g.ini_w, g.ini_b, k.scr_ini, s));
        if (mm) {
            VAG_TRY(vag_imagine_attn_ctx_bwd_impl(k.im_emb, k.enc, k.mask, w.ctx2ctx, w.emb2ctx, w.mlp_w, c.attn_method, B, Ts,
                                                  C, S, k.alpha_v, k.d_ctx, k.ws_img, k.d_enc, 1, k.d_im, 1, g.ctx2ctx,
                                                  g.emb2ctx, g.mlp_w, s));
            VAG_TRY(vag_img_proj_l2_bwd(im, w.im_w, k.y_im, k.nrm_im, k.im_emb, k.d_im, B, c.I, S, c.activation_vse, nullptr,
                                        g.im_w, g.im_b, stream));
        }
        VAG_TRY(vag_rmw_defer_flush(s));
        {
            // with the encoder's backward in the same call the leaves run beside its recurrence; a data-parallel driver's phase
            // call ends here (these gradients belong to the bucket it all-reduces next): joined at once
            hipStream_t sl = (phases & 4) ? br_leaf.fork(s, 2, 2) : s;
            VAG_TRY(vag_leaf_flush(sl));
        }
    }
    if (phases & 4) {
        // the last launch of the backward pass turns a give-up of any persistent recurrence of this step into a non-finite
        // gradient entry (persist.hip, optim.hip: the optimiser then skips the step, on every replica)
        ctx.poison_inject = true;
        VAG_TRY(vag_bigru_seq_bwd(src, lengths, w.enc_fw, w.enc_bw, c.p_emb, c.p_ctx, crng, B, Ts, c.Es, H, k.d_enc, k.ws_enc,
                                  g.enc_emb, g.enc_fw, g.enc_bw, stream));
        ctx.poison_inject = false;
    }
    VAG_TRY(br_leaf.join(s, 3));
    VAG_TRY(br_dw.join(s, 5));
    return VAG_OK;
}

extern "C" {

int vag_train_step(const vag_step_cfg* cfg, const vag_model_w* wp, const vag_model_g* gp, const int64_t* src,
                   const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight, uint64_t* rng,
                   const float* derived, float* ws, float* losses, int phases, vag_stream_t stream) {
    return train_step(cfg, nullptr, nullptr, wp, gp, src, lengths, tgt, im, vocab_weight, rng, derived, ws, losses, phases, stream);
}

int vag_step_kd_check(const vag_step_cfg* cfg, const vag_kd_cfg* kd) { return kd_cfg_ok(cfg, kd) ? VAG_OK : VAG_EINVAL; }

int vag_train_step_kd(const vag_step_cfg* cfg, const vag_kd_cfg* kd, const vag_model_w* wp, const vag_model_g* gp, const int64_t* src,
                      const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight, uint64_t* rng,
                      const float* derived, float* ws, float* losses, int phases, vag_stream_t stream) {
    VAG_CHECK_ARG(kd_cfg_ok(cfg, kd));
    return train_step(cfg, kd, nullptr, wp, gp, src, lengths, tgt, im, vocab_weight, rng, derived, ws, losses, phases, stream);
}

int vag_step_rdrop_check(const vag_step_cfg* cfg, const vag_rdrop_cfg* rd) { return rdrop_cfg_ok(cfg, rd) ? VAG_OK : VAG_EINVAL; }

int vag_train_step_rdrop(const vag_step_cfg* cfg, const vag_rdrop_cfg* rd, const vag_model_w* wp, const vag_model_g* gp,
                         const int64_t* src, const int32_t* lengths, const int64_t* tgt, const float* im, const float* vocab_weight,
                         uint64_t* rng, const float* derived, float* ws, float* losses, int phases, vag_stream_t stream) {
    VAG_CHECK_ARG(rdrop_cfg_ok(cfg, rd));
    return train_step(cfg, nullptr, rd, wp, gp, src, lengths, tgt, im, vocab_weight, rng, derived, ws, losses, phases, stream);
}

}  // extern "C"
