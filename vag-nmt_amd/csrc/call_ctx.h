// What a call tells the operators and launchers it reaches.  Host-side only: consulted when work is
// enqueued (at capture time for a captured step), never read by a kernel through a pointer to the context itself.
//
// Two levels.  Every host thread has a BASE context: vag_set_operator_context / vag_set_operator_guard edit it ("on the calling
// thread until changed"), and an operator entry point called on its own sees it.  vag_train_step builds a PER-CALL context on its
// stack -- a copy of the base with its own fields filled in -- and installs it with one VagCallScope for the duration of the call;
// the operator entry points it calls on the same thread see that one through vag_ctx().  Per thread because the forward runs on
// the caller's thread and the backward on the autograd engine's; one host thread drives a stream.
// The defaults mean "stand-alone operator call".  A hint or a request nobody consumed goes with the call that made it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vag_nmt.h"

// A held-back loss reduction (head.hip): handed to the next ce_bwd_colsum launch as a kernel argument.
struct LossTask {
    const float* nll = nullptr; const float* inv_cnt = nullptr; float* losses = nullptr;
    int B = 0, Tt = 0, has_vse = 0, ring = 0;
    float w_mt = 0.f, w_vse = 0.f;
};
// Held-back accumulations into one (B,Ts,C) tensor (attn.hip): the argument of the one pass that does them.
struct RmwDefer {
    float* out = nullptr;
    const float *a1 = nullptr, *x1 = nullptr, *a2 = nullptr, *x2 = nullptr;      // outer2's operands
    const float *mask = nullptr, *dx = nullptr; float coef = 0.f;                // meanpool_bwd's
    int64_t B = 0, Ts = 0, C = 0;
};

struct VagCallCtx {
    // ---------------- operator context (base: vag_set_operator_context / vag_set_operator_guard; a step: its own arguments) ----------------
    // Derived weights (functions of the parameters only: stacked / folded / transposed matrices the recurrences read).  The
    // stand-alone operators rebuild them per call inside their workspaces (NULL); a step driver that owns the optimiser refreshes
    // them once per optimiser step (vag_derive_weights) and points the operators at that copy.
    const float* derived = nullptr;
    // 2-byte storage mode (vag_step_cfg.storage = 1): the tensors the recurrences stream at every time step -- their weights (fp16
    // copies in the derived buffer) and the attention keys pe / projected keys encwp -- are fp16 in memory; every product still
    // accumulates in fp32, master weights, recurrent state, saved gates and all gradients stay fp32.
    bool store16 = false;
    // Planes per operand of the bf16 split (gemm.hip): 3 (default: six products, fp32-grade) or 2 (three products: the 2-byte
    // storage mode).  11: ONE fp16 plane (v_mfma_f32_32x32x16_f16; operands rounded to fp16 on their way into LDS -- the 2-byte
    // mode's forward products in the step driver), 1: one bf16 plane (that mode's gradient products: fp16 would flush small gradients).
    int gemm_planes = 3;
    // {void flag, give-up count} pair the persistent recurrence launches report to (persist.hip): the caller's own
    // (vag_step_cfg.guard, vag_set_operator_guard), or NULL: the process-wide pair (vag_persist_guard() resolves it).
    unsigned* guard = nullptr;
    // Caller-owned buffer (vag_set_handoff_planes) in which the one-launch backward recurrences publish their hand-off rows as bf16
    // planes (persist.hip: st_planes4).  The decoder's and the encoder's backward of a step follow each other on one stream and
    // share it.  NULL, or too small for the shape: the fp32 hand-off.
    float* handoff_planes = nullptr;
    int64_t handoff_floats = 0;

    // ---------------- step hints: set by vag_train_step (step.hip), read by the operators ----------------
    // The step's prologue launch has zeroed the head's tmid and the encoder's dx: the two operators that accumulate into them
    // from grouped products skip their own fill launch ...
    bool step_zeroed = false;
    // ... and has already embedded the decoder's input tokens of every step (teacher-forced form) into e_all
    bool step_gathered = false;
    // Around the encoder's backward of a step's last phase: its embedding scatter carries the persistent kernels' give-up word into
    // the gradient buffer (the per-operator entry points never do: their gradients go to the caller's own optimiser)
    bool poison_inject = false;
    // The step's prologue launch has zeroed every counter / exchange buffer of the step's recurrence kernels (one launch instead of
    // four): the launch functions of persist.hip skip their own zeroing
    bool persist_prezeroed = false;
    // ... among them the region of the plane buffer in which the decoder's forward hands h1 and h2 off as marked planes (persist.hip:
    // vag_dec_fwd_planes_region), zeroed in place of the two tensors.  NULL: the step zeroed h1 and h2, the launch keeps the fp32 form
    float* dec_fwd_planes_zeroed = nullptr;
    // Scratch of the slab form of split-K (gemm.hip: GemmArgs::slab): caller-owned (the step's workspace), handed over together with
    // the stream that owns it.  A launch takes what its products need from the start of it -- launches of one stream follow each
    // other, so the next one may reuse the same floats; a launch that goes to ANOTHER stream (a step_fork side stream, a leaf-stream
    // flush) gets none (atomics, as before): it may run concurrently with the owner's launches.
    struct GemmScratch { float* slab = nullptr; int64_t floats = 0; unsigned* tickets = nullptr; int64_t ntickets = 0; hipStream_t stream = nullptr; } gemm_scratch;
    // Outputs the step's prologue launch has already zeroed: a sliced (split-K) overwriting product into one of them skips its
    // own fill launch.  An entry is used once (gemm.hip: gemm_take_prezeroed).
    const float* gemm_prezeroed[4] = {nullptr, nullptr, nullptr, nullptr};
    // A side stream for the weight-gradient layout (TN: both operands outer-contiguous, g_W += dY^T X with its bias sums) of the
    // group flushes that follow, until taken back: the step sends the decoder's weight gradients there (step_fork bit 2).  Only
    // leaves have that layout -- nothing later in a step but the optimiser reads what they write -- and it is flushed first, so it
    // depends on nothing else in its flush; the event is recorded on the flushing stream right before, i.e. behind every launch
    // that produced the operands.  `used`: whether a flush went there since it was set.
    struct LeafStream { hipStream_t stream = nullptr; hipEvent_t event = nullptr; bool used = false; } leaf_stream;

    // ---------------- one-shot riders: a producer asks, a consumer takes, the asker checks ----------------
    // The next forward row launch of the visual attention (attn.hip) also leaves xmix (B,C) = split * context + (1 - split) *
    // mean-pool -- what vag_dec_init_fwd would compute from that context with a launch of its own.  done == xmix: it did.
    struct RowMix { float* xmix = nullptr; float split = 0.f; const float* done = nullptr; } row_mix;
    // A step whose initial state is h0 = tanh(.) asks the next persistent decoder backward launch (persist.hip) to apply the tanh's
    // derivative to d_h0 on its way out (a launch saved).  done == d_h0: it did (vag_dec_init_bwd then skips its own).
    struct Dh0Tanh { bool req = false; const float* done = nullptr; } dh0_tanh;
    // The loss reduction as a passenger of the launch that follows it in a training step (ce_bwd_colsum_kernel, which needs none of
    // its results: d(loss) is a constant of the step): while `on`, a vag_loss_mt_launch into the step's losses is held back as `task` and handed to the
    // next vag_ce_bwd_colsum_launch on `stream`, whose block (0,0) does it first; vag_loss_defer_flush launches it on its own if
    // no such launch came.
    struct LossDefer { bool on = false; LossTask task; hipStream_t stream = nullptr; } loss_defer;
    // While rmw.out is set, an accumulating vag_outer2_launch / vag_meanpool_bwd_launch into it is only recorded;
    // vag_rmw_defer_flush makes ONE pass over the tensor for both (they were two read-modify-write passes of 21 MB each).
    RmwDefer rmw;
    // Leaf queue (gemm.hip): small rank-B weight-gradient products (and their column sums) are held back until vag_leaf_flush
    bool leaf_on = false;
    // Left by vag_cgru_attn_decode_seq_bwd_loop when it has formed u_all beside d_uk, taken by the weight-gradient function of the
    // same backward (same scratch, same host thread; two ABI entry points, so it cannot travel as an argument)
    const float* u_all_ready = nullptr;
};

// the calling thread's active context: the per-call one while a VagCallScope is open, else the thread's base context
VagCallCtx& vag_ctx();

// Installs `c` as the calling thread's active context until the end of the scope (api.hip).
struct VagCallScope {
    VagCallCtx& ctx;
    VagCallCtx* prev;
    explicit VagCallScope(VagCallCtx& c);
    ~VagCallScope();
    VagCallScope(const VagCallScope&) = delete;
    VagCallScope& operator=(const VagCallScope&) = delete;
};
