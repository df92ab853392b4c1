"""Binding of the fused training step (vag_train_step, include/vag_nmt.h): the model's parameters and their flat-gradient
views as the C structs, the shape/config struct, the workspace and the static input buffers.

One ``FusedStep`` serves every batch shape: the workspace and the input buffers are sized for the largest shape seen and
each (B, Ts, Tt) batch is laid out densely at their front, so HIP graphs captured for different shapes share all memory
(a captured step owns nothing but its kernel nodes)."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import DecW, GruW, HeadW, KdCfg, ModelW, RdropCfg, StepCfgMrt, call, gru_w, ptr, stream
from .state import dropout_rng


def mt_label_smoothing(criterion_mt):
    """The label smoothing eps of a translation criterion the HIP loss kernels implement, or None for any other criterion:
    0.0 for the reference's ``nn.NLLLoss(weight, reduction='none')``, ``label_smoothing`` of a ``LabelSmoothedNLLLoss``.
    By exact type: a subclass may compute anything, and goes through the generic per-step criterion path."""
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    if type(criterion_mt) is nn.NLLLoss:
        ok = criterion_mt.reduction == 'none' and criterion_mt.weight is not None and criterion_mt.ignore_index < 0
        return 0.0 if ok else None
    if type(criterion_mt) is LabelSmoothedNLLLoss:
        return float(criterion_mt.label_smoothing)
    return None


def fusable(model, criterion_mt, criterion_vse):
    """The fused step implements the reference's own criteria (nmt_multimodal_beam_DE.py:291-299) and the label-smoothed
    translation loss; anything else goes through the per-operator autograd path."""
    from machine_translation_vision.losses import ImageRetrievalRankingLoss, PairwiseRankingLoss
    ok_mt = mt_label_smoothing(criterion_mt) is not None
    ok_vse = criterion_vse is None or type(criterion_vse) in (PairwiseRankingLoss, ImageRetrievalRankingLoss)
    return ok_mt and ok_vse and hasattr(model, "encoder") and hasattr(model, "decoder")


def _views(params, grad):
    return [p._vag_grad if grad else p for p in params]


def model_struct(model, grad=False):
    """vag_model_w (grad=False) or vag_model_g (grad=True: the parameters' views into the flat gradient buffer)."""
    enc, dec = model.encoder, model.decoder
    g = enc.gru
    t = lambda p: ptr(p._vag_grad if grad else p)       # noqa: E731
    gw = lambda a, b, c, d: GruW(t(a), t(b), t(c), t(d))   # noqa: E731
    mm = hasattr(model, "vse_imagine")
    s = ModelW()
    s.enc_emb = t(enc.embedding.weight)
    s.enc_fw = gw(g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
    s.enc_bw = gw(g.weight_ih_l0_reverse, g.weight_hh_l0_reverse, g.bias_ih_l0_reverse, g.bias_hh_l0_reverse)
    if mm:
        v = model.vse_imagine
        s.im_w, s.im_b = t(v.im_embedding.weight), t(v.im_embedding.bias)
        s.txt_w, s.txt_b = t(v.text_embedding.weight), t(v.text_embedding.bias)
        s.ctx2ctx, s.emb2ctx = t(v.imagine_attn.ctx2ctx.weight), t(v.imagine_attn.emb2ctx.weight)
        s.mlp_w = t(v.imagine_attn.mlp.weight) if v.imagine_attn.method == "mlp" else None
    s.ini_w, s.ini_b = t(model.decoderini.weight), t(model.decoderini.bias)
    s.attn_e = t(dec.attn.attn_e.weight)
    dp = dec.dec_params()
    s.dec = DecW(t(dec.embedding.weight), gw(dp[0], dp[1], dp[2], dp[3]), t(dp[4]), t(dp[5]), t(dp[6]),
                 gw(dp[7], dp[8], dp[9], dp[10]))
    s.head = HeadW(*[t(p) for p in dec.head_params()])
    return s


class FusedStep:
    LOSS_RING = 256
    def __init__(self, model, criterion_mt, criterion_vse, storage="f32"):
        """storage: "f32", or "f16" = BASELINE configs[4]'s 2-byte storage: the recurrences' weights and the attention keys
        are kept as fp16 in HBM on teacher-forced steps (free-running steps of the same driver use fp32 storage)."""
        if storage not in ("f32", "f16"):
            raise ValueError("storage must be 'f32' or 'f16'")
        self.storage16 = storage == "f16"
        self.model = model
        self.mm = hasattr(model, "vse_imagine")
        self.vw = criterion_mt.weight
        # read once: constant for the driver's lifetime, a by-value member of every captured step configuration
        self.label_smoothing = mt_label_smoothing(criterion_mt)
        if self.label_smoothing is None:
            raise ValueError("FusedStep: criterion_mt is not one the fused step implements (see fusable())")
        self.dev = self.vw.device
        dec, enc = model.decoder, model.encoder
        self.H = dec.hidden_size
        self.V = dec.out.bias.shape[0]
        self.ldl = (self.V + 3) // 4 * 4
        self.Es = enc.embedding.weight.shape[1]
        self.Et = dec.embedding.weight.shape[1]
        if self.storage16 and self.H % 8 != 0:
            raise ValueError("fp16 storage needs hidden_size % 8 == 0")
        self.S = model.vse_imagine.shared_embedding_size if self.mm else 0
        self.I = model.vse_imagine.im_size if self.mm else 0
        self.rank_kind, self.margin = -1, 0.0
        if self.mm and criterion_vse is not None:
            from machine_translation_vision.losses import PairwiseRankingLoss
            self.rank_kind = 0 if type(criterion_vse) is PairwiseRankingLoss else 1
            self.margin = float(criterion_vse.margin)
        self.w = model_struct(model, grad=False)
        self.g = model_struct(model, grad=True)
        self.derived = torch.empty(L.lib().vag_derived_floats(self.H), dtype=torch.float32, device=self.dev)
        # [loss, loss_mt, loss_vse, execution count] + a ring of the last LOSS_RING steps' results (vag_step_cfg.loss_ring): what a
        # step hands out stays valid for that many further steps without a copy launch per step
        self.losses = torch.zeros(4 + 4 * self.LOSS_RING, dtype=torch.float32, device=self.dev)
        self.executed = 0             # forward phases executed so far (eager calls and graph replays; the device counts the same)
        self.ws = None
        self.planes = None
        self.cap = (0, 0, 0)          # (B*Ts, B*Tt, B) capacity of the static input buffers
        self.src = self.tgt = self.im = self.lens = None
        self.mrt_cost = self.mrt_valid = None      # (B capacity,) static inputs of a minimum-risk step (vag_step_cfg.mrt_cost / mrt_valid)
        self.kd_idx = self.kd_q = None             # (Tt*B*K capacity) static inputs of a distillation step (vag_kd_cfg.idx / q)
        self.rd_kl = None                          # (B*Tt capacity,) static output of an R-Drop step (vag_rdrop_cfg.kl), rows time-major
        self.generation = 0           # bumped whenever a static buffer is re-allocated (captured graphs are then stale)
        # device address of the owning driver's guard pair {void flag, give-up count} (vag_step_cfg.guard; TrainStep keeps it in its
        # optimiser scratch) or None: the process-wide pair, which no optimiser reads
        self.guard = None
        self.refresh_derived()

    # ---- configuration ----
    def cfg(self, B, Ts, Tt, teacher, train=True, mrt=None):
        """mrt: None, or (N, alpha, scale) of a minimum-risk step (vag_step_cfg.mrt_*) on the static mrt_cost / mrt_valid buffers: no
        ranking loss and loss_w = 1 for that call."""
        m = self.model
        c = StepCfgMrt()
        c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = B, Ts, Tt, self.Es, self.Et, self.H, self.S, self.I, self.V, self.ldl
        c.multimodal = 1 if self.mm else 0
        c.attn_method = 1 if (self.mm and m.vse_imagine.imagine_attn.method == "mlp") else 0
        c.activation_vse = 1 if (self.mm and m.vse_imagine.activation_vse) else 0
        c.rank_kind = self.rank_kind
        c.free_run = 0 if teacher else 1
        c.storage = 1 if (self.storage16 and teacher) else 0
        c.margin = self.margin
        c.loss_w = float(m.loss_w) if self.mm else 1.0
        c.init_split = float(m.init_split) if self.mm else 0.0
        c.p_emb = float(m.encoder.dropout_emb) if train else 0.0
        c.p_ctx = float(m.encoder.dropout_ctx) if train else 0.0
        c.p_out = float(m.decoder.dropout_out) if train else 0.0
        c.loss_ring = self.LOSS_RING
        c.guard = self.guard
        c.label_smoothing = self.label_smoothing
        if mrt is not None:
            c.mrt_n, c.mrt_alpha, c.mrt_scale = int(mrt[0]), float(mrt[1]), float(mrt[2])
            c.mrt_cost, c.mrt_valid = ptr(self.mrt_cost), ptr(self.mrt_valid)
            c.rank_kind, c.loss_w = -1, 1.0
        return c

    def kd_cfg(self, kd):
        """vag_kd_cfg of a distillation step from kd = (K, lambda), on the static kd_idx / kd_q buffers; the ranking loss stays."""
        return KdCfg(int(kd[0]), float(kd[1]), ptr(self.kd_idx, torch.int32), ptr(self.kd_q))

    def rdrop_cfg(self, rdrop):
        """vag_rdrop_cfg of an R-Drop step from rdrop = (alpha,), on the static rd_kl buffer; label smoothing and the ranking loss stay."""
        return RdropCfg(float(rdrop[0]), ptr(self.rd_kl))

    def reserve(self, B, Ts, Tt):
        """Make the static buffers large enough for a (B,Ts,Tt) batch; returns True if anything was re-allocated."""
        c = self.cfg(B, Ts, Tt, True)
        need = L.lib().vag_step_ws_floats(c.ref())
        if need < 0:
            raise L.VagError("vag_step_ws_floats: bad configuration")
        grown = False
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(int(need * 1.25), dtype=torch.float32, device=self.dev)
            grown = True
        # the backward recurrences' hand-off rows as bf16 planes: a buffer of its own beside the workspace (vag_set_handoff_planes)
        need = L.lib().vag_handoff_planes_floats(B, Ts, Tt, self.H)
        if need > 0 and (self.planes is None or self.planes.numel() < need):
            self.planes = torch.empty(int(need * 1.25), dtype=torch.float32, device=self.dev)
            grown = True
        cap = (max(self.cap[0], B * Ts), max(self.cap[1], B * Tt), max(self.cap[2], B))
        if cap != self.cap:
            self.cap = cap
            self.src = torch.zeros(cap[0], dtype=torch.int64, device=self.dev)
            self.tgt = torch.zeros(cap[1], dtype=torch.int64, device=self.dev)
            self.lens = torch.zeros(cap[2], dtype=torch.int32, device=self.dev)
            self.im = torch.zeros(cap[2] * max(self.I, 1), dtype=torch.float32, device=self.dev)
            self.mrt_cost = torch.zeros(cap[2], dtype=torch.float32, device=self.dev)
            self.mrt_valid = torch.zeros(cap[2], dtype=torch.float32, device=self.dev)
            self.rd_kl = torch.zeros(cap[1], dtype=torch.float32, device=self.dev)
            grown = True
        if grown:
            self.generation += 1
        return grown

    def load_batch(self, src, lengths, tgt, im):
        """The batch into the static buffers, densely at their front: one launch (vag_copy4)."""
        B, Ts = src.shape
        Tt = tgt.shape[1]
        srcs = [src, tgt, lengths] + ([im] if self.mm else [])
        dsts = [self.src, self.tgt, self.lens] + ([self.im] if self.mm else [])
        for t in srcs:
            if not (t.is_cuda and t.is_contiguous()):
                raise L.VagError("batch tensors must be contiguous HIP tensors")
        if src.dtype != torch.int64 or tgt.dtype != torch.int64 or lengths.dtype != torch.int32 or \
                (self.mm and im.dtype != torch.float32):
            raise L.VagError("batch dtypes: src/tgt int64, lengths int32, im float32")
        n = len(srcs)
        sp = (C.c_void_p * 4)(*[t.data_ptr() for t in srcs])
        dp = (C.c_void_p * 4)(*[t.data_ptr() for t in dsts])
        nb = (C.c_int64 * 4)(*[t.numel() * t.element_size() for t in srcs])
        assert srcs[0].numel() == B * Ts and srcs[1].numel() == B * Tt and srcs[2].numel() == B
        call("vag_copy4", sp, dp, nb, n, stream())

    def load_mrt(self, cost, valid):
        """A minimum-risk step's per-row cost and validity (B,) into their static buffers (after reserve / load_batch)."""
        B = cost.numel()
        if valid.numel() != B or B > self.mrt_cost.numel():
            raise L.VagError("load_mrt: cost and valid must both hold one float per row of the loaded batch")
        self.mrt_cost[:B].copy_(cost.reshape(-1))
        self.mrt_valid[:B].copy_(valid.reshape(-1))

    def load_kd(self, idx, q):
        """A distillation step's targets idx (Tt, B, K) int32 and q (Tt, B, K) float32 into their static buffers (after reserve /
        load_batch); returns True if the buffers were re-allocated (captured graphs are then stale)."""
        n = idx.numel()
        if q.numel() != n or idx.dtype != torch.int32 or q.dtype != torch.float32:
            raise L.VagError("load_kd: idx int32 and q float32 must hold the same number of entries")
        grown = False
        if self.kd_idx is None or self.kd_idx.numel() < n:
            cap = max(n, self.cap[1] * (n // max(1, idx.shape[0] * idx.shape[1])))       # K entries per row of the largest batch seen
            self.kd_idx = torch.zeros(cap, dtype=torch.int32, device=self.dev)
            self.kd_q = torch.zeros(cap, dtype=torch.float32, device=self.dev)
            self.generation += 1
            grown = True
        self.kd_idx[:n].copy_(idx.reshape(-1))
        self.kd_q[:n].copy_(q.reshape(-1))
        return grown

    # ---- launches ----
    def refresh_derived(self):
        """Per optimiser step: the stacked / folded / transposed weights the recurrences read."""
        g = self.model.encoder.gru
        call("vag_derive_weights", self.w.dec, ptr(g.weight_hh_l0), ptr(g.weight_hh_l0_reverse), self.H,
             1 if self.storage16 else 0, ptr(self.derived), stream())

    def run(self, B, Ts, Tt, teacher, phases, mrt=None, kd=None, rdrop=None):
        m = self.model
        train = m.training
        c = self.cfg(B, Ts, Tt, teacher, train, mrt)
        rng = None
        if train and max(c.p_emb, c.p_ctx, c.p_out) > 0:
            rng = dropout_rng(m, self.dev)
        if (int(phases) & 1) and not (self.dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self.executed += 1
        if self.planes is not None:
            call("vag_set_handoff_planes", ptr(self.planes), self.planes.numel())
        try:
            args = (C.byref(self.w), C.byref(self.g), ptr(self.src, torch.int64), ptr(self.lens, torch.int32),
                    ptr(self.tgt, torch.int64), ptr(self.im) if self.mm else None, ptr(self.vw),
                    ptr(rng, torch.int64) if rng is not None else None, ptr(self.derived), ptr(self.ws), ptr(self.losses),
                    int(phases), stream())
            if rdrop is not None:
                call("vag_train_step_rdrop", c.ref(), C.byref(self.rdrop_cfg(rdrop)), *args)
            elif kd is not None:
                call("vag_train_step_kd", c.ref(), C.byref(self.kd_cfg(kd)), *args)
            else:
                call("vag_train_step", c.ref(), *args)
        finally:
            if self.planes is not None:
                call("vag_set_handoff_planes", None, 0)
