"""Word-level knowledge distillation (Kim & Rush 2016, section 3.1): train a student on a teacher's per-position distribution.

The teacher -- one model or an ``Ensemble`` -- runs its teacher-forced path on the batch (the members' logits and their rows'
log-sum-exp, as forced decoding forms them) and ONE launch (vag_kd_targets, distill.hip) keeps, per target position, the ``top_k``
<= 64 best words of the ensemble's distribution and their probabilities at ``temperature``, renormalised:

    SoftTargets(idx (Tt, B, K) int32, q (Tt, B, K) float32)        rows time-major, best word first, sum_k q = 1

``TrainStep.distill_step`` is then the teacher-forced fused step with the translation loss

    nll[t, b] = w[y] * ( (1 - kd_lambda) * CE(gold y) + kd_lambda * CE(teacher's K words) )          (include/vag_nmt.h)

-- the V-wide kernels of the plain loss plus two small launches per pass of the head that touch K + 1 logits of a row -- and one
optimiser call.  A multimodal student keeps its ranking loss.  Targets of a fixed teacher can be computed once and passed back as
``soft=``.  A teacher may be another ``TrainStep``'s model inside its ``averaged_weights()`` block.

Each follow-up is refused with NotImplementedError today: the per-operator autograd backend, data-parallel (world_size > 1) and zero1
distillation, the 2-byte storage mode, and a label-smoothed criterion.  Sequence-level distillation needs none of this: beam-search
the teacher and train on its output with ``step``."""
import ctypes as C
from collections import namedtuple

import torch

from vagnmt_hip._lib import call, ptr, stream

SoftTargets = namedtuple("SoftTargets", ["idx", "q"])

MAX_K = 64


def check_kd(kd_lambda, top_k, temperature, what="distill_step"):
    """(lambda, K, T) as numbers, or ValueError: 0 < lambda <= 1, 1 <= K <= 64, T > 0 and finite."""
    lam, k, t = float(kd_lambda), int(top_k), float(temperature)
    if not 0.0 < lam <= 1.0:                                   # (NaN fails)
        raise ValueError("%s: kd_lambda must lie in (0, 1], got %r" % (what, kd_lambda))
    if not 1 <= k <= MAX_K or k != top_k:
        raise ValueError("%s: top_k must be a whole number in 1 .. %d, got %r" % (what, MAX_K, top_k))
    if not 0.0 < t < float("inf"):
        raise ValueError("%s: temperature must be positive and finite, got %r" % (what, temperature))
    return lam, k, t


def teacher_targets(teacher, src_var, src_lengths, tgt, im_var=None, top_k=8, temperature=1.0, vocab_size=None):
    """The teacher's soft targets for targets ``tgt`` (B, Tt): SoftTargets(idx (Tt, B, K) int32, q (Tt, B, K) float32).  ``teacher``:
    a model or an Ensemble; it runs in eval mode under no_grad and its members' modes are restored.  vocab_size: the target
    vocabulary the caller is going to train on; a teacher over another one is refused."""
    from vagnmt_hip import scoring
    _, k, t = check_kd(1.0, top_k, temperature, "teacher_targets")
    models, multimodal = scoring.models_of(teacher)
    V = int(models[0].tgt_size)
    if vocab_size is not None and int(vocab_size) != V:
        raise ValueError("teacher_targets: the teacher's target vocabulary has %d words, the caller's %d" % (V, int(vocab_size)))
    if k > V:
        raise ValueError("teacher_targets: top_k=%d exceeds the vocabulary (%d words)" % (k, V))
    tgt, tok = scoring.forced_args(models, multimodal, src_var, tgt, im_var, what="teacher_targets")
    B, Tt = tgt.shape
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()                                           # inference: no dropout whatever the models' modes
        with torch.no_grad():
            outs = [scoring._member_logits(m, src_var, src_lengths, im_var, tok, tgt) for m in models]
            idx = torch.empty(Tt, B, k, dtype=torch.int32, device=tgt.device)
            q = torch.empty(Tt, B, k, dtype=torch.float32, device=tgt.device)
            M = len(outs)
            call("vag_kd_targets", (C.c_void_p * M)(*[ptr(o[0]) for o in outs]), (C.c_int64 * M)(*[o[0].shape[1] for o in outs]),
                 (C.c_void_p * M)(*[ptr(o[1]) for o in outs]), M, Tt * B, V, k, t, ptr(idx, torch.int32), ptr(q), stream())
    finally:
        for m, was in zip(models, modes):
            m.train(was)
    idx._vag_kd_checked = (V, idx._version)                    # the kernel's own output: distinct words inside [0, V)
    return SoftTargets(idx, q)


def _backend(ts):
    from vagnmt_hip.trainer import _FusedBackend
    if type(ts.backend) is not _FusedBackend:
        raise NotImplementedError("distill_step needs the fused backend: distillation through the per-operator autograd path is "
                                  "a follow-up")
    if ts.world != 1 or ts.zero1:
        raise NotImplementedError("distill_step runs on one GPU (world_size 1, no zero1): data-parallel and ZeRO-1 distillation "
                                  "are follow-ups")
    if ts.backend.f.storage16:
        raise NotImplementedError("distill_step: the 2-byte storage mode is a follow-up (its bf16 d(logits) has no correction)")
    if ts.backend.f.label_smoothing != 0.0:
        raise NotImplementedError("distill_step: combining distillation with a label-smoothed criterion is a follow-up")
    return ts.backend


def check_soft(soft, B, Tt, V, k=None):
    """SoftTargets for a (B, Tt) batch over V words: shapes, dtypes, words inside [0, V) and distinct within a row.  The look at
    the words costs a sort and a host sync: it is made once per tensor (and again after an in-place change of it)."""
    idx, q = soft
    if not (torch.is_tensor(idx) and torch.is_tensor(q)) or idx.dtype != torch.int32 or q.dtype != torch.float32:
        raise ValueError("distill_step: soft must be SoftTargets(idx int32, q float32)")
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (Tt, B) or q.shape != idx.shape or not 1 <= idx.shape[2] <= min(MAX_K, V):
        raise ValueError("distill_step: soft.idx and soft.q must be (Tt, B, K) = (%d, %d, 1 .. %d), got %s and %s"
                         % (Tt, B, min(MAX_K, V), tuple(idx.shape), tuple(q.shape)))
    if k is not None and idx.shape[2] != k:
        raise ValueError("distill_step: soft holds %d words per position, top_k=%d" % (idx.shape[2], k))
    if not (idx.is_cuda and q.is_cuda):
        raise ValueError("distill_step: soft must be on the GPU (there is no CPU path)")
    if getattr(idx, "_vag_kd_checked", None) != (V, idx._version):
        s = idx.sort(dim=2).values
        if int(s[..., 0].min()) < 0 or int(s[..., -1].max()) >= V or (idx.shape[2] > 1 and bool((s[..., 1:] == s[..., :-1]).any())):
            raise ValueError("distill_step: the words of a position must be distinct and lie in [0, %d)" % V)
        idx._vag_kd_checked = (V, idx._version)
    return idx.contiguous(), q.contiguous()


def distill_step(ts, src, lengths, tgt, im=None, teacher_model=None, soft=None, kd_lambda=0.5, top_k=8, temperature=1.0):
    """TrainStep.distill_step (see the module's text): always teacher-forced, one optimiser call, returns (loss, loss_mt,
    loss_vse) as ``step`` does.  Exactly one of teacher_model (a model or an Ensemble, evaluated here on this batch) and soft
    (precomputed SoftTargets; top_k is then read from it) is given."""
    lam, k, t = check_kd(kd_lambda, top_k, temperature)
    if (teacher_model is None) == (soft is None):
        raise ValueError("distill_step: give exactly one of teacher_model and soft")
    if not torch.is_tensor(src) or not torch.is_tensor(tgt) or src.dim() != 2 or tgt.dim() != 2 or src.shape[0] != tgt.shape[0] \
            or tgt.dtype != torch.int64:
        raise ValueError("distill_step: src (B, Ts) and tgt (B, Tt) int64 must share B")
    be = _backend(ts)
    if im is None and ts.multimodal:
        raise ValueError("distill_step: a multimodal model needs im")
    if not src.is_cuda or not tgt.is_cuda:
        raise ValueError("distill_step: src and tgt must be GPU tensors (there is no CPU path)")
    V = be.f.V
    B, Tt = tgt.shape
    if soft is None:
        soft = teacher_targets(teacher_model, src, lengths, tgt, im, k, t, vocab_size=V)
        idx, q = soft.idx, soft.q
    else:
        idx, q = check_soft(soft, B, Tt, V)
        k = idx.shape[2]
    ts.model.train()
    # (see TrainStep.step: the optimiser writes the parameters through the flat buffer, this counter tells the decode caches)
    ts.model._vag_weights_version = getattr(ts.model, "_vag_weights_version", 0) + 1
    if not torch.is_tensor(lengths):
        dt = getattr(lengths, "device_tensor", None)
        lengths = dt if dt is not None else torch.tensor(list(lengths), dtype=torch.int32, device=src.device)
    lengths = lengths.to(torch.int32)
    kd = (k, lam, idx, q)
    if ts.use_graph:
        be.run(src, lengths, tgt.contiguous(), im, True, 7, optimizer=True, kd=kd)      # forward, backward, optimiser: one graph
        return be.outputs()
    be.run(src, lengths, tgt.contiguous(), im, True, 7, kd=kd)
    out = be.outputs()
    ts._run_optimizer()
    return out
