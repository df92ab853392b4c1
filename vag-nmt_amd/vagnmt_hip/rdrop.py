"""R-Drop (Liang et al. 2021, "R-Drop: Regularized Dropout for Neural Networks"): close the gap between training under heavy dropout
and inference without it.

``TrainStep.rdrop_step`` puts every sentence of the batch TWICE into one teacher-forced fused step, in adjacent rows
(``repeat_interleave(2, 0)``, the layout ``mrt_step`` uses for its candidates).  The counter-based dropout is indexed by element, so
the two copies run under two different masks.  At every target position the two predicted distributions are pulled together:

    kl[t, r]  = KL(p_r || p_twin)                                              twin of row r: r ^ 1
    nll[t, r] = CE(row, label smoothing included) + w[y] * (alpha / 4) * (kl[t, r] + kl[t, twin])          (include/vag_nmt.h)

Per sentence that is mean(CE_1, CE_2) + (alpha / 2) * KL_sym / count, half of the paper's CE_1 + CE_2 + alpha * KL_sym: ``alpha`` is
the paper's (5 for translation).  Both directions carry gradient.  A multimodal model keeps its ranking loss; a twin is neither a
positive nor a negative of its sibling there, and the loss is scaled so that without dropout it is the plain step's.  The optimiser
runs once; EMA, checkpoints and ``check()`` work as in ``step``; a ``LabelSmoothedNLLLoss`` criterion is allowed.

    RDrop(loss, loss_mt, loss_vse, kl)        kl: (Tt, 2B) view of the step's static buffer, valid until the next rdrop_step

Each follow-up is refused with NotImplementedError today: the per-operator autograd backend, data-parallel (world_size > 1) and zero1
steps, the 2-byte storage mode.  Not built: a detached (one-directional) KL, more than two passes, the free-running step."""
import math
from collections import namedtuple

import torch

RDrop = namedtuple("RDrop", ["loss", "loss_mt", "loss_vse", "kl"])


def check_alpha(alpha, what="rdrop_step"):
    """alpha as a float, or ValueError: positive and finite ("no R-Drop" is ``step``)."""
    a = float(alpha)
    if not (a > 0.0 and math.isfinite(a)):                     # (NaN fails)
        raise ValueError("%s: alpha must be positive and finite, got %r (no R-Drop is step())" % (what, alpha))
    return a


def _backend(ts):
    from vagnmt_hip.trainer import _FusedBackend
    if type(ts.backend) is not _FusedBackend:
        raise NotImplementedError("rdrop_step needs the fused backend: R-Drop through the per-operator autograd path is a follow-up")
    if ts.world != 1 or ts.zero1:
        raise NotImplementedError("rdrop_step runs on one GPU (world_size 1, no zero1): data-parallel and ZeRO-1 R-Drop are "
                                  "follow-ups")
    if ts.backend.f.storage16:
        raise NotImplementedError("rdrop_step: the 2-byte storage mode is a follow-up (its bf16 d(logits) has no R-Drop form)")
    return ts.backend


def twins(t):
    """Every row twice, in adjacent rows (None stays None)."""
    return None if t is None else t.repeat_interleave(2, 0).contiguous()


def mean_kl(out, tgt):
    """The per-token mean of the symmetric KL of an ``RDrop`` result over the non-PAD positions of ``tgt`` (B, Tt): a () tensor,
    computed in torch outside the step (``out.kl`` is overwritten by the next rdrop_step)."""
    kl = out.kl if isinstance(out, RDrop) else out
    Tt, Bt = kl.shape
    if tgt.dim() != 2 or tgt.shape[0] * 2 != Bt or tgt.shape[1] != Tt:
        raise ValueError("mean_kl: kl (Tt, 2B) = %s does not belong to tgt (B, Tt) = %s" % (tuple(kl.shape), tuple(tgt.shape)))
    mask = (tgt != 0).t().to(kl.dtype)                         # (Tt, B)
    sym = 0.5 * (kl[:, 0::2] + kl[:, 1::2])
    return (sym * mask).sum() / mask.sum().clamp(min=1)


def rdrop_step(ts, src, lengths, tgt, im=None, alpha=5.0):
    """TrainStep.rdrop_step (see the module's text): duplicates the batch on the device, one teacher-forced fused step on the 2B rows
    (the coin flip of ``teacher_force_ratio`` is not used), one optimiser call.  Returns RDrop(loss, loss_mt, loss_vse, kl)."""
    a = check_alpha(alpha)
    if not torch.is_tensor(src) or not torch.is_tensor(tgt) or src.dim() != 2 or tgt.dim() != 2 or src.shape[0] != tgt.shape[0] \
            or tgt.dtype != torch.int64:
        raise ValueError("rdrop_step: src (B, Ts) and tgt (B, Tt) int64 must share B")
    be = _backend(ts)
    if im is None and ts.multimodal:
        raise ValueError("rdrop_step: a multimodal model needs im")
    if not src.is_cuda or not tgt.is_cuda:
        raise ValueError("rdrop_step: src and tgt must be GPU tensors (there is no CPU path)")
    ts.model.train()
    # (see TrainStep.step: the optimiser writes the parameters through the flat buffer, this counter tells the decode caches)
    ts.model._vag_weights_version = getattr(ts.model, "_vag_weights_version", 0) + 1
    if not torch.is_tensor(lengths):
        dt = getattr(lengths, "device_tensor", None)
        lengths = dt if dt is not None else torch.tensor(list(lengths), dtype=torch.int32, device=src.device)
    lengths = lengths.to(torch.int32)
    B, Tt = tgt.shape
    args = (twins(src), twins(lengths), twins(tgt), twins(im) if ts.multimodal else None, True, 7)      # (sorted lengths stay sorted)
    if ts.use_graph:
        be.run(*args, optimizer=True, rdrop=(a,))              # forward, backward, optimiser: one graph
    else:
        be.run(*args, rdrop=(a,))
    out = be.outputs()
    if not ts.use_graph:
        ts._run_optimizer()
    return RDrop(out[0], out[1], out[2], be.f.rd_kl[:Tt * 2 * B].view(Tt, 2 * B))
