import math

import torch


class LabelSmoothedNLLLoss(torch.nn.Module):
    """Label-smoothed, row-weighted negative log-likelihood, one value per row (no reduction):

        loss[n] = weight[y_n] * ( (1 - eps) * (-logp[n, y_n]) + eps * mean_j(-logp[n, j]) ),   eps = label_smoothing

    With unit weights this is ``F.cross_entropy(logits, y, reduction='none', label_smoothing=eps)``; the weight of the
    row's target multiplies the whole row, so rows whose target has weight 0 (PAD in the reference's vocabulary weight)
    contribute nothing -- the role ``ignore_index`` plays in torch.  eps = 0 is ``nn.NLLLoss(weight, reduction='none')``.

    Passed as ``criterion_mt`` (``criterion`` of the text-only model) it is recognised BY EXACT TYPE, like ``nn.NLLLoss``:
    the fused training step and the one-call output head then compute this loss in their HIP kernels
    (include/vag_nmt.h: vag_head_ce_seq_fwd_ls, vag_step_cfg.label_smoothing).  ``forward`` below is the executable definition
    in plain torch ops -- any device, any floating dtype -- and what a subclass, which takes the generic per-step criterion
    path, is evaluated with."""

    def __init__(self, weight, label_smoothing=0.1):
        super(LabelSmoothedNLLLoss, self).__init__()
        if weight is None:
            raise ValueError("LabelSmoothedNLLLoss needs the vocabulary weight vector (as nn.NLLLoss(weight=...))")
        eps = float(label_smoothing)
        if math.isnan(eps) or not (0.0 <= eps < 1.0):
            raise ValueError("label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
        self.register_buffer("weight", torch.as_tensor(weight))
        self.label_smoothing = eps

    def forward(self, logp, target):
        """logp (N, V) log-probabilities, target (N,) int64 -> (N,) per-row loss."""
        eps = self.label_smoothing
        nll = -logp.gather(1, target.unsqueeze(1)).squeeze(1)
        w = self.weight.to(logp.dtype)[target]
        if eps == 0.0:
            return w * nll
        return w * ((1.0 - eps) * nll + eps * (-logp.mean(1)))
