"""Minimum-risk training (Shen et al. 2016; Edunov et al. 2018): an optimiser step on the expected sentence-BLEU cost of a set of
candidate translations, in place of the token-level cross-entropy of ``TrainStep.step``.

    out = ts.mrt_step(src, lengths, tgt, im, n_candidates=16, alpha=5e-3)       # ts: a vagnmt_hip.trainer.TrainStep
    out.risk       ()    the step's risk: the mean over the sentences of sum_i Q_i (1 - BLEU_i), before the update
    out.bleu       ()    the Q-weighted mean sentence BLEU of the candidates, 1 - risk
    out.n_valid    (B,)  how many of a sentence's candidates took part.  With include_gold=False it can be 0 (every span of the
                         sentence holds the padding word): such a sentence adds 0 to the risk and nothing to the gradient, so risk
                         reads too low and bleu too high by its share -- n_valid is where that shows.  With the gold row it is >= 1.

For every source sentence: N candidates y_i (drawn on the current weights, plus the gold sentence), their scores s_i = log p(y_i | x)
from ONE forced pass of the fused step over all B N rows, Q = softmax(alpha s) over the sentence's valid candidates, the cost
c_i = 1 - smooth sentence BLEU(y_i, gold) from vag_mbr_select, and the gradient of R = sum_i Q_i c_i -- a cross-entropy gradient with
the per-row coefficient -alpha Q_i (c_i - R), which vag_mrt_weights leaves where the head's backward reads its per-sentence factor
(include/vag_nmt.h has the derivation).  Everything between the draw and the optimiser is enqueued without waiting for the host.

Candidates: ``method="stochastic"`` draws n_candidates DISTINCT translations (beamsearch_stochastic: the de-duplicated subset S(x) of
Shen et al.; at most 64), ``method="sample"`` draws with replacement (sample_decode: repeats are marked invalid), ``candidates=`` a
(B, Nc, L) int64 device tensor is used as given (off-policy sets, tests).  Decoding never applies dropout; the forced pass does, as
``step`` would.  A candidate whose span holds the padding word 0 is invalid (the loss skips that word).  The draws themselves poll
the device now and then as the decoders do.

Alternate with ``step`` freely: both drive the same flat parameters, optimiser state and graph cache (an MRT step's graphs are keyed
by (N, alpha, scale) as well).  The ranking loss is off in an MRT step (loss_vse = 0, loss_w = 1 for that call): a batch that repeats
every image N times has no negatives to rank.

    out = ts.mrt_step(src, lengths, tgt, im, cost="chrf", surface=table)      # table: vagnmt_hip.surface.Surface(words)

takes c_i = 1 - chrF(y_i, gold) on the characters the ids spell (vag_chrf_select; vagnmt_hip.mbr has the utility) in place of
1 - BLEU; everything after the costs is the same step.  MRT.bleu keeps its name and holds 1 - risk whatever the cost.

Known cost, left as it is: the encoder and the image branch run N times on identical rows.  Data-parallel MRT (world_size > 1, zero1)
and the per-operator autograd backend raise NotImplementedError: the follow-up."""
from collections import namedtuple

import torch

from vagnmt_hip import mbr, sampling, stochastic
from vagnmt_hip._lib import call, ptr, stream

MAX_CANDIDATES = 256        # rows per source sentence, the gold row included (include/vag_nmt.h: vag_mrt_weights)
METHODS = ("stochastic", "sample")
COSTS = ("bleu", "chrf")

MRT = namedtuple("MRT", ["risk", "bleu", "n_valid"])


def check_args(src, tgt, n_candidates, alpha, method, include_gold, max_length, candidates, max_rows, what="mrt_step", cost="bleu",
               surface=None):
    """Host-side checks, before anything is drawn; returns (Nc, alpha, include_gold, max_length, max_rows) as plain numbers.
    Nc is the candidates' count per sentence without the gold row.  cost "chrf" needs the vocabulary's Surface table, no other
    cost takes one, and the ids of tgt and of given candidates must lie below its V (one read of their maxima)."""
    if cost not in COSTS:
        raise ValueError("%s: cost must be one of %s, got %r" % (what, list(COSTS), cost))
    mbr.check_surface(cost, surface, what, "cost")
    if not torch.is_tensor(src) or not torch.is_tensor(tgt) or src.dim() != 2 or tgt.dim() != 2 or src.shape[0] != tgt.shape[0] or \
            tgt.dtype != torch.int64:
        raise ValueError("%s: src (B, Ts) and tgt (B, Tt) int64 tensors must share B" % what)
    a = float(alpha)
    if not (a > 0.0 and a < float("inf")):
        raise ValueError("%s: alpha must be positive and finite, got %r" % (what, alpha))
    gold = 1 if include_gold else 0
    ml = int(tgt.shape[1] if max_length is None else max_length)
    if ml < 1:
        raise ValueError("%s: max_length must be at least 1, got %d" % (what, ml))
    if candidates is not None:
        c = candidates
        if not torch.is_tensor(c) or c.dtype != torch.int64 or c.dim() != 3 or c.shape[0] != src.shape[0] or min(c.shape) < 1:
            raise ValueError("%s: candidates must be a (B, Nc, L) int64 tensor with B = %d" % (what, src.shape[0]))
        n, ml = int(c.shape[1]), int(c.shape[2])
    else:
        if method not in METHODS:
            raise ValueError("%s: method must be one of %s, got %r" % (what, list(METHODS), method))
        n = int(n_candidates)
        if method == "stochastic" and not 1 <= n <= 64:
            raise ValueError("%s: method='stochastic' draws 1 .. 64 candidates, got %d" % (what, n))
    if n < 1 or n + gold < 2 or n + gold > MAX_CANDIDATES:
        raise ValueError("%s: need 2 .. %d rows per sentence (candidates%s), got %d"
                         % (what, MAX_CANDIDATES, " + the gold row" if gold else "", n + gold))
    if ml > 511 or tgt.shape[1] > 512:
        raise ValueError("%s: candidates of up to 511 tokens, targets of up to 512: a packed row is a hypothesis of vag_mbr_select "
                         "(include/vag_nmt.h)" % what)
    if surface is not None:
        for name, t in (("tgt", tgt), ("candidates", candidates)):
            if t is not None and (int(t.min()) < 0 or int(t.max()) >= surface.V):
                raise ValueError("%s: %s must hold ids in [0, %d), the surface table's words, got [%d, %d]"
                                 % (what, name, surface.V, int(t.min()), int(t.max())))
    mr = int(max_rows)
    if mr < n + gold:
        raise ValueError("%s: max_rows=%d does not hold one sentence's %d rows" % (what, mr, n + gold))
    if not src.is_cuda or not tgt.is_cuda or (candidates is not None and not candidates.is_cuda):
        raise ValueError("%s: src, tgt and candidates must be GPU tensors (there is no CPU path)" % what)
    return n, a, gold, ml, mr


def _backend(ts, what):
    from vagnmt_hip.trainer import _FusedBackend
    if ts.world != 1 or ts.zero1 or type(ts.backend) is not _FusedBackend:
        raise NotImplementedError("%s needs the fused backend on one GPU (world_size 1, no zero1): data-parallel minimum-risk "
                                  "training is the follow-up" % what)
    if ts.backend.f.label_smoothing != 0.0 or ts.backend.f.storage16:
        raise NotImplementedError("%s: the risk is defined on the plain loss in fp32 storage (label_smoothing 0, storage 'f32')" % what)
    return ts.backend


def pack(candidates, gold, include_gold):
    """vag_mrt_pack: candidates (B, Nc, L) and gold (B, Tg) -> (rows (B N, Tt) int64 forced targets, valid (B N,) float32), N = Nc +
    include_gold, Tt = max(L + 1, Tg)."""
    B, Nc, L = candidates.shape
    Tg = gold.shape[1]
    N, Tt = Nc + include_gold, max(L + 1, Tg)
    rows = torch.empty(B * N, Tt, dtype=torch.int64, device=candidates.device)
    valid = torch.empty(B * N, dtype=torch.float32, device=candidates.device)
    call("vag_mrt_pack", ptr(candidates.contiguous(), torch.int64), B, Nc, L, ptr(gold.contiguous(), torch.int64), Tg, include_gold,
         ptr(rows, torch.int64), Tt, ptr(valid), stream())
    return rows, valid


def _draw(ts, src, lengths, im, n, ml, method, generator):
    """(B, n, ml) int64 candidates on the current weights; inference prologue, no dropout."""
    m = ts.model
    if method == "stochastic":
        return stochastic.stochastic_search(m, src, lengths, im, n, ml, generator, False, False, "mrt_step")[1]
    toks, _, _, B, n = sampling.sample_history(m, src, lengths, im, n, ml, 1.0, 0, generator, 1.0, False, "mrt_step")
    return toks.t().reshape(B, n, -1).contiguous()


def _prepare(src, lengths, tgt, im, cand, gold, surface=None):
    """Pack, cost, expand: (rows, valid, cost (B N,), N, src, lengths, im repeated N times).  The cost is 1 - smooth BLEU of every
    packed row against the gold row, or with a surface table 1 - chrF."""
    B = src.shape[0]
    rows, valid = pack(cand, tgt, gold)
    N = rows.shape[0] // B
    if surface is not None:
        bleu = mbr.run_chrf(rows.view(B, N, -1), tgt.contiguous().view(B, 1, -1), None, surface)[1]
    else:
        _, bleu, _, _ = mbr.run(rows.view(B, N, -1), tgt.contiguous().view(B, 1, -1), None, mbr.UTILITIES["bleu"])
    cost = (1.0 - bleu).reshape(-1)
    rep = lambda t: None if t is None else t.repeat_interleave(N, 0).contiguous()      # noqa: E731
    return rows, valid, cost, N, rep(src), rep(lengths), rep(im)


def _lengths(lengths, src):
    if not torch.is_tensor(lengths):
        dt = getattr(lengths, "device_tensor", None)
        lengths = dt if dt is not None else torch.tensor(list(lengths), dtype=torch.int32, device=src.device)
    return lengths.to(torch.int32)


def _run_groups(be, B, N, alpha, max_rows, rows, valid, cost, src, lengths, im, phases):
    """The forced pass over the B groups in chunks of whole groups (at most max_rows rows each), vag_step_cfg.mrt_scale = the chunk's
    share of the step; returns the sum of the chunks' risks = the step's risk."""
    per = max(1, max_rows // N)
    risk = None
    for g0 in range(0, B, per):
        g1 = min(B, g0 + per)
        sl = slice(g0 * N, g1 * N)
        be.run(src[sl], lengths[sl], rows[sl], None if im is None else im[sl], True, phases,
               mrt=(N, alpha, (g1 - g0) / B, cost[sl], valid[sl]))
        r = be.outputs()[1]
        risk = r.clone() if risk is None else risk + r
    return risk


def mrt_step(ts, src, lengths, tgt, im=None, n_candidates=16, alpha=5e-3, method="stochastic", include_gold=True, max_length=None,
             generator=None, candidates=None, max_rows=1024, cost="bleu", surface=None):
    """TrainStep.mrt_step (see the module's text).  max_length defaults to tgt.shape[1]; max_rows bounds the rows of one forced pass
    (whole sentences per pass; gradients accumulate over the passes, the optimiser runs once).  cost: "bleu", or "chrf" with
    surface, the vocabulary's Surface table.  MRT.bleu holds 1 - risk whatever the cost."""
    n, a, gold, ml, mr = check_args(src, tgt, n_candidates, alpha, method, include_gold, max_length, candidates, max_rows,
                                    "mrt_step", cost, surface)
    be = _backend(ts, "mrt_step")
    if im is None and ts.multimodal:
        raise ValueError("mrt_step: a multimodal model needs im")
    lengths = _lengths(lengths, src)
    cand = candidates if candidates is not None else _draw(ts, src, lengths, im, n, ml, method, generator)
    ts.model.train()
    rows, valid, costs, N, src_r, len_r, im_r = _prepare(src, lengths, tgt, im if ts.multimodal else None, cand, gold, surface)
    B = src.shape[0]
    risk = _run_groups(be, B, N, a, mr, rows, valid, costs, src_r, len_r, im_r, 7)
    ts._run_optimizer()                 # (bumps model._vag_weights_version, as step does)
    return MRT(risk, 1.0 - risk, valid.view(B, N).sum(1))


def expected_risk(ts, src, lengths, tgt, im, candidates, alpha, include_gold=True, max_rows=1024, cost="bleu", surface=None):
    """The risk of a fixed candidate set under the current weights: the forward phase only, no dropout, no optimiser.  A () device
    tensor.  cost, surface: as in mrt_step."""
    if candidates is None:
        raise ValueError("expected_risk: candidates must be a (B, Nc, L) int64 GPU tensor")
    n, a, gold, ml, mr = check_args(src, tgt, 1, alpha, "sample", include_gold, None, candidates, max_rows, "expected_risk", cost,
                                    surface)
    be = _backend(ts, "expected_risk")
    lengths = _lengths(lengths, src)
    was = ts.model.training
    ts.model.eval()
    try:
        rows, valid, costs, N, src_r, len_r, im_r = _prepare(src, lengths, tgt, im if ts.multimodal else None, candidates, gold,
                                                             surface)
        return _run_groups(be, src.shape[0], N, a, mr, rows, valid, costs, src_r, len_r, im_r, 1)
    finally:
        ts.model.train(was)
