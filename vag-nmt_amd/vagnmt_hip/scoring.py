"""Forced decoding: the log-probability one model or an ensemble assigns to GIVEN translations (n-best rescoring, per-sentence
perplexity, filtering data by score).

Each member runs its teacher-forced path -- the prologue, the whole-sequence cGRU (ops.cgru_decode_seq) and the head's logits with
their rows' log-sum-exp (vag_head_ce_seq_fwd) -- and ONE launch (vag_forced_score, beam.hip) reads word y_t's log-probability
logit - lse from every member, combines the members as the ensemble beam search does (include/vag_nmt.h, vag_beam_ens_step) and
reduces per sentence:

    token_logp (B, Tt)   0 at padding and after the first EOS
    logp (B,)            sum over the span up to and including the first EOS (to the last non-pad word if there is none)
    score (B,)           logp / max(1, #words > 3 in the span): the beam search's length normalisation (V11.py:315-321)
"""
import ctypes as C
from collections import namedtuple

import torch

from vagnmt_hip import ops, search
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.search import SOS_token, EOS_token, cut_nbest  # noqa: F401  (cut_nbest: this module's name for it)

Scores = namedtuple("Scores", ["score", "logp", "token_logp"])


def targets_tensor(tgt, batch, device=None):
    """(B, Tt) int64 targets from a tensor (taken as is, pad 0) or from a list of B token lists (EOS appended to a list that holds
    none, padded with 0) -- n-best output of beamsearch_nbest can be passed back flattened as it is."""
    if torch.is_tensor(tgt):
        if tgt.dim() != 2 or tgt.shape[0] != batch:
            raise ValueError("score_translations: tgt must be (B, Tt) = (%d, *), got %s" % (batch, tuple(tgt.shape)))
        if tgt.dtype != torch.int64:
            raise ValueError("score_translations: tgt must be int64, got %s" % tgt.dtype)
        return tgt.contiguous() if device is None else tgt.to(device).contiguous()
    rows = [[int(t) for t in r] for r in tgt]
    if len(rows) != batch:
        raise ValueError("score_translations: %d target lists for %d source sentences" % (len(rows), batch))
    rows = [r if EOS_token in r else r + [EOS_token] for r in rows]
    out = torch.zeros(batch, max(len(r) for r in rows), dtype=torch.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out if device is None else out.to(device)


def _member_logits(model, src_var, src_lengths, im_var, tok, tgt, rng=None):
    """Teacher-forced logits (Tt*B, ldl) and row log-sum-exp (Tt*B,) of one model (time-major rows).  rng (None: inference, no
    dropout): a device {seed, step} pair -- a model in train mode then runs its prologue and its head under the dropout masks of
    that pair (vagnmt_hip.confidence: Monte-Carlo dropout); the model's own generator is not touched."""
    dec = model.decoder
    p_out = 0.0
    if rng is None:
        enc, mask, h0 = model._decode_prologue(src_var, src_lengths, im_var)
    else:
        pro = (model._prologue(src_var, src_lengths, im_var, None, rng) if hasattr(model, "vse_imagine")
               else model._prologue(src_var, src_lengths, rng))
        enc, mask, h0 = pro[0], pro[1], pro[-1]
        p_out = float(dec.dropout_out) if model.training else 0.0
    B, Tt = tgt.shape
    V = dec.out.bias.shape[0]
    ldl = (V + 3) // 4 * 4
    E = dec.embedding.weight.shape[1]
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
    H = h2.shape[2]
    R = Tt * B
    dev = enc.device
    tmid = torch.empty(Tt, B, E, device=dev)
    logits = torch.empty(R, ldl, device=dev)
    lse = torch.empty(R, device=dev)
    nll = torch.empty(R, device=dev)
    inv_cnt = torch.empty(B, device=dev)
    loss = torch.empty(1, device=dev)
    vw = torch.ones(V, device=dev)
    call("vag_head_ce_seq_fwd", ptr(h2), ptr(c), ptr(e), ops._head_w(dec.head_params()), ptr(tgt, torch.int64), ptr(vw), B, Tt,
         E, H, V, p_out, ptr(rng, torch.int64) if rng is not None else None, 0, ptr(tmid), ptr(logits), ldl, ptr(lse), ptr(nll),
         ptr(inv_cnt), ptr(loss), stream())
    return logits, lse


def forced_args(models, multimodal, src_var, tgt, im_var, what="score_translations"):
    """Host-side checks of forced decoding (score_translations, align_translations); returns the targets (B, Tt) on the device
    and the decoder's inputs tok (Tt+1, B): SOS, then the targets (the inputs of steps 0..Tt-1, +1 unused row)."""
    if not torch.is_tensor(src_var) or not src_var.is_cuda:
        raise ValueError("%s: src_var must be a GPU tensor (there is no CPU path)" % what)
    if im_var is None and any(multimodal):
        raise ValueError("%s: a multimodal model needs im_var" % what)
    B = src_var.shape[0]
    V = int(models[0].tgt_size)
    tgt = targets_tensor(tgt, B, src_var.device)
    if not tgt.is_cuda:
        raise ValueError("%s: tgt must be on the GPU with src_var" % what)
    if tgt.shape[1] < 1:
        raise ValueError("%s: empty targets" % what)
    lo, hi = int(tgt.min()), int(tgt.max())
    if lo < 0 or hi >= V:
        raise ValueError("%s: target words must lie in [0, %d), got [%d, %d]" % (what, V, lo, hi))
    sos = torch.full((1, B), SOS_token, dtype=torch.int64, device=tgt.device)
    return tgt, torch.cat([sos, tgt.t()], 0).contiguous()


def score_models(models, multimodal, src_var, src_lengths, tgt, im_var=None):
    """score_translations of one model (M = 1) or of an ensemble's members; returns Scores(score, logp, token_logp)."""
    tgt, tok = forced_args(models, multimodal, src_var, tgt, im_var)
    B, Tt = tgt.shape
    V = int(models[0].tgt_size)
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()                                          # inference: no dropout whatever the models' modes
        with torch.no_grad():
            outs = [_member_logits(m, src_var, src_lengths, im_var, tok, tgt) for m in models]
            token_logp = torch.empty(B, Tt, device=tgt.device)
            logp = torch.empty(B, device=tgt.device)
            score = torch.empty(B, device=tgt.device)
            M = len(outs)
            call("vag_forced_score", (C.c_void_p * M)(*[ptr(o[0]) for o in outs]),
                 (C.c_int64 * M)(*[o[0].shape[1] for o in outs]), (C.c_void_p * M)(*[ptr(o[1]) for o in outs]), M,
                 ptr(tgt, torch.int64), B, Tt, V, ptr(token_logp), ptr(logp), ptr(score), stream())
    finally:
        for m, t in zip(models, modes):
            m.train(t)
    return Scores(score, logp, token_logp)


def models_of(obj):
    """(models, multimodal) of a model, an Ensemble or a TrainStep (its model, whatever weights it holds at the moment)."""
    if hasattr(obj, "backend") and hasattr(obj, "model"):
        obj = obj.model
    models = list(obj.models) if hasattr(obj, "models") else [obj]
    return models, [hasattr(m, "vse_imagine") for m in models]


def vocab_of(obj):
    """The target vocabulary's size of a model or an Ensemble."""
    return int(models_of(obj)[0][0].tgt_size)


def nbest_search(obj, src_var, src_lengths, im_var, k, max_length, flags, n_best, align=False):
    """The plain beam search of a model or an Ensemble on checked arguments, as their _beam runs it: beamsearch_align, and what
    beamsearch_knn / beamsearch_lm are at lam = 0 / beta = 0 without constraints.  Returns search.beam's result."""
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, max_length, "beam", flags, align)
        return obj._search_done(search.beam(s.members, s.h0s, k, max_length, flags, n_best, s.entry, s.pool,
                                            raw_logits=s.raw_logits, align=align), k)


def nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what="beamsearch_nbest"):
    """Host-side checks of beamsearch_nbest (and of beamsearch_align, which names itself in ``what``); returns (k, n, flags)."""
    k, n = int(beam_size), int(n_best)
    if not (1 <= n <= k <= 64):
        raise ValueError("%s: need 1 <= n_best <= beam_size <= 64, got n_best=%d beam_size=%d" % (what, n, k))
    if not torch.is_tensor(src_var) or not src_var.is_cuda:
        raise ValueError("%s: src_var must be a GPU tensor (there is no CPU path)" % what)
    return k, n, beam_flags(avoid_double, avoid_unk)


def beam_flags(avoid_double=True, avoid_unk=False):
    """The reference's beamsearch options as the expansion kernels' flags (include/vag_nmt.h: VAG_BEAM_ALLOW_REPEAT = 1,
    VAG_BEAM_AVOID_UNK = 2); 0 = the defaults."""
    return (0 if avoid_double else 1) | (2 if avoid_unk else 0)

