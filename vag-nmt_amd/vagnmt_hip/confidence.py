"""Word-level and sentence-level confidence from forced decoding: how sure one model or an ensemble was of every word of GIVEN
translations -- the glass-box features of unsupervised quality estimation (Fomicheva et al. 2020), the inputs of data filtering and
calibration checks, and corpus perplexity.

Each member runs the teacher-forced path of vagnmt_hip.scoring (prologue, whole-sequence cGRU, the head's logits and their rows'
log-sum-exp) and ONE call (vag_token_conf, conf.hip: a row kernel that reads every member's (Tt*B, ldl) logits once, and a sentence
kernel) writes, with s_j the ensemble's log-probability of word j and y the given word:

    token_logp (B, Tt)    s_y: score_translations' token_logp, bit for bit
    entropy (B, Tt)       -sum_j exp(s_j) s_j, nats
    rank (B, Tt) int32    the number of words ahead of y under (score descending, word ascending); 0 = the model's first choice
    top (B, Tt, 2) int32, top_logp (B, Tt, 2)    the best and the second-best word and their s
    sentence (B, 8)       logp, score (score_translations'), n, std and min of token_logp, mean and max entropy, share of rank == 0

Outside the scored span (scoring: up to and including the first EOS) floats are 0 and integers -1.  Nothing here touches training,
``validate()`` or the scoring path itself.  Not here: D-Lex-Sim, which needs DECODING under dropout (a search, not a forced pass).
"""
import ctypes as C
from collections import namedtuple

import torch

from vagnmt_hip import scoring
from vagnmt_hip._lib import call, ptr, stream

SENT = 8                # VAG_CONF_SENT (include/vag_nmt.h)
SENT_FIELDS = ("logp", "score", "n", "std_logp", "min_logp", "mean_entropy", "max_entropy", "top1_share")

Confidence = namedtuple("Confidence", ["score", "logp", "token_logp", "entropy", "rank", "top", "top_logp", "sentence"])
MCDropout = namedtuple("MCDropout", ["token_logp", "score", "mean_score", "var_score", "combo"])
Perplexity = namedtuple("Perplexity", ["ppl", "logp", "n_tokens"])


def _conf_call(outs, tgt, V):
    """vag_token_conf on the members' (logits, lse) -> Confidence, all on the device."""
    B, Tt = tgt.shape
    dev = tgt.device
    token_logp = torch.empty(B, Tt, device=dev)
    entropy = torch.empty(B, Tt, device=dev)
    rank = torch.empty(B, Tt, dtype=torch.int32, device=dev)
    top = torch.empty(B, Tt, 2, dtype=torch.int32, device=dev)
    top_logp = torch.empty(B, Tt, 2, device=dev)
    sent = torch.empty(B, SENT, device=dev)
    M = len(outs)
    call("vag_token_conf", (C.c_void_p * M)(*[ptr(o[0]) for o in outs]), (C.c_int64 * M)(*[o[0].shape[1] for o in outs]),
         (C.c_void_p * M)(*[ptr(o[1]) for o in outs]), M, ptr(tgt, torch.int64), B, Tt, V, ptr(token_logp), ptr(entropy),
         ptr(rank, torch.int32), ptr(top, torch.int32), ptr(top_logp), ptr(sent), stream())
    return Confidence(sent[:, 1], sent[:, 0], token_logp, entropy, rank, top, top_logp, sent)


def token_confidence(models, multimodal, src_var, src_lengths, tgt, im_var=None):
    """Confidence(score (B,), logp (B,), token_logp, entropy, rank, top, top_logp, sentence (B, 8)) of the given targets -- a
    (B, Tt) int64 tensor (pad 0) or B token lists, as for score_translations.  Device tensors, no host sync beyond the argument
    checks of forced decoding.  Inference only: the members run in eval mode under no_grad and their modes are restored."""
    tgt, tok = scoring.forced_args(models, multimodal, src_var, tgt, im_var, what="token_confidence")
    V = int(models[0].tgt_size)
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            outs = [scoring._member_logits(m, src_var, src_lengths, im_var, tok, tgt) for m in models]
            return _conf_call(outs, tgt, V)
    finally:
        for m, was in zip(models, modes):
            m.train(was)


def translation_confidence(obj, src_var, src_lengths, im_var, beam_size=12, n_best=1, max_length=80):
    """Translate, then say how sure the model was: beamsearch_nbest, then token_confidence of the B * n_best hypotheses (sentence
    b's n_best lists in a row, sources repeated n_best times).  Returns (hyps, Confidence) with B * n_best rows."""
    models, multimodal = scoring.models_of(obj)
    text_model = not hasattr(obj, "models") and not multimodal[0]
    args = (src_var, src_lengths) if text_model else (src_var, src_lengths, im_var)
    hyps, _ = obj.beamsearch_nbest(*args, beam_size=beam_size, n_best=n_best, max_length=max_length)
    n = int(n_best)
    flat = [list(h) for per in hyps for h in per]
    lens = [int(x) for x in (src_lengths.tolist() if torch.is_tensor(src_lengths) else src_lengths) for _ in range(n)]
    src_n = src_var.repeat_interleave(n, 0)
    im_n = im_var.repeat_interleave(n, 0) if im_var is not None else None
    return hyps, token_confidence(models, multimodal, src_n, lens, flat, im_n)


def mc_dropout_confidence(obj, src_var, src_lengths, tgt, im_var=None, passes=8, seed=0, step=0):
    """Monte-Carlo dropout over the forced pass: ``passes`` runs with the members in TRAIN mode (dropout on: the encoder's and the
    head's masks), each under the masks of a device {seed, step} pair owned by this call and advanced before every pass: pass i runs
    at step + 1 + i, so pass i of an N-pass call is a 1-pass call with ``step=i``.  The models' own generators, a TrainStep's state and
    Python's ``random`` are not touched; the members' modes are restored.
    Returns MCDropout(token_logp (N, B, Tt), score (N, B), mean_score (B,), var_score (B,), combo (B,)): the expectation and the
    variance of the length-normalised score over the passes (D-TP, D-Var) and combo = 1 - mean_score / var_score (D-Combo)."""
    models, multimodal = scoring.models_of(obj)
    N = int(passes)
    if N < 1 or N != passes:
        raise ValueError("mc_dropout_confidence: passes must be a whole number >= 1, got %r" % (passes,))
    tgt, tok = scoring.forced_args(models, multimodal, src_var, tgt, im_var, what="mc_dropout_confidence")
    V = int(models[0].tgt_size)
    rng = torch.tensor([int(seed), int(step)], dtype=torch.int64, device=tgt.device)
    modes = [m.training for m in models]
    toks, scores = [], []
    try:
        for m in models:
            m.train()
        with torch.no_grad():
            for _ in range(N):
                call("vag_rng_advance", ptr(rng, torch.int64), stream())
                outs = [scoring._member_logits(m, src_var, src_lengths, im_var, tok, tgt, rng=rng) for m in models]
                c = _conf_call(outs, tgt, V)
                toks.append(c.token_logp)
                scores.append(c.score)
    finally:
        for m, was in zip(models, modes):
            m.train(was)
    score = torch.stack(scores)
    mean = score.mean(0)
    var = score.var(0, unbiased=False)
    return MCDropout(torch.stack(toks), score, mean, var, 1.0 - mean / var)


def corpus_perplexity(obj, batches):
    """Perplexity(ppl, logp, n_tokens) of an iterable of (src, lengths, tgt[, im]) batches: exp(-sum logp / sum n) over the
    scored spans, the two sums kept on the device in float64 and read once at the end.  ``obj``: a model, an Ensemble or a
    TrainStep (its model under the weights it holds: inside ``averaged_weights()`` the averaged ones)."""
    models, multimodal = scoring.models_of(obj)
    total = None
    for batch in batches:
        src, lens, tgt = batch[:3]
        im = batch[3] if len(batch) > 3 else None
        s = token_confidence(models, multimodal, src, lens, tgt, im).sentence[:, [0, 2]].double().sum(0)
        total = s if total is None else total + s
    if total is None:
        raise ValueError("corpus_perplexity: no batches")
    logp, n = (float(x) for x in total.tolist())
    if n <= 0:
        raise ValueError("corpus_perplexity: no scored words")
    import math
    return Perplexity(math.exp(-logp / n), logp, int(n))


def calibration(conf, bins=10):
    """Expected calibration error of the model's first choice over the span positions of a Confidence: positions are binned by
    their confidence exp(top_logp[.., 0]) into ``bins`` equal bins of [0, 1]; a bin's accuracy is its share of rank == 0 (the given
    word IS the first choice).  Returns (ece, bin_conf, bin_acc, bin_count): ece = sum_b count_b / N |acc_b - conf_b|, the three
    (bins,) tensors in float64 (an empty bin: 0).  Torch only."""
    bins = int(bins)
    if bins < 1:
        raise ValueError("calibration: bins must be >= 1")
    span = conf.rank >= 0
    p = conf.top_logp[..., 0][span].double().exp()
    hit = (conf.rank[span] == 0).double()
    which = (p * bins).long().clamp_(0, bins - 1)
    count = torch.zeros(bins, dtype=torch.float64, device=p.device).index_add_(0, which, torch.ones_like(p))
    csum = torch.zeros_like(count).index_add_(0, which, p)
    asum = torch.zeros_like(count).index_add_(0, which, hit)
    safe = count.clamp(min=1)
    bin_conf, bin_acc = csum / safe, asum / safe
    ece = ((count / count.sum().clamp(min=1)) * (bin_acc - bin_conf).abs()).sum()
    return ece, bin_conf, bin_acc, count
