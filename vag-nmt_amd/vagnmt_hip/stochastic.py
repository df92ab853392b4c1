"""Stochastic beam search (Kool, van Hoof, Welling 2019, "Stochastic Beams and Where to Find Them"): n_samples DISTINCT
translations per sentence that are an exact sample WITHOUT replacement from one model's or an ensemble's sequence distribution.
sample_decode draws with replacement -- on peaked distributions many draws are the same translation; the beam searches give
distinct hypotheses that are not samples.  This is a beam search over Gumbel-perturbed scores: it returns the translations in
sampling order together with the importance weights that make weighted estimates (an expected utility, say) unbiased.

    gen = Generator(1234)
    s = model.beamsearch_stochastic(src_var, src_lengths, im_var, n_samples=12, generator=gen)
    s.hyps[b][i]          sample i of sentence b, a token list cut at EOS; pairwise distinct within a sentence
    s.logp (B, n)         the model's total log-probability of each (what score_translations gives)
    s.score (B, n)        its length-normalised form, the beam searches' score
    s.gumbel (B, n)       the perturbed score G of each, descending: the sampling order (sbs_uncondition of the search's values)
    s.log_weight (B, n)   log importance weights, sbs_log_weights(logp, gumbel): -inf for the last sample, whose G is the threshold

The expansion is vag_beam_sbs_step (include/vag_nmt.h states the rule; the search on the host is
vagnmt_hip.search.beam_stochastic), on models and on Ensemble alike.  The generator is sample_decode's (vagnmt_hip.sampling) and
advances the same way: once per call; the same state gives the same samples.  avoid_double defaults to False here, unlike the
beam searches: the draw is from the model's own distribution.  Temperature, top_k and top_p are out of scope: a tempered or
truncated SEQUENCE distribution needs every step's row renormalised before it is perturbed, which the expansion does not do.
A sample that reached max_length without EOS is a prefix: its logp is the prefix's probability, and two such samples may differ
only in the last word, which the finish overwrites with EOS."""
from collections import namedtuple

import torch

from vagnmt_hip import sampling, scoring, search
from vagnmt_hip.scoring import beam_flags

Stochastic = namedtuple("Stochastic", ["hyps", "logp", "score", "gumbel", "log_weight"])


def sbs_log_weights(logp, gumbel):
    """Log importance weights of a sample without replacement (Kool et al. 2019, section 4.2).  logp, gumbel: (B, k) tensors on any
    device, every sentence's k samples with their total log-probabilities and perturbed scores.  The threshold kappa is the
    sentence's k-th (smallest) G; a sample with G > kappa was included with probability q = P(G_phi > kappa) = 1 - exp(-exp(logp -
    kappa)) and gets log w = logp - log q; the k-th sample itself gets -inf (weight 0).  k = 1: the single sample gets 0.
    log q is formed as log(-expm1(-e)), e = exp(logp - kappa), and for e below 1e-4 as log(e) + log1p(-e / 2 + e^2 / 6) (the series of
    -expm1(-e) = e (1 - e/2 + e^2/6 - ...)): finite and accurate when logp - kappa is large in either direction."""
    if logp.shape != gumbel.shape or logp.dim() != 2:
        raise ValueError("sbs_log_weights: logp and gumbel must both be (B, k), got %s and %s" % (tuple(logp.shape), tuple(gumbel.shape)))
    k = logp.shape[1]
    if k == 1:
        return torch.zeros_like(logp)
    kappa, last = gumbel.min(dim=1, keepdim=True)
    x = logp - kappa
    e = torch.exp(x)
    log_q = torch.where(e < 1e-4, x + torch.log1p(e * (e / 6.0 - 0.5)), torch.log(-torch.expm1(-e)))
    w = logp - log_q
    drop = torch.zeros_like(w, dtype=torch.bool).scatter_(1, last, True)
    return torch.where(drop, torch.full_like(w, float("-inf")), w)


def sbs_uncondition(gumbel, top):
    """The search's perturbed scores with the conditioning on their maximum taken out.  The expansion starts from a root with
    G = 0, and a row's best child inherits its parent's G exactly: the largest G of every sentence is 0, and the others are
    distributed as independent Gumbel(logp) variables CONDITIONED on that maximum.  The estimator of sbs_log_weights needs them
    unconditioned.  With top (B, 1) one fresh Gumbel(0) draw per sentence -- the value the maximum would have had -- the exact
    coupling between the two truncations is G' = -log(exp(-top) + exp(-G) - 1) for G relative to the maximum: the largest G
    becomes top, the order is kept, and the G' are independent Gumbel(logp) draws given their order.  Pure torch, any device."""
    G = gumbel - gumbel.max(dim=1, keepdim=True)[0]
    b = torch.where(G > -0.6931472, torch.log(torch.expm1(-G)), -G + torch.log1p(-torch.exp(G)))     # log(exp(-G) - 1); -inf at G = 0
    return -torch.logaddexp(-top.to(G.dtype).reshape(-1, 1).expand_as(G), b)


def stochastic_args(src_var, n_samples, max_length, avoid_double, avoid_unk, vocab=None, what="beamsearch_stochastic"):
    """Host-side checks of beamsearch_stochastic; returns (k, max_length, flags).  vocab: the target vocabulary's size, which must
    hold at least n_samples words."""
    k, ml = int(n_samples), int(max_length)
    if not 1 <= k <= 64:
        raise ValueError("%s: need 1 <= n_samples <= 64, got %d" % (what, k))
    if ml < 1:
        raise ValueError("%s: max_length must be at least 1, got %d" % (what, ml))
    if vocab is not None and int(vocab) < k:
        raise ValueError("%s: n_samples=%d exceeds the target vocabulary (%d words)" % (what, k, int(vocab)))
    if not torch.is_tensor(src_var) or not src_var.is_cuda:
        raise ValueError("%s: src_var must be a GPU tensor (there is no CPU path)" % what)
    return k, ml, beam_flags(avoid_double, avoid_unk)


def mbr_args(without_replacement, temperature, top_k, top_p):
    """mbr_decode(without_replacement=True) takes its samples from the model's own distribution: no temperature, top_k or top_p."""
    if without_replacement and (float(temperature) != 1.0 or int(top_k) != 0 or float(top_p) != 1.0):
        raise ValueError("mbr_decode: without_replacement=True samples the model's own distribution; it cannot be combined with "
                         "temperature != 1, top_k or top_p (got temperature=%r top_k=%r top_p=%r)" % (temperature, top_k, top_p))
    return bool(without_replacement)


def assemble(res):
    """search.beam_stochastic's result -> Stochastic."""
    hyps, tokens, logp, score, gumbel, top = res
    gumbel = sbs_uncondition(gumbel, top)
    return Stochastic(hyps, logp, score, gumbel, sbs_log_weights(logp, gumbel))


def stochastic_search(obj, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double, avoid_unk,
                      what="beamsearch_stochastic"):
    """The draws of beamsearch_stochastic / mbr_decode(without_replacement=True) / mrt_step on a model or an Ensemble:
    search.beam_stochastic on its members, the generator (None: the object's own) advanced once.  Returns its (hyps, tokens, logp,
    score, gumbel, top).  No key fragment: the entry (kind "beam_sbs") owns the perturbed scores and the generator words its
    captured launches read."""
    k, ml, flags = stochastic_args(src_var, n_samples, max_length, avoid_double, avoid_unk, scoring.vocab_of(obj), what)
    gen = generator if generator is not None else sampling.default_generator(obj)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, ml, "beam_sbs", flags, what=what)
        res = obj._search_done(search.beam_stochastic(s.members, s.h0s, k, ml, gen.state(s.device), flags, s.entry, s.pool))
        gen.advance()
    return res


def beamsearch_stochastic(obj, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double, avoid_unk):
    """beamsearch_stochastic of a model or an Ensemble -> Stochastic."""
    return assemble(stochastic_search(obj, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double, avoid_unk))
