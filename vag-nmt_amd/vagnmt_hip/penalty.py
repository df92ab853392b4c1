"""Beam search with GNMT length and coverage penalties (Wu et al. 2016, section 7), applied at the finish or stepwise.

The beam searches rank their final hypotheses the reference's one way: total log-probability over the number of words above 3,
applied after the search has ended.  ``beamsearch_penalised`` exposes the knobs Marian, OpenNMT, Sockeye and fairseq have:

    p = model.beamsearch_penalised(src_var, src_lengths, im_var, beam_size=12, n_best=4, length_norm="gnmt", alpha=0.6, beta=0.2)
    p.hyps[b][r]                 the r-th best translation of sentence b, a token list cut at EOS
    p.scores (B, n)              the penalised score s, descending
    p.logp (B, n)                the model's total log-probability (what score_translations gives)
    p.length (B, n)              the number of words above 3 (int32)
    p.coverage_penalty (B, n)    cp

A hypothesis Y with log-probability c, L = max(1, #words > 3) and attention rows a_t scores

    s = (c + bonus[L]) / lp[L] + cp,     cp = beta * sum_i log(min(max(sum_t a_ti, 1e-10), 1))   over unmasked source positions

with lp[L] = ((5 + L) / 6)^alpha (``length_norm="gnmt"``), L^alpha (``"length"``) or 1 (``"none"``), and bonus[L] = word_bonus * L.
Both are tables of max_length + 1 floats built here in fp64 and rounded once, so the device evaluates no powf and every score can be
recomputed bit for bit in NumPy: s = fl(fl(fl(c + bonus[L]) / lp[L]) + cp) in fp32.  ``"length"`` with alpha = 1, beta = 0 and
word_bonus = 0 is beamsearch_nbest bit for bit.

``stepwise=False`` changes only the finish: the same k hypotheses as beamsearch_nbest, re-ranked.  ``stepwise=True`` (OpenNMT's
stepwise_penalty) selects by s at every step, so that a short finished hypothesis and a long unfinished one are no longer compared
on raw sums while they compete for slots -- the classic cause of beam search preferring short output.

The kernels are vag_beam_cover, vag_beam_pen_step and vag_beam_finish_pen (include/vag_nmt.h states the rule; the search on the
host is vagnmt_hip.search.beam_penalised), on models and on Ensemble alike.  ``penalised_score`` recomputes the score of given
translations in plain torch from score_translations' logp and align_translations' (or beamsearch_align's) attention."""
import math
from collections import namedtuple

import numpy as np
import torch

from vagnmt_hip import constrain, scoring, search
from vagnmt_hip.scoring import nbest_args

Penalised = namedtuple("Penalised", ["hyps", "scores", "logp", "length", "coverage_penalty"])
PenalisedScore = namedtuple("PenalisedScore", ["score", "coverage_penalty"])

LENGTH_NORMS = ("gnmt", "length", "none")
COV_FLOOR = 1e-10


def tables(max_length, length_norm="gnmt", alpha=0.6, word_bonus=0.0):
    """(lp, bonus): two float32 arrays of max_length + 1 entries, entry L formed in fp64 at max(L, 1) and rounded once."""
    if length_norm not in LENGTH_NORMS:
        raise ValueError("penalty.tables: length_norm must be one of %s, got %r" % (LENGTH_NORMS, length_norm))
    L = np.maximum(np.arange(int(max_length) + 1, dtype=np.float64), 1.0)
    if length_norm == "gnmt":
        lp = ((5.0 + L) / 6.0) ** float(alpha)
    elif length_norm == "length":
        lp = L ** float(alpha)
    else:
        lp = np.ones_like(L)
    return lp.astype(np.float32), (float(word_bonus) * L).astype(np.float32)


def penalised_args(src_var, beam_size, n_best, max_length, length_norm, alpha, beta, word_bonus, stepwise, avoid_double, avoid_unk,
                   vocab=None, what="beamsearch_penalised"):
    """Host-side checks of beamsearch_penalised; returns (k, n, max_length, flags, beta, stepwise)."""
    k, ml = int(beam_size), int(max_length)
    if ml < 1:
        raise ValueError("%s: max_length must be at least 1, got %d" % (what, ml))
    if vocab is not None and int(vocab) < k:
        raise ValueError("%s: beam_size=%d exceeds the target vocabulary (%d words)" % (what, k, int(vocab)))
    if length_norm not in LENGTH_NORMS:
        raise ValueError("%s: length_norm must be one of %s, got %r" % (what, LENGTH_NORMS, length_norm))
    a, b, wb = float(alpha), float(beta), float(word_bonus)
    if not (math.isfinite(a) and a >= 0.0):
        raise ValueError("%s: alpha must be finite and >= 0, got %r" % (what, alpha))
    if not (math.isfinite(b) and b >= 0.0):
        raise ValueError("%s: beta must be finite and >= 0, got %r" % (what, beta))
    if not math.isfinite(wb):
        raise ValueError("%s: word_bonus must be finite, got %r" % (what, word_bonus))
    if not isinstance(stepwise, (bool, np.bool_)):
        raise ValueError("%s: stepwise must be True or False, got %r" % (what, stepwise))
    k, n, flags = nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
    return k, n, ml, flags, float(np.float32(b)), bool(stepwise)


def coverage_penalty(attention, mask, beta):
    """cp of given attention: attention (..., T, Ts) rows per target position, zero outside the hypothesis (beamsearch_align's
    and align_translations' layout); mask (B, Ts), non-zero on real source positions, broadcast over the dimensions between."""
    cov = attention.sum(dim=-2)
    m = mask.to(cov.device)[..., :cov.shape[-1]]
    while m.dim() < cov.dim():
        m = m.unsqueeze(1)
    term = torch.log(cov.clamp(min=COV_FLOOR, max=1.0))
    term = torch.where(m != 0, term, torch.zeros_like(term))
    return float(beta) * term.sum(dim=-1)


def penalised_score(logp, length, attention, mask, length_norm="gnmt", alpha=0.6, beta=0.2, word_bonus=0.0, max_length=None):
    """The penalised score of given translations, in plain torch on any device: logp (...) and length (...) as score_translations
    / beamsearch_penalised give them (length = the number of words above 3), attention (..., T, Ts) as align_translations /
    beamsearch_align give it, mask (B, Ts).  beta = 0 (or attention None): no coverage term.  Returns PenalisedScore(score,
    coverage_penalty).  The tables are tables(); max_length (default: the largest length) only sizes them."""
    length = torch.as_tensor(length).to(torch.int64)
    L = length.clamp(min=1)
    ml = int(max_length) if max_length is not None else int(L.max().item())
    lp, bonus = tables(max(ml, int(L.max().item())), length_norm, alpha, word_bonus)
    lp, bonus = torch.from_numpy(lp).to(logp.device), torch.from_numpy(bonus).to(logp.device)
    L = L.to(logp.device)
    if attention is None or float(beta) == 0.0:
        cp = torch.zeros_like(logp, dtype=torch.float32)
    else:
        cp = coverage_penalty(attention.to(torch.float32), mask, beta).to(logp.device).reshape(logp.shape)
    return PenalisedScore((logp.to(torch.float32) + bonus[L]) / lp[L] + cp, cp)


def assemble(res):
    """search.beam_penalised's result -> Penalised."""
    return Penalised(*res)


def beamsearch_penalised(obj, src_var, src_lengths, im_var, beam_size, n_best, max_length, length_norm, alpha, beta, word_bonus,
                         stepwise, avoid_double, avoid_unk, no_repeat_ngram):
    """beamsearch_penalised of a model or an Ensemble: search.beam_penalised on its members, which keep their attention rows ->
    Penalised.  A no-repeat n-gram rule, when given, is masked before every expansion.  Key fragment ("penalty", beta, stepwise):
    by-value arguments of the captured launches; the entry owns the carried lengths, coverage and penalties and the two tables,
    refilled at every call, so one entry serves every alpha and word_bonus."""
    what = "beamsearch_penalised"
    V = scoring.vocab_of(obj)
    k, n, ml, flags, beta, stepwise = penalised_args(src_var, beam_size, n_best, max_length, length_norm, alpha, beta, word_bonus,
                                                     stepwise, avoid_double, avoid_unk, V, what)
    packed = constrain.any_of(constrain.pack(src_var.shape[0], V, ml, no_repeat_ngram=no_repeat_ngram, avoid_double=avoid_double,
                                             avoid_unk=avoid_unk, what=what))
    lp, bonus = tables(ml, length_norm, alpha, word_bonus)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, ml, "beam_pen", flags, align=True,
                              extra=constrain.graph_key(packed) + ("penalty", beta, stepwise), what=what)
        res = obj._search_done(search.beam_penalised(s.members, s.h0s, k, ml, lp, bonus, beta, stepwise, flags, n, s.entry, s.pool,
                                                     constrain=constrain.on_device(packed, s, ml)), k)
    return assemble(res)
