"""Diverse beam search (Vijayakumar et al. 2016): the beam's k slots are split into G groups that are expanded one after another
inside every step, and a group pays ``diversity`` for each slot of an earlier group that chose the same word at that step
(a Hamming penalty).  The k final hypotheses of a plain search differ in a word or two near the end; the groups of a diverse
search are pushed apart from their first word on, which is what an n-best list for rescoring, or the beam's candidates of
mbr_decode, want.

    d = model.beamsearch_diverse(src_var, src_lengths, im_var, beam_size=12, n_groups=3, diversity=0.5)
    d.hyps[b]          n_best token lists cut at EOS (default: all beam_size), best first
    d.scores (B, n)    their length-normalised scores on the device, descending
    d.group (B, n)     int64, the group each hypothesis ended in (final slot / (beam_size / n_groups))

The penalty steers the selection only: a returned score is the model's own (what score_translations gives for that hypothesis).
A finished hypothesis neither pays nor causes a penalty.  n_groups=1 is beamsearch_nbest; diversity=0 gives n_groups identical
copies of a search of width beam_size / n_groups.  The expansion is vag_beam_div_step (include/vag_nmt.h states the rule; the
search on the host is vagnmt_hip.search.beam_diverse), on models and on Ensemble alike."""
import math
from collections import namedtuple

import torch

from vagnmt_hip import scoring, search
from vagnmt_hip.scoring import beam_flags

Diverse = namedtuple("Diverse", ["hyps", "scores", "group"])


def group_args(beam_size, n_groups, diversity, what="beamsearch_diverse", names=("beam_size", "n_groups", "diversity")):
    """Checks of (beam width, groups, strength) alone -- mbr_decode names its own arguments; returns (k, G, strength)."""
    k, G, lam = int(beam_size), int(n_groups), float(diversity)
    if not 1 <= k <= 64:
        raise ValueError("%s: need 1 <= %s <= 64, got %d" % (what, names[0], k))
    if G < 1 or k % G:
        raise ValueError("%s: %s must be at least 1 and divide %s, got %s=%d %s=%d"
                         % (what, names[1], names[0], names[1], G, names[0], k))
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError("%s: %s must be a finite number >= 0, got %r" % (what, names[2], diversity))
    return k, G, lam


def diverse_args(src_var, beam_size, n_groups, diversity, n_best, avoid_double, avoid_unk, vocab=None, what="beamsearch_diverse"):
    """Host-side checks of beamsearch_diverse; returns (k, G, strength, n, flags).  n_best None: all beam_size.  vocab: the
    target vocabulary's size, which must hold at least beam_size words."""
    k, G, lam = group_args(beam_size, n_groups, diversity, what)
    n = k if n_best is None else int(n_best)
    if not 1 <= n <= k:
        raise ValueError("%s: need 1 <= n_best <= beam_size, got n_best=%d beam_size=%d" % (what, n, k))
    if vocab is not None and int(vocab) < k:
        raise ValueError("%s: beam_size=%d exceeds the target vocabulary (%d words)" % (what, k, int(vocab)))
    if not torch.is_tensor(src_var) or not src_var.is_cuda:
        raise ValueError("%s: src_var must be a GPU tensor (there is no CPU path)" % what)
    return k, G, lam, n, beam_flags(avoid_double, avoid_unk)


def mbr_beam_args(beam_size, beam_groups, beam_diversity):
    """What mbr_decode's beam_groups / beam_diversity add to its beam_size: (G, strength); G = 1 is the plain n-best list.
    beam_size = 0 (samples only) takes no groups."""
    k = int(beam_size)
    if k == 0:
        if int(beam_groups) != 1:
            raise ValueError("mbr_decode: beam_groups=%d needs beam_size > 0" % int(beam_groups))
        return 1, 0.0
    if int(beam_groups) == 1:
        return 1, 0.0
    _, G, lam = group_args(k, beam_groups, beam_diversity, "mbr_decode", ("beam_size", "beam_groups", "beam_diversity"))
    return G, lam


def beamsearch_diverse(obj, src_var, src_lengths, im_var, beam_size, n_groups, diversity, n_best, max_length, avoid_double, avoid_unk,
                       what="beamsearch_diverse"):
    """beamsearch_diverse of a model or an Ensemble (mbr_decode names itself in ``what``): search.beam_diverse on its members ->
    Diverse.  Key fragment ("diverse", groups, strength): by-value arguments of the captured expansions."""
    k, G, lam, n, flags = diverse_args(src_var, beam_size, n_groups, diversity, n_best, avoid_double, avoid_unk,
                                       scoring.vocab_of(obj), what)
    ml = int(max_length)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, ml, "beam_div", flags, extra=("diverse", G, lam), what=what)
        res = obj._search_done(search.beam_diverse(s.members, s.h0s, k, G, lam, ml, flags, n, s.entry, s.pool), k)
    return Diverse(*res)
