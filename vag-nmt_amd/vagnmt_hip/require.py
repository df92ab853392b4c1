"""Required words and phrases in beam search: what the output must contain (dynamic beam allocation, Post & Vilar 2018; Hu et
al. 2019).

    r = model.beamsearch_required(src_var, src_lengths, im_var, beam_size=12, n_best=1, max_length=80,
                                  required=[[[17, 5], [230]], []], prefix=None, banned=None, banned_per_sentence=None,
                                  no_repeat_ngram=0)
    r.hyps[b]           n_best token lists cut at EOS: the hypotheses that contain all their phrases first, best first
    r.scores (B, n)     their length-normalised scores on the device (vag_beam_finish_nbest's values), descending within
                        the complete and within the incomplete part
    r.met (B, n)        int64 bitmask: bit c = the c-th phrase given for the sentence occurs, contiguously, in the hypothesis
    r.complete (B, n)   bool: every phrase of the sentence is met

    required            a list of B lists of phrases (token lists of 1 .. 8 words), at most 16 per sentence

A hypothesis that has not produced a phrase yet is unfinished, not wrong, so no -1e5 mask can express the constraint.
Instead every hypothesis carries its state from step to step -- which phrases it has met, how far it is into each of the
others, and the sum of both in words, its bank -- and the expansion (vag_beam_req_step; include/vag_nmt.h states the rule)
deals the beam's slots round-robin over the banks, highest first: the best hypothesis of every bank survives, whatever it
scores.  The candidates are the plain search's k best, every row's own best word, and for every open phrase of every
hypothesis the word that advances it; EOS is ruled out while a phrase is open.  A stored score is the model's own, so a
returned score is what score_translations gives for the returned words.

The negative constraints of vagnmt_hip.constrain (prefix, banned, banned_per_sentence, no_repeat_ngram) combine with it: their
mask runs before the expansion, and the state follows the words whoever chose them, so a forced prefix word that advances a
phrase counts.  A search that reaches max_length with phrases open returns such hypotheses flagged incomplete, as they are.
With nothing required and no negative constraints the search is beamsearch_nbest bit for bit."""
from collections import namedtuple

import numpy as np
import torch

from vagnmt_hip import constrain, scoring, search
from vagnmt_hip.search import EOS_token, SOS_token, UNK_token

MAX_PHRASES = 16        # VAG_REQUIRE_MAX_PHRASES (include/vag_nmt.h)
MAX_LEN = constrain.MAX_LEN

Required = namedtuple("Required", ["hyps", "scores", "met", "complete"])


def _contains(ph, sub):
    return any(ph[i:i + len(sub)] == sub for i in range(len(ph) - len(sub) + 1))


def pack(B, V, max_length, required=None, banned=None, banned_per_sentence=None, avoid_double=True, avoid_unk=False,
         what="beamsearch_required"):
    """Host-side checks of beamsearch_required's ``required`` and its packing into the (B, MAX_PHRASES, MAX_LEN) int64 table
    vag_beam_req_step reads (phrase c of sentence b in row (b, c), pad 0).  Raises ValueError, the argument named, for what the
    search could not honour.  Identical phrases in one sentence are allowed; one occurrence meets both."""
    table = np.zeros((B, MAX_PHRASES, MAX_LEN), dtype=np.int64)
    if required is None:
        return table
    lists = list(required)
    if len(lists) != B:
        raise ValueError("%s: required holds %d lists for %d source sentences" % (what, len(lists), B))
    everywhere = [[int(t) for t in ph] for ph in (banned or [])]
    per = list(banned_per_sentence) if banned_per_sentence is not None else [[] for _ in range(B)]
    for b, lst in enumerate(lists):
        lst = [[int(t) for t in ph] for ph in (lst or [])]
        if len(lst) > MAX_PHRASES:
            raise ValueError("%s: required holds %d phrases for sentence %d, at most %d" % (what, len(lst), b, MAX_PHRASES))
        bans = everywhere + ([[int(t) for t in ph] for ph in (per[b] or [])] if b < len(per) else [])
        for c, ph in enumerate(lst):
            if not 1 <= len(ph) <= MAX_LEN:
                raise ValueError("%s: a phrase of required has %d words, need 1 .. %d" % (what, len(ph), MAX_LEN))
            for t, w in enumerate(ph):
                if not 1 <= w < V:
                    raise ValueError("%s: word %d of required lies outside the vocabulary [1, %d)" % (what, w, V))
                if w in (SOS_token, EOS_token):
                    raise ValueError("%s: required holds %d (SOS and EOS cannot be part of a phrase)" % (what, w))
                if avoid_double and t > 0 and ph[t - 1] == w:
                    raise ValueError("%s: a phrase of required repeats word %d, which avoid_double=True rules out" % (what, w))
                if avoid_unk and w == UNK_token:
                    raise ValueError("%s: a phrase of required holds UNK, which avoid_unk=True rules out" % what)
            for ban in bans:
                if ban and _contains(ph, ban):
                    raise ValueError("%s: a phrase of required for sentence %d contains the banned phrase %s" % (what, b, ban))
            table[b, c, :len(ph)] = ph
        total = sum(len(ph) for ph in lst)
        if total > max_length - 1:
            raise ValueError("%s: required holds %d words for sentence %d, at most max_length - 1 = %d"
                             % (what, total, b, max_length - 1))
    return table


def given_masks(table):
    """(B,) int64: bit c set for every phrase given for the sentence."""
    used = table[:, :, 0] != 0
    return (used.astype(np.int64) << np.arange(MAX_PHRASES, dtype=np.int64)[None, :]).sum(1)


def assemble(hyps, scores, slots, state, table, n_best):
    """The search's ranked hypotheses (all beam_size of them) -> Required: ``met`` of each through its final slot, a stable
    re-ordering that puts the hypotheses that met all their phrases first, the first n_best of it."""
    met = torch.gather(state[:, :, 0].to(torch.int64) & 0xffff, 1, slots)
    want = torch.from_numpy(given_masks(table)).to(met.device)[:, None]
    complete = (met & want) == want
    order = torch.sort((~complete).to(torch.int8), dim=1, stable=True).indices[:, :n_best]
    idx = order.cpu().tolist()
    return Required([[hyps[b][r] for r in rows] for b, rows in enumerate(idx)], torch.gather(scores, 1, order),
                    torch.gather(met, 1, order), torch.gather(complete, 1, order))


def beamsearch_required(obj, src_var, src_lengths, im_var, beam_size, n_best, max_length, required, prefix, banned,
                        banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk):
    """beamsearch_required of a model or an Ensemble: search.beam_required on its members -- all beam_size hypotheses finished,
    ``met`` of each looked up through its final slot, the complete ones first -> Required.  Negative constraints, when given, are
    masked before every expansion.  No key fragment of its own (constrain.graph_key joins with negative constraints): the entry
    (kind "beam_req") owns the static phrase table and state and serves every phrase set."""
    what = "beamsearch_required"
    k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
    ml, B, V = int(max_length), src_var.shape[0], scoring.vocab_of(obj)
    packed = constrain.any_of(constrain.pack(B, V, ml, prefix, banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk,
                                             what))
    table = pack(B, V, ml, required, banned, banned_per_sentence, avoid_double, avoid_unk, what)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, ml, "beam_req", flags, extra=constrain.graph_key(packed), what=what)
        res = obj._search_done(search.beam_required(s.members, s.h0s, k, ml, table, flags, k, s.entry, s.pool,
                                                    constrain=constrain.on_device(packed, s, ml)), k)
    return assemble(*res, table, n)
