"""Constrained beam search: what the output must begin with and what it must not contain.

    c = model.beamsearch_constrained(src_var, src_lengths, im_var, beam_size=12, n_best=1, max_length=80,
                                     prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0)
    c.hyps[b]          n_best token lists cut at EOS, the forced words included, best first
    c.scores (B, n)    their length-normalised scores on the device, descending (vag_beam_finish_nbest's)

    prefix               a list of B token lists (empty: none), or a (B, Lp) int64 tensor padded with 0: sentence b's output
                         begins with these words ("continue from here", a terminology-forced opening)
    banned               a list of token lists (words and phrases) no output may contain
    banned_per_sentence  a list of B such lists, one per sentence
    no_repeat_ngram      n >= 1: no n-gram occurs twice in a hypothesis (n = 1: no word does); 0: off

All three rule words out before a step's expansion as a function of the hypothesis's own history: one launch per step
(vag_beam_constrain, include/vag_nmt.h states the rule) writes -1e5, the search's own "ruled out" value, into the members'
log-probability rows.  A forced word keeps the model's value, so a returned score is the model's own (what score_translations
gives for the returned words).  The expansion, the finish and the default search are what they were.

The consequence of the -1e5 convention: while a sentence is forced only one continuation of a hypothesis is live, so the other
beam_size - 1 slots carry hypotheses that took a -1e5 step and score below -1e4 -- the entries vag_beam_finish_nbest's comment
describes.  They fall out of the beam as soon as live hypotheses fill it; an n-best list contains them only if the constraints
leave fewer than n live hypotheses, and they are returned as they are.

Positive ("must contain") constraints are another algorithm (they change how slots are allotted): vagnmt_hip.require."""
from collections import namedtuple

import numpy as np
import torch

from vagnmt_hip import scoring, search
from vagnmt_hip._lib import ptr
from vagnmt_hip.search import EOS_token, SOS_token, UNK_token

MAX_LEN = 8             # VAG_CONSTRAIN_MAX_LEN (include/vag_nmt.h): words in a banned phrase, largest no-repeat n
MAX_PHRASES = 256       # VAG_CONSTRAIN_MAX_PHRASES

Constrained = namedtuple("Constrained", ["hyps", "scores"])
# The constraints as the kernel reads them, on the host: prefix (B, Lp) int64 pad 0, phrases (P, MAX_LEN) int64 pad 0,
# phrase_sent (P,) int32 (-1: every sentence), ngram.
Packed = namedtuple("Packed", ["prefix", "phrases", "phrase_sent", "ngram"])


def _prefix_rows(prefix, B, what):
    if prefix is None:
        return [[] for _ in range(B)]
    if torch.is_tensor(prefix):
        if prefix.dim() != 2 or prefix.shape[0] != B:
            raise ValueError("%s: prefix must be (B, Lp) = (%d, *), got %s" % (what, B, tuple(prefix.shape)))
        if prefix.dtype != torch.int64:
            raise ValueError("%s: prefix must be int64, got %s" % (what, prefix.dtype))
        rows = []
        for b, r in enumerate(prefix.cpu().tolist()):
            n = len(r)
            while n and r[n - 1] == 0:
                n -= 1
            if 0 in r[:n]:
                raise ValueError("%s: prefix of sentence %d has a 0 (padding) inside it" % (what, b))
            rows.append(r[:n])
        return rows
    rows = [[int(t) for t in r] for r in prefix]
    if len(rows) != B:
        raise ValueError("%s: prefix holds %d lists for %d source sentences" % (what, len(rows), B))
    return rows


def _phrase(ph, V, what, name):
    ph = [int(t) for t in ph]
    if not 1 <= len(ph) <= MAX_LEN:
        raise ValueError("%s: a phrase of %s has %d words, need 1 .. %d" % (what, name, len(ph), MAX_LEN))
    for w in ph:
        if not 0 <= w < V:
            raise ValueError("%s: word %d of %s lies outside the vocabulary [0, %d)" % (what, w, name, V))
        if w == 0:
            raise ValueError("%s: word 0 of %s is the padding word, it cannot be part of a phrase" % (what, name))
    return ph


def pack(B, V, max_length, prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True,
         avoid_unk=False, what="beamsearch_constrained"):
    """Host-side checks of beamsearch_constrained's constraints and their packing into the arrays vag_beam_constrain reads.
    Raises ValueError, the argument named, for what the search could not honour: the expansion's own penalties (avoid_double,
    avoid_unk) come after the mask and would rule such a forced word out."""
    n = int(no_repeat_ngram)
    if not 0 <= n <= MAX_LEN:
        raise ValueError("%s: need 0 <= no_repeat_ngram <= %d, got %d" % (what, MAX_LEN, n))
    rows = _prefix_rows(prefix, B, what)
    for b, r in enumerate(rows):
        if len(r) > max_length - 1:
            raise ValueError("%s: prefix of sentence %d has %d words, at most max_length - 1 = %d" % (what, b, len(r), max_length - 1))
        for t, w in enumerate(r):
            if not 0 <= w < V:
                raise ValueError("%s: prefix word %d of sentence %d lies outside the vocabulary [0, %d)" % (what, w, b, V))
            if w in (0, SOS_token, EOS_token):
                raise ValueError("%s: prefix of sentence %d holds %d (padding, SOS and EOS cannot be forced)" % (what, b, w))
            if avoid_double and t > 0 and r[t - 1] == w:
                raise ValueError("%s: prefix of sentence %d repeats word %d, which avoid_double=True rules out" % (what, b, w))
            if avoid_unk and t > 0 and w == UNK_token:
                raise ValueError("%s: prefix of sentence %d holds UNK after its first word, which avoid_unk=True rules out"
                                 % (what, b))
    Lp = max([len(r) for r in rows] + [0])
    pre = np.zeros((B, Lp), dtype=np.int64)
    for b, r in enumerate(rows):
        pre[b, :len(r)] = r
    phr, sent = [], []
    for ph in (banned or []):
        phr.append(_phrase(ph, V, what, "banned"))
        sent.append(-1)
    if banned_per_sentence is not None:
        per = list(banned_per_sentence)
        if len(per) != B:
            raise ValueError("%s: banned_per_sentence holds %d lists for %d source sentences" % (what, len(per), B))
        for b, lst in enumerate(per):
            for ph in (lst or []):
                phr.append(_phrase(ph, V, what, "banned_per_sentence"))
                sent.append(b)
    if len(phr) > MAX_PHRASES:
        raise ValueError("%s: banned and banned_per_sentence hold %d phrases, at most %d" % (what, len(phr), MAX_PHRASES))
    phrases = np.zeros((len(phr), MAX_LEN), dtype=np.int64)
    for p, ph in enumerate(phr):
        phrases[p, :len(ph)] = ph
    return Packed(pre, phrases, np.asarray(sent, dtype=np.int32).reshape(len(phr)), n)


def flat_layout(B, Lp, P):
    """Offsets, in int64 words, of (prefix, phrases, phrase_sent) in the one buffer that holds them, and its size."""
    a = B * Lp
    b = a + P * MAX_LEN
    return a, b, b + (P + 1) // 2


def flatten(packed, B, Lp, P):
    """The packed constraints, zero-padded to a (B, Lp) prefix and P phrases, as one int64 host array (flat_layout)."""
    a, b, size = flat_layout(B, Lp, P)
    flat = np.zeros(size, dtype=np.int64)
    lp, p = packed.prefix.shape[1], packed.phrases.shape[0]
    assert packed.prefix.shape[0] == B and lp <= Lp and p <= P
    flat[:a].reshape(B, Lp)[:, :lp] = packed.prefix
    flat[a:b].reshape(P, MAX_LEN)[:p] = packed.phrases
    flat[b:].view(np.int32)[:p] = packed.phrase_sent
    return flat


class Constraints:
    """The constraints of one search on the device, as search.beam takes them: ONE int64 buffer (prefix | phrases | phrase_sent),
    one copy per call.  Eager mode (entry None): a fresh buffer of the set's own sizes; an empty set (Lp = P = ngram = 0)
    launches nothing.  Graph mode: the entry's static buffer, sized for a (B, max_length) prefix and MAX_PHRASES phrases and
    refilled COMPLETELY, zeros included, at every call -- the captured launches point at it and take Lp = max_length,
    P = MAX_PHRASES by value, so one entry serves every constraint set of one ``ngram`` (a by-value argument, part of the key)."""

    def __init__(self, packed, B, max_length, dev, entry=None):
        self.ngram = packed.ngram
        if entry is None:
            self.Lp, self.P = packed.prefix.shape[1], packed.phrases.shape[0]
        else:
            self.Lp, self.P = max_length, MAX_PHRASES
        a, b, size = flat_layout(B, self.Lp, self.P)
        host = torch.from_numpy(flatten(packed, B, self.Lp, self.P))
        if entry is None:
            buf = host.to(dev) if size else None
        else:
            buf = entry.get("constrain_buf")
            if buf is None:
                buf = entry["constrain_buf"] = torch.empty(size, dtype=torch.int64, device=dev)
            buf.copy_(host)
        self.buf = buf
        self.prefix = buf[:a].view(B, self.Lp) if self.Lp else None
        self.phrases = buf[a:b].view(self.P, MAX_LEN) if self.P else None
        self.phrase_sent = buf[b:].view(torch.int32)[:self.P] if self.P else None

    def args(self):
        """(prefix, Lp, phrases, phrase_sent, P, ngram) as vag_beam_constrain takes them."""
        return (ptr(self.prefix, torch.int64), self.Lp, ptr(self.phrases, torch.int64), ptr(self.phrase_sent, torch.int32), self.P,
                self.ngram)


def any_of(packed):
    """packed where it holds a constraint, else None: what the searches that merely accept negative constraints go by."""
    return packed if bool(packed.prefix.any()) or len(packed.phrases) > 0 or packed.ngram > 0 else None


def graph_key(packed):
    """Key fragment of a search with negative constraints (None: ()): ("constrain", n), the no-repeat n being a by-value
    argument of the captured mask launches.  Such entries also own the static constraint buffers; one serves every constraint
    set of one n."""
    return () if packed is None else ("constrain", packed.ngram)


def on_device(packed, setup, max_length):
    """The Constraints of one search (None: None) on the device and, in graph mode, in the entry of ``setup`` (search.Setup)."""
    return None if packed is None else Constraints(packed, setup.B, max_length, setup.device, setup.entry)


def beamsearch_constrained(obj, src_var, src_lengths, im_var, beam_size, n_best, max_length, prefix, banned, banned_per_sentence,
                           no_repeat_ngram, avoid_double, avoid_unk):
    """beamsearch_constrained of a model or an Ensemble: search.beam on its members with the mask before every expansion and the
    n-best finish -> Constrained.  The log-probability steps only: there is no raw-logits form."""
    what = "beamsearch_constrained"
    k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
    ml = int(max_length)
    packed = pack(src_var.shape[0], scoring.vocab_of(obj), ml, prefix, banned, banned_per_sentence, no_repeat_ngram, avoid_double,
                  avoid_unk, what)
    with torch.no_grad():
        s = obj._search_setup(src_var, src_lengths, im_var, k, ml, "beam_con", flags, extra=graph_key(packed), what=what)
        res = obj._search_done(search.beam(s.members, s.h0s, k, ml, flags, n, s.entry, s.pool, raw_logits=False,
                                           constrain=on_device(packed, s, ml)), k)
    return Constrained(*res)
