"""Minimum-Bayes-risk selection: of N candidate translations of a sentence, the one with the highest expected utility against
a set of pseudo-references -- usually the sampler's own draws (vagnmt_hip.sampling), optionally joined by the beam search's
n-best list as further candidates.

The pairwise utility (B x Nh x Nr sentence pairs, clipped 1..4-gram matches each) and the selection run on the device, two
launches of vag_mbr_select (csrc/mbr.hip; the definitions are in include/vag_nmt.h):

    sel = mbr_select(hyps)                               # the candidates are their own references
    sel = mbr_select(hyps, refs, weights, utility="ngram_f")
    sel.index (B,) int64      the chosen candidate of every sentence: the lowest index of maximal expected utility
    sel.expected (B, Nh)      every candidate's expected utility, float32
    sel.best                  the chosen token lists, cut at EOS
    sel, (util, matches) = mbr_select(hyps, return_utilities=True)      # util (B, Nh, Nr), matches (B, Nh, Nr, 4) int32

hyps / refs: (B, N, L) int64 GPU tensors (a row's content is what precedes its first EOS), or nested lists hyps[b][i] of token
lists as Sampled.hyps and beamsearch_nbest return them.  utility: "bleu" (segment-level smooth BLEU, the reference's
bleu.compute_bleu(smooth=True)) or "ngram_f" (a symmetric n-gram F score).

    best, sel, drawn = model.mbr_decode(src_var, src_lengths, im_var, n_samples=16, temperature=0.9, beam_size=4)

draws n_samples translations (sample_decode's arguments and generator), selects among them (and the beam_size-best list, if
asked for) against the samples, and returns the chosen token lists, the Selected and the Sampled.

    best, sel, drawn = model.mbr_decode(src_var, src_lengths, im_var, n_samples=16, without_replacement=True)

draws the n_samples WITHOUT replacement instead (beamsearch_stochastic, vagnmt_hip.stochastic: distinct translations, no pairwise
utility spent on duplicates) and weights them as pseudo-references by their importance weights exp(log_weight), so that the
expected utility is still an estimate under the model's distribution; drawn is then the Stochastic.  Not with a temperature,
top_k or top_p.

    table = Surface(words)                               # vagnmt_hip.surface: what the ids spell
    sel = mbr_select(hyps, utility="chrf", surface=table)
    sel, (util, matches, lens) = mbr_select(hyps, refs, utility="chrf", surface=table, return_utilities=True)
    best, sel, drawn = model.mbr_decode(src_var, src_lengths, im_var, n_samples=16, utility="chrf", surface=table)

utility "chrf" is chrF on surface characters (character 1..6-grams, F with beta = 2, averaged over the effective orders;
include/vag_nmt.h: vag_chrf_select has the definition): two candidates that differ in one sub-word split or one ending share few
token 3- and 4-grams and almost all their characters.  Both sides are expanded to character rows on the device
(vag_surface_expand, one launch each) and vag_chrf_select takes the place of vag_mbr_select; matches is (B, Nh, Nr, 6), and lens
is CharLens(hyps (B, Nh), refs (B, Nr), limit (Ch, Cr)): the TRUE character counts and the stored width.  A row longer than its
limit (min(1024, L * table.max_len) characters) is cut to its first characters -- documented behaviour, not an error; lens shows
it.  surface is required with "chrf" and refused with any other utility.  chrF++ (word n-grams) is not computed."""
from collections import namedtuple

import torch

from vagnmt_hip import diverse, sampling, scoring, stochastic
from vagnmt_hip._lib import call, lib, ptr, stream
from vagnmt_hip.search import EOS_token, cut

UTILITIES = {"bleu": 0, "ngram_f": 1, "chrf": 2}        # 0, 1: vag_mbr_select's utility; 2: vag_chrf_select
CHRF = UTILITIES["chrf"]

Selected = namedtuple("Selected", ["index", "expected", "best"])
CharLens = namedtuple("CharLens", ["hyps", "refs", "limit"])


def utility_id(utility, what="mbr_select"):
    if utility not in UTILITIES:
        raise ValueError("%s: utility must be one of %s, got %r" % (what, sorted(UTILITIES), utility))
    return UTILITIES[utility]


def check_surface(utility, surface, what="mbr_select", word="utility", vocab=None):
    """The surface table goes with "chrf" and with nothing else; a table must cover the vocabulary that produces the ids."""
    from vagnmt_hip.surface import Surface
    if utility == "chrf":
        if not isinstance(surface, Surface):
            raise ValueError("%s: %s 'chrf' needs surface=, a vagnmt_hip.surface.Surface of the target vocabulary, got %r"
                             % (what, word, surface))
        if vocab is not None and surface.V < vocab:
            raise ValueError("%s: surface holds %d words, the vocabulary %d" % (what, surface.V, vocab))
    elif surface is not None:
        raise ValueError("%s: surface goes with %s 'chrf' only, got %s %r" % (what, word, word, utility))


def pack(rows, what="hyps"):
    """Nested lists rows[b][i] of token lists -> a (B, N, L) int64 CPU tensor: EOS appended to a list that holds none, padded
    with 0.  Every sentence must have the same number of lists.  A tensor is returned as it is."""
    if torch.is_tensor(rows):
        return rows
    rows = [[[int(t) for t in r] for r in sent] for sent in rows]
    if not rows or not rows[0]:
        raise ValueError("mbr_select: %s is empty" % what)
    N = len(rows[0])
    if any(len(sent) != N for sent in rows):
        raise ValueError("mbr_select: every sentence needs the same number of %s, got %s"
                         % (what, sorted(set(len(sent) for sent in rows))))
    rows = [[r if EOS_token in r else r + [EOS_token] for r in sent] for sent in rows]
    out = torch.zeros(len(rows), N, max(len(r) for sent in rows for r in sent), dtype=torch.int64)
    for b, sent in enumerate(rows):
        for i, r in enumerate(sent):
            out[b, i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out


def _tokens(t, what, device, batch=None):
    """Host-side checks of one token operand; returns it as a contiguous (B, N, L) int64 tensor on the device.  Lists are packed
    and copied there; a tensor must be on a GPU already."""
    if torch.is_tensor(t):
        if not t.is_cuda:
            raise ValueError("mbr_select: %s must be a GPU tensor (there is no CPU path)" % what)
    else:
        t = pack(t, what).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    if t.dtype != torch.int64:
        raise ValueError("mbr_select: %s must be int64, got %s" % (what, t.dtype))
    if t.dim() != 3 or min(t.shape) < 1 or (batch is not None and t.shape[0] != batch):
        raise ValueError("mbr_select: %s must be (B, N, L)%s, got %s"
                         % (what, "" if batch is None else " with B = %d" % batch, tuple(t.shape)))
    return t.contiguous()


def select_args(hyps, refs=None, weights=None, utility="bleu", surface=None):
    """Host-side checks of mbr_select; returns (hyps, refs or None, weights or None, utility id) ready for the library.  Token
    lists go to the device of the first operand that is a GPU tensor, or to the current GPU.  With a surface table (utility
    "chrf") the ids must lie below its V."""
    uid = utility_id(utility)
    check_surface(utility, surface)
    dev = next((t.device for t in (hyps, refs, weights) if torch.is_tensor(t) and t.is_cuda), None)
    hyps = _tokens(hyps, "hyps", dev)
    if refs is not None:
        refs = _tokens(refs, "refs", dev, hyps.shape[0])
        if refs.device != hyps.device:
            raise ValueError("mbr_select: hyps and refs are on different devices")
    for name, t in (("hyps", hyps), ("refs", refs)):
        if t is not None:
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= 1 << 31:
                raise ValueError("mbr_select: %s must hold ids in [0, 2^31), got [%d, %d]" % (name, lo, hi))
            if surface is not None and hi >= surface.V:
                raise ValueError("mbr_select: %s holds id %d, the surface table %d words" % (name, hi, surface.V))
    r = hyps if refs is None else refs
    if not lib().vag_mbr_supported(hyps.shape[1], hyps.shape[2], r.shape[1], r.shape[2]):
        raise ValueError("mbr_select: unsupported shape: hyps %s, refs %s (include/vag_nmt.h: vag_mbr_select)"
                         % (tuple(hyps.shape), tuple(r.shape)))
    if weights is not None:
        if not torch.is_tensor(weights) or not weights.is_cuda:
            raise ValueError("mbr_select: weights must be a GPU tensor (there is no CPU path)")
        if tuple(weights.shape) != (r.shape[0], r.shape[1]):
            raise ValueError("mbr_select: weights must be (B, Nr) = %s, got %s" % ((r.shape[0], r.shape[1]), tuple(weights.shape)))
        weights = weights.to(device=hyps.device, dtype=torch.float32)
        total = weights.sum(1, keepdim=True)
        if not bool((weights >= 0).all()) or not bool((total > 0).all()) or not bool(torch.isfinite(total).all()):
            raise ValueError("mbr_select: weights must be non-negative and finite, with a positive sum for every sentence")
        weights = (weights / total).contiguous()
    return hyps, refs, weights, uid


def run(hyps, refs, weights, uid, return_utilities=False):
    """vag_mbr_select on checked operands (select_args, or tokens that come from the decoders): (index, expected, util or
    None, matches or None), all on the device; nothing waits for the host."""
    B, Nh, Lh = hyps.shape
    Nr, Lr = (Nh, Lh) if refs is None else refs.shape[1:]
    dev = hyps.device
    expected = torch.empty(B, Nh, device=dev)
    index = torch.empty(B, dtype=torch.int64, device=dev)
    util = torch.empty(B, Nh, Nr, device=dev) if return_utilities else None
    matches = torch.empty(B, Nh, Nr, 4, dtype=torch.int32, device=dev) if return_utilities else None
    call("vag_mbr_select", ptr(hyps, torch.int64), ptr(refs, torch.int64), ptr(weights), B, Nh, Lh, Nr, Lr, uid,
         ptr(matches, torch.int32), ptr(util), ptr(expected), ptr(index, torch.int64), stream())
    return index, expected, util, matches


def run_chrf(hyps, refs, weights, surface, return_utilities=False):
    """vag_chrf_select on checked token operands (ids below surface.V): both sides expanded to character rows (vag_surface_expand,
    one launch each; C = min(the kernel's limit, L * surface.max_len)), then the pairs and the arg-max.  Returns (index, expected,
    util or None, matches (B, Nh, Nr, 6) or None, CharLens); all on the device, nothing waits for the host."""
    B, Nh, _ = hyps.shape
    dev = hyps.device
    hchars, hlens = surface.expand(hyps)
    rchars, rlens = (None, None) if refs is None else surface.expand(refs)
    Nr, Cr = (Nh, hchars.shape[2]) if refs is None else rchars.shape[1:]
    expected = torch.empty(B, Nh, device=dev)
    index = torch.empty(B, dtype=torch.int64, device=dev)
    util = torch.empty(B, Nh, Nr, device=dev) if return_utilities else None
    matches = torch.empty(B, Nh, Nr, 6, dtype=torch.int32, device=dev) if return_utilities else None
    call("vag_chrf_select", ptr(hchars, torch.int32), ptr(hlens, torch.int32), ptr(rchars, torch.int32), ptr(rlens, torch.int32),
         ptr(weights), B, Nh, hchars.shape[2], Nr, Cr, ptr(matches, torch.int32), ptr(util), ptr(expected),
         ptr(index, torch.int64), stream())
    return index, expected, util, matches, CharLens(hlens, hlens if refs is None else rlens, (hchars.shape[2], Cr))


def _run(hyps, refs, weights, uid, surface):
    """(index, expected) by the utility's own entry point."""
    return (run_chrf(hyps, refs, weights, surface) if uid == CHRF else run(hyps, refs, weights, uid))[:2]


def chosen(hyps, index):
    """The rows hyps[b, index[b]] as token lists cut at EOS (one copy to the host)."""
    rows = hyps[torch.arange(hyps.shape[0], device=hyps.device), index].cpu().tolist()
    return cut(rows)


def mbr_select(hyps, refs=None, weights=None, utility="bleu", return_utilities=False, surface=None):
    """Selected(index (B,) int64, expected (B, Nh) float32, best) of the candidates hyps against the pseudo-references refs
    (None: the candidates themselves) -- see the module's text.  weights (B, Nr), non-negative, are normalised per sentence
    (None: uniform); a row that sums to zero raises.  With return_utilities also (util (B, Nh, Nr), matches (B, Nh, Nr, 4)); with
    utility "chrf" (surface: the vocabulary's Surface table) that is (util, matches (B, Nh, Nr, 6), CharLens).  best always
    comes from the token rows."""
    hyps, refs, weights, uid = select_args(hyps, refs, weights, utility, surface)
    if uid == CHRF:
        index, expected, util, matches, lens = run_chrf(hyps, refs, weights, surface, return_utilities)
        sel = Selected(index, expected, chosen(hyps, index))
        return (sel, (util, matches, lens)) if return_utilities else sel
    index, expected, util, matches = run(hyps, refs, weights, uid, return_utilities)
    sel = Selected(index, expected, chosen(hyps, index))
    return (sel, (util, matches)) if return_utilities else sel


def decode_args(n_samples, max_length, beam_size, utility, surface=None, vocab=None):
    """Host-side checks of what mbr_decode adds to sample_decode's arguments, before anything is drawn; returns (beam_size,
    utility id).  The beam's lists hold at most max_length words and the EOS that pack appends.  surface: the table of utility
    "chrf", which must cover the decoder's vocabulary (vocab words)."""
    k, n, ml = int(beam_size), int(n_samples), int(max_length)
    if not 0 <= k <= 64:
        raise ValueError("mbr_decode: beam_size must be 0 (samples only) or 1 .. 64, got %d" % k)
    uid = utility_id(utility, "mbr_decode")
    check_surface(utility, surface, "mbr_decode", vocab=vocab)
    if n >= 1 and ml >= 1 and not lib().vag_mbr_supported(n + k, ml + (1 if k else 0), n, ml):
        raise ValueError("mbr_decode: unsupported shape: %d candidates and %d samples of up to %d tokens (include/vag_nmt.h: "
                         "vag_mbr_select)" % (n + k, n, ml))
    return k, uid


def from_history(toks, lps, B, n, nbest, uid, surface=None):
    """mbr_decode after the draws: toks, lps (L, B n) the sampler's time-major history on the device (buffers of the sampling
    decode's own state, which no other decode writes); nbest None, or a call that runs the beam search and returns its lists
    beams[b][i].  The samples are the pseudo-references and the first n candidates; the beams follow them.  The token history
    stays on the device: one transpose to (B, n, L), and without beams nothing waits for the host before the selection is
    enqueued; the Sampled is assembled after it.  surface: the table of uid "chrf" (two more launches, the expansion of the
    candidates and of the references; the tokens stay on the device)."""
    dev = toks.device
    refs = toks.t().reshape(B, n, -1).contiguous()
    hyps = refs
    if nbest is not None:
        extra = pack(nbest(), "beams").to(dev)
        L = max(refs.shape[2], extra.shape[2])
        # a sample that ran to max_length holds no EOS: pad it with EOS, not with the padding word (which would be content)
        hyps = torch.cat([torch.nn.functional.pad(refs, (0, L - refs.shape[2]), value=EOS_token),
                          torch.nn.functional.pad(extra, (0, L - extra.shape[2]), value=0)], 1).contiguous()
    index, expected = _run(hyps, None if nbest is None else refs, None, uid, surface)
    drawn = sampling.assemble(toks, lps, B, n, dev)
    sel = Selected(index, expected, chosen(hyps, index))
    return sel.best, sel, drawn


def from_stochastic(tokens, drawn, nbest, utility, surface=None):
    """mbr_decode(without_replacement=True) after the draws: tokens (B, n, L) int64 on the device and drawn, the Stochastic of
    one stochastic beam search (vagnmt_hip.stochastic); nbest as in from_history.  The samples are the pseudo-references and the
    first n candidates, weighted by their importance weights exp(log_weight) (select_args normalises them per sentence; the
    last sample's weight is 0, a single sample's 1); the beams follow them as candidates.  The tokens stay on the device."""
    hyps = refs = tokens.contiguous()
    if nbest is not None:
        extra = pack(nbest(), "beams").to(tokens.device)
        L = max(refs.shape[2], extra.shape[2])
        hyps = torch.cat([torch.nn.functional.pad(refs, (0, L - refs.shape[2]), value=EOS_token),
                          torch.nn.functional.pad(extra, (0, L - extra.shape[2]), value=0)], 1).contiguous()
    hyps, r, weights, uid = select_args(hyps, None if nbest is None else refs, torch.exp(drawn.log_weight), utility, surface)
    index, expected = _run(hyps, r, weights, uid, surface)
    sel = Selected(index, expected, chosen(hyps, index))
    return sel.best, sel, drawn


def mbr_decode(obj, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, top_p, beam_size, utility, generator,
               beam_groups=1, beam_diversity=0.5, without_replacement=False, surface=None):
    """mbr_decode of a model or an Ensemble: the draws of one sample_decode, then the selection among them (and the
    beam_size-best list: beamsearch_nbest's, or with beam_groups > 1 beamsearch_diverse's) against the samples.
    without_replacement: the draws of one beamsearch_stochastic instead, weighted by their importance weights.
    surface: the target vocabulary's Surface table, with utility "chrf" and only with it."""
    k, uid = decode_args(n_samples, max_length, beam_size, utility, surface, scoring.vocab_of(obj))
    G, lam = diverse.mbr_beam_args(k, beam_groups, beam_diversity)
    nbest = (lambda: obj._nbest(src_var, src_lengths, im_var, k, k, max_length, True, False)[0]) if k else None
    if G > 1:
        nbest = lambda: diverse.beamsearch_diverse(obj, src_var, src_lengths, im_var, k, G, lam, k, max_length, True,  # noqa: E731
                                                   False, "mbr_decode").hyps
    if stochastic.mbr_args(without_replacement, temperature, top_k, top_p):
        res = stochastic.stochastic_search(obj, src_var, src_lengths, im_var, n_samples, max_length, generator, False, False,
                                           "mbr_decode")
        return from_stochastic(res[1], stochastic.assemble(res), nbest, utility, surface)
    toks, lps, _, B, n = sampling.sample_history(obj, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k,
                                                 generator, top_p, False, "mbr_decode")
    return from_history(toks, lps, B, n, nbest, uid, surface)
