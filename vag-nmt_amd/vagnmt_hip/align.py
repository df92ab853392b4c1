"""Attention alignments: which source positions each translated word looked at -- the decoder's Bahdanau attention
(layers/NMT_Decoder.py:27-51) along a hypothesis of the beam search or along a given translation.  This is the SOFT ATTENTION OF
THE CHOSEN PATH, not a trained aligner: good for replacing UNK by the aligned source word, for exporting rough word alignments
of a parallel corpus and for the attention heat maps of the VAG-NMT paper.

    a = model.beamsearch_align(src_var, src_lengths, im_var, beam_size=12, n_best=5, max_length=80)
    a.hyps[b][r]                 token list of sentence b's r-th best hypothesis, cut at EOS
    a.scores (B, n)              their length-normalised scores (device), as beamsearch_nbest returns them
    a.attention (B, n, L, Ts)    row t = the attention that produced word t; 0 after the hypothesis's EOS row (device)
    a.src_pos (B, n, L)          arg-max source position of each row (lowest index among equal values), -1 for a zeroed row

    f = model.align_translations(src_var, src_lengths, tgt, im_var)       # Alignment(attention (B, Tt, Ts), src_pos (B, Tt))

The search keeps every step's attention rows in a history buffer (vag_beam_attn_record: one small launch per step, inside the
captured decode graph) and its finish walks the back-pointers through it (vag_beam_finish_align); forced decoding reads the
attention the teacher-forced sequence kernel keeps for its backward pass (vag_forced_align).  An Ensemble averages its members'
attention rows.  ``unk_links`` / ``replace_unk`` are host helpers on lists and a CPU copy of src_pos."""
import ctypes as C
from collections import namedtuple

import torch

from vagnmt_hip import ops, scoring
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.search import UNK_token

Aligned = namedtuple("Aligned", ["hyps", "scores", "attention", "src_pos"])
Alignment = namedtuple("Alignment", ["attention", "src_pos"])


def _member_alpha(model, src_var, src_lengths, im_var, tok):
    """Teacher-forced attention (Tt, B, Ts) of one model: what its sequence kernel saved (ops.cgru_decode_seq_alpha)."""
    enc, mask, h0 = model._decode_prologue(src_var, src_lengths, im_var)
    dec = model.decoder
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    return ops.cgru_decode_seq_alpha(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=dec.out.bias.shape[0])


def align_models(models, multimodal, src_var, src_lengths, tgt, im_var=None):
    """align_translations of one model (M = 1) or of an ensemble's members; returns Alignment(attention, src_pos)."""
    tgt, tok = scoring.forced_args(models, multimodal, src_var, tgt, im_var, "align_translations")
    B, Tt = tgt.shape
    Ts = src_var.shape[1]
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()                                          # inference: no dropout whatever the models' modes
        with torch.no_grad():
            alphas = [_member_alpha(m, src_var, src_lengths, im_var, tok) for m in models]
            attention = torch.empty(B, Tt, Ts, device=tgt.device)
            src_pos = torch.empty(B, Tt, dtype=torch.int64, device=tgt.device)
            M = len(alphas)
            call("vag_forced_align", (C.c_void_p * M)(*[ptr(a) for a in alphas]), M, ptr(tgt, torch.int64), B, Tt, Ts,
                 ptr(attention), ptr(src_pos, torch.int64), stream())
    finally:
        for m, t in zip(models, modes):
            m.train(t)
    return Alignment(attention, src_pos)


def beamsearch_align(obj, src_var, src_lengths, im_var, beam_size, n_best, max_length, avoid_double, avoid_unk):
    """beamsearch_align of a model or an Ensemble: beamsearch_nbest's search with every member keeping its attention rows
    (decode states and entries of their own: ("align",) in their keys) -> Aligned."""
    k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, "beamsearch_align")
    return Aligned(*scoring.nbest_search(obj, src_var, src_lengths, im_var, k, int(max_length), flags, n, align=True))


def _pos_lists(src_pos):
    """src_pos as nested lists and whether it is the n-best form (B, n, L) rather than (B, L)."""
    pos = src_pos.tolist() if hasattr(src_pos, "tolist") else src_pos
    nested = len(pos) > 0 and len(pos[0]) > 0 and isinstance(pos[0][0], (list, tuple))
    return pos, nested


def _links(h, p, unk):
    return [(t, int(p[t])) for t, w in enumerate(h) if int(w) == unk and t < len(p) and int(p[t]) >= 0]


def unk_links(hyps, src_pos, unk=UNK_token):
    """Per hypothesis, the (target position, source position) pairs of its UNK words.  hyps with src_pos (B, n, L) as
    beamsearch_align returns them (hyps[b][r] a token list), or one token list per sentence with src_pos (B, L); src_pos a CPU
    tensor, an array or nested lists.  Words without an alignment (src_pos -1) are left out."""
    pos, nested = _pos_lists(src_pos)
    if nested:
        return [[_links(h, p, unk) for h, p in zip(hs, ps)] for hs, ps in zip(hyps, pos)]
    return [_links(h, p, unk) for h, p in zip(hyps, pos)]


def replace_unk(tgt_words, hyps, src_pos, src_words, lexicon=None, unk=UNK_token):
    """The hypotheses' word lists (tgt_words, shaped like hyps) with every UNK replaced by its aligned source word
    src_words[b][source position], translated where the lexicon has an entry: lexicon.get(src_word, src_word).  An UNK without
    an alignment (src_pos -1, or a position outside src_words[b]) keeps its word."""
    lexicon = lexicon or {}
    links, nested = unk_links(hyps, src_pos, unk), _pos_lists(src_pos)[1]

    def fix(words, lk, src):
        words = list(words)
        for t, s in lk:
            if t < len(words) and s < len(src):
                words[t] = lexicon.get(src[s], src[s])
        return words

    if nested:
        return [[fix(w, lk, src) for w, lk in zip(ws, lks)] for ws, lks, src in zip(tgt_words, links, src_words)]
    return [fix(w, lk, src) for w, lk, src in zip(tgt_words, links, src_words)]
