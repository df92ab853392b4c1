"""VAG-NMT multimodal model, drop-in for models/NMT_AttentionImagine_Seq2Seq_Beam_V11.py of the reference."""
import torch
import torch.nn as nn

from vagnmt_hip import align, confidence, constrain, diverse, mbr, ops, penalty, require, sampling, scoring, stochastic
from vagnmt_hip.align import align_models

from ..layers import LIUMCVC_Encoder, NMT_Decoder, VSE_Imagine_Enc
from ._seq2seq import Seq2SeqBase, SOS_token, EOS_token


class NMT_AttentionImagine_Seq2Seq_Beam_V11(Seq2SeqBase):
    """Same positional constructor arguments, attributes and method signatures as the reference class
    (models/...V11.py:21-80).  forward() returns (loss, loss_mt, loss_vse) with
    loss = loss_w * loss_mt + (1 - loss_w) * loss_vse (V11.py:166)."""

    def __init__(self, src_size, tgt_size, im_feats_size, src_embedding_size, tgt_embedding_size, hidden_size,
                 shared_embedding_size, loss_w, beam_size=1, attn_model='dot', n_layers=1, dropout_ctx=0.0,
                 dropout_emb=0.0, dropout_out=0.0, dropout_rnn_enc=0.0, dropout_rnn_dec=0.0, dropout_im_emb=0.0,
                 dropout_txt_emb=0.0, activation_vse=True, tied_emb=False, init_split=0.5):
        super(NMT_AttentionImagine_Seq2Seq_Beam_V11, self).__init__()
        self.src_size = src_size
        self.tgt_size = tgt_size
        self.im_feats_size = im_feats_size
        self.src_embedding_size = src_embedding_size
        self.tgt_embedding_size = tgt_embedding_size
        self.hidden_size = hidden_size
        self.n_layers = n_layers
        self.shared_embedding_size = shared_embedding_size
        self.beam_size = beam_size
        self.loss_w = loss_w
        self.tied_emb = tied_emb
        self.dropout_im_emb = dropout_im_emb
        self.dropout_txt_emb = dropout_txt_emb
        self.activation_vse = activation_vse
        self.attn_model = attn_model
        self.init_split = init_split
        self.encoder = LIUMCVC_Encoder(src_size, src_embedding_size, hidden_size, n_layers, dropout_rnn=dropout_rnn_enc,
                                       dropout_ctx=dropout_ctx, dropout_emb=dropout_emb)
        self.decoder = NMT_Decoder(tgt_size, tgt_embedding_size, hidden_size, 2 * hidden_size, n_layers,
                                   dropout_rnn=dropout_rnn_dec, dropout_out=dropout_out, dropout_emb=0.0,
                                   tied_emb=tied_emb)
        self.vse_imagine = VSE_Imagine_Enc(self.attn_model, self.im_feats_size, 2 * hidden_size,
                                           self.shared_embedding_size, self.dropout_im_emb, self.dropout_txt_emb,
                                           self.activation_vse)
        self.decoderini = nn.Linear(2 * hidden_size, hidden_size)
        self.reset_parameters()

    def _prologue(self, src_var, src_lengths, im_var, criterion_vse, rng):
        enc, mask = self._encode(src_var, src_lengths, rng)
        loss_vse, ctx = self.vse_imagine.forward_bm(im_var, enc, mask, criterion_vse)
        h0 = ops.DecInit.apply(enc, mask, ctx, self.decoderini.weight, self.decoderini.bias, self.init_split)
        return enc, mask, loss_vse, h0

    def _decode_prologue(self, src_var, src_lengths, im_var=None):
        """Inference prologue of decoding and scoring -> (enc, mask, h0)."""
        enc, mask, _, h0 = self._prologue(src_var, src_lengths, im_var, None, None)
        return enc, mask, h0

    def forward(self, src_var, src_lengths, tgt_var, im_var, teacher_force_ratio=1.0, max_length=80, criterion_mt=None,
                criterion_vse=None):
        """src_var (B,W_s) int64 (pad 0, rows sorted by length, descending); src_lengths list[B]; tgt_var (B,W_t) int64;
        im_var (B,I) fp32.  Returns (loss, loss_mt, loss_vse)."""
        self.tgt_l = tgt_var.size()[1]
        rng = self._train_rng(src_var.device)
        enc, mask, loss_vse, h0 = self._prologue(src_var, src_lengths, im_var, criterion_vse, rng)
        loss_mt = self._translation_loss(enc, mask, h0, tgt_var, teacher_force_ratio, criterion_mt, rng)
        loss = self.loss_w * loss_mt + (1 - self.loss_w) * loss_vse
        return loss, loss_mt, loss_vse

    def beamsearch_decode(self, src_var, src_lengths, im_var, beam_size=1, max_length=80, tgt_var=None):
        return self._decode(src_var, src_lengths, im_var, beam_size, max_length, tgt_var)

    def beamsearch_nbest(self, src_var, src_lengths, im_var, beam_size, n_best, max_length=80, avoid_double=True,
                         avoid_unk=False):
        """The n_best best hypotheses of the beam search (V11.py:233-337) and their length-normalised scores: returns (hyps,
        scores), hyps[b] a list of n_best token lists cut at EOS, scores (B, n_best) float32 on the device, descending.  With the
        default options hyps[b][0] is beamsearch_decode(..., beam_size, ...)[b].  1 <= n_best <= beam_size <= 64."""
        return self._nbest(src_var, src_lengths, im_var, beam_size, n_best, max_length, avoid_double, avoid_unk)

    def score_translations(self, src_var, src_lengths, tgt, im_var):
        """Forced decoding: Scores(score (B,), logp (B,), token_logp (B, Tt)) of the given targets -- a (B, Tt) int64 tensor
        (pad 0) or B token lists (EOS appended where missing).  Inference only (no gradient, no dropout)."""
        return scoring.score_models([self], [True], src_var, src_lengths, tgt, im_var)

    def token_confidence(self, src_var, src_lengths, tgt, im_var):
        """Word-level confidence of the given targets (vagnmt_hip.confidence): Confidence(score, logp, token_logp, entropy, rank,
        top, top_logp, sentence) -- the first three are score_translations', then the softmax entropy, the given word's rank, the
        two best words with their log-probabilities (B, Tt[, 2]) and the sentence's eight features.  Inference only."""
        return confidence.token_confidence([self], [True], src_var, src_lengths, tgt, im_var)

    def sample_decode(self, src_var, src_lengths, im_var=None, n_samples=1, max_length=80, temperature=1.0, top_k=0,
                      generator=None, top_p=1.0, return_sizes=False):
        """Translations drawn from the model's distribution (vagnmt_hip.sampling): n_samples per sentence, each word drawn
        from softmax(log p / temperature) over the top_k most probable words (0: the whole vocabulary, at most 64), for at most
        max_length steps.  Returns Sampled(hyps, token_logp (B, n_samples, max_length), logp (B, n_samples), score (B, n_samples)):
        hyps[b] holds n_samples token lists cut at EOS; token_logp is the model's own log-probability of each drawn word (what
        score_translations gives), logp its sum and score the beam search's length normalisation of it.  generator: a
        vagnmt_hip.sampling.Generator (None: this model's own, seeded from torch.initial_seed()); the same generator state
        gives the same samples.  top_k=1 is greedy decoding.  top_p in (0, 1]: nucleus sampling, the draw restricted to the best
        of those words that carry top_p of their tempered mass (1.0: all of them); return_sizes=True returns (Sampled, sizes), sizes
        (B, n_samples, max_length) int32 the number of words each draw chose from, 0 after a sample's first EOS.  Inference only."""
        return sampling.sample_decode(self, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator,
                                      top_p, return_sizes)

    def beamsearch_diverse(self, src_var, src_lengths, im_var=None, beam_size=12, n_groups=3, diversity=0.5, n_best=None,
                           max_length=80, avoid_double=True, avoid_unk=False):
        """Diverse beam search (vagnmt_hip.diverse): the beam_size slots in n_groups groups, a group paying ``diversity`` for every
        slot of an earlier group that chose the same word at that step.  Returns Diverse(hyps, scores, group): hyps[b] the n_best
        (default: all beam_size) token lists cut at EOS, scores (B, n_best) float32 on the device, descending -- the model's own
        length-normalised scores, without the penalty -- and group (B, n_best) int64, the group each hypothesis ended in.
        n_groups must divide beam_size <= 64; n_groups=1 is beamsearch_nbest, diversity=0 gives n_groups copies of a search of
        width beam_size / n_groups.  Inference only."""
        return diverse.beamsearch_diverse(self, src_var, src_lengths, im_var, beam_size, n_groups, diversity, n_best, max_length,
                                          avoid_double, avoid_unk)

    def beamsearch_stochastic(self, src_var, src_lengths, im_var=None, n_samples=12, max_length=80, generator=None,
                              avoid_double=False, avoid_unk=False):
        """Stochastic beam search (vagnmt_hip.stochastic; Kool et al. 2019): n_samples distinct translations per sentence, an exact
        sample WITHOUT replacement from the model's sequence distribution.  Returns Stochastic(hyps, logp, score, gumbel,
        log_weight): hyps[b] the n_samples token lists cut at EOS in sampling order, logp (B, n_samples) the model's total
        log-probability of each (what score_translations gives), score its length-normalised form, gumbel the perturbed scores,
        descending, and log_weight the log importance weights (sbs_log_weights: -inf for the last sample) -- all float32 on the
        device.  generator: a vagnmt_hip.sampling.Generator as for sample_decode (None: this model's own); it advances once
        per call and the same state gives the same samples.  avoid_double defaults to False, unlike the beam searches: the draw
        is from the model's own distribution.  There is no temperature, top_k or top_p: a tempered sequence distribution would
        need every step renormalised.  Inference only."""
        return stochastic.beamsearch_stochastic(self, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double,
                                                avoid_unk)

    def beamsearch_penalised(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, length_norm="gnmt",
                             alpha=0.6, beta=0.2, word_bonus=0.0, stepwise=False, avoid_double=True, avoid_unk=False,
                             no_repeat_ngram=0):
        """Beam search with GNMT length and coverage penalties (vagnmt_hip.penalty; Wu et al. 2016, section 7): every hypothesis
        scores s = (logp + word_bonus L) / lp(L) + cp, L = max(1, #words > 3), lp = ((5 + L) / 6)^alpha (length_norm="gnmt"),
        L^alpha ("length") or 1 ("none"), cp = beta * sum_i log(min(coverage_i, 1)) over the source positions.  stepwise=False
        re-ranks beamsearch_nbest's hypotheses at the finish; stepwise=True selects by s at every step (OpenNMT's
        stepwise_penalty).  Returns Penalised(hyps, scores, logp, length, coverage_penalty): hyps[b] the n_best token lists cut at
        EOS, best first, and per hypothesis its penalised score, the model's total log-probability (what score_translations
        gives), its number of words above 3 (int32) and its coverage penalty, all (B, n_best) on the device.
        length_norm="length", alpha=1, beta=0, word_bonus=0 is beamsearch_nbest bit for bit.  no_repeat_ngram = n >= 1: no n-gram
        occurs twice (beamsearch_constrained's rule).  Inference only."""
        return penalty.beamsearch_penalised(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, length_norm, alpha,
                                            beta, word_bonus, stepwise, avoid_double, avoid_unk, no_repeat_ngram)

    def beamsearch_constrained(self, src_var, src_lengths, im_var, beam_size=12, n_best=1, max_length=80, prefix=None,
                               banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False):
        """Constrained beam search (vagnmt_hip.constrain): beamsearch_nbest whose output begins with ``prefix`` (a list of B token
        lists, empty for none, or a (B, Lp) int64 tensor padded with 0), contains none of the words and phrases of ``banned``
        (token lists, every sentence) and ``banned_per_sentence`` (B such lists), and with no_repeat_ngram = n >= 1 repeats no
        n-gram.  Returns Constrained(hyps, scores): hyps[b] the n_best token lists cut at EOS, the forced words included, best
        first; scores (B, n_best) float32 on the device, descending -- the model's own length-normalised scores.  Hypotheses the
        constraints left no live continuation for score below -1e4 and are returned as they are.  Inference only."""
        return constrain.beamsearch_constrained(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, prefix, banned,
                                                banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk)

    def beamsearch_required(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, required=None, prefix=None,
                            banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False):
        """Beam search whose output must contain given phrases (vagnmt_hip.require; dynamic beam allocation): ``required`` is a
        list of B lists of phrases (token lists of 1 .. 8 words, at most 16 per sentence).  The beam's slots are dealt over the
        hypotheses' progress with their phrases, EOS is ruled out while a phrase is open; prefix / banned / banned_per_sentence /
        no_repeat_ngram are beamsearch_constrained's and combine with it.  Returns Required(hyps, scores (B, n_best), met
        (B, n_best) int64 bitmask, complete (B, n_best) bool): the hypotheses that met all their phrases first, best first in
        each part, scores the model's own length-normalised ones.  A search that reaches max_length with phrases open returns
        such hypotheses flagged incomplete.  Nothing required and no negative constraints: beamsearch_nbest.  Inference only."""
        return require.beamsearch_required(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, required, prefix,
                                           banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk)

    def mbr_decode(self, src_var, src_lengths, im_var=None, n_samples=16, max_length=80, temperature=1.0, top_k=0, top_p=1.0,
                   beam_size=0, utility="bleu", generator=None, beam_groups=1, beam_diversity=0.5, without_replacement=False,
                   surface=None):
        """Minimum-Bayes-risk decoding (vagnmt_hip.mbr): draws n_samples translations as sample_decode does (temperature, top_k,
        top_p, generator: the same meaning, and the generator advances exactly as in one sample_decode call), takes them as
        candidates and as pseudo-references, and chooses per sentence the candidate with the highest expected utility ("bleu":
        segment-level smooth BLEU, "ngram_f": an n-gram F score) -- on the device (vag_mbr_select).  beam_size > 0 adds the
        beam_size-best list of beamsearch_nbest as further candidates, after the samples; the pseudo-references stay the
        samples; beam_groups > 1 takes that list from beamsearch_diverse(beam_size, beam_groups, beam_diversity) instead
        (beam_groups=1: beam_diversity is not looked at).  Returns (best, Selected(index (B,), expected (B, n_samples + beam_size),
        best), Sampled).  without_replacement=True draws the n_samples with beamsearch_stochastic instead (distinct translations; the
        same generator, advanced once) and weights them as pseudo-references by their importance weights exp(log_weight); the
        third result is then the Stochastic.  It is an error together with temperature != 1, top_k or top_p.  utility="chrf" with
        surface=Surface(words) (vagnmt_hip.surface) rates the candidates by chrF on the characters their ids spell.  Inference only."""
        return mbr.mbr_decode(self, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, top_p, beam_size,
                              utility, generator, beam_groups, beam_diversity, without_replacement, surface)

    def beamsearch_align(self, src_var, src_lengths, im_var, beam_size, n_best, max_length=80, avoid_double=True,
                         avoid_unk=False):
        """beamsearch_nbest with the decoder's attention along every returned hypothesis -- the soft attention of the chosen
        path, not a trained aligner (vagnmt_hip.align): Aligned(hyps, scores, attention (B, n_best, max_length, Ts),
        src_pos (B, n_best, max_length)), hyps and scores as beamsearch_nbest returns them, attention and src_pos on the device.
        Row t is the attention that produced word t; rows after the hypothesis's EOS row are 0 with src_pos -1."""
        return align.beamsearch_align(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, avoid_double, avoid_unk)

    def align_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding's attention: Alignment(attention (B, Tt, Ts), src_pos (B, Tt)) of the given targets (as for
        score_translations), 0 / -1 outside the span score_translations counts.  Inference only (no gradient, no dropout)."""
        return align_models([self], [True], src_var, src_lengths, tgt, im_var)

    # ---- image retrieval (V11.py:341-397) ----
    def embed_sent_im_eval(self, src_var, src_lengths, tgt_var, im_feats):
        self.tgt_l = tgt_var.size()[1]
        return self._embed(src_var, src_lengths, im_feats)

    def embed_sent_im_test(self, src_var, src_lengths, im_feats, max_length=80):
        self.tgt_l = max_length
        return self._embed(src_var, src_lengths, im_feats)

    def _embed(self, src_var, src_lengths, im_feats):
        with torch.no_grad():
            enc, mask = self._encode(src_var, src_lengths, None)
            im_emb, txt_emb, _, _ = self.vse_imagine.embed_bm(im_feats, enc, mask)
        return im_emb.data, txt_emb.data

    def get_imagine_attention_eval(self, src_var, src_lengths, tgt_var, im_feats):
        self.tgt_l = tgt_var.size()[1]
        return self._imagine_weights(src_var, src_lengths, im_feats)

    def get_imagine_attention_test(self, src_var, src_lengths, im_feats, max_length=80):
        self.tgt_l = max_length
        return self._imagine_weights(src_var, src_lengths, im_feats)

    def _imagine_weights(self, src_var, src_lengths, im_feats):
        with torch.no_grad():
            enc, mask = self._encode(src_var, src_lengths, None)
            _, _, alpha, _ = self.vse_imagine.embed_bm(im_feats, enc, mask)
        return alpha.unsqueeze(1).data
