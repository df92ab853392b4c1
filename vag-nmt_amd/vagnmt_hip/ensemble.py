"""Ensemble decoding: M trained models that share the source and target vocabularies decode ONE search together.

At every step each member runs its own decoder step and head on the common hypotheses, and the search scores word w of
hypothesis n by the mean of the members' probabilities (include/vag_nmt.h, vag_beam_ens_step):

    s[n, w] = mx + log( (sum_m exp(x_m[n, w] - mx)) / M ),   mx = max_m x_m[n, w],   x_m = member m's log_softmax row

The search is the single model's (vagnmt_hip.search: models/...V11.py:207-226 greedy, :233-337 beam) applied to s, on the
log-probability path at every M (vag_ens_argmax, vag_beam_ens_step*: no raw logits, no one-launch greedy).  Every member keeps its
own encoder, image path and decoder state; the chosen words feed all M decoders and the back-pointers re-order all M hidden
states.  Members may differ in hidden / embedding size, tied_emb, attn_model and multimodal vs text-only (text-only members
ignore ``im_var``).

    ens = Ensemble([best_model, best_loss_model, best_meteor_model])
    hyps = ens.beamsearch_decode(src_var, src_lengths, im_var, beam_size=12, max_length=80)
    nbest, scores = ens.beamsearch_nbest(src_var, src_lengths, im_var, beam_size=12, n_best=5)
    forced = ens.score_translations(src_var, src_lengths, tgt, im_var)       # Scores(score, logp, token_logp)
    a = ens.beamsearch_align(src_var, src_lengths, im_var, beam_size=12, n_best=5)   # + the members' mean attention
    drawn = ens.sample_decode(src_var, src_lengths, im_var, n_samples=4, temperature=0.9, top_k=10)   # Sampled(hyps, ...)
    drawn = ens.sample_decode(src_var, src_lengths, im_var, n_samples=4, top_p=0.9)                   # nucleus sampling
    d = ens.beamsearch_diverse(src_var, src_lengths, im_var, beam_size=12, n_groups=3)     # diverse beam search: Diverse(...)
    c = ens.beamsearch_constrained(src_var, src_lengths, im_var, beam_size=12, prefix=[[17, 5], []], no_repeat_ngram=3)
    r = ens.beamsearch_required(src_var, src_lengths, im_var, beam_size=12, required=[[[17, 5], [230]], []])   # Required(...)
    s = ens.beamsearch_stochastic(src_var, src_lengths, im_var, n_samples=12)    # samples without replacement: Stochastic(...)
    p = ens.beamsearch_penalised(src_var, src_lengths, im_var, beam_size=12, alpha=0.6, beta=0.2, stepwise=True)   # Penalised(...)
"""
import torch

from vagnmt_hip import lm as lm_mod
from vagnmt_hip import align, confidence, constrain, diverse, knn, mbr, penalty, require, sampling, scoring, search, stochastic

MAX_MODELS = 8          # VAG_ENS_MAX (include/vag_nmt.h): the kernels are instantiated for M = 1 .. 8


class Ensemble:
    """A plain object over M models (not an nn.Module: it owns no parameters).  ``beamsearch_decode`` has the models'
    signature and return value; after a beam search ``last_beam_scores`` (B,) and ``last_decode_steps`` are set as on a
    model.  ``decode_graph = False`` runs the same kernels launch by launch instead of replaying captured graphs."""

    decode_graph = True

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("Ensemble: no models")
        if len(models) > MAX_MODELS:
            raise ValueError("Ensemble: %d models, at most %d" % (len(models), MAX_MODELS))
        for m in models:
            if not (hasattr(m, "_decode_prologue") and hasattr(m, "_decode_state") and hasattr(m, "decoder")):
                raise ValueError("Ensemble: %s is not a model of this package" % type(m).__name__)
        for attr in ("tgt_size", "src_size"):
            vals = [int(getattr(m, attr)) for m in models]
            if len(set(vals)) != 1:
                raise ValueError("Ensemble: members disagree on %s: %s" % (attr, vals))
        devs = [next(m.parameters()).device for m in models]
        if len(set(devs)) != 1:
            raise ValueError("Ensemble: members on different devices: %s" % [str(d) for d in devs])
        self.models = models
        self.multimodal = [hasattr(m, "vse_imagine") for m in models]
        self._cache = {}

    def __len__(self):
        return len(self.models)

    # ------------------------------------------------------------------------------------------ public entry
    def beamsearch_decode(self, src_var, src_lengths, im_var=None, beam_size=1, max_length=80, tgt_var=None):
        return self._decode(src_var, src_lengths, im_var, beam_size, max_length, tgt_var)

    def _decode(self, src_var, src_lengths, im_var, beam_size, max_length, tgt_var, device_rows=False):
        """beamsearch_decode, with the models' _decode signature.  device_rows: the search's (B, tgt_l) int64 rows as a GPU tensor
        instead of the cut lists (vagnmt_hip.validate)."""
        self._check_im(im_var)
        tgt_l = max_length if tgt_var is None else tgt_var.size()[1]
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            if beam_size == 1:
                self.last_decode_steps = tgt_l
                mem, hs, e = self._members(pro, 1, tgt_l, "ens_greedy")
                return search.greedy(mem, hs, tgt_l, e, self._pool, device_rows=device_rows)
            return self._beam(pro, int(beam_size), int(tgt_l), device_rows=device_rows)

    def beamsearch_nbest(self, src_var, src_lengths, im_var=None, beam_size=1, n_best=1, max_length=80, avoid_double=True,
                         avoid_unk=False):
        """The models' beamsearch_nbest on the ensemble's scores: (hyps, scores), hyps[b] a list of n_best token lists cut at
        EOS, scores (B, n_best) float32 on the device, descending.  beam_size == 1 runs the beam kernels (not the greedy branch)."""
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk)
        self._check_im(im_var)
        with torch.no_grad():
            return self._beam([m._decode_prologue(src_var, src_lengths, im_var) for m in self.models], k, int(max_length),
                              flags, n)

    def score_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding under the ensemble's scores (members combined per word as in the search): Scores(score (B,),
        logp (B,), token_logp (B, Tt)); tgt as for a model's score_translations."""
        return scoring.score_models(self.models, self.multimodal, src_var, src_lengths, tgt, im_var)

    def token_confidence(self, src_var, src_lengths, tgt, im_var=None):
        """Word-level confidence under the ensemble's scores (vagnmt_hip.confidence): Confidence(score, logp, token_logp, entropy,
        rank, top, top_logp, sentence); tgt as for score_translations."""
        return confidence.token_confidence(self.models, self.multimodal, src_var, src_lengths, tgt, im_var)

    def beamsearch_align(self, src_var, src_lengths, im_var=None, beam_size=1, n_best=1, max_length=80, avoid_double=True,
                         avoid_unk=False):
        """beamsearch_nbest with the attention along every returned hypothesis, the mean of the members' attention rows
        (vagnmt_hip.align: soft attention of the chosen path, not a trained aligner): Aligned(hyps, scores,
        attention (B, n_best, max_length, Ts), src_pos (B, n_best, max_length))."""
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, "beamsearch_align")
        self._check_im(im_var)
        with torch.no_grad():
            return align.Aligned(*self._beam([m._decode_prologue(src_var, src_lengths, im_var) for m in self.models], k,
                                             int(max_length), flags, n, True))

    def align_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding's attention, the mean over the members: Alignment(attention (B, Tt, Ts), src_pos (B, Tt)); tgt as
        for score_translations."""
        return align.align_models(self.models, self.multimodal, src_var, src_lengths, tgt, im_var)

    def sample_decode(self, src_var, src_lengths, im_var=None, n_samples=1, max_length=80, temperature=1.0, top_k=0,
                      generator=None, top_p=1.0, return_sizes=False):
        """The models' sample_decode on the ensemble's scores (vagnmt_hip.sampling): Sampled(hyps, token_logp, logp, score), or
        (Sampled, sizes) with return_sizes.  top_p: nucleus sampling as on a model (1.0 without sizes: the plain decode).
        generator=None: the ensemble's own generator, seeded from torch.initial_seed()."""
        toks, lps, sizes, B, n = self._sample_history(src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k,
                                                      generator, top_p, return_sizes)
        out = sampling.assemble(toks, lps, B, n, toks.device)
        return (out, sampling.assemble_sizes(sizes, B, n)) if return_sizes else out

    def beamsearch_diverse(self, src_var, src_lengths, im_var=None, beam_size=12, n_groups=3, diversity=0.5, n_best=None,
                           max_length=80, avoid_double=True, avoid_unk=False):
        """The models' beamsearch_diverse on the ensemble's scores (vagnmt_hip.diverse): Diverse(hyps, scores (B, n_best),
        group (B, n_best)), n_best None: all beam_size."""
        return self._diverse(src_var, src_lengths, im_var, beam_size, n_groups, diversity, n_best, max_length, avoid_double,
                             avoid_unk)

    def _diverse(self, src_var, src_lengths, im_var, beam_size, n_groups, diversity, n_best, max_length, avoid_double, avoid_unk,
                 what="beamsearch_diverse"):
        k, G, lam, n, flags = diverse.diverse_args(src_var, beam_size, n_groups, diversity, n_best, avoid_double, avoid_unk,
                                                   self.models[0].tgt_size, what)
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, k, int(max_length), "ens_beam_div", flags, diverse=(G, lam))
            res, self.last_beam_scores, self.last_decode_steps = search.beam_diverse(mem, hs, k, G, lam, int(max_length), flags, n,
                                                                                     e, self._pool)
        return diverse.Diverse(*res)

    def beamsearch_stochastic(self, src_var, src_lengths, im_var=None, n_samples=12, max_length=80, generator=None,
                              avoid_double=False, avoid_unk=False):
        """The models' beamsearch_stochastic on the ensemble's scores (vagnmt_hip.stochastic): Stochastic(hyps, logp, score,
        gumbel, log_weight), n_samples distinct translations drawn without replacement from the ensemble's sequence distribution.
        generator=None: the ensemble's own generator."""
        return stochastic.assemble(self._stochastic_search(src_var, src_lengths, im_var, n_samples, max_length, generator,
                                                           avoid_double, avoid_unk))

    def _stochastic_search(self, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double, avoid_unk,
                           what="beamsearch_stochastic"):
        k, ml, flags = stochastic.stochastic_args(src_var, n_samples, max_length, avoid_double, avoid_unk,
                                                  self.models[0].tgt_size, what)
        self._check_im(im_var)
        gen = generator if generator is not None else sampling.default_generator(self)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, k, ml, "ens_beam_sbs", flags)
            res, self.last_beam_scores, self.last_decode_steps = search.beam_stochastic(mem, hs, k, ml, gen.state(pro[0][0].device),
                                                                                        flags, e, self._pool)
            gen.advance()
        return res

    def beamsearch_penalised(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, length_norm="gnmt",
                             alpha=0.6, beta=0.2, word_bonus=0.0, stepwise=False, avoid_double=True, avoid_unk=False,
                             no_repeat_ngram=0):
        """The models' beamsearch_penalised on the ensemble's scores (vagnmt_hip.penalty): Penalised(hyps, scores, logp, length,
        coverage_penalty).  The coverage is that of the members' mean attention rows, as in beamsearch_align."""
        what = "beamsearch_penalised"
        V = int(self.models[0].tgt_size)
        k, n, ml, flags, beta, stepwise = penalty.penalised_args(src_var, beam_size, n_best, max_length, length_norm, alpha, beta,
                                                                 word_bonus, stepwise, avoid_double, avoid_unk, V, what)
        packed = constrain.pack(src_var.shape[0], V, ml, no_repeat_ngram=no_repeat_ngram, avoid_double=avoid_double,
                                avoid_unk=avoid_unk, what=what)
        lp, bonus = penalty.tables(ml, length_norm, alpha, word_bonus)
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, k, ml, "ens_beam_pen", flags, True, constrain=packed.ngram if packed.ngram else None,
                                       penalty=(beta, stepwise))
            con = constrain.Constraints(packed, pro[0][0].shape[0], ml, pro[0][0].device, e) if packed.ngram else None
            res, self.last_beam_scores, self.last_decode_steps = search.beam_penalised(mem, hs, k, ml, lp, bonus, beta, stepwise,
                                                                                       flags, n, e, self._pool, constrain=con)
        return penalty.assemble(res)

    def beamsearch_constrained(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, prefix=None,
                               banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False):
        """The models' beamsearch_constrained on the ensemble's scores (vagnmt_hip.constrain): Constrained(hyps, scores
        (B, n_best)).  A ban writes -1e5 into every member's row, so the ensemble sees it as a single model does."""
        what = "beamsearch_constrained"
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
        ml = int(max_length)
        packed = constrain.pack(src_var.shape[0], int(self.models[0].tgt_size), ml, prefix, banned, banned_per_sentence,
                                no_repeat_ngram, avoid_double, avoid_unk, what)
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, k, ml, "ens_beam_con", flags, constrain=packed.ngram)
            con = constrain.Constraints(packed, pro[0][0].shape[0], ml, pro[0][0].device, e)
            res, self.last_beam_scores, self.last_decode_steps = search.beam(mem, hs, k, ml, flags, n, e, self._pool,
                                                                             constrain=con)
        return constrain.Constrained(*res)

    def beamsearch_knn(self, src_var, src_lengths, im_var=None, datastore=None, beam_size=12, n_best=1, max_length=80, k=8,
                       temperature=10.0, lam=0.5, return_neighbours=False, avoid_double=True, avoid_unk=False, prefix=None,
                       banned=None, banned_per_sentence=None, no_repeat_ngram=0):
        """The models' beamsearch_knn on the ensemble's scores (vagnmt_hip.knn): ``datastore`` is a list with one store per
        member, each built with that member; member m's rows are mixed with member m's neighbours, and the mean of the mixed
        probabilities is the mixture of the means, so the expansion is the ensemble's own.  KnnSearch(hyps, scores[, neighbours:
        one Neighbours per member])."""
        return knn.beamsearch_knn(self, src_var, src_lengths, im_var, datastore, beam_size, n_best, max_length, k, temperature, lam,
                                  return_neighbours, avoid_double, avoid_unk, prefix, banned, banned_per_sentence, no_repeat_ngram)

    def knn_score_translations(self, src_var, src_lengths, tgt, im_var=None, datastore=None, k=8, temperature=10.0, lam=0.5):
        """score_translations under the distribution of beamsearch_knn (vagnmt_hip.knn.knn_score_translations)."""
        return knn.knn_score_translations(self, src_var, src_lengths, tgt, im_var, datastore, k, temperature, lam)

    def _knn_search(self, src_var, src_lengths, im_var, stores, k, n, ml, flags, K, temperature, lam, packed):
        """The ensemble's side of knn.beamsearch_knn, as a model's: (hyps, scores)."""
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            if lam == 0.0 and packed is None:
                return self._beam(pro, k, ml, flags, n)
            mem, hs, e = self._members(pro, k, ml, "ens_beam_knn", flags, constrain=packed.ngram if packed is not None else None,
                                       knn=knn.graph_key(stores, K, temperature, lam) if lam > 0.0 else None)
            B, dev = pro[0][0].shape[0], pro[0][0].device
            con = constrain.Constraints(packed, B, ml, dev, e) if packed is not None else None
            mix = knn.StepMix(knn.Retrieval(stores, B * k, K, dev, e), int(self.models[0].tgt_size), temperature, lam) \
                if lam > 0.0 else None
            res, self.last_beam_scores, self.last_decode_steps = search.beam(mem, hs, k, ml, flags, n, e, self._pool, constrain=con,
                                                                             knn=mix)
        return res

    def beamsearch_lm(self, src_var, src_lengths, im_var=None, lm=None, beta=0.3, beam_size=12, n_best=1, max_length=80,
                      avoid_double=True, avoid_unk=False, prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0):
        """The models' beamsearch_lm on the ensemble's scores (vagnmt_hip.lm): ONE language model, its term added to every
        member's row -- the same term in every member commutes with the log-mean, so the expansion is the ensemble's own.
        LmSearch(hyps, scores)."""
        return lm_mod.beamsearch_lm(self, src_var, src_lengths, im_var, lm, beta, beam_size, n_best, max_length, avoid_double,
                                avoid_unk, prefix, banned, banned_per_sentence, no_repeat_ngram)

    def lm_score_translations(self, src_var, src_lengths, tgt, im_var=None, lm=None, beta=0.3):
        """score_translations under the fused score of beamsearch_lm (vagnmt_hip.lm.lm_score_translations)."""
        return lm_mod.lm_score_translations(self, src_var, src_lengths, tgt, im_var, lm, beta)

    def _lm_search(self, src_var, src_lengths, im_var, model, beta, k, n, ml, flags, packed):
        """The ensemble's side of lm.beamsearch_lm, as a model's: (hyps, scores)."""
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            if beta == 0.0 and packed is None:
                return self._beam(pro, k, ml, flags, n)
            mem, hs, e = self._members(pro, k, ml, "ens_beam_lm", flags, constrain=packed.ngram if packed is not None else None,
                                       lm=lm_mod.graph_key(model, beta) if beta != 0.0 else None)
            B, dev = pro[0][0].shape[0], pro[0][0].device
            con = constrain.Constraints(packed, B, ml, dev, e) if packed is not None else None
            fuse = lm_mod.StepFuse(model, beta, e) if beta != 0.0 else None
            res, self.last_beam_scores, self.last_decode_steps = search.beam(mem, hs, k, ml, flags, n, e, self._pool, constrain=con,
                                                                             lm=fuse)
        return res

    def beamsearch_required(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, required=None,
                            prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True,
                            avoid_unk=False):
        """The models' beamsearch_required on the ensemble's scores (vagnmt_hip.require): Required(hyps, scores (B, n_best), met
        (B, n_best), complete (B, n_best)).  The phrase state follows the common hypotheses, so it is the single model's."""
        what = "beamsearch_required"
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
        ml, B, V = int(max_length), src_var.shape[0], int(self.models[0].tgt_size)
        packed = constrain.pack(B, V, ml, prefix, banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk, what)
        table = require.pack(B, V, ml, required, banned, banned_per_sentence, avoid_double, avoid_unk, what)
        negative = bool(packed.prefix.any()) or len(packed.phrases) > 0 or packed.ngram > 0
        self._check_im(im_var)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, k, ml, "ens_beam_req", flags, constrain=packed.ngram if negative else None)
            con = constrain.Constraints(packed, B, ml, pro[0][0].device, e) if negative else None
            res, self.last_beam_scores, self.last_decode_steps = search.beam_required(mem, hs, k, ml, table, flags, k, e,
                                                                                      self._pool, constrain=con)
        return require.assemble(*res, table, n)

    def mbr_decode(self, src_var, src_lengths, im_var=None, n_samples=16, max_length=80, temperature=1.0, top_k=0, top_p=1.0,
                   beam_size=0, utility="bleu", generator=None, beam_groups=1, beam_diversity=0.5, without_replacement=False,
                   surface=None):
        """The models' mbr_decode on the ensemble's scores (vagnmt_hip.mbr): the draws of one sample_decode, then the candidate
        of highest expected utility against them; beam_size > 0 adds the ensemble's beam_size-best list to the candidates
        (beam_groups > 1: the list of beamsearch_diverse).  Returns (best, Selected, Sampled).  without_replacement=True: the
        draws of one beamsearch_stochastic, weighted by exp(log_weight); the third result is then the Stochastic."""
        k, uid = mbr.decode_args(n_samples, max_length, beam_size, utility, surface, self.models[0].tgt_size)
        G, lam = diverse.mbr_beam_args(k, beam_groups, beam_diversity)
        nbest = (lambda: self.beamsearch_nbest(src_var, src_lengths, im_var, k, k, max_length)[0]) if k else None
        if G > 1:
            nbest = lambda: self._diverse(src_var, src_lengths, im_var, k, G, lam, k, max_length, True, False,  # noqa: E731
                                          "mbr_decode").hyps
        if stochastic.mbr_args(without_replacement, temperature, top_k, top_p):
            res = self._stochastic_search(src_var, src_lengths, im_var, n_samples, max_length, generator, False, False,
                                          "mbr_decode")
            return mbr.from_stochastic(res[1], stochastic.assemble(res), nbest, utility, surface)
        toks, lps, _, B, n = self._sample_history(src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k,
                                                  generator, top_p, False, "mbr_decode")
        return mbr.from_history(toks, lps, B, n, nbest, uid, surface)

    def _sample_history(self, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator, top_p,
                        return_sizes, what="sample_decode"):
        """The draws of sample_decode / mbr_decode, the generator advanced once: the sampler's time-major history on the device,
        (toks, lps, sizes or None, B, n)."""
        self._check_im(im_var)
        p = sampling.check_top_p(top_p, what)
        n, ml, t, k = sampling.check_args(src_var, n_samples, max_length, temperature, top_k, what)
        gen = generator if generator is not None else sampling.default_generator(self)
        with torch.no_grad():
            pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
            mem, hs, e = self._members(pro, n, ml, "ens_sample", sample=(t, k) + sampling.nucleus_key(p, return_sizes))
            dev, B = pro[0][0].device, pro[0][0].shape[0]
            sizes = torch.empty(ml, B * n, dtype=torch.int32, device=dev) if return_sizes else None
            toks, lps, self.last_decode_steps = search.sample(mem, hs, n, ml, t, k, gen.state(dev), e, self._pool, top_p=p,
                                                              sizes=sizes)
            gen.advance()
            return toks, lps, sizes, B, n

    def _check_im(self, im_var):
        if im_var is None and any(self.multimodal):
            raise ValueError("Ensemble: a multimodal member needs im_var")

    def _beam(self, pro, k, max_length, flags=0, n_best=0, aligning=False, device_rows=False):
        mem, hs, e = self._members(pro, k, max_length, "ens_beam", flags, aligning)
        res, self.last_beam_scores, self.last_decode_steps = search.beam(mem, hs, k, max_length, flags, n_best, e, self._pool,
                                                                         align=aligning, device_rows=device_rows)
        return res

    # ------------------------------------------------------------------------------------------ cache
    def _members(self, pro, k, max_length, kind, flags=0, aligning=False, sample=None, diverse=None, constrain=None,
                 penalty=None, knn=None, lm=None):
        """(members, initial hidden states, entry) of one search.  In graph mode each member runs on its model's own static
        buffers of this shape under kind ("ens_greedy" / "ens_beam": a member's own decode graphs stay untouched), and the
        entry holds the ensemble's search buffers and captured graph.  Its key holds the members' state dicts by identity and
        the entry holds the dicts themselves: a member that rebuilds its state makes a new entry, and the buffers a captured
        graph reads stay alive as long as the graph.  flags are a by-value argument of the captured expansions: part of the key.
        An aligning search captures another graph: it has entries of its own (the members' and the ensemble's).  sample:
        (temperature, top_k[, top_p, sizes recorded]) of a sampling decode, by-value arguments too; its members run the plain steps in
        both modes.  diverse: (groups, strength) of a diverse beam search, by-value arguments as well.  constrain: the
        no-repeat n of a constrained search, a by-value argument of its mask launches; the entry also owns the static
        constraint buffers those launches point at.  penalty: (beta, stepwise) of a penalised search, by-value arguments of its
        captured launches; the entry owns the carried lengths, coverage and penalties and the two tables.  knn: the graph_key of
        a kNN search (vagnmt_hip.knn), held by its captured launches by value and by pointer; the entry owns the neighbour lists
        and keeps the stores alive.  lm: the graph_key of a search fused with a language model (vagnmt_hip.lm), held by its
        captured launches by value and by pointer; the entry keeps the model alive."""
        graphed = self.decode_graph and pro[0][0].is_cuda
        mem = [search.Member(m, enc, mask, k, max_length, kind if graphed else None, align=aligning, hoist=sample is None,
                             sample=sample, diverse=diverse, constrain=constrain, penalty=penalty, knn=knn, lm=lm)
               for m, (enc, mask, _) in zip(self.models, pro)]
        hs = [h0 for (_, _, h0) in pro]
        if not graphed:
            return mem, hs, None
        key = (kind, pro[0][0].shape[0], k, max_length, flags) + (("align",) if aligning else ()) + \
            ((("sample",) + tuple(sample)) if sample is not None else ()) + \
            ((("diverse",) + tuple(diverse)) if diverse is not None else ()) + \
            (("constrain", constrain) if constrain is not None else ()) + \
            ((("penalty",) + tuple(penalty)) if penalty is not None else ()) + \
            ((("knn",) + tuple(knn)) if knn is not None else ()) + \
            ((("lm",) + tuple(lm)) if lm is not None else ()) + tuple(id(mb.st) for mb in mem)
        e = self._cache.get(key)
        if e is None:
            if len(self._cache) >= 32:
                self._cache.clear()
            e = self._cache[key] = {"graph": None}
        e["members"] = [mb.st for mb in mem]
        return mem, hs, e

    def _pool(self):
        pool = self._cache.get("__pool__")
        if pool is None:
            pool = self._cache["__pool__"] = torch.cuda.graph_pool_handle()
        return pool
