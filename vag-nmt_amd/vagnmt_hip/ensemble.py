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

    _nbest = beamsearch_nbest               # under the models' name for it (vagnmt_hip.mbr asks either for its beam_size-best list)

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
        return align.beamsearch_align(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, avoid_double, avoid_unk)

    def align_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding's attention, the mean over the members: Alignment(attention (B, Tt, Ts), src_pos (B, Tt)); tgt as
        for score_translations."""
        return align.align_models(self.models, self.multimodal, src_var, src_lengths, tgt, im_var)

    def sample_decode(self, src_var, src_lengths, im_var=None, n_samples=1, max_length=80, temperature=1.0, top_k=0,
                      generator=None, top_p=1.0, return_sizes=False):
        """The models' sample_decode on the ensemble's scores (vagnmt_hip.sampling): Sampled(hyps, token_logp, logp, score), or
        (Sampled, sizes) with return_sizes.  top_p: nucleus sampling as on a model (1.0 without sizes: the plain decode).
        generator=None: the ensemble's own generator, seeded from torch.initial_seed()."""
        return sampling.sample_decode(self, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, generator,
                                      top_p, return_sizes)

    def beamsearch_diverse(self, src_var, src_lengths, im_var=None, beam_size=12, n_groups=3, diversity=0.5, n_best=None,
                           max_length=80, avoid_double=True, avoid_unk=False):
        """The models' beamsearch_diverse on the ensemble's scores (vagnmt_hip.diverse): Diverse(hyps, scores (B, n_best),
        group (B, n_best)), n_best None: all beam_size."""
        return diverse.beamsearch_diverse(self, src_var, src_lengths, im_var, beam_size, n_groups, diversity, n_best, max_length,
                                          avoid_double, avoid_unk)

    def beamsearch_stochastic(self, src_var, src_lengths, im_var=None, n_samples=12, max_length=80, generator=None,
                              avoid_double=False, avoid_unk=False):
        """The models' beamsearch_stochastic on the ensemble's scores (vagnmt_hip.stochastic): Stochastic(hyps, logp, score,
        gumbel, log_weight), n_samples distinct translations drawn without replacement from the ensemble's sequence distribution.
        generator=None: the ensemble's own generator."""
        return stochastic.beamsearch_stochastic(self, src_var, src_lengths, im_var, n_samples, max_length, generator, avoid_double,
                                                avoid_unk)

    def beamsearch_penalised(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, length_norm="gnmt",
                             alpha=0.6, beta=0.2, word_bonus=0.0, stepwise=False, avoid_double=True, avoid_unk=False,
                             no_repeat_ngram=0):
        """The models' beamsearch_penalised on the ensemble's scores (vagnmt_hip.penalty): Penalised(hyps, scores, logp, length,
        coverage_penalty).  The coverage is that of the members' mean attention rows, as in beamsearch_align."""
        return penalty.beamsearch_penalised(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, length_norm, alpha,
                                            beta, word_bonus, stepwise, avoid_double, avoid_unk, no_repeat_ngram)

    def beamsearch_constrained(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, prefix=None,
                               banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False):
        """The models' beamsearch_constrained on the ensemble's scores (vagnmt_hip.constrain): Constrained(hyps, scores
        (B, n_best)).  A ban writes -1e5 into every member's row, so the ensemble sees it as a single model does."""
        return constrain.beamsearch_constrained(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, prefix, banned,
                                                banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk)

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

    def beamsearch_required(self, src_var, src_lengths, im_var=None, beam_size=12, n_best=1, max_length=80, required=None,
                            prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True,
                            avoid_unk=False):
        """The models' beamsearch_required on the ensemble's scores (vagnmt_hip.require): Required(hyps, scores (B, n_best), met
        (B, n_best), complete (B, n_best)).  The phrase state follows the common hypotheses, so it is the single model's."""
        return require.beamsearch_required(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, required, prefix,
                                           banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk)

    def mbr_decode(self, src_var, src_lengths, im_var=None, n_samples=16, max_length=80, temperature=1.0, top_k=0, top_p=1.0,
                   beam_size=0, utility="bleu", generator=None, beam_groups=1, beam_diversity=0.5, without_replacement=False,
                   surface=None):
        """The models' mbr_decode on the ensemble's scores (vagnmt_hip.mbr): the draws of one sample_decode, then the candidate
        of highest expected utility against them; beam_size > 0 adds the ensemble's beam_size-best list to the candidates
        (beam_groups > 1: the list of beamsearch_diverse).  Returns (best, Selected, Sampled).  without_replacement=True: the
        draws of one beamsearch_stochastic, weighted by exp(log_weight); the third result is then the Stochastic."""
        return mbr.mbr_decode(self, src_var, src_lengths, im_var, n_samples, max_length, temperature, top_k, top_p, beam_size,
                              utility, generator, beam_groups, beam_diversity, without_replacement, surface)

    def _check_im(self, im_var):
        if im_var is None and any(self.multimodal):
            raise ValueError("Ensemble: a multimodal member needs im_var")

    def _beam(self, pro, k, max_length, flags=0, n_best=0, aligning=False, device_rows=False):
        mem, hs, e = self._members(pro, k, max_length, "ens_beam", flags, aligning)
        res, self.last_beam_scores, self.last_decode_steps = search.beam(mem, hs, k, max_length, flags, n_best, e, self._pool,
                                                                         align=aligning, device_rows=device_rows)
        return res

    # ------------------------------------------------------------------------------------------ the variants' seam
    def _search_setup(self, src_var, src_lengths, im_var, k, max_length, kind, flags=0, align=False, hoist=True, extra=(),
                      what=None):
        """A model's _search_setup on the ensemble: the im_var check (always made, under the ensemble's own message), every
        member's inference prologue, and the members and the entry of a search of kind "ens_" + kind -> search.Setup."""
        self._check_im(im_var)
        pro = [m._decode_prologue(src_var, src_lengths, im_var) for m in self.models]
        mem, hs, e = self._members(pro, k, max_length, "ens_" + kind, flags, align, hoist, extra)
        return search.Setup(mem, hs, e, self._pool, pro[0][0].shape[0], pro[0][0].device, False)

    def _search_done(self, out, beam_size=None):
        """A model's _search_done (an ensemble keeps no beam_size)."""
        res, self.last_beam_scores, self.last_decode_steps = out
        return res

    # ------------------------------------------------------------------------------------------ cache
    def _members(self, pro, k, max_length, kind, flags=0, aligning=False, hoist=True, extra=()):
        """(members, initial hidden states, entry) of one search.  In graph mode each member runs on its model's own static
        buffers of this shape under kind ("ens_greedy" / "ens_beam": a member's own decode graphs stay untouched), and the
        entry holds the ensemble's search buffers and captured graph.  Its key holds the members' state dicts by identity and
        the entry holds the dicts themselves: a member that rebuilds its state makes a new entry, and the buffers a captured
        graph reads stay alive as long as the graph.  flags are a by-value argument of the captured expansions: part of the key.
        aligning, hoist, extra: as a model's _decode_state takes them; the tail of the members' keys is the tail of the
        entry's."""
        graphed = self.decode_graph and pro[0][0].is_cuda
        mem = [search.Member(m, enc, mask, k, max_length, kind if graphed else None, hoist=hoist, align=aligning, extra=extra)
               for m, (enc, mask, _) in zip(self.models, pro)]
        hs = [h0 for (_, _, h0) in pro]
        if not graphed:
            return mem, hs, None
        key = (kind, pro[0][0].shape[0], k, max_length, flags) + search.key_tail(aligning, extra) + tuple(id(mb.st) for mb in mem)
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
