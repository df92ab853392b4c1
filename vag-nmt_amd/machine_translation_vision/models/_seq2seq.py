"""Shared machinery of the two model classes on the hot path (text-only V2 and multimodal V11).  Decoding runs the search of
vagnmt_hip.search on this model as its one member; the static buffers and captured graphs of each decode shape live here."""
import random

import torch
import torch.nn as nn

from vagnmt_hip import _lib, knn, ops, scoring, search
from vagnmt_hip import lm as lm_mod
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.fused import mt_label_smoothing
from vagnmt_hip.search import SOS_token, EOS_token, UNK_token  # noqa: F401  (the drop-in modules' names)
from vagnmt_hip.state import dropout_rng


class Seq2SeqBase(nn.Module):
    """encoder -> [visual grounding] -> decoder init -> cGRU decoder over the target -> loss / decode."""

    def __getstate__(self):
        """Whole-module pickles (``torch.save(model)``, nmt_multimodal_beam_DE.py:491-520, right after an evaluation pass) carry the
        module, not what decoding cached on it: static buffers, per-weights tables and captured HIP graphs of the decode shapes
        (``_decode_cache`` / ``_decode_wcache``: a CUDAGraph does not pickle) are rebuilt on the next decode call."""
        state = dict(self.__dict__)
        for k in [k for k in state if k.startswith("_decode_")]:
            del state[k]
        return state

    def reset_parameters(self):
        # models/...V11.py:77-80: every >=2-D non-bias parameter (embeddings included) gets kaiming_normal_
        for name, param in self.named_parameters():
            if param.requires_grad and 'bias' not in name and param.data.dim() > 1:
                nn.init.kaiming_normal_(param.data)

    # ------------------------------------------------------------------------------------------ training
    def _train_rng(self, device):
        """Advance the dropout counter once per training forward; backward re-derives the same masks."""
        if not self.training:
            return None
        if max(self.encoder.dropout_emb, self.encoder.dropout_ctx, self.decoder.dropout_out) <= 0:
            return None
        rng = dropout_rng(self, device)
        call("vag_rng_advance", ptr(rng, torch.int64), stream())
        return rng

    def _encode(self, src_var, src_lengths, rng):
        enc_mod = self.encoder
        g = enc_mod.gru
        train = self.training and rng is not None
        from vagnmt_hip.state import lengths_tensor
        return ops.BiGRUEncode.apply(
            src_var, lengths_tensor(src_lengths, src_var.device), enc_mod.embedding.weight,
            g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0,
            g.weight_ih_l0_reverse, g.weight_hh_l0_reverse, g.bias_ih_l0_reverse, g.bias_hh_l0_reverse,
            float(enc_mod.dropout_emb) if train else 0.0, float(enc_mod.dropout_ctx) if train else 0.0, rng)

    def _translation_loss(self, enc, mask, h0, tgt_var, teacher_force_ratio, criterion, rng):
        """The decoder loop of models/...V11.py:136-164 as two fused operators.
        teacher forcing (python ``random`` coin, V11.py:136): whole-sequence cGRU + batched head/CE;
        free running: the sequence operator also runs the head per step and feeds back the argmax."""
        dec = self.decoder
        B, Tt = tgt_var.shape
        V = dec.out.bias.shape[0]
        ldl = (V + 3) // 4 * 4
        pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
        is_teacher = random.random() < teacher_force_ratio
        sos = torch.full((1, B), SOS_token, dtype=torch.int64, device=tgt_var.device)
        tok = torch.cat([sos, tgt_var.t()], 0).contiguous()          # (Tt+1,B): inputs of steps 0..Tt-1 (+1 unused row)
        p_out = float(dec.dropout_out) if (self.training and rng is not None) else 0.0
        head = dec.head_params()
        eps = mt_label_smoothing(criterion)       # None: a criterion the head's loss kernels do not implement
        if is_teacher:
            h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
            tmid = logits = None
        else:
            h2, c, e, tmid, logits = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(),
                                                         free_run=True, head=head, p_out=p_out, rng=rng, V=V, ldl=ldl)
        if eps == 0.0:
            return ops.HeadCE.apply(h2, c, e, tgt_var, criterion.weight, p_out, rng, tmid, logits, ldl, *head)
        if eps is not None:
            return ops.HeadCESmoothed.apply(h2, c, e, tgt_var, criterion.weight, p_out, rng, tmid, logits, ldl, eps, *head)
        # any other criterion: materialise the log-probabilities and call it per step, as the reference does
        H = h2.shape[2]
        logp = ops.HeadLogp.apply(h2.view(Tt * B, H), c.view(Tt * B, 2 * H), e.view(Tt * B, -1), p_out, rng, *head)
        logp = logp.view(Tt, B, V)
        loss = 0
        for di in range(Tt):
            loss = loss + criterion(logp[di], tgt_var[:, di])
        tgt_mask = (tgt_var != 0).float()
        return (loss / tgt_mask.sum(-1)).mean()

    # ------------------------------------------------------------------------------------------ decoding
    # Both decoders replay ONE captured HIP graph of search.DECODE_CHUNK steps per (batch, beam, padded source length);
    # ``model.decode_graph = False`` runs the same kernels launch by launch (vagnmt_hip.search).
    decode_graph = True
    decode_persistent = True      # greedy decoding in one launch where the shape allows it (ops.greedy_decode)
    decode_raw_logits = True      # beam search: expansion on raw logits + log-sum-exp pieces (no normalising pass) where available
    decode_hoisted = True         # decoding steps on keys projected once per call (4 launches, no context): ops.decode_step_h

    def _decode_pool(self):
        """One graph memory pool for every decode shape this model captures (their per-step outputs are allocated inside the captures):
        bounded by the largest shapes met, not by the number of shapes.  The handle lives IN the decode cache: a pool
        dies with the last graph that used it, and the cache is where those graphs live -- dropped or cleared together."""
        cache = self.__dict__.setdefault("_decode_cache", {})
        pool = cache.get("__pool__")
        if pool is None:
            pool = cache["__pool__"] = torch.cuda.graph_pool_handle()
        return pool

    def _decode_weights(self, dp, hp, emb, hoisted):
        """What decoding derives from the WEIGHTS alone -- the stacked / folded decoder matrices (ops.decode_prepare) and, for
        the hoisted step, the per-token tables (ops.decode_tables) -- shared by every decode shape and kept until the weights
        change: an optimiser step of the step driver bumps ``_vag_weights_version``, anything else that writes a parameter in
        place bumps the tensor's own version counter, a re-assigned parameter has another address.  Refreshed in place, so the
        captured graphs that read these buffers stay valid."""
        ts = list(dp) + list(hp) + [emb]
        ptrs = tuple(t.data_ptr() for t in ts) + (hoisted,)
        ver = (getattr(self, "_vag_weights_version", 0),) + tuple(int(t._version) for t in ts)
        wc = self.__dict__.setdefault("_decode_wcache", {})
        e = wc.get(ptrs)
        if e is None:
            if len(wc) >= 4:
                wc.clear()
                self.__dict__.pop("_decode_cache", None)          # (their graphs point at the buffers just dropped)
            H = dp[1].shape[1]
            e = {"prep": torch.empty(_lib.lib().vag_cgru_prep_floats(H), device=emb.device), "tables": None, "ver": None}
            wc[ptrs] = e
        if e["ver"] != ver:
            e["prep"].copy_(ops.decode_prepare(emb, dp))
            if hoisted:
                if e["ver"] is None:
                    e["tables"] = ops.decode_tables(emb, dp, hp)
                elif e["tables"] is not None:
                    ops.decode_tables(emb, dp, hp, out=e["tables"])
            e["ver"] = ver
        return e

    def _decode_state(self, kind, enc, mask, k, max_length, flags=0, align=False, hoist=True, extra=()):
        """Static buffers (+ captured graph and search buffers, filled in by vagnmt_hip.search) for one decode shape; refreshed
        per call.  flags (the beam search's options) are a by-value argument of the captured expansion launches, so they are
        part of the key.  align: an aligning search captures another graph (one more launch per step) and keeps the steps'
        attention rows in ``alpha`` (B k, Tp); it has entries of its own, a plain search's entry is what it was.  hoist: whether
        the steps may be the hoisted ones.  extra: the variant's part of the key (search.key_tail's fragments): a variant has
        entries of its own, which also own its static buffers."""
        dec = self.decoder
        B, Ts, C = enc.shape
        H = C // 2
        dev = enc.device
        dp, hp, emb = dec.dec_params(), dec.head_params(), dec.embedding.weight
        Tp = (Ts + 7) // 8 * 8
        hoisted = hoist and self.decode_hoisted and ops.decode_hoisted_ok(B * k, emb, dp, hp)
        wd = self._decode_weights(dp, hp, emb, hoisted)
        key = (kind, B, k, Tp, max_length, self.decode_raw_logits, hoisted, flags) + search.key_tail(align, extra) + \
            tuple(t.data_ptr() for t in list(dp) + list(hp) + [emb, dec.attn.attn_e.weight])
        cache = self.__dict__.setdefault("_decode_cache", {})
        st = cache.get(key)
        if st is None:
            if len(cache) >= 64:
                cache.clear()
            st = {"enc": torch.zeros(B, Tp, C, device=dev), "pe": torch.zeros(B, Tp, C, device=dev),
                  "mask": torch.zeros(B, Tp, device=dev), "h": torch.empty(B * k, H, device=dev),
                  "prep": wd["prep"], "tables": wd["tables"], "graph": None, "hoisted": hoisted}
            if hoisted:
                st["keys"] = torch.empty(_lib.lib().vag_cgru_decode_keys_floats(B, Tp, emb.shape[1], H), device=dev)
            if align:
                st["alpha"] = torch.empty(B * k, Tp, device=dev)
            cache[key] = st
        if Ts < Tp:
            st["enc"][:, Ts:].zero_(); st["pe"][:, Ts:].zero_(); st["mask"][:, Ts:].zero_()
        st["enc"][:, :Ts].copy_(enc)
        st["pe"][:, :Ts].copy_(ops.KeysProj.apply(enc, dec.attn.attn_e.weight))
        st["mask"][:, :Ts].copy_(mask)
        if hoisted:
            ops.decode_keys(st["enc"], st["prep"], hp, out=st["keys"])
        return st, dp, hp, emb

    def _greedy(self, enc, mask, h, tgt_l, device_rows=False):
        """beam_size == 1 branch (V11.py:207-226): argmax for exactly tgt_l steps, cut at EOS on the host (device_rows: the
        (B, tgt_l) rows left on the device instead)."""
        dec = self.decoder
        self.last_decode_steps = tgt_l
        if self.decode_persistent and enc.is_cuda:
            dp, hp, emb = dec.dec_params(), dec.head_params(), dec.embedding.weight
            if ops.greedy_decode_supported(enc.shape[0], enc.shape[1], tgt_l, emb.shape[1], h.shape[1], hp[7].shape[0]):
                # every step in ONE launch: the recurrence kernel forms the logits and the arg-max itself (persist.hip)
                pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
                toks = ops.greedy_decode(enc, pe, mask, h, emb, dp, hp, tgt_l, SOS_token)
                return toks.t().contiguous() if device_rows else search.cut(toks.t().cpu().numpy())
        # the head's fused arg-max.  Eager greedy runs the plain (not hoisted) steps, graph greedy the steps _decode_state picks,
        # as it always did: hoist follows the mode
        graphed = self.decode_graph and enc.is_cuda
        mb = search.Member(self, enc, mask, 1, tgt_l, "greedy" if graphed else None, hoist=graphed)
        return search.greedy([mb], [h], tgt_l, mb.st, self._decode_pool, fused_argmax=True, device_rows=device_rows)

    def _beam(self, enc, mask, h, beam_size, max_length, flags=0, n_best=0, align=False, device_rows=False):
        """Batched beam search (V11.py:233-337): search.beam on this model alone, with the raw-logit expansion where
        decode_raw_logits allows it.  flags, n_best, align and device_rows as there; the decoder steps run go to last_decode_steps
        (bench.py prices one step)."""
        graphed = self.decode_graph and enc.is_cuda
        mb = search.Member(self, enc, mask, beam_size, max_length, "beam" if graphed else None, flags, align=align)
        res, self.last_beam_scores, self.last_decode_steps = search.beam(
            [mb], [h], beam_size, max_length, flags, n_best, mb.st, self._decode_pool, raw_logits=self.decode_raw_logits,
            align=align, device_rows=device_rows)
        return res

    def _validate_args(self, src_var, tgt_var, max_length):
        """(batch_size, tgt_l) as the reference computes them (models/...V11.py:170-177, NMT_Seq2Seq_Beam_V2.py:115-122)."""
        return src_var.size()[0], (max_length if tgt_var is None else tgt_var.size()[1])

    def beamsearch(self, encoder_outputs, context_mask, decoder_input, decoder_hidden, beam_size, max_length, avoid_double=True,
                   avoid_unk=False):
        """The reference's public entry to the batched beam search (models/...V11.py:233-337, NMT_Seq2Seq_Beam_V2.py:173-277), with
        ITS argument layout: encoder_outputs (Ts, B, 2H) time-major, context_mask (Ts, B), decoder_input (B, 1) = SOS,
        decoder_hidden (1, B, H).  Returns the list of token lists cut at EOS.  avoid_double=False lets a hypothesis repeat its
        previous word (:279-280); avoid_unk=True gives UNK = 1 the -1e5 penalty from step 1 on (:283-284; V11.py never defines
        UNK_token, the text model's value is used for both).
        The options run on the reference's layout, decoder_input = the (B, 1) SOS tensor beamsearch_decode builds (:186-188).
        decoder_input=None is this port's shorthand for that tensor in the default search only, as it always was: the reference
        cannot run such a call (it feeds decoder_input to the decoder at step 0), and with an option it still raises
        NotImplementedError."""
        flags = scoring.beam_flags(avoid_double, avoid_unk)
        if decoder_input is None and flags:
            raise NotImplementedError("beamsearch: decoder_input=None stands for SOS in the default search only; pass the (B, 1) SOS "
                                      "tensor, as the reference's beamsearch_decode does, to use avoid_double=False / avoid_unk=True")
        if decoder_input is not None and not bool((decoder_input == SOS_token).all()):
            raise ValueError("beamsearch starts every hypothesis from SOS (models/...V11.py:186-188)")
        enc = encoder_outputs.transpose(0, 1).contiguous()
        mask = context_mask.transpose(0, 1).contiguous().to(enc.dtype)
        h = decoder_hidden.reshape(-1, decoder_hidden.shape[-1]).contiguous()
        with torch.no_grad():
            return self._beam(enc, mask, h, int(beam_size), int(max_length), flags)

    def _decode(self, src_var, src_lengths, im_var, beam_size, max_length, tgt_var, device_rows=False):
        """beamsearch_decode of both models (V11.py:170-337, V2.py:115-277): greedy for beam_size == 1, else the beam search.
        device_rows: the search's (B, tgt_l) int64 rows as a GPU tensor (a row's content is what precedes its first EOS) instead of
        the cut lists -- what vagnmt_hip.validate feeds to the metric kernels; final_sample is left alone then."""
        tgt_l = max_length
        if tgt_var is not None:
            tgt_l = tgt_var.size()[1]
        self.tgt_l = tgt_l
        self.beam_size = beam_size
        with torch.no_grad():
            enc, mask, h0 = self._decode_prologue(src_var, src_lengths, im_var)
            if device_rows:
                return self._greedy(enc, mask, h0, tgt_l, True) if beam_size == 1 else \
                    self._beam(enc, mask, h0, beam_size, tgt_l, device_rows=True)
            if beam_size == 1:
                self.final_sample = self._greedy(enc, mask, h0, tgt_l)
            else:
                self.final_sample = self._beam(enc, mask, h0, beam_size, tgt_l)
        return self.final_sample

    def _nbest(self, src_var, src_lengths, im_var, beam_size, n_best, max_length, avoid_double, avoid_unk):
        """beamsearch_nbest of both models.  beam_size == 1 runs the beam kernels, as the reference's beamsearch does, not the
        greedy branch."""
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk)
        self.beam_size = k
        with torch.no_grad():
            enc, mask, h0 = self._decode_prologue(src_var, src_lengths, im_var)
            return self._beam(enc, mask, h0, k, int(max_length), flags, n)

    # The decode variants (beamsearch_diverse, sample_decode, mbr_decode, ...) are written once, in their feature modules, as
    # functions of a model or an Ensemble; these two methods are all they ask of either.
    def _search_setup(self, src_var, src_lengths, im_var, k, max_length, kind, flags=0, align=False, hoist=True, extra=(),
                      what=None):
        """The im_var check (what: the caller's name in its message; None: no check), the inference prologue, and this model as
        the one member of a search of ``kind`` -> search.Setup.  Graph mode: the entry is the member's decode state.  flags,
        align, hoist, extra as _decode_state takes them."""
        if what is not None and im_var is None and hasattr(self, "vse_imagine"):
            raise ValueError("%s: a multimodal model needs im_var" % what)
        enc, mask, h0 = self._decode_prologue(src_var, src_lengths, im_var)
        graphed = self.decode_graph and enc.is_cuda
        mb = search.Member(self, enc, mask, k, max_length, kind if graphed else None, flags, hoist, align, extra)
        return search.Setup([mb], [h0], mb.st, self._decode_pool, enc.shape[0], enc.device, self.decode_raw_logits)

    def _search_done(self, out, beam_size=None):
        """(result, best scores (B,), decoder steps run) of a beam search -> result; the other two go to last_beam_scores and
        last_decode_steps, beam_size (where given) to beam_size."""
        if beam_size is not None:
            self.beam_size = beam_size
        res, self.last_beam_scores, self.last_decode_steps = out
        return res

    def beamsearch_knn(self, src_var, src_lengths, im_var=None, datastore=None, beam_size=12, n_best=1, max_length=80, k=8,
                       temperature=10.0, lam=0.5, return_neighbours=False, avoid_double=True, avoid_unk=False, prefix=None,
                       banned=None, banned_per_sentence=None, no_repeat_ngram=0):
        """Beam search with a nearest-neighbour datastore mixed into every step's distribution (vagnmt_hip.knn; kNN-MT):
        KnnSearch(hyps, scores[, neighbours]) as beamsearch_nbest returns them, under log((1 - lam) p_model + lam p_knn) with
        p_knn the softmax(score / temperature) of the k nearest entries of ``datastore`` (knn.Datastore.build) summed per word.
        lam = 0 is beamsearch_nbest bit for bit.  prefix / banned / banned_per_sentence / no_repeat_ngram are
        beamsearch_constrained's and still win over a neighbour.  A text-only model ignores im_var.  Inference only."""
        return knn.beamsearch_knn(self, src_var, src_lengths, im_var if hasattr(self, "vse_imagine") else None, datastore, beam_size,
                                  n_best, max_length, k, temperature, lam, return_neighbours, avoid_double, avoid_unk, prefix, banned,
                                  banned_per_sentence, no_repeat_ngram)

    def knn_score_translations(self, src_var, src_lengths, tgt, im_var=None, datastore=None, k=8, temperature=10.0, lam=0.5):
        """score_translations under the distribution of beamsearch_knn (vagnmt_hip.knn.knn_score_translations)."""
        return knn.knn_score_translations(self, src_var, src_lengths, tgt, im_var if hasattr(self, "vse_imagine") else None,
                                          datastore, k, temperature, lam)

    def beamsearch_lm(self, src_var, src_lengths, im_var=None, lm=None, beta=0.3, beam_size=12, n_best=1, max_length=80,
                      avoid_double=True, avoid_unk=False, prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0):
        """Beam search under shallow fusion with a back-off n-gram language model (vagnmt_hip.lm): LmSearch(hyps, scores) as
        beamsearch_nbest returns them, under logp_model + beta ln p_LM(w | the last order-1 words), not renormalised.
        ``lm``: a vagnmt_hip.lm.NgramLM.  beta = 0 is beamsearch_nbest bit for bit.  prefix / banned /
        banned_per_sentence / no_repeat_ngram are beamsearch_constrained's and still win.  A text-only model ignores im_var."""
        return lm_mod.beamsearch_lm(self, src_var, src_lengths, im_var if hasattr(self, "vse_imagine") else None, lm, beta,
                                beam_size, n_best, max_length, avoid_double, avoid_unk, prefix, banned, banned_per_sentence,
                                no_repeat_ngram)

    def lm_score_translations(self, src_var, src_lengths, tgt, im_var=None, lm=None, beta=0.3):
        """score_translations under the fused score of beamsearch_lm (vagnmt_hip.lm.lm_score_translations)."""
        return lm_mod.lm_score_translations(self, src_var, src_lengths, tgt, im_var if hasattr(self, "vse_imagine") else None,
                                        lm, beta)

    _cut = staticmethod(search.cut)          # the EOS cut (vagnmt_hip.search.cut) under its earlier name
