"""Ensemble decoding: M trained models that share the source and target vocabularies decode ONE search together.

At every step each member runs its own decoder step and head on the common hypotheses, and the search scores word w of
hypothesis n by the mean of the members' probabilities (include/vag_nmt.h, vag_beam_ens_step):

    s[n, w] = mx + log( (sum_m exp(x_m[n, w] - mx)) / M ),   mx = max_m x_m[n, w],   x_m = member m's log_softmax row

The search rules are the single model's (models/...V11.py:207-226 greedy, :233-337 beam) applied to s.  Every member keeps its
own encoder, image path and decoder state; the chosen words feed all M decoders and the back-pointers re-order all M hidden
states.  Members may differ in hidden / embedding size, tied_emb, attn_model and multimodal vs text-only (text-only members
ignore ``im_var``).

    ens = Ensemble([best_model, best_loss_model, best_meteor_model])
    hyps = ens.beamsearch_decode(src_var, src_lengths, im_var, beam_size=12, max_length=80)
    nbest, scores = ens.beamsearch_nbest(src_var, src_lengths, im_var, beam_size=12, n_best=5)
    forced = ens.score_translations(src_var, src_lengths, tgt, im_var)       # Scores(score, logp, token_logp)
"""
import ctypes as C

import torch

from vagnmt_hip import _lib, ops, scoring
from vagnmt_hip._lib import call, ptr, stream

SOS_token = 2
EOS_token = 3

MAX_MODELS = 8          # VAG_ENS_MAX (include/vag_nmt.h): the kernels are instantiated for M = 1 .. 8


def _p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _pp(tensors):
    return (C.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


class _Member:
    """What one member contributes to a search: its static decode buffers and weights (the model's own _decode_state /
    _decode_weights in graph mode, fresh tensors in eager mode) and its step: decoder step + head -> (h2, logp)."""

    def __init__(self, model, enc, mask, k, max_length, kind, graphed):
        dec = model.decoder
        self.H = enc.shape[2] // 2
        if graphed:
            st, self.dp, self.hp, self.emb = model._decode_state(kind, enc, mask, k, max_length)
            self.st = st
            self.enc, self.pe, self.mask, self.prep = st["enc"], st["pe"], st["mask"], st["prep"]
            self.hoisted, self.keys, self.tables = st["hoisted"], st.get("keys"), st.get("tables")
        else:
            self.st = None
            self.dp, self.hp, self.emb = dec.dec_params(), dec.head_params(), dec.embedding.weight
            self.enc, self.mask = enc, mask
            self.pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
            self.prep = ops.decode_prepare(self.emb, self.dp)
            self.hoisted = model.decode_hoisted and ops.decode_hoisted_ok(enc.shape[0] * k, self.emb, self.dp, self.hp)
            self.keys = ops.decode_keys(enc, self.prep, self.hp) if self.hoisted else None
            self.tables = ops.decode_tables(self.emb, self.dp, self.hp) if self.hoisted else None

    def step(self, tok, h, rows_per_src):
        if self.hoisted:
            h2, c, e, _ = ops.decode_step_h(self.pe, self.mask, self.keys, rows_per_src, tok, h, self.emb, self.dp, self.prep,
                                            tables=self.tables)
        else:
            h2, c, e, _ = ops.decode_step(self.enc, self.pe, self.mask, rows_per_src, tok, h, self.emb, self.dp, self.prep)
        logp, _ = ops.head_logp_step(h2, c, e, self.hp, hoisted=self.hoisted, tables=self.tables if self.hoisted else None,
                                     tok=tok)
        return h2, logp


class Ensemble:
    """A plain object over M models (not an nn.Module: it owns no parameters).  ``beamsearch_decode`` has the models'
    signature and return value; after a beam search ``last_beam_scores`` (B,) and ``last_decode_steps`` are set as on a
    model.  ``decode_graph = False`` runs the same kernels launch by launch instead of replaying captured graphs."""

    DECODE_CHUNK = 8
    decode_graph = True

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("Ensemble: no models")
        if len(models) > MAX_MODELS:
            raise ValueError("Ensemble: %d models, at most %d" % (len(models), MAX_MODELS))
        for m in models:
            if not (hasattr(m, "_prologue") and hasattr(m, "_decode_state") and hasattr(m, "decoder")):
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
        if im_var is None and any(self.multimodal):
            raise ValueError("Ensemble: a multimodal member needs im_var")
        tgt_l = max_length if tgt_var is None else tgt_var.size()[1]
        with torch.no_grad():
            pro = self._prologues(src_var, src_lengths, im_var)
            if beam_size == 1:
                return self._greedy(pro, tgt_l)
            return self._beam(pro, int(beam_size), int(tgt_l))

    def _prologues(self, src_var, src_lengths, im_var):
        pro = []
        for m, mm in zip(self.models, self.multimodal):
            if mm:
                enc, mask, _, h0 = m._prologue(src_var, src_lengths, im_var, None, None)
            else:
                enc, mask, h0 = m._prologue(src_var, src_lengths, None)
            pro.append((enc, mask, h0))
        return pro

    def beamsearch_nbest(self, src_var, src_lengths, im_var=None, beam_size=1, n_best=1, max_length=80, avoid_double=True,
                         avoid_unk=False):
        """The models' beamsearch_nbest on the ensemble's scores: (hyps, scores), hyps[b] a list of n_best token lists cut at
        EOS, scores (B, n_best) float32 on the device, descending.  beam_size == 1 runs the beam kernels (not the greedy branch)."""
        k, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk)
        if im_var is None and any(self.multimodal):
            raise ValueError("Ensemble: a multimodal member needs im_var")
        with torch.no_grad():
            return self._beam(self._prologues(src_var, src_lengths, im_var), k, int(max_length), flags, n)

    def score_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding under the ensemble's scores (members combined per word as in the search): Scores(score (B,),
        logp (B,), token_logp (B, Tt)); tgt as for a model's score_translations."""
        return scoring.score_models(self.models, self.multimodal, src_var, src_lengths, tgt, im_var)

    # ------------------------------------------------------------------------------------------ cache
    def _pool(self):
        pool = self._cache.get("__pool__")
        if pool is None:
            pool = self._cache["__pool__"] = torch.cuda.graph_pool_handle()
        return pool

    def _entry(self, key):
        """The search buffers and captured graph of one decode shape.  The key holds the members' state dicts by identity and
        the entry holds the dicts themselves: a member that rebuilds its state makes a new entry, and the buffers a captured
        graph reads stay alive as long as the graph."""
        e = self._cache.get(key)
        if e is None:
            if len(self._cache) >= 32:
                self._cache.clear()
            e = self._cache[key] = {"graph": None}
        return e

    # ------------------------------------------------------------------------------------------ greedy
    def _argmax(self, logps, out):
        N = out.numel()
        V = self.models[0].tgt_size
        call("vag_ens_argmax", _pp(logps), _p64([lp.shape[1] for lp in logps]), len(logps), N, V, ptr(out, torch.int64),
             stream())

    def _greedy(self, pro, tgt_l):
        """beam_size == 1 (V11.py:207-226 on the ensemble's scores): arg-max for exactly tgt_l steps, cut at EOS."""
        enc0 = pro[0][0]
        B, dev = enc0.shape[0], enc0.device
        graphed = self.decode_graph and enc0.is_cuda
        toks = torch.empty(tgt_l, B, dtype=torch.int64, device=dev)
        self.last_decode_steps = tgt_l
        mem = [_Member(m, enc, mask, 1, tgt_l, "ens_greedy", graphed) for m, (enc, mask, _) in zip(self.models, pro)]
        if not graphed:
            tok = torch.full((B,), SOS_token, dtype=torch.int64, device=dev)
            hs = [h0 for (_, _, h0) in pro]
            for di in range(tgt_l):
                outs = [mb.step(tok, h, 1) for mb, h in zip(mem, hs)]
                hs = [o[0] for o in outs]
                self._argmax([o[1] for o in outs], toks[di])
                tok = toks[di]
            return _cut(toks.t().cpu().numpy())
        CH = self.DECODE_CHUNK
        e = self._entry(("greedy", B, tgt_l) + tuple(id(mb.st) for mb in mem))
        e["members"] = [mb.st for mb in mem]
        for mb, (_, _, h0) in zip(mem, pro):
            mb.st["h"].copy_(h0)
        if e["graph"] is None:
            e["tok"] = torch.empty(B, dtype=torch.int64, device=dev)           # one token buffer for every member
            e["chunk"] = torch.empty(CH, B, dtype=torch.int64, device=dev)
        e["tok"].fill_(SOS_token)
        if e["graph"] is None:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _lib.capture(g, pool=self._pool()):
                hs, tc = [mb.st["h"] for mb in mem], e["tok"]
                for i in range(CH):
                    outs = [mb.step(tc, h, 1) for mb, h in zip(mem, hs)]
                    hs = [o[0] for o in outs]
                    self._argmax([o[1] for o in outs], e["chunk"][i])
                    tc = e["chunk"][i]
                for mb, h in zip(mem, hs):
                    mb.st["h"].copy_(h)
                e["tok"].copy_(tc)
            e["graph"] = g
        for d0 in range(0, tgt_l, CH):
            e["graph"].replay()
            n = min(CH, tgt_l - d0)
            toks[d0:d0 + n].copy_(e["chunk"][:n])
        return _cut(toks.t().cpu().numpy())

    # ------------------------------------------------------------------------------------------ beam
    def _beam(self, pro, beam_size, max_length, flags=0, n_best=0):
        """Batched beam search (V11.py:233-337) over the ensemble's scores; flags and n_best as in the models' _beam."""
        enc0 = pro[0][0]
        B, k, dev = enc0.shape[0], beam_size, enc0.device
        V = self.models[0].tgt_size
        M = len(self.models)
        graphed = self.decode_graph and enc0.is_cuda
        mem = [_Member(m, enc, mask, k, max_length, "ens_beam", graphed) for m, (enc, mask, _) in zip(self.models, pro)]
        Hs = _p64([mb.H for mb in mem])
        # flags are a by-value argument of the captured expansions: part of the key
        e = self._entry(("beam", B, k, max_length, flags) + tuple(id(mb.st) for mb in mem)) if graphed else {}
        if "flat" in e:
            e["flat"].zero_()
        else:
            # history (words | back-pointers), running scores, alive counter and device-side step index in ONE buffer, laid
            # out as the single model's (models/_seq2seq.py, _beam)
            nb = 2 * max_length * B * k
            flat = torch.zeros(nb + (B * k + 8 + 1) // 2, dtype=torch.int64, device=dev)
            tail = flat[nb:].view(torch.int32)
            e.update(flat=flat, beam=flat[:nb].view(2 * max_length, B, k), nll=tail[:B * k].view(torch.float32).view(B, k),
                     n_alive=tail[B * k:B * k + 1], di=tail[B * k + 2:B * k + 4],
                     scratch=torch.empty(_lib.lib().vag_beam_scratch_bytes(B, k, V, max_length), dtype=torch.uint8, device=dev),
                     one=torch.ones(1, dtype=torch.int32, device=dev))
            if graphed:
                e["members"] = [mb.st for mb in mem]
                e["tok"] = torch.empty(B * k, dtype=torch.int64, device=dev)     # one token buffer for every member
        beam, nll, n_alive, scratch = e["beam"], e["nll"], e["n_alive"], e["scratch"]
        tok = torch.full((B,), SOS_token, dtype=torch.int64, device=dev)
        hs = [h0 for (_, _, h0) in pro]
        steps = 0
        for di in range(max_length):
            rps = 1 if di == 0 else k
            outs = [mb.step(tok, h, rps) for mb, h in zip(mem, hs)]
            h_next = [mb.st["h"] for mb in mem] if graphed else [torch.empty(B * k, mb.H, device=dev) for mb in mem]
            call("vag_beam_ens_step_opt", _pp([o[1] for o in outs]), _p64([o[1].shape[1] for o in outs]), M, ptr(nll),
                 ptr(beam, torch.int64), di, max_length, _pp([o[0] for o in outs]), _pp(h_next), Hs, B, k, V,
                 ptr(n_alive, torch.int32), scratch.data_ptr(), flags, stream())
            steps = di + 1
            if graphed:
                break                                  # step 0 only (one hypothesis per sentence); the rest is replayed
            hs = h_next
            tok = beam[di].view(-1)
            if di % 8 == 7 and int(n_alive.item()) == 0:          # V11.py:266-269, polled now and then
                break
        if graphed and max_length > 1:
            CH = self.DECODE_CHUNK
            e["tok"].copy_(beam[0].view(-1))
            e["di"][0:1].copy_(e["one"])                # the replayed steps start at step 1
            if e["graph"] is None:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with _lib.capture(g, pool=self._pool()):
                    for _ in range(CH):
                        outs = [mb.step(e["tok"], mb.st["h"], k) for mb in mem]
                        call("vag_beam_ens_step_dev_opt", _pp([o[1] for o in outs]), _p64([o[1].shape[1] for o in outs]), M,
                             ptr(nll), ptr(beam, torch.int64), ptr(e["di"], torch.int32), max_length,
                             _pp([o[0] for o in outs]), _pp([mb.st["h"] for mb in mem]), Hs, ptr(e["tok"], torch.int64),
                             B, k, V, ptr(n_alive, torch.int32), scratch.data_ptr(), flags, stream())
                e["graph"] = g
            while steps < max_length:
                e["graph"].replay()
                steps = min(steps + CH, max_length)
                if int(n_alive.item()) == 0:           # V11.py:266-269, polled once per chunk
                    break
        if n_best:
            out = torch.empty(B, n_best, max_length, dtype=torch.int64, device=dev)
            scores = torch.empty(B, n_best, dtype=torch.float32, device=dev)
            call("vag_beam_finish_nbest", ptr(nll), ptr(beam, torch.int64), max_length, steps, B, k, n_best,
                 ptr(out, torch.int64), ptr(scores), stream())
            self.last_beam_scores = scores[:, 0]
            self.last_decode_steps = steps
            return scoring.cut_nbest(out.cpu().numpy(), n_best), scores
        out = torch.empty(B, max_length, dtype=torch.int64, device=dev)
        best = torch.empty(B, dtype=torch.float32, device=dev)
        call("vag_beam_finish", ptr(nll), ptr(beam, torch.int64), max_length, steps, B, k, ptr(out, torch.int64), ptr(best),
             stream())
        self.last_beam_scores = best
        self.last_decode_steps = steps
        return _cut(out.cpu().numpy())


def _cut(hyps):
    final = []
    for row in hyps:
        cur = []
        for t in row:
            if t == EOS_token:
                break
            cur.append(t)
        final.append(cur)
    return final
