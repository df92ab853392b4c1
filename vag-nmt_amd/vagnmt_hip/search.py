"""The decoders' search on the host: greedy (V11.py:207-226), batched beam search (V11.py:233-337) and its variants, and sampling,
over a list of members -- one model (one member) or an ensemble (M members, vagnmt_hip.ensemble).

Every member runs its own decoder step and head on the common hypotheses.  With M > 1, or for an Ensemble at any M, the step's
log-probabilities go to the ensemble kernels (vag_ens_argmax, vag_beam_ens_step*), which combine them per word as
mx + log(sum_m exp(x_m - mx) / M).  A single model's greedy step can take the arg-max fused into the head (``fused_argmax``).

Every beam search is ONE driver (``_Search``) and a description of what differs.  The driver owns the search buffer (made once,
re-zeroed on an entry that has one), the eager loop with its poll of the alive counter every 8 steps, and graph mode: step 0
launch by launch, then ONE captured HIP graph of DECODE_CHUNK steps per decode shape, replayed until nothing is alive -- the
step index lives in device memory (the ``_dev`` entries), the source side is padded to a multiple of 8 positions with mask 0
(exactly zero attention weight, so results do not change), and the host looks at the device once per chunk.  It also forms the
argument prefix every expansion shares.  A search names its scratch-size query, adds its own buffers to the entry, may enqueue
launches between the members' steps and the expansion (``before``), names its expansion with its trailing arguments, and
finishes.  The searches:

``beam``: the plain expansion (vag_beam_ens_step(_dev)_opt; at M = 1 the kernels and arguments of vag_beam_step(_dev)_opt).  Its
captured steps can expand raw logits plus the pieces of their rows' log-sum-exp where the vocabulary product provides them
(``raw_logits``, one member: vag_beam_step_logits_dev_opt).  ``align=True`` (vagnmt_hip.align) keeps every step's attention
rows, averaged over the members (vag_beam_attn_record(_dev) before the expansion), and resolves them through the back-pointers
in its finish (vag_beam_finish_align).  ``constrain=c`` (vagnmt_hip.constrain) rules words out before every expansion
(vag_beam_constrain(_dev): forced prefix words, banned phrases, no-repeat n-grams).  The default search enqueues neither.
``beam_diverse`` (vagnmt_hip.diverse): the grouped expansion (vag_beam_div_step(_dev)); its finish also reports final slots.
``beam_required`` (vagnmt_hip.require): the allotting expansion (vag_beam_req_step(_dev)), which carries every hypothesis's
phrase state from step to step; the mask of a constrained search may precede it.
``beam_stochastic`` (vagnmt_hip.stochastic): the Gumbel-perturbed expansion (vag_beam_sbs_step(_dev)), which carries every slot's
perturbed score and reads the sampler's generator state: k samples without replacement, in sampling order.
``beam_penalised`` (vagnmt_hip.penalty): the carried coverage (vag_beam_cover(_dev)) and the optional mask before an expansion
that can select by the length- and coverage-penalised score (vag_beam_pen_step(_dev)); its finish ranks by that score
(vag_beam_finish_pen).
All but ``beam`` run the members' log-probability steps only and have entries of their own.

Sampling (``sample``, vagnmt_hip.sampling) runs the members' plain steps on B n rows and draws each row's word with ONE launch
(vag_sample_step: temperature, top-k, Gumbel-max; vag_sample_step_p with a nucleus cut); graph mode captures step 0 and a chunk of
later steps once per decode shape, under entries of their own."""
import ctypes as C
from collections import namedtuple

import torch

from vagnmt_hip import _lib, ops
from vagnmt_hip._lib import call, ptr, stream

SOS_token = 2
EOS_token = 3
UNK_token = 1

DECODE_CHUNK = 8

I32, I64 = torch.int32, torch.int64


def cut(hyps):
    """Token rows -> token lists, each cut before its first EOS."""
    final = []
    for row in hyps:
        cur = []
        for t in row:
            if t == EOS_token:
                break
            cur.append(t)
        final.append(cur)
    return final


def cut_nbest(out, n):
    """(B, n, max_len) token array -> hyps[b] = n token lists, each cut at EOS."""
    return [[[int(t) for t in row] for row in cut(sent[:n])] for sent in out]


def _p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _pp(tensors, dtype=torch.float32):
    """void*[] of the tensors' device pointers (None -> NULL), each checked as ``ptr`` checks it; dtype None: taken as they are."""
    if dtype is None:
        return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
    return (C.c_void_p * len(tensors))(*[ptr(t, dtype) for t in tensors])


def key_tail(align, *fragments):
    """What follows ``flags`` in the key of a decode state and of an ensemble's entry: ("align",) for an aligning search, then the
    variant's fragments in the order given.  A fragment is a tuple that starts with its variant's name and holds what the
    variant's captured launches take by value or by pointer -- built, and documented, where the variant is (() for none)."""
    return sum((tuple(f) for f in fragments), ("align",) if align else ())


# What a model's or an Ensemble's _search_setup hands to a search: the first four are the search functions' (members, h0s, entry,
# pool) -- entry None in eager mode; B and device are the batch's; raw_logits: whether ``beam`` may expand raw logits.
Setup = namedtuple("Setup", ["members", "h0s", "entry", "pool", "B", "device", "raw_logits"])


class Member:
    """What one model contributes to a search: its decode buffers and weights and its step.  kind given (graph mode): the
    model's static buffers of this decode shape (its _decode_state entry; ``h`` is the hidden state the captured steps carry).
    kind None (eager mode): fresh tensors.  hoist: whether the steps may be the hoisted ones (sampling runs the plain ones).
    align: the member keeps its last step's attention rows in ``alpha`` (graph mode: in the state's static rows, so that a
    captured record launch finds them).  extra: the variant's part of the state's key (key_tail's fragments)."""

    def __init__(self, model, enc, mask, k, max_length, kind=None, flags=0, hoist=True, align=False, extra=()):
        dec = model.decoder
        self.H = enc.shape[2] // 2
        self.V = dec.out.bias.shape[0]
        self.Ts = enc.shape[1]
        self.align, self.alpha, self.alpha_rows = align, None, None
        if kind is not None:
            st, self.dp, self.hp, self.emb = model._decode_state(kind, enc, mask, k, max_length, flags, align, hoist, extra)
            self.st, self.h = st, st["h"]
            self.alpha_rows = st.get("alpha")
            self.enc, self.pe, self.mask, self.prep = st["enc"], st["pe"], st["mask"], st["prep"]
            self.hoisted, self.keys, self.tables = st["hoisted"], st.get("keys"), st.get("tables")
        else:
            self.st = self.h = None
            self.dp, self.hp, self.emb = dec.dec_params(), dec.head_params(), dec.embedding.weight
            self.enc, self.mask = enc, mask
            self.pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
            self.prep = ops.decode_prepare(self.emb, self.dp)
            self.hoisted = hoist and model.decode_hoisted and ops.decode_hoisted_ok(enc.shape[0] * k, self.emb, self.dp, self.hp)
            self.keys = ops.decode_keys(enc, self.prep, self.hp) if self.hoisted else None
            self.tables = ops.decode_tables(self.emb, self.dp, self.hp) if self.hoisted else None

    def _decode(self, tok, h, rows_per_src):
        if self.hoisted:
            h2, c, e, a = ops.decode_step_h(self.pe, self.mask, self.keys, rows_per_src, tok, h, self.emb, self.dp, self.prep,
                                            tables=self.tables, alpha=self.alpha_rows)
        else:
            h2, c, e, a = ops.decode_step(self.enc, self.pe, self.mask, rows_per_src, tok, h, self.emb, self.dp, self.prep,
                                          alpha=self.alpha_rows)
        if self.align:
            self.alpha = a
        return h2, c, e

    def step(self, tok, h, rows_per_src):
        """Decoder step + head -> (h2, logp)."""
        h2, c, e = self._decode(tok, h, rows_per_src)
        logp, _ = ops.head_logp_step(h2, c, e, self.hp, hoisted=self.hoisted, tables=self.tables, tok=tok)
        return h2, logp

    def step_argmax(self, tok, h, out):
        """Greedy step with the arg-max fused into the head, written into out -> h2 (single model only)."""
        h2, c, e = self._decode(tok, h, 1)
        ops.head_logp_step(h2, c, e, self.hp, want_argmax=True, argmax_out=out, hoisted=self.hoisted, tables=self.tables, tok=tok)
        return h2

    def step_logits(self, tok, h, rows_per_src, nparts):
        """Decoder step + head's raw logits -> (h2, logits, parts) (single model only)."""
        h2, c, e = self._decode(tok, h, rows_per_src)
        logits, parts = ops.head_logits_step(h2, c, e, self.hp, nparts, hoisted=self.hoisted, tables=self.tables, tok=tok)
        return h2, logits, parts


def search_buffer(B, k, V, max_length, dev, scratch_bytes="vag_beam_scratch_bytes"):
    """The beam search's state in ONE zeroed buffer a captured graph can point into: history (words | back-pointers), running
    scores, the alive counter and the device-side step index -- one fill per call instead of a fresh tensor and a copy each.
    scratch_bytes: the size query of the expansion that will run on it."""
    nb = 2 * max_length * B * k
    flat = torch.zeros(nb + (B * k + 8 + 1) // 2, dtype=I64, device=dev)
    tail = flat[nb:].view(I32)
    return dict(flat=flat, beam=flat[:nb].view(2 * max_length, B, k), nll=tail[:B * k].view(torch.float32).view(B, k),
                n_alive=tail[B * k:B * k + 1], di=tail[B * k + 2:B * k + 4],
                scratch=torch.empty(getattr(_lib.lib(), scratch_bytes)(B, k, V, max_length), dtype=torch.uint8, device=dev),
                one=torch.ones(1, dtype=I32, device=dev))


def _capture(entry, pool, body, name="graph"):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.capture(g, pool=pool()):
        body()
    entry[name] = g


def greedy(members, h0s, tgt_l, entry=None, pool=None, fused_argmax=False, device_rows=False):
    """Arg-max for exactly tgt_l steps, cut at EOS.  entry (graph mode): the dict that keeps the captured graph and its token
    buffers; pool() its graph memory pool.  fused_argmax: the head's own arg-max (one member), else vag_ens_argmax.
    device_rows: the (B, tgt_l) int64 rows on the device instead of the cut lists (nothing is copied to the host)."""
    B, dev = h0s[0].shape[0], h0s[0].device
    toks = torch.empty(tgt_l, B, dtype=I64, device=dev)

    def pick(tok, hs, out):                    # one step of every member; the chosen words go to out
        if fused_argmax:
            return [members[0].step_argmax(tok, hs[0], out)]
        outs = [mb.step(tok, h, 1) for mb, h in zip(members, hs)]
        call("vag_ens_argmax", _pp([o[1] for o in outs]), _p64([o[1].shape[1] for o in outs]), len(outs), B, members[0].V,
             ptr(out, I64), stream())
        return [o[0] for o in outs]

    if entry is None:
        tok, hs = torch.full((B,), SOS_token, dtype=I64, device=dev), list(h0s)
        for di in range(tgt_l):
            hs, tok = pick(tok, hs, toks[di]), toks[di]
        return toks.t().contiguous() if device_rows else cut(toks.t().cpu().numpy())
    CH = DECODE_CHUNK
    for mb, h0 in zip(members, h0s):
        mb.h.copy_(h0)
    if entry["graph"] is None:
        entry["tok"] = torch.empty(B, dtype=I64, device=dev)                # one token buffer for every member
        entry["chunk"] = torch.empty(CH, B, dtype=I64, device=dev)
    entry["tok"].fill_(SOS_token)
    if entry["graph"] is None:
        def body():
            hs, tc = [mb.h for mb in members], entry["tok"]
            for i in range(CH):
                hs, tc = pick(tc, hs, entry["chunk"][i]), entry["chunk"][i]
            for mb, h in zip(members, hs):
                mb.h.copy_(h)
            entry["tok"].copy_(tc)
        _capture(entry, pool, body)
    for d0 in range(0, tgt_l, CH):
        entry["graph"].replay()
        n = min(CH, tgt_l - d0)
        toks[d0:d0 + n].copy_(entry["chunk"][:n])
    return toks.t().contiguous() if device_rows else cut(toks.t().cpu().numpy())


def constrain_rows(constrain, outs, beam, di, max_length, B, k, V, dev_form=False):
    """The mask of a constrained search on the rows the members just wrote (outs: their (h2, logp) pairs), to be enqueued before
    the expansion that reads them: every search but ``beam_diverse`` calls it from its ``before`` hook.  constrain: None (nothing is
    enqueued) or an object with ``args()`` = (prefix, Lp, phrases, phrase_sent, P, ngram) as vag_beam_constrain takes them
    (vagnmt_hip.constrain.Constraints).  di: the step, or with dev_form the device-side step index."""
    if constrain is None:
        return
    call("vag_beam_constrain_dev" if dev_form else "vag_beam_constrain", _pp([o[1] for o in outs]),
         _p64([o[1].shape[1] for o in outs]), len(outs), ptr(beam, I64), di, max_length, B, k, V, *constrain.args(), stream())


class _Search:
    """One expansion search from its buffers to its last step: what ``beam`` and its variants share.

    The constructor makes the search buffer (scratch sized by ``scratch_bytes``) and, in graph mode, the token buffer -- or
    re-zeroes the buffer of an entry that has one; ``fresh`` tells a variant to add its own buffers to ``e``.  ``run`` takes
      names   the expansion's entries, (host form, ``_dev`` form);
      tail    the expansion's arguments after the common prefix (the stream follows them);
      before  None or before(outs, di, dev_form): the launches between the members' steps (outs: their (h2, logp) pairs) and the
              expansion, with di the step or, dev_form, the device-side step index -- the expansion's stage 2 advances it;
      chunk_step  None or a function called once, when the chunk is captured, that returns None or the replacement of a
              captured step (``beam``'s raw-logits step)
    and returns the decoder steps run.  The common prefix: (logp**, ldl*, M, nll, beam, di, max_len, h_in**, h_out**, H*, B, k, V,
    n_alive, scratch), the ``_dev`` form with tok_out before B."""

    def __init__(self, members, h0s, k, max_length, entry, scratch_bytes="vag_beam_scratch_bytes"):
        self.members, self.h0s, self.k, self.max_length = members, h0s, k, max_length
        self.B, self.dev = h0s[0].shape[0], h0s[0].device
        self.V, self.M = members[0].V, len(members)
        self.graphed = entry is not None
        self.e = e = entry if self.graphed else {}
        self.fresh = "flat" not in e
        if self.fresh:
            e.update(search_buffer(self.B, k, self.V, max_length, self.dev, scratch_bytes))
            if self.graphed:
                e["tok"] = torch.empty(self.B * k, dtype=I64, device=self.dev)           # one token buffer for every member
        else:
            e["flat"].zero_()

    def run(self, pool, names, tail, before=None, chunk_step=None):
        e, members, k, max_length = self.e, self.members, self.k, self.max_length
        B, V, M, dev, graphed = self.B, self.V, self.M, self.dev, self.graphed
        beam, nll, n_alive, scratch = e["beam"], e["nll"], e["n_alive"], e["scratch"]
        Hs = _p64([mb.H for mb in members])

        def expand(outs, h_next, di, *tok_out):    # (the stream is read at every call: a capture runs on a stream of its own)
            if before is not None:
                before(outs, di, bool(tok_out))
            call(names[bool(tok_out)], _pp([o[1] for o in outs]), _p64([o[1].shape[1] for o in outs]), M, ptr(nll), ptr(beam, I64), di,
                 max_length, _pp([o[0] for o in outs]), _pp(h_next), Hs, *tok_out, B, k, V, ptr(n_alive, I32), scratch.data_ptr(),
                 *tail, stream())

        tok = torch.full((B,), SOS_token, dtype=I64, device=dev)
        hs = list(self.h0s)
        steps = 0
        for di in range(max_length):
            outs = [mb.step(tok, h, 1 if di == 0 else k) for mb, h in zip(members, hs)]
            h_next = [mb.h for mb in members] if graphed else [torch.empty(B * k, mb.H, device=dev) for mb in members]
            expand(outs, h_next, di)
            steps = di + 1
            if graphed:
                break                                  # step 0 only (one hypothesis per sentence); the rest is replayed
            hs = h_next
            tok = beam[di].view(-1)
            # the reference stops once every hypothesis has emitted EOS (V11.py:266-269); running on is harmless (finished
            # hypotheses only re-emit EOS at cost 0), so the device counter is polled only now and then.
            if di % 8 == 7 and int(n_alive.item()) == 0:
                break
        if graphed and max_length > 1:
            e["tok"].copy_(beam[0].view(-1))
            e["di"][0:1].copy_(e["one"])                # the replayed steps start at step 1 (device to device: no host wait)
            if e["graph"] is None:
                one = chunk_step() if chunk_step is not None else None

                def body():
                    for _ in range(DECODE_CHUNK):
                        if one is not None:
                            one()
                            continue
                        outs = [mb.step(e["tok"], mb.h, k) for mb in members]
                        expand(outs, [mb.h for mb in members], ptr(e["di"], I32), ptr(e["tok"], I64))
                _capture(e, pool, body)
            while steps < max_length:
                e["graph"].replay()
                steps = min(steps + DECODE_CHUNK, max_length)
                if int(n_alive.item()) == 0:           # V11.py:266-269, polled once per chunk
                    break
        return steps

    def finish_slots(self, n, steps):
        """vag_beam_finish_nbest_slots -> (out (B, n, max_length) int64, scores (B, n), slots (B, n) int64), best first."""
        B, k, max_length, dev = self.B, self.k, self.max_length, self.dev
        out = torch.empty(B, n, max_length, dtype=I64, device=dev)
        scores = torch.empty(B, n, dtype=torch.float32, device=dev)
        slots = torch.empty(B, n, dtype=I64, device=dev)
        call("vag_beam_finish_nbest_slots", ptr(self.e["nll"]), ptr(self.e["beam"], I64), max_length, steps, B, k, n, ptr(out, I64),
             ptr(scores), ptr(slots, I64), stream())
        return out, scores, slots


def beam(members, h0s, k, max_length, flags=0, n_best=0, entry=None, pool=None, raw_logits=False, align=False, constrain=None,
         device_rows=False, knn=None, lm=None):
    """Batched beam search.  flags: the reference's options (scoring.beam_flags; 0 = avoid_double=True, avoid_unk=False).
    entry / pool as in greedy; entry also keeps the search buffer.  raw_logits (one member): the captured steps expand raw logits
    where the head provides their log-sum-exp pieces.  Returns (result, best scores (B,), decoder steps run): result is the best
    token list per sentence (n_best = 0), or (hyps, scores) with hyps[b] the n_best best token lists and scores (B, n_best) on
    the device, best first (vag_beam_finish_nbest).  align (with n_best; members built with align=True): result is (hyps, scores,
    attention (B, n_best, max_length, Ts), src_pos (B, n_best, max_length)) of vag_beam_finish_align.
    constrain: the constraints of a constrained search (constrain_rows), applied at every step, step 0 included; needs
    raw_logits=False (masking raw logits after their log-sum-exp pieces were formed would not give -1e5) and, in graph mode, an
    entry of its own whose static buffers the object points at.
    device_rows (n_best = 0, no align): result is the finish's (B, max_length) int64 rows on the device instead of the cut lists --
    every row holds an EOS (the finish forces one into the last position), so a row's span is its cut list.
    knn: None, or an object whose ``rows(outs)`` mixes a datastore's nearest neighbours into the rows the members just wrote
    (vagnmt_hip.knn.StepMix: vag_knn_search per member, then vag_knn_mix), enqueued before the constraints' mask so that a ban
    still wins; needs raw_logits=False and, in graph mode, an entry of its own.  None enqueues nothing.
    lm: None, or an object whose ``rows(outs, beam, di, max_length, B, k, V, dev_form)`` adds a language model's term to the rows
    the members just wrote (vagnmt_hip.lm.StepFuse: one vag_lm_fuse_beam(_dev)), enqueued after kNN's place and before the
    constraints' mask; the same conditions.  None enqueues nothing."""
    if device_rows and (n_best or align):
        raise ValueError("search.beam: device_rows returns the best row of every sentence (n_best = 0, align = False)")
    if constrain is not None and raw_logits:
        raise ValueError("search.beam: a constrained search runs the log-probability steps (raw_logits=False)")
    if knn is not None and raw_logits:
        raise ValueError("search.beam: a kNN search runs the log-probability steps (raw_logits=False)")
    if lm is not None and raw_logits:
        raise ValueError("search.beam: a search fused with a language model runs the log-probability steps (raw_logits=False)")
    s = _Search(members, h0s, k, max_length, entry)
    e, B, V, M, dev = s.e, s.B, s.V, s.M, s.dev
    beam, nll, n_alive, scratch = e["beam"], e["nll"], e["n_alive"], e["scratch"]
    Tp = members[0].mask.shape[1]                   # the source length the steps run on (padded in graph mode)
    if align and "attn_hist" not in e:
        e["attn_hist"] = torch.empty(max_length, B * k, Tp, device=dev)        # every row the finish reads is written first
    hist = e.get("attn_hist") if align else None

    def before(outs, di, dev_form):
        if align:
            call("vag_beam_attn_record_dev" if dev_form else "vag_beam_attn_record", _pp([mb.alpha for mb in members]), M, ptr(hist),
                 di, max_length, B, k, Tp, stream())
        if knn is not None:
            knn.rows(outs)
        if lm is not None:
            lm.rows(outs, beam, di, max_length, B, k, V, dev_form)
        constrain_rows(constrain, outs, beam, di, max_length, B, k, V, dev_form=dev_form)

    def logits_step():
        # raw logits + the pieces of their rows' log-sum-exp where the vocabulary product provides them: the beam expansion
        # normalises on the fly, no pass over the (B k, V) logits in between
        mb = members[0]
        nparts = ops.head_logits_parts_count(mb.hp, B * k, mb.emb.shape[1], V) if raw_logits else 0
        if nparts <= 0:
            return None

        def one():
            h2, logits, parts = mb.step_logits(e["tok"], mb.h, k, nparts)
            before(None, ptr(e["di"], I32), True)
            call("vag_beam_step_logits_dev_opt", ptr(logits), logits.shape[1], ptr(parts), nparts, ptr(nll), ptr(beam, I64),
                 ptr(e["di"], I32), max_length, ptr(h2), ptr(mb.h), ptr(e["tok"], I64), B, k, V, mb.H, ptr(n_alive, I32),
                 scratch.data_ptr(), flags, stream())
        return one

    steps = s.run(pool, ("vag_beam_ens_step_opt", "vag_beam_ens_step_dev_opt"), (flags,), before, logits_step)
    if align:
        Ts = members[0].Ts
        out = torch.empty(B, n_best, max_length, dtype=I64, device=dev)
        scores = torch.empty(B, n_best, dtype=torch.float32, device=dev)
        attention = torch.empty(B, n_best, max_length, Ts, dtype=torch.float32, device=dev)
        src_pos = torch.empty(B, n_best, max_length, dtype=I64, device=dev)
        call("vag_beam_finish_align", ptr(nll), ptr(beam, I64), ptr(hist), max_length, steps, B, k, n_best, Tp, Ts, ptr(out, I64),
             ptr(scores), ptr(attention), ptr(src_pos, I64), stream())
        return (cut_nbest(out.cpu().numpy(), n_best), scores, attention, src_pos), scores[:, 0], steps
    if n_best:
        out = torch.empty(B, n_best, max_length, dtype=I64, device=dev)
        scores = torch.empty(B, n_best, dtype=torch.float32, device=dev)
        call("vag_beam_finish_nbest", ptr(nll), ptr(beam, I64), max_length, steps, B, k, n_best, ptr(out, I64), ptr(scores),
             stream())
        return (cut_nbest(out.cpu().numpy(), n_best), scores), scores[:, 0], steps
    out = torch.empty(B, max_length, dtype=I64, device=dev)
    best = torch.empty(B, dtype=torch.float32, device=dev)
    call("vag_beam_finish", ptr(nll), ptr(beam, I64), max_length, steps, B, k, ptr(out, I64), ptr(best), stream())
    return (out if device_rows else cut(out.cpu().numpy())), best, steps


def beam_diverse(members, h0s, k, groups, strength, max_length, flags=0, n_best=0, entry=None, pool=None):
    """Diverse beam search: ``beam`` with the k slots in ``groups`` groups and the Hamming penalty ``strength`` between them
    (vag_beam_div_step: groups, strength and flags are by-value arguments of the captured launches, so an entry serves one value
    of each -- build the members with extra=("diverse", groups, strength)).  The members run their log-probability steps (there is no
    raw-logits form).  n_best 0: all k.  Returns ((hyps, scores, group), best scores (B,), decoder steps run): hyps and scores
    as beam's n-best result, group (B, n_best) int64 on the device, the group each ranked hypothesis ended in."""
    n_best = n_best or k
    s = _Search(members, h0s, k, max_length, entry, "vag_beam_div_scratch_bytes")
    steps = s.run(pool, ("vag_beam_div_step", "vag_beam_div_step_dev"), (flags, groups, strength))
    out, scores, slots = s.finish_slots(n_best, steps)
    group = torch.div(slots, k // groups, rounding_mode="floor")
    return (cut_nbest(out.cpu().numpy(), n_best), scores, group), scores[:, 0], steps


def beam_required(members, h0s, k, max_length, required, flags=0, n_best=0, entry=None, pool=None, constrain=None):
    """Beam search with required phrases (vagnmt_hip.require): the allotting expansion (vag_beam_req_step(_dev)) on the members'
    log-probability steps.  required: the (B, 16, 8) int64 phrase table on the host (require.pack).  The table and the per-slot
    state (B, k, 4) the expansion carries from step to step are buffers of the search -- in graph mode static buffers of the
    entry, which the captured launches point at: the table is refilled completely, zeros included, at every call, and step 0
    ignores what the state holds.  constrain: the negative constraints (constrain_rows), masked before every expansion in both
    modes; in graph mode they need an entry of their own, as in ``beam``.  n_best 0: all k.  Returns ((hyps, scores, slots,
    state), best scores (B,), decoder steps run): hyps and scores as beam's n-best result, slots (B, n_best) int64 the final slot
    of each ranked hypothesis, state (B, k, 4) int32 the final states by slot, both on the device."""
    n_best = n_best or k
    s = _Search(members, h0s, k, max_length, entry, "vag_beam_req_scratch_bytes")
    e, B, V, dev = s.e, s.B, s.V, s.dev
    if s.fresh:
        e["req_table"] = torch.empty(B, 16, 8, dtype=I64, device=dev)
        e["req_state"] = torch.empty(B, k, 4, dtype=I32, device=dev)
    table, state = e["req_table"], e["req_state"]
    table.copy_(torch.as_tensor(required, dtype=I64).reshape(B, 16, 8))
    state.zero_()

    def before(outs, di, dev_form):
        constrain_rows(constrain, outs, e["beam"], di, max_length, B, k, V, dev_form=dev_form)

    steps = s.run(pool, ("vag_beam_req_step", "vag_beam_req_step_dev"), (flags, ptr(table, I64), ptr(state, I32)), before)
    out, scores, slots = s.finish_slots(n_best, steps)
    return (cut_nbest(out.cpu().numpy(), n_best), scores, slots, state.clone()), scores[:, 0], steps


def beam_stochastic(members, h0s, k, max_length, rng, flags=0, entry=None, pool=None, constrain=None):
    """Stochastic beam search (vagnmt_hip.stochastic): the Gumbel-perturbed expansion (vag_beam_sbs_step(_dev)) on the members'
    log-probability steps -- k samples without replacement per sentence.  rng: the generator's uint64[2] state on the device; the
    caller advances it after the call.  The perturbed scores (B, k) the expansion carries from step to step are a buffer of the
    search, and in graph mode so are the generator's words the captured launches read (static buffers of the entry).
    constrain: the negative constraints (constrain_rows), masked before every expansion; in graph mode they need an entry of
    their own, as in ``beam``.  Returns ((hyps, tokens, logp, score, gumbel, top), best scores (B,), decoder steps run): the k
    hypotheses of every sentence in sampling order (largest G first; re-ordered from the finish's ranking with torch on the
    device) -- hyps[b] token lists cut at EOS, tokens (B, k, max_length) int64, logp the un-normalised running scores, score the
    finish's length-normalised ones, gumbel the final G (the largest is the root's 0), all (B, k) on the device; top (B, 1), one
    Gumbel(0) draw per sentence under the same generator state and the step index max_length, which no expansion uses."""
    s = _Search(members, h0s, k, max_length, entry, "vag_beam_sbs_scratch_bytes")
    e, B, V, dev = s.e, s.B, s.V, s.dev
    if s.fresh:
        e["gum"] = torch.empty(B, k, device=dev)
        if s.graphed:
            e["rng"] = torch.empty(2, dtype=I64, device=dev)
    gum = e["gum"]
    if s.graphed:
        e["rng"].copy_(rng)                         # the captured launches read the generator's state from the entry's own words
        rng = e["rng"]

    def before(outs, di, dev_form):
        constrain_rows(constrain, outs, e["beam"], di, max_length, B, k, V, dev_form=dev_form)

    steps = s.run(pool, ("vag_beam_sbs_step", "vag_beam_sbs_step_dev"), (flags, ptr(rng, I64), ptr(gum)), before)
    out, scores, slots = s.finish_slots(k, steps)
    # the finish ranks by score; the sampling order is G descending (ties: the finish's order).  Plumbing, not a kernel.
    g = gum.gather(1, slots)
    order = torch.sort(g, dim=1, descending=True, stable=True)[1]
    g, scores, logp = g.gather(1, order), scores.gather(1, order), e["nll"].gather(1, slots).gather(1, order)
    out = out.gather(1, order[:, :, None].expand(B, k, max_length)).contiguous()
    # one more Gumbel draw per sentence, under a step index no expansion used: what vagnmt_hip.stochastic.sbs_uncondition needs
    top = torch.empty(B, 1, device=dev)
    call("vag_sample_noise", ptr(rng, I64), max_length, B, 1, ptr(top), stream())
    return (cut_nbest(out.cpu().numpy(), k), out, logp, scores, g, top), scores[:, 0], steps


def beam_penalised(members, h0s, k, max_length, lp, bonus, beta, stepwise, flags=0, n_best=0, entry=None, pool=None,
                   constrain=None):
    """Beam search with length and coverage penalties (vagnmt_hip.penalty): three launches per step after the members' steps --
    vag_beam_cover(_dev) (with beta > 0: the carried coverage plus this step's attention rows, and its penalty per row), the
    optional mask of ``constrain``, and vag_beam_pen_step(_dev), which selects by the penalised score when ``stepwise`` and
    carries every slot's length, coverage and penalty -- and vag_beam_finish_pen, which ranks by the penalised score.  Build the
    members with align=True (their steps keep the attention rows).  lp, bonus: the host tables of max_length + 1 floats
    (penalty.tables).  lens / cpen (B, k), cov (B, k, Tp), cov_row (B k, Tp), cp_row (B k) and the two tables are buffers of the
    search -- in graph mode static buffers of the entry, whose key holds beta and stepwise (by-value arguments of the captured
    launches); the tables are refilled at every call, so one entry serves every alpha and word_bonus.  constrain: the negative
    constraints (constrain_rows); in graph mode they need an entry of their own, as in ``beam``.  n_best 0: all k.  Returns
    ((hyps, scores, logp, length, cp), best scores (B,), decoder steps run): hyps as beam's n-best result, the rest (B, n_best)
    on the device, best first."""
    n_best = n_best or k
    s = _Search(members, h0s, k, max_length, entry, "vag_beam_pen_scratch_bytes")
    e, B, V, M, dev = s.e, s.B, s.V, s.M, s.dev
    Tp = members[0].mask.shape[1]                   # the source length the steps run on (padded in graph mode)
    cover = beta > 0.0
    if s.fresh:
        e["pen_lens"] = torch.zeros(B, k, dtype=I32, device=dev)
        e["pen_cpen"] = torch.zeros(B, k, device=dev)
        e["pen_cp_row"] = torch.zeros(B * k, device=dev)           # stays +0 without a coverage term
        e["pen_tables"] = torch.empty(2, max_length + 1, device=dev)
        if cover:
            e["pen_cov"] = torch.zeros(B, k, Tp, device=dev)
            e["pen_cov_row"] = torch.zeros(B * k, Tp, device=dev)
    beam, nll = e["beam"], e["nll"]
    lens, cpen, cp_row, tabs = e["pen_lens"], e["pen_cpen"], e["pen_cp_row"], e["pen_tables"]
    cov, cov_row = e.get("pen_cov"), e.get("pen_cov_row")
    tabs.copy_(torch.stack([torch.as_tensor(lp, dtype=torch.float32), torch.as_tensor(bonus, dtype=torch.float32)]))
    mask = members[0].mask

    def before(outs, di, dev_form):
        if cover:
            call("vag_beam_cover_dev" if dev_form else "vag_beam_cover", _pp([mb.alpha for mb in members]), M, ptr(mask), ptr(cov),
                 ptr(beam, I64), di, max_length, B, k, Tp, beta, ptr(cov_row), ptr(cp_row), stream())
        constrain_rows(constrain, outs, beam, di, max_length, B, k, V, dev_form=dev_form)

    steps = s.run(pool, ("vag_beam_pen_step", "vag_beam_pen_step_dev"),
                  (flags, ptr(lens, I32), ptr(cp_row), ptr(cpen), ptr(cov_row), ptr(cov), Tp, ptr(tabs[0]), ptr(tabs[1]), int(stepwise)),
                  before)
    out = torch.empty(B, n_best, max_length, dtype=I64, device=dev)
    scores = torch.empty(B, n_best, dtype=torch.float32, device=dev)
    slots = torch.empty(B, n_best, dtype=I64, device=dev)
    logp = torch.empty(B, n_best, dtype=torch.float32, device=dev)
    length = torch.empty(B, n_best, dtype=I32, device=dev)
    cp = torch.empty(B, n_best, dtype=torch.float32, device=dev)
    call("vag_beam_finish_pen", ptr(nll), ptr(beam, I64), ptr(lens, I32), ptr(cpen), ptr(tabs[0]), ptr(tabs[1]), max_length, steps,
         B, k, n_best, ptr(out, I64), ptr(scores), ptr(slots, I64), ptr(logp), ptr(length, I32), ptr(cp), stream())
    return (cut_nbest(out.cpu().numpy(), n_best), scores, logp, length, cp), scores[:, 0], steps


def sample(members, h0s, n, max_length, temperature, top_k, rng, entry=None, pool=None, top_p=1.0, sizes=None):
    """Draws n samples per source sentence, for at most max_length steps (vag_sample_step: one launch per step after the members'
    steps, which are the plain ones -- build the members with hoist=False).  rng: the generator's uint64[2] state on the device;
    the caller advances it after the call.  entry / pool as in greedy; graph mode captures step 0 (the fan-out of every source
    row to its n samples) and a chunk of DECODE_CHUNK later steps once per decode shape, with the step index, the history and
    the token buffer in device memory; temperature, top_k and n are by-value arguments of the captured launches, so an entry
    serves one value of each.  The alive counter is polled once per chunk (eager mode: every 8 steps): a decode ends early once
    every row has emitted EOS.  Returns (toks (max_length, B n) int64, token_logp (max_length, B n), steps run): the time-major
    history, zero past the steps run (vagnmt_hip.sampling.assemble cuts it).
    top_p < 1 or sizes given: nucleus sampling, the same launches through vag_sample_step_p(_dev); top_p is one more by-value
    argument, so such a decode has entries of its own.  sizes: None, or a (max_length, B n) int32 tensor that receives every
    draw's nucleus size (0 for finished rows and past the steps run)."""
    B, dev = h0s[0].shape[0], h0s[0].device
    N, V, M = B * n, members[0].V, len(members)
    graphed = entry is not None
    e = entry if graphed else {}
    if "toks" in e:
        e["toks"].zero_(); e["lps"].zero_(); e["state"].zero_()
    else:
        e["toks"] = torch.zeros(max_length, N, dtype=I64, device=dev)
        e["lps"] = torch.zeros(max_length, N, device=dev)
        e["state"] = torch.zeros(4, dtype=I32, device=dev)         # n_alive[3] (the count and the kernel's two words) | step index
    toks, lps, n_alive, di_state = e["toks"], e["lps"], e["state"][:3], e["state"][3:]
    Hs = _p64([mb.H for mb in members])
    nucleus = top_p != 1.0 or sizes is not None
    step, step_dev, tail = "vag_sample_step", "vag_sample_step_dev", ()
    if nucleus:
        rec = None
        if sizes is not None:                      # recorded in a buffer of the entry's own: the captured launches point at it
            rec = e["sizes"] = e["sizes"].zero_() if "sizes" in e else torch.zeros(max_length, N, dtype=I32, device=dev)
        step, step_dev, tail = "vag_sample_step_p", "vag_sample_step_p_dev", (top_p, ptr(rec, I32))

    def draw(outs, name, state, *args):        # the step's one launch: name(logp.., history, *args, shape.., generator state, ..)
        call(name, _pp([o[1] for o in outs]), _p64([o[1].shape[1] for o in outs]), M, ptr(toks, I64), ptr(lps), *args, B, n, V,
             temperature, top_k, ptr(state, I64), ptr(n_alive, I32), *tail, stream())

    if not graphed:
        tok, hs, steps = torch.full((B,), SOS_token, dtype=I64, device=dev), list(h0s), 0
        for di in range(max_length):
            outs = [mb.step(tok, h, 1 if di == 0 else n) for mb, h in zip(members, hs)]
            hs = [o[0] for o in outs]
            if di == 0:                            # the states of the B source rows, replicated to the B n samples
                hs = [torch.empty(N, mb.H, device=dev) for mb in members]
            draw(outs, step, rng, di, max_length, _pp([o[0] for o in outs]), _pp(hs), Hs, None)
            tok, steps = toks[di], di + 1
            if di % 8 == 7 and int(n_alive[0].item()) == 0:
                break
        if sizes is not None:
            sizes.copy_(e["sizes"])
        return toks, lps, steps
    if "tok" not in e:
        e["tok"] = torch.empty(N, dtype=I64, device=dev)                     # one token buffer for every member
        e["sos"] = torch.full((B,), SOS_token, dtype=I64, device=dev)
        e["h0"] = [torch.empty_like(h0) for h0 in h0s]
        e["rng"] = torch.empty(2, dtype=I64, device=dev)
        e["one"] = torch.ones(1, dtype=I32, device=dev)
    for buf, h0 in zip(e["h0"], h0s):
        buf.copy_(h0)
    e["rng"].copy_(rng)                            # the captured launches read the generator's state from the entry's own words
    if e.get("graph0") is None:
        def body0():
            outs = [mb.step(e["sos"], h0, 1) for mb, h0 in zip(members, e["h0"])]
            draw(outs, step, e["rng"], 0, max_length, _pp([o[0] for o in outs]), _pp([mb.h for mb in members]), Hs,
                 ptr(e["tok"], I64))
        _capture(e, pool, body0, "graph0")
    e["graph0"].replay()
    steps = 1
    if max_length > 1:
        di_state.copy_(e["one"])                   # the replayed steps start at step 1 (device to device: no host wait)
        if e["graph"] is None:
            def body():
                hs = [mb.h for mb in members]
                for _ in range(DECODE_CHUNK):
                    outs = [mb.step(e["tok"], h, n) for mb, h in zip(members, hs)]
                    hs = [o[0] for o in outs]
                    draw(outs, step_dev, e["rng"], ptr(di_state, I32), max_length, ptr(e["tok"], I64))
                for mb, h in zip(members, hs):
                    mb.h.copy_(h)
            _capture(e, pool, body)
        while steps < max_length:
            e["graph"].replay()
            steps = min(steps + DECODE_CHUNK, max_length)
            if int(n_alive[0].item()) == 0:        # polled once per chunk
                break
    if sizes is not None:
        sizes.copy_(e["sizes"])
    return toks, lps, steps
