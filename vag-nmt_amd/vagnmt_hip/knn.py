"""kNN-MT (Khandelwal et al. 2021): a datastore of (decoder state -> next word) pairs from a translation memory, whose nearest
neighbours are mixed into the model's distribution at every step of a beam search or of forced decoding.  Domain and terminology
adaptation with no gradient step: the soft counterpart of ``required=``.

    store = knn.Datastore.build(model, batches)          # batches of (src_var, src_lengths, tgt, im_var)
    r = model.beamsearch_knn(src_var, src_lengths, im_var, store, beam_size=12, n_best=1, k=8, temperature=10.0, lam=0.5)
    r.hyps[b], r.scores (B, n_best)                      # as beamsearch_nbest, under the mixed distribution
    s = knn.knn_score_translations(model, src_var, src_lengths, tgt, im_var, store, k=8, temperature=10.0, lam=0.5)
    grid = knn.knn_sweep(model, store, dev_batches, lams=[0.2, 0.5], temperatures=[5.0, 10.0, 50.0], k=8)     # perplexities

The key of an entry is h2, the second GRU's state of the step that predicts the word (D = H), stored as bf16; its score for a query
q is 2 q.k - |k|^2 (squared L2 distance up to the row's constant); the K nearest entries' words get the weights
softmax(score / T), and the step's row becomes log((1 - lam) p_model + lam p_knn) (include/vag_nmt.h states all of it).  Three
entry points do the work: vag_knn_store_rows (append a forced batch), vag_knn_search (a streaming search over the keys with the
selection fused in; no (rows, N) matrix) and vag_knn_mix.  A search step pays one vag_knn_search per member and one vag_knn_mix
after the members' steps and before the mask of the constraints, so a ban still wins.  On an Ensemble every member has a store
of its own, built with that member; member m's rows are mixed with member m's neighbours, and the mean of the mixed
probabilities is the mixture of the means, so the expansion is what it was.

Limits: 0 <= lam < 1 (0: nothing is launched and the result is beamsearch_nbest / score_translations bit for bit), T > 0,
1 <= k <= 32, N < 2^31 entries, H a multiple of 8 up to 1024.  Not here: leave-one-out scoring of the store's own sentences,
adaptive lam, approximate or quantised indices, a store sharded over GPUs, kNN in the sampling decoder and the other expansion
searches (they share the hook), any effect on training."""
import math
from collections import namedtuple

import torch

from vagnmt_hip import _lib, constrain, ops, scoring, search
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.search import _p64, _pp

MAX_K = 32              # VAG_KNN_MAX_K (include/vag_nmt.h)
SLICE = 2048            # VAG_KNN_SLICE: keys of one stage-1 workgroup of the search
CHUNK_ROWS = 1 << 16    # entries a store grows by

I32, I64, BF16 = torch.int32, torch.int64, torch.bfloat16

KnnSearch = namedtuple("KnnSearch", ["hyps", "scores", "neighbours"], defaults=(None,))
# index / score (B, n_best, L, K) of the entries retrieved at every position of the returned hypotheses (L: the longest, its EOS
# included; -1 / -inf past a hypothesis's end and past K' = min(K, N)), value: the entries' words (-1 where there is none)
Neighbours = namedtuple("Neighbours", ["index", "score", "value"])


def check_params(k, temperature, lam, what="beamsearch_knn"):
    """Host-side checks of (k, temperature, lam); returns them as (int, float, float)."""
    k, t, lam = int(k), float(temperature), float(lam)
    if not 1 <= k <= MAX_K:
        raise ValueError("%s: need 1 <= k <= %d, got %d" % (what, MAX_K, k))
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError("%s: need a finite temperature > 0, got %r" % (what, temperature))
    if not 0.0 <= lam < 1.0:
        raise ValueError("%s: need 0 <= lam < 1, got %r" % (what, lam))
    return k, t, lam


def mix_scalars(temperature, lam):
    """(1 / T, log lam, log1p(-lam)) formed in double; ctypes rounds each once to fp32 (the precedent of the penalty tables)."""
    return 1.0 / temperature, math.log(lam), math.log1p(-lam)


class Datastore:
    """N entries on one device: ``keys`` (N, D) bf16, ``norm`` (N,) fp32 of the stored keys, ``values`` (N,) int32 words,
    ``sentence`` / ``position`` (N,) int32 provenance.  Storage grows by chunks while batches are appended; the properties (and
    ``finalize()``) make it contiguous."""

    def __init__(self, D, device, chunk_rows=CHUNK_ROWS):
        D = int(D)
        if D < 8 or D > 1024 or D % 8:
            raise ValueError("Datastore: the key depth must be a multiple of 8 in [8, 1024], got %d" % D)
        self.D, self.device, self.chunk_rows = D, torch.device(device), int(chunk_rows)
        self._chunks, self._fill, self._n, self._sentences = [], 0, 0, 0

    def __len__(self):
        return self._n

    def _new_chunk(self, rows):
        dev = self.device
        self._chunks.append(dict(keys=torch.empty(rows, self.D, dtype=BF16, device=dev), norm=torch.empty(rows, device=dev),
                                 values=torch.empty(rows, dtype=I32, device=dev), sentence=torch.empty(rows, dtype=I32, device=dev),
                                 position=torch.empty(rows, dtype=I32, device=dev)))
        self._fill = 0

    def append(self, h2, tgt):
        """One forced batch: h2 (Tt, B, H) fp32 as ops.cgru_decode_seq leaves it, tgt (B, Tt) int64 -- the rows of every
        sentence's scored span, in the order sentence, then position.  Returns the number of entries added."""
        Tt, B, H = h2.shape
        if H != self.D or tuple(tgt.shape) != (B, Tt):
            raise ValueError("Datastore.append: h2 %s / tgt %s do not fit a store of depth %d" % (tuple(h2.shape), tuple(tgt.shape), self.D))
        if self._n + B * Tt >= 1 << 31:
            raise ValueError("Datastore.append: a store holds fewer than 2^31 entries")
        if not self._chunks or self._chunks[-1]["norm"].shape[0] - self._fill < B * Tt:
            if self._chunks:
                self._trim()
            self._new_chunk(max(self.chunk_rows, B * Tt))
        c, f = self._chunks[-1], self._fill
        cap = c["norm"].shape[0] - f
        count = torch.zeros(1, dtype=I32, device=self.device)
        call("vag_knn_store_rows", ptr(h2), ptr(tgt, I64), B, Tt, H, self._sentences, cap, c["keys"][f:].data_ptr(),
             c["norm"][f:].data_ptr(), c["values"][f:].data_ptr(), c["sentence"][f:].data_ptr(), c["position"][f:].data_ptr(),
             ptr(count, I32), stream())
        n = int(count.item())
        assert 0 <= n <= cap
        self._fill += n
        self._n += n
        self._sentences += B
        return n

    def _trim(self):
        c = self._chunks[-1]
        self._chunks[-1] = {k: v[:self._fill] for k, v in c.items()}

    def finalize(self):
        """One contiguous tensor per field, exactly N entries long."""
        if not self._chunks:
            self._new_chunk(0)
        if len(self._chunks) > 1 or self._chunks[0]["norm"].shape[0] != self._fill:
            self._trim()
            self._chunks = [{k: torch.cat([c[k] for c in self._chunks]).contiguous() for k in self._chunks[0]}]
            self._fill = self._n
        return self

    keys = property(lambda self: self.finalize()._chunks[0]["keys"])
    norm = property(lambda self: self.finalize()._chunks[0]["norm"])
    values = property(lambda self: self.finalize()._chunks[0]["values"])
    sentence = property(lambda self: self.finalize()._chunks[0]["sentence"])
    position = property(lambda self: self.finalize()._chunks[0]["position"])

    def identity(self):
        """What a captured search launch holds of this store, by pointer and by value."""
        return (self.keys.data_ptr(), self.norm.data_ptr(), self.values.data_ptr(), self._n)

    @classmethod
    def from_tensors(cls, keys, values, sentence=None, position=None):
        """A store from given entries on a GPU: keys (N, D) -- rounded to bf16 here if they are not bf16 -- and values (N,) words;
        the norms are taken from the stored keys (torch, fp32).  sentence / position default to -1."""
        keys = keys.to(BF16).contiguous()
        if keys.dim() != 2 or values.shape != (keys.shape[0],) or not keys.is_cuda:
            raise ValueError("Datastore.from_tensors: need keys (N, D) and values (N,) on the GPU")
        store = cls(keys.shape[1], keys.device)
        n, none = keys.shape[0], lambda t: torch.full((keys.shape[0],), -1, dtype=I32, device=keys.device) if t is None else t.to(I32)
        store._chunks = [dict(keys=keys, norm=(keys.float() ** 2).sum(1), values=values.to(I32).contiguous(),
                              sentence=none(sentence).contiguous(), position=none(position).contiguous())]
        store._fill = store._n = n
        return store

    @classmethod
    def build(cls, model, batches, chunk_rows=CHUNK_ROWS):
        """The store of a translation memory under ``model``: every batch (src_var, src_lengths, tgt, im_var) runs the forced
        prologue and the whole-sequence decoder in eval mode without gradients -- no head -- and is appended."""
        store = None
        mode = model.training
        model.eval()
        try:
            with torch.no_grad():
                for src_var, src_lengths, tgt, im_var in batches:
                    mm = hasattr(model, "vse_imagine")
                    tgt, tok = scoring.forced_args([model], [mm], src_var, tgt, im_var, "Datastore.build")
                    h2 = member_forced(model, src_var, src_lengths, im_var, tok, tgt, head=False)
                    if store is None:
                        store = cls(h2.shape[2], h2.device, chunk_rows)
                    store.append(h2, tgt)
        finally:
            model.train(mode)
        if store is None:
            raise ValueError("Datastore.build: no batches")
        return store.finalize()

    def save(self, path):
        torch.save({k: getattr(self, k).cpu() for k in ("keys", "norm", "values", "sentence", "position")}, path)

    @classmethod
    def load(cls, path, device="cuda"):
        d = torch.load(path, map_location="cpu")
        keys = d["keys"]
        if keys.dim() != 2 or keys.dtype != BF16 or any(d[k].shape != (keys.shape[0],) for k in ("norm", "values", "sentence", "position")):
            raise ValueError("Datastore.load: %s does not hold a datastore" % path)
        store = cls(keys.shape[1], device)
        store._chunks = [{k: d[k].to(store.device).contiguous() for k in ("keys", "norm", "values", "sentence", "position")}]
        store._fill = store._n = keys.shape[0]
        store._sentences = int(d["sentence"].max()) + 1 if store._n else 0
        return store

    def check(self, model, what="beamsearch_knn"):
        """ValueError for a store that does not fit the model: another depth than its H, words beyond its V, no entries."""
        H, V = model.decoder.dec_params()[1].shape[1], model.decoder.out.bias.shape[0]
        if self.D != H:
            raise ValueError("%s: the datastore's keys have depth %d, the model's decoder state %d" % (what, self.D, H))
        if self._n < 1:
            raise ValueError("%s: the datastore is empty" % what)
        lo, hi = int(self.values.min()), int(self.values.max())
        if lo < 0 or hi >= V:
            raise ValueError("%s: the datastore's words lie in [%d, %d], the model's vocabulary is [0, %d)" % (what, lo, hi, V))


def member_forced(model, src_var, src_lengths, im_var, tok, tgt, head=True):
    """scoring._member_logits that also returns the decoder states: (logits (Tt*B, ldl), lse (Tt*B,), h2 (Tt, B, H)) of one model
    in inference mode, time-major rows; head=False: h2 alone, the head is not run."""
    dec = model.decoder
    enc, mask, h0 = model._decode_prologue(src_var, src_lengths, im_var)
    B, Tt = tgt.shape
    V = dec.out.bias.shape[0]
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
    h2 = h2.contiguous()
    if not head:
        return h2
    ldl = (V + 3) // 4 * 4
    E, H, R, dev = dec.embedding.weight.shape[1], h2.shape[2], Tt * B, enc.device
    tmid = torch.empty(Tt, B, E, device=dev)
    logits = torch.empty(R, ldl, device=dev)
    lse, nll = torch.empty(R, device=dev), torch.empty(R, device=dev)
    inv_cnt, loss, vw = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.ones(V, device=dev)
    call("vag_head_ce_seq_fwd", ptr(h2), ptr(c), ptr(e), ops._head_w(dec.head_params()), ptr(tgt, I64), ptr(vw), B, Tt, E, H, V, 0.0,
         None, 0, ptr(tmid), ptr(logits), ldl, ptr(lse), ptr(nll), ptr(inv_cnt), ptr(loss), stream())
    return logits, lse, h2


class Retrieval:
    """The neighbour lists of one search or one forced batch: per member the (rows, K) scores and indices vag_knn_search writes
    and its scratch.  Graph mode (entry given): static buffers of the entry, which also keeps the stores alive -- the captured
    launches point at both."""

    def __init__(self, stores, rows, k, dev, entry=None):
        self.stores, self.K, self.rows_max = list(stores), int(k), int(rows)
        bufs = entry.get("knn_bufs") if entry is not None else None
        if bufs is None:
            L = _lib.lib()
            bufs = [dict(score=torch.empty(rows, k, device=dev), index=torch.empty(rows, k, dtype=I32, device=dev),
                         scratch=torch.empty(L.vag_knn_scratch_bytes(rows, len(s), k), dtype=torch.uint8, device=dev))
                    for s in self.stores]
            if entry is not None:
                entry["knn_bufs"], entry["knn_stores"] = bufs, self.stores
        self.bufs = bufs

    def search(self, queries):
        """queries: per member a (rows, H) fp32 matrix (row stride = its leading dimension)."""
        for q, s, b in zip(queries, self.stores, self.bufs):
            if q.dim() != 2 or q.stride(1) != 1 or q.shape[0] > self.rows_max or q.shape[1] != s.D or q.dtype != torch.float32 \
                    or not q.is_cuda:
                raise _lib.VagError("knn: queries must be fp32 (rows <= %d, %d) on the GPU with contiguous rows" % (self.rows_max, s.D))
            call("vag_knn_search", q.data_ptr(), q.stride(0), q.shape[0], s.D, s.keys.data_ptr(),
                 ptr(s.norm), len(s), self.K, ptr(b["score"]), ptr(b["index"], I32), b["scratch"].data_ptr(), stream())

    def mix(self, rows, V, temperature, lam, lse=None):
        """rows: per member the (R, ldl) matrix to rewrite; lse: None or per member the rows' log-sum-exp."""
        inv_T, log_lam, log1m = mix_scalars(temperature, lam)
        call("vag_knn_mix", _pp(rows, None), _p64([r.shape[1] for r in rows]), len(rows), rows[0].shape[0], V,
             _pp([b["score"] for b in self.bufs], None), _pp([b["index"] for b in self.bufs], None), self.K,
             _pp([s.values for s in self.stores], None), _p64([len(s) for s in self.stores]),
             _pp(lse, None) if lse is not None else None, inv_T, log_lam, log1m, stream())


class StepMix:
    """What search.beam's ``knn=`` takes: ``rows(outs)`` enqueues, on the rows the members just wrote (outs: their (h2, logp)
    pairs), one vag_knn_search per member and one vag_knn_mix.  Neither depends on the step index: the same calls serve eager
    mode and a captured graph."""

    def __init__(self, retrieval, V, temperature, lam):
        self.r, self.V, self.t, self.lam = retrieval, V, temperature, lam

    def rows(self, outs):
        self.r.search([o[0] for o in outs])
        self.r.mix([o[1] for o in outs], self.V, self.t, self.lam)


def graph_key(stores, k, temperature, lam):
    """Everything the captured launches of a kNN search hold by value or by pointer: part of the graph entry's key."""
    return (k, temperature, lam) + tuple(x for s in stores for x in s.identity())


def search_args(models, datastore, k, temperature, lam, what="beamsearch_knn"):
    """Host-side checks shared by the search and the scoring: returns (stores, k, temperature, lam)."""
    k, t, lam = check_params(k, temperature, lam, what)
    stores = list(datastore) if isinstance(datastore, (list, tuple)) else [datastore]
    if len(stores) != len(models):
        raise ValueError("%s: %d datastores for %d models (an ensemble takes one per member)" % (what, len(stores), len(models)))
    for s, m in zip(stores, models):
        if not isinstance(s, Datastore):
            raise ValueError("%s: datastore must be a vagnmt_hip.knn.Datastore" % what)
        s.check(m, what)
    return stores, k, t, lam


def _retrieve_forced(models, stores, src_var, src_lengths, tgt, tok, im_var, k):
    """Per member the forced (logits, lse) and the neighbour lists of the Tt*B rows (one vag_knn_search per member)."""
    outs = [member_forced(m, src_var, src_lengths, im_var, tok, tgt) for m in models]
    B, Tt = tgt.shape
    r = Retrieval(stores, Tt * B, k, tgt.device)
    r.search([o[2].view(Tt * B, -1) for o in outs])
    return outs, r


def _forced_score(rows, lses, tgt, V):
    B, Tt = tgt.shape
    M = len(rows)
    token_logp, logp, score = torch.empty(B, Tt, device=tgt.device), torch.empty(B, device=tgt.device), torch.empty(B, device=tgt.device)
    call("vag_forced_score", _pp(rows, None), _p64([r.shape[1] for r in rows]), _pp(lses, None), M, ptr(tgt, I64), B, Tt, V,
         ptr(token_logp), ptr(logp), ptr(score), stream())
    return scoring.Scores(score, logp, token_logp)


def knn_score_translations(obj, src_var, src_lengths, tgt, im_var, datastore, k=8, temperature=10.0, lam=0.5):
    """score_translations under the mixed distribution: Scores(score (B,), logp (B,), token_logp (B, Tt)).  obj: a model or an
    Ensemble (then ``datastore`` is a list, one store per member).  One vag_knn_search over the Tt*B forced rows per member, one
    vag_knn_mix on the logits with their log-sum-exp, then the unchanged vag_forced_score with a zero log-sum-exp.  lam = 0 is
    score_translations bit for bit.  What the search's scores are checked against, and how lam and T are tuned."""
    what = "knn_score_translations"
    models, mm = scoring.models_of(obj)
    stores, k, t, lam = search_args(models, datastore, k, temperature, lam, what)
    tgt, tok = scoring.forced_args(models, mm, src_var, tgt, im_var, what)
    V = int(models[0].tgt_size)
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            if lam == 0.0:
                outs = [member_forced(m, src_var, src_lengths, im_var, tok, tgt) for m in models]
                return _forced_score([o[0] for o in outs], [o[1] for o in outs], tgt, V)
            outs, r = _retrieve_forced(models, stores, src_var, src_lengths, tgt, tok, im_var, k)
            r.mix([o[0] for o in outs], V, t, lam, [o[1] for o in outs])
            zero = torch.zeros(tgt.numel(), device=tgt.device)
            return _forced_score([o[0] for o in outs], [zero] * len(outs), tgt, V)
    finally:
        for m, tr in zip(models, modes):
            m.train(tr)


def span_words(tgt):
    """Number of scored positions of (B, Tt) targets: up to and including the first EOS, to the last non-pad word otherwise."""
    Tt = tgt.shape[1]
    pos = torch.arange(Tt, device=tgt.device)[None, :]
    eos, nz = tgt == search.EOS_token, tgt != 0
    first = torch.where(eos, pos, Tt).min(1)[0]
    last = torch.where(nz, pos, -1).max(1)[0]
    return (torch.where(eos.any(1), first, last) + 1).sum()


def knn_sweep(obj, datastore, dev_batches, lams, temperatures, k=8):
    """Corpus perplexities exp(-sum logp / sum n) of dev_batches (batches of (src_var, src_lengths, tgt, im_var)) under the mixed
    distribution for every (lam, T): a (len(lams), len(temperatures)) float64 tensor on the host.  The neighbours of a batch's
    forced rows are retrieved once (they depend on neither lam nor T); every grid point mixes a copy of the logits and scores
    it; the sums stay on the device and are read once."""
    what = "knn_sweep"
    models, mm = scoring.models_of(obj)
    lams, temps = [float(x) for x in lams], [float(x) for x in temperatures]
    if not lams or not temps:
        raise ValueError("%s: empty grid" % what)
    stores, k, _, _ = search_args(models, datastore, k, temps[0], lams[0], what)
    for lam in lams:
        for t in temps:
            check_params(k, t, lam, what)
    V = int(models[0].tgt_size)
    modes = [m.training for m in models]
    total = words = None
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            for src_var, src_lengths, tgt, im_var in dev_batches:
                tgt, tok = scoring.forced_args(models, mm, src_var, tgt, im_var, what)
                outs, r = _retrieve_forced(models, stores, src_var, src_lengths, tgt, tok, im_var, k)
                if total is None:
                    total = torch.zeros(len(lams), len(temps), dtype=torch.float64, device=tgt.device)
                    words = torch.zeros((), dtype=I64, device=tgt.device)
                words += span_words(tgt)
                zero = torch.zeros(tgt.numel(), device=tgt.device)
                for i, lam in enumerate(lams):
                    for j, t in enumerate(temps):
                        if lam == 0.0:
                            s = _forced_score([o[0] for o in outs], [o[1] for o in outs], tgt, V)
                        else:
                            rows = [o[0].clone() for o in outs]
                            r.mix(rows, V, t, lam, [o[1] for o in outs])
                            s = _forced_score(rows, [zero] * len(outs), tgt, V)
                        total[i, j] += s.logp.double().sum()
    finally:
        for m, tr in zip(models, modes):
            m.train(tr)
    if total is None:
        raise ValueError("%s: no batches" % what)
    return torch.exp(-(total / words.double())).cpu()


def neighbours_of(obj, src_var, src_lengths, im_var, hyps, datastore, k):
    """The entries retrieved along given hypotheses (hyps[b]: n token lists), by forced decoding of them: per member a
    Neighbours(index, score, value), each (B, n, L, K) on the device.  A single model gets the one Neighbours, an Ensemble a list."""
    models, mm = scoring.models_of(obj)
    stores, k, _, _ = search_args(models, datastore, k, 1.0, 0.5, "beamsearch_knn")
    B, n = len(hyps), len(hyps[0])
    flat = [list(h) for hs in hyps for h in hs]
    src_n = src_var.repeat_interleave(n, 0)
    lens_n = [x for x in list(src_lengths) for _ in range(n)]
    im_n = im_var.repeat_interleave(n, 0) if im_var is not None else None
    with torch.no_grad():
        tgt, tok = scoring.forced_args(models, mm, src_n, flat, im_n, "beamsearch_knn")
        _, r = _retrieve_forced(models, stores, src_n, lens_n, tgt, tok, im_n, k)
        Tt = tgt.shape[1]
        end = torch.tensor([len(h) if search.EOS_token not in h else list(h).index(search.EOS_token) for h in flat], device=tgt.device)
        live = (torch.arange(Tt, device=tgt.device)[:, None] <= end[None, :]).view(Tt, B * n, 1)          # (time-major rows)
        out = []
        for s, b in zip(stores, r.bufs):
            idx = torch.where(live, b["index"].view(Tt, B * n, k), -1)
            sc = torch.where(live, b["score"].view(Tt, B * n, k), float("-inf"))
            val = torch.where(idx >= 0, s.values[idx.clamp(min=0).long()], -1)
            out.append(Neighbours(*[x.permute(1, 0, 2).reshape(B, n, Tt, k).contiguous() for x in (idx, sc, val)]))
    return out if hasattr(obj, "models") else out[0]


def beamsearch_knn(obj, src_var, src_lengths, im_var, datastore, beam_size=12, n_best=1, max_length=80, k=8, temperature=10.0,
                   lam=0.5, return_neighbours=False, avoid_double=True, avoid_unk=False, prefix=None, banned=None,
                   banned_per_sentence=None, no_repeat_ngram=0):
    """beamsearch_nbest under the mixed distribution: KnnSearch(hyps, scores[, neighbours]); obj a model or an Ensemble (then
    ``datastore`` is a list with one store per member).  search.beam on the members' log-probability steps with ``knn=``: after
    the members' steps the rows (B at step 0, B beam_size afterwards) are searched and mixed, then masked by the constraints
    (prefix / banned / banned_per_sentence / no_repeat_ngram as beamsearch_constrained takes them: a ban still wins), then
    expanded.  The scores are the length-normalised sums of the mixed log-probabilities: what knn_score_translations gives for
    the returned words.  Graph mode keeps an entry of its own per (k, temperature, lam, store identity and length).
    return_neighbours: the entries retrieved along the returned hypotheses (neighbours_of: forced decoding of them)."""
    what = "beamsearch_knn"
    models, mm = scoring.models_of(obj)
    stores, k, t, lam = search_args(models, datastore, k, temperature, lam, what)
    kb, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
    ml, B, V = int(max_length), src_var.shape[0], int(models[0].tgt_size)
    packed = constrain.pack(B, V, ml, prefix, banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk, what)
    packed = constrain.any_of(packed)
    if im_var is None and any(mm):
        raise ValueError("%s: a multimodal model needs im_var" % what)
    if lam == 0.0 and packed is None:           # IS beamsearch_nbest; with constraints nothing of kNN is enqueued either
        res = scoring.nbest_search(obj, src_var, src_lengths, im_var, kb, ml, flags, n)
    else:
        key = (("knn",) + graph_key(stores, k, t, lam)) if lam > 0.0 else ()
        with torch.no_grad():
            s = obj._search_setup(src_var, src_lengths, im_var, kb, ml, "beam_knn", flags, extra=constrain.graph_key(packed) + key)
            mix = StepMix(Retrieval(stores, s.B * kb, k, s.device, s.entry), V, t, lam) if lam > 0.0 else None
            res = obj._search_done(search.beam(s.members, s.h0s, kb, ml, flags, n, s.entry, s.pool, raw_logits=False,
                                               constrain=constrain.on_device(packed, s, ml), knn=mix), kb)
    nb = neighbours_of(obj, src_var, src_lengths, im_var, res[0], datastore, k) if return_neighbours else None
    return KnnSearch(res[0], res[1], nb)
