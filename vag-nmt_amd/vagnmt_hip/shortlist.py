"""Lexical shortlists: decoding over a per-batch compact target vocabulary (Jean et al. 2015; Marian's --shortlist).

Every decoding path pays for the whole target vocabulary at every step.  A batch of short sentences has a few hundred plausible
target words: the special words, the most frequent words, and the ``best`` lexicon translations of the source words actually
present.  A search takes everything vocabulary-sized from three tensors of the decoder (``embedding.weight``, ``out.weight``,
``out.bias``), so cutting those three down to the chosen words -- per batch, on the device -- moves every existing kernel onto the
compact vocabulary without changing one of them.

    lex = Lexicon.from_alignments(model, batches, best=100)          # or from_counts / from_text / load
    sl = Shortlist(model, lex, first=100, best=100)                  # model: a model or an Ensemble
    hyps = sl.beamsearch_decode(src_var, src_lengths, im_var, beam_size=12, max_length=80)       # full ids, as the model's
    nbest, scores = sl.beamsearch_nbest(src_var, src_lengths, im_var, 12, 5)
    s = sl.score_translations(src_var, src_lengths, tgt, im_var)     # ShortScores(score, logp, token_logp, absent)
    sel = sl.select(src_var, src_lengths)                            # then any other search on sl.view:
    c = sl.to_full(sl.view.beamsearch_constrained(src_var, src_lengths, im_var, banned=sl.to_short([[17]])))

``select`` is three kinds of launches and no host read: vag_shortlist_select (the ids, ascending, and the full -> compact map),
one vag_shortlist_gather per tensor and member into persistent (capacity, .) buffers, and a bump of the views'
``_vag_weights_version``, on which the models' own ``_decode_weights`` refreshes ``prep`` and the token tables in place: one cache
key and one captured graph per decode shape for the object's life.  Rows past the chosen words are pad words: weight 0, bias
-1e30, so a pad's logit is -1e30 -- it adds exactly 0 to every log-sum-exp and is never chosen while a real word is left.

Compact ids ascend with full ids, so the searches' "word ascending" tie-break picks the same word in either numbering, and PAD,
UNK, SOS, EOS keep the ids 0 .. 3 every kernel knows.  Scores are renormalised over the shortlist, as in Marian: they are what
``sl.score_translations`` gives and NOT the full model's scores.

A view is decode-only.  It shares the encoder, the image branch and every recurrent and head parameter with its member (same
storage); the member itself, the training step and validate() are untouched.  The view follows the member's decode_* switches
and train/eval mode at every ``select``.  Not built: beamsearch_lm / beamsearch_knn on a view (their tables are indexed by full
ids), a shortlist inside the training step, per-sentence shortlists."""
import inspect
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from vagnmt_hip import _lib, scoring
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.ensemble import Ensemble
from vagnmt_hip.search import UNK_token
from vagnmt_hip.state import lengths_tensor

MAX_V = 131072          # vag_shortlist_supported's limits
MAX_K = 256
PAD_BIAS = -1e30        # a pad word's bias (its weights are 0): exp(-1e30 - lse) == 0 in fp32
N_SPECIAL = 4           # PAD, UNK, SOS, EOS

I32, I64 = torch.int32, torch.int64

Selection = namedtuple("Selection", ["n", "rank_used", "ids"])
ShortScores = namedtuple("ShortScores", ["score", "logp", "token_logp", "absent"])
# fields of the searches' named tuples that hold target words (token lists or int64 tensors); every other field passes through
TOKEN_FIELDS = ("hyps", "top", "best")
_DECODE_SWITCHES = ("decode_graph", "decode_persistent", "decode_raw_logits", "decode_hoisted")


# ------------------------------------------------------------------------------------------------------ lexicon
class Lexicon:
    """table (Vs, K) int32: row s holds the target ids of the K best translations of source word s, best first, padded with -1.
    Vt: the target vocabulary the ids belong to.  Host-side (NumPy); ``to(device)`` adds the device copy the kernel reads."""

    def __init__(self, table, Vt):
        table = np.ascontiguousarray(table, dtype=np.int32)
        if table.ndim != 2 or table.shape[0] < 1 or not 1 <= table.shape[1] <= MAX_K:
            raise ValueError("Lexicon: table must be (Vs >= 1, 1 <= K <= %d), got %s" % (MAX_K, table.shape))
        if int(Vt) < 1 or (table.size and int(table.max()) >= int(Vt)):
            raise ValueError("Lexicon: target ids must lie below Vt = %d" % int(Vt))
        self.table, self.Vt = table, int(Vt)
        self.Vs, self.K = table.shape
        self.device_table = None

    @classmethod
    def from_counts(cls, src_ids, tgt_ids, counts, Vs, Vt, best=100):
        """The top ``best`` target words per source word by summed count; ties go to the smaller target id.  Pairs outside
        [0, Vs) x [0, Vt) and counts <= 0 are dropped.  K = min(best, the longest row), at least 1."""
        best = int(best)
        if not 1 <= best <= MAX_K:
            raise ValueError("Lexicon: need 1 <= best <= %d, got %d" % (MAX_K, best))
        s = np.asarray(src_ids, dtype=np.int64).reshape(-1)
        t = np.asarray(tgt_ids, dtype=np.int64).reshape(-1)
        c = np.asarray(counts, dtype=np.float64).reshape(-1)
        if not (len(s) == len(t) == len(c)):
            raise ValueError("Lexicon.from_counts: src_ids, tgt_ids and counts differ in length")
        keep = (s >= 0) & (s < Vs) & (t >= 0) & (t < Vt) & (c > 0)
        key, inv = np.unique(s[keep] * int(Vt) + t[keep], return_inverse=True)
        tot = np.zeros(len(key), dtype=np.float64)
        np.add.at(tot, inv.reshape(-1), c[keep])
        s, t = key // int(Vt), key % int(Vt)
        order = np.lexsort((t, -tot, s))                  # source word, then count descending, then target id ascending
        s, t = s[order], t[order]
        start = np.searchsorted(s, s, side="left")        # first row of each source word's run
        rank = np.arange(len(s)) - start
        K = int(min(best, rank.max() + 1)) if len(s) else 1
        table = np.full((int(Vs), K), -1, dtype=np.int32)
        top = rank < K
        table[s[top], rank[top]] = t[top]
        return cls(table, Vt)

    @classmethod
    def from_alignments(cls, obj, batches, best=100):
        """Counts (source word, target word) pairs over ``batches`` of (src_var, src_lengths, tgt[, im_var]) from the attention
        arg-max of forced decoding (align_translations' src_pos) on a model or an Ensemble.  Target words <= 3 are not counted
        (the special words are always in a shortlist)."""
        models, _ = scoring.models_of(obj)
        Vs, Vt = int(models[0].src_size), int(models[0].tgt_size)
        ss, tt = [], []
        for batch in batches:
            src_var, src_lengths, tgt = batch[0], batch[1], batch[2]
            im_var = batch[3] if len(batch) > 3 else None
            tgt = scoring.targets_tensor(tgt, src_var.shape[0], src_var.device)
            pos = obj.align_translations(src_var, src_lengths, tgt, im_var).src_pos
            ok = (pos >= 0) & (tgt > 3)
            words = torch.gather(src_var, 1, pos.clamp(min=0).to(I64))
            ss.append(words[ok].cpu().numpy())
            tt.append(tgt[ok].cpu().numpy())
        s = np.concatenate(ss) if ss else np.zeros(0, np.int64)
        t = np.concatenate(tt) if tt else np.zeros(0, np.int64)
        return cls.from_counts(s, t, np.ones(len(s)), Vs, Vt, best)

    @classmethod
    def from_text(cls, path, src_vocab, tgt_vocab, best=100):
        """Reads "src tgt prob" lines (a probabilistic lexicon as fast_align / Marian's lex files give); src_vocab / tgt_vocab map
        words to ids.  Lines with an unknown word or a malformed number are skipped."""
        s, t, c = [], [], []
        with open(path, encoding="utf-8") as f:
            for line in f:
                parts = line.split()
                if len(parts) != 3 or parts[0] not in src_vocab or parts[1] not in tgt_vocab:
                    continue
                try:
                    p = float(parts[2])
                except ValueError:
                    continue
                s.append(int(src_vocab[parts[0]])); t.append(int(tgt_vocab[parts[1]])); c.append(p)
        Vs = max([int(v) for v in src_vocab.values()] + [0]) + 1
        Vt = max([int(v) for v in tgt_vocab.values()] + [0]) + 1
        return cls.from_counts(s, t, c, Vs, Vt, best)

    def save(self, path):
        np.savez(path, table=self.table, Vt=np.int64(self.Vt))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["table"], int(z["Vt"]))

    def to(self, device):
        self.device_table = torch.from_numpy(self.table).to(device)
        return self


# ------------------------------------------------------------------------------------------------------ host-side rules
def default_capacity(V, n_always, best):
    """min(V, n_always + 64 best) rounded up to a multiple of 256, and never above V."""
    c = min(int(V), int(n_always) + 64 * int(best))
    return min(int(V), (c + 255) // 256 * 256)


def check_beam_width(beam_size, n_always, what="shortlist"):
    """A beam of k expands k words per hypothesis at a step: with 2 k real words always present a pad word can never surface."""
    if int(beam_size) > int(n_always) // 2:
        raise ValueError("%s: beam_size %d exceeds len(always) // 2 = %d: a pad word could surface; widen `first` / `always`"
                         % (what, int(beam_size), int(n_always) // 2))


def _no_full_tables(name):
    def refuse(self, *args, **kwargs):
        raise NotImplementedError("%s on a shortlist view: its tables are indexed by full target ids (compact tables are not "
                                  "built); run it on the model itself" % name)
    refuse.__name__ = name
    return refuse


class _ViewRules:
    """What a view refuses, whichever class it wraps."""
    beamsearch_lm = _no_full_tables("beamsearch_lm")
    beamsearch_knn = _no_full_tables("beamsearch_knn")
    lm_score_translations = _no_full_tables("lm_score_translations")
    knn_score_translations = _no_full_tables("knn_score_translations")

    def _check_kind(self, k, kind):
        if kind in ("beam_lm", "beam_knn"):
            raise NotImplementedError("%s on a shortlist view: its tables are indexed by full target ids" % kind)
        if kind.startswith("beam"):
            check_beam_width(k, self._shortlist_always, kind)

    def _search_setup(self, src_var, src_lengths, im_var, k, max_length, kind, *args, **kwargs):
        self._check_kind(k, kind)
        return super()._search_setup(src_var, src_lengths, im_var, k, max_length, kind, *args, **kwargs)


class _ModelView(_ViewRules):
    def _beam(self, enc, mask, h, beam_size, *args, **kwargs):
        check_beam_width(beam_size, self._shortlist_always, "beam search")
        return super()._beam(enc, mask, h, beam_size, *args, **kwargs)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("a shortlist view is decode-only: train the model it was made from")


class _EnsembleView(_ViewRules, Ensemble):
    def _beam(self, pro, k, *args, **kwargs):
        check_beam_width(k, self._shortlist_always, "beam search")
        return super()._beam(pro, k, *args, **kwargs)


_view_classes = {}


def _view_class(cls):
    v = _view_classes.get(cls)
    if v is None:
        v = _view_classes[cls] = type("Shortlist" + cls.__name__, (_ModelView, cls), {})
    return v


def _shallow(module, cls=None):
    """A module object of its own over the SAME parameters, buffers and submodules (their containers copied, so that an entry can
    be replaced in the copy alone); what decoding cached on the original is not carried over."""
    new = object.__new__(cls or type(module))
    d = {k: v for k, v in module.__dict__.items() if not (k.startswith("_decode_") or k.startswith("_vag_"))}
    for name in ("_parameters", "_buffers", "_modules"):
        d[name] = type(d[name])(d[name])
    new.__dict__.update(d)
    return new


def _member_view(model, cap, n_always):
    """The decode-only view of one member: the member's class, its modules by reference, and a decoder whose embedding and
    output layer are (cap, .) buffers of their own (one buffer where tied_emb)."""
    dec = model.decoder
    emb_w, out_w, out_b = dec.embedding.weight, dec.out.weight, dec.out.bias
    dev, E = emb_w.device, emb_w.shape[1]
    with torch.random.fork_rng(devices=[]):                # (the placeholder layers' initialisers draw random numbers)
        emb = nn.Embedding(1, 1, padding_idx=0)
        out = nn.Linear(1, 1)
    emb.weight = nn.Parameter(torch.zeros(cap, E, device=dev), requires_grad=False)
    emb.num_embeddings, emb.embedding_dim = cap, E
    tied = out_w is emb_w
    out.weight = emb.weight if tied else nn.Parameter(torch.zeros(cap, out_w.shape[1], device=dev), requires_grad=False)
    out.bias = nn.Parameter(torch.full((cap,), PAD_BIAS, device=dev), requires_grad=False)
    out.in_features, out.out_features = out_w.shape[1], cap
    dview = _shallow(dec)
    dview._modules["embedding"] = emb
    dview._modules["out"] = out
    view = _shallow(model, _view_class(type(model)))
    view._modules["decoder"] = dview
    view.tgt_size = cap
    view._shortlist_always = n_always
    return view


# ------------------------------------------------------------------------------------------------------ the shortlist
class Shortlist:
    """Shortlist(obj, lexicon, first=100, best=100, capacity=None, always=None).

    obj: a model or an Ensemble (all members take one selection).  always: the ids every shortlist holds (default 0 .. 3 + first;
    PAD, UNK, SOS, EOS must be among them).  best: lexicon ranks per source word.  capacity: rows of the compact tensors, fixed
    for the object's life (default: default_capacity).  ``view``: the decode-only model (or Ensemble of such models) whose
    vocabulary is the last selection's."""

    def __init__(self, obj, lexicon, first=100, best=100, capacity=None, always=None):
        if hasattr(obj, "backend") and hasattr(obj, "model"):            # a step driver: its model, unless it stores 2-byte weights
            if getattr(getattr(obj.backend, "f", None), "storage16", False):
                raise NotImplementedError("Shortlist: the 2-byte storage mode is not supported (the gathers copy fp32 rows)")
            obj = obj.model
        models, multimodal = scoring.models_of(obj)
        for m in models:
            if not (hasattr(m, "_decode_prologue") and hasattr(m, "decoder")):
                raise ValueError("Shortlist: %s is not a model of this package" % type(m).__name__)
        if not isinstance(lexicon, Lexicon):
            raise ValueError("Shortlist: lexicon must be a shortlist.Lexicon")
        V, Vs = int(models[0].tgt_size), int(models[0].src_size)
        for m in models:
            d = m.decoder
            if int(m.tgt_size) != V or d.out.bias.shape[0] != V or d.embedding.weight.shape[0] != V:
                raise ValueError("Shortlist: the members disagree on the target vocabulary")
            for t in (d.embedding.weight, d.out.weight, d.out.bias):
                if t.dtype != torch.float32:
                    raise NotImplementedError("Shortlist: 2-byte storage (%s) is not supported: the gathers copy fp32 rows" % t.dtype)
        if lexicon.Vt != V or lexicon.Vs > Vs:
            raise ValueError("Shortlist: the lexicon is for vocabularies (%d, %d), the model's are (%d, %d)"
                             % (lexicon.Vs, lexicon.Vt, Vs, V))
        if always is None:
            always = np.arange(min(V, N_SPECIAL + max(0, int(first))), dtype=np.int64)
        always = np.asarray(always, dtype=np.int64).reshape(-1)
        if len(always) and (int(always.min()) < 0 or int(always.max()) >= V):
            raise ValueError("Shortlist: `always` holds ids outside [0, %d)" % V)
        if not set(range(N_SPECIAL)) <= set(always.tolist()):
            raise ValueError("Shortlist: `always` must hold PAD, UNK, SOS and EOS (0 .. 3)")
        self.best = int(min(int(best), lexicon.K))
        if self.best < 0:
            raise ValueError("Shortlist: best must be >= 0")
        self.n_always = int(len(np.unique(always)))
        cap = default_capacity(V, len(always), self.best) if capacity is None else int(capacity)
        if not (8 <= cap <= V) or len(always) > cap or V > MAX_V:
            raise ValueError("Shortlist: need 8 <= capacity <= V = %d <= %d and len(always) = %d <= capacity, got capacity %d"
                             % (V, MAX_V, len(always), cap))
        dev = next(models[0].parameters()).device
        if dev.type != "cuda":
            raise ValueError("Shortlist: the model must be on the GPU (there is no CPU path)")
        if not _lib.lib().vag_shortlist_supported(V, lexicon.Vs, lexicon.K, cap):
            raise ValueError("Shortlist: sizes outside the kernels' limits (V %d, K %d, capacity %d)" % (V, lexicon.K, cap))
        self.obj, self.models, self.multimodal = obj, models, multimodal
        self.lexicon = lexicon.to(dev) if lexicon.device_table is None or lexicon.device_table.device != dev else lexicon
        self.V, self.capacity, self.device = V, cap, dev
        self.always = torch.from_numpy(always.astype(np.int32)).to(dev)
        self.ids = torch.full((cap,), -1, dtype=I32, device=dev)
        self.full2short = torch.full((V,), -1, dtype=I32, device=dev)
        self._counts = torch.zeros(4, dtype=I32, device=dev)             # n, rank_used | coverage: absent, words
        self.views = [_member_view(m, cap, self.n_always) for m in models]
        if isinstance(obj, Ensemble):
            self.view = _EnsembleView(self.views)
            self.view._shortlist_always = self.n_always
        else:
            self.view = self.views[0]
        self._serial = 0
        self._host = None
        self.last = None

    # ---------------------------------------------------------------------------------------------- selection
    def select(self, src_var, src_lengths):
        """The shortlist of this batch into the views: select, gathers, version bump.  Returns Selection(n (1,), rank_used (1,),
        ids (capacity,)) as device tensors (views of the object's own buffers: the next select overwrites them); no host read."""
        if not torch.is_tensor(src_var) or not src_var.is_cuda:
            raise ValueError("Shortlist: src_var must be a GPU tensor (there is no CPU path)")
        if src_var.dim() != 2 or src_var.dtype != I64:
            raise ValueError("Shortlist: src_var must be (B, Ts) int64")
        src = src_var.contiguous()
        lens = lengths_tensor(src_lengths, src.device)
        lex = self.lexicon
        n, used = self._counts[0:1], self._counts[1:2]
        s = stream()
        call("vag_shortlist_select", ptr(src, I64), ptr(lens, I32), src.shape[0], src.shape[1], ptr(lex.device_table, I32), lex.Vs,
             lex.K, self.best, ptr(self.always, I32), self.always.shape[0], self.V, self.capacity, ptr(self.ids, I32), ptr(n, I32),
             ptr(used, I32), ptr(self.full2short, I32), s)
        self._serial += 1
        for m, v in zip(self.models, self.views):
            d, dv = m.decoder, v.decoder
            pairs = [(d.embedding.weight, dv.embedding.weight, 0.0), (d.out.bias, dv.out.bias, PAD_BIAS)]
            if dv.out.weight is not dv.embedding.weight:
                pairs.append((d.out.weight, dv.out.weight, 0.0))
            for full, short, pad in pairs:
                full = full.detach()
                W = 1 if full.dim() == 1 else full.shape[1]
                call("vag_shortlist_gather", ptr(self.ids, I32), ptr(n, I32), self.capacity, ptr(full), self.V, W, W, pad,
                     ptr(short.detach()), s)
            # _decode_weights compares this for equality: the member's own version, and the selection's number
            v._vag_weights_version = (getattr(m, "_vag_weights_version", 0), self._serial)
            for a in _DECODE_SWITCHES:
                setattr(v, a, getattr(m, a))
            v.training = dv.training = m.training
        if self.view is not self.views[0]:
            self.view.decode_graph = self.obj.decode_graph
        self._host = None
        self.last = Selection(n, used, self.ids)
        return self.last

    def _tables(self):
        """(ids, full2short) of the last selection on the host: one read per selection, made when token LISTS are mapped."""
        if self.last is None:
            raise ValueError("Shortlist: nothing selected yet (call select, or one of the decoding methods)")
        if self._host is None:
            self._host = (self.ids.cpu().numpy(), self.full2short.cpu().numpy())
        return self._host

    # ---------------------------------------------------------------------------------------------- id maps
    def _map_tensor(self, x, to_short, absent=None):
        if not x.is_cuda:
            raise ValueError("Shortlist: token tensors must be on the GPU (there is no CPU path)")
        if x.dtype != I64:
            raise ValueError("Shortlist: token tensors must be int64, got %s" % x.dtype)
        x = x.contiguous()
        out = torch.empty_like(x)
        table = self.full2short if to_short else self.ids
        call("vag_shortlist_map", ptr(x, I64), x.numel(), ptr(table, I32), table.shape[0], 1 if to_short else 0, ptr(out, I64),
             ptr(absent, I32) if absent is not None else None, stream())
        return out

    def _map(self, x, to_short, absent=None):
        if torch.is_tensor(x):
            return self._map_tensor(x, to_short, absent)
        if isinstance(x, tuple) and hasattr(x, "_fields"):
            return type(x)(*[self._map(v, to_short, absent) if f in TOKEN_FIELDS or (isinstance(v, tuple) and hasattr(v, "_fields"))
                             else v for f, v in zip(x._fields, x)])
        if isinstance(x, tuple):
            return tuple(self._map(v, to_short, absent) if isinstance(v, (list, tuple)) else v for v in x)
        if isinstance(x, list):
            return [self._map(v, to_short, absent) for v in x]
        if x is None:
            return None
        ids, f2s = self._tables()
        table = f2s if to_short else ids
        w = int(x)
        m = int(table[w]) if 0 <= w < len(table) else -1
        return m if m >= 0 else UNK_token

    def to_short(self, x, absent=None):
        """Full ids -> the last selection's compact ids; a word outside the shortlist becomes UNK.  x: an int64 GPU tensor of any
        shape (mapped on the device; absent: an int32 (1,) device counter that receives the number of such words), token lists
        nested to any depth (mapped on the host, one read per selection), or a search's named tuple (its word fields)."""
        return self._map(x, True, absent)

    def to_full(self, x):
        """Compact ids of the last selection -> full ids; x as for to_short.  In a plain tuple (beamsearch_nbest's (hyps, scores))
        the lists and named tuples are mapped and tensors pass through; pass a token tensor on its own."""
        return self._map(x, False)

    # ---------------------------------------------------------------------------------------------- decoding
    def _run(self, name, src_var, src_lengths, args, kwargs):
        self.select(src_var, src_lengths)
        return self.to_full(getattr(self.view, name)(src_var, src_lengths, *args, **kwargs))

    def beamsearch_decode(self, src_var, src_lengths, *args, device_rows=False, **kwargs):
        """The wrapped object's beamsearch_decode (its signature) over the batch's shortlist, in full ids.  device_rows=True: the
        search's (B, tgt_l) int64 rows as a GPU tensor instead of the cut lists, mapped on the device."""
        if not device_rows:
            return self._run("beamsearch_decode", src_var, src_lengths, args, kwargs)
        b = inspect.signature(self.view.beamsearch_decode).bind(src_var, src_lengths, *args, **kwargs)
        b.apply_defaults()
        a = b.arguments
        self.select(src_var, src_lengths)
        if int(a["beam_size"]) > 1:
            check_beam_width(a["beam_size"], self.n_always, "beamsearch_decode")
        return self.to_full(self.view._decode(src_var, src_lengths, a.get("im_var"), a["beam_size"], a["max_length"], a["tgt_var"],
                                              device_rows=True))

    def beamsearch_nbest(self, src_var, src_lengths, *args, **kwargs):
        """The wrapped object's beamsearch_nbest over the batch's shortlist: (hyps in full ids, scores renormalised over it)."""
        return self._run("beamsearch_nbest", src_var, src_lengths, args, kwargs)

    def sample_decode(self, src_var, src_lengths, *args, **kwargs):
        """The wrapped object's sample_decode over the batch's shortlist (generator=None: the view's own generator)."""
        return self._run("sample_decode", src_var, src_lengths, args, kwargs)

    def score_translations(self, src_var, src_lengths, tgt, im_var=None):
        """Forced decoding under the view: ShortScores(score, logp, token_logp, absent).  tgt in full ids (as for a model's
        score_translations); a word outside the batch's shortlist is scored as UNK and counted in absent, an int32 (1,) device
        tensor (no host read)."""
        if not torch.is_tensor(src_var) or not src_var.is_cuda:
            raise ValueError("Shortlist: src_var must be a GPU tensor (there is no CPU path)")
        self.select(src_var, src_lengths)
        tgt = scoring.targets_tensor(tgt, src_var.shape[0], src_var.device)
        absent = torch.zeros(1, dtype=I32, device=src_var.device)
        short = self.to_short(tgt, absent)
        if self.view is self.views[0] and not self.multimodal[0]:
            s = self.view.score_translations(src_var, src_lengths, short)
        else:
            s = self.view.score_translations(src_var, src_lengths, short, im_var)
        return ShortScores(s.score, s.logp, s.token_logp, absent)

    def coverage(self, batches):
        """The share of reference target words (non-pad) that lie inside their batch's shortlist, over ``batches`` of
        (src_var, src_lengths, tgt): counted on the device, read once at the end."""
        absent, words = self._counts[2:3], self._counts[3:4]
        self._counts[2:4].zero_()
        for batch in batches:
            src_var, src_lengths, tgt = batch[0], batch[1], batch[2]
            self.select(src_var, src_lengths)
            tgt = scoring.targets_tensor(tgt, src_var.shape[0], src_var.device)
            self.to_short(tgt, absent)
            words += (tgt != 0).sum().to(I32)
        a, w = [int(v) for v in self._counts[2:4].cpu()]
        return 1.0 - a / max(1, w)
