"""Shallow fusion (Gulcehre et al. 2015) with a back-off n-gram language model: target-side monolingual text steers beam search
and forced scoring,

    score(w | hyp) = logp_model(w | hyp) + beta * ln p_LM(w | the last order-1 words of hyp)         (not renormalised)

    lm = NgramLM.train(sentences, V, order=3)            # interpolated Kneser-Ney on the host, seconds for 30 k sentences
    lm = NgramLM.from_arpa("kenlm.arpa", word_to_id, V)  # or a model trained elsewhere
    r = model.beamsearch_lm(src_var, src_lengths, im_var, lm, beta=0.3, beam_size=12, n_best=1)     # LmSearch(hyps, scores)
    s = lm_score_translations(model, src_var, src_lengths, tgt, im_var, lm, beta=0.3)               # scoring.Scores
    lm.token_logp(tgt), lm.perplexity(batches)                                                      # the LM alone
    lm_tune(model, lm, dev_batches, betas=[0.0, 0.1, 0.3])                                          # corpus BLEU per beta

The model is held in ARPA's semantics (include/vag_nmt.h: vag_lm): a stored n-gram has logp and, below the top order, a back-off
weight; lm(w | c_L..c_1) is logp(c_L..c_1 w) where stored, otherwise bo(c_L..c_1) (0 for a context that is not stored) plus
lm(w | c_{L-1}..c_1).  On the device it is a forward trie in flat arrays inside ONE buffer, with a host mirror; the constructor
validates the trie, so the kernels can trust it.  A search step pays one vag_lm_fuse_beam launch after the members' steps (and
after kNN's place) and before the constraints' mask, so a ban still wins; on an Ensemble the one LM is added to every member's
row, which commutes with the log-mean.

Limits: order 2 .. 5, V <= 131072, fewer than 2^31 n-grams per order, beta finite (0: nothing is launched and the result is
beamsearch_nbest / score_translations bit for bit).  Not here: fusion in the sampling, diverse, required, stochastic and
penalised searches, kNN and LM in one search, a neural LM, renormalised fusion, any effect on training."""
import ctypes as C
import math
import time
from collections import namedtuple

import numpy as np
import torch

from vagnmt_hip import _lib, constrain, knn, scoring, search
from vagnmt_hip._lib import call, ptr, stream
from vagnmt_hip.search import _p64, _pp

MAX_ORDER = 5           # VAG_LM_MAX_ORDER (include/vag_nmt.h)
MAX_V = 131072          # VAG_LM_MAX_V: the kernel's claimed-word bitmap
UNK, SOS, EOS = 1, 2, 3
LN10 = math.log(10.0)

I32, I64 = torch.int32, torch.int64

LmSearch = namedtuple("LmSearch", ["hyps", "scores"])


# ------------------------------------------------------------------------------------------------------- rows of n-grams
def _unique_rows(rows):
    """Distinct rows of an (N, n) integer array in lexicographic order, and how often each occurs."""
    if rows.shape[0] == 0:
        return rows, np.zeros(0, dtype=np.int64)
    order = np.lexsort(rows.T[::-1])
    rows = rows[order]
    new = np.ones(rows.shape[0], dtype=bool)
    new[1:] = np.any(rows[1:] != rows[:-1], axis=1)
    start = np.flatnonzero(new)
    return rows[start], np.diff(np.append(start, rows.shape[0]))


def _match_rows(table, queries):
    """Index in ``table`` (distinct rows) of every row of ``queries``, -1 where the table does not hold it."""
    nt, nq = table.shape[0], queries.shape[0]
    if nq == 0 or nt == 0:
        return np.full(nq, -1, dtype=np.int64)
    both = np.concatenate([table, queries])
    src = np.concatenate([np.arange(nt), np.full(nq, nt, dtype=np.int64)])      # a table row sorts before its queries
    order = np.lexsort((src,) + tuple(both.T[::-1]))
    both, src = both[order], src[order]
    new = np.ones(nt + nq, dtype=bool)
    new[1:] = np.any(both[1:] != both[:-1], axis=1)
    group = np.cumsum(new) - 1
    head = np.full(group[-1] + 1, -1, dtype=np.int64)                          # the table row that opens a group, if one does
    first = np.flatnonzero(new)
    head[group[first]] = np.where(src[first] < nt, src[first], -1)
    out = np.empty(nt + nq, dtype=np.int64)
    out[order] = head[group]
    return out[nt:]


def _discount(counts):
    n1, n2 = int(np.sum(counts == 1)), int(np.sum(counts == 2))
    return n1 / (n1 + 2.0 * n2) if n1 and n2 else 0.5


def _sentences(sentences):
    """Token lists, or a (N, L) integer tensor / array padded with 0 -> (flat tokens with SOS / EOS added, sentence index)."""
    if torch.is_tensor(sentences):
        sentences = sentences.cpu().numpy()
    if isinstance(sentences, np.ndarray):
        if sentences.ndim != 2:
            raise ValueError("NgramLM.train: a tensor of sentences must be (N, L)")
        N, L = sentences.shape
        body = sentences != 0
        lens = body.sum(1)
        if np.any(body != (np.arange(L)[None, :] < lens[:, None])):
            raise ValueError("NgramLM.train: the padding (0) must follow the words")
        tok = np.full((N, L + 2), -1, dtype=np.int64)
        tok[:, 0] = SOS
        tok[:, 1:L + 1] = np.where(body, sentences, -1)
        tok[np.arange(N), lens + 1] = EOS
        keep = tok >= 0
        return tok[keep], np.broadcast_to(np.arange(N)[:, None], tok.shape)[keep]
    lens = np.fromiter((len(s) + 2 for s in sentences), dtype=np.int64)
    tok = np.empty(int(lens.sum()), dtype=np.int64)
    at = 0
    for s, n in zip(sentences, lens):
        tok[at] = SOS
        tok[at + 1:at + n - 1] = s
        tok[at + n - 1] = EOS
        at += n
    return tok, np.repeat(np.arange(len(lens)), lens)


class NgramLM:
    """A back-off n-gram model of order 2 .. 5 over the ids [0, V): <s> = 2, </s> = 3, <unk> = 1.

    ``levels[l]`` (l = n - 1) holds the n-grams as float64 / int32 host arrays: level 0 is indexed by the word (logp, bo, child);
    level l >= 1 has word, logp and, below the top order, bo and child -- the successors of node i of level l are the entries
    [child[i], child[i+1]) of level l+1, ascending by word.  The constructor validates all of it (ValueError) and packs the fp32 /
    int32 image the kernels read into one buffer (``host``); ``to(device)`` puts that buffer on a GPU."""

    def __init__(self, order, V, levels):
        order, V = int(order), int(V)
        if not 2 <= order <= MAX_ORDER:
            raise ValueError("NgramLM: the order must lie in [2, %d], got %d" % (MAX_ORDER, order))
        if not 4 <= V <= MAX_V:
            raise ValueError("NgramLM: V must lie in [4, %d], got %d" % (MAX_V, V))
        if len(levels) != order:
            raise ValueError("NgramLM: %d levels for order %d" % (len(levels), order))
        self.order, self.V = order, V
        self.levels = []
        for l, lv in enumerate(levels):
            top = l == order - 1
            d = {"logp": np.ascontiguousarray(lv["logp"], dtype=np.float64)}
            if l >= 1:
                d["word"] = np.ascontiguousarray(lv["word"], dtype=np.int64)
            if not top:
                d["bo"] = np.ascontiguousarray(lv["bo"], dtype=np.float64)
                d["child"] = np.ascontiguousarray(lv["child"], dtype=np.int64)
            self.levels.append(d)
        self._validate()
        self._pack()
        self._dev = None

    # ------------------------------------------------------------------------------------------------------- validation
    def _validate(self):
        V = self.V
        for l, d in enumerate(self.levels):
            n = V if l == 0 else d["word"].shape[0]
            name = "level %d" % (l + 1)
            if n >= 1 << 31:
                raise ValueError("NgramLM: %s holds 2^31 n-grams or more" % name)
            if d["logp"].shape != (n,) or ("bo" in d and d["bo"].shape != (n,)) or ("child" in d and d["child"].shape != (n + 1,)) \
                    or (l >= 1 and d["word"].ndim != 1):
                raise ValueError("NgramLM: %s: array lengths do not agree (%d entries)" % (name, n))
            if not np.all(np.isfinite(d["logp"])) or ("bo" in d and not np.all(np.isfinite(d["bo"]))):
                raise ValueError("NgramLM: %s: a value is not finite" % name)
            if np.any(np.abs(d["logp"]) > 3e38) or ("bo" in d and np.any(np.abs(d["bo"]) > 3e38)):
                raise ValueError("NgramLM: %s: a value does not fit fp32" % name)
            if l >= 1 and n and (d["word"].min() < 0 or d["word"].max() >= V):
                raise ValueError("NgramLM: %s: a word lies outside [0, %d)" % (name, V))
            if "child" in d:
                c = d["child"]
                nxt = self.levels[l + 1]["word"].shape[0]
                if c[0] != 0 or c[-1] != nxt or np.any(np.diff(c) < 0):
                    raise ValueError("NgramLM: %s: the child ranges are not monotone from 0 to the next level's %d entries" % (name, nxt))
                w = self.levels[l + 1]["word"]
                if nxt > 1:
                    inner = np.ones(nxt, dtype=bool)                    # entries that do not open a parent's range
                    inner[c[:-1][c[:-1] < nxt]] = False
                    if np.any(inner[1:] & (w[1:] <= w[:-1])):
                        raise ValueError("NgramLM: level %d: a node's successors are not ascending and distinct" % (l + 2))

    # ---------------------------------------------------------------------------------------------------------- packing
    def _pack(self):
        """The device image: every array as fp32 / int32 in one buffer of 4-byte words, each array on a 16-byte boundary."""
        parts, self._offsets, at = [], [], 0
        for l, d in enumerate(self.levels):
            off = {}
            for name in ("word", "logp", "bo", "child"):
                if name not in d:
                    continue
                a = d[name].astype(np.float32).view(np.int32) if name in ("logp", "bo") else d[name].astype(np.int32)
                pad = (-a.shape[0]) % 4
                off[name] = at
                parts += [a, np.zeros(pad, dtype=np.int32)]
                at += a.shape[0] + pad
            self._offsets.append(off)
        self.host = np.concatenate(parts + [np.zeros(4, dtype=np.int32)])      # (never empty: an empty level still has an address)

    def host_array(self, level, name):
        """The fp32 / int32 array the kernels read, as a view of the host mirror."""
        n = self.counts[level] + (1 if name == "child" else 0)
        a = self.host[self._offsets[level][name]:self._offsets[level][name] + n]
        return a.view(np.float32) if name in ("logp", "bo") else a

    @property
    def counts(self):
        return [self.V] + [d["word"].shape[0] for d in self.levels[1:]]

    def to(self, device):
        """Puts the buffer on ``device`` (once per device; another device replaces it) and returns self."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev.device != device:
            self._dev = torch.from_numpy(self.host).to(device)
            self._struct = None
        return self

    @property
    def buffer(self):
        if self._dev is None:
            raise _lib.VagError("NgramLM: the model is not on a GPU yet (lm.to(device))")
        return self._dev

    def struct(self):
        """The vag_lm of the device buffer (ctypes; the library reads it while a call enqueues)."""
        if getattr(self, "_struct", None) is None:
            base, s = self.buffer.data_ptr(), _lib.Lm()
            s.order, s.V = self.order, self.V
            for l, off in enumerate(self._offsets):
                s.count[l] = self.counts[l]
                for name in ("word", "logp", "bo", "child"):
                    if name in off:
                        getattr(s, name)[l] = base + 4 * off[name]
            self._struct = s
        return self._struct

    def identity(self):
        """What a captured launch holds of this model, by pointer and by value: part of the graph keys."""
        return (self.buffer.data_ptr(), self.order, self.V) + tuple(self.counts)

    # ------------------------------------------------------------------------------------------------- host-side lookup
    def rows(self, level):
        """The n-grams of a level as a (count, level+1) int64 array, in the trie's order."""
        if level == 0:
            return np.arange(self.V, dtype=np.int64)[:, None]
        prev = self.rows(level - 1)
        parent = np.repeat(np.arange(prev.shape[0]), np.diff(self.levels[level - 1]["child"]))
        return np.concatenate([prev[parent], self.levels[level]["word"][:, None]], axis=1)

    def _node(self, words):
        """Trie node of an n-gram (a tuple of ids, oldest first) at level len(words)-1, or -1."""
        node = int(words[0])
        for l, w in enumerate(words[1:]):
            c = self.levels[l]["child"]
            lo, hi = int(c[node]), int(c[node + 1])
            seg = self.levels[l + 1]["word"][lo:hi]
            i = int(np.searchsorted(seg, w))
            if i >= seg.shape[0] or seg[i] != w:
                return -1
            node = lo + i
        return node

    def logprob(self, word, context=()):
        """(lm(word | context), matched order) in float64 on the host; context: ids, oldest first (the last order-1 count)."""
        ctx = [int(c) for c in context][-(self.order - 1):]
        for i in range(len(ctx) - 1, -1, -1):                       # a word outside the vocabulary ends the context
            if not 0 <= ctx[i] < self.V:
                ctx = ctx[i + 1:]
                break
        total = 0.0
        while ctx:
            node = self._node(ctx)
            if node >= 0:
                hit = self._node(ctx + [int(word)])
                if hit >= 0:
                    return total + float(self.levels[len(ctx)]["logp"][hit]), len(ctx) + 1
                total += float(self.levels[len(ctx) - 1]["bo"][node])
            ctx = ctx[1:]
        return total + float(self.levels[0]["logp"][int(word)]), 1

    # --------------------------------------------------------------------------------------------------------- building
    @classmethod
    def from_ngrams(cls, order, V, uni_logp, uni_bo, rows, logp, bo):
        """The model from its n-grams: uni_logp / uni_bo (V,), and for every order n = 2 .. order rows[n-2] (N_n, n) ids, logp[n-2]
        (N_n,) and -- below the top order -- bo[n-2] (N_n,), in any order, natural logs.  An n-gram whose first n-1 words are not
        stored one level down is dropped (a trie cannot hold it)."""
        levels = [{"logp": np.asarray(uni_logp, dtype=np.float64), "bo": np.asarray(uni_bo, dtype=np.float64)}]
        prev = np.arange(V, dtype=np.int64)[:, None]
        for n in range(2, order + 1):
            r = np.asarray(rows[n - 2], dtype=np.int64).reshape(-1, n)
            lp = np.asarray(logp[n - 2], dtype=np.float64)
            b = np.asarray(bo[n - 2], dtype=np.float64) if n < order else None
            o = np.lexsort(r.T[::-1]) if r.shape[0] else np.zeros(0, dtype=np.int64)
            r, lp = r[o], lp[o]
            b = b[o] if b is not None else None
            if r.shape[0] > 1 and np.any(np.all(r[1:] == r[:-1], axis=1)):
                raise ValueError("NgramLM: an n-gram of order %d is given twice" % n)
            parent = _match_rows(prev, r[:, :-1])
            keep = parent >= 0
            r, lp, parent = r[keep], lp[keep], parent[keep]
            levels[-1]["child"] = np.searchsorted(parent, np.arange(prev.shape[0] + 1))
            lv = {"word": r[:, -1], "logp": lp}
            if b is not None:
                lv["bo"] = b[keep]
            levels.append(lv)
            prev = r
        return cls(order, V, levels)

    @classmethod
    def train(cls, sentences, V, order=3):
        """Interpolated Kneser-Ney from sentences of target ids (token lists, or a (N, L) int64 tensor padded with 0; SOS is
        prepended and EOS appended).  The top order uses the counts, every lower order continuation counts -- the number of
        distinct words seen before the n-gram; an n-gram that opens with SOS has no predecessor and keeps its count; SOS itself is
        never predicted -- with one discount per order D_n = n1 / (n1 + 2 n2) (0.5 where n1 or n2 is 0):
            p_n(w | h) = max(c(h w) - D_n, 0) / c(h) + gamma(h) p_{n-1}(w | h'),   gamma(h) = D_n N1+(h .) / c(h),
        the unigram level interpolated with the uniform 1/V, so no word has probability 0.  In back-off form logp(h w) is the
        interpolated value and bo(h) = ln gamma(h): sum_w exp(lm(w | ctx)) = 1 for every context, seen or not."""
        order, V = int(order), int(V)
        if not 2 <= order <= MAX_ORDER:
            raise ValueError("NgramLM.train: the order must lie in [2, %d], got %d" % (MAX_ORDER, order))
        t0 = time.perf_counter()
        tok, sent = _sentences(sentences)
        if tok.size and (tok.min() < 0 or tok.max() >= V):
            raise ValueError("NgramLM.train: a word lies outside [0, %d)" % V)
        body = np.ones(tok.shape[0], dtype=bool)
        body[np.flatnonzero(np.diff(sent, prepend=-1) != 0)] = False         # the added SOS
        if np.any(tok[body] == SOS):
            raise ValueError("NgramLM.train: SOS (%d) inside a sentence" % SOS)
        raw = []                                                             # per order: distinct n-grams and their counts
        for n in range(1, order + 1):
            m = tok.shape[0] - n + 1
            if m <= 0:
                raw.append((np.zeros((0, n), dtype=np.int64), np.zeros(0, dtype=np.int64)))
                continue
            ok = sent[:m] == sent[n - 1:]
            raw.append(_unique_rows(np.stack([tok[i:i + m][ok] for i in range(n)], axis=1)))
        adj = [None] * order                                                 # the counts each order is estimated from
        adj[order - 1] = raw[order - 1]
        for n in range(order - 1, 0, -1):
            cont = _unique_rows(raw[n][0][:, 1:])                            # distinct predecessors of every n-gram that has one
            first = raw[n - 1][0][:, 0] == SOS
            if n == 1:
                first[:] = False                                             # (SOS is not an event: nothing predicts it)
            rows = np.concatenate([cont[0], raw[n - 1][0][first]])
            cnt = np.concatenate([cont[1], raw[n - 1][1][first]])
            o = np.lexsort(rows.T[::-1]) if rows.shape[0] else np.zeros(0, dtype=np.int64)
            adj[n - 1] = (rows[o], cnt[o])
        # unigrams
        c1 = np.zeros(V, dtype=np.float64)
        c1[adj[0][0][:, 0]] = adj[0][1]
        total = c1.sum()
        if total > 0:
            D = _discount(adj[0][1])
            p = np.maximum(c1 - D, 0.0) / total + D * np.count_nonzero(c1) / total / V
        else:
            p = np.full(V, 1.0 / V)
        tables = [(np.arange(V, dtype=np.int64)[:, None], p)]                # per order: rows (sorted) and probabilities
        uni_bo = np.zeros(V, dtype=np.float64)
        bos, logps, rows_out = [], [], []
        for n in range(2, order + 1):
            rows, cnt = adj[n - 1]
            cnt = cnt.astype(np.float64)
            if rows.shape[0]:
                new = np.ones(rows.shape[0], dtype=bool)
                new[1:] = np.any(rows[1:, :-1] != rows[:-1, :-1], axis=1)
                start = np.flatnonzero(new)
                size = np.diff(np.append(start, rows.shape[0]))
                ctot = np.add.reduceat(cnt, start)
                D = _discount(adj[n - 1][1])
                gamma = D * size / ctot
                g = np.cumsum(new) - 1
                low_rows, low_p = tables[-1]
                at = _match_rows(low_rows, rows[:, 1:])
                assert np.all(at >= 0)                                       # (h w) seen => (h' w) has a predecessor
                p = (cnt - D) / ctot[g] + gamma[g] * low_p[at]
                ctx_at = _match_rows(low_rows, rows[start][:, :-1])
                assert np.all(ctx_at >= 0)
            else:
                p, gamma, ctx_at = np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64)
            if n == 2:
                uni_bo[ctx_at] = np.log(gamma)
            else:
                bos[-1][ctx_at] = np.log(gamma)
            tables.append((rows, p))
            rows_out.append(rows)
            logps.append(np.log(p))
            if n < order:
                bos.append(np.zeros(rows.shape[0], dtype=np.float64))
        lm = cls.from_ngrams(order, V, np.log(tables[0][1]), uni_bo, rows_out, logps, bos)
        lm.train_seconds = time.perf_counter() - t0
        return lm

    # ------------------------------------------------------------------------------------------------------------ files
    @classmethod
    def from_arpa(cls, path, word_to_id, V):
        """Reads plain ARPA text (log10 -> natural log).  word_to_id: a dict from the file's words to ids (``<s>``, ``</s>`` and
        ``<unk>`` map to 2, 3 and 1 unless the dict says otherwise).  An n-gram holding a word the dict does not know is
        dropped; an id no unigram covers gets <unk>'s value (ValueError if the file has no <unk> then)."""
        ids = {"<s>": SOS, "</s>": EOS, "<unk>": UNK}
        ids.update(word_to_id)
        grams, n = {}, 0
        with open(path, encoding="utf-8") as f:
            for line in f:
                line = line.strip()
                if not line or line.startswith("ngram ") or line == "\\data\\":
                    continue
                if line == "\\end\\":
                    break
                if line.startswith("\\") and line.endswith("-grams:"):
                    n = int(line[1:line.index("-")])
                    grams[n] = []
                    continue
                if n == 0:
                    continue
                parts = line.split()
                if len(parts) not in (n + 1, n + 2):
                    raise ValueError("NgramLM.from_arpa: cannot read %r as a %d-gram" % (line, n))
                words = parts[1:n + 1]
                if all(w in ids for w in words):
                    grams[n].append(([ids[w] for w in words], float(parts[0]) * LN10,
                                     float(parts[n + 1]) * LN10 if len(parts) == n + 2 else 0.0))
        order = max(grams) if grams else 0
        if not 2 <= order <= MAX_ORDER or sorted(grams) != list(range(1, order + 1)):
            raise ValueError("NgramLM.from_arpa: %s holds the orders %s; need 1 .. n with n in [2, %d]" % (path, sorted(grams), MAX_ORDER))
        uni_logp, uni_bo = np.full(V, np.nan), np.zeros(V)
        for w, lp, b in grams[1]:
            if 0 <= w[0] < V:
                uni_logp[w[0]], uni_bo[w[0]] = lp, b
        if np.any(np.isnan(uni_logp)):
            if np.isnan(uni_logp[UNK]):
                raise ValueError("NgramLM.from_arpa: %s covers neither every id nor <unk>" % path)
            uni_logp[np.isnan(uni_logp)] = uni_logp[UNK]
        uni_logp = np.maximum(uni_logp, -99.0 * LN10)                        # (ARPA's -99 for <s> stays finite in fp32)
        rows, logp, bo = [], [], []
        for n in range(2, order + 1):
            g = [x for x in grams[n] if all(0 <= w < V for w in x[0])]
            rows.append(np.array([x[0] for x in g], dtype=np.int64).reshape(-1, n))
            logp.append(np.array([x[1] for x in g], dtype=np.float64))
            if n < order:
                bo.append(np.array([x[2] for x in g], dtype=np.float64))
        return cls.from_ngrams(order, V, uni_logp, uni_bo, rows, logp, bo)

    def to_arpa(self, path, id_to_word=None):
        """Writes plain ARPA text (natural log -> log10, 17 significant digits).  id_to_word: a dict or list from ids to words;
        ids it does not hold are written as ``<id>``; 1, 2, 3 default to <unk>, <s>, </s>."""
        names = {UNK: "<unk>", SOS: "<s>", EOS: "</s>"}
        if id_to_word is not None:
            names.update(id_to_word.items() if hasattr(id_to_word, "items") else enumerate(id_to_word))
        word = lambda i: names.get(int(i), "<%d>" % int(i))                  # noqa: E731
        with open(path, "w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for l, c in enumerate(self.counts):
                f.write("ngram %d=%d\n" % (l + 1, c))
            for l, d in enumerate(self.levels):
                f.write("\n\\%d-grams:\n" % (l + 1))
                rows = self.rows(l)
                for i in range(rows.shape[0]):
                    line = "%.17g\t%s" % (d["logp"][i] / LN10, " ".join(word(w) for w in rows[i]))
                    if "bo" in d:
                        line += "\t%.17g" % (d["bo"][i] / LN10)
                    f.write(line + "\n")
            f.write("\n\\end\\\n")

    def save(self, path):
        arrays = {"order": np.int64(self.order), "V": np.int64(self.V)}
        for l, d in enumerate(self.levels):
            for name, a in d.items():
                arrays["%s%d" % (name, l)] = a
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            order = int(z["order"])
            levels = [{name: z["%s%d" % (name, l)] for name in ("word", "logp", "bo", "child") if "%s%d" % (name, l) in z.files}
                      for l in range(order)]
            return cls(order, int(z["V"]), levels)

    # ------------------------------------------------------------------------------------------------- LM-only scoring
    def contexts(self, inputs):
        """(B, T, order-1) int32 contexts of the positions of decoder inputs (B, T) -- position t sees inputs[t-order+2 .. t], -1
        before the first -- formed on the inputs' device."""
        B, T = inputs.shape
        n = self.order - 1
        pad = torch.full((B, n - 1), -1, dtype=inputs.dtype, device=inputs.device)
        return torch.cat([pad, inputs], 1).unfold(1, n, 1).to(I32).contiguous()

    def query(self, ctx, word):
        """vag_lm_query: ctx (R, order-1) int32, word (R,) int32 on the model's device -> (logp (R,) fp32, order (R,) int32)."""
        R = word.shape[0]
        if tuple(ctx.shape) != (R, self.order - 1):
            raise ValueError("NgramLM.query: ctx must be (%d, %d), got %s" % (R, self.order - 1, tuple(ctx.shape)))
        logp = torch.empty(R, device=word.device)
        matched = torch.empty(R, dtype=I32, device=word.device)
        call("vag_lm_query", C.byref(self.struct()), ptr(ctx, I32), ptr(word, I32), R, ptr(logp), ptr(matched, I32), stream())
        return logp, matched

    def token_logp(self, tgt):
        """ln p_LM of every target word given its predecessors: tgt (B, Tt) int64 on a GPU (pad 0) -> (B, Tt) fp32, 0 past the
        scored span (the first EOS, or the last non-pad word where there is none)."""
        if not torch.is_tensor(tgt) or tgt.dim() != 2 or tgt.dtype != I64 or not tgt.is_cuda:
            raise ValueError("NgramLM.token_logp: tgt must be a (B, Tt) int64 tensor on the GPU")
        self.to(tgt.device)
        B, Tt = tgt.shape
        sos = torch.full((B, 1), SOS, dtype=I64, device=tgt.device)
        ctx = self.contexts(torch.cat([sos, tgt[:, :-1]], 1))
        logp, _ = self.query(ctx.view(B * Tt, -1), tgt.reshape(-1).to(I32))
        pos = torch.arange(Tt, device=tgt.device)[None, :]
        eos, nz = tgt == EOS, tgt != 0
        end = torch.where(eos.any(1), torch.where(eos, pos, Tt).min(1)[0], torch.where(nz, pos, -1).max(1)[0])
        return torch.where(pos <= end[:, None], logp.view(B, Tt), torch.zeros((), device=tgt.device))

    def perplexity(self, batches):
        """exp(-sum ln p / words) over batches of (B, Tt) int64 targets on a GPU (each word of a scored span counts, EOS too)."""
        total, words = 0.0, 0
        for tgt in batches:
            total += float(self.token_logp(tgt).double().sum())
            words += int(knn.span_words(tgt))
        if words == 0:
            raise ValueError("NgramLM.perplexity: no words")
        return math.exp(-total / words)


# ------------------------------------------------------------------------------------------------------------- the search
def check_beta(beta, what="beamsearch_lm"):
    beta = float(beta)
    if not math.isfinite(beta):
        raise ValueError("%s: need a finite beta, got %r" % (what, beta))
    return beta


def graph_key(lm, beta):
    """Everything the captured launches of an LM search hold by value or by pointer: part of the graph entry's key."""
    return (float(beta),) + tuple(lm.identity())


class StepFuse:
    """What search.beam's ``lm=`` takes: ``rows`` enqueues one vag_lm_fuse_beam(_dev) on the rows the members just wrote.  Graph
    mode (entry given): the entry keeps the model alive -- the captured launches hold its pointers."""

    def __init__(self, lm, beta, entry=None):
        self.lm, self.beta = lm, beta
        if entry is not None:
            entry["lm_model"] = lm

    def rows(self, outs, beam, di, max_length, B, k, V, dev_form=False):
        call("vag_lm_fuse_beam_dev" if dev_form else "vag_lm_fuse_beam", _pp([o[1] for o in outs], None),
             _p64([o[1].shape[1] for o in outs]), len(outs), ptr(beam, I64), di, max_length, B, k, V, C.byref(self.lm.struct()),
             self.beta, stream())


def check_lm(lm, models, device, what):
    if not isinstance(lm, NgramLM):
        raise ValueError("%s: lm must be a vagnmt_hip.lm.NgramLM" % what)
    V = int(models[0].tgt_size)
    if lm.V != V:
        raise ValueError("%s: the language model covers %d ids, the model's vocabulary %d" % (what, lm.V, V))
    return lm.to(device)


def beamsearch_lm(obj, src_var, src_lengths, im_var, lm, beta=0.3, beam_size=12, n_best=1, max_length=80, avoid_double=True,
                  avoid_unk=False, prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0):
    """beamsearch_nbest under the fused score: LmSearch(hyps, scores); obj a model or an Ensemble (one LM, added to every member's
    row).  search.beam on the members' log-probability steps with ``lm=``: after the members' steps every row gets
    beta ln p_LM(. | its last order-1 words), then the constraints' mask (prefix / banned / banned_per_sentence /
    no_repeat_ngram as beamsearch_constrained takes them: a ban still wins), then the expansion.  The scores are the fused scores
    under the search's own length normalisation: what lm_score_translations gives for the returned words.  Graph mode keeps an
    entry of its own per (beta, the model's identity).  beta = 0 without constraints is beamsearch_nbest bit for bit."""
    what = "beamsearch_lm"
    models, mm = scoring.models_of(obj)
    beta = check_beta(beta, what)
    kb, n, flags = scoring.nbest_args(src_var, beam_size, n_best, avoid_double, avoid_unk, what)
    lm = check_lm(lm, models, src_var.device, what)
    ml, B, V = int(max_length), src_var.shape[0], int(models[0].tgt_size)
    packed = constrain.pack(B, V, ml, prefix, banned, banned_per_sentence, no_repeat_ngram, avoid_double, avoid_unk, what)
    packed = constrain.any_of(packed)
    if im_var is None and any(mm):
        raise ValueError("%s: a multimodal model needs im_var" % what)
    if beta == 0.0 and packed is None:          # IS beamsearch_nbest; with constraints nothing of the language model is enqueued either
        res = scoring.nbest_search(obj, src_var, src_lengths, im_var, kb, ml, flags, n)
    else:
        key = (("lm",) + graph_key(lm, beta)) if beta != 0.0 else ()
        with torch.no_grad():
            s = obj._search_setup(src_var, src_lengths, im_var, kb, ml, "beam_lm", flags, extra=constrain.graph_key(packed) + key)
            fuse = StepFuse(lm, beta, s.entry) if beta != 0.0 else None
            res = obj._search_done(search.beam(s.members, s.h0s, kb, ml, flags, n, s.entry, s.pool, raw_logits=False,
                                               constrain=constrain.on_device(packed, s, ml), lm=fuse), kb)
    return LmSearch(res[0], res[1])


def lm_score_translations(obj, src_var, src_lengths, tgt, im_var, lm, beta):
    """score_translations under the fused score: Scores(score (B,), logp (B,), token_logp (B, Tt)).  The members' forced logits,
    contexts formed from the decoder's inputs on the device, one vag_lm_fuse_rows on the logits, then the unchanged
    vag_forced_score with the rows' log-sum-exp: token_logp = logp_model + beta ln p_LM.  What the search's scores are checked
    against.  beta = 0 is score_translations bit for bit."""
    what = "lm_score_translations"
    models, mm = scoring.models_of(obj)
    beta = check_beta(beta, what)
    tgt, tok = scoring.forced_args(models, mm, src_var, tgt, im_var, what)
    lm = check_lm(lm, models, tgt.device, what)
    V = int(models[0].tgt_size)
    B, Tt = tgt.shape
    modes = [m.training for m in models]
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            outs = [knn.member_forced(m, src_var, src_lengths, im_var if h else None, tok, tgt) for m, h in zip(models, mm)]
            rows = [o[0] for o in outs]
            if beta != 0.0:
                ctx = lm.contexts(tok[:Tt].t()).permute(1, 0, 2).contiguous()              # time-major rows, as the logits
                call("vag_lm_fuse_rows", _pp(rows, None), _p64([r.shape[1] for r in rows]), len(rows), Tt * B, V, C.byref(lm.struct()),
                     ptr(ctx, I32), beta, stream())
            return knn._forced_score(rows, [o[1] for o in outs], tgt, V)
    finally:
        for m, tr in zip(models, modes):
            m.train(tr)


def lm_tune(obj, lm, dev_batches, betas, beam_size=12, max_length=80):
    """Corpus BLEU of the dev set per beta: dev_batches are (src_var, src_lengths, refs, im_var) with refs as
    validate.corpus_bleu takes them; the set is decoded once per beta (beam search, the best hypothesis) and scored by
    validate.BleuStats.  Returns a list of validate.CorpusBLEU, one per beta."""
    from vagnmt_hip import validate
    betas = [check_beta(b, "lm_tune") for b in betas]
    dev_batches = list(dev_batches)
    if not betas or not dev_batches:
        raise ValueError("lm_tune: no betas or no batches")
    out = []
    for beta in betas:
        stats = None
        for src_var, src_lengths, refs, im_var in dev_batches:
            r = beamsearch_lm(obj, src_var, src_lengths, im_var, lm, beta, beam_size, 1, max_length)
            if stats is None:
                stats = validate.BleuStats(src_var.device)
            stats.add([[int(t) for t in h[0]] for h in r.hyps], refs)
        out.append(stats.result())
    return out
