"""NumPy restatement of the constrained beam search as include/vag_nmt.h states it (vag_beam_constrain followed by
vag_beam_ens_step_opt): the yardstick of tests/test_constrain_host.py and tests/test_gpu_constrain.py.  No shortcut: a row's
history is walked back-pointer by back-pointer, every phrase and every position is looked at, the expansion ranks all k V
candidates under an explicit total order (score descending, flat index j V + w ascending) with float32 adds.

    history(beam, max_len, di, b, j)                       the words of row (b, j) before step di
    mask(rows, beam, di, max_len, B, k, V, ...)            vag_beam_constrain on copies of the M members' rows
    expand(lp, base, prev, k, flags)                       one sentence, one plain expansion (M = 1)
    search(fn, B, k, V, max_len, steps, ...)               a whole constrained search on logp = fn(previous words)
"""
import numpy as np

SOS, EOS, UNK = 2, 3, 1
NEG_PEN = np.float32(-1e5)
ALLOW_REPEAT, AVOID_UNK = 1, 2
MAX_LEN, MAX_PHRASES = 8, 256
F32 = np.float32
BRANCHES = ("forced", "unigram", "multiword", "finished")


def new_counts():
    """Rows each branch touched: forced / finished rows, rows with a one-word ban or a longer phrase's ban that applied (the
    word inside [0, V)), and per n the rows an n-gram ban applied to."""
    c = {name: 0 for name in BRANCHES}
    c["ngram"] = {}
    return c


def history(beam, max_len, di, b, j):
    """h[0 .. di-1] of row (b, j) at step di: s_{di-1} = j, h[t] = beam[t][b][s_t], s_{t-1} = beam[max_len + t][b][s_t]."""
    h = [0] * di
    s = j
    for t in range(di - 1, -1, -1):
        h[t] = int(beam[t, b, s])
        s = int(beam[max_len + t, b, s])
    return h


def banned_words(h, di, b, V, phrases, phrase_sent, ngram, counts=None):
    """The words [0, V) the phrase list and the n-gram rule ban for a live, unforced row of sentence b with history h."""
    out = set()
    uni = multi = gram = False
    for p in range(len(phrases)):
        if phrase_sent[p] != -1 and phrase_sent[p] != b:
            continue
        ph = [int(w) for w in phrases[p]]
        L = 0
        while L < len(ph) and ph[L] != 0:
            L += 1
        if L == 0 or L - 1 > di:
            continue
        if h[di - L + 1:di] == ph[:L - 1] and 0 <= ph[L - 1] < V:
            out.add(ph[L - 1])
            uni, multi = uni or L == 1, multi or L > 1
    n = int(ngram)
    if n >= 1:
        for t in range(0, di - n + 1):
            if h[t:t + n - 1] == h[di - n + 1:di] and 0 <= h[t + n - 1] < V:
                out.add(h[t + n - 1])
                gram = True
    if counts is not None:
        counts["unigram"] += uni
        counts["multiword"] += multi
        if n >= 1:
            counts["ngram"][n] = counts["ngram"].get(n, 0) + gram
    return out


def mask(rows, beam, di, max_len, B, k, V, prefix=None, phrases=(), phrase_sent=(), ngram=0, counts=None):
    """vag_beam_constrain: rows = M arrays (N, ldl[m]) float32, N = B at step 0 and B k afterwards; returns masked COPIES.
    prefix: None or (B, Lp) int64 pad 0.  Columns [V, ldl) are never touched."""
    out = [np.array(r, dtype=F32, copy=True) for r in rows]
    k_in = 1 if di == 0 else k
    Lp = 0 if prefix is None else prefix.shape[1]
    for b in range(B):
        for j in range(k_in):
            n = b * k_in + j
            h = history(beam, max_len, di, b, j)
            if di >= 1 and h[di - 1] == EOS:
                if counts is not None:
                    counts["finished"] += 1
                continue
            f = int(prefix[b, di]) if di < Lp else 0
            if 1 <= f < V:
                for r in out:
                    keep = r[n, f]
                    r[n, :V] = NEG_PEN
                    r[n, f] = keep
                if counts is not None:
                    counts["forced"] += 1
                continue
            for w in banned_words(h, di, b, V, phrases, phrase_sent, ngram, counts):
                for r in out:
                    r[n, w] = NEG_PEN
    return out


def expand(lp, base, prev, k, flags=0):
    """One sentence, one plain expansion of ONE model's rows lp (R, V) (vag_beam_ens_step_opt, M = 1): the expansion's own
    penalties, c = base + lp in float32, the k best under (c descending, flat index ascending).  Step 0: base = prev = None.
    Returns (words (k,), parents (k,), scores (k,) float32)."""
    lp = np.array(lp, dtype=F32, copy=True)
    R, V = lp.shape
    if prev is None:
        c = lp
    else:
        for j in range(R):
            if prev[j] == EOS:
                lp[j, :] = NEG_PEN
                lp[j, EOS] = 0.0
            else:
                if not flags & ALLOW_REPEAT:
                    lp[j, prev[j]] = NEG_PEN
                if flags & AVOID_UNK:
                    lp[j, UNK] = NEG_PEN
        c = (np.asarray(base, dtype=F32)[:, None] + lp).astype(F32)
    flat = np.arange(R * V)
    order = np.lexsort((flat, -c.ravel().astype(np.float64)))[:k]
    return (order % V).astype(np.int64), (order // V).astype(np.int64), c.ravel()[order].astype(F32)


def search(fn, B, k, V, max_len, steps, prefix=None, phrases=(), phrase_sent=(), ngram=0, flags=0, counts=None):
    """A whole constrained search of one model: fn(previous words (N,) int64) -> (N, V) float32 log-probabilities (N = B at step
    0, B k afterwards), masked, then expanded.  Returns (beam (2 max_len, B, k) int64: words | parents, nll (B, k) float32)."""
    beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
    nll = np.zeros((B, k), dtype=F32)
    for di in range(steps):
        tok = np.full(B, SOS, dtype=np.int64) if di == 0 else beam[di - 1].reshape(-1)
        lp = mask([fn(tok)], beam, di, max_len, B, k, V, prefix, phrases, phrase_sent, ngram, counts)[0]
        k_in = 1 if di == 0 else k
        lp = lp.reshape(B, k_in, -1)[:, :, :V]
        for b in range(B):
            w, p, sc = expand(lp[b], None if di == 0 else nll[b], None if di == 0 else beam[di - 1, b], k, flags)
            beam[di, b], beam[max_len + di, b], nll[b] = w, p, sc
    return beam, nll
