"""Plain-Python float64 restatement of the minimum-Bayes-risk definitions of include/vag_nmt.h (vag_mbr_select): the span of
a row, clipped n-gram matches by Counter intersection, the two utilities, the expected utility.  A test helper, not a test."""
import math
from collections import Counter

import numpy as np

EOS = 3


def span(row):
    """The tokens before the first EOS (the whole row if there is none)."""
    out = []
    for t in row:
        t = int(t)
        if t == EOS:
            break
        out.append(t)
    return out


def ngrams(seg, n):
    return Counter(tuple(seg[i:i + n]) for i in range(len(seg) - n + 1))


def matches(h, r):
    """m_1..m_4 of two spans: sum over n-grams of min(count_h, count_r)."""
    return [sum((ngrams(h, n) & ngrams(r, n)).values()) for n in (1, 2, 3, 4)]


def T(l, n):
    return max(0, l - n + 1)


def bleu(m, lh, lr):
    if lh == 0:
        return 0.0
    bp = 1.0 if lh > lr else math.exp(1.0 - lr / lh)
    return bp * math.exp(0.25 * sum(math.log((m[n - 1] + 1.0) / (T(lh, n) + 1.0)) for n in (1, 2, 3, 4)))


def ngram_f(m, lh, lr):
    terms = [2.0 * m[n - 1] / (T(lh, n) + T(lr, n)) for n in (1, 2, 3, 4) if T(lh, n) + T(lr, n) > 0]
    return sum(terms) / len(terms) if terms else 0.0


UTILITY = {"bleu": bleu, "ngram_f": ngram_f}


def pairwise(hyps, refs=None):
    """hyps (B, Nh, Lh), refs (B, Nr, Lr) integer arrays (refs None: the candidates) -> m (B, Nh, Nr, 4) int64, lh (B, Nh),
    lr (B, Nr)."""
    hyps = np.asarray(hyps)
    refs = hyps if refs is None else np.asarray(refs)
    B, Nh, Nr = hyps.shape[0], hyps.shape[1], refs.shape[1]
    m = np.zeros((B, Nh, Nr, 4), dtype=np.int64)
    lh = np.zeros((B, Nh), dtype=np.int64)
    lr = np.zeros((B, Nr), dtype=np.int64)
    for b in range(B):
        hs = [span(r) for r in hyps[b]]
        rs = [span(r) for r in refs[b]]
        hg = [[ngrams(s, n) for n in (1, 2, 3, 4)] for s in hs]
        rg = [[ngrams(s, n) for n in (1, 2, 3, 4)] for s in rs]
        lh[b] = [len(s) for s in hs]
        lr[b] = [len(s) for s in rs]
        for i in range(Nh):
            for j in range(Nr):
                m[b, i, j] = [sum((hg[i][n] & rg[j][n]).values()) for n in range(4)]
    return m, lh, lr


def utilities(m, lh, lr, utility):
    """u (B, Nh, Nr) float64 from pairwise()'s output."""
    f = UTILITY[utility]
    B, Nh, Nr = m.shape[:3]
    u = np.zeros((B, Nh, Nr))
    for b in range(B):
        for i in range(Nh):
            for j in range(Nr):
                u[b, i, j] = f([int(x) for x in m[b, i, j]], int(lh[b, i]), int(lr[b, j]))
    return u


def expected(u, weights=None):
    """E (B, Nh) float64: sum_j w_j u[b, i, j]; weights (B, Nr) as given, None: 1 / Nr."""
    w = np.full((u.shape[0], u.shape[2]), 1.0 / u.shape[2]) if weights is None else np.asarray(weights, dtype=np.float64)
    return (u * w[:, None, :]).sum(2)
