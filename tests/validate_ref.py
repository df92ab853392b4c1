"""Plain Python restatement of the validation metrics' definitions (include/vag_nmt.h: vag_corpus_bleu_stats; vagnmt_hip/validate.py),
written from the definitions, independent of the library and of the reference's bleu.py: per-sentence statistics, totals, the
corpus BLEU finish and the corpus chrF finish.  Counter arithmetic on tuples; nothing here is shared with the code under test."""
import math
from collections import Counter

EOS = 3


def span(row):
    """The tokens before the first EOS, or the whole row; ids on their low 32 bits."""
    out = []
    for t in row:
        t = int(t)
        if t == EOS:
            break
        out.append(t & 0xffffffff)
    return out


def ngrams(x, n):
    return Counter(tuple(x[i:i + n]) for i in range(len(x) - n + 1))


def sentence_stats(hyp, refs):
    """[m_1..m_4, T_1..T_4, l_h, l_r] of one hypothesis span against its reference spans (at least one)."""
    m, T = [], []
    for n in (1, 2, 3, 4):
        ch = ngrams(hyp, n)
        merged = Counter()
        for r in refs:
            for g, c in ngrams(r, n).items():
                merged[g] = max(merged[g], c)                  # the per-n-gram maximum over the references
        m.append(sum(min(c, merged[g]) for g, c in ch.items()))
        T.append(max(0, len(hyp) - n + 1))
    return m + T + [len(hyp), min(len(r) for r in refs)]


def corpus_stats(hyps, refs, n_refs=None):
    """hyps: N token rows; refs: N lists of R token rows; n_refs: None or N counts (clamped to [1, R]; rows beyond are not read).
    Returns (per_sentence N x 10, totals 10) as Python ints."""
    per = []
    for b, (h, rs) in enumerate(zip(hyps, refs)):
        rs = list(rs)
        k = len(rs) if n_refs is None else min(max(int(n_refs[b]), 1), len(rs))
        per.append(sentence_stats(span(h), [span(r) for r in rs[:k]]))
    return per, [sum(p[i] for p in per) for i in range(10)]


def bleu_finish(totals, smooth=False):
    """(bleu, precisions, bp, ratio, translation_length, reference_length) from the ten totals.  precision_n = M_n / T_n (0 when
    T_n = 0), smoothed (M_n + 1) / (T_n + 1); the geometric mean exp(sum 1/4 log p_n) when every p_n > 0, else 0; ratio = the
    translation length over the reference length; bp = 1 above ratio 1, 0 at ratio 0, else exp(1 - 1 / ratio)."""
    M, T, tl, rl = totals[0:4], totals[4:8], totals[8], totals[9]
    p = []
    for n in range(4):
        if smooth:
            p.append((M[n] + 1.0) / (T[n] + 1.0))
        else:
            p.append(float(M[n]) / T[n] if T[n] > 0 else 0.0)
    geo = math.exp(sum(0.25 * math.log(x) for x in p)) if min(p) > 0 else 0
    ratio = float(tl) / rl
    bp = 1.0 if ratio > 1.0 else (0.0 if ratio == 0.0 else math.exp(1 - 1.0 / ratio))
    return geo * bp, p, bp, ratio, tl, rl


def corpus_bleu(hyps, refs, n_refs=None, smooth=False):
    return bleu_finish(corpus_stats(hyps, refs, n_refs)[1], smooth)


# ---- chrF pooled over the corpus -------------------------------------------------------------------------------------
def chars(row, surfaces, limit):
    """The code points the row's span spells, cut to the first `limit` characters (the stored row)."""
    out = []
    for t in span(row):
        out.extend(ord(c) for c in surfaces[t])
    return out[:limit]


def chrf_totals(hyps, refs, surfaces, limit_h, limit_r):
    """[M_1..M_6, H_1..H_6, R_1..R_6]: clipped character n-gram matches and the n-gram counts of both sides, summed."""
    M, H, R = [0] * 6, [0] * 6, [0] * 6
    for h, r in zip(hyps, refs):
        hc, rc = chars(h, surfaces, limit_h), chars(r, surfaces, limit_r)
        for n in range(1, 7):
            a, b = ngrams(hc, n), ngrams(rc, n)
            M[n - 1] += sum(min(c, b[g]) for g, c in a.items())
            H[n - 1] += max(0, len(hc) - n + 1)
            R[n - 1] += max(0, len(rc) - n + 1)
    return M + H + R


def chrf_finish(totals):
    """F with beta = 2 of the mean precision and recall over the effective orders (both totals > 0), float64; 0 with none, or
    when P + R = 0."""
    M, H, R = totals[0:6], totals[6:12], totals[12:18]
    eff = [n for n in range(6) if H[n] > 0 and R[n] > 0]
    if not eff:
        return 0.0
    sp = sr = 0.0
    for n in eff:
        sp += M[n] / H[n]
        sr += M[n] / R[n]
    P, Rc = sp / len(eff), sr / len(eff)
    if P + Rc == 0.0:
        return 0.0
    return 5.0 * P * Rc / (4.0 * P + Rc)
