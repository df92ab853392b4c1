#!/usr/bin/env python3
"""Generate tests/golden/corpus_bleu.npz by RUNNING THE REFERENCE's bleu.py on seeded random corpora (build container only).

Usage (from the repo root; the reference checkout must exist, it does not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_corpus_bleu.py

Every corpus is N sentences: a hypothesis row (N, Lh) and up to R reference rows (N, R, Lr) with n_refs (N,) of them in use, as
vag_corpus_bleu_stats takes them (a row's content is what precedes its first EOS = 3; rows j >= n_refs[b] hold a copy of the
hypothesis, which must not count).  The fixture records, for smooth = False and True,
    compute_bleu(reference spans, hypothesis spans, smooth=smooth)      all six fields
as f (2, 7) float64 = (bleu, p_1..p_4, bp, ratio) and i (2,) int64 = (translation_length, reference_length).  The corpora: 1 to
40 sentences, 1 to 5 references of different lengths, vocabularies of 2, 6 and 30 words; empty hypotheses, hypotheses longer and
shorter than every reference, corpora without a 4-gram match (geometric mean 0).  Every sentence has a non-empty reference and
every corpus a positive reference length, so bleu.py never divides by zero.  Data only: token arrays and recorded results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "corpus_bleu.npz")
EOS = 3
# (N, R, Lh, Lr, vocabulary size, kind)
SETS = [(1, 1, 9, 12, 6, "plain"), (1, 3, 7, 5, 2, "plain"), (5, 2, 12, 9, 2, "plain"), (12, 5, 14, 18, 6, "plain"),
        (40, 4, 20, 24, 30, "plain"), (17, 3, 24, 16, 6, "long_hyps"), (9, 5, 6, 20, 6, "short_hyps"),
        (8, 2, 4, 10, 30, "no_4gram"), (6, 1, 16, 16, 30, "disjoint"), (33, 5, 10, 10, 2, "plain"), (3, 4, 30, 8, 6, "related")]


def span(row):
    out = []
    for t in row:
        if int(t) == EOS:
            break
        out.append(int(t))
    return out


def row(rng, L, n, V, lo=4):
    """n words of lo .. lo+V-1, an EOS (if there is room), padding 0."""
    x = np.zeros(L, dtype=np.int64)
    n = min(n, L)
    x[:n] = rng.integers(lo, lo + V, size=n)
    if n < L:
        x[n] = EOS
    return x


def corpus(rng, N, R, Lh, Lr, V, kind):
    hyps = np.zeros((N, Lh), dtype=np.int64)
    refs = np.zeros((N, R, Lr), dtype=np.int64)
    n_refs = rng.integers(1, R + 1, size=N).astype(np.int32)
    n_refs[0] = R
    for b in range(N):
        lens = rng.permutation(np.arange(1, Lr + 1))[:R]                     # different lengths, none empty
        lh = int(rng.integers(0, Lh + 1))
        if kind == "long_hyps":
            lens = np.minimum(lens, Lh // 2)
            lh = int(rng.integers(Lh // 2 + 1, Lh + 1))
        elif kind == "short_hyps":
            lens = np.maximum(lens, Lh)
            lh = int(rng.integers(0, Lh - 1))
        elif kind == "no_4gram":
            lh = int(rng.integers(0, 4))                                     # no hypothesis has a 4-gram
        elif b % 7 == 3:
            lh = 0                                                           # an empty hypothesis
        hyps[b] = row(rng, Lh, lh, V)
        for j in range(R):
            if j >= n_refs[b]:
                refs[b, j, :min(Lh, Lr)] = hyps[b, :min(Lh, Lr)]           # unused rows: the hypothesis itself
                continue
            refs[b, j] = row(rng, Lr, int(lens[j]), V, lo=4 + V if kind == "disjoint" else 4)
            if kind == "related" or (kind == "plain" and rng.random() < 0.5):    # a noisy copy of the hypothesis
                n = min(lh, int(lens[j]))
                keep = rng.random(n) < 0.8
                refs[b, j, :n] = np.where(keep, hyps[b, :n], refs[b, j, :n])
    return hyps, refs, n_refs


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import bleu
    rng = np.random.default_rng(20261020)
    out = {}
    for s, (N, R, Lh, Lr, V, kind) in enumerate(SETS):
        hyps, refs, n_refs = corpus(rng, N, R, Lh, Lr, V, kind)
        hs = [span(h) for h in hyps]
        rs = [[span(r) for r in refs[b, :n_refs[b]]] for b in range(N)]
        assert all(any(len(r) > 0 for r in sent) for sent in rs) and sum(min(len(r) for r in sent) for sent in rs) > 0
        f = np.zeros((2, 7))
        i = np.zeros(2, dtype=np.int64)
        for k, smooth in enumerate((False, True)):
            b, p, bp, ratio, tl, rl = bleu.compute_bleu(rs, hs, smooth=smooth)
            f[k] = [b] + list(p) + [bp, ratio]
            i[:] = [tl, rl]
        if kind in ("no_4gram", "disjoint"):
            assert f[0, 0] == 0.0 and f[0, 4] == 0.0
        print("set %d %-10s N=%2d R=%d: bleu %.6f smooth %.6f  tl %d rl %d" % (s, kind, N, R, f[0, 0], f[1, 0], i[0], i[1]))
        out["hyps%d" % s], out["refs%d" % s], out["nrefs%d" % s], out["f%d" % s], out["i%d" % s] = hyps, refs, n_refs, f, i
    np.savez_compressed(OUT, n_sets=np.int64(len(SETS)), **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
