#!/usr/bin/env python3
"""Generate tests/golden/mbr_bleu.npz by RUNNING THE REFERENCE's bleu.py on seeded random candidate sets (build container only).

Usage (from the repo root; the reference checkout must exist, it does not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mbr.py

For every set (B sentences of N rows of L tokens over a small vocabulary, so that n-grams repeat and clipping occurs) and every
ordered pair (i, j) of a sentence's rows with a non-empty reference span r_j, the fixture records
    m      the clipped match counts m_1..m_4: the reference's Counter intersection of _get_ngrams(h_i, 4) and _get_ngrams(r_j, 4)
    bleu   compute_bleu([[r_j]], [h_i], smooth=True)[0], float64
where h_i, r_j are the rows' spans (the tokens before the first EOS = 3).  Pairs with an empty reference span are skipped
(bleu.py divides by zero there); their entries are -1 / NaN.  Data only: token arrays and recorded results, a few tens of KB."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import REF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mbr_bleu.npz")
EOS = 3
# (B, N, L, vocabulary size, probability of an EOS at each position)
SETS = [(3, 6, 9, 2, 0.10), (3, 6, 12, 6, 0.08), (2, 5, 24, 30, 0.05), (1, 4, 70, 6, 0.01), (1, 6, 5, 3, 0.25)]


def span(row):
    out = []
    for t in row:
        if int(t) == EOS:
            break
        out.append(int(t))
    return out


def candidates(rng, B, N, L, V, p_eos):
    """Rows of words 4 .. 4+V-1 with an occasional drawn padding word 0, an EOS somewhere (or nowhere), random words after it."""
    x = rng.integers(4, 4 + V, size=(B, N, L))
    x[rng.random((B, N, L)) < 0.03] = 0
    x[rng.random((B, N, L)) < p_eos] = EOS
    x[:, 0, 0] = EOS                                     # one empty row per sentence
    x[:, 1, :] = np.where(x[:, 1, :] == EOS, 4, x[:, 1, :])          # one row without an EOS
    return x.astype(np.int64)


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import bleu
    rng = np.random.default_rng(20261018)
    out = {}
    pairs = 0
    for s, (B, N, L, V, p_eos) in enumerate(SETS):
        x = candidates(rng, B, N, L, V, p_eos)
        m = np.full((B, N, N, 4), -1, dtype=np.int32)
        u = np.full((B, N, N), np.nan)
        for b in range(B):
            spans = [span(r) for r in x[b]]
            for i in range(N):
                for j in range(N):
                    if not spans[j]:
                        continue
                    overlap = bleu._get_ngrams(spans[i], 4) & bleu._get_ngrams(spans[j], 4)
                    m[b, i, j] = [sum(c for g, c in overlap.items() if len(g) == n) for n in (1, 2, 3, 4)]
                    u[b, i, j] = bleu.compute_bleu([[spans[j]]], [spans[i]], smooth=True)[0]
                    pairs += 1
        out["tok%d" % s], out["m%d" % s], out["bleu%d" % s] = x, m, u
    np.savez_compressed(OUT, n_sets=np.int64(len(SETS)), **out)
    print("wrote %s (%d bytes, %d pairs)" % (OUT, os.path.getsize(OUT), pairs))


if __name__ == "__main__":
    main()
