"""NumPy restatement of the lexical shortlist's selection rule and gather (include/vag_nmt.h: vag_shortlist_select,
vag_shortlist_gather), and the table of selection cases the host and GPU tests share.

Selection: the `always` ids are marked first; then the lexicon's ranks r = 0 .. best-1, rank r of every source word at a position
inside its sentence's length.  A rank whose NEW words would push the count over cap is not applied, and neither are later ranks.
Ids outside their ranges are ignored.  ids: the chosen words ascending, then -1; full2short: the inverse map, -1 elsewhere."""
import numpy as np

MAX_V = 131072


def rank_words(src, lengths, lex, r, V):
    """The target words rank r proposes: those of the source words inside their sentences' lengths, in range."""
    B, Ts = src.shape
    Vs = lex.shape[0]
    out = set()
    for b in range(B):
        for t in range(min(int(lengths[b]), Ts)):
            s = int(src[b, t])
            if 0 <= s < Vs:
                w = int(lex[s, r])
                if 0 <= w < V:
                    out.add(w)
    return out


def select(src, lengths, lex, best, always, V, cap):
    """-> (ids (cap,) int32, n, rank_used, full2short (V,) int32)."""
    mark = np.zeros(V, dtype=bool)
    for w in always:
        if 0 <= int(w) < V:
            mark[int(w)] = True
    count, used = int(mark.sum()), 0
    for r in range(best):
        new = [w for w in rank_words(src, lengths, lex, r, V) if not mark[w]]
        if count + len(new) > cap:
            break
        mark[new] = True
        count += len(new)
        used = r + 1
    chosen = np.nonzero(mark)[0]
    assert len(chosen) == count <= cap
    ids = np.full(cap, -1, dtype=np.int32)
    ids[:count] = chosen
    full2short = np.full(V, -1, dtype=np.int32)
    full2short[chosen] = np.arange(count, dtype=np.int32)
    return ids, count, used, full2short


def counts_by_rank(src, lengths, lex, best, always, V):
    """c[r]: the number of chosen words after the always ids and ranks 0 .. r-1 with no cap (c[0]: the always ids alone)."""
    return [select(src, lengths, lex, r, always, V, V)[1] for r in range(best + 1)]


def gather(ids, n, cap, src, pad):
    """(cap, W): row j < n is src[ids[j]], rows >= n hold pad."""
    src2 = src.reshape(src.shape[0], -1)
    out = np.full((cap, src2.shape[1]), pad, dtype=np.float32)
    out[:n] = src2[ids[:n]]
    return out


def _random(rng, B, Ts, Vs, K, V, fill=0.8):
    src = rng.integers(0, Vs, size=(B, Ts)).astype(np.int64)
    lengths = rng.integers(1, Ts + 1, size=B).astype(np.int32)
    lengths[0] = Ts
    lex = rng.integers(4, V, size=(Vs, K)).astype(np.int32)
    width = rng.integers(0, K + 1, size=Vs)                      # rows are padded with -1 behind their width
    lex[np.arange(K)[None, :] >= width[:, None]] = -1
    if fill >= 1.0:
        lex = rng.integers(4, V, size=(Vs, K)).astype(np.int32)
    return src, lengths, lex


def cases():
    """name -> dict(src, lengths, lex, best, always, V, cap[, rank_used]); rank_used where the case is built to end there."""
    rng = np.random.default_rng(20240521)
    out = {}
    base = np.arange(8, dtype=np.int32)
    for V in (37, 1000, 9391):                                  # not multiples of 32: the bitmap's tail word
        src, lengths, lex = _random(rng, 3, 7, 50, 6, V)
        lex[5, 0] = V - 1                                       # the last word of the vocabulary, chosen
        src[0, 0] = 5
        out["V%d" % V] = dict(src=src, lengths=lengths, lex=lex, best=6, always=base, V=V, cap=max(8, min(V, 160) - 3))
    src, lengths, lex = _random(rng, 1, 1, 20, 4, 200, fill=1.0)
    out["one_word"] = dict(src=src, lengths=np.array([1], np.int32), lex=lex, best=4, always=base, V=200, cap=16)
    # a short sentence whose padding positions hold real-looking ids: they must not count
    src, _, lex = _random(rng, 2, 8, 40, 3, 500, fill=1.0)
    lengths = np.array([8, 2], np.int32)
    c = dict(src=src, lengths=lengths, lex=lex, best=3, always=base, V=500, cap=64)
    assert select(**c)[1] < select(**dict(c, lengths=np.array([8, 8], np.int32)))[1]
    out["padding_ids"] = c
    src, lengths, lex = _random(rng, 3, 6, 30, 4, 300, fill=1.0)
    src[:] = src[0, 0]
    src[1, 2:] = src[0, 1] = (src[0, 0] + 1) % 30
    out["duplicate_source"] = dict(src=src, lengths=np.array([6, 6, 6], np.int32), lex=lex, best=4, always=base, V=300, cap=32)
    src, lengths, lex = _random(rng, 2, 5, 30, 4, 300)
    lex[:] = -1
    out["empty_lexicon"] = dict(src=src, lengths=lengths, lex=lex, best=4, always=base, V=300, cap=16, rank_used=4)
    src, lengths, lex = _random(rng, 2, 5, 30, 4, 300, fill=1.0)
    always = np.array([0, 1, 2, 3, 3, 2, 9, 9, 9, int(lex[src[0, 0], 0]), int(lex[src[1, 0], 1]), 0], dtype=np.int32)
    out["always_duplicates"] = dict(src=src, lengths=lengths, lex=lex, best=4, always=always, V=300, cap=40)
    src, lengths, lex = _random(rng, 3, 6, 30, 5, 300, fill=1.0)
    src[0, 1], src[1, 0], src[2, 2] = -1, 30, 10 ** 12
    lex[:, 1] = 300
    lex[::2, 2] = -7
    lex[1::3, 3] = 2 ** 31 - 1
    out["out_of_range"] = dict(src=src, lengths=np.array([6, 6, 6], np.int32), lex=lex, best=5, always=base, V=300, cap=64)
    # the count meets cap exactly after the last rank: everything is applied
    src, lengths, lex = _random(rng, 3, 6, 40, 5, 1000, fill=1.0)
    cs = counts_by_rank(src, lengths, lex, 5, base, 1000)
    out["cap_exact"] = dict(src=src, lengths=lengths, lex=lex, best=5, always=base, V=1000, cap=cs[5], rank_used=5)
    # cap falls inside rank 2 of 5: ranks 0 and 1 are applied, rank 2 and the later ones are not
    assert cs[3] - cs[2] >= 2 and cs[2] > cs[1] > cs[0]
    out["cap_mid_rank"] = dict(src=src, lengths=lengths, lex=lex, best=5, always=base, V=1000, cap=cs[2] + (cs[3] - cs[2]) // 2,
                               rank_used=2)
    out["cap_is_always"] = dict(src=src, lengths=lengths, lex=lex, best=5, always=np.arange(12, dtype=np.int32), V=1000, cap=12,
                                rank_used=0)
    src, lengths, lex = _random(rng, 4, 9, 300, 8, MAX_V, fill=1.0)
    lex[7, 0] = MAX_V - 1
    src[0, 0] = 7
    out["largest_V"] = dict(src=src, lengths=lengths, lex=lex, best=8, always=np.arange(104, dtype=np.int32), V=MAX_V, cap=512)
    return out
