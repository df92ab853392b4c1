"""NumPy restatement of diverse beam search as include/vag_nmt.h states it (vag_beam_div_step, vag_beam_finish_nbest_slots):
the yardstick of tests/test_diverse_host.py and tests/test_gpu_diverse.py.  float32 arithmetic, an explicit total order
(key descending, flat index j V + w ascending), no shortcut: every group ranks all candidates of its rows.

    step(logp, base, prev, k, G, lam, flags)     one sentence, one step
    search(fn, B, k, G, lam, V, max_len, steps)  a whole search on logp = fn(previous words)
    finish(beam, nll, max_len, steps, n)         the n-best finish with the final slots
"""
import numpy as np

SOS, EOS, UNK = 2, 3, 1
NEG_PEN = np.float32(-1e5)
ALLOW_REPEAT, AVOID_UNK = 1, 2
F32 = np.float32


def ens_combine(xs):
    """select.h's ens_score of M members' rows, in float32: mx + log(sum_m exp(x_m - mx) / M); M = 1 is x itself."""
    xs = [np.asarray(x, dtype=F32) for x in xs]
    if len(xs) == 1:
        return xs[0]
    mx = xs[0]
    for x in xs[1:]:
        mx = np.maximum(mx, x)
    tot = np.zeros_like(mx)
    for x in xs:
        tot = (tot + np.exp((x - mx).astype(F32)).astype(F32)).astype(F32)
    return (mx + np.log((tot / F32(len(xs))).astype(F32)).astype(F32)).astype(F32)


def model_values(logp, base, prev, flags=0):
    """c(j, w) = base_j + lp'(j, w) in float32.  logp (R, V); step 0: base = prev = None (R = 1, no penalty)."""
    lp = np.array(logp, dtype=F32, copy=True)
    R = lp.shape[0]
    if prev is None:
        return (np.zeros((R, 1), dtype=F32) + lp).astype(F32)
    for j in range(R):
        if prev[j] == EOS:
            lp[j, :] = NEG_PEN
            lp[j, EOS] = 0.0
        else:
            if not flags & ALLOW_REPEAT:
                lp[j, prev[j]] = NEG_PEN
            if flags & AVOID_UNK:
                lp[j, UNK] = NEG_PEN
    return (np.asarray(base, dtype=F32)[:, None] + lp).astype(F32)


def keys(c, cnt, lam, fin):
    """s = float32(float64(c) - float64(lam) cnt[w]); a finished row keeps c."""
    s = (c.astype(np.float64) - np.float64(lam) * cnt[None, :].astype(np.float64)).astype(F32)
    return np.where(np.asarray(fin, dtype=bool)[:, None], c, s)


def step(logp, base, prev, k, G, lam, flags=0):
    """One sentence, one step -> (words (k,), parents (k,), scores (k,) float32 = c of the chosen candidates)."""
    c = model_values(logp, base, prev, flags)
    R, V = c.shape
    assert k % G == 0 and V >= k and R in (1, k)
    g = k // G
    fin = np.zeros(R, dtype=bool) if prev is None else np.asarray(prev) == EOS
    cnt = np.zeros(V, dtype=np.int64)
    words, parents, scores = [], [], []
    for i in range(G):
        rows = np.arange(R) if R == 1 else np.arange(i * g, (i + 1) * g)
        s = keys(c[rows], cnt, lam, fin[rows])
        flat = (rows[:, None] * V + np.arange(V)[None, :]).ravel()
        order = np.lexsort((flat, -s.ravel().astype(np.float64)))[:g]          # key descending, then flat index ascending
        for f in flat[order]:
            j, w = int(f) // V, int(f) % V
            words.append(w); parents.append(j); scores.append(c[j, w])
            if not fin[j]:
                cnt[w] += 1
    return np.array(words, dtype=np.int64), np.array(parents, dtype=np.int64), np.array(scores, dtype=F32)


def search(fn, B, k, G, lam, V, max_len, steps, flags=0):
    """A whole search: fn(previous words (N,) int64) -> (N, V) float32 log-probabilities (N = B at step 0, B k afterwards).
    Returns (beam (2 max_len, B, k) int64: words | parents, nll (B, k) float32)."""
    beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
    nll = np.zeros((B, k), dtype=F32)
    for di in range(steps):
        if di == 0:
            lp = fn(np.full(B, SOS, dtype=np.int64)).reshape(B, 1, V)
        else:
            lp = fn(beam[di - 1].reshape(-1)).reshape(B, k, V)
        for b in range(B):
            w, p, sc = step(lp[b], None if di == 0 else nll[b], None if di == 0 else beam[di - 1, b], k, G, lam, flags)
            beam[di, b], beam[max_len + di, b], nll[b] = w, p, sc
    return beam, nll


def finish(beam, nll, max_len, steps, n):
    """vag_beam_finish_nbest_slots: score = nll / max(1, #words > 3) over the written rows (row max_len - 1 is forced to EOS and
    never counts), order (score descending, slot ascending) -> out (B, n, max_len), scores (B, n) float32, slots (B, n)."""
    _, B, k = beam.shape
    out = np.zeros((B, n, max_len), dtype=np.int64)
    scores = np.zeros((B, n), dtype=F32)
    slots = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        rows, sc = [], []
        for j in range(k):
            row = np.zeros(max_len, dtype=np.int64)
            p = j
            for t in range(steps - 1, -1, -1):
                row[t] = beam[t, b, p]
                p = beam[max_len + t, b, p]
            words = int((row[:min(steps, max_len - 1)] > 3).sum())
            row[max_len - 1] = EOS
            rows.append(row)
            sc.append(F32(nll[b, j]) / F32(max(1, words)))
        order = sorted(range(k), key=lambda j: (-float(sc[j]), j))[:n]
        for r, j in enumerate(order):
            out[b, r], scores[b, r], slots[b, r] = rows[j], sc[j], j
    return out, scores, slots


def cut(row):
    row = [int(t) for t in row]
    return row[:row.index(EOS)] if EOS in row else row
