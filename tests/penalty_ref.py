"""NumPy restatement of the penalised beam search as include/vag_nmt.h states it (vag_beam_cover, vag_beam_pen_step,
vag_beam_finish_pen): the yardstick of tests/test_penalty_host.py and tests/test_gpu_penalty.py.  float32 arithmetic with one
rounding per operation, an explicit total order (key descending, flat index j V + w ascending), no shortcut: every candidate of
every row is ranked.

    tables(max_len, norm, alpha, word_bonus)                           the host tables, restated (fp64, rounded once)
    score(c, length, cp, lp, bonus)                                    s = fl(fl(fl(c + bonus[L]) / lp[L]) + cp)
    cover(alphas, mask, cov, prev, beta)                               cov_row (float32, exact) and cp_row (float64)
    step(logp, base, prev, lens, cp_row, k, lp, bonus, stepwise, ...)  one sentence, one step
    search(fn, afn, mask, ...)                                         a whole search on a table model
    finish(beam, nll, lens, cpen, lp, bonus, max_len, steps, n)        the ranking finish
"""
import numpy as np

from diverse_ref import EOS, SOS, F32, model_values

COV_FLOOR = F32(1e-10)


def tables(max_len, norm="gnmt", alpha=0.6, word_bonus=0.0):
    L = np.maximum(np.arange(max_len + 1, dtype=np.float64), 1.0)
    lp = {"gnmt": ((5.0 + L) / 6.0) ** alpha, "length": L ** alpha, "none": np.ones_like(L)}[norm]
    return lp.astype(F32), (np.float64(word_bonus) * L).astype(F32)


def score(c, length, cp, lp, bonus):
    """The penalised score, elementwise: float32 at every operation."""
    L = np.maximum(np.asarray(length, dtype=np.int64), 1)
    with np.errstate(all="ignore"):
        t = (np.asarray(c, dtype=F32) + bonus[L]).astype(F32)
        t = (t / lp[L]).astype(F32)
        return (t + np.asarray(cp, dtype=F32)).astype(F32)


def mean_rows(alphas):
    """vag_beam_attn_record's mean over members: sum in member order, one division; M = 1 is the row itself."""
    a = np.asarray(alphas[0], dtype=F32)
    if len(alphas) == 1:
        return a
    for x in alphas[1:]:
        a = (a + np.asarray(x, dtype=F32)).astype(F32)
    return (a / F32(len(alphas))).astype(F32)


def cover(alphas, mask, cov, prev, beta):
    """One step's rows of one or more sentences.  alphas: M arrays (N, Tp); mask (N, Tp) (every row's own sentence's mask); cov
    (N, Tp) or None at step 0; prev (N,) previous words or None at step 0.  Returns (cov_row float32 -- exact --, cp_row float64:
    the sum is order-free here, the device's fp32 order is stated in the header)."""
    a = mean_rows(alphas)
    if cov is None:
        row = a
    else:
        fin = (np.asarray(prev) == EOS)[:, None]
        row = np.where(fin, np.asarray(cov, dtype=F32), (np.asarray(cov, dtype=F32) + a).astype(F32)).astype(F32)
    term = np.log(np.minimum(np.maximum(row, COV_FLOOR), F32(1.0)).astype(np.float64))
    cp = np.float64(beta) * np.where(np.asarray(mask) != 0, term, 0.0).sum(axis=1)
    return row, cp


def step(logp, base, prev, lens, cp_row, k, lp, bonus, stepwise, di, max_len, flags=0):
    """One sentence, one step.  logp (R, V) the (combined) log-probabilities; step 0: base = prev = lens = None (R = 1).
    cp_row (R,) float32.  Returns (words, parents, c of the chosen (float32), len' (int32), cpen (float32), keys (float32))."""
    c = model_values(logp, base, prev, flags)
    R, V = c.shape
    assert V >= k and R in (1, k)
    fin = np.zeros(R, dtype=bool) if prev is None else np.asarray(prev) == EOS
    ln = np.zeros(R, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)
    cp_row = np.asarray(cp_row, dtype=F32)
    key = np.zeros((R, V), dtype=F32)
    l2 = np.zeros((R, V), dtype=np.int64)
    valid = np.ones((R, V), dtype=bool)
    for j in range(R):
        if fin[j]:                                              # (j, EOS) alone, c = base_j, the frozen length
            c[j, EOS] = F32(F32(base[j]) + F32(0.0))
            l2[j] = ln[j]
            valid[j] = False
            valid[j, EOS] = True
        else:
            l2[j] = ln[j] + ((np.arange(V) > 3) & (di < max_len - 1)).astype(np.int64)
        key[j] = score(c[j], l2[j], np.full(V, cp_row[j], dtype=F32), lp, bonus) if stepwise else c[j]
    flat = np.flatnonzero(valid.ravel())
    order = flat[np.lexsort((flat, -key.ravel()[flat].astype(np.float64)))[:k]]      # key descending, then flat index ascending
    words, parents = order % V, order // V
    return (words.astype(np.int64), parents.astype(np.int64), c.ravel()[order].astype(F32), l2.ravel()[order].astype(np.int32),
            cp_row[parents], key.ravel()[order].astype(F32))


def f32_cp(row, mask, beta):
    """cp of cov rows in float32 NumPy (the CPU tests' own stand-in for the device's logf and summation order)."""
    term = np.log(np.minimum(np.maximum(row, COV_FLOOR), F32(1.0))).astype(F32)
    term = np.where(np.asarray(mask) != 0, term, F32(0.0)).astype(F32)
    acc = np.zeros(row.shape[0], dtype=F32)
    for i in range(row.shape[1]):
        acc = (acc + term[:, i]).astype(F32)
    return (F32(beta) * acc).astype(F32)


def search(fn, afn, mask, B, k, V, max_len, steps, lp, bonus, beta, stepwise, flags=0, cp_rows=None, trace=None):
    """A whole search on a table model: fn(previous words (N,)) -> (N, V) float32 log-probabilities, afn(previous words) ->
    (N, Tp) float32 attention rows (N = B at step 0, B k afterwards); mask (B, Tp).  cp_rows: None (cp from f32_cp) or a list
    of the per-step cp_row arrays (N,) to use instead (the device's own, whose logf NumPy cannot restate bit for bit).
    trace: a list that receives, per step, (c (B, R, V), keys chosen, parents, words, prev) for the tests' own assertions.
    Returns dict(beam, nll, lens, cpen, cov, cov_rows (per step))."""
    Tp = mask.shape[1]
    beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
    nll = np.zeros((B, k), dtype=F32)
    lens = np.zeros((B, k), dtype=np.int32)
    cpen = np.zeros((B, k), dtype=F32)
    cov = np.zeros((B, k, Tp), dtype=F32)
    cov_rows = []
    for di in range(steps):
        R = 1 if di == 0 else k
        prev = np.full((B, 1), SOS, dtype=np.int64) if di == 0 else beam[di - 1]
        lpm = fn(prev.reshape(-1)).reshape(B, R, V)
        if beta > 0:
            row, _ = cover([afn(prev.reshape(-1))], np.repeat(mask, R, axis=0), None if di == 0 else cov.reshape(B * k, Tp),
                           None if di == 0 else prev.reshape(-1), beta)
            cp = f32_cp(row, np.repeat(mask, R, axis=0), beta) if cp_rows is None else np.asarray(cp_rows[di], dtype=F32)
        else:
            row, cp = np.zeros((B * R, Tp), dtype=F32), np.zeros(B * R, dtype=F32)
        cov_rows.append(row)
        row, cp = row.reshape(B, R, Tp), cp.reshape(B, R)
        new_cov = np.zeros_like(cov)
        for b in range(B):
            w, p, sc, ln, cpn, keys = step(lpm[b], None if di == 0 else nll[b], None if di == 0 else beam[di - 1, b],
                                           None if di == 0 else lens[b], cp[b], k, lp, bonus, stepwise, di, max_len, flags)
            if trace is not None:
                trace.append(dict(di=di, b=b, c=model_values(lpm[b], None if di == 0 else nll[b].copy(),
                                                             None if di == 0 else beam[di - 1, b].copy(), flags),
                                  words=w, parents=p, keys=keys, prev=None if di == 0 else beam[di - 1, b].copy()))
            beam[di, b], beam[max_len + di, b], nll[b], lens[b], cpen[b] = w, p, sc, ln, cpn
            new_cov[b] = row[b][p]
        cov = new_cov
    return dict(beam=beam, nll=nll, lens=lens, cpen=cpen, cov=cov, cov_rows=cov_rows)


def finish(beam, nll, lens, cpen, lp, bonus, max_len, steps, n):
    """vag_beam_finish_pen: s from the carried values, order (s descending, slot ascending) -> dict(out (B, n, max_len), scores,
    slots, logp, length, cp), all (B, n)."""
    _, B, k = beam.shape
    out = np.zeros((B, n, max_len), dtype=np.int64)
    res = dict(out=out, scores=np.zeros((B, n), dtype=F32), slots=np.zeros((B, n), dtype=np.int64), logp=np.zeros((B, n), dtype=F32),
               length=np.zeros((B, n), dtype=np.int32), cp=np.zeros((B, n), dtype=F32))
    for b in range(B):
        s = score(nll[b], lens[b], cpen[b], lp, bonus)
        order = sorted(range(k), key=lambda j: (-float(s[j]), j))[:n]
        for r, j in enumerate(order):
            p = j
            for t in range(steps - 1, -1, -1):
                out[b, r, t] = beam[t, b, p]
                p = beam[max_len + t, b, p]
            out[b, r, max_len - 1] = EOS
            res["scores"][b, r], res["slots"][b, r], res["logp"][b, r] = s[j], j, nll[b, j]
            res["length"][b, r], res["cp"][b, r] = lens[b, j], cpen[b, j]
    return res


def walk_length(beam, max_len, steps, b, j):
    """The length vag_beam_finish_nbest's walk implies for final slot j of sentence b."""
    n, p = 0, j
    for t in range(steps - 1, -1, -1):
        if t < max_len - 1:
            n += int(beam[t, b, p] > 3)
        p = beam[max_len + t, b, p]
    return n
