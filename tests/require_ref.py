"""NumPy restatement of the required-phrase beam search as include/vag_nmt.h states it (vag_beam_req_step, optionally after
vag_beam_constrain): the yardstick of tests/test_require_host.py and tests/test_gpu_require.py.  Written from the header's text:
float32 adds, explicit total orders, every candidate of a step looked at, the slots dealt by a literal order over
(rho ascending, bank descending).

    lengths(table)                                  L_c of a sentence's (16, 8) phrase table
    transition(phrase, L, p, w)                     the progress p' of one phrase on word w
    child(state, fin, w, table)                     the state {met, prog_lo, prog_hi, n} of a child
    slot_order(cands) / round_robin(cands)          the allotment in closed form / as the loop it abbreviates
    step(logps, base, prev, k, table, states, ...)  one sentence, one expansion (M members: the ensemble formula)
    search(fn, B, k, V, max_len, steps, required)   a whole search on logp = fn(previous words), step records kept
"""
import numpy as np

import constrain_ref
from diverse_ref import ens_combine

SOS, EOS, UNK = 2, 3, 1
NEG_PEN = np.float32(-1e5)
LIVE = np.float32(-5e4)
ALLOW_REPEAT, AVOID_UNK = 1, 2
MAX_PHRASES, MAX_LEN = 16, 8
F32 = np.float32
ZERO = (0, 0, 0, 0)
BRANCHES = ("completed", "fell_back", "reset", "b_outside", "b_dedup", "eos_ruled_out", "finished_kept", "banks3", "dead_fill")


def new_counts():
    """(row, step) pairs -- for banks3 and dead_fill (sentence, step) pairs -- in which each branch fired."""
    return {name: 0 for name in BRANCHES}


def lengths(table):
    """L_c = the number of leading non-zero words of every row of a (16, 8) table."""
    out = []
    for row in table:
        L = 0
        while L < len(row) and row[L] != 0:
            L += 1
        out.append(L)
    return out


def transition(phrase, L, p, w):
    """The largest q <= min(L, p + 1) such that the last q words of phrase[0..p-1] + [w] equal phrase[0..q-1]."""
    s = [int(x) for x in phrase[:p]] + [int(w)]
    for q in range(min(L, p + 1), 0, -1):
        if s[len(s) - q:] == [int(x) for x in phrase[:q]]:
            return q
    return 0


def progress(state, c):
    return ((state[1] if c < 8 else state[2]) >> (4 * (c % 8))) & 15


def child(state, fin, w, table, counts=None):
    """The child of a row with `state` that takes word w; a finished row's child keeps the state.  counts: the branches of the
    transition this child took (at most one count each)."""
    if fin:
        return tuple(int(x) for x in state)
    met, lo, hi, n = int(state[0]), 0, 0, 0
    hit = set()
    for c, L in enumerate(lengths(table)):
        if L == 0:
            continue
        if (met >> c) & 1:
            n += L
            continue
        p = progress(state, c)
        q = transition(table[c], L, p, w)
        if q == L:
            met |= 1 << c
            n += L
            hit.add("completed")
            continue
        if p >= 1 and q == 0:
            hit.add("reset")
        if p >= 1 and 0 < q <= p:
            hit.add("fell_back")
        if c < 8:
            lo |= q << (4 * c)
        else:
            hi |= q << (4 * (c - 8))
        n += q
    if counts is not None:
        for name in hit:
            counts[name] += 1
    return (met, lo, hi, n)


def is_open(state, fin, table):
    """A row that is not finished and has a phrase with L_c > 0 that is not met."""
    return (not fin) and any(L > 0 and not (int(state[0]) >> c) & 1 for c, L in enumerate(lengths(table)))


def values(logps, base, prev, flags, open_rows):
    """c(j, w) = base_j + lp'(j, w) in float32, logps = M arrays (R, V).  Step 0: base = prev = None."""
    lp = np.array(ens_combine(logps), dtype=F32, copy=True)
    R = lp.shape[0]
    for j in range(R):
        if prev is not None and prev[j] == EOS:
            lp[j, :] = NEG_PEN
            lp[j, EOS] = 0.0
            continue
        if prev is not None:
            if not flags & ALLOW_REPEAT:
                lp[j, prev[j]] = NEG_PEN
            if flags & AVOID_UNK:
                lp[j, UNK] = NEG_PEN
        if open_rows[j]:
            lp[j, EOS] = NEG_PEN
    b = np.zeros(R, dtype=F32) if base is None else np.asarray(base, dtype=F32)
    return (b[:, None] + lp).astype(F32)


def best_first(cands):
    """Candidates (value, flat, bank) under (value descending, flat index ascending)."""
    return sorted(cands, key=lambda t: (-float(t[0]), t[1]))


def slot_order(cands, k):
    """The closed form: live candidates (value > -5e4) get rho = their rank within their bank and fill the slots in the order
    (rho ascending, bank descending); dead ones follow under (value descending, flat ascending).  Returns the first k."""
    live = [t for t in cands if F32(t[0]) > LIVE]
    dead = [t for t in cands if not F32(t[0]) > LIVE]
    keyed = []
    for bank in {t[2] for t in live}:
        for rho, t in enumerate(best_first([u for u in live if u[2] == bank])):
            keyed.append((rho, -bank, t))
    keyed.sort(key=lambda x: (x[0], x[1]))
    return ([t for _, _, t in keyed] + best_first(dead))[:k]


def round_robin(cands, k):
    """The loop slot_order abbreviates: the best unseen live candidate of each bank, highest bank first, repeated until the
    slots or the live candidates run out; then the dead ones."""
    live = best_first([t for t in cands if F32(t[0]) > LIVE])
    dead = best_first([t for t in cands if not F32(t[0]) > LIVE])
    out, left = [], list(live)
    while left and len(out) < k:
        for bank in sorted({t[2] for t in left}, reverse=True):
            pick = next(t for t in left if t[2] == bank)
            left.remove(pick)
            out.append(pick)
    return (out + dead)[:k]


def step(logps, base, prev, k, table, states, flags=0, counts=None, last=False):
    """One sentence, one expansion.  logps: M arrays (R, V) (R = 1 at step 0, else k); states: R tuples (ignored at step 0).
    last: the step di = max_len - 1, whose row the finish overwrites with EOS: every child keeps its parent's state.
    Returns (words (k,), parents (k,), scores (k,) float32, child states: k tuples)."""
    R, V = np.asarray(logps[0]).shape
    assert R in (1, k) and V >= k
    if prev is None:
        states = [ZERO] * R
    fin = [prev is not None and prev[j] == EOS for j in range(R)]
    opn = [is_open(states[j], fin[j], table) for j in range(R)]
    c = values(logps, base, prev, flags, opn)
    flat = np.arange(R * V)
    order = np.lexsort((flat, -c.ravel().astype(np.float64)))
    a = [int(f) for f in order[:k]]
    cc = [j * V + int(np.lexsort((np.arange(V), -c[j].astype(np.float64)))[0]) for j in range(R)]
    bb = []
    L = lengths(table)
    for j in range(R):
        if fin[j]:
            continue
        for ci in range(MAX_PHRASES):
            if L[ci] > 0 and not (int(states[j][0]) >> ci) & 1:
                w = int(table[ci][progress(states[j], ci)])
                if 1 <= w < V:
                    bb.append(j * V + w)
    ac = set(a) | set(cc)
    pool = sorted(ac | set(bb))
    cands = []
    for f in pool:
        j, w = f // V, f % V
        cands.append((c[j, w], f, child(states[j], fin[j] or last, w, table)[3]))
    chosen = slot_order(cands, k)
    words = np.array([t[1] % V for t in chosen], dtype=np.int64)
    parents = np.array([t[1] // V for t in chosen], dtype=np.int64)
    scores = np.array([t[0] for t in chosen], dtype=F32)
    new = [child(states[p], fin[p] or last, w, table, counts) for p, w in zip(parents.tolist(), words.tolist())]
    if counts is not None:
        picked = {t[1] for t in chosen}
        counts["b_outside"] += len((set(bb) - ac) & picked)
        counts["b_dedup"] += len(set(bb) & ac)
        counts["finished_kept"] += sum(1 for p in parents.tolist() if fin[p] and states[p][3] > 0)
        live = [t for t in chosen if F32(t[0]) > LIVE]
        counts["banks3"] += len({t[2] for t in live}) >= 3
        counts["dead_fill"] += len(live) < k
        if any(opn):
            # the same step with the rule lifted: (j, EOS) of an open row that the plain selection would have taken
            free = values(logps, base, prev, flags, [False] * R)
            top = np.lexsort((flat, -free.ravel().astype(np.float64)))[:k]
            counts["eos_ruled_out"] += sum(1 for f in top if int(f) % V == EOS and opn[int(f) // V])
    return words, parents, scores, new


def pack_states(states):
    return np.array(states, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(len(states), 4)


def search(fn, B, k, V, max_len, steps, required, flags=0, counts=None, prefix=None, phrases=(), phrase_sent=(), ngram=0,
           records=None):
    """A whole search: fn(previous words (N,) int64) -> M arrays (N, V) float32 (N = B at step 0, B k afterwards), masked by
    constrain_ref.mask when negative constraints are given, then expanded.  required: (B, 16, 8) int64.  Returns (beam
    (2 max_len, B, k) int64: words | parents, nll (B, k) float32, state (B, k, 4) int32); records (a list) receives a copy of
    (beam row, parent row, nll, state, n_alive) after every step."""
    beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
    nll = np.zeros((B, k), dtype=F32)
    states = [[ZERO] * k for _ in range(B)]
    constrained = prefix is not None or len(phrases) or ngram
    for di in range(steps):
        tok = np.full(B, SOS, dtype=np.int64) if di == 0 else beam[di - 1].reshape(-1)
        rows = [np.asarray(r, dtype=F32)[:, :V] for r in fn(tok)]
        if constrained:
            rows = constrain_ref.mask(rows, beam, di, max_len, B, k, V, prefix, phrases, phrase_sent, ngram)
        k_in = 1 if di == 0 else k
        alive = 0
        for b in range(B):
            lp = [r.reshape(B, k_in, V)[b] for r in rows]
            w, p, sc, new = step(lp, None if di == 0 else nll[b], None if di == 0 else beam[di - 1, b], k, required[b],
                                 states[b], flags, counts, last=di == max_len - 1)
            beam[di, b], beam[max_len + di, b], nll[b], states[b] = w, p, sc, new
            alive += int((w != EOS).sum())
        if records is not None:
            records.append((beam[di].copy(), beam[max_len + di].copy(), nll.copy(),
                            np.stack([pack_states(s) for s in states]), alive))
    return beam, nll, np.stack([pack_states(s) for s in states])


def table_of(phrase_lists, B):
    """(B, 16, 8) int64 from B lists of (phrase or None) entries; None leaves the entry unused."""
    t = np.zeros((B, MAX_PHRASES, MAX_LEN), dtype=np.int64)
    for b, lst in enumerate(phrase_lists):
        for c, ph in enumerate(lst):
            if ph:
                t[b, c, :len(ph)] = ph
    return t


def contains(h, ph):
    h, ph = [int(t) for t in h], [int(t) for t in ph]
    return any(h[i:i + len(ph)] == ph for i in range(len(h) - len(ph) + 1))
