"""References for the language-model fusion (vagnmt_hip.lm; include/vag_nmt.h: vag_lm_fuse_rows, vag_lm_fuse_beam, vag_lm_query).

None of this is the trie code.  A model here is a dict from n-gram tuples (oldest word first) to (logp, bo) in float64 with ARPA's
recursion; the estimator is a brute-force interpolated Kneser-Ney from raw counts in Python dicts.

1. ``lm64``              lm(w | ctx) and the matched order by the recursion, float64.
2. ``kn_bruteforce``     interpolated Kneser-Ney as NgramLM.train documents it, from Counters.
3. ``fuse_row_fp32``     the kernel's arithmetic restated in fp32, operation for operation, with the catalogue's defects.
4. ``eps``               the per-element error bound, derived below, not tuned on the device.
5. ``beam_contexts``     the walk over a search buffer that gives every row's context.
6. the case tables of the GPU tests.

The bound.  u = 2^-24.  For one element the kernel forms, every operation rounded once,
    B = ((b_1 + b_2) + ...)           the k <= 4 back-offs of the stored longer contexts, longest first: k - 1 roundings
    t = lp + B,  s = beta * t,  out = x + s
from fp32 inputs lp, b_i (each within u of the float64 model's value, relatively) and beta (within u of the given double).
With a = |lp| and S = sum |b_i|, to first order in u:
    inputs       u a + u S
    B            (k - 1) u S <= 3 u S
    t            u (a + S)
    beta         u |beta| (a + S)                 (beta's own rounding, relative u on the product)
    s            u |beta| (a + S)                 (every line from B on is multiplied by |beta| on its way to out)
    out          u (|x| + |beta| (a + S))
so |out - exact| <= u (|x| + |beta| (5 a + 8 S)); the factor (1 + 2^-20) covers the second-order terms (at most 8 roundings).
The float64 reference's own error is 2^-29 of that.  x is the row's fp32 value, exact in both."""
import math
from collections import Counter

import numpy as np

U = 2.0 ** -24
UNK, SOS, EOS = 1, 2, 3
F32 = np.float32

DEFECTS = ("absent_bo_counted", "lower_overwrites", "bsum_off_by_one", "ctx_reversed", "last_successor_missed", "beta_on_model",
           "walk_follows_slot")


# ------------------------------------------------------------------------------------------------------------ the recursion
def clean_ctx(ctx, V, order):
    """The usable context, oldest first: the last order-1 entries, cut after the last entry that is no word of [0, V)."""
    ctx = [int(c) for c in ctx][-(order - 1):] if order > 1 else []
    for i in range(len(ctx) - 1, -1, -1):
        if not 0 <= ctx[i] < V:
            return ctx[i + 1:]
    return ctx


def lm64(grams, w, ctx):
    """(lm(w | ctx), matched order, a = |logp|, S = sum |bo| of the back-offs taken) by ARPA's recursion; ctx oldest first."""
    ctx = tuple(ctx)
    total, S = 0.0, 0.0
    while ctx:
        if ctx + (w,) in grams:
            lp = grams[ctx + (w,)][0]
            return total + lp, len(ctx) + 1, abs(lp), S
        if ctx in grams:
            total += grams[ctx][1]
            S += abs(grams[ctx][1])
        ctx = ctx[1:]
    lp = grams[(w,)][0]
    return total + lp, 1, abs(lp), S


def order_of(grams):
    return max(len(g) for g in grams)


def fuse_row64(grams, V, order, row, ctx, beta):
    """row[:V] + beta lm(. | ctx) in float64, the matched orders, and the bound eps per element."""
    c = clean_ctx(ctx, V, order)
    out = np.array(row, dtype=np.float64)
    matched = np.zeros(V, dtype=np.int32)
    bound = np.zeros(V)
    for w in range(V):
        v, n, a, S = lm64(grams, w, c)
        bound[w] = eps(float(row[w]), beta, a, S)
        out[w] = float(row[w]) + beta * v
        matched[w] = n
    return out, matched, bound


def eps(x, beta, a, S):
    return U * (abs(x) + abs(beta) * (5.0 * a + 8.0 * S)) * (1.0 + 2.0 ** -20)


# --------------------------------------------------------------------------------------------------- the fp32 restatement
def fuse_row_fp32(grams, V, order, row, ctx, beta, defect=None):
    """The kernel's arithmetic on one row, fp32, operation for operation: contexts resolved per suffix, back-off sums from the
    longest down, the successors of the longest stored context first, the unigrams last.  ``defect``: one of DEFECTS."""
    g32 = grams
    c = clean_ctx(ctx, V, order)
    if defect == "ctx_reversed":
        c = c[::-1]
    L = len(c)
    beta32 = F32(beta)
    node = [None] * (L + 1)                                    # node[j]: the suffix of j words, where stored
    for j in range(1, L + 1):
        s = tuple(c[L - j:])
        if s in g32 and not (defect == "last_successor_missed" and j >= 2 and is_last_successor(g32, s)):
            node[j] = s
    bo = [F32(0)] * (L + 1)
    for j in range(1, L + 1):
        if node[j] is not None:
            bo[j] = F32(g32[node[j]][1])
        elif defect == "absent_bo_counted":
            bo[j] = bo[j - 1]                                  # the value of the last context found
    bsum = [F32(0)] * (L + 2)
    acc = F32(0)
    for j in range(L, 0, -1):
        bsum[j] = acc
        if node[j] is not None or defect == "absent_bo_counted":
            acc = F32(acc + bo[j])
    bsum[0] = acc
    out = np.array(row, dtype=np.float32)
    claimed = np.zeros(V, dtype=bool)

    def term(lp, j):
        b = bsum[j + 1] if defect == "bsum_off_by_one" else bsum[j]
        return F32(beta32 * F32(F32(lp) + b))

    def write(w, t):
        if defect == "beta_on_model":
            out[w] = F32(F32(beta32 * out[w]) + F32(t / beta32))
        else:
            out[w] = F32(out[w] + t)

    x0 = np.array(row, dtype=np.float32)
    for j in range(L, 0, -1):
        if node[j] is None:
            continue
        succ = successors(g32, node[j])
        if defect == "last_successor_missed":
            succ = succ[:-1]
        for w in succ:
            if claimed[w] and defect != "lower_overwrites":
                continue
            if claimed[w]:
                out[w] = x0[w]
            claimed[w] = True
            write(w, term(g32[node[j] + (w,)][0], j))
    for w in range(V):
        if not claimed[w]:
            write(w, term(g32[(w,)][0], 0))
    return out


_SUCC = {}


def successors(grams, ctx):
    """Words w with ctx + (w,) stored, ascending (cached per model)."""
    table = _SUCC.get(id(grams))
    if table is None or table[0] is not grams:
        by = {}
        for g in grams:
            if len(g) >= 2:
                by.setdefault(g[:-1], []).append(g[-1])
        for v in by.values():
            v.sort()
        table = _SUCC[id(grams)] = (grams, by)
    return table[1].get(tuple(ctx), [])


def is_last_successor(grams, gram):
    s = successors(grams, gram[:-1])
    return bool(s) and s[-1] == gram[-1]


# ------------------------------------------------------------------------------------------------ brute-force Kneser-Ney
def kn_bruteforce(sentences, V, order):
    """Interpolated Kneser-Ney as NgramLM.train documents it -> {n-gram: (logp, bo)}; bo is 0.0 at the top order and for a
    stored n-gram with no successor."""
    sents = [[SOS] + [int(t) for t in s] + [EOS] for s in sentences]
    raw = [Counter() for _ in range(order + 1)]
    for s in sents:
        for n in range(1, order + 1):
            for i in range(len(s) - n + 1):
                raw[n][tuple(s[i:i + n])] += 1
    adj = [None] * (order + 1)
    adj[order] = dict(raw[order])
    for n in range(order - 1, 0, -1):
        a = Counter()
        for g in raw[n + 1]:
            a[g[1:]] += 1                                       # one more distinct predecessor
        for g, c in raw[n].items():
            if g[0] == SOS and n > 1:
                a[g] = c                                        # nothing precedes SOS: the count itself
        adj[n] = dict(a)
    adj[1].pop((SOS,), None)

    def discount(counts):
        n1 = sum(1 for c in counts if c == 1)
        n2 = sum(1 for c in counts if c == 2)
        return n1 / (n1 + 2.0 * n2) if n1 and n2 else 0.5

    prob = [None, {}]
    total = float(sum(adj[1].values()))
    D = discount(adj[1].values())
    for w in range(V):
        c = adj[1].get((w,), 0)
        prob[1][(w,)] = (max(c - D, 0.0) / total + D * len(adj[1]) / total / V) if total else 1.0 / V
    gammas = {}
    for n in range(2, order + 1):
        D = discount(adj[n].values())
        ctot, size = Counter(), Counter()
        for g, c in adj[n].items():
            ctot[g[:-1]] += c
            size[g[:-1]] += 1
        prob.append({})
        for h in ctot:
            gammas[h] = D * size[h] / ctot[h]
        for g, c in adj[n].items():
            prob[n][g] = (c - D) / ctot[g[:-1]] + gammas[g[:-1]] * prob[n - 1][g[1:]]
    grams = {}
    for n in range(1, order + 1):
        for g, p in prob[n].items():
            grams[g] = (math.log(p), math.log(gammas[g]) if g in gammas else 0.0)
    return grams


def to_arrays(grams, order):
    """The dict as NgramLM.from_ngrams takes it: (uni_logp, uni_bo, rows, logp, bo); V = the number of unigrams."""
    V = sum(1 for g in grams if len(g) == 1)
    uni_logp = np.array([grams[(w,)][0] for w in range(V)])
    uni_bo = np.array([grams[(w,)][1] for w in range(V)])
    rows, logp, bo = [], [], []
    for n in range(2, order + 1):
        gs = [g for g in grams if len(g) == n]
        rows.append(np.array(gs, dtype=np.int64).reshape(-1, n))
        logp.append(np.array([grams[g][0] for g in gs]))
        if n < order:
            bo.append(np.array([grams[g][1] for g in gs]))
    return uni_logp, uni_bo, rows, logp, bo


def round_fp32(grams):
    """The model the device holds: every value rounded to fp32 (returned as float64 numbers)."""
    return {g: (float(F32(v[0])), float(F32(v[1]))) for g, v in grams.items()}


# ------------------------------------------------------------------------------------------------------- the case tables
CHAIN = (10, 11, 12, 13)       # the fully seen context
LEAF = (20, 21, 22, 23)        # stored, no successors
BIG = (14, 15, 16, 17)         # a node with more successors than the workgroup has threads
FAR = (33, 34, 35, 36)         # words nothing follows
KINDS = ("empty", "short", "full", "last_only", "unseen", "leaf", "big")
BIG_SUCCESSORS = 300

# (name, V, ld, order, M, R): R = 7 runs every kind of context, R = 1 the one named
DENSE_CASES = [
    ("v37_o2_m1_r7", 37, 37, 2, 1, 7),
    ("v37_o3_m3_r7", 37, 41, 3, 3, 7),
    ("v37_o5_m1_r1_full", 37, 37, 5, 1, 1),
    ("v503_o2_m3_r1_big", 503, 504, 2, 3, 1),
    ("v503_o3_m1_r7", 503, 504, 3, 1, 7),
    ("v503_o5_m3_r7", 503, 504, 5, 3, 7),
    ("v2049_o3_m1_r7", 2049, 2049, 3, 1, 7),
    ("v2049_o5_m1_r1_big", 2049, 2052, 5, 1, 1),
    ("v2049_o2_m3_r7", 2049, 2051, 2, 3, 7),
]


def case_model(V, order, seed=0):
    """A model with arbitrary finite values (the kernels do not need a normalised one) that holds every structure KINDS names."""
    rng = np.random.default_rng(seed)
    grams = {}

    def val():
        return (-float(rng.uniform(0.5, 9.0)), -float(rng.uniform(0.05, 2.5)))

    def add(g):
        for n in range(1, len(g) + 1):
            if tuple(g[:n]) not in grams:
                grams[tuple(g[:n])] = val()

    for w in range(V):
        add((w,))
    nc = order - 1
    pool = [w for w in range(4, V) if w not in FAR]
    for ctx, many in ((CHAIN[:nc], min(12, V // 3)), (BIG[:nc], BIG_SUCCESSORS if V > BIG_SUCCESSORS + 8 else min(24, V // 2))):
        add(ctx)
        for j in range(1, nc + 1):                              # every suffix is a context with successors of its own; they overlap
            s = ctx[nc - j:]
            add(s)
            n = many if j == nc else min(12, V // 3) + 2 * j
            for w in rng.choice(pool, size=n, replace=False):
                if len(s) + 1 <= order:
                    add(s + (int(w),))
            add(s + (V - 1,))                                   # the last word of the vocabulary, last of its range
    leaf = LEAF[:nc]
    add(leaf)
    for j in range(1, nc):
        for w in rng.choice(pool, size=5, replace=False):
            add(leaf[nc - j:] + (int(w),))
    for _ in range(30):                                         # noise under parents the kinds do not use
        n = int(rng.integers(2, order + 1))
        g = tuple(int(x) for x in rng.integers(24, 30, size=n - 1)) + (int(rng.choice(pool)),)
        add(g)
    assert not successors(grams, leaf) or nc == 0
    return grams


def case_contexts(V, order, R, name=""):
    """(R, order-1) int32 contexts, the most recent word last, -1 = no word."""
    nc = order - 1

    def left(words):
        return [-1] * (nc - len(words)) + list(words)

    kinds = {
        "empty": left([]),
        "short": left(CHAIN[:nc][-1:]) if nc > 1 else left([24]),
        "full": left(CHAIN[:nc]),
        "last_only": left(list(FAR[:nc - 1]) + [CHAIN[nc - 1]]),
        "unseen": left(FAR[:nc]),
        "leaf": left(LEAF[:nc]),
        "big": left(BIG[:nc]),
    }
    if R == len(KINDS):
        rows = [kinds[k] for k in KINDS]
    else:
        rows = [kinds[next(k for k in KINDS if name.endswith(k))]] * R
    return np.array(rows, dtype=np.int32).reshape(R, nc)


def case_rows(V, ld, M, R, seed):
    """M poisoned matrices: log-probability-like values in [0, V), NaN in [V, ld) and in a guard band of 8 after every matrix."""
    rng = np.random.default_rng(seed + 100)
    out = []
    for _ in range(M):
        a = np.full(R * ld + 8, np.nan, dtype=np.float32)
        body = a[:R * ld].reshape(R, ld)
        body[:, :V] = -rng.uniform(0.01, 14.0, size=(R, V)).astype(np.float32)
        out.append(a)
    return out


# ------------------------------------------------------------------------------------------------------------ the beam walk
BEAM_CASE = dict(B=3, k=6, max_len=10, steps=(0, 1, 2, 7), V=503)


def beam_case(seed=4):
    """A search buffer (2 max_len, B, k) int64 -- words, then back-pointers -- with back-pointers that cross slots, an EOS in some
    slots and a back-pointer outside [0, k) that the walk must clamp."""
    c = BEAM_CASE
    rng = np.random.default_rng(seed)
    B, k, ml = c["B"], c["k"], c["max_len"]
    words = rng.integers(4, 40, size=(ml, B, k)).astype(np.int64)
    words[:, :, :] = np.where(rng.uniform(size=words.shape) < 0.5, rng.choice([10, 11, 12, 13, 14, 15], size=words.shape), words)
    parent = np.stack([np.stack([rng.permutation(k) for _ in range(B)]) for _ in range(ml)]).astype(np.int64)
    parent[:, :, 0] = parent[:, :, 1]                            # two slots share a parent
    words[0, 1, 2] = EOS
    words[1, 0, 3] = EOS
    words[6, 2, 1] = EOS
    parent[6, 0, 4] = k + 3                                      # clamped to k - 1
    parent[1, 2, 5] = -2                                         # clamped to 0
    assert any(np.any(parent[t] != np.arange(k)[None, :]) for t in range(ml))
    return np.concatenate([words, parent])


def beam_contexts(beam, di, B, k, max_len, order, V, defect=None):
    """Per row of step di (B rows at step 0, B k afterwards): the context (order-1 int32, most recent last, -1 = none) the walk
    gives, and whether the row is finished (its previous word is EOS)."""
    nc = order - 1
    k_in = 1 if di == 0 else k
    ctx = np.full((B * k_in, nc), -1, dtype=np.int32)
    done = np.zeros(B * k_in, dtype=bool)
    for n in range(B * k_in):
        b, s = divmod(n, k_in)
        t = di - 1
        for i in range(nc):
            if t >= 0:
                w = int(beam[t, b, s])
                p = int(beam[max_len + t, b, s])
                ctx[n, nc - 1 - i] = w if 0 <= w < V else -1
                if defect != "walk_follows_slot":
                    s = min(max(p, 0), k - 1)
            elif t == -1:
                ctx[n, nc - 1 - i] = SOS
            t -= 1
        done[n] = di >= 1 and ctx[n, nc - 1] == EOS
    return ctx, done
