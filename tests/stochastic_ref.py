"""NumPy restatement of one step of stochastic beam search as include/vag_nmt.h states it (vag_beam_sbs_step): the yardstick of
tests/test_stochastic_host.py and tests/test_gpu_stochastic.py.  The noise is an argument.  The float32 roundings of c, g, d and
fl(G_j - g) are the definition's; everything transcendental, and what follows it, is float64 -- so the inputs of the
transcendental part are bit for bit the device's, and the device's result differs by its own few ulp per function only.

    step(logp, noise, base, prev, G, k, flags)     B sentences, one step, no shortcut: every candidate is transformed and ranked
    markov_search(T, B, k, steps, rng)             whole searches on a first-order Markov "model", numpy's own Gumbel noise
    exact_markov(T, steps, k)                      the leaves of that model, their probabilities and inclusion probabilities
    CASES / make_case(case)                        the shapes and inputs of the one-step tests (shared by the CPU and GPU tests)
"""
import itertools

import numpy as np

SOS, EOS, UNK = 2, 3, 1
NEG_PEN = np.float32(-1e5)
ALLOW_REPEAT, AVOID_UNK = 1, 2
F32, F64 = np.float32, np.float64
LN2 = np.float32(0.6931472)
ULPS = 16.0 * 2.0 ** -23


def model_values(logp, base, prev, flags=0):
    """c(j, w) = base_j + lp'(j, w) in float32, the diverse search's value.  logp (B, R, V); step 0: base = prev = None."""
    lp = np.array(logp, dtype=F32, copy=True)
    B, R, V = lp.shape
    if prev is None:
        return (np.zeros((B, R, 1), dtype=F32) + lp).astype(F32)
    prev = np.asarray(prev)
    bi, ji = np.nonzero(prev != EOS)
    if not flags & ALLOW_REPEAT:
        lp[bi, ji, prev[bi, ji]] = NEG_PEN
    if flags & AVOID_UNK:
        lp[bi, ji, UNK] = NEG_PEN
    bf, jf = np.nonzero(prev == EOS)
    lp[bf, jf, :] = NEG_PEN
    lp[bf, jf, EOS] = 0.0
    return (np.asarray(base, dtype=F32)[:, :, None] + lp).astype(F32)


def step(logp, noise, base, prev, G, k, flags=0):
    """B sentences, one step.  logp, noise (B, R, V) float32 (R = 1 at step 0, else k); base, G (B, R) float32 and prev (B, R)
    int, or None at step 0 (G = 0).  Returns a dict: words, parents (B, k); c (B, k) float32, the stored scores; gum (B, k)
    float64, the reference G~ of the chosen; tol (B, k), the bound on a device value's distance from it; exact (B, k) bool, where
    the device value must be the parent's G bit for bit (the row's arg-max child, the child of a finished row); parent_G (B, k)
    float32; comparable (B,) bool: no candidate outside the chosen k is within the two tolerances of one inside, so the chosen
    SET is decided; and the full (B, R, V) arrays c_all, g_all, gt_all, tol_all, exact_all, cand."""
    logp = np.asarray(logp, dtype=F32)
    B, R, V = logp.shape
    c = model_values(logp, base, prev, flags)
    fin = np.zeros((B, R), dtype=bool) if prev is None else np.asarray(prev) == EOS
    Gp = np.zeros((B, R), dtype=F32) if G is None else np.asarray(G, dtype=F32)
    g = (c + np.asarray(noise, dtype=F32)).astype(F32)
    Z = g.max(axis=2)
    d = (g - Z[:, :, None]).astype(F32)
    d64 = d.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l = np.where(d == 0, -np.inf, np.where(d > -LN2, np.log(-np.expm1(d64)), np.log1p(-np.exp(d64))))
        v = (Gp[:, :, None] - g).astype(F32).astype(F64) + l
        gt = Gp.astype(F64)[:, :, None] - np.maximum(v, 0.0) - np.log1p(np.exp(-np.abs(v)))
    mags = [np.broadcast_to(np.abs(Gp.astype(F64))[:, :, None], g.shape), np.abs(g.astype(F64)), np.abs(l), np.abs(v)]
    tol = ULPS * np.maximum.reduce([np.ones(g.shape)] + [np.where(np.isfinite(m), m, 0.0) for m in mags])
    exact = d == 0
    cand = np.ones((B, R, V), dtype=bool)
    if fin.any():                                          # a finished row: (j, EOS) alone, G~ = G_j, no noise
        bf, jf = np.nonzero(fin)
        cand[bf, jf, :] = False
        cand[bf, jf, EOS] = True
        gt[bf, jf, :] = -np.inf
        gt[bf, jf, EOS] = Gp[bf, jf].astype(F64)
        tol[bf, jf, :] = ULPS * np.maximum(1.0, np.abs(Gp[bf, jf].astype(F64)))[:, None]
        exact[bf, jf, :] = True
    flat = np.broadcast_to(np.arange(R * V)[None, :], (B, R * V))
    gtf, candf, tolf = gt.reshape(B, -1), cand.reshape(B, -1), tol.reshape(B, -1)
    order = np.lexsort((flat, -gtf, ~candf), axis=-1)      # candidates first, G~ descending, then flat index ascending
    top, rest = order[:, :k], order[:, k:]
    assert candf[np.arange(B)[:, None], top].all(), "fewer than k candidates"
    take = lambda a, ix: np.take_along_axis(a, ix, axis=1)     # noqa: E731
    lo = (take(gtf, top) - take(tolf, top)).min(axis=1)
    if rest.shape[1]:
        hi = np.where(take(candf, rest), take(gtf, rest) + take(tolf, rest), -np.inf).max(axis=1)
    else:
        hi = np.full(B, -np.inf)
    return dict(words=top % V, parents=top // V, c=take(c.reshape(B, -1), top), gum=take(gtf, top), tol=take(tolf, top),
                exact=take(exact.reshape(B, -1), top), parent_G=np.take_along_axis(Gp, top // V, axis=1), comparable=lo > hi,
                c_all=c, gt_all=gt, tol_all=tol, cand=cand, exact_all=exact, g_all=g)


# ---- the one-step cases ---------------------------------------------------------------------------------------------
# B = 3; k in {1, 5, 12}; V = 37 (one slice), 2048 + 37 (two slices: the row maximum spans slices) and 14400 (k = 12: 12 * 8 * 12 =
# 1152 > 1024 stage 1 winners, the block-scan path of stage 2); step 0 and a later step
CASES = [(3, k, V, di) for k in (1, 5, 12) for V in (37, 2048 + 37, 14400) for di in (0, 2)]


def case_seed(case):
    B, k, V, di = case
    return 100003 * V + 101 * k + di


def make_case(case):
    """The inputs of one case but the noise: logp (B, R, V) random log-softmax rows, base / G (B, k) and prev (B, k) with some
    rows finished (None at step 0), flags."""
    B, k, V, di = case
    rng = np.random.default_rng(case_seed(case))
    R = 1 if di == 0 else k
    x = (3.0 * rng.standard_normal((B, R, V))).astype(F32)
    x64 = x.astype(F64)
    logp = (x64 - np.log(np.exp(x64 - x64.max(2, keepdims=True)).sum(2, keepdims=True)) - x64.max(2, keepdims=True)).astype(F32)
    flags = (0, 3, 1)[(k + di) % 3]
    if di == 0:
        return dict(logp=logp, base=None, prev=None, G=None, flags=flags)
    base = (-20.0 * rng.random((B, k))).astype(F32)
    G = (base.astype(F64) + rng.gumbel(size=(B, k))).astype(F32)
    prev = rng.integers(0, V, size=(B, k))
    prev[rng.random((B, k)) < 0.3] = EOS
    if k > 1:
        prev[:, k - 1] = prev[:, 0]
    return dict(logp=logp, base=base, prev=prev, G=G, flags=flags)


# ---- a first-order Markov model ---------------------------------------------------------------------------------------
def markov_table(V=5, seed=3):
    """T (V, V) float32: log p(word | previous word), rows that sum to 1 in float64 up to float32 rounding."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((V, V))
    return (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(F32)


def exact_markov(T, steps, k):
    """The leaves after `steps` steps from SOS (a hypothesis that emitted EOS stays as it is), in float64: (leaves: list of word
    tuples, p (n,), incl (n,): the probability that the leaf is among k draws without replacement)."""
    V = T.shape[0]
    P = np.exp(T.astype(F64))
    P = P / P.sum(1, keepdims=True)
    leaves = {(): 1.0}
    for _ in range(steps):
        nxt = {}
        for y, p in leaves.items():
            if y and y[-1] == EOS:
                nxt[y + (EOS,)] = p
                continue
            prev = y[-1] if y else SOS
            for w in range(V):
                nxt[y + (w,)] = p * P[prev, w]
        leaves = nxt
    names = sorted(leaves)
    p = np.array([leaves[y] for y in names])
    p = p / p.sum()
    incl = np.zeros(len(names))
    for tup in itertools.permutations(range(len(names)), min(k, len(names))):
        q, left = 1.0, 1.0
        for i in tup:
            q *= p[i] / left
            left -= p[i]
        for i in tup:
            incl[i] += q
    return names, p, incl


def markov_search(T, B, k, steps, rng, flags=ALLOW_REPEAT):
    """B independent searches of `steps` steps on the table model with numpy's Gumbel noise: (hyps (B, k, steps) int, logp
    (B, k) float32, gum (B, k) float64, in slot order)."""
    V = T.shape[0]
    words, parents = [], []
    base = prev = G = None
    for di in range(steps):
        R = 1 if di == 0 else k
        logp = np.broadcast_to(T[SOS], (B, 1, V)) if di == 0 else T[prev]
        r = step(logp, rng.gumbel(size=(B, R, V)).astype(F32), base, prev, G, k, flags)
        words.append(r["words"]); parents.append(r["parents"])
        base, prev, G = r["c"], r["words"], r["gum"].astype(F32)
    return resolve(np.stack(words), np.stack(parents)), base, r["gum"]


def resolve(words, parents):
    """Histories through the back-pointers: words, parents (steps, B, k) -> (B, k, steps)."""
    steps, B, k = words.shape
    out = np.zeros((B, k, steps), dtype=np.int64)
    p = np.broadcast_to(np.arange(k)[None, :], (B, k)).copy()
    for t in range(steps - 1, -1, -1):
        out[:, :, t] = np.take_along_axis(words[t], p, axis=1)
        p = np.take_along_axis(parents[t], p, axis=1)
    return out
