"""Word-level confidence of forced decoding (include/vag_nmt.h: vag_token_conf) restated in NumPy, WITH ITS OWN ERROR BOUND: per
position of the scored span the softmax entropy, the rank of the given word under the library's total order (score descending, word
ascending), the two best words; per sentence the eight values of `sent`.

Scores.  s_j = combine_m(logits_m[j] - lse_m) is tests/distill_ref.py's `scores`.  At M = 1 the kernel's s is ONE IEEE subtraction,
float32(x) - float32(lse), reproducible here bit for bit: the float64 reference then starts from exactly those numbers (ranks, best
words and token_logp are exact; the entropy's only errors are its own).  At M > 1 the reference is float64 throughout and the
kernel's s carries delta_s = 16 * 2^-24 * max(1, |s|), the allowance tests/test_gpu_distill.py gives a combined score (one
subtraction, expf, an M-term sum, logf and one add, each within about 2 ulp).

The entropy's bound, per position, with T = sum_j |p_j s_j| (u = 2^-24; constants from tests/ground_ref.py):
  summation       gamma(k) T, k = ceil(V / 256) + 16: a lane adds at most ceil(V / 256) + 3 products in column order (whole groups of
                  four, then one tail word), the wave tree has 6 levels, the waves add 3 more -- gamma_k is the theorem for ANY order
                  of k roundings, and one more covers the product p_j * s_j (fused or not);
  transcendental  EPS T: expf within a few ulp (EPS = 8 u is ground_ref's allowance for an exponential; no ROCm document on this
                  tree states a tighter figure for expf / logf, so none is cited);
  flushed p       V * 2^-126 * max_j |s_j| over finite s: a p_j below the smallest normal number may be flushed to 0;
  M > 1           sum_j delta_s(s_j) p_j |s_j + 1|: d(p s)/ds = p (s + 1), first order.
A word with p_j == 0 (s_j = -inf included) contributes exactly 0 to the value and to the bound.

The cases of tests/test_gpu_confidence.py live here too (tied_case, random_case, targets), so that the host test checks the bound at
exactly the inputs the device is tested at."""
import numpy as np

from distill_ref import scores
from ground_ref import EPS, U24, ULP, gamma

EOS = 3
SENT = 8
B, TT = 5, 6
VS = [5, 67, 1031, 2047]


def ceil4(v):
    return (v + 3) // 4 * 4


def delta_s(s):
    return 16 * U24 * np.maximum(1.0, np.abs(s))


# ---- the span ------------------------------------------------------------------------------------------------------------
def span_mask(tgt, past_eos=False):
    """keep (B, Tt) bool: non-pad positions up to and including the first EOS (to the last non-pad word if there is none).
    past_eos (a defect): the span runs to the last non-pad word whatever EOS it meets."""
    tgt = np.asarray(tgt)
    keep = np.zeros(tgt.shape, dtype=bool)
    for b, row in enumerate(tgt.tolist()):
        nz = [t for t, w in enumerate(row) if w != 0]
        end = row.index(EOS) if (EOS in row and not past_eos) else (nz[-1] if nz else -1)
        for t in range(end + 1):
            keep[b, t] = row[t] != 0
    return keep


# ---- one row -------------------------------------------------------------------------------------------------------------
def entropy_terms(s):
    """p_j s_j in float64 with the convention 0 * (-inf) = 0, and p."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(s)
        return np.where(p > 0, p * np.where(p > 0, s, 0.0), 0.0), p


def entropy_bound(s, V, M):
    s = np.asarray(s, dtype=np.float64)
    terms, p = entropy_terms(s)
    T = np.abs(terms).sum()
    fin = np.isfinite(s)
    bound = (gamma(-(-V // 256) + 16) + EPS) * T + V * 2.0 ** -126 * (np.abs(s[fin]).max() if fin.any() else 0.0)
    if M > 1:
        bound += float(np.where(p > 0, delta_s(np.where(fin, s, 0.0)) * p * np.abs(np.where(fin, s, 0.0) + 1.0), 0.0).sum())
    return float(bound)


def uniform_slack(V, x=0.5):
    """What a constant row of logits x may miss log V by BEFORE the entropy's own errors: its lse = x + log V is rounded to fp32 and
    so is s = x - lse, and dH/ds = -(s + 1) sum_j p_j = -(s + 1): u (|lse| + |s|) |1 - log V|."""
    return U24 * (abs(x + np.log(V)) + np.log(V)) * abs(1.0 - np.log(V))


def rank_of(s, y, ties_after=False):
    """#{j : s_j > s_y or (s_j == s_y and j < y)}; ties_after (a defect): ties are counted BEHIND the word (j > y)."""
    j = np.arange(len(s))
    tie = (s == s[y]) & ((j > y) if ties_after else (j < y))
    return int(((s > s[y]) | tie).sum())


def top2(s):
    order = np.lexsort((np.arange(len(s)), -np.asarray(s, dtype=np.float64)))
    return order[:2].astype(np.int32)


# ---- the whole call ------------------------------------------------------------------------------------------------------
def sentence_values(tgt, token_logp, entropy, rank, keep=None, ddof=0):
    """sent (B, 8) in float64 from the per-position values (any dtype): logp, score, n, std, min, mean entropy, max entropy,
    share of rank == 0.  ddof = 1 (a defect): the sample standard deviation."""
    tgt = np.asarray(tgt)
    keep = span_mask(tgt) if keep is None else keep
    out = np.zeros((tgt.shape[0], SENT))
    for b in range(tgt.shape[0]):
        k = keep[b]
        v, h = np.asarray(token_logp[b], dtype=np.float64)[k], np.asarray(entropy[b], dtype=np.float64)[k]
        n = int(k.sum())
        out[b, 0] = v.sum()
        out[b, 1] = v.sum() / max(1, int((tgt[b][k] > 3).sum()))
        out[b, 2] = n
        if n:
            out[b, 3] = np.sqrt(((v - v.mean()) ** 2).sum() / max(1, n - ddof))
            out[b, 4:8] = v.min(), h.mean(), h.max(), (np.asarray(rank[b])[k] == 0).mean()
    return out


def sentence_bounds(tgt, token_logp, entropy):
    """Bounds (B, 8) on |fp32 sentence value - sentence_values(...)| for values reduced from the SAME fp32 token_logp / entropy:
    n, min, max are exact (0) and so is the share up to its one division (u); a sum of n <= Tt numbers in position order is within
    gamma(Tt) sum|.|; the mean adds one division; the standard deviation: the mean's error e_m enters every deviation, so the
    variance is off by at most 2 std e_m + e_m^2 + gamma(Tt + 3) var, and sqrt(a + e) - sqrt(a) <= min(sqrt(e), e / sqrt(a))."""
    tgt = np.asarray(tgt)
    keep = span_mask(tgt)
    Tt = tgt.shape[1]
    out = np.zeros((tgt.shape[0], SENT))
    for b in range(tgt.shape[0]):
        k = keep[b]
        n = int(k.sum())
        if not n:
            continue
        v, h = np.asarray(token_logp[b], dtype=np.float64)[k], np.asarray(entropy[b], dtype=np.float64)[k]
        g = float(gamma(Tt + 1))
        out[b, 0] = g * np.abs(v).sum()
        out[b, 1] = out[b, 0] + U24 * np.abs(v).sum()
        e_m = g * np.abs(v).sum() / n
        var = ((v - v.mean()) ** 2).sum() / n
        e_var = 2 * np.sqrt(var) * e_m + e_m ** 2 + float(gamma(Tt + 3)) * var
        out[b, 3] = (min(np.sqrt(e_var), e_var / np.sqrt(var)) if var > 0 else np.sqrt(e_var)) + ULP * np.sqrt(var)
        out[b, 5] = g * np.abs(h).sum() / n
        out[b, 7] = U24
    return out


def reference(logits, lse, tgt, V):
    """The float64 reference of vag_token_conf for M members' logits [(Tt*B, >= V)] (time-major rows t*B + b) and lse [(Tt*B,)]:
    a dict of sentence-major arrays token_logp, entropy, bound (the entropy's), rank, top (.., 2), top_logp (.., 2), keep, and s
    (Tt*B, V) float64 -- at M = 1 the float32 scores the kernel forms, widened."""
    M = len(logits)
    tgt = np.asarray(tgt)
    Bn, Tt = tgt.shape
    x = [np.asarray(l)[:, :V] for l in logits]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = scores(x, lse, fp32=True).astype(np.float64) if M == 1 else scores(x, lse)
    keep = span_mask(tgt)
    r = dict(token_logp=np.zeros((Bn, Tt)), entropy=np.zeros((Bn, Tt)), bound=np.zeros((Bn, Tt)),
             rank=np.full((Bn, Tt), -1, dtype=np.int32), top=np.full((Bn, Tt, 2), -1, dtype=np.int32),
             top_logp=np.zeros((Bn, Tt, 2)), keep=keep, s=s)
    for b in range(Bn):
        for t in range(Tt):
            if not keep[b, t]:
                continue
            row, y = s[t * Bn + b], int(tgt[b, t])
            r["token_logp"][b, t] = row[y]
            r["entropy"][b, t] = -entropy_terms(row)[0].sum()
            r["bound"][b, t] = entropy_bound(row, V, M)
            r["rank"][b, t] = rank_of(row, y)
            r["top"][b, t] = top2(row)
            r["top_logp"][b, t] = row[r["top"][b, t]]
    return r


def restate_fp32(logits, lse, tgt, V, defect=None):
    """M = 1 in np.float32, as the kernel computes: s = float32(x) - float32(lse), p = exp(s) in float32, the products and their sum
    in float32 (numpy's pairwise order), a word of p == 0 adding 0.  Returns the same dict as `reference` plus sent (B, 8) float32.
    defect: one subtle mistake -- 'bits' (entropy in bits), 'padding' (the padding columns [V, ldl) join the row), 'ties_after',
    'past_eos', 'ddof'."""
    tgt = np.asarray(tgt)
    Bn, Tt = tgt.shape
    x = np.asarray(logits[0], dtype=np.float32)
    x = x if defect == "padding" else x[:, :V]
    with np.errstate(invalid="ignore"):
        s = x - np.asarray(lse[0], dtype=np.float32)[:, None]
    keep = span_mask(tgt, past_eos=defect == "past_eos")
    r = dict(token_logp=np.zeros((Bn, Tt), dtype=np.float32), entropy=np.zeros((Bn, Tt), dtype=np.float32),
             rank=np.full((Bn, Tt), -1, dtype=np.int32), top=np.full((Bn, Tt, 2), -1, dtype=np.int32),
             top_logp=np.zeros((Bn, Tt, 2), dtype=np.float32), keep=keep, s=s)
    for b in range(Bn):
        for t in range(Tt):
            if not keep[b, t]:
                continue
            row, y = s[t * Bn + b], int(tgt[b, t])
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.exp(row)
                terms = np.where(p == 0, np.float32(0), p * np.where(p == 0, np.float32(0), row)).astype(np.float32)
            h = -terms.sum(dtype=np.float32)
            r["token_logp"][b, t] = row[y]
            r["entropy"][b, t] = h / np.float32(np.log(2.0)) if defect == "bits" else h
            r["rank"][b, t] = rank_of(row, y, ties_after=defect == "ties_after")
            r["top"][b, t] = top2(row)
            r["top_logp"][b, t] = row[r["top"][b, t]]
    r["sent"] = sentence_values(tgt, r["token_logp"], r["entropy"], r["rank"], keep, ddof=1 if defect == "ddof" else 0).astype(np.float32)
    return r


# ---- the cases -----------------------------------------------------------------------------------------------------------
PEAKED, UNIFORM, NEG_INF = (0, 0), (0, 1), (4, 0)      # (b, t) of the three special rows of tied_case


def targets(V):
    """tgt (5, 6): b = 0 has words after its first EOS; b = 1 has no EOS, a pad INSIDE its span (not a span position) and a pad
    tail; b = 2 is all pad (n = 0); b = 3 is one word; b = 4 starts and goes on with word V - 1 and ends in EOS at the last place."""
    w = lambda i: 4 + i % (V - 4)          # noqa: E731  (words > 3 inside [0, V))
    return np.array([[w(0), 2, EOS, w(7), w(1), 0],
                     [w(2), 0, w(9), 1, 0, 0],
                     [0, 0, 0, 0, 0, 0],
                     [EOS, 0, 0, 0, 0, 0],
                     [V - 1, w(5), V - 1, 1, 2, EOS]], dtype=np.int64)


def _finish(x, V):
    with np.errstate(divide="ignore"):
        m = x[:, :V].astype(np.float64).max(1)
        lse = m + np.log(np.exp(x[:, :V].astype(np.float64) - m[:, None]).sum(1))
    return lse.astype(np.float32)


def tied_case(V, ldl=None):
    """M = 1: B * Tt = 30 rows of logits quantised to five levels (hundreds of exact ties at V >= 1031), the padding columns
    [V, ldl) filled with 99; row PEAKED has one column 80 above the rest, row UNIFORM is constant, row NEG_INF holds a -inf logit.
    Returns ([x (30, ldl) float32], [lse (30,) float32], tgt)."""
    ldl = ceil4(V) if ldl is None else ldl
    g = np.random.default_rng(V + 7 * ldl)
    x = np.full((B * TT, ldl), 99.0, dtype=np.float32)
    x[:, :V] = np.clip(np.round(g.normal(size=(B * TT, V)) * 1.5), -2, 2)
    row = lambda bt: bt[1] * B + bt[0]          # noqa: E731
    x[row(PEAKED), :V] = -1.0
    x[row(PEAKED), V // 2] = 79.0
    x[row(UNIFORM), :V] = 0.5
    x[row(NEG_INF), 1] = -np.inf
    return [x], [_finish(x, V)], targets(V)


def random_case(V, M, same=False):
    """M members of scales 1 + 0.5 m (tests/test_gpu_distill.py's ensemble); same: M copies of member 0."""
    g = np.random.default_rng(1000 * V + M)
    ldl = ceil4(V)
    xs = []
    for m in range(M):
        x = np.full((B * TT, ldl), 99.0, dtype=np.float32)
        x[:, :V] = g.normal(size=(B * TT, V)) * (1.0 + 0.5 * m)
        xs.append(x)
    if same:
        xs = [xs[0]] * M
    return xs, [_finish(x, V) for x in xs], targets(V)
