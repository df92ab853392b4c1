"""NumPy references of kNN-MT (include/vag_nmt.h: vag_knn_store_rows, vag_knn_search, vag_knn_mix), in float64, with the
stored-key rounding and the total order restated; an fp32 restatement of the search kernel's arithmetic; the error bounds the GPU
tests accept against; and a catalogue of subtle defects the bounds must reject (tests/test_knn_host.py).

The arithmetic of the search kernel, restated (csrc/knn.hip):
  * a stored key is bf16 (8 significand bits), round to nearest even; its norm is an fp32 array the search reads;
  * a query value is split into three bf16 planes q1 = bf16(q), q2 = bf16(q - q1), q3 = bf16(q - q1 - q2): both differences
    are exact in fp32 and the part left over is below 2^-27 |q| (three roundings of relative half-ulp 2^-9);
  * every product plane x key is exact in fp32 (8 x 8 bits); they are accumulated in fp32 by one matrix instruction per
    (k-step of 16 depth values, plane), n_mfma = 3 ceil(D / 16) instructions, each adding 16 products to the running sum;
  * s = fma(2, acc, -norm): 2 acc is exact, one rounding.
Bound of one score.  With A = sum_i |q_i| |k_i|: the planes' left-over contributes 2^-27 A.  How a matrix instruction orders its 17
additions (16 products and the running sum) is not documented; it is taken to round every one of them once to nearest (unit
roundoff 2^-24, fp32 accumulation with nothing wider inside, as the f32-input instruction is documented to do) in WHATEVER order,
and every absolute partial sum is at most (1 + 2^-8) A, so acc is within n_mfma 17 2^-24 (1 + 2^-8) A + 2^-27 A of the exact
product; the last rounding adds 2^-24 |s|.  Hence
    eps(q, k) = 2 A (17 n_mfma 2^-24 (1 + 2^-8) + 2^-27) + 2^-24 |s| + 2^-126.
The restatement below adds the 16 products one by one, the longest chain such an instruction can have.
"""
import numpy as np

NEG = -1e5                    # the search's "ruled out"
MAX_K = 32


# ------------------------------------------------------------------------------------------------------------------ store
def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 bit patterns -> float32 values."""
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def span_end(row):
    """Last position of the scored span of a target row: the first EOS (3), else the last non-pad word, else -1."""
    row = np.asarray(row)
    e = np.nonzero(row == 3)[0]
    if len(e):
        return int(e[0])
    nz = np.nonzero(row != 0)[0]
    return int(nz[-1]) if len(nz) else -1


def store_rows(h2, tgt, sent_base=0, defect=None):
    """h2 (Tt, B, H) float32, tgt (B, Tt) -> dict(keys uint16 (n, H), norm float64 (n), value, sentence, position, count), entries in
    the order sentence b, then position t.  norm is the float64 sum of the ROUNDED key's squares (the device's fp32 norm is compared
    within norm_bound).  defect "norm_unrounded": the norm of the key before it was rounded."""
    Tt, B, H = h2.shape
    keys, norm, val, sen, pos = [], [], [], [], []
    for b in range(B):
        for t in range(span_end(tgt[b]) + 1):
            bits = bf16_bits(h2[t, b])
            keys.append(bits)
            src = h2[t, b] if defect == "norm_unrounded" else bf16_value(bits)
            norm.append(float(np.sum(src.astype(np.float64) ** 2)))
            val.append(int(tgt[b, t])); sen.append(sent_base + b); pos.append(t)
    n = len(keys)
    return dict(keys=np.array(keys, dtype=np.uint16).reshape(n, H), norm=np.array(norm, dtype=np.float64),
                value=np.array(val, dtype=np.int32), sentence=np.array(sen, dtype=np.int32), position=np.array(pos, dtype=np.int32),
                count=n)


def norm_bound(norm64, H):
    """|fp32 norm - float64 norm|: H exact-product fmas and a 6-level tree, each one rounding of 2^-24 of a partial sum <= norm."""
    return (H + 8) * 2.0 ** -24 * np.asarray(norm64) + 2.0 ** -126


# ----------------------------------------------------------------------------------------------------------------- search
def scores64(q, key_bits, norm):
    """s[r, i] = 2 q_r . k_i - norm[i] in float64 from the stored keys and the stored (fp32) norms."""
    k = bf16_value(key_bits).astype(np.float64)
    return 2.0 * (np.asarray(q, dtype=np.float64) @ k.T) - np.asarray(norm, dtype=np.float64)[None, :]


def n_mfma(D):
    return 3 * ((D + 15) // 16)


def score_eps(q, key_bits, s64):
    """eps[r, i] of the module docstring."""
    k = np.abs(bf16_value(key_bits).astype(np.float64))
    A = np.abs(np.asarray(q, dtype=np.float64)) @ k.T
    D = q.shape[1]
    return 2.0 * A * (17 * n_mfma(D) * 2.0 ** -24 * (1 + 2.0 ** -8) + 2.0 ** -27) + 2.0 ** -24 * np.abs(s64) + 2.0 ** -126


def rank_order(s, tie="asc"):
    """Indices of one row's scores under the total order: score descending, index ascending (defect tie="desc": descending)."""
    idx = np.arange(len(s))
    return np.lexsort((idx if tie == "asc" else -idx, -np.asarray(s)))


def search(q, key_bits, norm, K, defect=None):
    """-> (score (R, K) float64, index (R, K) int32): every row's K' = min(K, N) best, ranked; places past K' hold (-inf, -1).
    defect "tie_desc": ties broken by the larger index."""
    s = scores64(q, key_bits, norm)
    R, N = s.shape
    Kp = min(K, N)
    out_s = np.full((R, K), -np.inf)
    out_i = np.full((R, K), -1, dtype=np.int32)
    for r in range(R):
        o = rank_order(s[r], "desc" if defect == "tie_desc" else "asc")[:Kp]
        out_s[r, :Kp], out_i[r, :Kp] = s[r, o], o
    return out_s, out_i


def split3(q):
    """The three bf16 planes of a float32 array, as float32 values."""
    q = np.asarray(q, dtype=np.float32)
    p1 = bf16_round(q)
    r1 = (q - p1).astype(np.float32)
    p2 = bf16_round(r1)
    p3 = bf16_round((r1 - p2).astype(np.float32))
    return p1, p2, p3


def scores_fp32(q, key_bits, norm):
    """The kernel's arithmetic in fp32: planes, k-steps of 16 in order, per (k-step, plane) the 16 exact products added to the
    running sum one by one in fp32 (the matrix instruction's own inner order is not documented: this is its longest chain, and
    any order of one-rounding additions lies inside score_eps), then fma(2, acc, -norm)."""
    q = np.asarray(q, dtype=np.float32)
    R, D = q.shape
    k = bf16_value(key_bits)
    N = k.shape[0]
    Dp = (D + 15) // 16 * 16
    planes = [np.pad(p, ((0, 0), (0, Dp - D))) for p in split3(q)]
    kp = np.pad(k, ((0, 0), (0, Dp - D)))
    acc = np.zeros((R, N), dtype=np.float32)
    for ks in range(Dp // 16):
        for p in planes:
            for d in range(16 * ks, 16 * ks + 16):
                acc = (acc + (p[:, d:d + 1] * kp[None, :, d]).astype(np.float32)).astype(np.float32)
    s = 2.0 * acc.astype(np.float64) - np.asarray(norm, dtype=np.float32).astype(np.float64)[None, :]
    return s.astype(np.float32)


def check_search(got_s, got_i, q, key_bits, norm, K):
    """The acceptance of the GPU test for every row, with t the reference's K'-th score and eps the row's largest bound: every
    entry with s64 > t + 2 eps is returned, nothing with s64 < t - 2 eps is, returned scores lie within eps of s64, the ranking is
    the reference's wherever adjacent reference scores differ by more than 2 eps.  Returns the list of failures (empty: accepted)."""
    s = scores64(q, key_bits, norm)
    eps = score_eps(q, key_bits, s)
    R, N = s.shape
    Kp = min(K, N)
    bad = []
    for r in range(R):
        o = rank_order(s[r])
        t, e = s[r, o[Kp - 1]], float(eps[r].max())
        gi = np.asarray(got_i[r])
        if not (np.all(gi[Kp:] == -1) and np.all(np.isneginf(np.asarray(got_s[r], dtype=np.float64)[Kp:]))):
            bad.append((r, "places past K' are not (-inf, -1)"))
        gi = gi[:Kp]
        if np.any(gi < 0) or np.any(gi >= N) or len(set(gi.tolist())) != Kp:
            bad.append((r, "indices invalid or repeated", gi.tolist()))
            continue
        must = set(np.nonzero(s[r] > t + 2 * e)[0].tolist())
        if not must <= set(gi.tolist()):
            bad.append((r, "missing", sorted(must - set(gi.tolist()))))
        if np.any(s[r, gi] < t - 2 * e):
            bad.append((r, "returned an entry below the K'-th", gi.tolist()))
        if np.any(np.abs(np.asarray(got_s[r][:Kp], dtype=np.float64) - s[r, gi]) > eps[r, gi]):
            bad.append((r, "score outside eps", float(np.abs(np.asarray(got_s[r][:Kp], dtype=np.float64) - s[r, gi]).max())))
        place = {int(i): j for j, i in enumerate(gi.tolist())}
        for j in range(Kp - 1):
            a, b = int(o[j]), int(o[j + 1])
            if s[r, a] - s[r, b] > 2 * e and a in place and b in place and place[a] > place[b]:
                bad.append((r, "ranking differs at place %d" % j))
    return bad


def kth_gap(q, key_bits, norm, K):
    """Per row (gap between the K'-th and the (K'+1)-th reference score, the row's largest eps); gap = inf when N <= K."""
    s = scores64(q, key_bits, norm)
    eps = score_eps(q, key_bits, s)
    R, N = s.shape
    Kp = min(K, N)
    srt = -np.sort(-s, axis=1)
    gap = srt[:, Kp - 1] - srt[:, Kp] if N > Kp else np.full(R, np.inf)
    return gap, eps.max(axis=1)


# -------------------------------------------------------------------------------------------------------------------- mix
def host_scalars(lam, T):
    """(1 / T, log lam, log1p(-lam)) formed in double and rounded once to fp32, as the callers pass them."""
    return np.float32(1.0 / T), np.float32(np.log(lam)), np.float32(np.log1p(-lam))


def knn_probs(nb_score, nb_index, values, V, T, defect=None):
    """One row's neighbour distribution: dict word -> p_knn.  An index < 0 or a word outside [0, V) is no neighbour.
    defect "no_max_shift": the weights exp(s / T) without the shift by the largest score."""
    s = np.asarray(nb_score, dtype=np.float64)
    idx = np.asarray(nb_index)
    ok = (idx >= 0) & (idx < len(values))
    words = np.where(ok, np.asarray(values)[np.clip(idx, 0, len(values) - 1)], -1)
    ok &= (words >= 0) & (words < V)
    if not ok.any():
        return {}
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(ok, np.exp((s - (0.0 if defect == "no_max_shift" else s[ok].max())) / T), 0.0)
        w = w / w.sum()
    out = {}
    for j in np.nonzero(ok)[0]:
        out[int(words[j])] = out.get(int(words[j]), 0.0) + float(w[j])
    return out


def mix_row(row, nb_score, nb_index, values, V, lam, T, lse=0.0, defect=None):
    """One member's row (ldl values; only [0, V) is read) -> the mixed log-probabilities of [0, V) in float64 (columns past V are
    returned as they were).  defects: "no_max_shift", "one_by_one" (same-word neighbours mixed one after the other instead of
    summed), "no_log1m" (log(1 - lam) missing on the words no neighbour carries), "past_v" (column V rewritten too)."""
    out = np.array(row, dtype=np.float64)
    x = out[:V] - float(lse)
    l1m = np.log1p(-lam)
    mixed = x + (0.0 if defect == "no_log1m" else l1m)
    if defect == "past_v" and len(out) > V:
        out[V] = out[V] - float(lse) + l1m
    if defect == "one_by_one":
        s = np.asarray(nb_score, dtype=np.float64)
        idx = np.asarray(nb_index)
        ok = idx >= 0
        w = np.where(ok, np.exp((s - s[ok].max()) / T), 0.0)
        w = w / w.sum()
        for j in np.nonzero(ok)[0]:
            wd = int(values[idx[j]])
            mixed[wd] = np.logaddexp(x[wd] + l1m, np.log(lam) + np.log(w[j]))       # each neighbour overwrites the word's mix
    else:
        for wd, p in knn_probs(nb_score, nb_index, values, V, T, defect).items():
            with np.errstate(divide="ignore", invalid="ignore"):
                mixed[wd] = np.logaddexp(x[wd] + l1m, np.log(lam) + np.log(p))
    out[:V] = mixed
    return out


def mix_bound(row, nb_score, V, lam, T, lse=0.0):
    """Bound of one row's mixed values computed in fp32 from EXACT inputs (the lists and rows the kernel is given), u = 2^-24:
      other words:   (x - lse) + log1m: two roundings and the rounded constant: 3 u (|x| + |lse| + |log1m|);
      neighbour words: the weights' arguments (s - s_max) / T carry 3 u |arg| (two roundings and the rounded 1 / T) and enter exp, whose
                     relative error is then 3 u |arg|_max + 2 u (expf within 2 ulp); the sums of at most 32 weights add 32 u each;
                     the ratio, logf, the add of log lam and the final log1p(exp()) form add 8 u relative to values of magnitude
                     <= |x| + |lse| + |log lam| + |log p|: in all  u (6 |arg|_max + 80) on the neighbour term and the other words'
                     bound on the model term; the log-sum of the two is 1-Lipschitz in each, so the bounds add."""
    u = 2.0 ** -24
    x = np.abs(np.asarray(row, dtype=np.float64)[:V])
    base = 3 * u * (x + abs(float(lse)) + abs(np.log1p(-lam))) + 2.0 ** -126
    s = np.asarray(nb_score, dtype=np.float64)
    s = s[np.isfinite(s)]
    arg = float((s.max() - s.min()) / T) if len(s) else 0.0
    return base + u * (6 * arg + 80) * (1.0 + abs(np.log(lam)) + arg) + 8 * u * (x + abs(float(lse)))


def mix_bound_from_search(eps_row, T):
    """What a score error of eps per neighbour adds to a mixed log-probability: the weights' arguments (s_j - s_max) / T move by at
    most 2 eps / T, so every weight ratio and p_knn move by a factor within exp(+-4 eps / T), log p_knn by 4 eps / T, and the mixed
    value, 1-Lipschitz in it, by no more."""
    return 4.0 * float(eps_row) / T


DEFECTS = ["norm_unrounded", "tie_desc", "no_max_shift", "one_by_one", "no_log1m", "past_v"]


# ------------------------------------------------------------------------------------- the GPU tests' inputs, made on the host
SLICE = 2048                  # VAG_KNN_SLICE: keys of one stage-1 workgroup (the GPU test compares it with vag_knn_slice())
ROW_TILE = 32                 # vag_knn_row_tile(D) for D <= 640

# (name, N, R, D, K, ldq, seed): N in {1, K - 1, one slice - 1, one slice + 1, 3 slices + 17}, R in {1, 12, one row tile + 1, 192},
# D in {8, 40, 256, 512}, K in {1, 8, 32}, a leading dimension larger than D.  The seeds are the first for which every row's gap
# at the K-th place exceeds 4 eps (tests/test_knn_host.py asserts it): the device's set must then equal the reference's.
SEARCH_CASES = [
    ("one_entry", 1, 1, 8, 1, 8, 0),
    ("fewer_than_k", 7, 12, 40, 8, 40, 0),
    ("fewer_than_k32", 31, 1, 8, 32, 8, 0),
    ("slice_minus_1", SLICE - 1, ROW_TILE + 1, 256, 8, 256, 8),
    ("slice_plus_1", SLICE + 1, 12, 512, 8, 520, 1),
    ("three_slices_17", 3 * SLICE + 17, 192, 40, 8, 48, 2),
    ("k1_two_slices", SLICE + 300, 12, 8, 1, 8, 0),
    ("k32_two_slices", SLICE + 300, 12, 40, 32, 40, 0),
]


def search_case(N, R, D, K, ldq, seed):
    """-> (q (R, ldq) float32 with NaN in the columns past D, key_bits (N, D) uint16, norm (N) float32 from the stored keys)."""
    rng = np.random.default_rng(1000 + seed)
    q = np.full((R, ldq), np.nan, dtype=np.float32)
    q[:, :D] = rng.standard_normal((R, D)).astype(np.float32)
    bits = bf16_bits(rng.standard_normal((N, D)).astype(np.float32))
    norm = np.sum(bf16_value(bits).astype(np.float64) ** 2, axis=1).astype(np.float32)
    return q, bits, norm


DUP_CASE = dict(N=2 * SLICE + 100, R=ROW_TILE + 8, D=40, K=8,
                a=[5, 300, SLICE + 1, 2 * SLICE + 3, 2 * SLICE + 99], b=[6, SLICE - 1, SLICE, SLICE + 7, 2 * SLICE + 50])


def duplicate_case(seed=0):
    """Exact duplicates: two small stored keys a and b, five copies each, spread over the first slice, its last and the next
    slice's first entry, the second slice and the tail slice; every other key is twice as long, so for every query row (two row
    tiles) the ten copies are the ten best and the K = 8 returned hold one whole group and three of the other: the K-th and the
    (K+1)-th place are copies of one key and only the index decides.  -> (q, key_bits, norm)."""
    c = DUP_CASE
    rng = np.random.default_rng(2000 + seed)
    q = rng.standard_normal((c["R"], c["D"])).astype(np.float32)
    bits = bf16_bits((2.0 * rng.standard_normal((c["N"], c["D"]))).astype(np.float32))
    ka = bf16_bits((0.05 * rng.standard_normal(c["D"])).astype(np.float32))
    kb = bf16_bits((0.05 * rng.standard_normal(c["D"])).astype(np.float32))
    bits[c["a"]] = ka
    bits[c["b"]] = kb
    norm = np.sum(bf16_value(bits).astype(np.float64) ** 2, axis=1).astype(np.float32)
    return q, bits, norm


def mix_case(V, ldl, M, K, kind, seed, raw):
    """Rows and neighbour lists of one mix test: 4 rows per member.  kind: "one_word" (all neighbours carry one word), "distinct"
    (all different), "mixed" (random words with repeats), "underflow" (a neighbour word whose model value is -1e5), "short" (K' = 3 <
    K: places past it hold (-inf, -1)).  raw: rows are raw logits and a log-sum-exp is given.  -> list of M dicts(row (4, ldl) float32 with
    NaN past V, lse (4) float32 or None, nb_score (4, K) float32, nb_index (4, K) int32, values int32)."""
    rng = np.random.default_rng(3000 + seed)
    Rr, Nv = 4, 50
    out = []
    for m in range(M):
        logits = (3.0 * rng.standard_normal((Rr, V))).astype(np.float32)
        lse = np.log(np.sum(np.exp(logits.astype(np.float64)), axis=1)).astype(np.float32)
        row = np.full((Rr, ldl), np.nan, dtype=np.float32)
        row[:, :V] = logits if raw else (logits.astype(np.float64) - lse[:, None].astype(np.float64)).astype(np.float32)
        if kind == "one_word":
            values = np.full(Nv, min(V - 1, 4), dtype=np.int32)
        elif kind == "distinct":
            values = (np.arange(Nv) % V).astype(np.int32)
        else:
            values = rng.integers(0, V, size=Nv).astype(np.int32)
        idx = np.stack([rng.permutation(Nv)[:K] for _ in range(Rr)]).astype(np.int32)
        if kind == "distinct":
            idx = (3 * np.arange(Rr)[:, None] + np.arange(K)[None, :]).astype(np.int32)      # consecutive entries, consecutive words
            if V < K:
                idx[:, V:] = -1                # (no more distinct words than the vocabulary holds)
        sc = -np.sort(rng.uniform(0.0, 60.0, size=(Rr, K)), axis=1).astype(np.float32) - np.float32(20.0)
        if kind == "short":
            idx[:, 3:] = -1
            sc[:, 3:] = -np.inf
        sc = np.where(idx < 0, -np.inf, sc).astype(np.float32)
        if kind == "underflow":
            for r in range(Rr):
                row[r, values[idx[r, 0]]] = NEG + (lse[r] if raw else 0.0)
        out.append(dict(row=row, lse=lse if raw else None, nb_score=sc, nb_index=idx, values=values))
    return out
