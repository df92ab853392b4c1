"""Word-level distillation (include/vag_nmt.h: vag_kd_targets, vag_kd_head_ce_seq_fwd) restated in NumPy float64: the teacher's
sparse targets from the members' logits and log-sum-exp, a row's loss and a row's gradient with respect to its logits.  The order
is the library's total order: score descending, word ascending."""
import numpy as np


def scores(logits, lse, fp32=False):
    """s (R, V) from M members' logits [(R, V)] and lse [(R,)]: the mean of the members' probabilities in log space.  fp32 (M = 1
    only): float32(x) - float32(lse), the one IEEE subtraction the kernel performs, returned as float32."""
    if fp32:
        assert len(logits) == 1
        return np.asarray(logits[0], dtype=np.float32) - np.asarray(lse[0], dtype=np.float32)[:, None]
    x = np.stack([np.asarray(l, dtype=np.float64) - np.asarray(s, dtype=np.float64)[:, None] for l, s in zip(logits, lse)])
    mx = x.max(0)
    return mx + np.log(np.exp(x - mx).mean(0))


def targets(s, K, T):
    """idx (R, K) int32 -- the K best words of every row of s (value desc, word asc), best first -- and q (R, K) float64,
    q_k = exp((s_k - s_0) / T) / sum."""
    R, V = s.shape
    idx = np.empty((R, K), dtype=np.int32)
    for r in range(R):
        idx[r] = np.lexsort((np.arange(V), -s[r].astype(np.float64)))[:K]
    top = np.take_along_axis(s.astype(np.float64), idx.astype(np.int64), 1)
    e = np.exp((top - top[:, :1]) / T)
    return idx, e / e.sum(1, keepdims=True)


def nll_row(x, y, w, idx, q, lam):
    """w * (lse - (1 - lam) x[y] - lam sum_k q_k x[idx_k])"""
    x = np.asarray(x, dtype=np.float64)
    lse = x.max() + np.log(np.exp(x - x.max()).sum())
    return w * (lse - (1.0 - lam) * x[y] - lam * float(np.dot(q, x[idx])))


def dlogits_row(x, y, coef, idx, q, lam):
    """coef * (softmax - (1 - lam) [j == y] - lam sum_k q_k [j == idx_k])"""
    x = np.asarray(x, dtype=np.float64)
    p = np.exp(x - x.max())
    g = p / p.sum()
    g[y] -= 1.0 - lam
    np.subtract.at(g, np.asarray(idx, dtype=np.int64), lam * np.asarray(q, dtype=np.float64))
    return coef * g


def synth_targets(rng, tgt_rows, V, K):
    """Synthesised soft targets for rows with gold words tgt_rows (R,): random distinct words and random normalised q per row; rows
    0, 3, 6, .. contain their gold word (at a random place), rows 1, 4, .. do not, row 2 holds word V - 1 and row 5 word 0."""
    R = len(tgt_rows)
    idx = np.empty((R, K), dtype=np.int32)
    for r in range(R):
        y = int(tgt_rows[r])
        pool = np.setdiff1d(np.arange(V), [y])
        row = rng.choice(pool, size=K, replace=False)
        if r % 3 == 0:
            row[rng.integers(0, K)] = y
        if r == 2 and V - 1 not in row and y != V - 1:
            row[0] = V - 1
        if r == 5 and 0 not in row and y != 0:
            row[K - 1] = 0
        assert len(set(row.tolist())) == K
        idx[r] = row
    q = rng.uniform(0.05, 1.0, size=(R, K))
    q /= q.sum(1, keepdims=True)
    return idx, q.astype(np.float32)
