"""NumPy float64 restatement of R-Drop as include/vag_nmt.h defines it (vag_rdrop_head_ce_seq_fwd, vag_rank_loss_fwd's kind | 2): the
per-row KL between twins, the per-row nll with label smoothing, loss_mt, d(loss_mt)/d(logits), and the twin-aware ranking loss.
Rows are time-major, r = t*Bt + b; the twin of r is r ^ 1 (Bt even); tgt is (Bt, Tt) with PAD = 0; w = [y != 0] unless given."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def rows_targets(tgt):
    """y (Tt*Bt,) of the time-major rows."""
    return np.asarray(tgt).T.reshape(-1)


def kl_rows(x):
    """x (R, V) logits, R even in pairs -> kl (R,): kl[r] = sum_j p_r[j] (lp_r[j] - lp_twin[j])."""
    lp = log_softmax(x)
    tw = lp.reshape(-1, 2, lp.shape[-1])[:, ::-1].reshape(lp.shape)
    return (np.exp(lp) * (lp - tw)).sum(-1)


def nll_rows(x, tgt, alpha, eps=0.0, w=None):
    """(nll (R,), kl (R,)): the smoothed nll of every row plus w_r (alpha / 4) (kl[r] + kl[twin])."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[-1]
    y = rows_targets(tgt)
    w = (y != 0).astype(np.float64) if w is None else np.asarray(w, dtype=np.float64)[y]
    lp = log_softmax(x)
    plain = -((1.0 - eps) * lp[np.arange(len(y)), y] + eps / V * lp.sum(-1))
    kl = kl_rows(x)
    both = kl.reshape(-1, 2).sum(-1).repeat(2)
    return w * (plain + alpha / 4.0 * both), kl


def loss_mt(nll, tgt):
    """mean over the Bt rows' sentences of sum_t nll / count."""
    tgt = np.asarray(tgt)
    Bt, Tt = tgt.shape
    cnt = (tgt != 0).sum(-1).astype(np.float64)
    return float((np.asarray(nll).reshape(Tt, Bt).sum(0) / cnt).mean())


def dlogits(x, tgt, alpha, eps=0.0, d_loss=1.0, w=None):
    """d(d_loss * loss_mt)/d x, (R, V): the closed form of the header."""
    x = np.asarray(x, dtype=np.float64)
    tgt = np.asarray(tgt)
    R, V = x.shape
    Bt, Tt = tgt.shape
    y = rows_targets(tgt)
    wv = (y != 0).astype(np.float64) if w is None else np.asarray(w, dtype=np.float64)[y]
    inv_cnt = 1.0 / (tgt != 0).sum(-1).astype(np.float64)
    coef = d_loss * np.tile(inv_cnt, Tt) / Bt * wv
    lp = log_softmax(x)
    p = np.exp(lp)
    sw = lambda a: a.reshape(R // 2, 2, *a.shape[1:])[:, ::-1].reshape(a.shape)      # noqa: E731
    kl = (p * (lp - sw(lp))).sum(-1)
    hot = np.zeros_like(x)
    hot[np.arange(R), y] = 1.0
    g = coef[:, None] * (p - (1.0 - eps) * hot - eps / V)
    c2 = alpha / 4.0 * (coef + sw(coef))
    return g + c2[:, None] * (p * ((lp - sw(lp)) - kl[:, None]) + p - sw(p))


def rank_loss_twins(im, s, margin, kind):
    """The ranking loss with the twin rule, unscaled: entries (i, j), i != j, of one pair (i >> 1 == j >> 1) enter neither hinge.
    kind 0: both hinges (PairwiseRankingLoss), 1: the first only (ImageRetrievalRankingLoss).  Returns (loss, G = d loss / d S)."""
    im, s = np.asarray(im, dtype=np.float64), np.asarray(s, dtype=np.float64)
    S = im @ s.T
    B = S.shape[0]
    loss, G = 0.0, np.zeros_like(S)
    for i in range(B):
        for j in range(B):
            if i == j or i >> 1 == j >> 1:
                continue
            hinges = [j] + ([i] if kind == 0 else [])
            for d in hinges:
                c = margin - S[d, d] + S[i, j]
                if c > 0:
                    loss += c
                    G[i, j] += 1.0
                    G[d, d] -= 1.0
    return loss, G


def rank_loss_plain(im, s, margin, kind):
    """The same without the twin rule (every i != j)."""
    im, s = np.asarray(im, dtype=np.float64), np.asarray(s, dtype=np.float64)
    S = im @ s.T
    d = np.diag(S)
    off = ~np.eye(S.shape[0], dtype=bool)
    loss = np.maximum(0.0, margin - d[None, :] + S)[off].sum()
    if kind == 0:
        loss += np.maximum(0.0, margin - d[:, None] + S)[off].sum()
    return float(loss)
