"""Plain NumPy / torch float64 restatement of the minimum-risk definitions of include/vag_nmt.h (vag_mrt_weights, vag_mrt_pack) and of
vagnmt_hip.mrt's cost (1 - the segment-level smooth BLEU of tests/mbr_ref.py against the gold sentence).  A test helper, not a
test."""
import numpy as np
import torch

import mbr_ref

EOS = 3


def weights(nll, cost, valid, N, alpha, scale):
    """nll (Tt, B), cost (B,), valid (B,) or None -> (inv_cnt (B,), q (B,), risk) in float64, from the inputs as given."""
    nll = np.asarray(nll, dtype=np.float64)
    cost = np.asarray(cost, dtype=np.float64)
    B = nll.shape[1]
    ok = np.ones(B, dtype=bool) if valid is None else np.asarray(valid) != 0
    G = B // N
    assert G * N == B
    s = -nll.sum(0)
    inv_cnt, q = np.zeros(B), np.zeros(B)
    total = 0.0
    for g in range(G):
        idx = [b for b in range(g * N, g * N + N) if ok[b]]
        if not idx:
            continue
        x = alpha * s[idx]
        e = np.exp(x - x.max())
        Q = e / e.sum()
        R = float((Q * cost[idx]).sum())
        q[idx] = Q
        inv_cnt[idx] = -scale * N * alpha * Q * (cost[idx] - R)
        total += R
    return inv_cnt, q, scale / G * total


def risk_torch(s, cost, valid, N, alpha):
    """The risk of a whole step as a differentiable float64 torch expression of the rows' scores s (B,): the mean over the groups of
    sum_i Q_i c_i, Q the softmax of alpha s over the group's valid rows."""
    B = s.shape[0]
    G = B // N
    cost = torch.as_tensor(np.asarray(cost), dtype=torch.float64)
    ok = torch.ones(B, dtype=torch.bool) if valid is None else torch.as_tensor(np.asarray(valid)) != 0
    total = 0.0
    for g in range(G):
        idx = torch.nonzero(ok[g * N:g * N + N]).flatten() + g * N
        if idx.numel() == 0:
            continue
        Q = torch.softmax(alpha * s[idx], 0)
        total = total + (Q * cost[idx]).sum()
    return total / G


def span(row):
    return mbr_ref.span(row)


def pack(cand, gold, include_gold, Tt=None):
    """cand (G, Nc, L), gold (G, Tg) integer arrays -> (tgt (G N, Tt) int64, valid (G N,) float32): every row its span, one EOS,
    zeros; the gold row first when included; a row is invalid when its span holds 0 or equals the span of an earlier valid row of
    its group."""
    cand, gold = np.asarray(cand), np.asarray(gold)
    G, Nc, L = cand.shape
    Tg = gold.shape[1]
    N = Nc + (1 if include_gold else 0)
    Tt = max(L + 1, Tg) if Tt is None else Tt
    assert Tt >= L + 1 and (not include_gold or Tt >= Tg)
    tgt = np.zeros((G * N, Tt), dtype=np.int64)
    valid = np.zeros(G * N, dtype=np.float32)
    for g in range(G):
        rows = ([gold[g]] if include_gold else []) + list(cand[g])
        seen = []
        for i, r in enumerate(rows):
            sp = span(r)[:Tt - 1]
            tgt[g * N + i, :len(sp)] = sp
            tgt[g * N + i, len(sp)] = EOS
            ok = 0 not in sp and sp not in seen
            if ok:
                seen.append(sp)
            valid[g * N + i] = 1.0 if ok else 0.0
    return tgt, valid


def bleu_cost(tgt, gold, N):
    """1 - smooth BLEU of every packed row against its group's gold row, float64 (G N,)."""
    tgt, gold = np.asarray(tgt), np.asarray(gold)
    G = gold.shape[0]
    m, lh, lr = mbr_ref.pairwise(tgt.reshape(G, N, -1), gold.reshape(G, 1, -1))
    return 1.0 - mbr_ref.utilities(m, lh, lr, "bleu")[:, :, 0].reshape(-1)


def edge_case():
    """One group of candidates that meets every rule of the pack (L = 6, Tg = 6): the gold sentence sampled again, a repeated
    sample, a span without EOS at full length, an empty span (twice: the second is a repeat), a span holding 0 and its repeat.
    Returns (cand (1, 8, 6), gold (1, 6), the expected valid with the gold row included, and without it)."""
    gold = np.array([[10, 11, 12, 3, 0, 0]], dtype=np.int64)
    cand = np.array([[[10, 11, 12, 3, 7, 7],        # the gold sentence (what follows its EOS is not content)
                      [20, 21, 3, 0, 0, 0],
                      [20, 21, 3, 9, 9, 3],         # a repeat of the row above
                      [30, 31, 32, 33, 34, 35],     # no EOS: the whole row
                      [3, 5, 5, 5, 5, 5],           # empty
                      [3, 0, 0, 0, 0, 0],           # empty again
                      [40, 0, 41, 3, 0, 0],         # holds the padding word
                      [40, 0, 41, 3, 0, 0]]], dtype=np.int64)
    with_gold = np.array([1, 0, 1, 0, 1, 1, 0, 0, 0], dtype=np.float32)
    without = np.array([1, 1, 0, 1, 1, 0, 0, 0], dtype=np.float32)
    return cand, gold, with_gold, without


# ------------------------------------------------------------------------------------------------------------------
# "it learns": five minimum-risk steps on one batch with a fixed candidate set, in float64 on the oracle
# ------------------------------------------------------------------------------------------------------------------
LEARN = {"golden": "text_tied_s0_f32", "alpha": 0.5, "lr": 2e-3, "seed": 5, "Nc": 3, "L": 5, "steps": 5}


def learn_candidates(tgt, Vt):
    """The fixed candidates of the learning case, (B, Nc, L) int64: random words of the target vocabulary with an EOS somewhere in
    most rows; the first candidate of every sentence shares the gold sentence's first words (a partial match: costs differ)."""
    g = np.random.default_rng(LEARN["seed"])
    tgt = np.asarray(tgt)
    B = tgt.shape[0]
    Nc, L = LEARN["Nc"], LEARN["L"]
    c = g.integers(4, Vt, size=(B, Nc, L)).astype(np.int64)
    for b in range(B):
        gs = span(tgt[b])
        k = min(len(gs), 2)
        c[b, 0, :k] = gs[:k]
        for i in range(Nc):
            e = int(g.integers(1, L + 1))
            if e < L:
                c[b, i, e] = EOS
    return c


def learn_reference(P, src, lengths, tgt, cand):
    """The risks R_0 .. R_steps of the learning case in float64: oracle.vag_oracle's forward on the expanded batch, risk_torch,
    autograd, and the oracle's clip + Adam (the step driver's defaults) at LEARN's rate."""
    from oracle import vag_oracle as O
    alpha, lr, steps = LEARN["alpha"], LEARN["lr"], LEARN["steps"]
    P = {k: v.double() for k, v in P.items()}
    rows, valid = pack(cand, tgt, True)
    B = np.asarray(tgt).shape[0]
    N = rows.shape[0] // B
    cost = bleu_cost(rows, tgt, N)
    rows_t = torch.from_numpy(rows)
    src_r = torch.as_tensor(np.asarray(src)).repeat_interleave(N, 0)
    lens_r = [int(n) for n in lengths for _ in range(N)]
    vw = torch.ones(P["decoder.out.bias"].shape[0], dtype=torch.float64)
    vw[0] = 0

    def risk_of(leaves):
        out = O.model_forward(leaves, src_r, lens_r, rows_t, None, keep=True)
        s = sum(vw[rows_t[:, t]] * st["logp"].gather(1, rows_t[:, t:t + 1]).squeeze(1) for t, st in enumerate(out["steps"]))
        return risk_torch(s, cost, valid, N, alpha)

    risks, state = [], {}
    for _ in range(steps):
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
        R = risk_of(leaves)
        risks.append(float(R.detach()))
        R.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        _, cg = O.clip_grad_norm(grads, 1.0)
        with torch.no_grad():
            P = O.adam_step({k: v.detach() for k, v in leaves.items()}, cg, state, lr=lr, weight_decay=1e-5)
    with torch.no_grad():
        risks.append(float(risk_of(P)))
    return risks
