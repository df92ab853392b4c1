"""GPU: the decode kernels behind the search drivers, called through the ABI on synthetic state and compared with numpy
restatements kept in this file: the finish family (vag_beam_finish, vag_beam_finish_nbest, vag_beam_finish_align), forced
decoding (vag_forced_score, vag_forced_align) and the attention record (vag_beam_attn_record, vag_beam_attn_record_dev).

The whole-model searches run these kernels at toy lengths only; the shapes here reach the branches those never take: the
finish's history in global memory (steps * k > 4096 words), targets longer than one 64-lane ballot block, the scalar and the
16-byte attention paths, a device step index past the end."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EOS = 3
FIN_LDS = 4096            # (word, parent) pairs of one sentence's history the finish keeps in LDS


def _ptrs(ts):
    from vagnmt_hip._lib import ptr
    return (C.c_void_p * len(ts))(*[ptr(t) for t in ts])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# 1. the finish family
# ------------------------------------------------------------------------------------------------------------------
def _search_state(B, k, ML, steps, ties, seed, V=23):
    """beam (2 ML, B, k): words in rows [0, ML) (EOS, the other words <= 3 and ordinary words), parents in rows [ML, 2 ML);
    nll (B, k).  ties: integer nll, and slots 0 / 2 (and 1 / k-1) get equal nll and equal length but different rows: they
    share their last word and differ in the word before it (5 against 6, both counted), reached through different parents
    with a common ancestor -- only the slot index orders them."""
    g = np.random.default_rng(seed)
    words = g.integers(0, V, size=(ML, B, k))
    words[g.random((ML, B, k)) < 0.08] = EOS
    low = g.random((ML, B, k)) < 0.08
    words[low] = g.integers(0, 3, size=int(low.sum()))
    parents = g.integers(0, k, size=(ML, B, k))
    nll = (-g.random((B, k)) * 40).astype(np.float32)
    if ties:
        nll = np.round(nll)
        t = steps - 1
        for (a, c), (pa, pc) in (((0, 2), (0, 1)), ((1, k - 1), (2, 3))):
            words[t, :, c] = words[t, :, a]
            parents[t, :, a], parents[t, :, c] = pa, pc
            words[t - 1, :, pa], words[t - 1, :, pc] = 5, 6
            parents[t - 1, :, pc] = parents[t - 1, :, pa]
            nll[:, c] = nll[:, a]
    return np.concatenate([words, parents]).astype(np.int64), nll


def _attn_hist(ML, B, k, Tp, seed):
    """(ML, B k, Tp) in [0, 1); every other row is quantised to quarters so that its maximum is usually shared by columns."""
    g = np.random.default_rng(seed)
    h = g.random((ML, B * k, Tp)).astype(np.float32)
    h[:, ::2] = np.round(h[:, ::2] * 4) / 4
    return h


def restate_finish(beam, nll, ML, steps):
    """Walks the back-pointers of all B k final hypotheses as the kernels do.  Returns, ranked (score desc, slot asc):
    rows (B, k, ML), scores (B, k) fp32, src (B, k, ML) = the attn_hist row (flat over (ML, B k)) behind each word or -1."""
    B, k = nll.shape
    words, par = beam[:ML], beam[ML:]
    bi = np.arange(B)[:, None]
    p = np.tile(np.arange(k), (B, 1))
    rows = np.zeros((B, k, ML), np.int64)
    src = np.full((B, k, ML), -1, np.int64)
    ln = np.zeros((B, k), np.int64)
    first_eos = np.full((B, k), ML)
    for t in range(steps - 1, -1, -1):
        w = words[t, bi, p]
        rows[:, :, t] = w
        if t < ML - 1:
            ln += w > 3
        first_eos = np.where((w == EOS) | (t == ML - 1), t, first_eos)
        p = par[t, bi, p]                                      # the slot after step t-1 that this word extends
        src[:, :, t] = t * B * k + (bi * k + p if t > 0 else bi + 0 * p)
    src[np.arange(ML)[None, None, :] > first_eos[:, :, None]] = -1
    rows[:, :, ML - 1] = EOS
    score = nll.astype(np.float32) / np.maximum(ln, 1).astype(np.float32)
    assert score.dtype == np.float32
    order = np.stack([np.lexsort((np.arange(k), -score[b].astype(np.float64))) for b in range(B)])
    return rows[bi, order], score[bi, order], src[bi, order]


def restate_attention(hist, src, Ts):
    flat = hist.reshape(-1, hist.shape[-1])
    live = src >= 0
    att = np.where(live[..., None], flat[np.maximum(src, 0), :Ts], np.float32(0))
    pos = np.where(live, att.argmax(-1), -1)                    # np.argmax: the lowest index among equal values
    return att, pos


FINISH_CASES = {
    "lds": (3, 5, 9, 9, False),
    "lds_early_stop": (3, 5, 9, 6, False),
    "lds_ties": (3, 5, 9, 9, True),
    "global": (2, 64, 80, 70, False),              # 70 * 64 = 4480 > FIN_LDS: the history stays in global memory
    "global_ties": (2, 64, 80, 70, True),
    "lds_last": (2, 64, 80, 64, False),            # 64 * 64 = 4096: the last shape that fits
}


@pytest.mark.parametrize("case", list(FINISH_CASES))
def test_finish_family(case):
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import call, ptr
    B, k, ML, steps, ties = FINISH_CASES[case]
    assert (steps * k > FIN_LDS) == case.startswith("global")
    beam_h, nll_h = _search_state(B, k, ML, steps, ties, seed=len(case) + steps)
    rows, score, src = restate_finish(beam_h, nll_h, ML, steps)
    if ties:                                   # every sentence ranks two different rows of equal score
        assert all(any(score[b, r] == score[b, r + 1] and not np.array_equal(rows[b, r], rows[b, r + 1]) for r in range(k - 1))
                   for b in range(B))
    assert (rows[:, :, :ML - 1] == EOS).any() and (src[:, :, :steps] == -1).any()
    beam, nll = torch.from_numpy(beam_h).cuda(), torch.from_numpy(nll_h).cuda()
    i64, f32 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.float32, device="cuda")

    # vag_beam_finish: the best row and its score; best_score may be NULL
    out1 = torch.full((B, ML), -7, **i64)
    best = torch.full((B,), -7.0, **f32)
    call("vag_beam_finish", ptr(nll), ptr(beam, torch.int64), ML, steps, B, k, ptr(out1, torch.int64), ptr(best), L.stream())
    out1n = torch.full((B, ML), -7, **i64)
    call("vag_beam_finish", ptr(nll), ptr(beam, torch.int64), ML, steps, B, k, ptr(out1n, torch.int64), None, L.stream())
    assert torch.equal(out1, out1n)
    assert np.array_equal(out1.cpu().numpy(), rows[:, 0])

    for n in sorted({1, (k + 1) // 2 if k < 10 else 7, k}):
        out = torch.full((B, n, ML), -7, **i64)
        sc = torch.full((B, n), -7.0, **f32)
        call("vag_beam_finish_nbest", ptr(nll), ptr(beam, torch.int64), ML, steps, B, k, n, ptr(out, torch.int64), ptr(sc),
             L.stream())
        got_sc = sc.cpu().numpy()
        assert np.array_equal(out.cpu().numpy(), rows[:, :n]), (case, n)                  # tokens and ranks
        # Exact: the device's fp32 divide is correctly rounded (observed: 0 ulp from the numpy quotient in every case here).
        ulp = np.abs(_bits(got_sc).astype(np.int64) - _bits(score[:, :n]).astype(np.int64)).max()
        print("%s n=%d: scores differ from the numpy fp32 quotient by at most %d ulp" % (case, n, ulp))
        assert np.array_equal(_bits(got_sc), _bits(score[:, :n])), (case, n, ulp)
        if n == 1:
            assert torch.equal(out[:, 0], out1) and torch.equal(sc[:, 0].view(torch.int32), best.view(torch.int32))
        for Tp, Ts in ((8, 8), (8, 5), (7, 7)):      # 16-byte loads and stores; 16-byte loads, scalar stores; scalar both
            hist_h = _attn_hist(ML, B, k, Tp, seed=Tp)
            att, pos = restate_attention(hist_h, src[:, :n], Ts)
            hist = torch.from_numpy(hist_h).cuda()
            out_a = torch.full((B, n, ML), -7, **i64)
            sc_a = torch.full((B, n), -7.0, **f32)
            attention = torch.full((B, n, ML, Ts), -7.0, **f32)
            src_pos = torch.full((B, n, ML), -7, **i64)
            call("vag_beam_finish_align", ptr(nll), ptr(beam, torch.int64), ptr(hist), ML, steps, B, k, n, Tp, Ts,
                 ptr(out_a, torch.int64), ptr(sc_a), ptr(attention), ptr(src_pos, torch.int64), L.stream())
            assert torch.equal(out_a, out) and torch.equal(sc_a.view(torch.int32), sc.view(torch.int32)), (case, n, Tp, Ts)
            assert np.array_equal(src_pos.cpu().numpy(), pos), (case, n, Tp, Ts)
            assert np.array_equal(_bits(attention.cpu().numpy()), _bits(att)), (case, n, Tp, Ts)


# ------------------------------------------------------------------------------------------------------------------
# 2. forced decoding: the span scan over two ballot blocks
# ------------------------------------------------------------------------------------------------------------------
F_B, F_TT, F_V, F_LDL = 4, 70, 11, 12


def _forced_targets():
    g = np.random.default_rng(70)
    y = g.integers(4, F_V, size=(F_B, F_TT))
    y[:, 5] = 1                                    # words <= 3 inside the span: scored, not counted
    y[:, 9] = 2
    y[:, 11] = 0                                   # a pad inside the span: neither scored nor counted
    y[0, 66] = EOS                                 # first EOS in the second ballot block, words after it
    y[0, 68] = EOS
    y[1, 3] = EOS                                  # an early EOS, non-pad words after it
    y[2, 69] = 0                                   # no EOS: the span ends at the last non-pad word, t = 68
    y[3, :] = 0                                    # all pad: an empty span
    assert not (y[2] == EOS).any()
    return y.astype(np.int64)


def _span_end(row):
    row = row.tolist()
    return row.index(EOS) if EOS in row else max([t for t, w in enumerate(row) if w != 0], default=-1)


def _forced_member(seed, Ts):
    """One member's teacher-forced outputs, time-major: logits (Tt B, ldl) with a NaN padding column (never read), their rows'
    log-sum-exp (Tt B) and the attention (Tt, B, Ts)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((F_TT * F_B, F_LDL), float("nan"))
    logits[:, :F_V] = torch.randn(F_TT * F_B, F_V, generator=g)
    lse = torch.logsumexp(logits[:, :F_V], dim=1)
    alpha = torch.softmax(torch.randn(F_TT, F_B, Ts, generator=g) * 2, dim=2)
    alpha[::3] = (alpha[::3] * 8).round() / 8                       # rows whose maximum is shared by columns
    return logits.contiguous(), lse.contiguous(), alpha.contiguous()


def _forced_run(members, y, Ts):
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import call, ptr
    M = len(members)
    dev = [[t.cuda() for t in m] for m in members]
    tgt = torch.from_numpy(y).cuda()
    tok = torch.full((F_B, F_TT), -7.0, device="cuda")
    logp = torch.full((F_B,), -7.0, device="cuda")
    score = torch.full((F_B,), -7.0, device="cuda")
    call("vag_forced_score", _ptrs([d[0] for d in dev]), (C.c_int64 * M)(*[F_LDL] * M), _ptrs([d[1] for d in dev]), M,
         ptr(tgt, torch.int64), F_B, F_TT, F_V, ptr(tok), ptr(logp), ptr(score), L.stream())
    attention = torch.full((F_B, F_TT, Ts), -7.0, device="cuda")
    src_pos = torch.full((F_B, F_TT), -7, dtype=torch.int64, device="cuda")
    call("vag_forced_align", _ptrs([d[2] for d in dev]), M, ptr(tgt, torch.int64), F_B, F_TT, Ts, ptr(attention),
         ptr(src_pos, torch.int64), L.stream())
    return [t.cpu().numpy() for t in (tok, logp, score, attention, src_pos)]


def _member_x(member, y):
    """x[b, t] = logit - lse of the target word in fp32 (0 where the word is the pad)."""
    logits, lse, _ = [t.numpy() for t in member]
    x = np.zeros((F_B, F_TT), np.float32)
    for b in range(F_B):
        for t in range(F_TT):
            x[b, t] = logits[t * F_B + b, y[b, t]] - lse[t * F_B + b]
    return x


def _forced_masks(y):
    ends = [_span_end(y[b]) for b in range(F_B)]
    assert ends == [66, 3, 68, -1]
    inside = np.arange(F_TT)[None, :] <= np.array(ends)[:, None]
    return inside, inside & (y != 0), np.maximum((inside & (y > 3)).sum(1), 1).astype(np.float32)


def _check_forced_attention(attention, src_pos, mean, inside):
    want = np.where(inside[..., None], mean.transpose(1, 0, 2), np.float32(0))
    assert np.array_equal(_bits(attention), _bits(want))
    assert np.array_equal(src_pos, np.where(inside, want.argmax(-1), -1))


@pytest.mark.parametrize("Ts", [8, 5])
def test_forced_single_model(Ts):
    y = _forced_targets()
    member = _forced_member(71, Ts)
    tok, logp, score, attention, src_pos = _forced_run([member], y, Ts)
    inside, scored, words = _forced_masks(y)
    want_tok = np.where(scored, _member_x(member, y), np.float32(0))
    assert np.array_equal(_bits(tok), _bits(want_tok))
    want_logp = np.zeros(F_B, np.float32)
    for b in range(F_B):
        for t in range(F_TT):                                       # a sequential fp32 sum in t order
            want_logp[b] = want_logp[b] + want_tok[b, t]
    assert np.array_equal(_bits(logp), _bits(want_logp))
    assert np.array_equal(_bits(score), _bits(want_logp / words))
    assert logp[3] == 0 and score[3] == 0
    _check_forced_attention(attention, src_pos, member[2].numpy(), inside)


@pytest.mark.parametrize("Ts", [8, 5])
def test_forced_two_members(Ts):
    y = _forced_targets()
    a, b = _forced_member(72, Ts), _forced_member(73, Ts)
    inside, scored, words = _forced_masks(y)
    # two identical members (separate storage): the single model bit for bit
    one = _forced_run([a], y, Ts)
    two = _forced_run([a, tuple(t.clone() for t in a)], y, Ts)
    for u, v in zip(one, two):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    # two distinct members: the combined score in float64 from the members' fp32 x, under test_gpu_nbest_score.py's bounds
    tok, logp, score, attention, src_pos = _forced_run([a, b], y, Ts)
    x = np.stack([_member_x(m, y).astype(np.float64) for m in (a, b)])
    mx = x.max(0)
    want_tok = (mx + np.log(np.exp(x - mx).sum(0) / 2)) * scored
    want_logp = want_tok.sum(1)
    tol = 2e-6
    e_tok = np.abs(tok - want_tok).max()
    e_lp = np.abs(logp - want_logp).max()
    e_sc = np.abs(score - want_logp / words).max()
    print("M=2 Ts=%d: max abs err token_logp %.2e logp %.2e score %.2e" % (Ts, e_tok, e_lp, e_sc))
    assert e_tok <= tol and e_lp <= tol * F_TT and e_sc <= tol * F_TT, (e_tok, e_lp, e_sc)
    assert not (tok != 0)[~scored].any()                             # exactly 0 outside the span
    mean = (a[2].numpy() + b[2].numpy()) / np.float32(2)
    assert mean.dtype == np.float32
    _check_forced_attention(attention, src_pos, mean, inside)


# ------------------------------------------------------------------------------------------------------------------
# 3. the attention record
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("Tp", [8, 7])
def test_attn_record(M, Tp):
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import call, ptr
    B, k, ML = 3, 4, 5
    g = torch.Generator().manual_seed(80 + M + Tp)
    alphas = [torch.rand(B * k, Tp, generator=g) for _ in range(M)]
    mean = alphas[0] if M == 1 else (alphas[0] + alphas[1]) / 2          # fp32: the sum, then an exact halving
    hist0 = torch.rand(ML, B * k, Tp, generator=g)
    dev = [a.cuda() for a in alphas]

    def record(di=None, di_state=None):
        hist = hist0.clone().cuda()
        if di_state is None:
            call("vag_beam_attn_record", _ptrs(dev), M, ptr(hist), di, ML, B, k, Tp, L.stream())
            return hist.cpu()
        st = torch.tensor([di_state, 0], dtype=torch.int32, device="cuda")
        call("vag_beam_attn_record_dev", _ptrs(dev), M, ptr(hist), ptr(st, torch.int32), ML, B, k, Tp, L.stream())
        assert st.tolist() == [di_state, 0]                              # the record reads the step index, never advances it
        return hist.cpu()

    want = hist0.clone()
    want[0, :B] = mean[:B]                                               # step 0: one hypothesis per sentence, B rows
    assert torch.equal(record(di=0), want)
    want = hist0.clone()
    want[2] = mean                                                       # later steps: B k rows
    assert torch.equal(record(di=2), want)
    assert torch.equal(record(di_state=2), want)
    assert torch.equal(record(di_state=ML), hist0)                       # past the end: the history is untouched
