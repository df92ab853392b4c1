"""GPU: word-level distillation -- vag_kd_targets against the float64 restatement (tests/distill_ref.py), the head with soft targets
(vag_kd_head_ce_seq_fwd / _bwd) against torch fp64 autograd, the fused distillation step (vag_train_step_kd) against torch
autograd over the existing operators, and TrainStep.distill_step end to end.

Tolerances.  q, losses, nll and the head operator's gradients: the suite's rule, test_gpu_golden.close with TOL = 1e-4.  The
selection at M = 1: exact (the score is one IEEE subtraction, reproducible in NumPy).  The selection at M = 3: within
delta = 16 * 2^-24 * max(1, |s_K|) of the fp64 order -- one subtraction, expf, an M-term sum, logf and one add, each within about
2 ulp.  Gradients of the fused step: test_gpu_mrt's rule and constant, GRAD_TOL times each reference tensor's largest entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distill_ref as R
from conftest import load_golden
from test_gpu_golden import close
from test_gpu_label_smoothing import HEAD_NAMES, _abi_run, _head_case, _model_case
from test_gpu_mrt import GRAD_TOL, SMALL_GRADS, _compare, _grads

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
VS = [1000, 2047, 9001, 10243]          # lse_nll's NV = 8, 8 (V % 4 = 3), 40 (V % 4 = 1), streaming (V % 4 = 3); 2 .. 21 slices of 512 words


def _guarded(n, fill, dtype):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def _guards_intact(bufs, fill=-7):
    for k, v in bufs.items():
        assert bool((v[:GUARD] == fill).all()) and bool((v[-GUARD:] == fill).all()), "guard of %s overwritten" % k


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: vag_kd_targets
# ------------------------------------------------------------------------------------------------------------------
def run_targets(logits, lse, V, K, T):
    """vag_kd_targets at the ABI on lists of M device tensors logits (R, ldl) and lse (R,); outputs inside guard margins."""
    from vagnmt_hip._lib import lib, ptr, stream
    M, Rn = len(logits), logits[0].shape[0]
    bufs = {"idx": _guarded(Rn * K, -7, torch.int32), "q": _guarded(Rn * K, -7.0, torch.float32)}
    rc = lib().vag_kd_targets((C.c_void_p * M)(*[ptr(x) for x in logits]), (C.c_int64 * M)(*[x.shape[1] for x in logits]),
                              (C.c_void_p * M)(*[ptr(x) for x in lse]), M, Rn, V, K, T, bufs["idx"][GUARD:-GUARD].data_ptr(),
                              bufs["q"][GUARD:-GUARD].data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _guards_intact(bufs)
    return bufs["idx"][GUARD:-GUARD].view(Rn, K).cpu().numpy(), bufs["q"][GUARD:-GUARD].view(Rn, K).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _tied_case(V):
    """R = 48 rows of logits quantised to five levels (hundreds of exact ties across every K-th place); row 7's best 64 words lie
    in the last columns (word V - 1 among them), row 9's best word is 0.  Returns the device inputs and the scores float32(x) -
    float32(lse) with their full order per row, computed once."""
    g = np.random.default_rng(V)
    Rn, ldl = 48, (V + 3) // 4 * 4
    x = np.zeros((Rn, ldl), dtype=np.float32)
    x[:, :V] = np.clip(np.round(g.normal(size=(Rn, V)) * 1.5), -2, 2)
    x[:, V:] = 99.0                                             # padding columns: never read
    x[7, V - 64:V] = 8.0 + (np.arange(64) % 5)
    x[9, 0] = 12.0
    lse = torch.logsumexp(torch.from_numpy(x[:, :V]), 1).numpy().astype(np.float32)
    s = R.scores([x[:, :V]], [lse], fp32=True)
    order = np.stack([np.lexsort((np.arange(V), -s[r].astype(np.float64))) for r in range(Rn)])
    return torch.from_numpy(x).to(DEV), torch.from_numpy(lse).to(DEV), s, order


@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("V", VS)
def test_targets_single_model_exact_under_ties(V, K, T):
    x, lse, s, order = _tied_case(V)
    want_idx = order[:, :K].astype(np.int32)
    top = np.take_along_axis(s.astype(np.float64), want_idx.astype(np.int64), 1)
    e = np.exp((top - top[:, :1]) / T)
    want_q = e / e.sum(1, keepdims=True)
    # the case is what it says: ties cross the K-th place, row 7's words lie in the last columns, row 9 starts with word 0
    tied = sum(int((s[r] == top[r, -1]).sum()) for r in range(48) if r not in (7, 9))
    assert tied > 100 * 46 and want_idx[7].min() >= V - 64 and (K < 64 or V - 1 in want_idx[7]) and want_idx[9, 0] == 0
    idx, q = run_targets([x], [lse], V, K, T)
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    print("[kd targets] V=%d K=%d T=%.1f: q max abs err %.3e, max |sum q - 1| %.3e"
          % (V, K, T, np.abs(q - want_q).max(), np.abs(q.astype(np.float64).sum(1) - 1).max()))
    close(q, want_q, what="q")
    assert np.abs(q.astype(np.float64).sum(1) - 1).max() <= 1e-5
    idx2, q2 = run_targets([x], [lse], V, K, T)                 # two runs: the same bits
    assert np.array_equal(idx, idx2) and np.array_equal(q.view(np.int32), q2.view(np.int32))


@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("V", [1000, 10243])
def test_targets_three_members_within_rounding_of_fp64(V, K):
    g = torch.Generator().manual_seed(V + K)
    Rn, ldl = 48, (V + 3) // 4 * 4
    xs = [(torch.randn(Rn, ldl, generator=g) * (1.0 + 0.5 * m)).to(DEV) for m in range(3)]
    ls = [torch.logsumexp(x[:, :V], 1).contiguous() for x in xs]
    s = R.scores([x[:, :V].cpu().numpy() for x in xs], [l.cpu().numpy() for l in ls])          # float64
    idx, q = run_targets(xs, ls, V, K, 1.0)
    worst = 0.0
    for r in range(Rn):
        srt = np.sort(s[r])[::-1]
        sK = srt[K - 1]
        delta = 16 * 2.0 ** -24 * max(1.0, abs(sK))
        got = s[r][idx[r]]
        assert len(set(idx[r].tolist())) == K and idx[r].min() >= 0 and idx[r].max() < V
        assert (got >= sK - delta).all(), (r, got.min(), sK, delta)                       # nothing selected from clearly below
        above = np.nonzero(s[r] > sK + delta)[0]
        assert np.isin(above, idx[r]).all(), r                                              # everything clearly above is selected
        assert (got[:-1] >= got[1:] - delta).all(), r                                       # ranked, within delta
        worst = max(worst, float((sK - got).max() / delta), float((got[1:] - got[:-1]).max() / delta) if K > 1 else 0.0)
    print("[kd targets] M=3 V=%d K=%d: worst gap / delta %.3f" % (V, K, worst))
    close(q.astype(np.float64).sum(1), np.ones(Rn), tol=1e-5, what="sum q")
    # M identical members: the single model's idx bit for bit
    one_idx, one_q = run_targets([xs[0]], [ls[0]], V, K, 1.0)
    three_idx, three_q = run_targets([xs[0]] * 3, [ls[0]] * 3, V, K, 1.0)
    assert np.array_equal(one_idx, three_idx)
    assert np.array_equal(one_q.view(np.int32), three_q.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------
# 3, 4: the head operator
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_inputs(V):
    return _head_case(V)


def _kd_fp64_reference(x, tgt, V, idx, q, lam):
    """torch autograd in fp64 on the CPU: the definition of include/vag_nmt.h on logits from the same weights."""
    d = {k: v.double().clone().requires_grad_(True) for k, v in x.items()}
    Tt, B, _ = d["h2"].shape
    t = torch.tanh(d["h2"] @ d["w1"].t() + d["b1"] + d["c"] @ d["w2"].t() + d["b2"] + d["e"] @ d["w3"].t() + d["b3"])
    logits = (t @ d["out_w"].t() + d["out_b"]).view(Tt * B, V)
    y = tgt.t().reshape(-1)
    w = (y != 0).double()
    lse = torch.logsumexp(logits, 1)
    soft = (torch.from_numpy(q).double() * logits.gather(1, torch.from_numpy(idx).long())).sum(1)
    nll = (w * (lse - (1.0 - lam) * logits.gather(1, y[:, None])[:, 0] - lam * soft)).view(Tt, B)
    loss = (nll.sum(0) / (tgt != 0).double().sum(-1)).mean()
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in d.items()}, nll.detach()


def _abi_run_kd(x, tgt, V, idx, q, lam):
    """One forward + one backward through vag_kd_head_ce_seq_fwd / _bwd on private buffers; idx, q and nll inside guard margins."""
    from vagnmt_hip._lib import HeadW, call, ptr, stream
    Tt, B, H = x["h2"].shape
    E = x["e"].shape[2]
    Rn, ldl, K = Tt * B, (V + 3) // 4 * 4, idx.shape[1]
    d = {k: v.to(DEV).contiguous() for k, v in x.items()}
    tg = tgt.to(DEV).contiguous()
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    f = lambda *s: torch.zeros(*s, device=DEV)        # noqa: E731
    bufs = {"idx": _guarded(Rn * K, -7, torch.int32), "q": _guarded(Rn * K, -7.0, torch.float32), "nll": _guarded(Rn, -7.0, torch.float32)}
    di, dq, nll = bufs["idx"][GUARD:-GUARD], bufs["q"][GUARD:-GUARD], bufs["nll"][GUARD:-GUARD]
    di.copy_(torch.from_numpy(idx).reshape(-1))
    dq.copy_(torch.from_numpy(q).reshape(-1))
    o = {"tmid": f(Tt, B, E), "logits": f(Rn, ldl), "lse": f(Rn), "nll": nll, "inv_cnt": f(B), "loss": f(1),
         "d_h2": f(Tt, B, H), "d_c": f(Tt, B, 2 * H), "d_e": f(Tt, B, E), "scratch": f(Rn * E)}
    g = {k: torch.zeros_like(d[k]) for k in HEAD_NAMES}
    hw = HeadW(*[ptr(d[k]) for k in HEAD_NAMES])
    hg = HeadW(*[ptr(g[k]) for k in HEAD_NAMES])
    one = torch.ones(1, device=DEV)
    kd = (K, lam, ptr(di, torch.int32), ptr(dq))
    call("vag_kd_head_ce_seq_fwd", ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None, 0,
         ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(nll), ptr(o["inv_cnt"]), ptr(o["loss"]), *kd, stream())
    call("vag_kd_head_ce_seq_bwd", ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None,
         ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["inv_cnt"]), ptr(one), ptr(o["d_h2"]), ptr(o["d_c"]),
         ptr(o["d_e"]), hg, ptr(o["scratch"]), *kd, stream())
    torch.cuda.synchronize()
    _guards_intact(bufs)
    assert torch.equal(di.cpu(), torch.from_numpy(idx).reshape(-1)) and torch.equal(dq.cpu(), torch.from_numpy(q).reshape(-1))
    o.update({"g_" + k: v for k, v in g.items()})
    del o["scratch"]
    return o


@pytest.mark.parametrize("lam", [0.5, 1.0])
@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("V", VS)
def test_head_operator_with_soft_targets_matches_fp64(V, K, lam):
    x, tgt = _head_inputs(V)
    Tt, B, _ = x["h2"].shape
    y = tgt.t().reshape(-1).numpy()
    idx, q = R.synth_targets(np.random.default_rng(100 * V + K), y, V, K)
    has_y = np.array([y[r] in idx[r] for r in range(len(y))])
    assert has_y.any() and (not has_y.all() or K == V) and (idx == V - 1).any() and (idx == 0).any()
    want_loss, want_g, want_nll = _kd_fp64_reference(x, tgt, V, idx, q, lam)
    o = _abi_run_kd(x, tgt, V, idx, q, lam)
    print("[kd operator] V=%d K=%d lambda=%.1f loss %.7f (fp64 %.7f)" % (V, K, lam, float(o["loss"]), float(want_loss)))
    for k in x:
        got = o["d_" + k] if k in ("h2", "c", "e") else o["g_" + k]
        ref = want_g[k].numpy()
        print("   d%-6s max abs err %.3e  scale %.3e" % (k, np.abs(got.cpu().double().numpy() - ref).max(), np.abs(ref).max()))
    close(o["loss"][0], want_loss.numpy(), what="loss_mt")
    close(o["nll"].view(Tt, B), want_nll.numpy(), what="nll")
    pad_rows = (tgt.t().reshape(-1) == 0).to(DEV)
    assert bool(pad_rows.any()) and torch.equal(o["nll"][pad_rows], torch.zeros_like(o["nll"][pad_rows]))      # PAD rows: exactly nothing
    for k in ("h2", "c", "e"):
        close(o["d_" + k], want_g[k].numpy(), what="d " + k)
    for k in HEAD_NAMES:
        close(o["g_" + k], want_g[k].numpy(), what="d " + k)
    dl = o["logits"]                         # now d(logits)
    ldl = (V + 3) // 4 * 4
    assert dl.shape[1] == ldl
    if ldl > V:
        assert torch.equal(dl[:, V:], torch.zeros_like(dl[:, V:])), "d(logits) padding columns must stay exactly 0"
    assert torch.equal(dl[pad_rows], torch.zeros_like(dl[pad_rows]))
    # every row still sums to zero: coef * (sum softmax - (1 - lambda) - lambda sum q); the bound and the reasoning of
    # test_gpu_label_smoothing (lse carries an ulp of its own size, coef <= 1/B)
    assert dl[:, :V].double().sum(-1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("V", VS)
def test_k1_idx_y_is_the_plain_loss(V):
    """K = 1, idx = y, q = 1: the plain loss for any lambda (0.7 here), up to the rounding of + coef lambda - coef lambda."""
    x, tgt = _head_inputs(V)
    y = tgt.t().reshape(-1).numpy()
    o = _abi_run_kd(x, tgt, V, y.astype(np.int32)[:, None].copy(), np.ones((len(y), 1), dtype=np.float32), 0.7)
    p = _abi_run(x, tgt, V, 0.0, "plain")
    for k in p:
        close(o[k], p[k].cpu().double().numpy(), what="K=1 idx=y " + k)
    assert float(p["loss"]) > 0 and p["g_out_w"].abs().max().item() > 0


# ------------------------------------------------------------------------------------------------------------------
# 5: off is off
# ------------------------------------------------------------------------------------------------------------------
def test_step_after_distill_steps_is_the_plain_step_bit_for_bit():
    """A driver that has run distill_step and step (graphs of both kinds cached) and is put back to the initial weights and
    optimiser state gives, from `step`, the losses and parameters of a fresh driver that never distilled -- at a shape where the
    plain step reproduces itself (test_gpu_mrt.test_mrt_off_is_the_plain_step_bit_for_bit: text model, untied, B = 2, Ts = 4,
    Tt = 3); a second fresh driver is the control that says so if the shape stops being reproducible."""
    from vagnmt_hip.trainer import TrainStep

    def fresh():
        m, batch, V = _model_case("text", B=2, Ts=4, Tt=3)
        vw = torch.ones(V, device=DEV)
        vw[0] = 0
        return m, TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, use_graph=True, pad_src=1), batch, V

    def plain_steps(ts, batch, n=3):
        src, lens, tgt, im = batch
        losses = [torch.stack(ts.step(src, lens, tgt, im, teacher=True)).clone() for _ in range(n)]
        torch.cuda.synchronize()
        return torch.stack(losses), ts.fp.flat.clone()
    m, ts, batch, V = fresh()
    src, lens, tgt, im = batch
    flat0 = ts.fp.flat.clone()
    y = tgt.t().reshape(-1).cpu().numpy()
    idx, q = R.synth_targets(np.random.default_rng(1), y, V, 8)
    soft = (torch.from_numpy(idx).view(3, 2, 8).to(DEV), torch.from_numpy(q).view(3, 2, 8).to(DEV))
    for _ in range(3):
        ts.distill_step(src, lens, tgt, im, soft=soft, kd_lambda=0.5)
    plain_steps(ts, batch)
    torch.cuda.synchronize()
    assert ts.stats["captures"] == 2 and not torch.equal(ts.fp.flat, flat0), ts.stats
    kinds = [any(isinstance(p, tuple) and p[:1] == ("kd",) for p in k) for k in ts._graphs]
    assert sorted(kinds) == [False, True], list(ts._graphs)     # graphs of both kinds are cached
    # back to the start: weights, moments, step counter, derived weights
    ts.fp.flat.copy_(flat0)
    ts.fp.m.zero_()
    ts.fp.v.zero_()
    ts.fp.grad.zero_()
    ts.step_count.zero_()
    ts.backend.after_optimizer()
    la, pa = plain_steps(ts, batch)
    _, ts_b, batch_b, _ = fresh()
    lb, pb = plain_steps(ts_b, batch_b)
    _, ts_c, batch_c, _ = fresh()
    lc, pc = plain_steps(ts_c, batch_c)
    assert float(lb[0, 0]) > 0 and not torch.equal(pb, flat0)
    assert torch.equal(lb, lc) and torch.equal(pb, pc), "control: the plain step does not reproduce itself at this shape"
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    ts.check()


# ------------------------------------------------------------------------------------------------------------------
# 6, 7: the fused distillation step against autograd over the existing operators
# ------------------------------------------------------------------------------------------------------------------
KD_K, KD_LAMBDA = 8, 0.5


def _criteria(kind, V):
    from machine_translation_vision.losses import PairwiseRankingLoss
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    return torch.nn.NLLLoss(weight=vw, reduction="none"), (PairwiseRankingLoss(margin=0.1) if kind == "mm" else None)


def _autograd_reference(m, batch, V, idx, q, lam, cv):
    """The mixed loss in torch fp64 on log-probabilities formed by ops.HeadLogp over the per-operator chain (the chain of
    test_gpu_mrt._row_scores), the ranking loss through the model's own prologue."""
    from vagnmt_hip import ops
    src, lens, tgt, im = batch
    m.eval()
    m.zero_grad()
    dec = m.decoder
    B, Tt = tgt.shape
    if im is not None:
        enc, mask, loss_vse, h0 = m._prologue(src, lens, im, cv, None)
    else:
        enc, mask, h0 = m._prologue(src, lens, None)
        loss_vse = None
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    tok = torch.cat([torch.full((1, B), 2, dtype=torch.int64, device=DEV), tgt.t()], 0).contiguous()
    h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
    H = h2.shape[2]
    logp = ops.HeadLogp.apply(h2.view(Tt * B, H), c.view(Tt * B, 2 * H), e.view(Tt * B, -1), 0.0, None, *dec.head_params())
    logp = logp.view(Tt * B, V).double()
    y = tgt.t().reshape(-1)
    gold = logp.gather(1, y[:, None])[:, 0]
    soft = (q.view(Tt * B, -1).double() * logp.gather(1, idx.view(Tt * B, -1).long())).sum(1)
    nll = (-(y != 0).double() * ((1.0 - lam) * gold + lam * soft)).view(Tt, B)
    loss_mt = (nll.sum(0) / (tgt != 0).double().sum(-1)).mean()
    loss = loss_mt
    if loss_vse is not None:
        loss = m.loss_w * loss_mt + (1 - m.loss_w) * loss_vse.double()
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    return (float(loss.detach()), float(loss_mt.detach()), float(loss_vse.detach()) if loss_vse is not None else 0.0), grads


@functools.lru_cache(maxsize=None)
def _step_case(kind):
    """test_gpu_label_smoothing._model_case's model and batch (H = 64, V = 61, B = 8, Ts = 9, Tt = 7, PAD tails), synthesised soft
    targets of K = 8 words per row, and the autograd reference, computed once."""
    m, batch, V = _model_case(kind)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tgt = batch[2]
    y = tgt.t().reshape(-1).cpu().numpy()
    idx, q = R.synth_targets(np.random.default_rng(7), y, V, KD_K)
    Tt, B = tgt.shape[1], tgt.shape[0]
    idx = torch.from_numpy(idx).view(Tt, B, KD_K).to(DEV)
    q = torch.from_numpy(q).view(Tt, B, KD_K).to(DEV)
    want = _autograd_reference(m, batch, V, idx, q, KD_LAMBDA, _criteria(kind, V)[1])
    return state, batch, V, idx, q, want


def _fused_driver(kind, state, **kw):
    from vagnmt_hip.trainer import TrainStep, _FusedBackend
    m, _, V = _model_case(kind)
    m.load_state_dict(state)
    kw.setdefault("pad_src", 1)
    ts = TrainStep(m, *_criteria(kind, V), **kw)
    assert type(ts.backend) is _FusedBackend
    m.eval()
    return m, ts


def _kd_visits(ts, batch, idx, q, n):
    src, lens, tgt, im = batch
    out = []
    for _ in range(n):
        ts.fp.grad.zero_()
        ts.backend.run(src, lens, tgt, im, True, 7, kd=(KD_K, KD_LAMBDA, idx, q))
        torch.cuda.synchronize()
        out.append(([float(v) for v in ts.backend.outputs()], _grads(ts)))
    return out


def _check_visits(kind, tag, expect_stats=True):
    state, batch, V, idx, q, want = _step_case(kind)
    (want_loss, want_mt, want_vse), want_g = want
    m, ts = _fused_driver(kind, state, use_graph=True)
    runs = _kd_visits(ts, batch, idx, q, 3)
    if expect_stats:
        assert ts.stats["eager_steps"] == 1 and ts.stats["captures"] == 1 and ts.stats["replays"] == 2, ts.stats
    for i, (l, g) in enumerate(runs):
        close(l[0], want_loss, what="%s visit %d loss" % (tag, i))
        close(l[2], want_vse, what="%s visit %d loss_vse" % (tag, i))
        _compare("%s visit %d" % (tag, i), l[1], g, (want_mt, want_g, None))
    ts.check()                                                  # the result ring is in step with the host's count
    return runs


@pytest.mark.parametrize("kind", ["mm", "text"])
def test_fused_distill_step_matches_autograd(kind):
    state, batch, V, idx, q, want = _step_case(kind)
    (want_loss, want_mt, want_vse), want_g = want
    nonzero = {k: v.abs().max().item() for k, v in want_g.items() if v.abs().max().item() > 0}
    print("[kd step] %s: reference losses %.6f %.6f %.6f; gradient maxima %s"
          % (kind, want_loss, want_mt, want_vse, {k: "%.2e" % v for k, v in nonzero.items()}))
    # the comparison is not vacuous (test_gpu_mrt's asserts on the reference's magnitudes); every parameter has a gradient here
    assert all(v > 1e-3 for k, v in nonzero.items() if k not in SMALL_GRADS), nonzero
    assert all(v > 1e-4 for k, v in nonzero.items() if k in SMALL_GRADS), nonzero
    assert set(want_g) == set(nonzero)
    if kind == "mm":
        assert want_vse > 1e-3                                  # a multimodal student keeps a non-zero ranking loss
    _check_visits(kind, kind)


@pytest.mark.parametrize("head_fuse", [1, 0])
def test_fused_distill_step_chunked_head(head_fuse):
    """The head in row chunks of 16 of the 56 rows (a short last chunk of 8): finished inside the forward (head_fuse 1) and
    recomputed by the backward (head_fuse 0); idx / q are offset per chunk."""
    from vagnmt_hip import _lib as L
    try:
        L.set_option("head_chunk", 2 * 8)
        L.set_option("head_fuse", head_fuse)
        _check_visits("mm", "chunked head_fuse=%d" % head_fuse)
    finally:
        L.set_option("head_chunk", -1)
        L.set_option("head_fuse", 1)


def test_distilled_gradient_is_not_the_plain_gradient():
    """A step that ignored kd_* would compute the plain step's gradient: some tensor of it differs from the distilled reference
    by more than ten times the tolerance, relative to the reference's largest entry."""
    state, batch, V, idx, q, want = _step_case("mm")
    src, lens, tgt, im = batch
    m, ts = _fused_driver("mm", state, use_graph=False)
    ts.fp.grad.zero_()
    ts.backend.run(src, lens, tgt, im, True, 7)
    torch.cuda.synchronize()
    plain = _grads(ts)
    ratios = {}
    for k, ref in want[1].items():
        scale = ref.abs().max().item()
        if scale > 0.0:
            ratios[k] = (plain[k].double() - ref.double()).abs().max().item() / scale
    print("[kd differs] plain - distilled, relative to the reference's largest entry: %s" % {k: "%.2e" % v for k, v in ratios.items()})
    assert max(ratios.values()) > 10 * GRAD_TOL
    assert ratios["decoder.out.bias"] > 10 * GRAD_TOL          # the soft part's own correction


# ------------------------------------------------------------------------------------------------------------------
# 8: TrainStep.distill_step end to end
# ------------------------------------------------------------------------------------------------------------------
def _golden_pair(name, **kw):
    """The golden model as the teacher, the same architecture from another seed as the student, and the golden batch."""
    from test_gpu_golden import build
    from vagnmt_hip.trainer import TrainStep
    meta, P, z = load_golden(name)
    teacher, student = build(meta, P), build(meta, P)
    torch.manual_seed(1234)
    with torch.no_grad():
        for p in student.parameters():
            p.uniform_(-0.08, 0.08)
    V = meta["dims"][1]
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    ts = TrainStep(student, torch.nn.NLLLoss(weight=vw, reduction="none"), None, **kw)
    src, tgt = torch.from_numpy(z["src"]).to(DEV), torch.from_numpy(z["tgt"]).to(DEV)
    im = torch.from_numpy(z["im"]).to(DEV) if meta["kind"] == "mm" else None
    return meta, teacher, student, ts, (src, torch.tensor(meta["lengths"], dtype=torch.int32, device=DEV), tgt, im)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_distill_step_end_to_end(name, use_graph):
    from vagnmt_hip import distill, scoring
    from vagnmt_hip.ensemble import Ensemble
    meta, teacher, student, ts, (src, lens, tgt, im) = _golden_pair(name, lr=2e-3, use_graph=use_graph, pad_src=1)
    V, B, Tt = meta["dims"][1], tgt.shape[0], tgt.shape[1]
    hyp = [[int(t) for t in h] for h in teacher._decode(src, meta["lengths"], im, 1, Tt + 1, None)]
    score = lambda: float(scoring.score_models([student], [im is not None], src, lens, hyp, im).score.mean())      # noqa: E731
    before = score()
    losses = []
    for _ in range(20):
        losses.append(ts.distill_step(src, lens, tgt, im, teacher_model=teacher, kd_lambda=1.0, top_k=8))
    torch.cuda.synchronize()
    ts.check()
    assert not teacher.training and student.training            # the teacher's mode is restored, the student trains
    mt = [float(l[1]) for l in losses]
    after = score()
    print("[kd e2e] %s %s: loss_mt %.5f -> %.5f; score of the teacher's greedy output %.5f -> %.5f"
          % (name, "graph" if use_graph else "eager", mt[0], mt[-1], before, after))
    assert all(np.isfinite(mt)) and mt[-1] < mt[0]
    assert after > before
    if use_graph:
        assert ts.stats["captures"] == 1 and ts.stats["replays"] == 19, ts.stats
    # precomputed targets give the step the same launches; an Ensemble of two members as the teacher
    soft = distill.teacher_targets(Ensemble([teacher, student]), src, lens, tgt, im, top_k=8, temperature=2.0, vocab_size=V)
    torch.cuda.synchronize()
    assert soft.idx.shape == (Tt, B, 8) and soft.idx.dtype == torch.int32 and soft.q.shape == (Tt, B, 8)
    assert (soft.q.double().sum(-1) - 1).abs().max().item() <= 1e-5
    assert int(soft.idx.min()) >= 0 and int(soft.idx.max()) < V and bool((soft.q[..., :-1] >= soft.q[..., 1:]).all())
    out = ts.distill_step(src, lens, tgt, im, soft=soft, kd_lambda=0.5)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in out)
    with pytest.raises(ValueError, match="vocabulary"):
        distill.teacher_targets(teacher, src, lens, tgt, im, vocab_size=V + 1)
    ts.check()
