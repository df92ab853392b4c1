"""GPU: R-Drop -- the head with the symmetric KL between twin rows (vag_rdrop_head_ce_seq_fwd / _bwd) against torch fp64 autograd,
the twin rule of the ranking loss (vag_rank_loss_fwd, kind | 2) against tests/rdrop_ref.py, the fused R-Drop step
(vag_train_step_rdrop) against torch fp64 autograd over the existing operators, and TrainStep.rdrop_step: against the plain step
without dropout, against the oracle under the step's own dropout masks, and end to end.

Tolerances.  kl, losses, nll and the head operator's gradients: the suite's rule, test_gpu_golden.close with TOL = 1e-4.  Gradients of
the fused step: test_gpu_mrt's rule and constant, GRAD_TOL times each reference tensor's largest entry.  Parameters after an
optimiser step: test_gpu_trainer's post-Adam bound (close with 2e-5)."""
import functools

import numpy as np
import pytest
import torch

import rdrop_ref as R
from conftest import load_golden
from test_gpu_golden import TOL, close
from test_gpu_label_smoothing import HEAD_NAMES, _model_case
from test_gpu_mrt import GRAD_TOL, SMALL_GRADS, _compare, _grads

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
VS = [5, 1000, 2047, 9001, 10243]       # a row shorter than one wave, then test_gpu_distill.VS: lse_nll's NV = 8, 8 (V % 4 = 3), 40 (V % 4 = 1), streaming
POST_ADAM_TOL = 2e-5                    # test_gpu_trainer: parameters after an Adam step


def _guarded(shape, dtype=torch.float32, fill=-7):
    """(whole buffer, its interior viewed as `shape` and zeroed): GUARD elements of `fill` on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    inner = buf[GUARD:GUARD + n]
    inner.zero_()
    return buf, inner.view(*shape)


def _guards_intact(bufs, fill=-7):
    for k, v in bufs.items():
        assert bool((v[:GUARD] == fill).all()) and bool((v[-GUARD:] == fill).all()), "guard of %s overwritten" % k


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: the head operator
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_inputs(Bt, Tt, V):
    """Random head inputs and weights, E = H = 32: independent twins (KL of order 1); where the shape has room, one pair of identical
    rows (t = Tt // 2, rows 0, 1), one pair with a PAD target in both rows (t = 2, rows 2, 3) and pairs with a PAD target in one row
    (rows 4, 5 at t >= 1; for Bt = 2 rows 0, 1 at t = 2).  A target in the last column at t = 0."""
    E = H = 32
    g = torch.Generator().manual_seed(10007 * Bt + 101 * Tt + V)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)     # noqa: E731
    x = {"h2": r(Tt, Bt, H), "c": r(Tt, Bt, 2 * H), "e": r(Tt, Bt, E),
         "w1": r(E, H, k=0.2), "b1": r(E, k=0.1), "w2": r(E, 2 * H, k=0.2), "b2": r(E, k=0.1), "w3": r(E, E, k=0.2), "b3": r(E, k=0.1),
         "out_w": r(V, E, k=0.3), "out_b": r(V, k=0.1)}
    tgt = torch.randint(1, V, (Bt // 2, Tt), generator=g).repeat_interleave(2, 0)
    tgt[Bt - 2:, 0] = V - 1
    same = None
    if Bt * Tt > 2:
        same = (Tt // 2) * Bt                                   # row index of the identical pair's first row
        for k in ("h2", "c", "e"):
            x[k][Tt // 2, 1] = x[k][Tt // 2, 0]
    if Tt == 3:
        if Bt >= 6:
            tgt[2:4, 2] = 0
            tgt[4, 1:] = 0
        else:
            tgt[0, 2] = 0
    return x, tgt, same


def _fp64_reference(x, tgt, V, eps, alpha):
    """torch autograd in fp64 on the CPU: the definition of include/vag_nmt.h on logits from the same weights."""
    d = {k: v.double().clone().requires_grad_(True) for k, v in x.items()}
    Tt, Bt, _ = d["h2"].shape
    t = torch.tanh(d["h2"] @ d["w1"].t() + d["b1"] + d["c"] @ d["w2"].t() + d["b2"] + d["e"] @ d["w3"].t() + d["b3"])
    logits = (t @ d["out_w"].t() + d["out_b"]).view(Tt * Bt, V)
    y = tgt.t().reshape(-1)
    w = (y != 0).double()
    lp = torch.log_softmax(logits, -1)
    tw = lp.view(-1, 2, V).flip(1).reshape(-1, V)
    kl = (lp.exp() * (lp - tw)).sum(-1)
    both = kl.view(-1, 2).sum(-1).repeat_interleave(2)
    plain = -((1.0 - eps) * lp.gather(1, y[:, None])[:, 0] + eps / V * lp.sum(-1))
    nll = (w * (plain + alpha / 4.0 * both)).view(Tt, Bt)
    loss = (nll.sum(0) / (tgt != 0).double().sum(-1)).mean()
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in d.items()}, nll.detach(), kl.detach().view(Tt, Bt)


def _abi_run(x, tgt, V, eps, alpha, backward=True):
    """One forward (+ one backward) through vag_rdrop_head_ce_seq_fwd / _bwd on private buffers -- alpha None: through the _ls entry
    points, the plain loss.  Every output sits inside guard margins; the logits' padding columns start as NaN."""
    from vagnmt_hip._lib import HeadW, call, ptr, stream
    Tt, Bt, H = x["h2"].shape
    E = x["e"].shape[2]
    Rn, ldl = Tt * Bt, (V + 3) // 4 * 4
    d = {k: v.to(DEV).contiguous() for k, v in x.items()}
    tg = tgt.to(DEV).contiguous()
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    shapes = {"tmid": (Tt, Bt, E), "logits": (Rn, ldl), "lse": (Rn,), "nll": (Rn,), "kl": (Rn,), "inv_cnt": (Bt,), "loss": (1,),
              "d_h2": (Tt, Bt, H), "d_c": (Tt, Bt, 2 * H), "d_e": (Tt, Bt, E), "scratch": (Rn * E,)}
    shapes.update({"g_" + k: tuple(d[k].shape) for k in HEAD_NAMES})
    bufs, o = {}, {}
    for k, s in shapes.items():
        bufs[k], o[k] = _guarded(s)
    o["logits"][:, V:] = float("nan")
    o["kl"].fill_(-3.0)                                         # (the plain run leaves it alone)
    hw = HeadW(*[ptr(d[k]) for k in HEAD_NAMES])
    hg = HeadW(*[ptr(o["g_" + k]) for k in HEAD_NAMES])
    one = torch.ones(1, device=DEV)
    fwd = (ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), Bt, Tt, E, H, V, 0.0, None, 0,
           ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["nll"]), ptr(o["inv_cnt"]), ptr(o["loss"]), eps)
    bwd = (ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), Bt, Tt, E, H, V, 0.0, None,
           ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["inv_cnt"]), ptr(one), ptr(o["d_h2"]), ptr(o["d_c"]),
           ptr(o["d_e"]), hg, ptr(o["scratch"]), eps)
    if alpha is None:
        call("vag_head_ce_seq_fwd_ls", *fwd, stream())
        if backward:
            call("vag_head_ce_seq_bwd_ls", *bwd, stream())
    else:
        call("vag_rdrop_head_ce_seq_fwd", *fwd, alpha, ptr(o["kl"]), stream())
        if backward:
            call("vag_rdrop_head_ce_seq_bwd", *bwd, alpha, ptr(o["kl"]), stream())
    torch.cuda.synchronize()
    _guards_intact(bufs)
    del o["scratch"]
    return o


@functools.lru_cache(maxsize=None)
def _plain_dlogits(Bt, Tt, V, eps):
    x, tgt, _ = _head_inputs(Bt, Tt, V)
    return _abi_run(x, tgt, V, eps, None)["logits"]


@pytest.mark.parametrize("alpha", [1.0, 5.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("Tt", [1, 3])
@pytest.mark.parametrize("Bt", [2, 6, 16])
def test_head_operator_matches_fp64(Bt, Tt, V, eps, alpha):
    x, tgt, same = _head_inputs(Bt, Tt, V)
    want_loss, want_g, want_nll, want_kl = _fp64_reference(x, tgt, V, eps, alpha)
    y = tgt.t().reshape(-1)
    live = (y != 0)
    if same is None:
        assert float(want_kl.mean()) > 0.1                      # independent twins: KL of order 1, far above the tolerance
    else:
        others = torch.ones(Tt * Bt, dtype=torch.bool)
        others[same:same + 2] = False
        assert float(want_kl.view(-1)[others].mean()) > 0.1 and float(want_kl.view(-1)[same]) == 0.0
    if Tt == 3 and Bt >= 6:                                     # the case holds what it says
        pairs = (y.view(-1, 2) == 0)
        assert bool(pairs.all(1).any()) and bool((pairs.any(1) & ~pairs.all(1)).any())
    o = _abi_run(x, tgt, V, eps, alpha)
    print("[rdrop operator] Bt=%d Tt=%d V=%d eps=%.1f alpha=%.0f loss %.7f (fp64 %.7f); kl max abs err %.3e (max %.3e)"
          % (Bt, Tt, V, eps, alpha, float(o["loss"]), float(want_loss),
             (o["kl"].view(Tt, Bt).cpu().double() - want_kl).abs().max().item(), want_kl.abs().max().item()))
    for k in x:
        got = o["d_" + k] if k in ("h2", "c", "e") else o["g_" + k]
        ref = want_g[k].numpy()
        print("   d%-6s max abs err %.3e  scale %.3e" % (k, np.abs(got.cpu().double().numpy() - ref).max(), np.abs(ref).max()))
    close(o["kl"].view(Tt, Bt), want_kl.numpy(), what="kl")
    close(o["loss"][0], want_loss.numpy(), what="loss_mt")
    close(o["nll"].view(Tt, Bt), want_nll.numpy(), what="nll")
    assert torch.equal(o["nll"][~live.to(DEV)], torch.zeros(int((~live).sum()), device=DEV))      # PAD rows: exactly nothing
    for k in ("h2", "c", "e"):
        close(o["d_" + k], want_g[k].numpy(), what="d " + k)
    for k in HEAD_NAMES:
        close(o["g_" + k], want_g[k].numpy(), what="d " + k)
    dl = o["logits"]                         # now d(logits)
    ldl = (V + 3) // 4 * 4
    assert dl.shape[1] == ldl
    if ldl > V:
        assert torch.equal(dl[:, V:], torch.zeros_like(dl[:, V:])), "d(logits) padding columns must be exactly 0"
    both_pad = (y.view(-1, 2) == 0).all(1).repeat_interleave(2).to(DEV)
    assert torch.equal(dl[both_pad], torch.zeros_like(dl[both_pad]))
    assert bool(torch.isfinite(dl).all())
    # every row still sums to zero, the KL part too: sum_j p (d - kl) + p - p_twin = 0.  The bound and the reasoning of
    # test_gpu_label_smoothing (1e-5 at coef <= 1/8: lse carries an ulp of its own size), scaled to this shape's coef <= 1 / Bt and
    # to the KL term's (alpha / 4) (coef + coef_twin) <= (alpha / 2) / Bt
    assert dl[:, :V].double().sum(-1).abs().max().item() <= 1e-5 * max(1.0, 8.0 / Bt) * max(1.0, alpha / 2)
    if same is not None:
        # identical rows: kl is exactly 0 in both directions, and the rows' d(logits) is the plain loss's
        assert float(o["kl"][same]) == 0.0 and float(o["kl"][same + 1]) == 0.0
        plain = _plain_dlogits(Bt, Tt, V, eps)
        close(dl[same:same + 2], plain[same:same + 2].cpu().double().numpy(), what="identical pair d(logits)")
        assert plain[same].abs().max().item() > 0


@pytest.mark.parametrize("V", VS)
def test_forward_is_reproducible(V):
    """Two runs of the forward: bit-identical kl and nll (a fixed summation order, no floating-point atomics)."""
    x, tgt, _ = _head_inputs(16, 3, V)
    a = _abi_run(x, tgt, V, 0.1, 5.0, backward=False)
    b = _abi_run(x, tgt, V, 0.1, 5.0, backward=False)
    assert float(a["kl"].abs().max()) > 0.1
    for k in ("kl", "nll", "lse", "loss"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("Bt", [2, 6, 16, 34])
def test_ranking_loss_twin_flag_matches_reference(Bt, kind):
    """vag_rank_loss_fwd / _bwd with kind | 2 (ops.RankLoss) against the float64 loops of rdrop_ref; Bt = 16 takes the one-launch
    backward, the others the two products; Bt = 2 (one sentence) is exactly 0.  kind without the flag is the plain loss."""
    from vagnmt_hip import ops
    g = torch.Generator().manual_seed(Bt + kind)
    S = 32
    im = torch.nn.functional.normalize(torch.randn(Bt, S, generator=g), dim=1)
    s = torch.nn.functional.normalize(torch.randn(Bt, S, generator=g), dim=1)
    want, G = R.rank_loss_twins(im.numpy(), s.numpy(), 0.1, kind)
    a, b = im.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
    loss = ops.RankLoss.apply(a, b, 0.1, kind | 2)
    loss.backward()
    torch.cuda.synchronize()
    close(loss, want, what="twin loss")
    close(a.grad, G @ s.double().numpy(), what="d im")
    close(b.grad, G.T @ im.double().numpy(), what="d s")
    if Bt == 2:
        assert float(loss.detach()) == 0.0 and float(a.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
    else:
        assert want > 1.0
        plain = ops.RankLoss.apply(im.to(DEV), s.to(DEV), 0.1, kind)
        close(plain, R.rank_loss_plain(im.numpy(), s.numpy(), 0.1, kind), what="plain loss")
        assert float(plain) > float(loss.detach())


# ------------------------------------------------------------------------------------------------------------------
# 3, 4: the fused step against torch fp64 autograd over the existing operators
# ------------------------------------------------------------------------------------------------------------------
RD_ALPHA = 5.0


def _criteria(kind, V, eps=0.0):
    from machine_translation_vision.losses import LabelSmoothedNLLLoss, PairwiseRankingLoss
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    cm = LabelSmoothedNLLLoss(vw, eps) if eps > 0 else torch.nn.NLLLoss(weight=vw, reduction="none")
    return cm, (PairwiseRankingLoss(margin=0.1) if kind == "mm" else None)


def _twin_rank_loss(im, s, margin=0.1):
    """The step's ranking loss in torch fp64: the pairwise loss with the twin rule, times 1/4."""
    S = im.double() @ s.double().t()
    i = torch.arange(S.shape[0], device=S.device)
    keep = (i[:, None] >> 1) != (i[None, :] >> 1)
    d = torch.diagonal(S)
    both = torch.clamp(margin - d[None, :] + S, min=0) + torch.clamp(margin - d[:, None] + S, min=0)
    return 0.25 * both[keep].sum()


def _autograd_reference(m, batch, V, alpha, eps, kind):
    """test_gpu_distill._autograd_reference's method: the loss in torch fp64 on log-probabilities formed by ops.HeadLogp over the
    per-operator chain; the ranking loss through the model's own prologue with the twin rule stated in torch."""
    from vagnmt_hip import ops
    src, lens, tgt, im = batch
    m.eval()
    m.zero_grad()
    dec = m.decoder
    B, Tt = tgt.shape
    if kind == "mm":
        enc, mask, loss_vse, h0 = m._prologue(src, lens, im, _twin_rank_loss, None)
    else:
        enc, mask, h0 = m._prologue(src, lens, None)
        loss_vse = None
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    tok = torch.cat([torch.full((1, B), 2, dtype=torch.int64, device=DEV), tgt.t()], 0).contiguous()
    h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
    H = h2.shape[2]
    logp = ops.HeadLogp.apply(h2.view(Tt * B, H), c.view(Tt * B, 2 * H), e.view(Tt * B, -1), 0.0, None, *dec.head_params())
    lp = logp.view(Tt * B, V).double()
    y = tgt.t().reshape(-1)
    w = (y != 0).double()
    tw = lp.view(-1, 2, V).flip(1).reshape(-1, V)
    kl = (lp.exp() * (lp - tw)).sum(-1)
    both = kl.view(-1, 2).sum(-1).repeat_interleave(2)
    plain = -((1.0 - eps) * lp.gather(1, y[:, None])[:, 0] + eps / V * lp.sum(-1))
    nll = (w * (plain + alpha / 4.0 * both)).view(Tt, B)
    loss_mt = (nll.sum(0) / (tgt != 0).double().sum(-1)).mean()
    loss = loss_mt
    if loss_vse is not None:
        loss = m.loss_w * loss_mt + (1 - m.loss_w) * loss_vse
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    mean_kl = float((kl.detach() * w).sum() / w.sum())
    return (float(loss.detach()), float(loss_mt.detach()), float(loss_vse.detach()) if loss_vse is not None else 0.0), grads, mean_kl


@functools.lru_cache(maxsize=None)
def _step_case(kind, eps):
    """test_gpu_label_smoothing._model_case's model and batch (H = 64, V = 61, B = 8, Ts = 9, Tt = 7, PAD tails) made into 16 rows
    whose twins are DIFFERENT sources (of the same length, so the lengths stay sorted) and images with the same target: the KL term
    is large without dropout.  Returns the model's state, the batch and the autograd reference, computed once."""
    m, (src, lens, tgt, im), V = _model_case(kind)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    src2 = torch.where(src != 0, torch.randint(4, 50, src.shape, generator=g).to(DEV), src)
    src16 = torch.stack([src, src2], 1).reshape(16, -1).contiguous()
    lens16 = lens.repeat_interleave(2).contiguous()
    tgt16 = tgt.repeat_interleave(2, 0).contiguous()
    im16 = None
    if im is not None:
        im16 = torch.stack([im, torch.randn(im.shape, generator=g).abs().to(DEV)], 1).reshape(16, -1).contiguous()
    batch = (src16, lens16, tgt16, im16)
    assert not torch.equal(src16[0], src16[1]) and torch.equal(tgt16[0], tgt16[1]) and lens16.tolist() == sorted(lens16.tolist(), reverse=True)
    want = _autograd_reference(m, batch, V, RD_ALPHA, eps, kind)
    return state, batch, V, want


def _fused_driver(kind, state, eps=0.0, **kw):
    from vagnmt_hip.trainer import TrainStep, _FusedBackend
    m, _, V = _model_case(kind)
    m.load_state_dict(state)
    kw.setdefault("pad_src", 1)
    ts = TrainStep(m, *_criteria(kind, V, eps), **kw)
    assert type(ts.backend) is _FusedBackend
    m.eval()
    return m, ts


def _rd_visits(ts, batch, n, rdrop=(RD_ALPHA,)):
    src, lens, tgt, im = batch
    out = []
    for _ in range(n):
        ts.fp.grad.zero_()
        ts.backend.run(src, lens, tgt, im, True, 7, rdrop=rdrop)
        torch.cuda.synchronize()
        out.append(([float(v) for v in ts.backend.outputs()], _grads(ts)))
    return out


def _check_visits(kind, tag, eps=0.0, visits=3):
    state, batch, V, want = _step_case(kind, eps)
    (want_loss, want_mt, want_vse), want_g, _ = want
    m, ts = _fused_driver(kind, state, eps, use_graph=True)
    runs = _rd_visits(ts, batch, visits)
    if visits == 3:
        assert ts.stats["eager_steps"] == 1 and ts.stats["captures"] == 1 and ts.stats["replays"] == 2, ts.stats
    for i, (l, g) in enumerate(runs):
        close(l[0], want_loss, what="%s visit %d loss" % (tag, i))
        close(l[2], want_vse, what="%s visit %d loss_vse" % (tag, i))
        _compare("%s visit %d" % (tag, i), l[1], g, (want_mt, want_g, None))
    ts.check()                                                  # the result ring is in step with the host's count
    return runs


@pytest.mark.parametrize("kind", ["mm", "text"])
def test_fused_rdrop_step_matches_autograd(kind):
    state, batch, V, want = _step_case(kind, 0.0)
    (want_loss, want_mt, want_vse), want_g, mean_kl = want
    nonzero = {k: v.abs().max().item() for k, v in want_g.items() if v.abs().max().item() > 0}
    print("[rdrop step] %s: reference losses %.6f %.6f %.6f, mean kl %.4f; gradient maxima %s"
          % (kind, want_loss, want_mt, want_vse, mean_kl, {k: "%.2e" % v for k, v in nonzero.items()}))
    # nothing compared is vacuous (test_gpu_mrt's asserts on the reference's magnitudes); every parameter has a gradient here
    assert all(v > 1e-3 for k, v in nonzero.items() if k not in SMALL_GRADS), nonzero
    assert all(v > 1e-4 for k, v in nonzero.items() if k in SMALL_GRADS), nonzero
    assert set(want_g) == set(nonzero)
    assert mean_kl > 1e3 * TOL
    if kind == "mm":
        assert want_vse > 1e-3
    _check_visits(kind, kind)


def test_fused_rdrop_step_with_label_smoothing_matches_autograd():
    """R-Drop is normally used with label smoothing: a LabelSmoothedNLLLoss criterion (eps = 0.1) through the same comparison."""
    _check_visits("text", "text eps=0.1", eps=0.1)


@pytest.mark.parametrize("head_fuse", [1, 0])
def test_fused_rdrop_step_chunked_head(head_fuse):
    """The head in row chunks of 32 of the 112 rows (two time steps of 16 rows; a short last chunk of 16): finished inside the
    forward (head_fuse 1) and recomputed by the backward (head_fuse 0), which reads kl from the forward's buffer."""
    from vagnmt_hip import _lib as L
    try:
        L.set_option("head_chunk", 32)
        L.set_option("head_fuse", head_fuse)
        _check_visits("mm", "chunked head_fuse=%d" % head_fuse)
    finally:
        L.set_option("head_chunk", -1)
        L.set_option("head_fuse", 1)


@pytest.mark.parametrize("kind", ["mm", "text"])
def test_rdrop_gradient_is_not_the_plain_gradient(kind):
    """A step that ignored alpha would compute the plain step's gradient on the 16 rows: some tensor of it differs from the R-Drop
    reference by more than ten times the tolerance, relative to the reference's largest entry."""
    state, batch, V, want = _step_case(kind, 0.0)
    src, lens, tgt, im = batch
    m, ts = _fused_driver(kind, state, use_graph=False)
    ts.fp.grad.zero_()
    ts.backend.run(src, lens, tgt, im, True, 7)
    torch.cuda.synchronize()
    plain = _grads(ts)
    ratios = {}
    for k, ref in want[1].items():
        scale = ref.abs().max().item()
        if scale > 0.0:
            ratios[k] = (plain[k].double() - ref.double()).abs().max().item() / scale
    print("[rdrop differs] plain - R-Drop, relative to the reference's largest entry: %s" % {k: "%.2e" % v for k, v in ratios.items()})
    assert max(ratios.values()) > 10 * GRAD_TOL
    assert ratios["decoder.out.bias"] > 10 * GRAD_TOL           # the KL term's own part of d(logits)
    assert abs(float(ts.backend.outputs()[1]) - want[0][1]) > 10 * TOL


# ------------------------------------------------------------------------------------------------------------------
# 5, 6: rdrop_step with real twins
# ------------------------------------------------------------------------------------------------------------------
def _pair_of_drivers(kind, dropout=0.0, **kw):
    from vagnmt_hip.trainer import TrainStep
    out = []
    for _ in range(2):
        m, batch, V = _model_case(kind, dropout=dropout)
        out.append((m, TrainStep(m, *_criteria(kind, V), pad_src=1, **kw), batch))
    assert torch.equal(out[0][1].fp.flat, out[1][1].fp.flat)
    return out


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["mm", "text"])
def test_without_dropout_rdrop_step_is_the_plain_step(kind, use_graph):
    """Every dropout 0: the twins are the same computation, so kl is at rounding level, all three losses are the plain step's on the
    8 sentences and so are the updated parameters -- the 1/Bt normalisation, the twin rule and the 1/4 of the ranking loss together."""
    (ma, tsa, batch), (mb, tsb, _) = _pair_of_drivers(kind, use_graph=use_graph)
    src, lens, tgt, im = batch
    for i in range(2 if use_graph else 1):                      # (graph: the second visit replays a captured step)
        plain = [v.clone() for v in tsa.step(src, lens, tgt, im, teacher=True)]
        out = tsb.rdrop_step(src, lens, tgt, im, alpha=5.0)
        torch.cuda.synchronize()
        live = (tgt != 0).t().repeat_interleave(2, 1)            # (Tt, 2B)
        print("[rdrop no dropout] %s visit %d: losses %s (plain %s); max |kl| %.3e"
              % (kind, i, [float(v) for v in out[:3]], [float(v) for v in plain], float(out.kl.abs().max())))
        assert out.kl.shape == live.shape
        close(out.kl[live], np.zeros(int(live.sum())), what="kl without dropout")
        for k, a, b in zip(("loss", "loss_mt", "loss_vse"), out[:3], plain):
            close(a, float(b), what=k)
        if kind == "mm":
            assert float(plain[2]) > 1e-3
        for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            close(pb, pa.detach().cpu().double().numpy(), POST_ADAM_TOL, "post-Adam " + n)
    assert int(tsb.step_count.item()) == int(tsa.step_count.item()) and not torch.equal(tsb.fp.flat, torch.zeros_like(tsb.fp.flat))
    tsb.check()


@pytest.mark.parametrize("kind", ["mm", "text"])
def test_with_dropout_twins_run_under_different_masks_and_match_the_oracle(kind):
    """Train mode, the model's dropout rates (0.3 / 0.5 / 0.5): the step's masks for the 16 rows, materialised by the library, go to the
    oracle's model_forward on the duplicated batch.  loss_mt minus the KL term formed in fp64 from the returned kl equals the
    oracle's loss_mt (the mean of both passes' cross-entropy), and kl > 0 on every non-PAD row: the twins saw different masks."""
    from oracle import vag_oracle as O
    from vagnmt_hip import ops, rdrop
    from vagnmt_hip.trainer import TrainStep
    alpha = 5.0
    m, (src, lens, tgt, im), V = _model_case(kind, dropout=0.5)
    ts = TrainStep(m, *_criteria(kind, V), pad_src=1, use_graph=False)
    P = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    out = ts.rdrop_step(src, lens, tgt, im, alpha=alpha)
    torch.cuda.synchronize()
    kl = out.kl.double().cpu()
    B, Tt = tgt.shape
    Bt, Ts, E, H = 2 * B, src.shape[1], 32, 64
    rng = m._vag_rng
    masks = {"emb": ops.dropout_mask(rng, 1, Ts * Bt * E, 0.3).view(Ts, Bt, E).cpu(),
             "ctx": ops.dropout_mask(rng, 2, Bt * Ts * 2 * H, 0.5).view(Bt, Ts, 2 * H).transpose(0, 1).contiguous().cpu(),
             "out": ops.dropout_mask(rng, 3, Tt * Bt * E, 0.5).view(Tt, Bt, E).cpu()}
    assert not torch.equal(masks["out"][:, 0], masks["out"][:, 1]) and not torch.equal(masks["ctx"][:, 0], masks["ctx"][:, 1])
    tw = rdrop.twins
    ref = O.model_forward(P, tw(src).cpu(), tw(lens).tolist(), tw(tgt).cpu(), tw(im).cpu() if im is not None else None, teacher=True,
                          masks=masks, attn=m.attn_model if kind == "mm" else "dot")
    t16 = tw(tgt).cpu()
    w = (t16 != 0).double().t()                                 # (Tt, Bt)
    cnt = (t16 != 0).double().sum(-1)
    both = kl + kl.view(Tt, B, 2).flip(2).reshape(Tt, Bt)
    term = float(((w * both).sum(0) / cnt).mean())
    print("[rdrop dropout] %s: loss_mt %.6f = oracle CE %.6f + alpha/4 x %.6f; mean kl %.5f (rdrop.mean_kl %.5f)"
          % (kind, float(out.loss_mt), float(ref["loss_mt"]), term, float((kl * w).sum() / w.sum()), float(rdrop.mean_kl(out, tgt))))
    close(float(out.loss_mt) - alpha / 4.0 * term, float(ref["loss_mt"]), what="loss_mt - KL term")
    assert bool((kl[w > 0] > 0).all()) and term > 1e3 * TOL
    close(rdrop.mean_kl(out, tgt), float((kl * w).sum() / w.sum()), what="mean_kl")
    ts.check()


# ------------------------------------------------------------------------------------------------------------------
# 7: off is off
# ------------------------------------------------------------------------------------------------------------------
def test_step_after_rdrop_steps_is_the_plain_step_bit_for_bit():
    """A driver that has run rdrop_step and step (graphs of both kinds cached) and is put back to the initial weights and optimiser
    state gives, from `step`, the losses and parameters of a fresh driver that never ran R-Drop -- at a shape where the plain step
    reproduces itself (test_gpu_distill's: text model, untied, B = 2, Ts = 4, Tt = 3); a second fresh driver is the control."""
    from vagnmt_hip.trainer import TrainStep

    def fresh():
        m, batch, V = _model_case("text", B=2, Ts=4, Tt=3)
        return m, TrainStep(m, *_criteria("text", V), use_graph=True, pad_src=1), batch

    def plain_steps(ts, batch, n=3):
        src, lens, tgt, im = batch
        losses = [torch.stack(ts.step(src, lens, tgt, im, teacher=True)).clone() for _ in range(n)]
        torch.cuda.synchronize()
        return torch.stack(losses), ts.fp.flat.clone()
    m, ts, batch = fresh()
    src, lens, tgt, im = batch
    flat0 = ts.fp.flat.clone()
    for _ in range(3):
        ts.rdrop_step(src, lens, tgt, im, alpha=5.0)
    plain_steps(ts, batch)
    torch.cuda.synchronize()
    assert ts.stats["captures"] == 2 and not torch.equal(ts.fp.flat, flat0), ts.stats
    kinds = [any(isinstance(p, tuple) and p[:1] == ("rdrop",) for p in k) for k in ts._graphs]
    assert sorted(kinds) == [False, True], list(ts._graphs)     # graphs of both kinds are cached
    ts.fp.flat.copy_(flat0)
    ts.fp.m.zero_()
    ts.fp.v.zero_()
    ts.fp.grad.zero_()
    ts.step_count.zero_()
    ts.backend.after_optimizer()
    la, pa = plain_steps(ts, batch)
    _, ts_b, batch_b = fresh()
    lb, pb = plain_steps(ts_b, batch_b)
    _, ts_c, batch_c = fresh()
    lc, pc = plain_steps(ts_c, batch_c)
    assert float(lb[0, 0]) > 0 and not torch.equal(pb, flat0)
    assert torch.equal(lb, lc) and torch.equal(pb, pc), "control: the plain step does not reproduce itself at this shape"
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    ts.check()


# ------------------------------------------------------------------------------------------------------------------
# 8: end to end
# ------------------------------------------------------------------------------------------------------------------
def _golden_driver(name, **kw):
    from test_gpu_golden import build, criteria
    from vagnmt_hip.trainer import TrainStep
    meta, P, z = load_golden(name)
    m = build(meta, P)
    m.encoder.dropout_emb, m.encoder.dropout_ctx, m.decoder.dropout_out = 0.3, 0.5, 0.5      # the reference's training rates
    cm, cv = criteria(meta)
    ts = TrainStep(m, cm, cv if meta["kind"] == "mm" else None, pad_src=1, **kw)
    src, tgt = torch.from_numpy(z["src"]).to(DEV), torch.from_numpy(z["tgt"]).to(DEV)
    im = torch.from_numpy(z["im"]).to(DEV) if meta["kind"] == "mm" else None
    return meta, m, ts, (src, torch.tensor(meta["lengths"], dtype=torch.int32, device=DEV), tgt, im)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_rdrop_step_end_to_end(name, use_graph, tmp_path):
    """The golden models under the reference's dropout rates: three rdrop_steps with averaged weights on, check(), and a checkpoint
    saved after the second step and resumed into a fresh driver whose third step gives the first driver's third loss
    (test_gpu_round2's resume tolerance: the dropout generator's words travel with the checkpoint, so the masks are the same)."""
    from vagnmt_hip import rdrop
    from vagnmt_hip.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(lr=2e-3, use_graph=use_graph, ema_decay=0.9, capture_after=1)
    meta, m, ts, (src, lens, tgt, im) = _golden_driver(name, **kw)
    path = str(tmp_path / "rdrop.pt")
    outs = []
    for i in range(3):
        out = ts.rdrop_step(src, lens, tgt, im, alpha=5.0)
        outs.append([float(v) for v in out[:3]] + [float(rdrop.mean_kl(out, tgt))])
        if i == 1:
            save_checkpoint(path, m, ts)
    torch.cuda.synchronize()
    ts.check()
    print("[rdrop e2e] %s %s: (loss, loss_mt, loss_vse, mean kl) %s" % (name, "graph" if use_graph else "eager", outs))
    assert m.training and int(ts.step_count.item()) == 3 and np.isfinite(np.array(outs)).all()
    assert all(o[3] > 1e3 * TOL for o in outs)                  # the twins ran under different masks in every step
    assert out.kl.shape == (tgt.shape[1], 2 * tgt.shape[0])
    assert not torch.equal(ts.fp.ema, ts.fp.flat)               # the average moved with the steps
    if use_graph:
        assert ts.stats["captures"] == 1 and ts.stats["replays"] == 2, ts.stats
    with ts.averaged_weights():
        with pytest.raises(ValueError, match="averaged_weights"):
            ts.rdrop_step(src, lens, tgt, im)
    _, m2, ts2, _ = _golden_driver(name, **kw)
    load_checkpoint(path, m2, ts2)
    out2 = ts2.rdrop_step(src, lens, tgt, im, alpha=5.0)
    torch.cuda.synchronize()
    assert int(ts2.step_count.item()) == 3
    assert np.allclose([float(v) for v in out2[:3]], outs[2][:3], rtol=2e-5), ([float(v) for v in out2[:3]], outs[2])
    ts2.check()


# ------------------------------------------------------------------------------------------------------------------
# 9: refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from vagnmt_hip._lib import HeadW, lib, ptr
    from vagnmt_hip.trainer import TrainStep, _AutogradBackend
    m, (src, lens, tgt, im), V = _model_case("text")
    ts = TrainStep(m, *_criteria("text", V), pad_src=1, storage="f16")
    with pytest.raises(NotImplementedError, match="2-byte storage"):
        ts.rdrop_step(src, lens, tgt, im)
    m, _, V = _model_case("text")
    with pytest.raises(NotImplementedError, match="zero1"):
        TrainStep(m, *_criteria("text", V), pad_src=1, zero1=True).rdrop_step(src, lens, tgt, im)
    m, _, V = _model_case("text")
    ts = TrainStep(m, *_criteria("text", V), pad_src=1, fused=False)
    assert type(ts.backend) is _AutogradBackend
    with pytest.raises(NotImplementedError, match="autograd path"):
        ts.rdrop_step(src, lens, tgt, im)
    with pytest.raises(ValueError, match="alpha"):
        ts.rdrop_step(src, lens, tgt, im, alpha=0.0)
    # the ABI: -EINVAL and nothing launched (real buffers, every output still as it was filled)
    x, t3, _ = _head_inputs(6, 3, 1000)
    d = {k: v.to(DEV).contiguous() for k, v in x.items()}
    hw = HeadW(*[ptr(d[k]) for k in HEAD_NAMES])
    tg = t3[:5].to(DEV).contiguous()
    o = {k: torch.full((n,), -7.0, device=DEV) for k, n in (("tmid", 18 * 32), ("logits", 18 * 1000), ("lse", 18), ("nll", 18), ("kl", 18),
                                                           ("inv_cnt", 6), ("loss", 1))}
    vw = torch.ones(1000, device=DEV)

    def fwd(B, alpha, kl):
        return lib().vag_rdrop_head_ce_seq_fwd(ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), B, 3, 32, 32, 1000, 0.0,
                                               None, 0, ptr(o["tmid"]), ptr(o["logits"]), 1000, ptr(o["lse"]), ptr(o["nll"]),
                                               ptr(o["inv_cnt"]), ptr(o["loss"]), 0.1, alpha, kl, None)
    assert fwd(5, 5.0, ptr(o["kl"])) == -22 and fwd(4, 0.0, ptr(o["kl"])) == -22 and fwd(4, float("nan"), ptr(o["kl"])) == -22
    assert fwd(4, 5.0, None) == -22
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v == -7.0).all()), k


# ------------------------------------------------------------------------------------------------------------------
# 10: the train.py shim
# ------------------------------------------------------------------------------------------------------------------
def test_shim_routes_through_rdrop_step_when_the_environment_says_so(monkeypatch):
    """VAG_RDROP_ALPHA set when the pair's driver is made: train_imagine_beam / train_nmt run rdrop_step (the step's key carries
    ("rdrop", alpha)); unset: the plain step.  The golden model has no dropout, so both return the same losses."""
    from test_gpu_golden import build, criteria
    from test_gpu_round5 import _reference_optimizer, _shim
    T = _shim()
    meta, P, z = load_golden("mm_dot_tied_s0_f32")
    cm, cv = criteria(meta)
    src, tgt, im = torch.from_numpy(z["src"]).to(DEV), torch.from_numpy(z["tgt"]).to(DEV), torch.from_numpy(z["im"]).to(DEV)
    out, keys = {}, {}
    for alpha in (None, "5"):
        if alpha is None:
            monkeypatch.delenv("VAG_RDROP_ALPHA", raising=False)
        else:
            monkeypatch.setenv("VAG_RDROP_ALPHA", alpha)
        m = build(meta, P)
        opt = _reference_optimizer(m)
        out[alpha] = T.train_imagine_beam(src, tgt, im, meta["lengths"], m, opt, cm, cv, meta["loss_w"], 1.0, clip=1.0)
        d = opt._vag_driver
        assert type(d.ts.backend).__name__ == "_FusedBackend" and int(d.ts.step_count.item()) == 1
        keys[alpha] = [k[0] for k in d.ts._seen if len(k) == 2]             # (step key, phases) entries
        d.ts.check()
    assert all(("rdrop", 5.0) in k for k in keys["5"]) and keys["5"] and keys["5"][0][0] == 2 * src.shape[0]
    assert not any(isinstance(p, tuple) and p[:1] == ("rdrop",) for k in keys[None] for p in k) and keys[None][0][0] == src.shape[0]
    close(np.array(out["5"]), np.array(out[None]), what="shim losses without dropout")
