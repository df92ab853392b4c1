"""GPU: the label-smoothed translation loss in the output head (vag_head_ce_seq_*_ls, ops.HeadCESmoothed) and in the fused
training step (vag_step_cfg.label_smoothing, read from criterion_mt by FusedStep).

Definition (include/vag_nmt.h): nll_eps = w[y] * (lse - (1 - eps) x[y] - eps/V sum_{j<V} x[j]); the executable definition is
machine_translation_vision.losses.LabelSmoothedNLLLoss.forward (pinned to torch's cross_entropy(label_smoothing=) on the CPU
by tests/test_label_smoothing_host.py).  Every comparison against fp64 uses the suite's own rule and number:
test_gpu_golden.close with TOL = 1e-4 (BASELINE.json's fp32 tolerance): max abs error <= 1e-4 * max(1, max|ref|)."""
import numpy as np
import pytest
import torch

from test_gpu_golden import TOL, close

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEAD_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "out_w", "out_b")


def _crit(V, eps, cls=None):
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    return (cls or LabelSmoothedNLLLoss)(vw, eps)


def _generic_cls():
    """A trivial subclass: recognised by nothing, so it takes the generic path (log-probabilities materialised, the criterion's own
    torch forward called once per time step) -- an independent reference on the same device."""
    from machine_translation_vision.losses import LabelSmoothedNLLLoss

    class Generic(LabelSmoothedNLLLoss):
        pass
    return Generic


# ------------------------------------------------------------------------------------------------------------------
# the operator
# ------------------------------------------------------------------------------------------------------------------
def _head_case(V, B=8, Tt=6, E=32, H=64, seed=0):
    """Random head inputs and weights (R = Tt*B = 48 rows); tgt with PAD tails and one all-but-one-PAD sentence."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)     # noqa: E731
    x = {"h2": r(Tt, B, H), "c": r(Tt, B, 2 * H), "e": r(Tt, B, E),
         "w1": r(E, H, k=0.2), "b1": r(E, k=0.1), "w2": r(E, 2 * H, k=0.2), "b2": r(E, k=0.1), "w3": r(E, E, k=0.2), "b3": r(E, k=0.1),
         "out_w": r(V, E, k=0.3), "out_b": r(V, k=0.1)}
    tgt = torch.randint(4, V, (B, Tt), generator=g)
    tgt[:, -1] = 3
    tgt[0, 0], tgt[1, 1] = V - 1, V - 2               # targets in the last (for V % 4 != 0: partial) group of columns
    for b, n in ((2, 4), (3, 2), (5, 3)):             # PAD tails
        if b < B - 1 and n < Tt:
            tgt[b, n - 1] = 3
            tgt[b, n:] = 0
    tgt[B - 1, 0] = 3                                 # all but one PAD
    tgt[B - 1, 1:] = 0
    return x, tgt


def _fp64_reference(x, tgt, V, eps):
    """torch autograd in fp64 on the CPU: logits from the same weights, LabelSmoothedNLLLoss.forward per row, the per-sentence
    normalisation of models/...V11.py:164."""
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    d = {k: v.double().clone().requires_grad_(True) for k, v in x.items()}
    Tt, B, _ = d["h2"].shape
    t = torch.tanh(d["h2"] @ d["w1"].t() + d["b1"] + d["c"] @ d["w2"].t() + d["b2"] + d["e"] @ d["w3"].t() + d["b3"])
    logits = t @ d["out_w"].t() + d["out_b"]
    vw = torch.ones(V, dtype=torch.float64)
    vw[0] = 0
    crit = LabelSmoothedNLLLoss(vw, eps)
    nll = crit(torch.log_softmax(logits, -1).view(Tt * B, V), tgt.t().reshape(-1)).view(Tt, B)
    loss = (nll.sum(0) / (tgt != 0).double().sum(-1)).mean()
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in d.items()}, nll.detach()


def _abi_run(x, tgt, V, eps, which):
    """One forward + one backward straight through the C ABI on private buffers.  which: "plain" (the entry points without
    _ls; eps must be 0), "ls" (vag_head_ce_seq_fwd_ls + _bwd_ls), "ls_data" (_fwd_ls + _bwd_data_ls + vag_head_bwd_weights)."""
    from vagnmt_hip._lib import HeadW, call, ptr, stream
    Tt, B, H = x["h2"].shape
    E = x["e"].shape[2]
    R, ldl = Tt * B, (V + 3) // 4 * 4
    d = {k: v.to(DEV).contiguous() for k, v in x.items()}
    tg = tgt.to(DEV).contiguous()
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    f = lambda *s: torch.zeros(*s, device=DEV)        # noqa: E731
    o = {"tmid": f(Tt, B, E), "logits": f(R, ldl), "lse": f(R), "nll": f(R), "inv_cnt": f(B), "loss": f(1),
         "d_h2": f(Tt, B, H), "d_c": f(Tt, B, 2 * H), "d_e": f(Tt, B, E), "scratch": f(R * E)}
    g = {k: torch.zeros_like(d[k]) for k in HEAD_NAMES}
    hw = HeadW(*[ptr(d[k]) for k in HEAD_NAMES])
    hg = HeadW(*[ptr(g[k]) for k in HEAD_NAMES])
    one = torch.ones(1, device=DEV)
    fwd = (ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None, 0,
           ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["nll"]), ptr(o["inv_cnt"]), ptr(o["loss"]))
    bwd = (ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), hw, ptr(tg, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None,
           ptr(o["tmid"]), ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["inv_cnt"]), ptr(one), ptr(o["d_h2"]), ptr(o["d_c"]),
           ptr(o["d_e"]), hg, ptr(o["scratch"]))
    if which == "plain":
        assert eps == 0.0
        call("vag_head_ce_seq_fwd", *fwd, stream())
        call("vag_head_ce_seq_bwd", *bwd, stream())
    else:
        call("vag_head_ce_seq_fwd_ls", *fwd, eps, stream())
        if which == "ls":
            call("vag_head_ce_seq_bwd_ls", *bwd, eps, stream())
        else:
            call("vag_head_ce_seq_bwd_data_ls", hw, ptr(tg, torch.int64), ptr(vw), B, Tt, E, H, V, 0.0, None, ptr(o["tmid"]),
                 ptr(o["logits"]), ldl, ptr(o["lse"]), ptr(o["inv_cnt"]), ptr(one), ptr(o["d_h2"]), ptr(o["d_c"]), ptr(o["d_e"]),
                 ptr(o["scratch"]), eps, stream())
            call("vag_head_bwd_weights", ptr(d["h2"]), ptr(d["c"]), ptr(d["e"]), R, E, H, V, ptr(o["tmid"]), ptr(o["logits"]), ldl,
                 ptr(o["scratch"]), hg, stream())
    torch.cuda.synchronize()
    o.update({"g_" + k: v for k, v in g.items()})
    del o["scratch"]
    return o


@pytest.mark.parametrize("V", [1000, 2047, 9001, 10243])       # lse_nll's NV = 8, 8 (V % 4 = 3), 40 (V % 4 = 1), streaming (V % 4 = 3)
@pytest.mark.parametrize("eps", [0.1, 0.3])
def test_smoothed_head_operator_matches_fp64(V, eps):
    from vagnmt_hip import ops
    x, tgt = _head_case(V)
    want_loss, want_g, want_nll = _fp64_reference(x, tgt, V, eps)
    # (a) the autograd function
    d = {k: v.to(DEV).requires_grad_(True) for k, v in x.items()}
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    ldl = (V + 3) // 4 * 4
    loss = ops.HeadCESmoothed.apply(d["h2"], d["c"], d["e"], tgt.to(DEV), vw, 0.0, None, None, None, ldl, eps,
                                    *[d[k] for k in HEAD_NAMES])
    loss.backward()
    print("[ls operator] V=%d eps=%.1f loss %.7f (fp64 %.7f)" % (V, eps, float(loss), float(want_loss)))
    for k in x:
        ref = want_g[k].numpy()
        print("   d%-6s max abs err %.3e  scale %.3e" % (k, np.abs(d[k].grad.cpu().double().numpy() - ref).max(), np.abs(ref).max()))
    close(loss, want_loss.numpy(), what="loss_mt")
    for k in x:
        close(d[k].grad, want_g[k].numpy(), what="d " + k)
    # (b) the three _ls entry points on private buffers: per-row nll, the same gradients from both backward forms, and the
    # padding columns of d(logits)
    Tt, B, _ = x["h2"].shape
    for which in ("ls", "ls_data"):
        o = _abi_run(x, tgt, V, eps, which)
        close(o["loss"][0], want_loss.numpy(), what=which + " loss_mt")
        close(o["nll"].view(Tt, B), want_nll.numpy(), what=which + " nll")
        pad_rows = (tgt.t().reshape(-1) == 0).to(DEV)
        assert torch.equal(o["nll"][pad_rows], torch.zeros_like(o["nll"][pad_rows]))        # PAD rows: exactly nothing
        for k in ("h2", "c", "e"):
            close(o["d_" + k], want_g[k].numpy(), what=which + " d " + k)
        for k in HEAD_NAMES:
            close(o["g_" + k], want_g[k].numpy(), what=which + " d " + k)
        dl = o["logits"]                     # now d(logits)
        assert dl.shape[1] == ldl
        if ldl > V:
            assert torch.equal(dl[:, V:], torch.zeros_like(dl[:, V:])), "d(logits) padding columns must stay exactly 0"
        assert torch.equal(dl[pad_rows], torch.zeros_like(dl[pad_rows]))
        # every row of the smoothed gradient still sums to zero: coef * (sum softmax - (1-eps) - eps).  fp32: lse carries an ulp of
        # its own size (1e-6 at lse ~ 10), so sum softmax = 1 + O(1e-6); coef <= 1/B -- 1e-5 leaves an order of magnitude
        assert dl[:, :V].double().sum(-1).abs().max().item() <= 1e-5


# What the library computes reproducibly from run to run -- and so what torch.equal can be asked of.  The loss kernels (lse_nll,
# ce_bwd, ce_bwd_colsum's element-wise result) are: one thread or a fixed-order tree per value.  Sums that meet in fp32 atomics are
# not, once three or more contributions land on one word: the output-bias column sums above two row strips (more than 16 rows), the
# split-K products over the vocabulary (d(tmid) above ~2048 columns) and over the rows.  The PLAIN entry points called twice on
# the same inputs differ there in the last bit (measured on an MI355X: R = 48 rows: g_b1/g_b2/g_b3/g_out_b at V = 1000, every
# gradient behind d(tmid) at V = 10243; R = 16: every gradient behind d(tmid) at V = 2047, nothing at V = 1000 in four runs).
REPRODUCIBLE = ("loss", "lse", "nll", "inv_cnt", "tmid", "logits")          # "logits" holds d(logits) after backward


@pytest.mark.parametrize("V", [1000, 2047, 9001, 10243])
def test_eps_zero_entry_points_are_the_existing_ones_bit_for_bit(V):
    """`_ls` with eps = 0 launches the kernels of the plain loss: losses, lse, nll and d(logits) -- everything the three kernels
    the option touches write -- are identical to the plain entry points' in all three lse_nll regimes, and at a shape where
    the plain entry points reproduce themselves (16 rows, V = 1000) so is every gradient."""
    x, tgt = _head_case(V, seed=1)
    a = _abi_run(x, tgt, V, 0.0, "plain")
    b = _abi_run(x, tgt, V, 0.0, "ls")
    c = _abi_run(x, tgt, V, 0.0, "ls_data")
    assert float(a["loss"]) > 0 and a["logits"].abs().max().item() > 0
    for k in REPRODUCIBLE:
        assert torch.equal(a[k], b[k]), ("vag_head_ce_seq_*_ls(eps=0) differs from the plain entry points", k)
        assert torch.equal(a[k], c[k]), ("vag_head_ce_seq_bwd_data_ls(eps=0) differs from the plain entry points", k)
    for k in a:            # (the rest: equal up to the summation order of the atomics, see above)
        close(b[k], a[k].cpu().double().numpy(), what="eps=0 " + k)
    if V == 1000:
        x, tgt = _head_case(V, B=4, Tt=4, seed=2)
        a = _abi_run(x, tgt, V, 0.0, "plain")
        a2 = _abi_run(x, tgt, V, 0.0, "plain")
        b = _abi_run(x, tgt, V, 0.0, "ls")
        c = _abi_run(x, tgt, V, 0.0, "ls_data")
        for k in a:
            assert torch.equal(a[k], a2[k]), ("the plain entry points do not reproduce themselves at this shape", k)
            assert torch.equal(a[k], b[k]), ("vag_head_ce_seq_*_ls(eps=0) differs from the plain entry points", k,
                                             (a[k] - b[k]).abs().max().item())
        for k in REPRODUCIBLE + ("d_h2", "d_c", "d_e"):
            assert torch.equal(a[k], c[k]), ("vag_head_ce_seq_bwd_data_ls(eps=0)", k, (a[k] - c[k]).abs().max().item())


# ------------------------------------------------------------------------------------------------------------------
# the fused step
# ------------------------------------------------------------------------------------------------------------------
def _model_case(kind, dropout=0.0, seed=3, B=8, Ts=9, Tt=7):
    """A small fused-path model and batch: H = 64, B = 8, Ts = 9, Tt = 7, V = 61 (V % 4 = 1), ragged, with PAD tails."""
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    Vs, Vt, I, E, H, S = 50, 61, 48, 32, 64, 32
    lens = [min(n, Ts) for n in (9, 9, 8, 6, 5, 4, 2, 1)][:B - 1] + [1]
    torch.manual_seed(seed)
    if kind == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, 0.9, dropout_ctx=dropout, dropout_emb=dropout * 0.6,
                                                  dropout_out=dropout, tied_emb=True)
    else:
        m = NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, dropout_ctx=dropout, dropout_emb=dropout * 0.6, dropout_out=dropout, tied_emb=False)
    g = torch.Generator().manual_seed(seed + 1)
    src = torch.zeros(B, Ts, dtype=torch.long)
    for b, n in enumerate(lens):
        src[b, :n] = torch.randint(4, Vs, (n,), generator=g)
    tgt = torch.randint(4, Vt, (B, Tt), generator=g)
    tgt[:, -1] = 3
    for b, n in ((1, 5), (4, 3), (6, 2)):
        if b < B - 1 and n < Tt:
            tgt[b, n - 1] = 3
            tgt[b, n:] = 0
    tgt[B - 1, 0] = 3
    tgt[B - 1, 1:] = 0
    im = torch.randn(B, I, generator=g).abs().to(DEV) if kind == "mm" else None
    return m.to(DEV), (src.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), tgt.to(DEV), im), Vt


def _driver(kind, crit_of, state=None, **kw):
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip.trainer import TrainStep
    m, batch, V = _model_case(kind)
    if state is not None:
        m.load_state_dict(state)
    cv = PairwiseRankingLoss(margin=0.1) if kind == "mm" else None
    kw.setdefault("pad_src", 1)
    return m, TrainStep(m, crit_of(V), cv, **kw), batch


def _visits(ts, batch, teacher, n):
    """n forward+backward passes (no optimiser) through the driver's own graph cache: eager, capture + replay, replay."""
    src, lt, tgt, im = batch
    out = []
    for _ in range(n):
        ts.fp.grad.zero_()
        ts.backend.run(src, lt, tgt, im, teacher, 7)
        torch.cuda.synchronize()
        out.append(([float(v) for v in ts.backend.outputs()],
                    {k: p._vag_grad.detach().clone() for k, p in ts.model.named_parameters()}))
    return out


def _fused_vs_generic(kind, teacher, eps=0.1, visits=3, use_graph=True):
    from vagnmt_hip.trainer import _AutogradBackend, _FusedBackend
    m0, _, _ = _model_case(kind)
    state = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    mg, tsg, batch = _driver(kind, lambda V: _crit(V, eps, _generic_cls()), state, use_graph=False)
    assert type(tsg.backend) is _AutogradBackend
    mg.eval()                                   # dropout off (the models are built without any, too)
    (want_l, want_g), = _visits(tsg, batch, teacher, 1)
    mf, tsf, _ = _driver(kind, lambda V: _crit(V, eps), state, use_graph=use_graph)
    assert type(tsf.backend) is _FusedBackend and tsf.backend.f.label_smoothing == pytest.approx(eps)
    mf.eval()
    runs = _visits(tsf, batch, teacher, visits)
    if use_graph and visits >= 3:
        assert tsf.stats["eager_steps"] == 1 and tsf.stats["captures"] == 1 and tsf.stats["replays"] == visits - 1, tsf.stats
    for i, (got_l, got_g) in enumerate(runs):
        tag = "%s tfr=%s visit %d" % (kind, 1.0 if teacher else 0.0, i)
        worst = max((got_g[k].double() - want_g[k].double()).abs().max().item() / max(1.0, want_g[k].abs().max().item()) for k in want_g)
        print("[ls step] %s: losses %s vs generic %s; worst gradient error / max(1, scale) %.3e" % (tag, got_l, want_l, worst))
        for j, name in enumerate(("loss", "loss_mt", "loss_vse")):
            close(got_l[j], want_l[j], what=tag + " " + name)
        for k in want_g:
            close(got_g[k], want_g[k].cpu().double().numpy(), what=tag + " d " + k)
    return runs[0][0], want_l


@pytest.mark.parametrize("teacher", [True, False], ids=["tfr1", "tfr0"])
@pytest.mark.parametrize("kind", ["mm", "text"])
def test_fused_step_matches_generic_criterion_path(kind, teacher):
    """One step with the criterion (fused: vag_train_step with cfg.label_smoothing) against the same step with a trivial
    subclass of it (generic path: HeadLogp + the criterion's torch forward per time step); eager, captured and replayed."""
    _fused_vs_generic(kind, teacher)


@pytest.mark.parametrize("head_fuse", [1, 0])
def test_fused_step_chunked_head_matches_generic_criterion_path(head_fuse):
    """The head in row chunks of two time steps (Tt = 7: a ragged last chunk): finished inside the forward (head_fuse 1) and
    recomputed by the backward (head_fuse 0)."""
    from vagnmt_hip import _lib as L
    try:
        L.set_option("head_chunk", 2 * 8)
        L.set_option("head_fuse", head_fuse)
        _fused_vs_generic("mm", True)
    finally:
        L.set_option("head_chunk", -1)
        L.set_option("head_fuse", 1)


def test_smoothed_loss_differs_from_the_plain_loss():
    """A path that dropped eps would pass every comparison of two smoothed runs: at eps = 0.1 the fused loss_mt is far
    (more than 10 x the tolerance) from the eps = 0 value on the same batch, in the teacher-forced and the free-running step."""
    for teacher in (True, False):
        out = {}
        for eps in (0.0, 0.1):
            m, ts, batch = _driver("mm", lambda V: _crit(V, eps), use_graph=False)
            m.eval()
            (l, _), = _visits(ts, batch, teacher, 1)
            out[eps] = l
        print("[ls differs] teacher=%s loss_mt eps=0 %.6f, eps=0.1 %.6f" % (teacher, out[0.0][1], out[0.1][1]))
        assert abs(out[0.1][1] - out[0.0][1]) > 10 * TOL * max(1.0, abs(out[0.0][1])), out
        assert out[0.1][2] == out[0.0][2]          # the ranking loss does not know about it


def test_eps_zero_criterion_trains_bit_for_bit_like_nll_loss():
    """Two TrainSteps from the same seed (dropout on), one with nn.NLLLoss and one with LabelSmoothedNLLLoss(eps = 0): five
    optimiser steps through graph replay, teacher-forced and free-running -- every loss and every parameter identical.

    Shape: the text-only model with untied embeddings, B = 2, Ts = 4, Tt = 3.  The step's gradient sums meet in fp32 atomics
    (embedding scatters, split-K slices, bias column sums), so two drivers with the SAME nn.NLLLoss only agree bit for bit
    while no word receives three or more contributions in an order the scheduler decides.  Measured on an MI355X, drivers
    alternating nn.NLLLoss / eps = 0 from one seed: this shape 10 of 10 identical; the multimodal model with tied embeddings at
    the same B (the tied matrix collects the head's out.weight product, the embedding scatter and gru_1's share) 3 of 9 differed
    from the first in the last bit (decoder.embedding.weight 1.9e-9), nn.NLLLoss against nn.NLLLoss included; at B = 8, Ts = 9,
    Tt = 7 every parameter did (<= 6e-8; losses <= 2e-6).  The third driver (nn.NLLLoss again) is the control that says so if
    this shape stops being reproducible."""
    from vagnmt_hip.trainer import TrainStep, _FusedBackend
    res = []
    for which in ("nll", "ls0", "nll"):
        m, batch, V = _model_case("text", dropout=0.5, B=2, Ts=4, Tt=3)
        vw = torch.ones(V, device=DEV)
        vw[0] = 0
        crit = torch.nn.NLLLoss(weight=vw, reduction="none") if which == "nll" else _crit(V, 0.0)
        torch.manual_seed(77)                    # the dropout generator's seed is drawn on the first training step
        ts = TrainStep(m, crit, None, use_graph=True, pad_src=1)
        assert type(ts.backend) is _FusedBackend
        src, lt, tgt, im = batch
        losses = []
        for i in range(5):
            out = ts.step(src, lt, tgt, im, teacher=(i != 3))
            losses.append(torch.stack([v.clone() for v in out]))
        torch.cuda.synchronize()
        assert ts.stats["replays"] >= 3, ts.stats
        ts.check()
        res.append((torch.stack(losses).cpu(), {k: p.detach().clone() for k, p in m.named_parameters()}))
    (la, pa), (lb, pb), (lc, pc) = res
    print("[ls eps=0] losses nll %s\n           losses ls0 %s" % (la[:, 0].tolist(), lb[:, 0].tolist()))
    assert la[0, 0] != la[1, 0] and torch.isfinite(la).all()
    assert torch.equal(la, lc) and all(torch.equal(pa[k], pc[k]) for k in pa), "control: two nn.NLLLoss drivers differ at this shape"
    assert torch.equal(la, lb), (la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, (pa[k] - pb[k]).abs().max().item())


@pytest.mark.parametrize("chunked", [False, True], ids=["whole_head", "chunked_bf16_dlogits_on"])
def test_two_byte_storage_mode_against_fp32_storage(chunked):
    """TrainStep(storage="f16") with eps = 0.1 against the fp32-storage smoothed step on the same batch, at the tolerances
    tests/test_gpu_benched_path.py uses for these quantities in that mode (its _check: losses 2e-3, gradients 1e-2 of each
    tensor's largest entry, per-tensor relative L2 2e-2 with the matching cosine).  Second case: head_bf16_dlogits on and the
    head in row chunks of two time steps (at B = 16, Tt = 12 no chunk is long enough for the bf16 form of d(logits) itself:
    test_two_byte_storage_bf16_dlogits_form_with_smoothing runs that one)."""
    from test_gpu_benched_path import _check
    from test_gpu_round2 import _fp16_case
    from vagnmt_hip import _lib as L
    from vagnmt_hip.trainer import TrainStep
    m_of, (src, lens, tgt, im), cm, cv = _fp16_case("mid")       # H = 64, B = 16, Ts = Tt = 12, ragged
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    V = cm.weight.shape[0]
    out = {}
    try:
        L.set_option("head_bf16_dlogits", 1)
        if chunked:
            L.set_option("head_chunk", 2 * src.shape[0])
        for storage in ("f32", "f16"):
            m = m_of()
            ts = TrainStep(m, _crit(V, 0.1), cv, use_graph=False, storage=storage, pad_src=1)
            m.eval()
            ts.backend.run(src, lt, tgt, im, True, 7)
            torch.cuda.synchronize()
            out[storage] = ([float(v) for v in ts.backend.outputs()],
                            {k: p._vag_grad.detach().clone() for k, p in m.named_parameters()})
    finally:
        L.set_option("head_chunk", -1)
        L.set_option("head_bf16_dlogits", 1)
    l32, g32 = out["f32"]
    l16, g16 = out["f16"]
    print("[ls f16] losses f32 %s f16 %s" % (l32, l16))
    assert l16 != l32                                   # not silently the fp32 path
    _check("ls f16 vs f32" + (" chunked" if chunked else ""), l16, g16, dict(zip(("loss", "loss_mt", "loss_vse"), l32)),
           {k: v.cpu() for k, v in g32.items()}, ltol=2e-3, gtol=1e-2, l2tol=2e-2)


def test_two_byte_storage_bf16_dlogits_form_with_smoothing():
    """The bf16 form of d(logits) (ce_bwd_colsum's out16) needs chunks above 128 rows: the 2-byte mode at H = 1024, B = 256
    with one time step per chunk, eps = 0.1, bf16 d(logits) against fp32 d(logits) in place -- the bound and the shape of
    test_gpu_round3.test_bf16_dlogits_chunks_match_fp32_dlogits_in_the_two_byte_mode (one bf16 rounding of d(logits): 1e-2 of
    each tensor's largest entry; losses untouched), and the smoothed gradient is not the plain one."""
    from test_gpu_round2 import _fp16_case
    from vagnmt_hip import _lib as L
    from vagnmt_hip.trainer import TrainStep
    m_of, (src, lens, tgt, im), cm, cv = _fp16_case("wide")
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    V = cm.weight.shape[0]
    out = {}
    try:
        L.set_option("head_chunk", src.shape[0])
        for flag, eps in ((0, 0.1), (1, 0.1), (1, 0.0)):
            L.set_option("head_bf16_dlogits", flag)
            m = m_of()
            ts = TrainStep(m, _crit(V, eps), cv, use_graph=False, storage="f16", pad_src=1)
            m.eval()
            ts.backend.run(src, lt, tgt, im, True, 7)
            torch.cuda.synchronize()
            out[flag, eps] = ([float(v) for v in ts.backend.outputs()],
                              {k: p._vag_grad.detach().clone() for k, p in m.named_parameters()})
    finally:
        L.set_option("head_chunk", -1)
        L.set_option("head_bf16_dlogits", 1)
    (l0, g0), (l1, g1), (lp, _) = out[0, 0.1], out[1, 0.1], out[1, 0.0]
    assert np.allclose(l0, l1, rtol=1e-6, atol=1e-7), (l0, l1)
    # eps reached the bf16 form: the output-bias gradient (column sums of the smoothed d(logits)) is eps = 10 % away from the
    # plain one in its dominant, one-hot part (an untrained model's softmax is near uniform, so the LOSS barely moves here)
    gb, gbp = g1["decoder.out.bias"], out[1, 0.0][1]["decoder.out.bias"]
    assert (gb - gbp).abs().max().item() > 3e-2 * gbp.abs().max().item(), ((gb - gbp).abs().max().item(), gbp.abs().max().item())
    differs = False
    for k in g0:
        scale = max(g0[k].abs().max().item(), 1e-8)
        err = (g0[k] - g1[k]).abs().max().item()
        assert err <= 1e-2 * scale, (k, err, scale)
        differs = differs or err > 0.0
    assert differs                                           # the bf16 form really ran
