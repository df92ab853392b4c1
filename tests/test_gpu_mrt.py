"""GPU: minimum-risk training -- vag_mrt_weights and vag_mrt_pack against the float64 restatement (tests/mrt_ref.py), the fused
minimum-risk step (vag_step_cfg.mrt_*) against torch autograd over the existing operators, and TrainStep.mrt_step end to end.

Tolerances.  q and risk: the suite's rule, test_gpu_golden.close with TOL = 1e-4.  The coefficients inv_cnt: 1e-4 of the REFERENCE's
own largest coefficient (they are small: an absolute 1e-4 would pass a dropped alpha).  Gradients of the fused step: relative to
each reference tensor's largest entry, GRAD_TOL below."""
import functools

import numpy as np
import pytest
import torch

import mrt_ref as R
from conftest import load_golden
from test_gpu_golden import TOL, close

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64

# The fused step's gradients against autograd's, relative to each reference tensor's largest entry.  Measured on an MI355X on the
# parent commit for the plain NLL step at the shape used here (test_gpu_label_smoothing._model_case: H = 64, V = 61, B = 8, Ts = 9,
# Tt = 7, no ranking criterion), fused step against the generic per-operator path: NLL_STEP_REL_ERR, the worst of both models and
# all parameters (tools/exp_mrt.py prints it; profiles/exp_mrt.txt records it).  Four times that is allowed: the minimum-risk step
# weights the rows of the same sums differently (coefficients of both signs, so more cancellation than the NLL step's).
NLL_STEP_REL_ERR = 7.091e-7          # (mm 7.091e-07, text 6.689e-07; this tree's plain step gives the same two numbers)
GRAD_TOL = 4 * NLL_STEP_REL_ERR


# ------------------------------------------------------------------------------------------------------------------
# vag_mrt_weights
# ------------------------------------------------------------------------------------------------------------------
def _guarded(n, fill=-7.0, dtype=torch.float32):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def _guards_intact(bufs, fill=-7.0):
    for k, v in bufs.items():
        assert bool((v[:GUARD] == fill).all()) and bool((v[-GUARD:] == fill).all()), "guard of %s overwritten" % k


def run_weights(nll, cost, valid, N, alpha, scale, want_q=True, expect=0):
    """vag_mrt_weights at the ABI on numpy inputs; outputs inside guard margins.  Returns (inv_cnt, q or None, risk) CPU tensors
    (as left by the call: the fill value where nothing was written)."""
    from vagnmt_hip._lib import lib, ptr, stream
    Tt, B = nll.shape
    d_nll = torch.as_tensor(nll, dtype=torch.float32).to(DEV).contiguous()
    d_cost = torch.as_tensor(cost, dtype=torch.float32).to(DEV).contiguous()
    d_valid = None if valid is None else torch.as_tensor(valid, dtype=torch.float32).to(DEV).contiguous()
    bufs = {"inv_cnt": _guarded(B), "q": _guarded(B), "risk": _guarded(1)}
    rc = lib().vag_mrt_weights(ptr(d_nll), ptr(d_cost), ptr(d_valid), B, Tt, N, alpha, scale, bufs["inv_cnt"][GUARD:-GUARD].data_ptr(),
                               bufs["q"][GUARD:-GUARD].data_ptr() if want_q else None, bufs["risk"][GUARD:-GUARD].data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    _guards_intact(bufs)
    return bufs["inv_cnt"][GUARD:-GUARD].cpu(), bufs["q"][GUARD:-GUARD].cpu() if want_q else None, bufs["risk"][GUARD:-GUARD].cpu()


def _weights_inputs(kind, N, G, Tt, seed):
    """fp32 inputs of one case, as numpy: (nll (Tt, B), cost (B,), valid (B,) or None, alpha)."""
    g = np.random.default_rng(seed)
    B = G * N
    nll = g.uniform(0.0, 4.0, size=(Tt, B)).astype(np.float32)
    cost = g.uniform(0.0, 1.0, size=B).astype(np.float32)
    valid, alpha = None, 0.5
    if kind == "random_valid":
        valid = (g.uniform(size=B) < 0.7).astype(np.float32)
        valid[g.integers(0, N)::N] = 1.0                      # at least one valid row per group (not always the first)
    elif kind == "one_valid":
        valid = (g.uniform(size=B) < 0.7).astype(np.float32)
        valid[:N] = 0.0                                        # group 0: exactly one valid row
        valid[int(g.integers(0, N))] = 1.0
        valid[N::N] = 1.0
    elif kind == "equal_cost":
        cost[:] = np.float32(0.6180339)
    elif kind == "spread_500":
        # alpha * s spread evenly over 500 within every group (alpha = 2: s from -250 to 0, shared among the Tt steps), shuffled
        alpha = 2.0
        s = -np.linspace(0.0, 250.0, N)
        for gi in range(G):
            nll[:, gi * N:(gi + 1) * N] = (-g.permutation(s) / Tt)[None, :]
        nll = nll.astype(np.float32)
    return nll, cost, valid, alpha


@pytest.mark.parametrize("Tt", [1, 7])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("N", [2, 5, 64, 65, 256])
def test_weights_match_fp64(N, G, Tt):
    scale = 0.25
    for kind in ("random_valid", "one_valid", "equal_cost", "spread_500"):
        nll, cost, valid, alpha = _weights_inputs(kind, N, G, Tt, 1000 * N + 10 * G + Tt)
        want_inv, want_q, want_risk = R.weights(nll, cost, valid, N, alpha, scale)
        inv, q, risk = run_weights(nll, cost, valid, N, alpha, scale)
        tag = "%s N=%d G=%d Tt=%d" % (kind, N, G, Tt)
        assert torch.isfinite(inv).all() and torch.isfinite(q).all() and torch.isfinite(risk).all(), tag
        close(q, want_q, what=tag + " q")
        close(risk, np.array([want_risk]), what=tag + " risk")
        err = np.abs(inv.double().numpy() - want_inv).max()
        if kind == "equal_cost":
            # exactly 0 in exact arithmetic: at most the tolerance
            print("[mrt weights] %s: max |inv_cnt| %.3e (bound %.3e)" % (tag, np.abs(inv.numpy()).max(), TOL))
            assert np.abs(inv.numpy()).max() <= TOL, tag
        else:
            ref_max = np.abs(want_inv).max()
            print("[mrt weights] %s: inv_cnt max err %.3e / ref max %.3e = %.3e" % (tag, err, ref_max, err / max(ref_max, 1e-300)))
            # (a reference maximum of 0 -- one valid row in the only group -- asks for exact zeros; one below fp32's smallest normal
            # number -- N = 2 at a spread of 500: Q = e^-500 -- cannot be written to an fp32 output at all)
            assert err <= TOL * ref_max + float(np.finfo(np.float32).tiny), (tag, err, ref_max)
            assert ref_max > 1e-4 or kind != "random_valid" or N < 5, (tag, ref_max)      # not a vacuous comparison
        if valid is not None:
            off = torch.as_tensor(valid) == 0
            assert not inv[off].any() and not q[off].any(), tag + ": invalid rows must get exactly 0"
        if kind == "one_valid":
            on = np.nonzero(valid[:N])[0]
            assert len(on) == 1 and q[on[0]] == 1.0 and inv[on[0]] == 0.0, tag
        # two runs: the same bits; q = NULL changes nothing else
        inv2, q2, risk2 = run_weights(nll, cost, valid, N, alpha, scale)
        inv3, _, risk3 = run_weights(nll, cost, valid, N, alpha, scale, want_q=False)
        for a, b in ((inv, inv2), (q, q2), (risk, risk2), (inv, inv3), (risk, risk3)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tag + ": not reproducible"


def test_weights_scale_splits_a_step_into_calls():
    """The groups of one step run as two calls with scale = groups of the call / groups of the step: the same coefficients, and
    risks that add up to the step's."""
    N, G, Tt = 5, 4, 3
    nll, cost, valid, alpha = _weights_inputs("random_valid", N, G, Tt, 77)
    inv, q, risk = run_weights(nll, cost, valid, N, alpha, 1.0)
    parts = [run_weights(nll[:, sl], cost[sl], valid[sl], N, alpha, sc) for sl, sc in
             ((slice(0, 3 * N), 0.75), (slice(3 * N, 4 * N), 0.25))]
    # per call the coefficient is -scale N alpha Q (c - R): the backward divides by the call's rows, 3/4 resp. 1/4 of the step's
    want_inv, _, want_risk = R.weights(nll, cost, valid, N, alpha, 1.0)
    got = torch.cat([parts[0][0] / 0.75, parts[1][0] / 0.25])
    assert np.abs(got.double().numpy() - want_inv).max() <= TOL * np.abs(want_inv).max()
    close(parts[0][2] + parts[1][2], np.array([want_risk]), what="risk of two calls")
    close(risk, np.array([want_risk]), what="risk of one call")


def test_weights_einval_cases_launch_nothing():
    nll, cost, valid, alpha = _weights_inputs("random_valid", 4, 2, 3, 5)
    for N, a, sc in ((1, 0.5, 1.0), (3, 0.5, 1.0), (257, 0.5, 1.0), (4, 0.0, 1.0), (4, -0.5, 1.0), (4, float("inf"), 1.0),
                     (4, float("nan"), 1.0), (4, 0.5, 0.0), (4, 0.5, -1.0), (4, 0.5, float("nan"))):
        inv, q, risk = run_weights(nll, cost, valid, N, a, sc, expect=-22)
        assert bool((inv == -7.0).all()) and bool((q == -7.0).all()) and bool((risk == -7.0).all()), (N, a, sc)


# ------------------------------------------------------------------------------------------------------------------
# vag_mrt_pack
# ------------------------------------------------------------------------------------------------------------------
def run_pack(cand, gold, include_gold, Tt=None):
    from vagnmt_hip._lib import call, ptr, stream
    G, Nc, L = cand.shape
    Tg = gold.shape[1]
    N = Nc + include_gold
    Tt = max(L + 1, Tg) if Tt is None else Tt
    c = torch.as_tensor(cand).to(DEV).contiguous()
    gd = torch.as_tensor(gold).to(DEV).contiguous()
    bufs = {"tgt": _guarded(G * N * Tt, -77, torch.int64), "valid": _guarded(G * N)}
    call("vag_mrt_pack", ptr(c, torch.int64), G, Nc, L, ptr(gd, torch.int64), Tg, include_gold,
         bufs["tgt"][GUARD:-GUARD].data_ptr(), Tt, bufs["valid"][GUARD:-GUARD].data_ptr(), stream())
    torch.cuda.synchronize()
    _guards_intact({"tgt": bufs["tgt"]}, -77)
    _guards_intact({"valid": bufs["valid"]})
    return bufs["tgt"][GUARD:-GUARD].view(G * N, Tt).cpu().numpy(), bufs["valid"][GUARD:-GUARD].cpu().numpy()


def _pack_rows(seed, G, Nc, L, Tg):
    """Rows over a three-word vocabulary (repeats are common), an EOS or a padding word now and then; gold rows in the training
    format, one of them equal to its sentence's first candidate's span where that fits."""
    g = np.random.default_rng(seed)
    cand = g.choice(np.array([0, 3, 4, 5, 6], dtype=np.int64), size=(G, Nc, L), p=[0.05, 0.25, 0.3, 0.2, 0.2])
    gold = np.zeros((G, Tg), dtype=np.int64)
    for b in range(G):
        n = int(g.integers(0, Tg))
        gold[b, :n] = g.integers(4, 7, size=n)
        gold[b, n] = 3
    sp = [t for t in R.span(cand[0, 0]) if t != 0][:Tg - 1]
    gold[0] = 0
    gold[0, :len(sp)] = sp
    gold[0, len(sp)] = 3
    return cand, gold


@pytest.mark.parametrize("include_gold", [0, 1])
@pytest.mark.parametrize("L", [1, 6])
@pytest.mark.parametrize("Nc", [1, 7])
def test_pack_matches_reference_exactly(Nc, L, include_gold):
    G = 3
    for Tg, Tt in ((5, None), (2, None), (9, 12)):
        cand, gold = _pack_rows(100 * Nc + 10 * L + Tg, G, Nc, L, Tg)
        want_t, want_v = R.pack(cand, gold, include_gold, Tt)
        got_t, got_v = run_pack(cand, gold, include_gold, Tt)
        assert got_t.shape == want_t.shape and (got_t == want_t).all(), (Nc, L, include_gold, Tg, got_t, want_t)
        assert (got_v == want_v).all(), (Nc, L, include_gold, Tg, got_v, want_v)
        if include_gold:
            assert (got_v.reshape(G, -1)[:, 0] == 1).all()     # a gold row is always valid


def test_pack_edge_rows_and_wide_groups():
    cand, gold, with_gold, without = R.edge_case()
    for include_gold, want_valid in ((1, with_gold), (0, without)):
        got_t, got_v = run_pack(cand, gold, include_gold)
        want_t, want_v = R.pack(cand, gold, include_gold)
        assert (got_t == want_t).all() and (got_v == want_v).all() and (got_v == want_valid).all()
    # more rows than a workgroup has waves, rows longer than a wave: N = 256, L = 70 (an EOS in the second chunk of 64)
    g = np.random.default_rng(3)
    cand = g.integers(4, 6, size=(2, 255, 70)).astype(np.int64)
    cand[:, :, :60] = 4                                        # long common prefixes: equality is decided late in the row
    cand[:, ::3, 66] = 3
    cand[0, 17, 2] = 0
    gold = np.full((2, 71), 4, dtype=np.int64)
    gold[:, 70] = 3
    gold[0, :70] = cand[0, 5]                                  # the gold sentence is candidate 5's span (which holds no EOS)
    gold[0, 66:70] = cand[0, 5, 66:70]
    got_t, got_v = run_pack(cand, gold, 1)
    want_t, want_v = R.pack(cand, gold, 1)
    assert (got_t == want_t).all() and (got_v == want_v).all()
    assert 0 < got_v.sum() < got_v.size


# ------------------------------------------------------------------------------------------------------------------
# the fused minimum-risk step against autograd over the existing operators
# ------------------------------------------------------------------------------------------------------------------
ALPHA = 0.5

# Reference gradients whose largest entry does not reach 1e-3 in the step case below (measured on an MI355X: 2.7e-4 .. 9.9e-4; every
# other tensor 2e-3 .. 6e-2).  All six lie behind a softmax over the source positions of an UNTRAINED model -- the decoder
# attention's query and key projections, and the visual attention with the image projection that feeds only it (no ranking loss in a
# minimum-risk step).  Such a softmax is nearly uniform, and the gradient through it is the weights times the SPREAD of the attended
# values' gradients around their mean, an order of magnitude below the gradient of the values themselves; alpha, the model and the
# batch are fixed by the case, and the candidates move every tensor by the same factor.  They are compared like the rest, relative to
# their own maximum; for them "not vacuous" is asserted at 1e-4, still three orders above the error bound's absolute size.
SMALL_GRADS = ("decoder.attn.attn_h.weight", "decoder.attn.attn_e.weight", "vse_imagine.imagine_attn.ctx2ctx.weight",
               "vse_imagine.imagine_attn.emb2ctx.weight", "vse_imagine.im_embedding.weight", "vse_imagine.im_embedding.bias")


@functools.lru_cache(maxsize=None)
def _step_case(kind):
    """G = 2 source sentences x N = 4 fixed candidates on test_gpu_label_smoothing._model_case's model and batch (rows 0 and 3 of
    it, each four times): the gold row, two other rows, and a repeat of one of them (invalid).  Returns the model's state, the
    expanded batch, the forced rows, their validity and cost, and the autograd reference (risk, gradients), computed once."""
    from test_gpu_label_smoothing import _model_case
    m, (src, lens, tgt, im), V = _model_case(kind)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pick = torch.tensor([0, 3], device=DEV)
    gold = tgt[pick].cpu().numpy()                             # (2, 7): full-length rows with their EOS last
    g = np.random.default_rng(11)
    cand = g.integers(4, V, size=(2, 3, 6)).astype(np.int64)   # six words and no EOS: every row has the gold rows' seven tokens, so
    cand[:, 0, :3] = gold[:, :3]                               # the scores differ by words, not by lengths, and Q stays spread out
    cand[:, 1, 4:6] = gold[:, 4:6]                             # two partial matches of different cost
    cand[0, 2] = cand[0, 1]                                    # a repeat: invalid
    cand[1, 2] = cand[1, 0]
    rows, valid = R.pack(cand, gold, True)                     # (8, 7)
    assert valid.tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    cost = R.bleu_cost(rows, gold, 4).astype(np.float32)
    rep = lambda t: None if t is None else t[pick].repeat_interleave(4, 0).contiguous()      # noqa: E731
    batch = (rep(src), rep(lens), torch.from_numpy(rows).to(DEV), rep(im))
    want = _autograd_reference(m, batch, valid, cost, V)
    return state, batch, valid, cost, V, want


def _row_scores(m, batch, V):
    """log p(row | source) of every forced row, with a graph: the encoder / decoder-init / ops.cgru_decode_seq / ops.HeadLogp chain
    of models/_seq2seq.py's generic criterion branch."""
    from vagnmt_hip import ops
    src, lens, rows, im = batch
    dec = m.decoder
    B, Tt = rows.shape
    if im is not None:
        enc, mask, _, h0 = m._prologue(src, lens, im, None, None)
    else:
        enc, mask, h0 = m._prologue(src, lens, None)
    pe = ops.KeysProj.apply(enc, dec.attn.attn_e.weight)
    tok = torch.cat([torch.full((1, B), 2, dtype=torch.int64, device=DEV), rows.t()], 0).contiguous()
    h2, c, e = ops.cgru_decode_seq(enc, pe, mask, h0, tok, dec.embedding.weight, dec.dec_params(), V=V)
    H = h2.shape[2]
    logp = ops.HeadLogp.apply(h2.view(Tt * B, H), c.view(Tt * B, 2 * H), e.view(Tt * B, -1), 0.0, None, *dec.head_params())
    picked = logp.view(Tt, B, V).gather(2, rows.t().unsqueeze(2)).squeeze(2)          # (Tt, B)
    return (picked.double() * (rows.t() != 0).double()).sum(0)


def _autograd_reference(m, batch, valid, cost, V):
    m.eval()
    m.zero_grad()
    s = _row_scores(m, batch, V)
    ok = torch.as_tensor(valid).to(DEV) != 0
    c = torch.as_tensor(cost, dtype=torch.float64).to(DEV)
    risk = 0.0
    for g in range(2):
        idx = torch.nonzero(ok[4 * g:4 * g + 4]).flatten() + 4 * g
        Q = torch.softmax(ALPHA * s[idx], 0)
        risk = risk + (Q * c[idx]).sum()
    risk = risk / 2
    risk.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    q_max = max(float(torch.softmax(ALPHA * s[torch.nonzero(ok[4 * g:4 * g + 4]).flatten() + 4 * g], 0).max()) for g in range(2))
    return float(risk), grads, q_max


def _fused_driver(kind, state, **kw):
    from test_gpu_label_smoothing import _model_case
    from vagnmt_hip.trainer import TrainStep, _FusedBackend
    m, _, V = _model_case(kind)
    m.load_state_dict(state)
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    kw.setdefault("pad_src", 1)
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, **kw)
    assert type(ts.backend) is _FusedBackend
    m.eval()
    return m, ts


def _grads(ts):
    return {k: p._vag_grad.detach().clone() for k, p in ts.model.named_parameters()}


def _compare(tag, got_risk, got_g, want, tol=GRAD_TOL):
    want_risk, want_g, _ = want
    worst = 0.0
    for k in want_g:
        scale = want_g[k].abs().max().item()
        err = (got_g[k].double() - want_g[k].double()).abs().max().item()
        if scale == 0.0:
            assert err == 0.0, (tag, k, err)                   # (the text projection of the visual grounding: no ranking loss, no gradient)
            continue
        worst = max(worst, err / scale)
    print("[mrt step] %s: risk %.7f (autograd %.7f); worst gradient error / reference max %.3e (allowed %.3e)"
          % (tag, got_risk, want_risk, worst, tol))
    close(got_risk, want_risk, what=tag + " risk")
    for k in want_g:
        scale = want_g[k].abs().max().item()
        err = (got_g[k].double() - want_g[k].double()).abs().max().item()
        assert err <= tol * scale, "%s: d %s max abs err %.3e > %.3e x reference max %.3e" % (tag, k, err, tol, scale)


def _mrt_visits(ts, batch, valid, cost, n, scale=1.0):
    src, lens, rows, im = batch
    out = []
    for _ in range(n):
        ts.fp.grad.zero_()
        ts.backend.run(src, lens, rows, im, True, 7, mrt=(4, ALPHA, scale, torch.as_tensor(cost).to(DEV), torch.as_tensor(valid).to(DEV)))
        torch.cuda.synchronize()
        out.append(([float(v) for v in ts.backend.outputs()], _grads(ts)))
    return out


@pytest.mark.parametrize("kind", ["mm", "text"])
def test_fused_mrt_step_matches_autograd(kind):
    state, batch, valid, cost, V, want = _step_case(kind)
    want_risk, want_g, q_max = want
    nonzero = {k: v.abs().max().item() for k, v in want_g.items() if v.abs().max().item() > 0}
    print("[mrt step] %s: reference gradient maxima %s; largest Q %.3f" % (kind, {k: "%.2e" % v for k, v in nonzero.items()}, q_max))
    # the comparison is not vacuous: every reference gradient's largest entry exceeds 1e-3, except the tensors of SMALL_GRADS
    small = {k: v for k, v in nonzero.items() if k in SMALL_GRADS}
    assert all(v > 1e-3 for k, v in nonzero.items() if k not in SMALL_GRADS), nonzero
    assert all(v > 1e-4 for v in small.values()), small
    assert set(want_g) - set(nonzero) <= {"vse_imagine.text_embedding.weight", "vse_imagine.text_embedding.bias"}
    assert q_max < 0.9                                          # alpha = 0.5 keeps Q away from one-hot on these short rows
    m, ts = _fused_driver(kind, state, use_graph=True)
    runs = _mrt_visits(ts, batch, valid, cost, 3)
    assert ts.stats["eager_steps"] == 1 and ts.stats["captures"] == 1 and ts.stats["replays"] == 2, ts.stats
    for i, (l, g) in enumerate(runs):
        assert l[0] == l[1] and l[2] == 0.0                     # loss = risk (loss_w is 1 for the call), no ranking loss
        _compare("%s visit %d" % (kind, i), l[1], g, want)
    ts.check()                                                  # the result ring is in step with the host's count


def test_fused_mrt_step_chunked_head_recomputes_in_backward():
    """The head in row chunks of two time steps (Tt = 7: a ragged last chunk) with head_fuse on: a minimum-risk step must not
    finish its chunks inside the forward (their coefficients do not exist yet)."""
    from vagnmt_hip import _lib as L
    state, batch, valid, cost, V, want = _step_case("mm")
    try:
        L.set_option("head_chunk", 2 * 8)
        m, ts = _fused_driver("mm", state, use_graph=True)
        for i, (l, g) in enumerate(_mrt_visits(ts, batch, valid, cost, 3)):
            _compare("chunked visit %d" % i, l[1], g, want)
    finally:
        L.set_option("head_chunk", -1)


def test_fused_mrt_step_in_two_chunks_of_one_group():
    """max_rows = 4: two forced passes of one group each with mrt_scale = 1/2; the risks add up and the gradients accumulate."""
    from vagnmt_hip import mrt
    state, batch, valid, cost, V, want = _step_case("mm")
    src, lens, rows, im = batch
    m, ts = _fused_driver("mm", state, use_graph=True)
    for i in range(3):
        ts.fp.grad.zero_()
        risk = mrt._run_groups(ts.backend, 2, 4, ALPHA, 4, rows, torch.as_tensor(valid).to(DEV), torch.as_tensor(cost).to(DEV),
                               src, lens, im, 7)
        torch.cuda.synchronize()
        _compare("two chunks visit %d" % i, float(risk), _grads(ts), want)
    assert ts.stats["captures"] == 1 and ts.stats["eager_steps"] == 1 and ts.stats["replays"] == 5, ts.stats


def test_mrt_gradient_is_not_the_nll_gradient():
    """A step that ignored mrt_* would compute the plain step's gradient on the same rows: the two differ by more than ten times the
    tolerance, relative to the reference's largest entry, in every parameter that has a gradient."""
    state, batch, valid, cost, V, want = _step_case("mm")
    src, lens, rows, im = batch
    m, ts = _fused_driver("mm", state, use_graph=False)
    ts.fp.grad.zero_()
    ts.backend.run(src, lens, rows, im, True, 7)
    torch.cuda.synchronize()
    plain = _grads(ts)
    (l, g), = _mrt_visits(ts, batch, valid, cost, 1)
    for k, ref in want[1].items():
        scale = ref.abs().max().item()
        if scale == 0.0:
            continue
        diff = (plain[k].double() - ref.double()).abs().max().item()
        assert diff > 10 * GRAD_TOL * scale, (k, diff, scale)
    assert abs(l[1] - want[0]) <= TOL


def test_mrt_off_is_the_plain_step_bit_for_bit():
    """mrt_n = 0 with the other mrt_* fields set to anything is the plain step: losses and gradients are bitwise those of a
    zero-initialised tail of vag_step_cfg, at a shape where the plain step reproduces itself
    (test_gpu_label_smoothing.test_eps_zero_criterion_trains_bit_for_bit_like_nll_loss: text model, untied, B = 2, Ts = 4, Tt = 3)."""
    import ctypes as C
    from test_gpu_label_smoothing import _model_case
    from vagnmt_hip._lib import call, ptr, stream
    from vagnmt_hip.trainer import TrainStep
    res = []
    for tail in ("zero", "set", "zero"):
        m, (src, lens, tgt, im), V = _model_case("text", B=2, Ts=4, Tt=3)
        vw = torch.ones(V, device=DEV)
        vw[0] = 0
        ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, use_graph=False, pad_src=1)
        m.eval()
        f = ts.backend.f
        f.reserve(2, 4, 3)
        f.load_batch(src, lens, tgt, im)
        c = f.cfg(2, 4, 3, True, False)
        if tail == "set":
            c.mrt_alpha, c.mrt_scale, c.mrt_cost, c.mrt_valid = 0.5, 0.25, ptr(f.mrt_cost), ptr(f.mrt_valid)
        assert c.mrt_n == 0
        ts.fp.grad.zero_()
        call("vag_train_step", c.ref(), C.byref(f.w), C.byref(f.g), ptr(f.src, torch.int64), ptr(f.lens, torch.int32),
             ptr(f.tgt, torch.int64), None, ptr(f.vw), None, ptr(f.derived), ptr(f.ws), ptr(f.losses), 7, stream())
        torch.cuda.synchronize()
        res.append((f.losses[:3].clone(), ts.fp.grad.clone()))
    (la, ga), (lb, gb), (lc, gc) = res
    assert float(la[0]) > 0 and ga.abs().max().item() > 0
    assert torch.equal(la, lc) and torch.equal(ga, gc), "control: the plain step does not reproduce itself at this shape"
    assert torch.equal(la, lb) and torch.equal(ga, gb)


# ------------------------------------------------------------------------------------------------------------------
# TrainStep.mrt_step
# ------------------------------------------------------------------------------------------------------------------
def _golden_driver(name, **kw):
    from test_gpu_golden import build
    from vagnmt_hip.trainer import TrainStep
    meta, P, z = load_golden(name)
    m = build(meta, P)
    V = meta["dims"][1]
    vw = torch.ones(V, device=DEV)
    vw[0] = 0
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, **kw)
    src, tgt = torch.from_numpy(z["src"]).to(DEV), torch.from_numpy(z["tgt"]).to(DEV)
    im = torch.from_numpy(z["im"]).to(DEV) if meta["kind"] == "mm" else None
    return meta, z, m, ts, (src, torch.tensor(meta["lengths"], dtype=torch.int32, device=DEV), tgt, im)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_it_learns(use_graph):
    """Five mrt_steps on one batch with a fixed candidate set and no dropout: expected_risk falls at every step, as the float64
    reference does (tests/test_mrt_host.py checks that on the oracle at the same rate and seed)."""
    from vagnmt_hip import mrt
    L = R.LEARN
    meta, z, m, ts, (src, lens, tgt, im) = _golden_driver(L["golden"], lr=L["lr"], use_graph=use_graph, pad_src=1)
    cand_np = R.learn_candidates(z["tgt"], meta["dims"][1])
    cand = torch.from_numpy(cand_np).to(DEV)
    risks, stepped = [], []
    for _ in range(L["steps"]):
        risks.append(mrt.expected_risk(ts, src, lens, tgt, im, cand, L["alpha"]))
        stepped.append(ts.mrt_step(src, lens, tgt, im, alpha=L["alpha"], candidates=cand))
    risks.append(mrt.expected_risk(ts, src, lens, tgt, im, cand, L["alpha"]))
    torch.cuda.synchronize()
    ts.check()
    risks = [float(r) for r in risks]
    print("[mrt learns] " + " ".join("%.6f" % r for r in risks))
    for a, b in zip(risks, risks[1:]):
        assert b < a, risks
    for r, s in zip(risks, stepped):
        assert float(s.risk) == pytest.approx(r, abs=2e-6)      # a step reports the risk before its update
        assert float(s.bleu) == pytest.approx(1.0 - r, abs=2e-6) and s.n_valid.tolist() == [4.0] * 5
    _, P, _ = load_golden(L["golden"])
    want = R.learn_reference(P, z["src"], meta["lengths"], z["tgt"], cand_np)
    print("[mrt learns] float64 reference " + " ".join("%.6f" % r for r in want))
    close(risks[0], want[0], what="the risk before any step against the float64 reference")


@pytest.mark.parametrize("method", ["stochastic", "sample"])
@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_mrt_step_end_to_end(name, method):
    """Candidates drawn on the current weights, twice (the second visit goes through the captured graphs); then a plain step and
    a beam decode on the updated weights."""
    from vagnmt_hip.sampling import Generator
    meta, z, m, ts, (src, lens, tgt, im) = _golden_driver(name, use_graph=True, pad_src=1)
    gen = Generator(7)
    before = m.decoder.out.bias.detach().clone()
    v0 = getattr(m, "_vag_weights_version", 0)
    m.eval()
    dec0 = m._decode(src, meta["lengths"], im, 2, 8, None)     # builds the decode tables of the initial weights
    for visit in range(2):
        out = ts.mrt_step(src, lens, tgt, im, n_candidates=6, alpha=0.05, method=method, generator=gen, max_length=7)
        torch.cuda.synchronize()
        nv = out.n_valid.cpu()
        print("[mrt e2e] %s %s visit %d: risk %.5f bleu %.5f n_valid %s" % (name, method, visit, float(out.risk), float(out.bleu), nv.tolist()))
        assert out.n_valid.shape == (5,) and bool((nv >= 1).all()) and bool((nv <= 7).all())
        assert np.isfinite(float(out.risk)) and 0.0 <= float(out.risk) <= 1.0 and float(out.bleu) == pytest.approx(1 - float(out.risk), abs=1e-6)
    assert getattr(m, "_vag_weights_version", 0) == v0 + 2
    assert not torch.equal(before, m.decoder.out.bias)
    # the gold row is valid: the rows mrt_step forms from candidates drawn the same way keep candidate 0 of every sentence, and
    # that row is the gold sentence in the training format
    from vagnmt_hip import mrt
    cand = mrt._draw(ts, src, lens, im, 6, 7, method, gen)
    rows, valid, cost, N, _, _, _ = mrt._prepare(src, lens, tgt, im, cand, 1)
    torch.cuda.synchronize()
    assert N == 7 and valid.view(5, N)[:, 0].tolist() == [1.0] * 5
    assert torch.equal(rows.view(5, N, -1)[:, 0, :tgt.shape[1]], tgt) and not rows.view(5, N, -1)[:, 0, tgt.shape[1]:].any()
    assert cost.view(5, N)[:, 0].abs().max().item() <= 1e-6         # ... whose BLEU against itself is 1
    loss = ts.step(src, lens, tgt, im, teacher=True)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in loss)
    ts.check()
    m.eval()
    cur = getattr(m, "_vag_weights_version", 0)
    assert cur == v0 + 3
    wcache = m.__dict__["_decode_wcache"]
    assert all(e["ver"][0] < cur for e in wcache.values())     # (the draws of the second visit saw version v0 + 1)
    dec1 = m._decode(src, meta["lengths"], im, 2, 8, None)
    assert any(e["ver"][0] == cur for e in wcache.values()), "the decode tables were not refreshed after the optimiser steps"
    assert len(dec1) == len(dec0) == 5
