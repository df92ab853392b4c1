"""GPU: word-level confidence -- vag_token_conf at the ABI against tests/confidence_ref.py (exact at M = 1, inside the reference's
own bound for the entropy, within delta_s of the float64 order at M > 1), against vag_forced_score and vag_kd_targets on the same
inputs, and the Python layer (token_confidence, translation_confidence, mc_dropout_confidence, corpus_perplexity) on the golden
fixtures.

Shapes: B = 5, Tt = 6 (confidence_ref.targets: words after the first EOS, no EOS with a pad inside the span, an all-pad row, one
word, gold word V - 1); V = 5 is less than one lane round, 67 just over a wave, 1031 has every lane looping with V % 4 = 3, 2047 two
rounds of 16-byte loads; ldl = ceil4(V) and one odd ldl (the scalar path).  Outputs lie inside guard margins of 64 elements, inputs
are followed by NaN, the padding columns [V, ldl) hold 99."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import confidence_ref as R
from conftest import load_golden
from test_gpu_nbest_score import golden_model, make_model, span_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
CASES = [(V, None) for V in R.VS] + [(67, 69)]
OUTS = (("token_logp", 1, torch.float32), ("entropy", 1, torch.float32), ("rank", 1, torch.int32), ("top", 2, torch.int32),
        ("top_logp", 2, torch.float32))


def _dev_inputs(xs, ls):
    """Device copies of the members' logits / lse, each followed by 64 NaN floats."""
    out = []
    for a in list(xs) + list(ls):
        buf = torch.full((a.size + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        buf[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        out.append(buf)
    return out[:len(xs)], out[len(xs):]


def run_conf(xs, ls, tgt, V):
    """vag_token_conf at the ABI on M members' numpy logits (R, ldl) and lse (R,); every output inside guard margins."""
    from vagnmt_hip._lib import lib, stream
    M = len(xs)
    Bn, Tt = tgt.shape
    dx, dl = _dev_inputs(xs, ls)
    tg = torch.from_numpy(np.asarray(tgt)).to(DEV)
    bufs = {k: torch.full((Bn * Tt * w + 2 * GUARD,), -7, dtype=dt, device=DEV) for k, w, dt in OUTS}
    bufs["sent"] = torch.full((Bn * R.SENT + 2 * GUARD,), -7.0, dtype=torch.float32, device=DEV)
    p = lambda k: bufs[k][GUARD:-GUARD].data_ptr()          # noqa: E731
    rc = lib().vag_token_conf((C.c_void_p * M)(*[x.data_ptr() for x in dx]), (C.c_int64 * M)(*[x.shape[1] for x in xs]),
                              (C.c_void_p * M)(*[x.data_ptr() for x in dl]), M, tg.data_ptr(), Bn, Tt, V, p("token_logp"),
                              p("entropy"), p("rank"), p("top"), p("top_logp"), p("sent"), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, v in bufs.items():
        assert bool((v[:GUARD] == -7).all()) and bool((v[-GUARD:] == -7).all()), "guard of %s overwritten" % k
    out = {k: bufs[k][GUARD:-GUARD].view(*((Bn, Tt) + ((w,) if w > 1 else ()))).cpu().numpy() for k, w, _ in OUTS}
    out["sent"] = bufs["sent"][GUARD:-GUARD].view(Bn, R.SENT).cpu().numpy()
    return out


def run_forced(xs, ls, tgt, V):
    from vagnmt_hip._lib import lib, stream
    M = len(xs)
    Bn, Tt = tgt.shape
    dx, dl = _dev_inputs(xs, ls)
    tg = torch.from_numpy(np.asarray(tgt)).to(DEV)
    tok, logp, score = torch.empty(Bn, Tt, device=DEV), torch.empty(Bn, device=DEV), torch.empty(Bn, device=DEV)
    rc = lib().vag_forced_score((C.c_void_p * M)(*[x.data_ptr() for x in dx]), (C.c_int64 * M)(*[x.shape[1] for x in xs]),
                                (C.c_void_p * M)(*[x.data_ptr() for x in dl]), M, tg.data_ptr(), Bn, Tt, V, tok.data_ptr(),
                                logp.data_ptr(), score.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return tok.cpu().numpy(), logp.cpu().numpy(), score.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@functools.lru_cache(maxsize=None)
def _tied(V, ldl):
    x, lse, tgt = R.tied_case(V, ldl)
    return x, lse, tgt, R.reference(x, lse, tgt, V), R.restate_fp32(x, lse, tgt, V), run_conf(x, lse, tgt, V)


@functools.lru_cache(maxsize=None)
def _random(V, M):
    x, lse, tgt = R.random_case(V, M)
    return x, lse, tgt, R.reference(x, lse, tgt, V), run_conf(x, lse, tgt, V)


def _worst(got, ref):
    k = ref["keep"]
    return float((np.abs(got["entropy"].astype(np.float64) - ref["entropy"])[k] / ref["bound"][k]).max())


def _outside_is_blank(got, keep):
    o = ~keep
    assert (got["token_logp"][o] == 0).all() and (got["entropy"][o] == 0).all() and (got["top_logp"][o] == 0).all()
    assert (got["rank"][o] == -1).all() and (got["top"][o] == -1).all()


# ------------------------------------------------------------------------------------------------------------------
# 1. M = 1, exact
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", CASES)
def test_single_model_exact_under_ties(V, ldl):
    x, lse, tgt, ref, f32, got = _tied(V, ldl)
    k = ref["keep"]
    if V >= 1031:                                                # the case is what it says: hundreds of ties with the given word
        s = f32["s"]
        assert sum(int((s[t * R.B + b] == s[t * R.B + b][tgt[b, t]]).sum()) for b, t in zip(*np.nonzero(k))) > 100 * 5
    for name in ("rank", "top"):                                 # every position, none excluded (outside the span: -1)
        assert np.array_equal(got[name], f32[name]), (name, np.argwhere(got[name] != f32[name])[:5])
    for name in ("token_logp", "top_logp"):
        assert np.array_equal(bits(got[name]), bits(f32[name])), name
    _outside_is_blank(got, k)
    print("[conf] M=1 V=%d ldl=%s: worst |dH| / bound %.3f" % (V, ldl, _worst(got, ref)))
    assert _worst(got, ref) <= 1.0
    b, t = R.UNIFORM
    assert abs(float(got["entropy"][b, t]) - np.log(V)) <= ref["bound"][b, t] + R.uniform_slack(V)
    assert got["rank"][b, t] == tgt[b, t]
    for b, t in (R.PEAKED, R.NEG_INF):
        assert np.isfinite(got["entropy"][b, t]) and np.isfinite(got["top_logp"][b, t]).all()
    assert got["top"][R.PEAKED][0] == V // 2
    assert same_bits(got, run_conf(x, lse, tgt, V))               # two runs: the same bits in every output


# ------------------------------------------------------------------------------------------------------------------
# 2. agreement with the existing kernels on the same inputs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldl", CASES)
def test_agrees_with_forced_score_and_kd_targets(V, ldl):
    from test_gpu_distill import run_targets
    x, lse, tgt, ref, _, got = _tied(V, ldl)
    tok, logp, score = run_forced(x, lse, tgt, V)
    assert np.array_equal(bits(got["token_logp"]), bits(tok))
    assert np.array_equal(bits(got["sent"][:, 0]), bits(logp)) and np.array_equal(bits(got["sent"][:, 1]), bits(score))
    if ldl is None:                                              # (run_targets takes ldl from a dense tensor)
        idx, _ = run_targets([torch.from_numpy(x[0]).to(DEV)], [torch.from_numpy(lse[0]).to(DEV)], V, 2, 1.0)
        idx = idx.reshape(R.TT, R.B, 2).transpose(1, 0, 2)       # rows t*B + b -> (B, Tt, 2)
        assert np.array_equal(got["top"][ref["keep"]], idx[ref["keep"]])


@pytest.mark.parametrize("V", R.VS)
def test_ensemble_agrees_with_forced_score(V):
    x, lse, tgt, _, got = _random(V, 3)
    tok, logp, score = run_forced(x, lse, tgt, V)
    assert np.array_equal(bits(got["token_logp"]), bits(tok))
    assert np.array_equal(bits(got["sent"][:, 0]), bits(logp)) and np.array_equal(bits(got["sent"][:, 1]), bits(score))


# ------------------------------------------------------------------------------------------------------------------
# 3. M = 3 and M = 8, random members
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 8])
@pytest.mark.parametrize("V", R.VS)
def test_ensemble_within_rounding_of_fp64(V, M):
    x, lse, tgt, ref, got = _random(V, M)
    k, s = ref["keep"], ref["s"]
    _outside_is_blank(got, k)
    worst = 0.0
    for b, t in zip(*np.nonzero(k)):                             # every span position
        row, y = s[t * R.B + b], int(tgt[b, t])
        d = float(R.delta_s(row[y]))
        lo, hi = int((row > row[y] + d).sum()), int((row >= row[y] - d).sum()) - 1
        assert lo <= got["rank"][b, t] <= hi, (b, t, got["rank"][b, t], lo, hi)
        srt = np.sort(row)[::-1]
        i0, i1 = (int(i) for i in got["top"][b, t])
        assert 0 <= i0 < V and 0 <= i1 < V and i0 != i1
        assert abs(row[i0] - srt[0]) <= R.delta_s(srt[0]) and abs(row[i1] - srt[1]) <= R.delta_s(srt[1]), (b, t)
        assert abs(got["top_logp"][b, t, 0] - row[i0]) <= R.delta_s(row[i0]) and abs(got["top_logp"][b, t, 1] - row[i1]) <= R.delta_s(row[i1])
        assert abs(got["token_logp"][b, t] - row[y]) <= d
        worst = max(worst, abs(got["top_logp"][b, t, 0] - srt[0]) / float(R.delta_s(srt[0])))
    print("[conf] M=%d V=%d: worst |dH| / bound %.3f, worst best-score error / delta %.3f" % (M, V, _worst(got, ref), worst))
    assert _worst(got, ref) <= 1.0
    # M identical members: the single model bit for bit in every output
    xs, ls, _ = R.random_case(V, M, same=True)
    assert same_bits(run_conf(xs[:1], ls[:1], tgt, V), run_conf(xs, ls, tgt, V))


# ------------------------------------------------------------------------------------------------------------------
# 4. the sentence values from the device's own per-position values
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,V,ldl", [("tied", V, ldl) for V, ldl in CASES] + [("random", 1031, None)])
def test_sentence_values(which, V, ldl):
    if which == "tied":
        tgt, got = _tied(V, ldl)[2], _tied(V, ldl)[5]
    else:
        tgt, got = _random(V, 3)[2], _random(V, 3)[4]
    want = R.sentence_values(tgt, got["token_logp"], got["entropy"], got["rank"])
    sb = R.sentence_bounds(tgt, got["token_logp"], got["entropy"])
    sent = got["sent"].astype(np.float64)
    for c in (2, 4, 6):                                          # n, min token_logp, max entropy: exact
        assert np.array_equal(sent[:, c], want[:, c]), c
    keep = R.span_mask(tgt)
    first = np.array([np.float32((got["rank"][b][keep[b]] == 0).sum()) / np.float32(max(1, keep[b].sum())) for b in range(R.B)])
    assert np.array_equal(got["sent"][:, 7], first.astype(np.float32))       # the share: one fp32 division of two small integers
    for c in (0, 1, 3, 5):
        err = np.abs(sent[:, c] - want[:, c])
        print("[conf] %s sent[:, %d]: worst err / bound %.3f" % (which, c, float((err / np.maximum(sb[:, c], 1e-300)).max())))
        assert (err <= sb[:, c]).all(), (c, err, sb[:, c])
    assert want[:, 2].tolist() == [3, 3, 0, 1, 6] and got["sent"][2].tolist() == [0.0] * R.SENT        # the all-pad row
    assert got["sent"][3, 3] == 0.0                              # one word: no spread


# ------------------------------------------------------------------------------------------------------------------
# 5. model level
# ------------------------------------------------------------------------------------------------------------------
def restate_rows(m, src, lens, im, tgt):
    """float64 log-probability ROWS (B, Tt, V) from the oracle's prologue and decoder step, teacher forced
    (test_gpu_nbest_score.restate_token_logp with the whole row kept)."""
    from oracle import vag_oracle as O
    P = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
    mm = hasattr(m, "vse_imagine")
    src, tgt = src.cpu(), tgt.cpu()
    with torch.no_grad():
        enc, mask, h = O._decode_prologue(P, src, lens, im.cpu().double() if mm else None, 0.5, getattr(m, "attn_model", "dot"), True)
        pe = enc.transpose(0, 1) @ P["decoder.attn.attn_e.weight"].t()
        Bn, Tt = tgt.shape
        tok = torch.full((Bn,), 2, dtype=torch.long)
        rows = []
        for t in range(Tt):
            logp, h, _ = O.decoder_step(P, tok, h, enc, mask, pe=pe)
            rows.append(logp)
            tok = tgt[:, t]
    return torch.stack(rows, 1).numpy()


def _golden_batch(name):
    m, meta, z = golden_model(name)
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
    tgt = torch.from_numpy(z["tgt"]).cuda()
    tgt[0, 2] = 3                                                # words after the first EOS
    return m, meta, src, im, tgt


def _args(meta, src, lens, tgt, im):
    return (src, lens, tgt) + ((im,) if meta["kind"] == "mm" else ())


@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_model_confidence_against_scoring_and_the_oracle(name):
    from vagnmt_hip import confidence
    m, meta, src, im, tgt = _golden_batch(name)
    lens = meta["lengths"]
    m.train()
    got = m.token_confidence(*_args(meta, src, lens, tgt, im))
    assert m.training                                            # the flag is restored
    sc = m.score_translations(*_args(meta, src, lens, tgt, im))
    m.eval()
    assert torch.equal(got.score, sc.score) and torch.equal(got.logp, sc.logp) and torch.equal(got.token_logp, sc.token_logp)
    assert got.rank.dtype == torch.int32 and got.top.shape == tgt.shape + (2,) and got.sentence.shape == (tgt.shape[0], 8)
    lp = restate_rows(m, src, lens, im, tgt)                     # (B, Tt, V) float64
    keep = span_mask(tgt).numpy() > 0
    p = np.exp(lp)
    H = -(p * lp).sum(-1)
    tol = 2 * 1e-4 * (p * np.abs(lp + H[..., None])).sum(-1)     # first-order sensitivity to a 1e-4 error of every log-probability
    err = np.abs(got.entropy.cpu().double().numpy() - H)
    print("[conf] %s: entropy worst err / tolerance %.3f (tolerance %.2e .. %.2e)" % (name, (err / tol)[keep].max(), tol[keep].min(), tol[keep].max()))
    assert (err[keep] <= tol[keep]).all()
    srt = np.sort(lp, -1)
    clear = keep & (srt[..., -1] - srt[..., -2] > 2e-4)
    y = tgt.cpu().numpy()
    lead = lp.argmax(-1) == y
    rank = got.rank.cpu().numpy()
    assert clear.sum() >= keep.sum() // 2
    assert ((rank == 0) == lead)[clear].all()                    # rank == 0 wherever the oracle's best word clearly leads
    assert (got.top.cpu().numpy()[..., 0] == lp.argmax(-1))[clear].all()
    assert (rank[~keep] == -1).all() and (got.entropy.cpu().numpy()[~keep] == 0).all()
    # translation_confidence: beamsearch_nbest's hypotheses, then their confidence
    nb_args = (src, lens) + ((im,) if meta["kind"] == "mm" else ())
    want_hyps, want_sc = m.beamsearch_nbest(*nb_args, beam_size=4, n_best=2, max_length=10)
    hyps, conf = confidence.translation_confidence(m, src, lens, im, beam_size=4, n_best=2, max_length=10)
    assert [[list(map(int, h)) for h in per] for per in hyps] == [[list(map(int, h)) for h in per] for per in want_hyps]
    assert conf.score.shape == (2 * src.shape[0],) and not m.training


def test_ensemble_confidence_of_two_seeds():
    from vagnmt_hip import confidence
    from vagnmt_hip.ensemble import Ensemble
    m, meta, src, im, tgt = _golden_batch("mm_dot_tied_s0_f32")
    Vs, Vt, I, E, H, S = meta["dims"][:6]
    m2 = make_model("mm", Vs, Vt, E, H, seed=5, I=I, S=S)
    m2.train()
    ens = Ensemble([m, m2])
    got = ens.token_confidence(src, meta["lengths"], tgt, im)
    sc = ens.score_translations(src, meta["lengths"], tgt, im)
    assert m2.training and not m.training
    assert torch.equal(got.score, sc.score) and torch.equal(got.logp, sc.logp) and torch.equal(got.token_logp, sc.token_logp)
    one = m.token_confidence(src, meta["lengths"], tgt, im)
    assert not torch.equal(one.entropy, got.entropy)
    same = Ensemble([m, m]).token_confidence(src, meta["lengths"], tgt, im)
    for a, b in zip(same, one):
        assert torch.equal(a, b)
    hyps, conf = confidence.translation_confidence(ens, src, meta["lengths"], im, beam_size=3, n_best=1, max_length=10)
    want, _ = ens.beamsearch_nbest(src, meta["lengths"], im, beam_size=3, n_best=1, max_length=10)
    assert [[list(map(int, h)) for h in per] for per in hyps] == [[list(map(int, h)) for h in per] for per in want]
    ece, bc, ba, n = confidence.calibration(got, bins=5)
    assert float(n.sum()) == float((got.rank >= 0).sum()) and 0.0 <= float(ece) <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# 6. Monte-Carlo dropout
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_mc_dropout(name):
    import random
    from vagnmt_hip import confidence
    m, meta, src, im, tgt = _golden_batch(name)
    lens = meta["lengths"]
    # the fixture builds every dropout at 0: every pass is the inference pass
    plain = m.token_confidence(*_args(meta, src, lens, tgt, im))
    mc = confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=3, seed=11)
    assert mc.token_logp.shape == (3,) + tuple(tgt.shape) and mc.score.shape == (3, tgt.shape[0])
    for i in range(3):
        assert torch.equal(mc.token_logp[i], plain.token_logp) and torch.equal(mc.score[i], plain.score)
    assert not m.training and getattr(m, "_vag_rng", None) is None
    # the reference's training rates
    m.encoder.dropout_emb, m.encoder.dropout_ctx, m.decoder.dropout_out = 0.3, 0.5, 0.5
    rng = torch.tensor([5, 17], dtype=torch.int64, device=DEV)
    m._vag_rng = rng
    state = random.getstate()
    a = confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=4, seed=11)
    b = confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=4, seed=11)
    assert torch.equal(a.token_logp, b.token_logp) and torch.equal(a.score, b.score)           # the same seed: the same bits
    for i in (0, 2, 3):                                          # pass i of an N-pass call: a 1-pass call started at step i
        one = confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=1, seed=11, step=i)
        assert torch.equal(one.token_logp[0], a.token_logp[i]) and torch.equal(one.score[0], a.score[i])
    assert not torch.equal(a.token_logp[0], a.token_logp[1])     # two passes differ
    other = confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=1, seed=12)
    assert not torch.equal(other.token_logp[0], a.token_logp[0])
    assert bool((a.var_score > 0).all())
    assert torch.equal(a.mean_score, a.score.mean(0)) and torch.equal(a.combo, 1.0 - a.mean_score / a.var_score)
    assert not m.training and m._vag_rng is rng and rng.tolist() == [5, 17] and random.getstate() == state
    m.train()
    confidence.mc_dropout_confidence(m, src, lens, tgt, im, passes=1)
    assert m.training


# ------------------------------------------------------------------------------------------------------------------
# 7. corpus perplexity
# ------------------------------------------------------------------------------------------------------------------
def test_corpus_perplexity_over_two_batches():
    from vagnmt_hip import confidence
    m, meta, src, im, tgt = _golden_batch("mm_dot_tied_s0_f32")
    lens = meta["lengths"]
    tgt2 = torch.from_numpy(load_golden("mm_dot_tied_s0_f32")[2]["tgt"]).cuda()
    got = confidence.corpus_perplexity(m, [(src, lens, tgt, im), (src, lens, tgt2, im)])
    logp = n = 0.0
    for t in (tgt, tgt2):
        logp += float(m.score_translations(src, lens, t, im).logp.double().sum())
        n += float(span_mask(t).sum())
    assert got.n_tokens == int(n) and abs(got.logp - logp) <= 1e-12 * abs(logp)
    assert abs(got.ppl - np.exp(-logp / n)) <= 1e-12 * got.ppl and got.ppl > 1.0


def test_corpus_perplexity_inside_averaged_weights():
    from test_gpu_ema import _fixture, _six_steps
    from vagnmt_hip import confidence
    meta, P, cm, cv, batch = _fixture("text_tied_s0_f32")
    m, ts, _ = _six_steps(meta, P, cm, cv, batch, True, 0.9, lr=1e-2, check=False)
    src, lens, tgt, im = batch
    raw = confidence.corpus_perplexity(ts, [(src, lens, tgt)])
    with ts.averaged_weights():
        avg = confidence.corpus_perplexity(ts, [(src, lens, tgt)])
    again = confidence.corpus_perplexity(m, [(src, lens, tgt)])
    assert np.isfinite(avg.ppl) and avg.n_tokens == raw.n_tokens and avg.ppl != raw.ppl
    assert again.n_tokens == raw.n_tokens and abs(again.ppl - raw.ppl) <= 1e-5 * raw.ppl          # the raw weights are back
