"""GPU: shallow fusion with an n-gram language model (vagnmt_hip.lm; include/vag_nmt.h: vag_lm_fuse_rows, vag_lm_fuse_beam(_dev),
vag_lm_query).

1. the kernels through the ABI by hand against tests/lm_ref.py: the dense form on the case table (every element within eps of
   float64, poison kept, two runs bitwise equal), the sparse form against the dense one bit for bit, the beam form on a hand-built
   search buffer against the dense form with the reference walk's contexts, the ABI's argument errors;
2. the models and Ensemble: beta = 0 is beamsearch_nbest, scores against lm_score_translations, token scores against the sum of
   the two models' own, graph against eager mode and stale graphs, steering, bans, lm_tune."""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_ref as R

pytestmark = pytest.mark.gpu

EOS = 3
I32, I64 = torch.int32, torch.int64


def L():
    from vagnmt_hip import _lib
    return _lib.lib()


def stream():
    from vagnmt_hip import _lib
    return _lib.stream()


def LM():
    from vagnmt_hip import lm
    return lm


def pp(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def bits(t):
    return t.detach().cpu().contiguous().view(I32)


_MODELS = {}


def device_model(V, order, seed=0):
    """(the reference's dict, the NgramLM built from it on the GPU), shared among the tests and left unchanged."""
    key = (V, order, seed)
    if key not in _MODELS:
        grams = R.case_model(V, order, seed)
        _MODELS[key] = (grams, LM().NgramLM.from_ngrams(order, V, *R.to_arrays(grams, order)).to("cuda"))
    return _MODELS[key]


def to_device(flat):
    """Per member the poisoned flat array on the device; member 1 starts 4 bytes off a 16-byte boundary."""
    out = []
    for m, a in enumerate(flat):
        if m == 1:
            t = torch.empty(a.shape[0] + 1, device="cuda")[1:]
            t.copy_(torch.from_numpy(a))
        else:
            t = torch.from_numpy(a).cuda()
        out.append(t)
    return out


def fuse_rows(m, rows, ld, Rr, ctx, beta):
    rc = L().vag_lm_fuse_rows(pp(rows), p64([ld] * len(rows)), len(rows), Rr, m.V, C.byref(m.struct()), ctx.data_ptr(), beta, stream())
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------------------ the dense form
@pytest.mark.parametrize("case", R.DENSE_CASES, ids=[c[0] for c in R.DENSE_CASES])
def test_dense_rows_match_float64_within_eps(case):
    name, V, ld, order, M, Rr = case
    grams, m = device_model(V, order)
    ctx = R.case_contexts(V, order, Rr, name)
    flat = R.case_rows(V, ld, M, Rr, 0)
    cd = torch.from_numpy(ctx).cuda()
    for beta in (0.3, -1.7):
        runs = []
        for _ in range(2):
            rows = to_device(flat)
            fuse_rows(m, rows, ld, Rr, cd, beta)
            torch.cuda.synchronize()
            runs.append([r.cpu().numpy() for r in rows])
        worst = 0.0
        for mi in range(M):
            got, again, src = runs[0][mi], runs[1][mi], flat[mi]
            assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs differ"
            assert np.array_equal(got[Rr * ld:].view(np.int32), src[Rr * ld:].view(np.int32)), "guard band written"
            g2, s2 = got[:Rr * ld].reshape(Rr, ld), src[:Rr * ld].reshape(Rr, ld)
            assert np.array_equal(g2[:, V:].view(np.int32), s2[:, V:].view(np.int32)), "columns [V, ld) written"
            for r in range(Rr):
                want, _, bound = R.fuse_row64(grams, V, order, s2[r, :V], ctx[r], beta)
                err = np.abs(g2[r, :V].astype(np.float64) - want)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (name, beta, mi, r, int(np.argmax(err / bound)), float((err / bound).max()))
        print("%s beta %.1f: worst error %.3f eps" % (name, beta, worst))


@pytest.mark.parametrize("case", [c for c in R.DENSE_CASES if c[5] == 7 and c[4] == 1], ids=lambda c: c[0])
def test_sparse_query_is_the_dense_increment_bit_for_bit(case):
    name, V, ld, order, M, Rr = case
    grams, m = device_model(V, order)
    ctx = R.case_contexts(V, order, Rr, name)
    cd = torch.from_numpy(ctx).cuda()
    rows = [torch.zeros(Rr, ld, device="cuda")]
    fuse_rows(m, rows, ld, Rr, cd, 1.0)
    pairs_ctx = cd[:, None, :].expand(Rr, V, order - 1).reshape(Rr * V, order - 1).contiguous()
    words = torch.arange(V, dtype=I32, device="cuda").repeat(Rr)
    logp, matched = m.query(pairs_ctx, words)
    torch.cuda.synchronize()
    assert torch.equal(bits(logp.view(Rr, V)), bits(rows[0][:, :V].contiguous()))
    assert bool((rows[0][:, V:] == 0).all())
    want = np.stack([R.fuse_row64(grams, V, order, np.zeros(V, dtype=np.float32), ctx[r], 1.0)[1] for r in range(Rr)])
    assert np.array_equal(matched.view(Rr, V).cpu().numpy(), want)
    # a word outside the vocabulary matches nothing
    lp, od = m.query(cd[:2].contiguous(), torch.tensor([-1, V], dtype=I32, device="cuda"))
    assert od.tolist() == [0, 0] and bool(torch.isinf(lp).all())


# ------------------------------------------------------------------------------------------------------------- the beam form
@pytest.mark.parametrize("order", [2, 3, 5])
def test_beam_form_is_the_dense_form_on_the_walks_contexts(order):
    c = R.BEAM_CASE
    B, k, ml, V = c["B"], c["k"], c["max_len"], c["V"]
    grams, m = device_model(V, order)
    beam = R.beam_case()
    bd = torch.from_numpy(beam).cuda()
    ld, M, beta = 504, 2, 0.7
    g = torch.Generator().manual_seed(order)
    base = [(-14.0 * torch.rand(B * k, ld, generator=g)).cuda() for _ in range(M)]
    for di in c["steps"]:
        n = B if di == 0 else B * k
        ctx, done = R.beam_contexts(beam, di, B, k, ml, order, V)
        want = [b.clone() for b in base]
        fuse_rows(m, want, ld, n, torch.from_numpy(ctx).cuda(), beta)
        keep = torch.from_numpy(done).cuda()
        for w, b in zip(want, base):
            w[:n][keep] = b[:n][keep]                                         # rows after EOS stay as they were
        host = [b.clone() for b in base]
        rc = L().vag_lm_fuse_beam(pp(host), p64([ld] * M), M, bd.data_ptr(), di, ml, B, k, V, C.byref(m.struct()), beta, stream())
        assert rc == 0, rc
        dev = [b.clone() for b in base]
        di_state = torch.tensor([di], dtype=I32, device="cuda")
        rc = L().vag_lm_fuse_beam_dev(pp(dev), p64([ld] * M), M, bd.data_ptr(), di_state.data_ptr(), ml, B, k, V, C.byref(m.struct()),
                                      beta, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert int(di_state[0]) == di
        for w, h, d, b in zip(want, host, dev, base):
            assert torch.equal(bits(h), bits(w)), (order, di)
            assert torch.equal(bits(d), bits(h)), (order, di)
            assert not torch.equal(bits(h[:n][~keep]), bits(b[:n][~keep]))       # (and the live rows did change)
        if di >= 1:
            assert done.any()
    # the device form does nothing once the index has reached max_len
    dev = [b.clone() for b in base]
    di_state = torch.tensor([ml], dtype=I32, device="cuda")
    assert L().vag_lm_fuse_beam_dev(pp(dev), p64([ld] * M), M, bd.data_ptr(), di_state.data_ptr(), ml, B, k, V, C.byref(m.struct()), beta,
                                    stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(bits(d), bits(b)) for d, b in zip(dev, base))


def test_abi_errors_launch_nothing():
    from vagnmt_hip import _lib
    grams, m = device_model(37, 3)
    rows = [torch.zeros(2, 40, device="cuda")]
    ctx = torch.full((2, 2), -1, dtype=I32, device="cuda")
    beam = torch.zeros(20, 3, 6, dtype=I64, device="cuda")
    s = m.struct()

    def changed(**kw):
        t = _lib.Lm.from_buffer_copy(s)
        for k_, v in kw.items():
            setattr(t, k_, v)
        return C.byref(t)

    F, Bm = L().vag_lm_fuse_rows, L().vag_lm_fuse_beam
    ok = C.byref(s)
    assert F(pp(rows), p64([40]), 1, 2, 37, changed(order=6), ctx.data_ptr(), 0.5, stream()) == -22
    assert F(pp(rows), p64([40]), 1, 2, 36, ok, ctx.data_ptr(), 0.5, stream()) == -22
    assert F(pp(rows), p64([36]), 1, 2, 37, ok, ctx.data_ptr(), 0.5, stream()) == -22
    assert F(pp(rows), p64([40]), 9, 2, 37, ok, ctx.data_ptr(), 0.5, stream()) == -22
    assert F(pp(rows), p64([40]), 1, 2, 37, ok, None, 0.5, stream()) == -22
    assert F(pp(rows), p64([40]), 1, 2, 37, ok, ctx.data_ptr(), float("nan"), stream()) == -22
    assert F(pp([None]), p64([40]), 1, 2, 37, ok, ctx.data_ptr(), 0.5, stream()) == -22
    assert Bm(pp(rows), p64([40]), 1, beam.data_ptr(), 0, 10, 3, 65, 37, ok, 0.5, stream()) == -22
    assert Bm(pp(rows), p64([40]), 1, beam.data_ptr(), 0, 1025, 3, 6, 37, ok, 0.5, stream()) == -22
    assert Bm(pp(rows), p64([40]), 1, beam.data_ptr(), 10, 10, 3, 6, 37, ok, 0.5, stream()) == -22
    assert Bm(pp(rows), p64([40]), 1, None, 0, 10, 3, 6, 37, ok, 0.5, stream()) == -22
    assert L().vag_lm_fuse_beam_dev(pp(rows), p64([40]), 1, beam.data_ptr(), None, 10, 3, 6, 37, ok, 0.5, stream()) == -22
    out, od = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=I32, device="cuda")
    w = torch.zeros(2, dtype=I32, device="cuda")
    assert L().vag_lm_query(changed(V=38), ctx.data_ptr(), w.data_ptr(), 2, out.data_ptr(), od.data_ptr(), stream()) == -22
    assert L().vag_lm_query(ok, ctx.data_ptr(), w.data_ptr(), 0, out.data_ptr(), od.data_ptr(), stream()) == -22
    # beta = 0 is valid and writes nothing
    assert F(pp(rows), p64([40]), 1, 2, 37, ok, ctx.data_ptr(), 0.0, stream()) == 0
    torch.cuda.synchronize()
    assert bool((rows[0] == 0).all()) and bool((out == 0).all()) and bool((od == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# the models and Ensemble (the sizes of make_model in tests/test_gpu_knn.py)
# ------------------------------------------------------------------------------------------------------------------
VS, VT, IM, ML, H = 70, 503, 64, 10, 64
LENS = [9, 6, 3]
KB = 6
BETA = 0.4


def make_model(kind, seed, eos_bias=0.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    if kind == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(VS, VT, IM, 32, 32, H, 48, 0.99, attn_model="dot", tied_emb=True)
    else:
        m = NMT_Seq2Seq_Beam_V2(VS, VT, 32, 32, H, tied_emb=True)
    with torch.no_grad():
        m.decoder.out.bias[EOS] += eos_bias
    return m.cuda().eval()


def make_inputs(lens=LENS, seed=9):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        src[b, :n] = torch.randint(4, VS, (n,), generator=g)
    return src.cuda(), torch.randn(len(lens), IM, generator=g).abs().cuda()


def text(seed, n=40):
    """Monolingual text: n sentences of 3 .. 8 words over a small part of the vocabulary, no immediate repeat."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        row = [int(rng.integers(4, 60))]
        while len(row) < int(rng.integers(3, 9)):
            w = int(rng.integers(4, 60))
            if w != row[-1]:
                row.append(w)
        out.append(row)
    return out


_LMS = {}


def trained(seed):
    """(sentences, NgramLM of order 3, the brute-force dict of the same text)."""
    if seed not in _LMS:
        s = text(seed)
        _LMS[seed] = (s, LM().NgramLM.train(s, VT, 3).to("cuda"), R.kn_bruteforce(s, VT, 3))
    return _LMS[seed]


@pytest.fixture(scope="module", params=["mm", "text", "ens"])
def subject(request):
    """(kind, searcher, members, src, im): a multimodal model, a text-only one, an Ensemble of two multimodal ones; the models
    carry an EOS bias so that hypotheses end before max_length."""
    kind = request.param
    src, im = make_inputs()
    if kind == "ens":
        from vagnmt_hip.ensemble import Ensemble
        ms = [make_model("mm", 31, 5.0), make_model("mm", 32, 5.0)]
        return kind, Ensemble(ms), ms, src, im
    m = make_model(kind, 31, 5.0)
    return kind, m, [m], src, (im if kind == "mm" else None)


def is_text(s):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    return isinstance(s, NMT_Seq2Seq_Beam_V2)


def nbest(s, src, im, k=KB, n=KB, lens=LENS):
    return s.beamsearch_nbest(src, lens, k, n, ML) if is_text(s) else s.beamsearch_nbest(src, lens, im, k, n, ML)


def plain_scores(s, src, lens, tgt, im):
    return s.score_translations(src, lens, tgt) if is_text(s) else s.score_translations(src, lens, tgt, im)


def lm_search(s, src, im, lm, lens=LENS, **kw):
    kw.setdefault("beam_size", KB)
    kw.setdefault("n_best", KB)
    kw.setdefault("max_length", ML)
    kw.setdefault("beta", BETA)
    return s.beamsearch_lm(src, lens, im, lm, **kw)


def set_graph(s, members, on):
    s.decode_graph = on
    for m in members:
        m.decode_graph = on


def ints(hyps):
    return [[[int(t) for t in r] for r in h] for h in hyps]


def same(a, b):
    return ints(a.hyps) == ints(b.hyps) and torch.equal(bits(a.scores), bits(b.scores))


def test_beta_0_is_beamsearch_nbest_and_launches_nothing(subject, monkeypatch):
    lm_mod = LM()
    kind, s, members, src, im = subject
    _, lm, _ = trained(3)
    seen = []
    real = lm_mod.call
    monkeypatch.setattr(lm_mod, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    for graph in (True, False):
        set_graph(s, members, graph)
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(s, src, im, k, n)
            r = lm_search(s, src, im, lm, beam_size=k, n_best=n, beta=0.0)
            assert ints(r.hyps) == ints(hyps) and torch.equal(bits(r.scores), bits(sc)), (graph, k)
    assert not [x for x in seen if x.startswith("vag_lm")], seen
    r = lm_search(s, src, im, lm)
    assert any(x.startswith("vag_lm_fuse_beam") for x in seen) and not same(r, lm_search(s, src, im, lm, beta=0.0))
    set_graph(s, members, True)


def forced_pieces(members, src_n, lens_n, flat, im_n):
    """Per member the forced logits at the target words and the rows' log-sum-exp, (B, Tt) each, and the targets."""
    from vagnmt_hip import knn, scoring
    out = []
    with torch.no_grad():
        for m in members:
            mm = hasattr(m, "vse_imagine")
            tgt, tok = scoring.forced_args([m], [mm], src_n, flat, im_n if mm else None)
            logits, lse, _ = knn.member_forced(m, src_n, lens_n, im_n if mm else None, tok, tgt)
            B, Tt = tgt.shape
            x = logits.view(Tt, B, -1).gather(2, tgt.t()[:, :, None])[:, :, 0].t()
            out.append((x.cpu().numpy().astype(np.float64), lse.view(Tt, B).t().cpu().numpy().astype(np.float64)))
    return out, tgt.cpu().numpy()


def token_eps(pieces, tgt, ref, beta):
    """(B, Tt) bound on a fused token score, from lm_ref.eps: the fusion's own error with x the largest member logit at the word
    (the kernel adds to the raw logit), plus 8 u (|logit| + |lse| + |beta lm|) for what follows it on either path -- the
    subtraction of the log-sum-exp, the members' log-mean (exp, a sum of at most 8 terms, log; 2 ulp each for the device's exp
    and log), and the multiply-add of the path that sums the two models' own scores: at most 8 roundings of values no larger."""
    B, Tt = tgt.shape
    out = np.zeros((B, Tt))
    for b in range(B):
        hist = [R.SOS]
        for t in range(Tt):
            w = int(tgt[b, t])
            v, _, a, S = R.lm64(ref, w, R.clean_ctx(hist, VT, 3))
            x = max(abs(p[0][b, t]) for p in pieces)
            lse = max(abs(p[1][b, t]) for p in pieces)
            out[b, t] = R.eps(x, beta, a, S) + 8 * R.U * (x + lse + abs(beta * v))
            hist.append(w)
    return out


def flat_inputs(r, src, im):
    B = len(LENS)
    flat = [list(r.hyps[b][j]) for b in range(B) for j in range(KB)]
    return flat, src.repeat_interleave(KB, 0), [n for n in LENS for _ in range(KB)], im.repeat_interleave(KB, 0) if im is not None else None


def test_scores_are_the_forced_fused_scores(subject):
    """Every returned hypothesis that ended before max_length scores, forced under the fused score, what the search scored it.
    Tolerance: relative 2e-4 -- the bound tests/test_gpu_constrain.py and test_gpu_knn.py use for a search score against a
    forced score of the same model (the step and the whole-sequence kernels differ) -- plus the language model's margin: both
    paths hold every token's LM term within eps of the exact one, so two eps per token, and a length-normalised score is a
    mean of those."""
    kind, s, members, src, im = subject
    _, lm, ref = trained(3)
    r = lm_search(s, src, im, lm)
    sc = r.scores.cpu().numpy()
    B = len(LENS)
    idx = [(b, j) for b in range(B) for j in range(KB) if len(r.hyps[b][j]) < ML - 1]
    assert len(idx) >= 4, len(idx)
    flat, src_n, lens_n, im_n = flat_inputs(r, src, im)
    f = s.lm_score_translations(src_n, lens_n, flat, im_n, lm, BETA)
    fs = f.score.cpu().numpy().reshape(B, KB)
    pieces, tgt = forced_pieces(members, src_n, lens_n, flat, im_n)
    te = token_eps(pieces, tgt, ref, BETA)
    worst = 0.0
    for b, j in idx:
        n = len(r.hyps[b][j]) + 1
        margin = 2.0 * te[b * KB + j, :n].sum() / n
        worst = max(worst, (abs(float(fs[b, j]) - float(sc[b, j])) - margin) / max(1.0, abs(float(sc[b, j]))))
    print("%s: %d finished hypotheses, worst relative excess %.3e" % (kind, len(idx), worst))
    assert worst <= 2e-4, worst
    # the fused token scores are the two models' own, summed
    p = plain_scores(s, src_n, lens_n, flat, im_n)
    t = torch.from_numpy(tgt).cuda()
    want = p.token_logp.double() + BETA * lm.token_logp(t).double()
    err = (f.token_logp.double() - want).abs().cpu().numpy()
    live = p.token_logp.cpu().numpy() != 0
    assert live.any() and np.all(err[live] <= te[live]), float((err[live] / te[live]).max())
    assert bool((f.token_logp.cpu()[torch.from_numpy(~live)] == 0).all())
    # and beta = 0 of the scoring is score_translations bit for bit
    z = s.lm_score_translations(src_n, lens_n, flat, im_n, lm, 0.0)
    assert torch.equal(bits(z.score), bits(p.score)) and torch.equal(bits(z.token_logp), bits(p.token_logp))


def test_token_logp_and_perplexity_are_the_references():
    sents, lm, ref = trained(3)
    rows = sents[:6] + [[7, 499, 8], [R.UNK]]
    Tt = max(len(x) for x in rows) + 1
    tgt = torch.zeros(len(rows), Tt, dtype=I64)
    for b, x in enumerate(rows):
        tgt[b, :len(x)] = torch.tensor(x)
        tgt[b, len(x)] = EOS
    tgt[-1, 1] = 0                                                           # no EOS: scored to the last non-pad word
    got = lm.token_logp(tgt.cuda()).cpu().numpy()
    total, words = 0.0, 0
    for b in range(len(rows)):
        hist = [R.SOS]
        x = [int(w) for w in tgt[b]]
        end = x.index(EOS) if EOS in x else max(i for i, w in enumerate(x) if w != 0)
        for t in range(Tt):
            if t > end:
                assert got[b, t] == 0.0
                continue
            v, _, a, S = R.lm64(ref, x[t], R.clean_ctx(hist, VT, 3))
            assert abs(float(got[b, t]) - v) <= R.eps(0.0, 1.0, a, S), (b, t)
            total, words = total + v, words + 1
            hist.append(x[t])
    ppl = lm.perplexity([tgt[:4].cuda(), tgt[4:].cuda()])
    assert abs(ppl - np.exp(-total / words)) <= 1e-5 * ppl


def test_graph_equals_eager_and_no_stale_graph(subject):
    kind, s, members, src, im = subject
    _, lm, _ = trained(3)
    _, other, _ = trained(5)
    runs = [(lm, 0.4), (lm, 0.9), (other, 0.4), (lm, 0.4)]
    set_graph(s, members, False)
    eager = [lm_search(s, src, im, m, beta=b) for m, b in runs]
    set_graph(s, members, True)
    graph = [lm_search(s, src, im, m, beta=b) for m, b in runs]
    for e, g in zip(eager, graph):
        assert same(e, g)
    assert not same(eager[0], eager[1]) and not same(eager[0], eager[2])       # another beta, another model: other results
    assert same(eager[0], eager[3])
    # the constraints still win over the language model
    w = next(int(h[0]) for hs in eager[0].hyps for h in hs if len(h))
    for on in (False, True):
        set_graph(s, members, on)
        c = lm_search(s, src, im, lm, banned=[[w]])
        live = [(b, j) for b in range(len(LENS)) for j in range(KB) if float(c.scores[b, j]) > -1e4]
        assert live and all(w not in [int(t) for t in c.hyps[b][j]] for b, j in live)
    set_graph(s, members, True)


def test_a_strong_language_model_steers_the_search(subject):
    """The LM knows one sentence.  beta is chosen so that beta times the LM's smallest margin along that sentence exceeds the
    model's largest log-probability spread at those steps -- asserted from the forced rows -- and the best hypothesis of every
    source is that sentence."""
    from vagnmt_hip import knn, scoring
    kind, s, members, src, im = subject
    sent = [17, 230, 5, 499, 42]
    lm = LM().NgramLM.train([sent], VT, 3).to("cuda")
    full = sent + [EOS]
    margins, hist = [], [R.SOS]
    for w in full:
        lp = np.array([lm.logprob(v, hist)[0] for v in range(VT)])
        margins.append(lp[w] - np.delete(lp, w).max())
        hist.append(w)
    assert min(margins) > 0.0
    B = len(LENS)
    spread = 0.0
    with torch.no_grad():
        for m in members:
            mm = hasattr(m, "vse_imagine")
            tgt, tok = scoring.forced_args([m], [mm], src, [full] * B, im if mm else None)
            logits, lse, _ = knn.member_forced(m, src, LENS, im if mm else None, tok, tgt)
            rows = logits.view(len(full), B, -1)[:, :, :VT]
            spread = max(spread, float((rows.max(2)[0] - rows.min(2)[0]).max()))
    beta = 1.25 * spread / min(margins)
    assert beta * min(margins) > spread                                      # the premise
    for on in (False, True):
        set_graph(s, members, on)
        r = lm_search(s, src, im, lm, beta=beta, n_best=1)
        assert ints(r.hyps) == [[sent]] * B, (on, ints(r.hyps))
    set_graph(s, members, True)


def test_lm_tune_gives_one_bleu_per_beta(subject):
    from vagnmt_hip import validate
    kind, s, members, src, im = subject
    sents, lm, _ = trained(3)
    refs = [sents[0], sents[1], sents[2]]
    batches = [(src[:2, :].contiguous(), LENS[:2], refs[:2], im[:2].contiguous() if im is not None else None),
               (src[2:, :LENS[2]].contiguous(), LENS[2:], refs[2:], im[2:].contiguous() if im is not None else None)]
    betas = [0.0, 0.5]
    got = LM().lm_tune(s, lm, batches, betas, beam_size=KB, max_length=ML)
    assert len(got) == len(betas)
    hyps = []
    for a, b, _, d in batches:
        out = s.beamsearch_decode(a, b, KB, ML) if is_text(s) else s.beamsearch_decode(a, b, d, KB, ML)
        hyps += [[int(t) for t in h] for h in out]
    assert tuple(got[0]) == tuple(validate.corpus_bleu(hyps, refs))
