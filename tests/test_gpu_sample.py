"""GPU: the sampling decoder (vag_sample_step*, vagnmt_hip.search.sample, sample_decode on the models and the Ensemble).

1. exact selection, M = 1: the kernel's token against argmax(s * inv_T + g) in fp32 over the top-k set, g fetched with
   vag_sample_noise; token_logp bitwise; the EOS rule; the step-0 fan-out;
2. exact selection, M = 3 distinct members against a float64 restatement, on rows whose margin between the best and the
   second-best perturbed value is >= 1e-3 (at most 1 % of the rows may be left out); M identical members are check 1 bit for bit;
3. the noise is Gumbel: Pearson's chi-square of 65 536 draws against softmax(s / T) over the candidate set, below the
   1 - 1e-6 quantile (deterministic: a fixed seed);
4. top_k = 1 is greedy: Ensemble([m]).beamsearch_decode(beam_size=1)'s token lists, in eager and in graph mode, at any temperature;
5. samples score as themselves: score_translations of the drawn words against the returned token_logp / logp / score, within
   the bound test_gpu_nbest_score.py uses between the step kernels and the teacher-forced kernels (1e-4 absolute per token,
   2e-4 relative on sums); a drawn padding word 0, which forced decoding feeds on but does not score, is taken out of the sums;
6. determinism: generator states, seeds, cache hits and graph replays;
7. existing decode paths are untouched by sampling calls."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

EOS = 3
TEMPS = [0.5, 1.0, 1.5]
TOPKS = [0, 1, 10, 64]
SHAPES = [(4096, 1000), (2048, 8000)]


# ------------------------------------------------------------------------------------------------------------------
# the kernel on synthetic rows
# ------------------------------------------------------------------------------------------------------------------
def _pp(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def synth_rows(N, V, seed, M=1):
    """M matrices of log_softmax(normal(0, 3)) rows, leading dimension padded to a multiple of 4 (the pad holds +1e9: a kernel
    that read it would pick it)."""
    g = torch.Generator().manual_seed(seed)
    ldl = (V + 3) // 4 * 4 + 4
    xs = []
    for _ in range(M):
        x = torch.full((N, ldl), 1e9)
        x[:, :V] = torch.log_softmax(torch.randn(N, V, generator=g) * 3.0, dim=1)
        xs.append(x.cuda())
    return xs


def rng_words(seed, counter=0):
    return torch.tensor([seed, counter], dtype=torch.int64, device="cuda")


def run_step(xs, prev, T, k, rng, V, n=1, hs=None):
    """One launch at step 1 (prev (N,) = the previous words) or, with prev None, at step 0 (N_in = B rows fan out to B n).
    Returns (tok, token_logp, tok_out, n_alive[, h_out])."""
    from vagnmt_hip._lib import call, ptr, stream
    M = len(xs)
    B = xs[0].shape[0] if prev is None else xs[0].shape[0] // n
    N = B * n
    di = 0 if prev is None else 1
    toks = torch.zeros(2, N, dtype=torch.int64, device="cuda")
    lps = torch.full((2, N), 7.0, device="cuda")
    if prev is not None:
        toks[0] = prev
    tok_out = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    alive = torch.zeros(3, dtype=torch.int32, device="cuda")
    ldl = (C.c_int64 * M)(*[x.shape[1] for x in xs])
    h_out = None
    if di == 0:
        hs = hs if hs is not None else [torch.zeros(B, 4, device="cuda") for _ in xs]
        h_out = [torch.full((N, h.shape[1]), -5.0, device="cuda") for h in hs]
        hargs = (_pp(hs), _pp(h_out), (C.c_int64 * M)(*[h.shape[1] for h in hs]))
    else:
        hargs = (None, None, None)
    call("vag_sample_step", _pp(xs), ldl, M, ptr(toks, torch.int64), ptr(lps), di, 2, *hargs, ptr(tok_out, torch.int64), B, n, V,
         float(T), k, ptr(rng, torch.int64), ptr(alive, torch.int32), stream())
    torch.cuda.synchronize()
    assert int(alive[1]) == 0 and int(alive[2]) == 0                            # the kernel's own words are left zero
    assert float(lps[1 - di].min()) == 7.0 and float(lps[1 - di].max()) == 7.0        # only row di of the history is written
    return toks[di].clone(), lps[di].clone(), tok_out, int(alive[0]), h_out


def noise(rng, di, N, V):
    from vagnmt_hip._lib import call, ptr, stream
    out = torch.empty(N, V, device="cuda")
    call("vag_sample_noise", ptr(rng, torch.int64), di, N, V, ptr(out), stream())
    return out


def restate_fp32(s, g, T, k):
    """argmax_w (s * inv_T + g) over the top-k set under (value desc, index asc), two separately rounded fp32 operations, ties
    to the lowest word.  s, g (N, V) fp32 on the device.  Returns (tok (N,), candidate words (N, k') sorted best first)."""
    N, V = s.shape
    inv_T = float(np.float32(1.0) / np.float32(T))
    if k == 0:
        cand = torch.arange(V, device=s.device).expand(N, V)
    else:
        cand = torch.sort(s, dim=1, descending=True, stable=True)[1][:, :k]     # stable: equal values keep index order
    p = s.gather(1, cand) * inv_T
    p = p + g.gather(1, cand)
    best = p.max(1, keepdim=True)[0]
    tok = torch.where(p == best, cand, torch.full_like(cand, V)).min(1)[0]
    return tok, cand


@pytest.mark.parametrize("N,V", SHAPES)
def test_exact_selection_single(N, V):
    xs = synth_rows(N, V, 11)
    s = xs[0][:, :V].contiguous()
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    ended = torch.arange(0, N, 97, device="cuda")
    prev[ended] = EOS
    live = prev != EOS
    rng = rng_words(20261017, 3)
    g = noise(rng, 1, N, V)
    assert torch.isfinite(g).all() and float(g.min()) > -3.0 and float(g.max()) < 17.0      # u in [2^-24, 1 - 2^-24]
    assert not torch.equal(g, noise(rng_words(20261017, 4), 1, N, V)) and not torch.equal(g, noise(rng, 0, N, V))
    seen = set()
    for T in TEMPS:
        for k in TOPKS:
            tok, lp, tok_out, alive, _ = run_step(xs, prev, T, k, rng, V)
            want, cand = restate_fp32(s, g, T, k)
            assert torch.equal(tok_out, tok)
            assert bool((tok[~live] == EOS).all()) and float(lp[~live].abs().max()) == 0.0, (T, k)       # finished rows
            bad = int((tok[live] != want[live]).sum())
            assert bad == 0, (N, V, T, k, bad)
            assert bool((cand[live] == tok[live, None]).any(1).all()), (T, k)    # never outside the top-k set
            got_bits = lp[live].view(torch.int32)
            want_bits = s[live].gather(1, tok[live, None])[:, 0].view(torch.int32)
            assert torch.equal(got_bits, want_bits), (T, k)                      # token_logp = s[n, tok], bitwise
            assert alive == int((tok != EOS).sum()), (T, k)
            if k == 1:
                assert torch.equal(tok[live], s.argmax(1)[live])
            seen.add((T, k, int(tok[live].sum())))
    assert len(set(x[2] for x in seen if x[1] == 0)) == len(TEMPS)              # the temperature matters


def test_step0_fans_out_and_replicates_states():
    B, n, V = 8, 4, 333
    xs = synth_rows(B, V, 5, M=2)
    hs = [torch.randn(B, 12).cuda(), torch.randn(B, 7).cuda()]
    rng = rng_words(99)
    tok, lp, tok_out, alive, h_out = run_step(xs, None, 1.0, 0, rng, V, n=n, hs=hs)
    for h, ho in zip(hs, h_out):
        assert torch.equal(ho, h.repeat_interleave(n, 0))
    # output row r draws from input row r // n under its own key
    from_rows = [x[:, :V].repeat_interleave(n, 0).contiguous() for x in xs]
    s = ens_score_fp64([f.cpu().double() for f in from_rows])
    g = noise(rng, 0, B * n, V).cpu().double()
    p = s + g
    top2 = p.topk(2, dim=1)[0]
    ok = (top2[:, 0] - top2[:, 1]) >= 1e-3
    assert int(ok.sum()) >= B * n - 2
    assert torch.equal(tok.cpu()[ok], p.argmax(1)[ok])
    assert len(set(tok.cpu().tolist())) > B                                      # samples of one source row differ
    assert torch.equal(tok_out, tok) and alive == int((tok != EOS).sum())
    assert float((lp.cpu().double() - s.gather(1, tok.cpu()[:, None])[:, 0]).abs().max()) < 1e-5


def ens_score_fp64(xs):
    """s = mx + log(sum_m exp(x_m - mx) / M) in float64 (include/vag_nmt.h, vag_beam_ens_step)."""
    x = torch.stack(xs, 0)
    mx = x.max(0)[0]
    return mx + torch.log(torch.exp(x - mx).sum(0) / len(xs))


@pytest.mark.parametrize("N,V", SHAPES)
def test_exact_selection_ensemble(N, V):
    xs = synth_rows(N, V, 23, M=3)
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    rng = rng_words(77, 1)
    g32 = noise(rng, 1, N, V)
    g = g32.cpu().double()
    s = ens_score_fp64([x[:, :V].cpu().double() for x in xs])
    order = torch.sort(s, dim=1, descending=True, stable=True)[1]
    for T in TEMPS:
        inv_T = float(np.float32(1.0) / np.float32(T))
        for k in TOPKS:
            tok, lp, _, _, _ = run_step(xs, prev, T, k, rng, V)
            cand = order[:, :k] if k else torch.arange(V).expand(N, V)
            p = s.gather(1, cand) * inv_T + g.gather(1, cand)
            if k == 1:
                ok = torch.ones(N, dtype=torch.bool)
            else:
                top2 = p.topk(2, dim=1)[0]
                ok = (top2[:, 0] - top2[:, 1]) >= 1e-3
            want = cand.gather(1, p.argmax(1, keepdim=True))[:, 0]
            left_out = 1.0 - float(ok.float().mean())
            print("M=3 N=%d V=%d T=%.1f top_k=%d: %.3f %% of the rows left out" % (N, V, T, k, 100 * left_out))
            assert left_out <= 0.01, (T, k, left_out)
            tok_c = tok.cpu()
            if k == 1:      # the winner of an exact tie on s in fp64 may differ in fp32: compare scores there, words elsewhere
                same = tok_c == want
                gap = (s.gather(1, tok_c[:, None]) - s.gather(1, want[:, None]))[:, 0].abs()
                assert bool((same | (gap < 1e-5)).all()), (T, k)
            else:
                assert torch.equal(tok_c[ok], want[ok]), (N, V, T, k, int((tok_c[ok] != want[ok]).sum()))
            assert float((lp.cpu().double() - s.gather(1, tok_c[:, None])[:, 0]).abs().max()) < 1e-5, (T, k)
    # M identical members: the single member's draw, bit for bit
    for T, k in [(0.5, 0), (1.0, 10), (1.5, 64), (1.0, 1)]:
        one = run_step(xs[:1], prev, T, k, rng, V)
        three = run_step([xs[0], xs[0].clone(), xs[0].clone()], prev, T, k, rng, V)
        assert torch.equal(one[0], three[0]) and torch.equal(one[1].view(torch.int32), three[1].view(torch.int32)), (T, k)


# ------------------------------------------------------------------------------------------------------------------
# 3. the noise is Gumbel
# ------------------------------------------------------------------------------------------------------------------
def chi2_quantile(df, z=4.753424308822899):
    """The 1 - 1e-6 quantile of chi2(df): scipy if importable, else Wilson-Hilferty (z = the normal's 1 - 1e-6 quantile)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.mark.parametrize("T,k", [(1.0, 0), (0.7, 0), (1.3, 16)])
def test_draws_follow_the_tempered_distribution(T, k):
    N, V = 65536, 64
    g = torch.Generator().manual_seed(4)
    row = torch.log_softmax(torch.randn(V, generator=g) * 1.5, dim=0)
    x = row.expand(N, V).contiguous().cuda()
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    tok, _, _, _, _ = run_step([x], prev, T, k, rng_words(31337), V)
    counts = np.bincount(tok.cpu().numpy(), minlength=V).astype(np.float64)
    s = row.double().numpy()
    cand = np.argsort(-s, kind="stable")[:k] if k else np.arange(V)
    assert counts.sum() == N and counts[np.setdiff1d(np.arange(V), cand)].sum() == 0
    inv_T = float(np.float32(1.0) / np.float32(T))
    p = np.exp(s[cand] * inv_T - np.max(s[cand] * inv_T))
    expect = N * p / p.sum()
    obs = counts[cand]
    small = expect < 5.0
    if small.any():                                                             # cells with an expected count below 5: one pooled cell
        expect = np.append(expect[~small], expect[small].sum())
        obs = np.append(obs[~small], obs[small].sum())
    stat = float(((obs - expect) ** 2 / expect).sum())
    df = len(expect) - 1
    bound = chi2_quantile(df)
    print("T=%.1f top_k=%d: chi-square %.1f, df %d, bound %.1f" % (T, k, stat, df, bound))
    assert stat < bound, (T, k, stat, df, bound)
    # the check has power: the same counts against a temperature 10 % off
    p2 = np.exp(s[cand] * inv_T / 1.1 - np.max(s[cand] * inv_T / 1.1))
    e2 = N * p2 / p2.sum()
    assert float(((counts[cand] - e2) ** 2 / e2).sum()) > 3 * bound


# ------------------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------------------
def golden_model(name, eos_bias=0.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    meta, P, z = load_golden(name)
    Vs, Vt, I, E, H, S, B, Ts, Tt = meta["dims"]
    if meta["kind"] == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, meta["loss_w"], attn_model=meta["attn"],
                                                  tied_emb=meta["tied"], init_split=meta["init_split"])
    else:
        m = NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, tied_emb=meta["tied"])
    m.load_state_dict(P, strict=False)
    with torch.no_grad():
        m.decoder.out.bias[EOS] += eos_bias
    m = m.cuda().eval()
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
    return m, src, meta["lengths"], im


def ints(h):
    return [[int(t) for t in r] for r in h]


FIXTURES = ["text_tied_s0_f32", "mm_dot_tied_s0_f32"]


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("name", FIXTURES)
def test_top_k_one_is_greedy(name, graph):
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Generator
    m, src, lens, im = golden_model(name)
    m.decode_graph = graph
    ens = Ensemble([m])
    ens.decode_graph = graph
    for ML in (12, 5):
        want = ints(ens.beamsearch_decode(src, lens, im, beam_size=1, max_length=ML))
        for T in (0.5, 1.0, 2.0):
            got = m.sample_decode(src, lens, im, n_samples=1, max_length=ML, temperature=T, top_k=1, generator=Generator(int(T * 10)))
            assert [h[0] for h in got.hyps] == want, (name, graph, ML, T)
            got = ens.sample_decode(src, lens, im, n_samples=1, max_length=ML, temperature=T, top_k=1)
            assert [h[0] for h in got.hyps] == want, (name, graph, ML, T, "ensemble")


def _score(obj, src, lens, im, tgt, text):
    return obj.score_translations(src, lens, tgt) if text else obj.score_translations(src, lens, tgt, im)


def check_scores_as_themselves(obj, src, lens, im, text, ML, n, k, what):
    from vagnmt_hip.sampling import Generator
    out = obj.sample_decode(src, lens, im, n_samples=n, max_length=ML, temperature=1.0, top_k=k, generator=Generator(5))
    B = src.shape[0]
    assert len(out.hyps) == B and all(len(h) == n for h in out.hyps)
    assert out.token_logp.shape == (B, n, ML) and out.logp.shape == (B, n) and out.score.shape == (B, n)
    flat = [list(out.hyps[b][j]) for b in range(B) for j in range(n)]
    # the words as drawn: EOS closes a sample that ended inside max_length, none is appended to one that did not
    Tt = max(len(r) + (len(r) < ML) for r in flat)
    tgt = torch.zeros(B * n, Tt, dtype=torch.int64)
    for i, r in enumerate(flat):
        r = r + [EOS] if len(r) < ML else r
        tgt[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    src_n = src.repeat_interleave(n, 0)
    im_n = im.repeat_interleave(n, 0) if im is not None else None
    lens_n = [L for L in lens for _ in range(n)]
    forced = _score(obj, src_n, lens_n, im_n, tgt.cuda(), text)
    tl = out.token_logp.reshape(B * n, ML)
    assert float(tl[:, Tt:].abs().sum()) == 0.0
    # A draw from the whole vocabulary can be the padding word 0 (a candidate like any other: check 1).  score_translations
    # does not score a padding position by its contract (token_logp 0 there, include/vag_nmt.h: vag_forced_score), but it does
    # feed the word to the next step.  So every other position is compared as it is, and the sums are compared after taking the
    # drawn padding words' own log-probabilities out of the sampler's sum; the word count (> 3) is not affected.
    tgt_d = tgt.cuda()
    scored = tgt_d != 0
    drawn_pad = int(((tl[:, :Tt] != 0) & ~scored).sum())
    assert float((forced.token_logp * ~scored).abs().sum()) == 0.0
    err_tok = float(((tl[:, :Tt] - forced.token_logp).abs() * scored).max())
    words = (tgt_d > 3).sum(1).clamp(min=1).float()
    own_lp = out.logp.reshape(-1) - (tl[:, :Tt] * ~scored).sum(1)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
    assert rel(out.score.reshape(-1), out.logp.reshape(-1) / words) <= 1e-6
    err_lp, err_sc = rel(own_lp, forced.logp), rel(own_lp / words, forced.score)
    ended = sum(len(r) < ML for r in flat)
    print("%s: %d samples, %d ended inside max_length, %d drawn padding words; per-token max abs err %.3e, logp rel err %.3e, "
          "score rel err %.3e" % (what, len(flat), ended, drawn_pad, err_tok, err_lp, err_sc))
    assert err_tok <= 1e-4, (what, err_tok)
    assert err_lp <= 2e-4 and err_sc <= 2e-4, (what, err_lp, err_sc)
    if k:                                                                        # no word outside what a top-k draw can give
        assert float(out.token_logp.min()) > -30.0
    return out, ended


@pytest.mark.parametrize("graph", [True, False])
def test_samples_score_as_themselves(graph):
    from vagnmt_hip.ensemble import Ensemble
    ML, n = 12, 4
    ended = 0
    models = {}
    for name in FIXTURES:
        m, src, lens, im = golden_model(name, eos_bias=2.0)
        m.decode_graph = graph
        models[name] = (m, src, lens, im)
        for k in (0, 10):
            ended += check_scores_as_themselves(m, src, lens, im, im is None, ML, n, k, "%s graph=%s top_k=%d" % (name, graph, k))[1]
    t, (mm, src, lens, im) = models[FIXTURES[0]][0], models[FIXTURES[1]]
    ens = Ensemble([mm, t])
    ens.decode_graph = graph
    for k in (0, 10):
        ended += check_scores_as_themselves(ens, src, lens, im, False, ML, n, k, "Ensemble of 2 graph=%s top_k=%d" % (graph, k))[1]
    assert ended > 0                                                             # the EOS rule was exercised


def same(a, b):
    return a.hyps == b.hyps and torch.equal(a.token_logp, b.token_logp) and torch.equal(a.logp, b.logp) and \
        torch.equal(a.score, b.score)


@pytest.mark.parametrize("graph", [True, False])
def test_determinism(graph):
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Generator
    m, src, lens, im = golden_model(FIXTURES[1], eos_bias=1.0)
    t = golden_model(FIXTURES[0], eos_bias=1.0)[0]
    for obj in (m, Ensemble([m, t])):
        obj.decode_graph = graph
        kw = dict(n_samples=3, max_length=10, temperature=0.9, top_k=0)
        gen = Generator(123)
        st = gen.get_state()
        a = obj.sample_decode(src, lens, im, generator=gen, **kw)
        assert gen.get_state() == [st[0], st[1] + 1]                             # advanced once per call
        b = obj.sample_decode(src, lens, im, generator=gen, **kw)
        assert not same(a, b)                                                    # consecutive calls differ
        gen.set_state(st)
        assert same(a, obj.sample_decode(src, lens, im, generator=gen, **kw))    # the same state: the same samples
        assert same(b, obj.sample_decode(src, lens, im, generator=gen, **kw))
        assert same(a, obj.sample_decode(src, lens, im, generator=Generator(123), **kw))
        assert not same(a, obj.sample_decode(src, lens, im, generator=Generator(124), **kw))       # different seeds differ
        # another decode shape, other by-value arguments, then back: a cache hit (graph mode: a replay) gives the same samples
        other = obj.sample_decode(src[:3], lens[:3], im[:3], generator=Generator(123), **kw)
        assert len(other.hyps) == 3
        obj.sample_decode(src, lens, im, generator=Generator(123), n_samples=2, max_length=10, temperature=0.9, top_k=0)
        c = obj.sample_decode(src, lens, im, generator=Generator(123), n_samples=3, max_length=10, temperature=0.6, top_k=5)
        assert not same(a, c)
        assert same(a, obj.sample_decode(src, lens, im, generator=Generator(123), **kw))
        assert same(c, obj.sample_decode(src, lens, im, generator=Generator(123), n_samples=3, max_length=10, temperature=0.6,
                                         top_k=5))
        # the default generator: one per object, advancing
        d1 = obj.sample_decode(src, lens, im, **kw)
        d2 = obj.sample_decode(src, lens, im, **kw)
        assert not same(d1, d2)


def test_existing_decode_paths_are_untouched():
    from vagnmt_hip.ensemble import Ensemble
    for name in FIXTURES:
        m, src, lens, im = golden_model(name)
        text = im is None
        args = (src, lens) if text else (src, lens, im)
        ens = Ensemble([m])

        def snapshot():
            out = []
            for graph in (True, False):
                m.decode_graph = ens.decode_graph = graph
                hyps, sc = m.beamsearch_nbest(*args, beam_size=3, n_best=2, max_length=9)
                out.append((ints(m.beamsearch_decode(*args, beam_size=3, max_length=9)),
                            m.last_beam_scores.cpu().numpy().copy(), ints(m.beamsearch_decode(*args, beam_size=1, max_length=9)),
                            hyps, sc.cpu().numpy().copy(), ints(ens.beamsearch_decode(src, lens, im, beam_size=3, max_length=9))))
            return out

        before = snapshot()
        for graph in (True, False):
            m.decode_graph = ens.decode_graph = graph
            for k in (0, 3):
                m.sample_decode(src, lens, im, n_samples=3, max_length=9, temperature=0.8, top_k=k)
                ens.sample_decode(src, lens, im, n_samples=3, max_length=9, temperature=0.8, top_k=k)
        after = snapshot()
        for x, y in zip(before, after):
            assert x[0] == y[0] and x[2] == y[2] and x[3] == y[3] and x[5] == y[5], name
            assert np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) and np.array_equal(x[4].view(np.int32), y[4].view(np.int32))
