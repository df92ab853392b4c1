"""GPU: nucleus (top-p) sampling (vag_sample_step_p*, vagnmt_hip.search.sample(top_p=...), sample_decode(top_p=...) on the models
and the Ensemble).

The candidate pool P is the whole row (top_k = 0) or the exact top_k set under (s desc, word asc); with t = fl32(s * inv_T),
e = exp(t - max_P t), the nucleus is { w in P : s[w] >= s* }, s* the largest score whose words at or above it carry top_p of the
pool's mass.  The kernel reports the set's size r, which determines it (a prefix of the (s desc, word asc) order).

1. set and draw, M = 1: r against a float64 restatement of the masses -- r ends on a tie-group boundary, the mass of the first r
   words is >= top_p - d, the mass before r's last tie group is < top_p + d, with d = 2 |P| 2^-24 (the worst-case error of an
   fp32 sum of |P| non-negative terms of total <= 1 in any order, doubled for the rounding of expf), on every live row; r equals
   the float64 size exactly on rows where no cumulative mass lies within d of top_p.  The word is the arg-max of the fp32
   restatement over the first r words with the kernel's own noise; token_logp is s[tok] bitwise.  The sizes show that both small
   nuclei (<= 64 words) and large ones (hundreds, thousands of words) are exercised;
2. ties: rows with many exactly equal scores;
3. limits: top_p = 1 is vag_sample_step bit for bit with r = |P|; top_p = 1e-6 is the arg-max; an all-NaN row gives word 0,
   NaN and size 0 (top_k = 0; the top-k selection does not order NaNs);
4. M = 3 against ens_score in float64, on rows with a margin of 1e-3 between neighbours at the boundary and at the winner;
5. the draws follow softmax(s / T) renormalised over the nucleus (Pearson's chi-square, 65 536 draws);
6. the models and the Ensemble: graph and eager mode, determinism, cache hits, scores, sizes, and the other decode paths
   untouched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

EOS = 3
CASES = [(1.0, 0.9), (0.7, 0.5), (1.5, 0.95)]                                    # (temperature, top_p)
TOPKS = [0, 10, 64]


# ------------------------------------------------------------------------------------------------------------------
# the kernel on synthetic rows
# ------------------------------------------------------------------------------------------------------------------
def _pp(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def synth_rows(N, V, seed, M=1, step=None):
    """M matrices of log_softmax(normal(0, 3)) rows, leading dimension padded to a multiple of 4 (the pad holds +1e9: a kernel
    that read it would pick it).  step: the logits are rounded to multiples of it first (many exactly equal scores)."""
    g = torch.Generator().manual_seed(seed)
    ldl = (V + 3) // 4 * 4 + 4
    xs = []
    for _ in range(M):
        x = torch.full((N, ldl), 1e9)
        z = torch.randn(N, V, generator=g) * 3.0
        if step:
            z = torch.round(z / step) * step
        x[:, :V] = torch.log_softmax(z, dim=1)
        xs.append(x.cuda())
    return xs


def rng_words(seed, counter=0):
    return torch.tensor([seed, counter], dtype=torch.int64, device="cuda")


def noise(rng, di, N, V):
    from vagnmt_hip._lib import call, ptr, stream
    out = torch.empty(N, V, device="cuda")
    call("vag_sample_noise", ptr(rng, torch.int64), di, N, V, ptr(out), stream())
    return out


def run_step(xs, prev, T, k, rng, V, top_p=None):
    """One launch at step 1 (prev (N,) = the previous words): vag_sample_step, or vag_sample_step_p with top_p given.
    Returns (tok, token_logp, sizes or None); tok_out, n_alive, the kernel's own words and the untouched history row are
    checked here."""
    from vagnmt_hip._lib import call, ptr, stream
    M, N = len(xs), xs[0].shape[0]
    toks = torch.zeros(2, N, dtype=torch.int64, device="cuda")
    lps = torch.full((2, N), 7.0, device="cuda")
    sizes = torch.full((2, N), -7, dtype=torch.int32, device="cuda")
    toks[0] = prev
    tok_out = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    alive = torch.zeros(3, dtype=torch.int32, device="cuda")
    ldl = (C.c_int64 * M)(*[x.shape[1] for x in xs])
    head = (_pp(xs), ldl, M, ptr(toks, torch.int64), ptr(lps), 1, 2, None, None, None, ptr(tok_out, torch.int64), N, 1, V, float(T), k,
            ptr(rng, torch.int64), ptr(alive, torch.int32))
    if top_p is None:
        call("vag_sample_step", *head, stream())
    else:
        call("vag_sample_step_p", *head, float(top_p), ptr(sizes, torch.int32), stream())
    torch.cuda.synchronize()
    assert int(alive[1]) == 0 and int(alive[2]) == 0                            # the kernel's own words are left zero
    assert float(lps[0].min()) == 7.0 and float(lps[0].max()) == 7.0            # only row di of the history is written
    assert bool((toks[0] == prev).all()) and bool((sizes[0] == -7).all())
    assert torch.equal(tok_out, toks[1]) and int(alive[0]) == int((toks[1] != EOS).sum())
    if top_p is None:
        assert bool((sizes == -7).all())
        return toks[1].clone(), lps[1].clone(), None
    return toks[1].clone(), lps[1].clone(), sizes[1].clone().long()


def inv_temp(T):
    return float(np.float32(1.0) / np.float32(T))


def pool_masses(s, T, k):
    """The pool of every row of s (N, V; CPU, float32 or float64), best first under (s desc, word asc): (scores (N, |P|), words
    (N, |P|), c (N, |P|) float64: the cumulative mass of exp(t - max), t = s * inv_T rounded as s is, normalised)."""
    ss, order = torch.sort(s, dim=1, descending=True, stable=True)              # stable: equal values keep index order
    if k:
        ss, order = ss[:, :k], order[:, :k]
    t = (ss * inv_temp(T)).double()
    e = torch.exp(t - t.max(1, keepdim=True)[0])
    return ss, order, torch.cumsum(e, 1) / e.sum(1, keepdim=True)


def size_fp64(ss, c, top_p):
    """The nucleus' size by the float64 masses: the first word at which c reaches top_p, and every word that ties with it."""
    first = ((c >= top_p) | (torch.arange(c.shape[1]) == c.shape[1] - 1)).int().argmax(1)
    return (ss >= ss.gather(1, first[:, None])).sum(1)


def check_sizes(ss, c, r, top_p, rows, what, slack=0.0):
    """The checks of the kernel's sizes r (N,) on the rows `rows` (bool).  slack: added to d where ss and c come from scores
    that are not the kernel's bit for bit.  Returns (float64 sizes, rows that were compared exactly)."""
    P = ss.shape[1]
    d = 2.0 * P * 2.0 ** -24 + slack
    r = r.cpu()
    assert bool(((r >= 1) & (r <= P))[rows].all()), what
    rr = r.clamp(1, P)
    last = ss.gather(1, (rr - 1)[:, None])[:, 0]                                 # the score of the set's last word
    nxt = ss.gather(1, rr.clamp(max=P - 1)[:, None])[:, 0]
    assert bool(((rr == P) | (nxt < last))[rows].all()), what + ": a tie group is split"
    mass = c.gather(1, (rr - 1)[:, None])[:, 0]
    assert bool((mass >= top_p - d)[rows].all()), (what, float((mass - top_p)[rows].min()), d)
    g = (ss > last[:, None]).sum(1)                                              # where the set's last tie group begins
    before = torch.cat([torch.zeros(len(c), 1, dtype=c.dtype), c], 1).gather(1, g[:, None])[:, 0]
    assert bool((before < top_p + d)[rows].all()), (what, float((before - top_p)[rows].max()), d)
    want = size_fp64(ss, c, top_p)
    far = ((c - top_p).abs() > d).all(1) & rows
    assert torch.equal(r[far], want[far]), (what, int((r[far] != want[far]).sum()))
    return want, far


def draw_fp32(s, g, order, r, T):
    """argmax_w (s * inv_T + g) over the first r words of `order`, two separately rounded fp32 operations, ties to the lowest
    word.  s, g (N, V) fp32 on the device; order (N, |P|), r (N,)."""
    N, V = s.shape
    order, r = order.cuda(), r.cuda()
    inset = torch.zeros(N, V, dtype=torch.bool, device=s.device)
    inset.scatter_(1, order, torch.arange(order.shape[1], device=s.device)[None, :] < r[:, None])
    p = s * inv_temp(T)
    p = p + g
    p = torch.where(inset, p, torch.full_like(p, -float("inf")))
    best = p.max(1, keepdim=True)[0]
    words = torch.arange(V, device=s.device).expand(N, V)
    return torch.where(p == best, words, torch.full_like(words, V)).min(1)[0]


def check_single(xs, V, seed_words, what, seen=None):
    """Checks 1 and 2 on one matrix of rows: every (temperature, top_p) of CASES and every top_k of TOPKS."""
    N = xs[0].shape[0]
    s = xs[0][:, :V].contiguous()
    s_cpu = s.cpu()
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    prev[torch.arange(0, N, 9, device="cuda")] = EOS                            # some rows are finished
    live = prev != EOS
    live_c = live.cpu()
    rng = rng_words(*seed_words)
    g = noise(rng, 1, N, V)
    exact = 0
    for k in TOPKS:
        for T, top_p in CASES:
            w = "%s V=%d T=%.1f top_p=%.2f top_k=%d" % (what, V, T, top_p, k)
            ss, order, c = pool_masses(s_cpu, T, k)
            tok, lp, r = run_step(xs, prev, T, k, rng, V, top_p)
            assert bool((tok[~live] == EOS).all()) and float(lp[~live].abs().max()) == 0.0 and int(r[~live].abs().sum()) == 0, w
            want_r, far = check_sizes(ss, c, r, top_p, live_c, w)
            exact += int(far.sum())
            print("%s: sizes %d .. %d, %d of %d live rows compared exactly" % (w, int(r[live].min()), int(r[live].max()), int(far.sum()),
                                                                             int(live_c.sum())))
            want = draw_fp32(s, g, order, r, T)
            assert torch.equal(tok[live], want[live]), (w, int((tok[live] != want[live]).sum()))
            got_bits = lp[live].view(torch.int32)
            assert torch.equal(got_bits, s[live].gather(1, tok[live, None])[:, 0].view(torch.int32)), w     # s[n, tok], bitwise
            if seen is not None:
                seen[(T, top_p, k)] = (r[live].cpu(), far, int(live_c.sum()))
    return exact


@pytest.mark.parametrize("V", [333, 1000, 8000])
def test_set_and_draw_single(V):
    seen = {}
    check_single(synth_rows(64, V, 11), V, (20261018, 3), "M=1", seen)
    r, far, n_live = seen[(0.7, 0.5, 0)]
    assert int(r.min()) >= 1 and int(r.max()) <= 10                              # small nuclei: well inside 64 words
    if V in (333, 1000):
        assert int(far.sum()) == n_live                                          # no mass near top_p: every row compared exactly
    if V == 8000:                                                                # large nuclei: the search over the whole row
        r = seen[(1.0, 0.9, 0)][0]
        assert int(r.min()) > 64 and int(r.max()) < 1000
        r = seen[(1.5, 0.95, 0)][0]
        assert int(r.min()) > 2000 and int(r.max()) < 4000
    for T, top_p in CASES:                                                       # top_p cuts a top-k pool further
        assert int(seen[(T, top_p, 64)][0].max()) <= 64 and int(seen[(T, top_p, 10)][0].max()) <= 10
    assert int(seen[(0.7, 0.5, 64)][0].max()) < 64


def test_ties():
    V = 1000
    xs = synth_rows(64, V, 12, step=0.5)
    s = xs[0][:, :V].cpu()
    assert int(torch.unique(s[0]).numel()) < 60                                  # many exactly equal scores in a row
    seen = {}
    check_single(xs, V, (5, 1), "ties", seen)
    # the sets are whole tie groups: at the same top_p a tied row's set is larger than the position at which the mass is reached
    ss, _, c = pool_masses(s, 1.0, 0)
    first = (c >= 0.9).int().argmax(1) + 1
    r = size_fp64(ss, c, 0.9)
    assert bool((r >= first).all()) and int((r > first).sum()) > 32


def test_limits():
    N, V = 64, 1000
    xs = synth_rows(N, V, 13)
    xs[0][7, :V] = float("nan")                                                  # an all-NaN row
    s = xs[0][:, :V].contiguous()
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    prev[3] = EOS
    rows = torch.ones(N, dtype=torch.bool, device="cuda")
    rows[3] = rows[7] = False
    rng = rng_words(8, 2)
    for T in (0.7, 1.0):
        for k in (0, 1, 10, 64):
            # top_p = 1: the plain kernel bit for bit, the size is the pool's.  (The all-NaN row only at top_k = 0: the radix
            # selection does not order NaNs, what a top-k pool holds for such a row is not defined, here as in vag_sample_step.)
            cmp = rows.clone()
            cmp[3], cmp[7] = True, k == 0
            a = run_step(xs, prev, T, k, rng, V)
            b = run_step(xs, prev, T, k, rng, V, 1.0)
            assert torch.equal(a[0][cmp], b[0][cmp]) and torch.equal(a[1][cmp].view(torch.int32), b[1][cmp].view(torch.int32)), (T, k)
            assert bool((b[2][rows] == (k if k else V)).all()) and int(b[2][3]) == 0, (T, k)
            # top_p -> 0: the arg-max (unique in these rows), a set of one word
            tok, lp, r = run_step(xs, prev, T, k, rng, V, 1e-6)
            top2 = s[rows].topk(2, dim=1)[0]
            assert bool((top2[:, 0] > top2[:, 1]).all())
            assert torch.equal(tok[rows], s[rows].argmax(1)) and bool((r[rows] == 1).all()), (T, k)
            assert torch.equal(lp[rows].view(torch.int32), top2[:, 0].contiguous().view(torch.int32))
            for top_p in (1e-6, 0.9, 1.0):
                tok, lp, r = run_step(xs, prev, T, k, rng, V, top_p)
                assert int(tok[3]) == EOS and float(lp[3]) == 0.0 and int(r[3]) == 0, (T, k, top_p)          # the finished row
                if k == 0:                                                       # the all-NaN row: the padding word, NaN, no set
                    assert int(tok[7]) == 0 and math.isnan(float(lp[7])) and int(r[7]) == 0, (T, top_p)


# ------------------------------------------------------------------------------------------------------------------
# 4. the ensemble
# ------------------------------------------------------------------------------------------------------------------
def ens_score_fp64(xs):
    """s = mx + log(sum_m exp(x_m - mx) / M) in float64 (include/vag_nmt.h, vag_beam_ens_step)."""
    x = torch.stack(xs, 0)
    mx = x.max(0)[0]
    return mx + torch.log(torch.exp(x - mx).sum(0) / len(xs))


@pytest.mark.parametrize("V", [1000, 8000])
def test_set_and_draw_ensemble(V):
    N = 64
    xs = synth_rows(N, V, 23, M=3)
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    rng = rng_words(77, 1)
    g = noise(rng, 1, N, V).cpu().double()
    s = ens_score_fp64([x[:, :V].cpu().double() for x in xs])
    checked = total = 0
    for k in TOPKS:
        for T, top_p in CASES:
            w = "M=3 V=%d T=%.1f top_p=%.2f top_k=%d" % (V, T, top_p, k)
            ss, order, c = pool_masses(s, T, k)
            P = ss.shape[1]
            tok, lp, r = run_step(xs, prev, T, k, rng, V, top_p)
            tok, r = tok.cpu(), r.cpu()
            # The kernel's scores are ens_score in fp32, these are float64: they agree to 1e-5 (asserted below), so the order of
            # two words is only known where their scores differ by more.  Rows to compare: a margin of 1e-3 between the scores
            # on either side of the set's boundary (and of the pool's); for the word, 1e-3 between the two best perturbed values.
            # The masses move by the scores' error times inv_T: 1e-5 is added to d.
            pad = torch.cat([ss, torch.full((N, 1), -float("inf"), dtype=ss.dtype)], 1)
            rr = r.clamp(1, P)
            ok = (pad.gather(1, (rr - 1)[:, None]) - pad.gather(1, rr[:, None]))[:, 0] >= 1e-3
            if k:
                full = torch.sort(s, dim=1, descending=True, stable=True)[0]
                ok &= (full[:, k - 1] - full[:, k]) >= 1e-3
            _, far = check_sizes(ss, c, r, top_p, ok, w, slack=1e-5)
            inset = torch.arange(P)[None, :] < rr[:, None]
            p = torch.where(inset, ss * inv_temp(T) + g.gather(1, order), torch.full_like(ss, -float("inf")))
            top2 = p.topk(2, dim=1)[0]
            won = ok & ((top2[:, 0] - top2[:, 1]) >= 1e-3)
            want = order.gather(1, p.argmax(1, keepdim=True))[:, 0]
            checked, total = checked + int(won.sum()), total + N
            print("%s: sizes %d .. %d; of %d rows %d with the margin at the boundary, %d of them compared exactly, %d with the "
                  "margin at the winner" % (w, int(r.min()), int(r.max()), N, int(ok.sum()), int(far.sum()), int(won.sum())))
            assert torch.equal(tok[won], want[won]), (w, int((tok[won] != want[won]).sum()))
            assert float((lp.cpu().double() - s.gather(1, tok[:, None])[:, 0]).abs().max()) < 1e-5, w
    assert checked >= total // 2, (checked, total)
    # M identical members: the single member's set and draw, bit for bit
    for (T, top_p), k in zip(CASES, TOPKS):
        one = run_step(xs[:1], prev, T, k, rng, V, top_p)
        three = run_step([xs[0], xs[0].clone(), xs[0].clone()], prev, T, k, rng, V, top_p)
        assert torch.equal(one[0], three[0]) and torch.equal(one[1].view(torch.int32), three[1].view(torch.int32)), (T, k)
        assert torch.equal(one[2], three[2]), (T, k)


# ------------------------------------------------------------------------------------------------------------------
# 5. the draws follow the renormalised distribution
# ------------------------------------------------------------------------------------------------------------------
def chi2_quantile(df, z=4.753424308822899):
    """The 1 - 1e-6 quantile of chi2(df): scipy if importable, else Wilson-Hilferty (z = the normal's 1 - 1e-6 quantile)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.mark.parametrize("T,top_p,k", [(1.0, 0.8, 0), (0.7, 0.9, 16)])
def test_draws_follow_the_renormalised_distribution(T, top_p, k):
    N, V = 65536, 64
    g = torch.Generator().manual_seed(4)
    row = torch.log_softmax(torch.randn(V, generator=g) * 1.5, dim=0)
    x = row.expand(N, V).contiguous().cuda()
    prev = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    tok, _, r = run_step([x], prev, T, k, rng_words(31337), V, top_p)
    ss, order, c = pool_masses(row[None, :], T, k)
    assert float((c - top_p).abs().min()) > 1e-4                                 # the set does not hang on a rounding
    size = int(size_fp64(ss, c, top_p))
    assert 2 < size < (k if k else V)
    assert bool((r == size).all())
    nucleus = order[0, :size].numpy()
    counts = np.bincount(tok.cpu().numpy(), minlength=V).astype(np.float64)
    assert counts.sum() == N and counts[np.setdiff1d(np.arange(V), nucleus)].sum() == 0       # no draw outside the nucleus
    t = row.double().numpy()[nucleus] * inv_temp(T)
    p = np.exp(t - t.max())
    expect = N * p / p.sum()
    assert expect.min() >= 5.0                                                   # no cell needs pooling: df = size - 1
    stat = float(((counts[nucleus] - expect) ** 2 / expect).sum())
    bound = chi2_quantile(size - 1)
    print("T=%.1f top_p=%.2f top_k=%d: nucleus of %d words, chi-square %.1f, df %d, bound %.1f" % (T, top_p, k, size, stat, size - 1, bound))
    assert stat < bound, (T, top_p, k, stat, bound)
    # the check has power: the same counts against a temperature 10 % off
    p2 = np.exp((t - t.max()) / 1.1)
    e2 = N * p2 / p2.sum()
    assert float(((counts[nucleus] - e2) ** 2 / e2).sum()) > 3 * bound


# ------------------------------------------------------------------------------------------------------------------
# 6. the models
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


FIXTURES = ["text_tied_s0_f32", "mm_dot_tied_s0_f32"]


def ints(h):
    return [[int(t) for t in r] for r in h]


def same(a, b):
    return a.hyps == b.hyps and torch.equal(a.token_logp, b.token_logp) and torch.equal(a.logp, b.logp) and \
        torch.equal(a.score, b.score)


def check_sizes_of(out, sizes, ML):
    """sizes (B, n, ML): at least 1 on every sample's span (its words and the EOS that closes it), 0 after it."""
    B, n = len(out.hyps), len(out.hyps[0])
    assert sizes.shape == (B, n, ML) and sizes.dtype == torch.int32
    sz = sizes.cpu().numpy()
    for b in range(B):
        for j in range(n):
            span = min(ML, len(out.hyps[b][j]) + 1)
            assert (sz[b, j, :span] >= 1).all() and (sz[b, j, span:] == 0).all(), (b, j, sz[b, j], out.hyps[b][j])


def check_scores(obj, src, lens, im, text, out, ML, what):
    """score_translations of the drawn words against token_logp: 1e-4 per token (the bound of test_gpu_sample.py).  A drawn
    padding word 0 is fed on but not scored by forced decoding: such positions are left out."""
    B, n = len(out.hyps), len(out.hyps[0])
    flat = [list(out.hyps[b][j]) for b in range(B) for j in range(n)]
    Tt = max(len(r) + (len(r) < ML) for r in flat)
    tgt = torch.zeros(B * n, Tt, dtype=torch.int64)
    for i, r in enumerate(flat):
        r = r + [EOS] if len(r) < ML else r
        tgt[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    src_n = src.repeat_interleave(n, 0)
    lens_n = [L for L in lens for _ in range(n)]
    tgt = tgt.cuda()
    forced = obj.score_translations(src_n, lens_n, tgt) if text else obj.score_translations(src_n, lens_n, tgt, im.repeat_interleave(n, 0))
    tl = out.token_logp.reshape(B * n, ML)
    assert float(tl[:, Tt:].abs().sum()) == 0.0
    err = float(((tl[:, :Tt] - forced.token_logp).abs() * (tgt != 0)).max())
    print("%s: per-token max abs err %.3e" % (what, err))
    assert err <= 1e-4, (what, err)


@pytest.mark.parametrize("name", FIXTURES)
def test_models_nucleus_decode(name):
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Generator
    m, src, lens, im = golden_model(name, eos_bias=2.0)
    text = im is None
    ML, n = 10, 3
    kw = dict(n_samples=n, max_length=ML, temperature=0.9, top_p=0.9, return_sizes=True)
    res, ended = {}, 0
    for graph in (True, False):
        m.decode_graph = graph
        gen = Generator(123)
        st = gen.get_state()
        a, sa = m.sample_decode(src, lens, im, generator=gen, **kw)
        assert gen.get_state() == [st[0], st[1] + 1]
        b, sb = m.sample_decode(src, lens, im, generator=gen, **kw)              # another counter: other words
        assert not same(a, b)
        gen.set_state(st)
        a2, sa2 = m.sample_decode(src, lens, im, generator=gen, **kw)            # the same state (graph mode: a cache hit)
        assert same(a, a2) and torch.equal(sa, sa2)
        # another shape and other by-value arguments in between, then back
        m.sample_decode(src[:3], lens[:3], None if text else im[:3], generator=Generator(1), **kw)
        c, sc = m.sample_decode(src, lens, im, generator=Generator(123), n_samples=n, max_length=ML, temperature=0.9, top_p=0.5,
                                return_sizes=True)
        assert not same(a, c) and int(sc.sum()) < int(sa.sum())                  # a smaller nucleus
        a3, sa3 = m.sample_decode(src, lens, im, generator=Generator(123), **kw)
        assert same(a, a3) and torch.equal(sa, sa3)
        # without sizes: the same samples
        assert same(a, m.sample_decode(src, lens, im, generator=Generator(123), n_samples=n, max_length=ML, temperature=0.9, top_p=0.9))
        check_sizes_of(a, sa, ML)
        check_scores(m, src, lens, im, text, a, ML, "%s graph=%s" % (name, graph))
        ended += sum(len(h) < ML for hs in a.hyps for h in hs)
        # the sets are real cuts: smaller than the vocabulary, and a top-k pool is cut further
        V = m.decoder.out.bias.shape[0]
        assert 1 <= int(sa[sa > 0].min()) and int(sa.max()) < V
        d, sd = m.sample_decode(src, lens, im, generator=Generator(123), n_samples=n, max_length=ML, temperature=0.9, top_k=5, top_p=0.9,
                                return_sizes=True)
        assert int(sd.max()) <= 5
        check_sizes_of(d, sd, ML)
        # Ensemble([m]) is m
        ens = Ensemble([m])
        ens.decode_graph = graph
        e, se = ens.sample_decode(src, lens, im, generator=Generator(123), **kw)
        assert same(a, e) and torch.equal(sa, se)
        assert same(e, ens.sample_decode(src, lens, im, generator=Generator(123), **kw)[0])      # the ensemble's cache hit
        res[graph] = (a, sa, d, sd)
    assert ended > 0                                                             # the EOS rule was exercised
    assert same(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])       # graph and eager mode agree
    assert same(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])


def test_top_p_one_is_the_plain_decode_and_other_paths_are_untouched():
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Generator
    for name in FIXTURES:
        m, src, lens, im = golden_model(name, eos_bias=1.0)
        args = (src, lens) if im is None else (src, lens, im)
        ens = Ensemble([m])

        def snapshot():
            out = []
            for graph in (True, False):
                m.decode_graph = ens.decode_graph = graph
                hyps, sc = m.beamsearch_nbest(*args, beam_size=3, n_best=2, max_length=9)
                smp = [obj.sample_decode(src, lens, im, n_samples=3, max_length=9, temperature=0.8, top_k=k, generator=Generator(9))
                       for obj in (m, ens) for k in (0, 3)]
                out.append((ints(m.beamsearch_decode(*args, beam_size=3, max_length=9)), m.last_beam_scores.cpu().numpy().copy(),
                            ints(m.beamsearch_decode(*args, beam_size=1, max_length=9)), hyps, sc.cpu().numpy().copy(),
                            ints(ens.beamsearch_decode(src, lens, im, beam_size=3, max_length=9)), smp))
            return out

        before = snapshot()
        for graph in (True, False):
            m.decode_graph = ens.decode_graph = graph
            for obj in (m, ens):
                keys = set(m.__dict__.get("_decode_cache", {})), set(ens._cache)
                for k in (0, 3):
                    kw = dict(n_samples=3, max_length=9, temperature=0.8, top_k=k)
                    plain = obj.sample_decode(src, lens, im, generator=Generator(9), **kw)
                    one = obj.sample_decode(src, lens, im, generator=Generator(9), top_p=1.0, **kw)
                    assert same(plain, one), (name, graph, k)                    # bit for bit, and through the same decode state
                assert (set(m.__dict__.get("_decode_cache", {})), set(ens._cache)) == keys, (name, graph)
                for k in (0, 3):
                    kw = dict(n_samples=3, max_length=9, temperature=0.8, top_k=k)
                    plain = obj.sample_decode(src, lens, im, generator=Generator(9), **kw)
                    sized, sz = obj.sample_decode(src, lens, im, generator=Generator(9), top_p=1.0, return_sizes=True, **kw)
                    assert same(plain, sized), (name, graph, k)
                    V = m.decoder.out.bias.shape[0]
                    assert set(sz.unique().tolist()) <= {0, k if k else V}
                    check_sizes_of(sized, sz, 9)
                    obj.sample_decode(src, lens, im, top_p=0.7, **kw)
        after = snapshot()
        for x, y in zip(before, after):
            assert x[0] == y[0] and x[2] == y[2] and x[3] == y[3] and x[5] == y[5], name
            assert np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) and np.array_equal(x[4].view(np.int32), y[4].view(np.int32))
            assert all(same(p, q) for p, q in zip(x[6], y[6])), name
