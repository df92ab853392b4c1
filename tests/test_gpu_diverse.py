"""GPU: diverse beam search (vagnmt_hip.diverse; include/vag_nmt.h: vag_beam_div_step, vag_beam_finish_nbest_slots).

1. the expansion kernels against tests/diverse_ref.py, exactly: words, parents, score bits, hidden states, n_alive, tok_out --
   on log-probabilities quantised to 1/8 (ties everywhere: the total order is what is tested), with finished and repeating
   rows, strengths 0.5 and 2.0 (powers of two: strength * count is exact, the fused and the unfused key agree);
2. the device-index form, a whole search on a table "model" with the slots finish, the ABI's argument errors;
3. the models and Ensemble: n_groups = 1 is beamsearch_nbest, diversity = 0 is n_groups narrow searches, graph and eager mode,
   the decode caches' keys, scores against forced scores, mbr_decode's beam_groups."""
import ctypes as C

import numpy as np
import pytest
import torch

import diverse_ref as R

pytestmark = pytest.mark.gpu

EOS, UNK = 3, 1
I32, I64 = torch.int32, torch.int64


# ------------------------------------------------------------------------------------------------------------------
# the ABI by hand
# ------------------------------------------------------------------------------------------------------------------
def L():
    from vagnmt_hip import _lib
    return _lib.lib()


def stream():
    from vagnmt_hip import _lib
    return _lib.stream()


def pp(ts, off=0):
    return (C.c_void_p * len(ts))(*[t.data_ptr() + off for t in ts])


def p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Search:
    """The buffers of one search, driven step by step through the ABI."""

    def __init__(self, B, k, V, max_len, Hs):
        self.B, self.k, self.V, self.max_len, self.Hs = B, k, V, max_len, list(Hs)
        self.beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
        self.nll = torch.zeros(B, k, device="cuda")
        self.n_alive = torch.full((1,), -7, dtype=I32, device="cuda")
        self.scratch = torch.empty(L().vag_beam_div_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        self.tok = torch.full((B * k,), -1, dtype=I64, device="cuda")
        self.di_state = torch.zeros(2, dtype=I32, device="cuda")

    def step(self, logps, h_ins, di, G, lam, flags=0, device_index=False):
        """One expansion; logps / h_ins: M tensors (rows, ldl) / (rows, H[m]).  Returns (rc, h_outs)."""
        h_outs = [torch.full((self.B * self.k, H), float("nan"), device="cuda") for H in self.Hs]
        ldl = p64([x.shape[1] for x in logps])
        if device_index:
            rc = L().vag_beam_div_step_dev(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(),
                                           self.di_state.data_ptr(), self.max_len, pp(h_ins), pp(h_outs), p64(self.Hs),
                                           self.tok.data_ptr(), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                           self.scratch.data_ptr(), flags, G, lam, stream())
        else:
            rc = L().vag_beam_div_step(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(), di, self.max_len,
                                       pp(h_ins), pp(h_outs), p64(self.Hs), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                       self.scratch.data_ptr(), flags, G, lam, stream())
        return rc, h_outs


def quantised(rng, rows, V, ldl):
    """Log-probabilities on a grid of 1/8 in [-12, 0]; the columns past V hold +100 (a read there would win every selection)."""
    a = np.full((rows, ldl), 100.0, dtype=np.float32)
    a[:, :V] = rng.integers(-96, 1, size=(rows, V)) / 8.0
    return a


def kernel_combined(logps, V):
    """The kernels' own ensemble scores of every (row, word), read back through groups = 1 calls at step 0 on windows of at
    most 64 words (k = the window: the step then returns every word of the window with its score, c = 0 + score)."""
    rows = logps[0].shape[0]
    kw = min(64, V)
    starts = list(range(0, V - kw + 1, kw))
    if starts[-1] + kw < V:
        starts.append(V - kw)
    out = np.full((rows, V), np.nan, dtype=np.float32)
    s = Search(rows, kw, kw, 1, [1] * len(logps))
    h = [torch.zeros(rows, 1, device="cuda") for _ in logps]
    for w0 in starts:
        ho = [torch.empty(rows * kw, 1, device="cuda") for _ in logps]
        rc = L().vag_beam_div_step(pp(logps, 4 * w0), p64([x.shape[1] for x in logps]), len(logps), s.nll.data_ptr(),
                                   s.beam.data_ptr(), 0, 1, pp(h), pp(ho), p64(s.Hs), rows, kw, kw, s.n_alive.data_ptr(),
                                   s.scratch.data_ptr(), 0, 1, 0.0, stream())
        assert rc == 0
        words, vals = s.beam[0].cpu().numpy(), s.nll.cpu().numpy()
        assert all(sorted(r) == list(range(kw)) for r in words.tolist())
        np.put_along_axis(out[:, w0:w0 + kw], words, vals, axis=1)
    assert not np.isnan(out).any()
    return out


def check_step(B, k, G, V, ldl, M, di, lam, flags, seed, Hs):
    rng = np.random.default_rng(seed)
    k_in = 1 if di == 0 else k
    rows = B * k_in
    max_len = 4
    lp = [quantised(rng, rows, V, ldl) for _ in range(M)]
    if M > 1:                                     # members that disagree, off the grid
        lp = [a + np.float32(0.01 * m) * rng.standard_normal(a.shape).astype(np.float32) for m, a in enumerate(lp)]
        for a in lp:
            a[:, V:] = 100.0
    s = Search(B, k, V, max_len, Hs)
    base = prev = None
    if di > 0:
        base = (rng.integers(-400, 0, size=(B, k)) / 8.0).astype(np.float32)
        prev = rng.integers(0, V, size=(B, k))
        prev[rng.random((B, k)) < 0.3] = EOS
        prev[:, k - 1] = prev[:, 0]               # two rows with the same previous word
        s.nll.copy_(dev(base))
        s.beam[di - 1].copy_(dev(prev))
    h_in = [rng.standard_normal((rows, H)).astype(np.float32) for H in Hs]
    logps = [dev(a) for a in lp]
    if M == 1:
        comb = lp[0][:, :V]
    else:
        # the NumPy restatement of ens_score may differ from the device's expf / logf in the last bits: it is checked to a few
        # ulp, and the selection is compared exactly on the kernels' own combined values
        comb = kernel_combined(logps, V)
        want = R.ens_combine([a[:, :V] for a in lp])
        assert np.allclose(comb, want, rtol=2e-6, atol=2e-6), np.abs(comb - want).max()
    s.di_state.copy_(torch.tensor([di, 0], dtype=I32))
    rc, h_out = s.step(logps, [dev(h) for h in h_in], di, G, lam, flags, device_index=di > 0)
    assert rc == 0
    words, parents = s.beam[di].cpu().numpy(), s.beam[max_len + di].cpu().numpy()
    nll = s.nll.cpu().numpy()
    alive = 0
    for b in range(B):
        w, p, sc = R.step(comb[b * k_in:(b + 1) * k_in], None if di == 0 else base[b], None if di == 0 else prev[b], k, G, lam,
                          flags)
        what = (B, k, G, V, M, di, lam, flags, b)
        assert words[b].tolist() == w.tolist(), what
        assert parents[b].tolist() == p.tolist(), what
        assert nll[b].tobytes() == sc.tobytes(), what
        for m, H in enumerate(Hs):
            got = h_out[m].cpu().numpy()[b * k:(b + 1) * k]
            assert got.tobytes() == h_in[m][b * k_in + p].tobytes(), what
        alive += int((w != EOS).sum())
    assert int(s.n_alive.item()) == alive
    if di > 0:
        assert s.tok.cpu().numpy().tolist() == words.reshape(-1).tolist()
        assert s.di_state.cpu().tolist() == [di + 1, 0]


SHAPES = [(3, 6, 3, 50, 50), (2, 4, 4, 2500, 2504), (1, 12, 2, 4100, 4100), (2, 64, 8, 70, 70), (2, 12, 3, 10000, 10000)]


@pytest.mark.parametrize("B,k,G,V,ldl", SHAPES)
def test_step_matches_reference_exactly(B, k, G, V, ldl):
    seed = 0
    for lam in (0.5, 2.0):
        for flags in (0, 3):
            for di in (0, 2):
                seed += 1
                check_step(B, k, G, V, ldl, 1, di, lam, flags, 1000 * V + seed, [8] if seed % 2 else [6])


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("B,k,G,V,ldl", [SHAPES[0], SHAPES[-1]])
def test_ensemble_step_matches_reference_exactly(B, k, G, V, ldl, M):
    for n, (lam, flags, di) in enumerate([(0.5, 0, 0), (2.0, 3, 1), (0.5, 3, 2)]):
        check_step(B, k, G, V, ldl, M, di, lam, flags, 77 * V + 10 * M + n, [8, 6, 4][:M])


def test_one_group_is_the_plain_step_bit_for_bit():
    """groups = 1 against vag_beam_ens_step_opt on the same inputs: words, parents, score bits, hidden states."""
    rng = np.random.default_rng(5)
    B, k, V, max_len, H = 2, 12, 4100, 4, 8
    for di, flags in [(0, 0), (2, 3), (1, 0)]:
        k_in = 1 if di == 0 else k
        logp = [dev(quantised(rng, B * k_in, V, V))]
        h_in = [dev(rng.standard_normal((B * k_in, H)).astype(np.float32))]
        base = dev((rng.integers(-400, 0, size=(B, k)) / 8.0).astype(np.float32))
        prev = rng.integers(0, V, size=(B, k))
        prev[rng.random((B, k)) < 0.3] = EOS
        a, p = Search(B, k, V, max_len, [H]), Search(B, k, V, max_len, [H])
        for s in (a, p):
            s.nll.copy_(base)
            if di > 0:
                s.beam[di - 1].copy_(dev(prev))
        rc, ha = a.step(logp, h_in, di, 1, 0.5, flags)
        assert rc == 0
        hp = [torch.empty(B * k, H, device="cuda")]
        scratch = torch.empty(L().vag_beam_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        assert L().vag_beam_ens_step_opt(pp(logp), p64([V]), 1, p.nll.data_ptr(), p.beam.data_ptr(), di, max_len, pp(h_in), pp(hp),
                                         p64([H]), B, k, V, p.n_alive.data_ptr(), scratch.data_ptr(), flags, stream()) == 0
        assert torch.equal(a.beam, p.beam) and torch.equal(a.nll.view(I32), p.nll.view(I32)), (di, flags)
        assert torch.equal(ha[0].view(I32), hp[0].view(I32)) and torch.equal(a.n_alive, p.n_alive)


def test_device_index_form():
    rng = np.random.default_rng(6)
    B, k, G, V, max_len, H, lam = 3, 6, 3, 50, 3, 8, 0.5
    lps = [dev(quantised(rng, B * (1 if di == 0 else k), V, V)) for di in range(3)]
    h0 = dev(rng.standard_normal((B, H)).astype(np.float32))
    a, d = Search(B, k, V, max_len, [H]), Search(B, k, V, max_len, [H])
    for s in (a, d):
        rc, h = s.step([lps[0]], [h0], 0, G, lam)
        assert rc == 0
        s.h = h
    for di in (1, 2):
        rc, a.h = a.step([lps[di]], a.h, di, G, lam)
        assert rc == 0
    d.di_state.copy_(torch.tensor([1, 0], dtype=I32))
    for di in (1, 2):
        rc, d.h = d.step([lps[di]], d.h, 0, G, lam, device_index=True)
        assert rc == 0
    assert d.di_state.cpu().tolist() == [3, 0]
    assert torch.equal(a.beam, d.beam) and torch.equal(a.nll.view(I32), d.nll.view(I32)) and torch.equal(a.h[0], d.h[0])
    assert torch.equal(a.n_alive, d.n_alive) and torch.equal(d.tok, d.beam[2].view(-1))
    # at di >= max_len the launches write nothing
    before = [t.clone() for t in (d.beam, d.nll, d.tok, d.n_alive, d.di_state)]
    d.n_alive.fill_(-3); before[3].fill_(-3)
    rc, h = d.step([lps[2]], d.h, 0, G, lam, device_index=True)
    assert rc == 0
    for t, b in zip((d.beam, d.nll, d.tok, d.n_alive, d.di_state), before):
        assert torch.equal(t, b)
    assert bool(torch.isnan(h[0]).all())


def test_whole_search_on_a_table_model():
    rng = np.random.default_rng(7)
    B, k, G, V, steps, H, lam = 2, 6, 3, 50, 8, 4, 0.5
    max_len = steps
    T = (rng.integers(-96, 1, size=(V, V)) / 8.0).astype(np.float32)
    T[:, EOS] += np.float32(1.5)                                         # some hypotheses finish
    Td = dev(T)
    s = Search(B, k, V, max_len, [H])
    h = [torch.zeros(B, H, device="cuda")]
    for di in range(steps):
        tok = torch.full((B,), R.SOS, dtype=I64, device="cuda") if di == 0 else s.beam[di - 1].reshape(-1)
        rc, h = s.step([Td[tok].contiguous()], h, di, G, lam)
        assert rc == 0
    beam, nll = R.search(lambda tok: T[tok], B, k, G, lam, V, max_len, steps)
    assert np.array_equal(s.beam.cpu().numpy(), beam) and s.nll.cpu().numpy().tobytes() == nll.tobytes()
    want_out, want_sc, want_slots = R.finish(beam, nll, max_len, steps, k)
    out = torch.empty(B, k, max_len, dtype=I64, device="cuda")
    sc = torch.empty(B, k, device="cuda")
    slots = torch.empty(B, k, dtype=I64, device="cuda")
    assert L().vag_beam_finish_nbest_slots(s.nll.data_ptr(), s.beam.data_ptr(), max_len, steps, B, k, k, out.data_ptr(),
                                           sc.data_ptr(), slots.data_ptr(), stream()) == 0
    assert np.array_equal(out.cpu().numpy(), want_out) and sc.cpu().numpy().tobytes() == want_sc.tobytes()
    assert np.array_equal(slots.cpu().numpy() // (k // G), want_slots // (k // G))
    assert np.array_equal(slots.cpu().numpy(), want_slots)
    assert len({tuple(r) for r in want_out[0].tolist()}) > 1
    out2, sc2 = torch.empty_like(out), torch.empty_like(sc)
    assert L().vag_beam_finish_nbest(s.nll.data_ptr(), s.beam.data_ptr(), max_len, steps, B, k, k, out2.data_ptr(),
                                     sc2.data_ptr(), stream()) == 0
    assert torch.equal(out, out2) and torch.equal(sc.view(I32), sc2.view(I32))


def test_abi_argument_errors_launch_nothing():
    B, k, V, max_len, H = 2, 6, 50, 4, 8
    s = Search(B, k, V, max_len, [H])
    logp = [torch.zeros(B, V, device="cuda")]
    h = [torch.zeros(B, H, device="cuda")]

    def call(G=3, lam=0.5, k_=k, V_=V, flags=0, M=1, di=0, nll=None, dev_form=False, state=True):
        ho = [torch.full((B * 64, H), float("nan"), device="cuda")]
        nllp = s.nll.data_ptr() if nll is None else nll
        if dev_form:
            rc = L().vag_beam_div_step_dev(pp(logp), p64([V]), M, nllp, s.beam.data_ptr(), s.di_state.data_ptr() if state else None,
                                           max_len, pp(h), pp(ho), p64([H]), s.tok.data_ptr(), B, k_, V_, s.n_alive.data_ptr(),
                                           s.scratch.data_ptr(), flags, G, lam, stream())
        else:
            rc = L().vag_beam_div_step(pp(logp), p64([V]), M, nllp, s.beam.data_ptr(), di, max_len, pp(h), pp(ho), p64([H]), B, k_,
                                       V_, s.n_alive.data_ptr(), s.scratch.data_ptr(), flags, G, lam, stream())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ho[0]).all())
    bad = [dict(G=0), dict(G=-1), dict(G=4), dict(V_=5), dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(flags=4), dict(M=0), dict(M=9), dict(k_=65, G=5), dict(k_=0), dict(di=-1), dict(di=max_len), dict(nll=0),
           dict(dev_form=True, state=False)]
    for kw in bad:
        assert call(**kw) == (-22, True), kw
    assert int(s.n_alive.item()) == -7 and not bool(s.beam.any()) and not bool(s.nll.any())
    assert L().vag_beam_div_step(None, p64([V]), 1, s.nll.data_ptr(), s.beam.data_ptr(), 0, max_len, pp(h), pp(h), p64([H]), B, k, V,
                                 s.n_alive.data_ptr(), s.scratch.data_ptr(), 0, 3, 0.5, stream()) == -22
    out = torch.zeros(B, k, max_len, dtype=I64, device="cuda")
    sc = torch.zeros(B, k, device="cuda")
    assert L().vag_beam_finish_nbest_slots(s.nll.data_ptr(), s.beam.data_ptr(), max_len, 2, B, k, k, out.data_ptr(), sc.data_ptr(),
                                           None, stream()) == -22
    assert L().vag_beam_finish_nbest_slots(s.nll.data_ptr(), s.beam.data_ptr(), max_len, 2, B, k, k + 1, out.data_ptr(),
                                           sc.data_ptr(), out.data_ptr(), stream()) == -22
    assert L().vag_beam_div_scratch_bytes(16, 12, 9391, 80) >= 16 * 12 * 5 * 12 * 12
    assert call() == (0, False)                                             # and the good call goes through


# ------------------------------------------------------------------------------------------------------------------
# models (small random ones, built as tests/test_gpu_nbest_score.py builds them)
# ------------------------------------------------------------------------------------------------------------------
VS, VT, IM, ML = 70, 503, 64, 10
LENS = [9, 6, 3]


def make_model(kind, seed, E=32, H=64, attn="dot", tied=True, eos_bias=0.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    if kind == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(VS, VT, IM, E, E, H, 48, 0.99, attn_model=attn, tied_emb=tied)
    else:
        m = NMT_Seq2Seq_Beam_V2(VS, VT, E, E, H, tied_emb=tied)
    with torch.no_grad():
        m.decoder.out.bias[EOS] += eos_bias
    return m.cuda().eval()


def make_inputs(lens=LENS, seed=9):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        src[b, :n] = torch.randint(4, VS, (n,), generator=g)
    return src.cuda(), torch.randn(len(lens), IM, generator=g).abs().cuda()


def ints(hyps):
    return [[[int(t) for t in r] for r in h] for h in hyps]


def bits(t):
    return t.detach().cpu().contiguous().view(I32)


@pytest.fixture(scope="module", params=["mm", "text"])
def subject(request):
    m = make_model(request.param, 21, eos_bias=2.0)
    src, im = make_inputs()
    return request.param, m, src, (im if request.param == "mm" else None)


def nbest(m, src, im, k, n, lens=LENS):
    return m.beamsearch_nbest(src, lens, im, k, n, ML) if im is not None else m.beamsearch_nbest(src, lens, k, n, ML)


def by_group(d, G):
    """hyps and scores of a Diverse, per sentence and group, in rank order."""
    grp = d.group.cpu().tolist()
    sc = bits(d.scores).tolist()
    hy = ints(d.hyps)
    return [[[(hy[b][r], sc[b][r]) for r in range(len(hy[b])) if grp[b][r] == i] for i in range(G)] for b in range(len(hy))]


def test_one_group_is_beamsearch_nbest(subject):
    _, m, src, im = subject
    for graph in (True, False):
        m.decode_graph = graph
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(m, src, im, k, n)
            d = m.beamsearch_diverse(src, LENS, im, beam_size=k, n_groups=1, diversity=0.5, n_best=n, max_length=ML)
            assert ints(d.hyps) == ints(hyps) and torch.equal(bits(d.scores), bits(sc)), (graph, k)
            assert d.group.dtype == I64 and d.group.shape == (3, n) and not bool(d.group.any())
    m.decode_graph = True


def test_zero_diversity_is_narrow_searches(subject):
    _, m, src, im = subject
    for graph in (True, False):
        m.decode_graph = graph
        hyps, sc = nbest(m, src, im, 2, 2)
        d = m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=3, diversity=0.0, max_length=ML)
        want = [list(zip(h, s)) for h, s in zip(ints(hyps), bits(sc).tolist())]
        got = by_group(d, 3)
        for b in range(3):
            for i in range(3):
                assert got[b][i] == want[b], (graph, b, i)
    m.decode_graph = True


def test_graph_and_eager_agree_and_the_cache_keeps_settings_apart(subject):
    kind, m, src, im = subject
    res = {}
    for graph in (True, False):
        m.decode_graph = graph
        for G, lam in [(3, 0.5), (2, 0.5), (3, 4.0), (3, 0.5)]:           # a graph captured for one setting is not another's
            d = m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=G, diversity=lam, max_length=ML)
            fresh = make_model(kind, 21, eos_bias=2.0)                     # the same weights, nothing cached
            fresh.decode_graph = graph
            f = fresh.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=G, diversity=lam, max_length=ML)
            assert ints(d.hyps) == ints(f.hyps) and torch.equal(d.group, f.group) and torch.equal(bits(d.scores), bits(f.scores)), \
                (graph, G, lam)
            sc = d.scores.cpu()
            assert bool((sc[:, 1:] <= sc[:, :-1]).all()) and sorted(d.group[0].tolist()) == sorted(list(range(G)) * (6 // G))
            res.setdefault((G, lam), []).append(d)
    for key, ds in res.items():
        g, e = ds[0], ds[-1]
        # two fp32 evaluations of the same sums (graph mode pads the source to 8 positions, which regroups the attention's
        # reductions): the relative 2e-4 the search-vs-forced-score test accepts for such a pair; lists and groups are equal
        rel = ((g.scores - e.scores).abs() / e.scores.abs().clamp(min=1.0)).max().item()
        print("graph vs eager", key, "max rel score diff %.3e" % rel)
        assert ints(g.hyps) == ints(e.hyps) and torch.equal(g.group, e.group) and rel <= 2e-4, key
    m.decode_graph = True


def test_ensemble_of_twins_is_the_model(subject):
    from vagnmt_hip.ensemble import Ensemble
    _, m, src, im = subject
    ens = Ensemble([m, m])
    for graph in (True, False):
        m.decode_graph = ens.decode_graph = graph
        d = m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=3, diversity=0.5, n_best=4, max_length=ML)
        e = ens.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=3, diversity=0.5, n_best=4, max_length=ML)
        assert ints(d.hyps) == ints(e.hyps) and torch.equal(bits(d.scores), bits(e.scores)) and torch.equal(d.group, e.group)
    m.decode_graph = True


def test_huge_diversity_separates_first_words(subject):
    _, m, src, im = subject
    d = m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=3, diversity=1e6, max_length=ML)
    for b, groups in enumerate(by_group(d, 3)):
        firsts = [{(h[0] if h else EOS) for h, _ in grp} for grp in groups]
        assert all(len(grp) == 2 for grp in groups)
        assert all(not (firsts[i] & firsts[j]) for i in range(3) for j in range(i)), (b, firsts)
    assert bool((d.scores[:, 0] > -1e4).all())                    # the penalty is not part of a score


def test_scores_are_forced_scores(subject):
    """Every returned hypothesis that ended before max_length without a -1e5 step scores, forced, what the search scored it:
    relative 2e-4, the bound of the search-vs-scoring test of beamsearch_nbest.  Six sentences: 36 hypotheses to find 8 in."""
    kind, _, _, _ = subject
    m = make_model(kind, 23)
    lens = [9, 8, 6, 5, 3, 2]
    src, im = make_inputs(lens, seed=11)
    im = im if kind == "mm" else None
    k, B = 6, len(lens)
    idx = []
    for extra in (0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0):
        with torch.no_grad():
            m.decoder.out.bias[EOS] += extra
        d = m.beamsearch_diverse(src, lens, im, beam_size=k, n_groups=3, diversity=0.5, max_length=ML)
        sc = d.scores.cpu().numpy()
        idx = [(b, r) for b in range(B) for r in range(k) if len(d.hyps[b][r]) < ML - 1 and sc[b, r] > -1e4]
        if len(idx) >= 8:
            break
    assert len(idx) >= 8, len(idx)
    flat = [list(d.hyps[b][r]) for b in range(B) for r in range(k)]
    src_n = src.repeat_interleave(k, 0)
    lens_n = [n for n in lens for _ in range(k)]
    forced = m.score_translations(src_n, lens_n, flat, im.repeat_interleave(k, 0)) if kind == "mm" else \
        m.score_translations(src_n, lens_n, flat)
    f = forced.score.cpu().numpy().reshape(B, k)
    rel = max(abs(float(f[b, r]) - float(sc[b, r])) / max(1.0, abs(float(sc[b, r]))) for b, r in idx)
    print("%d finished hypotheses, forced vs search score: max rel err %.3e" % (len(idx), rel))
    assert rel <= 2e-4, rel


def test_mbr_decode_takes_the_diverse_list(subject):
    from vagnmt_hip.mbr import mbr_select
    from vagnmt_hip.sampling import Generator
    _, m, src, im = subject
    n = 4
    kw = dict(n_samples=n, max_length=ML, temperature=0.9)
    gen = Generator(5)
    st = gen.get_state()
    best0, sel0, drawn = m.mbr_decode(src, LENS, im, beam_size=6, generator=gen, **kw)
    gen.set_state(st)
    best1, sel1, drawn1 = m.mbr_decode(src, LENS, im, beam_size=6, beam_groups=1, beam_diversity=3.0, generator=gen, **kw)
    assert best0 == best1 and torch.equal(sel0.index, sel1.index) and torch.equal(bits(sel0.expected), bits(sel1.expected))
    plain = nbest(m, src, im, 6, 6)[0]
    want0 = mbr_select([drawn.hyps[b] + plain[b] for b in range(3)], refs=drawn.hyps)
    assert torch.equal(sel0.index, want0.index) and torch.equal(bits(sel0.expected), bits(want0.expected))
    gen.set_state(st)
    best3, sel3, drawn3 = m.mbr_decode(src, LENS, im, beam_size=6, beam_groups=3, beam_diversity=0.5, generator=gen, **kw)
    assert ints(drawn3.hyps) == ints(drawn.hyps) and sel3.expected.shape == (3, n + 6)
    beams = m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=3, diversity=0.5, max_length=ML).hyps
    cands = [drawn.hyps[b] + beams[b] for b in range(3)]
    want3 = mbr_select(cands, refs=drawn.hyps)
    assert torch.equal(sel3.index, want3.index) and torch.equal(bits(sel3.expected), bits(want3.expected))
    assert best3 == [cands[b][int(sel3.index[b])] for b in range(3)] == sel3.best
    with pytest.raises(ValueError, match="mbr_decode"):
        m.mbr_decode(src, LENS, im, beam_size=6, beam_groups=4, generator=gen, **kw)
    with pytest.raises(ValueError, match="beamsearch_diverse"):
        m.beamsearch_diverse(src, LENS, im, beam_size=6, n_groups=4)
