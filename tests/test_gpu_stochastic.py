"""GPU: stochastic beam search (vagnmt_hip.stochastic; include/vag_nmt.h: vag_beam_sbs_step).

1. one step against tests/stochastic_ref.py on the noise read back through vag_sample_noise: every perturbed score within
   16 ulp of the largest magnitude it was formed from, the scores bit for bit, the chosen set wherever the reference's gaps decide
   it, both paths of stage 2, finished rows, the device-index form;
2. the distribution: the ABI on a 5-word Markov model, 16384 replications against the exact probabilities, inclusion
   probabilities and the unbiasedness of the weighted estimator;
3. the public call on a small golden model: distinct hypotheses, scores against forced scores, determinism, eager and graph
   mode, an Ensemble of twins, mbr_decode(without_replacement=True).
The neighbours (sample_decode, beamsearch_nbest) are pinned by their own suites."""
import ctypes as C

import numpy as np
import pytest
import torch

import stochastic_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

EOS = 3
I32, I64 = torch.int32, torch.int64


def L():
    from vagnmt_hip import _lib
    return _lib.lib()


def stream():
    from vagnmt_hip import _lib
    return _lib.stream()


def pp(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(I32)


class Search:
    """The buffers of one search, driven step by step through the ABI."""

    def __init__(self, B, k, V, max_len, H, seed=5, counter=2):
        self.B, self.k, self.V, self.max_len, self.H = B, k, V, max_len, H
        self.beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
        self.nll = torch.zeros(B, k, device="cuda")
        self.gum = torch.full((B, k), float("nan"), device="cuda")            # step 0 ignores it
        self.n_alive = torch.full((1,), -7, dtype=I32, device="cuda")
        self.scratch = torch.empty(L().vag_beam_sbs_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        self.tok = torch.full((B * k,), -1, dtype=I64, device="cuda")
        self.di_state = torch.zeros(2, dtype=I32, device="cuda")
        self.rng = torch.tensor([seed, counter], dtype=I64, device="cuda")

    def noise(self, di, rows):
        out = torch.empty(rows, self.V, device="cuda")
        assert L().vag_sample_noise(self.rng.data_ptr(), di, rows, self.V, out.data_ptr(), stream()) == 0
        return out

    def step(self, logp, h_in, di, flags=0, device_index=False):
        h_out = torch.full((self.B * self.k, self.H), float("nan"), device="cuda")
        a = (pp([logp]), p64([logp.shape[1]]), 1, self.nll.data_ptr(), self.beam.data_ptr())
        b = (self.B, self.k, self.V, self.n_alive.data_ptr(), self.scratch.data_ptr(), flags, self.rng.data_ptr(),
             self.gum.data_ptr(), stream())
        if device_index:
            rc = L().vag_beam_sbs_step_dev(*a, self.di_state.data_ptr(), self.max_len, pp([h_in]), pp([h_out]), p64([self.H]),
                                           self.tok.data_ptr(), *b)
        else:
            rc = L().vag_beam_sbs_step(*a, di, self.max_len, pp([h_in]), pp([h_out]), p64([self.H]), *b)
        return rc, h_out


# ------------------------------------------------------------------------------------------------------------------
# 1. one step against the reference
# ------------------------------------------------------------------------------------------------------------------
def run_case(case):
    """One case of stochastic_ref.CASES on the device and in the reference: (largest |gum - reference| / tol, sentences whose
    chosen set was compared, sentences)."""
    B, k, V, di = case
    c = R.make_case(case)
    rows_in = 1 if di == 0 else k
    max_len, H = 4, 8
    s = Search(B, k, V, max_len, H, seed=R.case_seed(case))
    if di > 0:
        s.nll.copy_(dev(c["base"]))
        s.gum.copy_(dev(c["G"]))
        s.beam[di - 1].copy_(dev(c["prev"]))
    ldl = V + 3                                           # columns past V hold +100: a read there would win every selection
    logp = torch.full((B * rows_in, ldl), 100.0, device="cuda")
    logp[:, :V] = dev(c["logp"].reshape(B * rows_in, V))
    h_in = torch.randn(B * rows_in, H, device="cuda")
    noise = s.noise(di, B * rows_in).cpu().numpy().reshape(B, rows_in, V)
    device_index = di > 0 and k != 5
    s.di_state.copy_(torch.tensor([di, 0], dtype=I32))
    rc, h_out = s.step(logp, h_in, di, c["flags"], device_index)
    assert rc == 0, case
    r = R.step(c["logp"], noise, c["base"], c["prev"], c["G"], k, c["flags"])
    words, parents = s.beam[di].cpu().numpy(), s.beam[max_len + di].cpu().numpy()
    nll, gum = s.nll.cpu().numpy(), s.gum.cpu().numpy()
    assert ((words >= 0) & (words < V) & (parents >= 0) & (parents < rows_in)).all(), case
    at = lambda a: a[np.arange(B)[:, None], parents, words]                  # noqa: E731
    assert at(r["cand"]).all(), case                                         # only candidates are chosen
    for b in range(B):
        assert len({(int(p), int(w)) for p, w in zip(parents[b], words[b])}) == k, case
    # the perturbed scores: within tol of the reference's value for the same (parent, word); ranked; exact where inherited
    ratio = np.abs(gum.astype(np.float64) - at(r["gt_all"])) / at(r["tol_all"])
    assert ratio.max() <= 1.0, (case, ratio.max())
    assert (np.diff(gum, axis=1) <= 0).all(), case
    Gp = np.zeros((B, rows_in), dtype=np.float32) if di == 0 else c["G"]
    ex = at(r["exact_all"])
    assert ex[:, 0].all() and gum[ex].tobytes() == np.take_along_axis(Gp, parents, axis=1)[ex].tobytes(), case
    # the stored score is c, bit for bit
    assert nll.tobytes() == at(r["c_all"]).tobytes(), case
    # the chosen set, wherever the reference's gaps decide it
    compared = 0
    for b in range(B):
        if r["comparable"][b]:
            compared += 1
            got = {(int(p), int(w)) for p, w in zip(parents[b], words[b])}
            want = {(int(p), int(w)) for p, w in zip(r["parents"][b], r["words"][b])}
            assert got == want, (case, b)
    # and what every expansion does besides: the hidden states, the alive count, the device-index form's words and step
    hi = h_in.cpu().numpy().reshape(B, rows_in, H)
    assert h_out.cpu().numpy().reshape(B, k, H).tobytes() == hi[np.arange(B)[:, None], parents].tobytes(), case
    assert int(s.n_alive.item()) == int((words != EOS).sum()), case
    if device_index:
        assert s.tok.cpu().numpy().tolist() == words.reshape(-1).tolist() and s.di_state.cpu().tolist() == [di + 1, 0], case
    return float(ratio.max()), compared, B


def test_one_step_matches_the_reference():
    worst, compared, total = 0.0, 0, 0
    for case in R.CASES:
        ratio, n, B = run_case(case)
        print("case B=%d k=%d V=%d di=%d: largest |gum - ref| / tol = %.3f, %d of %d sets compared" % (case + (ratio, n, B)))
        worst, compared, total = max(worst, ratio), compared + n, total + B
    print("largest ratio over all cases: %.3f; %d of %d (sentence, step) cases left out of the set comparison"
          % (worst, total - compared, total))
    assert (total - compared) * 100 <= total


def test_abi_argument_errors_launch_nothing():
    B, k, V, max_len, H = 2, 6, 50, 4, 8
    s = Search(B, k, V, max_len, H)
    logp, h = torch.zeros(B, V, device="cuda"), torch.zeros(B, H, device="cuda")

    def call(rng=True, gum=True, k_=k, V_=V, flags=0, M=1, di=0):
        ho = torch.full((B * 64, H), float("nan"), device="cuda")
        rc = L().vag_beam_sbs_step(pp([logp]), p64([V]), M, s.nll.data_ptr(), s.beam.data_ptr(), di, max_len, pp([h]), pp([ho]),
                                   p64([H]), B, k_, V_, s.n_alive.data_ptr(), s.scratch.data_ptr(), flags,
                                   s.rng.data_ptr() if rng else None, s.gum.data_ptr() if gum else None, stream())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ho).all())
    for kw in [dict(rng=False), dict(gum=False), dict(V_=5), dict(flags=4), dict(M=0), dict(M=9), dict(k_=65), dict(k_=0),
               dict(di=-1), dict(di=max_len)]:
        assert call(**kw) == (-22, True), kw
    assert int(s.n_alive.item()) == -7 and not bool(s.beam.any()) and bool(torch.isnan(s.gum).all())
    assert call() == (0, False)                                             # and the good call goes through
    # past the end the device-index form writes nothing
    s.di_state.copy_(torch.tensor([max_len, 0], dtype=I32))
    before = [t.clone() for t in (s.beam, s.nll, s.gum, s.tok, s.di_state)]
    rc, ho = s.step(torch.zeros(B * k, V, device="cuda"), torch.zeros(B * k, H, device="cuda"), 0, device_index=True)
    assert rc == 0 and bool(torch.isnan(ho).all())
    for t, b in zip((s.beam, s.nll, s.gum, s.tok, s.di_state), before):
        assert torch.equal(t, b)


# ------------------------------------------------------------------------------------------------------------------
# 2. the distribution
# ------------------------------------------------------------------------------------------------------------------
def test_samples_without_replacement_from_a_markov_model():
    """V = 5, k = 3, two steps, 16384 replications of the one sentence through the ABI (B k = 49152 rows).  Exact values from
    enumerating the 21 leaves and their ordered triples.  The weighted estimator takes the perturbed scores as the public call
    hands them on, through sbs_uncondition with one more draw of the same generator: the search's own are conditioned on their
    maximum, the root's G = 0 (tests/test_stochastic_host.py pins what that would cost)."""
    from vagnmt_hip.stochastic import sbs_log_weights, sbs_uncondition
    T = R.markov_table()
    B, k, V, max_len, steps = 16384, 3, 5, 3, 2
    names, p, incl = R.exact_markov(T, steps, k)
    Td = dev(T)
    s = Search(B, k, V, max_len, 1, seed=20190614, counter=0)
    h = torch.zeros(B, 1, device="cuda")
    for di in range(steps):
        prev = torch.full((B,), R.SOS, dtype=I64, device="cuda") if di == 0 else s.beam[di - 1].reshape(-1)
        rc, h = s.step(Td[prev].contiguous(), h, di, R.ALLOW_REPEAT)
        assert rc == 0
    beam = s.beam.cpu().numpy()
    hyps = R.resolve(beam[:steps], beam[max_len:max_len + steps])
    index = {y: i for i, y in enumerate(names)}
    ids = np.array([[index[tuple(y)] for y in sent] for sent in hyps.tolist()])
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                                 # the three hypotheses are pairwise distinct
    logp, gum = s.nll.cpu(), s.gum.cpu()
    assert np.abs(logp.numpy().astype(np.float64) - np.log(p)[ids]).max() < 1e-5
    assert bool((gum[:, 0] == 0).all()) and bool((gum[:, 1:] <= gum[:, :-1]).all())
    first = np.bincount(ids[:, 0], minlength=len(names)) / B
    z1 = np.abs(first - p) / np.sqrt(p * (1 - p) / B)
    inc = np.array([(ids == i).any(axis=1).mean() for i in range(len(names))])
    z2 = np.abs(inc - incl) / np.sqrt(incl * (1 - incl) / B)
    print("slot 0 against p: largest deviation %.2f standard errors; inclusion: %.2f" % (z1.max(), z2.max()))
    assert z1.max() <= 5 and z2.max() <= 5
    # the estimator: mean_b sum_i w_i 1[y_i = y] against p(y), the standard error the reference's own over as many replications
    top = torch.empty(B, 1, device="cuda")
    assert L().vag_sample_noise(s.rng.data_ptr(), max_len, B, 1, top.data_ptr(), stream()) == 0
    w = torch.exp(sbs_log_weights(logp, sbs_uncondition(gum, top.cpu()))).numpy()
    nrng = np.random.default_rng(7)
    rh, rlp, rg = R.markov_search(T, B, k, steps, nrng)
    rids = np.array([[index[tuple(y)] for y in sent] for sent in rh.tolist()])
    rfree = sbs_uncondition(torch.from_numpy(rg.astype(np.float32)), torch.from_numpy(nrng.gumbel(size=(B, 1)).astype(np.float32)))
    rw = torch.exp(sbs_log_weights(torch.from_numpy(rlp), rfree)).numpy()
    z3 = []
    for i in range(len(names)):
        se = (rw * (rids == i)).sum(axis=1).std(ddof=1) / np.sqrt(B)
        z3.append(abs((w * (ids == i)).sum(axis=1).mean() - p[i]) / se)
    print("weighted estimator against p: largest deviation %.2f standard errors" % max(z3))
    assert max(z3) <= 5


# ------------------------------------------------------------------------------------------------------------------
# 3. the public call
# ------------------------------------------------------------------------------------------------------------------
ML, N = 16, 6
LENS = [8, 6, 5, 3]                  # a source of 8 positions: graph mode pads to a multiple of 8, here nothing


def golden_model(name="mm_dot_tied_s0_f32", eos_bias=3.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    meta, P, z = load_golden(name)
    Vs, Vt, I, E, H, S, B, Ts, Tt = meta["dims"]
    m = NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, meta["loss_w"], attn_model=meta["attn"],
                                              tied_emb=meta["tied"], init_split=meta["init_split"])
    m.load_state_dict(P, strict=False)
    with torch.no_grad():
        m.decoder.out.bias[EOS] += eos_bias
    g = torch.Generator().manual_seed(4)
    src = torch.zeros(len(LENS), max(LENS), dtype=torch.long)
    for b, n in enumerate(LENS):
        src[b, :n] = torch.randint(4, Vs, (n,), generator=g)
    im = torch.randn(len(LENS), I, generator=g).abs()
    return m.cuda().eval(), src.cuda(), im.cuda()


@pytest.fixture(scope="module")
def subject():
    return golden_model()


def draw(obj, src, im, seed=1234, **kw):
    from vagnmt_hip.sampling import Generator
    return obj.beamsearch_stochastic(src, LENS, im, n_samples=N, max_length=ML, generator=Generator(seed), **kw)


def same(a, b):
    return a.hyps == b.hyps and all(torch.equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))


def test_public_call(subject):
    m, src, im = subject
    B = len(LENS)
    m.decode_graph = True
    s = draw(m, src, im)
    assert len(s.hyps) == B and all(len(h) == N for h in s.hyps)
    for t in (s.logp, s.score, s.gumbel, s.log_weight):
        assert t.shape == (B, N) and t.dtype == torch.float32 and t.is_cuda
    for b in range(B):
        assert len({tuple(h) for h in s.hyps[b]}) == N, (b, s.hyps[b])      # pairwise distinct
    g = s.gumbel.cpu()
    assert bool((g[:, 1:] <= g[:, :-1]).all())
    lw = s.log_weight.cpu()
    assert bool(torch.isneginf(lw[:, -1]).all()) and bool(torch.isfinite(lw[:, :-1]).all())
    assert bool((lw[:, :-1] >= s.logp.cpu()[:, :-1] - 1e-6).all())
    # logp against forced decoding: the hypotheses that ended before max_length (the finish forces EOS into the last row) and hold
    # no padding word (which forced decoding feeds on but does not score); relative 2e-4, the n-best search-vs-scoring bound
    flat = [list(h) for sent in s.hyps for h in sent]
    lens_n = [n for n in LENS for _ in range(N)]
    forced = m.score_translations(src.repeat_interleave(N, 0), lens_n, flat, im.repeat_interleave(N, 0))
    f_lp, f_sc = forced.logp.cpu().numpy().reshape(B, N), forced.score.cpu().numpy().reshape(B, N)
    lp, sc = s.logp.cpu().numpy(), s.score.cpu().numpy()
    idx = [(b, r) for b in range(B) for r in range(N) if len(s.hyps[b][r]) < ML - 1 and 0 not in s.hyps[b][r]]
    assert len(idx) >= B * N // 2, len(idx)
    rel = max(max(abs(float(f_lp[b, r]) - float(lp[b, r])) / max(1.0, abs(float(lp[b, r]))),
                  abs(float(f_sc[b, r]) - float(sc[b, r])) / max(1.0, abs(float(sc[b, r])))) for b, r in idx)
    print("%d finished hypotheses, forced vs search logp / score: max rel err %.3e" % (len(idx), rel))
    assert rel <= 2e-4, rel


def test_determinism_modes_and_ensemble(subject):
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Generator
    m, src, im = subject
    ens = Ensemble([m, m])
    res = {}
    for graph in (True, False):
        m.decode_graph = ens.decode_graph = graph
        a = draw(m, src, im)
        assert same(a, draw(m, src, im)), graph                             # the same generator state: the same bits
        other = draw(m, src, im, seed=99)
        assert other.hyps != a.hyps and not torch.equal(bits(other.gumbel), bits(a.gumbel)), graph
        gen = Generator(1234)
        st = gen.get_state()
        assert same(a, m.beamsearch_stochastic(src, LENS, im, n_samples=N, max_length=ML, generator=gen))
        assert gen.get_state() == [st[0], st[1] + 1]                        # advanced once, as sample_decode does
        second = m.beamsearch_stochastic(src, LENS, im, n_samples=N, max_length=ML, generator=gen)
        assert second.hyps != a.hyps
        assert same(a, draw(ens, src, im)), graph                           # two copies of the model: the model bit for bit
        # the options reach the expansion: with avoid_double no hypothesis repeats a word
        nd = draw(m, src, im, avoid_double=True)
        assert all(x != y for sent in nd.hyps for h in sent for x, y in zip(h, h[1:])), graph
        res[graph] = a
    assert same(res[True], res[False])                                      # eager and graph mode agree bit for bit
    m.decode_graph = True


def test_mbr_decode_without_replacement(subject):
    from vagnmt_hip.mbr import mbr_select
    from vagnmt_hip.sampling import Generator
    m, src, im = subject
    B = len(LENS)
    for graph in (True, False):
        m.decode_graph = graph
        gen = Generator(31)
        st = gen.get_state()
        s = m.beamsearch_stochastic(src, LENS, im, n_samples=N, max_length=ML, generator=gen)
        gen.set_state(st)
        best, sel, drawn = m.mbr_decode(src, LENS, im, n_samples=N, max_length=ML, without_replacement=True, generator=gen)
        assert gen.get_state() == [st[0], st[1] + 1] and same(s, drawn), graph
        w = torch.exp(s.log_weight)
        want = mbr_select(s.hyps, weights=w)
        assert torch.equal(sel.index, want.index) and torch.equal(bits(sel.expected), bits(want.expected)), graph
        assert best == sel.best == [s.hyps[b][int(sel.index[b])] for b in range(B)], graph
        assert sel.expected.shape == (B, N)
        # the weights matter, and only up to their scale
        assert torch.equal(bits(mbr_select(s.hyps, weights=4.0 * w).expected), bits(want.expected))
        assert not torch.equal(bits(mbr_select(s.hyps).expected), bits(want.expected))
        # with the beam's list: the candidates that follow the samples are beamsearch_nbest's, the references stay the samples
        gen.set_state(st)
        best3, sel3, _ = m.mbr_decode(src, LENS, im, n_samples=N, max_length=ML, without_replacement=True, beam_size=3,
                                      generator=gen)
        beams = m.beamsearch_nbest(src, LENS, im, 3, 3, ML)[0]
        cands = [s.hyps[b] + beams[b] for b in range(B)]
        want3 = mbr_select(cands, refs=s.hyps, weights=w)
        assert torch.equal(sel3.index, want3.index) and torch.equal(bits(sel3.expected), bits(want3.expected)), graph
        assert best3 == [cands[b][int(sel3.index[b])] for b in range(B)]
        with pytest.raises(ValueError, match="without_replacement"):
            m.mbr_decode(src, LENS, im, n_samples=N, max_length=ML, without_replacement=True, temperature=0.9, generator=gen)
    m.decode_graph = True
