"""GPU: minimum-Bayes-risk selection (vag_mbr_select, vagnmt_hip.mbr.mbr_select, mbr_decode on the models and the Ensemble)
against the float64 restatement of include/vag_nmt.h's definitions (tests/mbr_ref.py) and the fixture recorded from the
reference's bleu.py (tests/golden/mbr_bleu.npz).

1. exact counts: `matches` equals the restatement integer for integer -- L in {1, 3, 4, 63, 64, 65, 80} (the kernel walks a row
   in chunks of 64 positions and reads references four tokens at a time), N in {1, 2, 5, 33, 64} (four waves split the
   references), B in {1, 3}, Lh != Lr, vocabularies of 2, 6 and 30 words; rows that are empty, hold no EOS, hold a drawn 0, and
   carry copies of their own n-grams after the EOS; symmetry when the candidates are their own references;
2. utilities: util and expected within 1e-5 absolute of the restatement for both utilities (values in [0, 1]; an fp32
   evaluation of the formulas is within 1.5e-7 of float64, logf / expf within a few ulp: a margin of more than 10x) and of the
   golden BLEU; util[b, i, i] == 1.0 exactly for non-empty rows under "bleu"; util == 0 exactly for an empty candidate;
3. selection: best is the first arg-max of the returned expected, bitwise; duplicated rows have bitwise equal expected and the
   lower index wins; the float64 expected utility of best[b] is within 2e-5 of the float64 maximum;
4. weights: used as given at the ABI; a zero weight removes a reference; non-uniform weights; refs given as a copy of hyps is
   refs = None bit for bit;
5. determinism and containment: two calls agree bitwise; outputs allocated with a guard margin keep it (every call of this file
   goes through the guarded helper); the NULL matches / util variants give the same expected and best;
6. mbr_decode on a tiny golden model and a 3-member Ensemble, eager and graph mode."""
import functools
import os

import numpy as np
import pytest
import torch

import mbr_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

EOS = 3
GUARD = 64
LS = [1, 3, 4, 63, 64, 65, 80]
NS = [(1, 3), (2, 3), (5, 3), (33, 1), (64, 1), (2, 1)]                          # (N, B): every N, both B
VOCABS = [2, 6, 30]


# ------------------------------------------------------------------------------------------------------------------
# rows, the guarded call, the shared references
# ------------------------------------------------------------------------------------------------------------------
def make_rows(seed, B, N, L, V):
    """(B, N, L) int64 rows of words 4 .. 4+V-1.  By (b N + i) mod 7: 0 an EOS at a random position, or none; 1 no EOS; 2 empty
    (EOS first); 3 a drawn padding word 0 inside the span; 4 one word repeated ("a a a a"); 5 the same word twice ("a a");
    6 a short span.  After an EOS: copies of the span's own beginning (its n-grams again), a random tail, further EOS."""
    g = np.random.default_rng(seed)
    x = g.integers(4, 4 + V, size=(B, N, L)).astype(np.int64)
    for b in range(B):
        for i in range(N):
            kind = (b * N + i) % 7
            e = int(g.integers(0, L + 1))                                        # the EOS position (L: none)
            if kind == 1:
                e = L
            elif kind == 2:
                e = 0
            elif kind == 3 and L > 1:
                e = max(e, 2)
                x[b, i, int(g.integers(0, min(e, L)))] = 0
            elif kind == 4:
                x[b, i] = 4
                e = min(4, L)
            elif kind == 5:
                x[b, i] = 4
                e = min(2, L)
            elif kind == 6:
                e = min(e, 5)
            if e < L:
                x[b, i, e] = EOS
                tail = L - e - 1
                if tail > 0:
                    x[b, i, e + 1:] = np.resize(x[b, i, :max(e, 1)], tail)       # in-span n-grams after the EOS
                    if tail > 3:
                        x[b, i, e + 1 + int(g.integers(0, tail))] = EOS
    return x


def select(hyps, refs=None, weights=None, utility=0, want_m=True, want_u=True):
    """vag_mbr_select at the ABI on numpy / tensor inputs, every output inside a guard margin that must come back untouched.
    Returns (matches or None, util or None, expected, best) as CPU tensors."""
    from vagnmt_hip._lib import call, ptr, stream
    h = torch.as_tensor(hyps).cuda().contiguous()
    r = None if refs is None else torch.as_tensor(refs).cuda().contiguous()
    w = None if weights is None else torch.as_tensor(weights, dtype=torch.float32).cuda().contiguous()
    B, Nh, Lh = h.shape
    Nr, Lr = (Nh, Lh) if r is None else r.shape[1:]

    def guarded(n, dtype, fill):
        return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")

    bufs = {"m": guarded(B * Nh * Nr * 4, torch.int32, -77) if want_m else None,
            "u": guarded(B * Nh * Nr, torch.float32, -7.0) if want_u else None,
            "e": guarded(B * Nh, torch.float32, -7.0), "b": guarded(B, torch.int64, -77)}
    inner = {k: (None if v is None else v[GUARD:-GUARD]) for k, v in bufs.items()}
    call("vag_mbr_select", ptr(h, torch.int64), ptr(r, torch.int64), ptr(w), B, Nh, Lh, Nr, Lr, utility,
         None if inner["m"] is None else inner["m"].data_ptr(), None if inner["u"] is None else inner["u"].data_ptr(),
         inner["e"].data_ptr(), inner["b"].data_ptr(), stream())
    torch.cuda.synchronize()
    for k, v in bufs.items():
        if v is not None:
            fill = -77 if v.dtype in (torch.int32, torch.int64) else -7.0
            assert bool((v[:GUARD] == fill).all()) and bool((v[-GUARD:] == fill).all()), "guard of %s overwritten" % k
    m = None if inner["m"] is None else inner["m"].reshape(B, Nh, Nr, 4).cpu()
    u = None if inner["u"] is None else inner["u"].reshape(B, Nh, Nr).cpu()
    return m, u, inner["e"].reshape(B, Nh).cpu(), inner["b"].cpu()


@functools.lru_cache(maxsize=None)
def case(L, V, N, B):
    """One shape's rows and their float64 reference, computed once and shared (read only)."""
    x = make_rows(1000 * L + 10 * V + N, B, N, L, V)
    m, lh, lr = R.pairwise(x)
    return x, m, lh, lr, {name: R.utilities(m, lh, lr, name) for name in R.UTILITY}


def bits(t):
    return t.contiguous().view(torch.int32)


def first_argmax(e):
    return (e == e.max(1, keepdim=True)[0]).int().argmax(1)


# ------------------------------------------------------------------------------------------------------------------
# 1, 2, 3 on the grid of shapes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("L", LS)
def test_counts_utilities_and_selection(L, V):
    worst = {"util": 0.0, "expected": 0.0, "best": 0.0}
    clipped = 0
    for N, B in NS:
        x, m_ref, lh, lr, u_ref = case(L, V, N, B)
        what = "L=%d V=%d N=%d B=%d" % (L, V, N, B)
        for name, uid in (("bleu", 0), ("ngram_f", 1)):
            m, u, e, best = select(x, utility=uid)
            assert np.array_equal(m.numpy().astype(np.int64), m_ref), what                      # 1: integer for integer
            assert torch.equal(m, m.transpose(1, 2)), what                                     # symmetric
            ud = u.double().numpy()
            assert ud.min() >= 0.0 and ud.max() <= 1.0 + 1e-6, what
            e_ref = R.expected(u_ref[name])
            worst["util"] = max(worst["util"], float(np.abs(ud - u_ref[name]).max()))
            worst["expected"] = max(worst["expected"], float(np.abs(e.double().numpy() - e_ref).max()))
            empty = torch.from_numpy(lh == 0)
            assert bool((u[empty] == 0.0).all()), what                                         # an empty candidate: exactly 0
            if name == "bleu":
                diag = torch.diagonal(u, dim1=1, dim2=2)
                assert bool((diag[~empty] == 1.0).all()), what                                 # a row against itself: exactly 1
            assert torch.equal(best, first_argmax(e)), what                                    # 3: the first arg-max, bitwise
            picked = e_ref[np.arange(B), best.numpy()]
            worst["best"] = max(worst["best"], float((e_ref.max(1) - picked).max()))
        # clipping occurred: the candidate's matching unigram positions exceed the clipped count somewhere
        for b in range(B):
            spans = [R.span(r) for r in x[b]]
            clipped += sum(sum(t in r for t in h) > m_ref[b, i, j, 0] for i, h in enumerate(spans) for j, r in enumerate(spans))
    print("L=%d V=%d: max abs err util %.2e expected %.2e, fp64 regret of best %.2e, clipped pairs %d"
          % (L, V, worst["util"], worst["expected"], worst["best"], clipped))
    assert worst["util"] <= 1e-5 and worst["expected"] <= 1e-5, worst
    assert worst["best"] <= 2e-5, worst
    if L >= 3 and V <= 6:
        assert clipped > 0


def test_hand_cases_and_other_reference_shape():
    a = 9
    # "a a a a" against "a a": 2 unigrams and 1 bigram survive the clip, either way round
    x = np.array([[[a, a, a, a, EOS], [a, a, EOS, a, a]]], dtype=np.int64)
    m, u, e, best = select(x)
    assert m[0, 0, 1].tolist() == [2, 1, 0, 0] and m[0, 1, 0].tolist() == [2, 1, 0, 0]
    assert m[0, 0, 0].tolist() == [4, 3, 2, 1] and m[0, 1, 1].tolist() == [2, 1, 0, 0]
    # Lh != Lr: 7 against 65, 5 candidates against 33 references, three sentences
    h = make_rows(5, 3, 5, 7, 6)
    r = make_rows(6, 3, 33, 65, 6)
    m_ref, lh, lr = R.pairwise(h, r)
    for name, uid in (("bleu", 0), ("ngram_f", 1)):
        m, u, e, best = select(h, r, utility=uid)
        assert np.array_equal(m.numpy().astype(np.int64), m_ref), name
        u_ref = R.utilities(m_ref, lh, lr, name)
        assert float(np.abs(u.double().numpy() - u_ref).max()) <= 1e-5, name
        assert float(np.abs(e.double().numpy() - R.expected(u_ref)).max()) <= 1e-5, name
        assert torch.equal(best, first_argmax(e)), name
    # and the other way round (65 against 7)
    m2 = select(r, h)[0]
    assert torch.equal(m2, m.transpose(1, 2))


def test_golden_bleu():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mbr_bleu.npz"))
    pairs, worst = 0, 0.0
    for s in range(int(z["n_sets"])):
        tok, m_gold, u_gold = z["tok%d" % s], z["m%d" % s], z["bleu%d" % s]
        m, u, _, _ = select(tok)
        have = ~np.isnan(u_gold)
        assert np.array_equal(m.numpy()[have], m_gold[have])
        worst = max(worst, float(np.abs(u.double().numpy() - u_gold)[have].max()))
        pairs += int(have.sum())
    print("golden BLEU: %d pairs, max abs err %.2e" % (pairs, worst))
    assert pairs > 200 and worst <= 1e-5


def test_duplicates_and_ties():
    g = np.random.default_rng(3)
    # all rows identical: every expected utility is the same number, the lowest index wins
    x = np.repeat(make_rows(1, 2, 1, 12, 6), 5, axis=1)
    for uid in (0, 1):
        _, _, e, best = select(x, utility=uid)
        assert bool((bits(e) == bits(e)[:, :1]).all()) and best.tolist() == [0, 0]
    # rows 1 and 3 are the same sentence and the consensus of the set; rows 0, 2, 4 share little with anything
    x = g.integers(4, 34, size=(3, 5, 14)).astype(np.int64)
    x[:, :, 10] = EOS
    x[:, 3] = x[:, 1]
    x[:, 4, :5] = x[:, 1, :5]                                                    # a partial copy: second best
    m, lh, lr = R.pairwise(x)
    for name, uid in (("bleu", 0), ("ngram_f", 1)):
        e_ref = R.expected(R.utilities(m, lh, lr, name))
        others = np.delete(e_ref, [1, 3], axis=1).max(1)
        assert float((e_ref[:, 1] - others).min()) > 1e-3                        # by the float64 reference: a clear winner
        _, _, e, best = select(x, utility=uid)
        assert torch.equal(bits(e[:, 1]), bits(e[:, 3])) and best.tolist() == [1, 1, 1], name
        assert torch.equal(best, first_argmax(e))


# ------------------------------------------------------------------------------------------------------------------
# 4. weights
# ------------------------------------------------------------------------------------------------------------------
def test_weights():
    from vagnmt_hip.mbr import mbr_select
    B, N, L, V = 3, 5, 12, 6
    x, m_ref, lh, lr, u_ref = case(L, V, N, B)
    g = np.random.default_rng(8)
    for name, uid in (("bleu", 0), ("ngram_f", 1)):
        # used as given: weights that sum to 0.7, not to 1
        w = g.random((B, N))
        w = (0.7 * w / w.sum(1, keepdims=True)).astype(np.float32)
        _, u, e, best = select(x, weights=w, utility=uid)
        assert float(np.abs(e.double().numpy() - R.expected(u_ref[name], w)).max()) <= 1e-5, name
        assert float(np.abs(e.double().numpy() - R.expected(u_ref[name], w / 0.7)).max()) > 1e-3       # (normalising would show)
        assert torch.equal(best, first_argmax(e))
        # a zero weight removes a reference: the call with that reference deleted
        w0 = w.copy()
        w0[:, 2] = 0.0
        _, _, e0, b0 = select(x, x, w0, utility=uid)
        keep = [0, 1, 3, 4]
        _, _, e1, b1 = select(x, x[:, keep], w0[:, keep], utility=uid)
        assert float((e0 - e1).abs().max()) <= 1e-5 and torch.equal(b0, first_argmax(e0)) and torch.equal(b1, first_argmax(e1)), name
        # refs given as a copy of hyps: refs = None, bit for bit
        a = select(x, utility=uid)
        c = select(x, x.copy(), utility=uid)
        assert torch.equal(a[0], c[0]) and torch.equal(bits(a[1]), bits(c[1])) and torch.equal(bits(a[2]), bits(c[2])) and \
            torch.equal(a[3], c[3]), name
        # the Python entry normalises per sentence: non-uniform weights against the restatement
        wt = torch.tensor([[3.0, 0.0, 1.0, 0.5, 0.5]] * B, device="cuda")
        sel, (u2, m2) = mbr_select(torch.from_numpy(x).cuda(), weights=wt, utility=name, return_utilities=True)
        wn = (wt / wt.sum(1, keepdim=True)).cpu().numpy()
        assert float(np.abs(sel.expected.cpu().double().numpy() - R.expected(u_ref[name], wn)).max()) <= 1e-5, name
        assert np.array_equal(m2.cpu().numpy().astype(np.int64), m_ref)
        assert torch.equal(sel.index.cpu(), first_argmax(sel.expected.cpu()))
        assert sel.best == [R.span(x[b, int(sel.index[b])]) for b in range(B)]
    with pytest.raises(ValueError, match="weights"):
        mbr_select(torch.from_numpy(x).cuda(), weights=torch.zeros(B, N, device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        mbr_select(torch.from_numpy(x).cuda(), weights=-torch.ones(B, N, device="cuda"))


def test_python_entry_on_lists_and_checks():
    from vagnmt_hip.mbr import mbr_select, pack
    x, m_ref, lh, lr, u_ref = case(12, 6, 5, 3)
    lists = [[R.span(r) for r in sent] for sent in x]
    a = mbr_select(torch.from_numpy(x).cuda())
    b, (u, m) = mbr_select(lists, return_utilities=True)
    assert torch.equal(a.index, b.index) and torch.equal(bits(a.expected), bits(b.expected)) and a.best == b.best
    assert np.array_equal(m.cpu().numpy().astype(np.int64), m_ref)
    c = mbr_select(lists, refs=[sent[:3] for sent in lists], utility="ngram_f")
    m3, lh3, lr3 = R.pairwise(x, x[:, :3])
    assert float(np.abs(c.expected.cpu().double().numpy() - R.expected(R.utilities(m3, lh3, lr3, "ngram_f"))).max()) <= 1e-5
    xc = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="int64"):
        mbr_select(xc.int())
    with pytest.raises(ValueError, match="2\\^31"):
        mbr_select(torch.where(xc == 5, torch.full_like(xc, 1 << 31), xc))
    with pytest.raises(ValueError, match="2\\^31"):
        mbr_select(torch.where(xc == 5, torch.full_like(xc, -1), xc))
    with pytest.raises(ValueError, match="unsupported shape"):
        mbr_select(torch.zeros(1, 2, 513, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="B = 3"):
        mbr_select(xc, refs=xc[:2])
    assert pack(lists).shape[2] <= 13


# ------------------------------------------------------------------------------------------------------------------
# 5. determinism and containment
# ------------------------------------------------------------------------------------------------------------------
def test_determinism_and_null_outputs():
    for L, V, N, B in ((65, 2, 33, 1), (12, 6, 5, 3)):
        x = case(L, V, N, B)[0]
        for uid in (0, 1):
            a = select(x, utility=uid)
            b = select(x, utility=uid)
            assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(bits(a[2]), bits(b[2])) and \
                torch.equal(a[3], b[3])
            for want_m, want_u in ((False, True), (True, False), (False, False)):
                c = select(x, utility=uid, want_m=want_m, want_u=want_u)
                assert (c[0] is None) == (not want_m) and (c[1] is None) == (not want_u)
                assert torch.equal(bits(a[2]), bits(c[2])) and torch.equal(a[3], c[3])


# ------------------------------------------------------------------------------------------------------------------
# 6. mbr_decode
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


def same(a, b):
    return a.hyps == b.hyps and torch.equal(a.token_logp, b.token_logp) and torch.equal(a.logp, b.logp) and \
        torch.equal(a.score, b.score)


def subject(name):
    """(object, src, lengths, im, nbest call, beam call) of "text", "mm" (the multimodal model) or "ens3" (three members)."""
    from vagnmt_hip.ensemble import Ensemble
    if name == "text":
        t, src, lens, _ = golden_model("text_tied_s0_f32", eos_bias=1.5)
        return (t, src, lens, None, lambda k, ml: t.beamsearch_nbest(src, lens, k, k, ml),
                lambda k, ml: t.beamsearch_decode(src, lens, k, ml))
    m, src, lens, im = golden_model("mm_dot_tied_s0_f32", eos_bias=1.5)
    obj = m
    if name == "ens3":
        obj = Ensemble([m, golden_model("text_tied_s0_f32", eos_bias=1.5)[0], golden_model("mm_dot_tied_s0_f32", eos_bias=0.5)[0]])
    return (obj, src, lens, im, lambda k, ml: obj.beamsearch_nbest(src, lens, im, k, k, ml),
            lambda k, ml: obj.beamsearch_decode(src, lens, im, k, ml))


@pytest.mark.parametrize("name", ["text", "mm", "ens3"])
def test_mbr_decode(name):
    from vagnmt_hip.mbr import mbr_select
    from vagnmt_hip.sampling import Generator
    ML, n = 10, 6
    kw = dict(n_samples=n, max_length=ML, temperature=0.9, top_k=10, top_p=0.95)
    obj, src, lens, im, nbest, beam = subject(name)
    B = src.shape[0]
    res = {}
    for graph in (True, False):
        obj.decode_graph = graph
        for m in getattr(obj, "models", []):
            m.decode_graph = graph
        what = "%s graph=%s" % (name, graph)
        before = (beam(3, ML), nbest(3, ML), obj.sample_decode(src, lens, im, generator=Generator(5), **kw))
        for utility in ("bleu", "ngram_f"):
            gen = Generator(77)
            st = gen.get_state()
            drawn = obj.sample_decode(src, lens, im, generator=gen, **kw)
            after_one = gen.get_state()
            assert after_one == [st[0], st[1] + 1]
            gen.set_state(st)
            best, sel, smp = obj.mbr_decode(src, lens, im, utility=utility, generator=gen, **kw)
            assert gen.get_state() == after_one, what                        # advanced exactly as one sample_decode
            assert same(drawn, smp), what
            want = mbr_select(drawn.hyps, utility=utility)                   # mbr_select on what sample_decode returned
            assert torch.equal(sel.index, want.index) and best == want.best == sel.best, what
            # (the lists are packed to their own width, the history is max_length wide: the same spans, the same numbers)
            assert torch.equal(bits(sel.expected), bits(want.expected)), what
            assert sel.expected.shape == (B, n) and best == [drawn.hyps[b][int(sel.index[b])] for b in range(B)]
            res[(graph, utility)] = (best, sel.index.cpu(), sel.expected.cpu())
            # with the beam's list: n + 3 candidates, the last three are beamsearch_nbest's, the references stay the samples
            gen.set_state(st)
            best3, sel3, smp3 = obj.mbr_decode(src, lens, im, utility=utility, beam_size=3, generator=gen, **kw)
            assert gen.get_state() == after_one and same(drawn, smp3), what
            assert sel3.expected.shape == (B, n + 3), what
            beams = nbest(3, ML)[0]
            cands = [drawn.hyps[b] + beams[b] for b in range(B)]
            want3 = mbr_select(cands, refs=drawn.hyps, utility=utility)
            assert torch.equal(sel3.index, want3.index) and torch.equal(bits(sel3.expected), bits(want3.expected)), what
            assert best3 == [cands[b][int(sel3.index[b])] for b in range(B)] == sel3.best, what
            assert torch.equal(bits(sel3.expected[:, :n]), bits(sel.expected)), what
        # n_samples = 1: the sample itself
        gen = Generator(3)
        one = obj.sample_decode(src, lens, im, n_samples=1, max_length=ML, generator=gen)
        best1, sel1, _ = obj.mbr_decode(src, lens, im, n_samples=1, max_length=ML, generator=Generator(3))
        assert best1 == [h[0] for h in one.hyps] and sel1.index.tolist() == [0] * B, what
        # the other decode paths give what they gave before
        after = (beam(3, ML), nbest(3, ML), obj.sample_decode(src, lens, im, generator=Generator(5), **kw))
        assert [list(map(int, h)) for h in before[0]] == [list(map(int, h)) for h in after[0]], what
        assert before[1][0] == after[1][0] and torch.equal(bits(before[1][1]), bits(after[1][1])), what
        assert same(before[2], after[2]), what
    for utility in ("bleu", "ngram_f"):                                      # graph and eager mode agree
        a, b = res[(True, utility)], res[(False, utility)]
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(bits(a[2]), bits(b[2])), name


def test_mbr_decode_argument_checks():
    from vagnmt_hip.sampling import Generator
    obj, src, lens, im, _, _ = subject("mm")
    gen = Generator(1)
    st = gen.get_state()
    with pytest.raises(ValueError, match="beam_size"):
        obj.mbr_decode(src, lens, im, n_samples=2, max_length=5, beam_size=65, generator=gen)
    with pytest.raises(ValueError, match="utility"):
        obj.mbr_decode(src, lens, im, n_samples=2, max_length=5, utility="chrf", generator=gen)
    with pytest.raises(ValueError, match="unsupported shape"):
        obj.mbr_decode(src, lens, im, n_samples=2, max_length=513, generator=gen)
    with pytest.raises(ValueError, match="im_var"):
        obj.mbr_decode(src, lens, None, n_samples=2, max_length=5, generator=gen)
    assert gen.get_state() == st                                                 # nothing was drawn
