"""GPU: constrained beam search (vagnmt_hip.constrain; include/vag_nmt.h: vag_beam_constrain).

1. the mask kernel against tests/constrain_ref.py bit for bit at every step of a random history -- forced rows, one-word and
   longer bans, n-gram bans, finished rows, NaN in the columns past V that must stay -- for one and three members; the empty
   set, the device-index form, the ABI's argument errors, a whole search on a table "model";
2. the models and Ensemble: no constraints is beamsearch_nbest, prefixes, bans, no-repeat bigrams, scores against forced scores,
   a search driven from the test with the NumPy mask, graph against eager mode, the static buffers of the graph entries."""
import ctypes as C

import numpy as np
import pytest
import torch

import constrain_ref as R

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


def pp(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def dptr(t):
    return None if t is None else t.data_ptr()


class Case:
    """One random history with its constraints, on the host and on the device."""

    def __init__(self, B, k, V, ldl, max_len, seed, M=3):
        rng = np.random.default_rng(seed)
        self.B, self.k, self.V, self.ldl, self.max_len = B, k, V, ldl, max_len
        self.beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
        self.beam[:max_len] = rng.integers(3, 7, size=(max_len, B, k))           # words {3 = EOS, 4, 5, 6}
        self.beam[max_len:] = rng.integers(0, k, size=(max_len, B, k))           # back-pointers anywhere in [0, k)
        self.prefix = np.zeros((B, 3), dtype=np.int64)
        self.prefix[0] = [4, 5, 6]
        self.prefix[1, 0] = 6
        self.phrases = np.zeros((6, R.MAX_LEN), dtype=np.int64)
        self.phrases[0, :1] = [5]
        self.phrases[1, :2] = [4, 6]
        self.phrases[2, :3] = [6, 5, 4]                                         # (row 3 stays empty: ignored)
        self.phrases[4, :4] = [4, 5, 6, 4]
        self.phrases[5, :2] = [5, 5]
        self.sent = np.array([B - 1, -1, -1, -1, -1, 0], dtype=np.int32)        # the one-word ban and (5 5) bound to a sentence
        self.rows = []
        for _ in range(M):
            a = np.full((B * k, ldl), np.nan, dtype=np.float32)                  # NaN past V: must stay
            a[:, :V] = rng.standard_normal((B * k, V)).astype(np.float32)
            self.rows.append(a)

    def upload(self):
        self.d_beam, self.d_prefix = dev(self.beam), dev(self.prefix)
        self.d_phrases, self.d_sent = dev(self.phrases), dev(self.sent)
        return self

    def n_rows(self, di):
        return self.B if di == 0 else self.B * self.k

    def want(self, di, M, ngram, counts=None):
        N = self.n_rows(di)
        return R.mask([a[:N] for a in self.rows[:M]], self.beam, di, self.max_len, self.B, self.k, self.V, self.prefix,
                      self.phrases, self.sent, ngram, counts)

    def run(self, di, M, ngram, di_state=None, full=True):
        """The kernel on fresh copies of the rows; full=False: the empty constraint set.  Returns (rc, M arrays)."""
        N = self.n_rows(di)
        logp = [dev(a[:N]) for a in self.rows[:M]]
        con = (dptr(self.d_prefix), 3, dptr(self.d_phrases), dptr(self.d_sent), 6, ngram) if full else (None, 0, None, None, 0, 0)
        if di_state is None:
            rc = L().vag_beam_constrain(pp(logp), p64([self.ldl] * M), M, self.d_beam.data_ptr(), di, self.max_len, self.B, self.k,
                                        self.V, *con, stream())
        else:
            rc = L().vag_beam_constrain_dev(pp(logp), p64([self.ldl] * M), M, self.d_beam.data_ptr(), di_state.data_ptr(),
                                            self.max_len, self.B, self.k, self.V, *con, stream())
        return rc, [t.cpu().numpy() for t in logp]


# (B, k, V, ldl, max_len, seed): a row shorter than a workgroup; a row that takes the block-stride loop, unaligned row starts.
# The seeds are chosen on the host, with the reference alone, so that every branch fires in at least 3 rows (asserted below).
SHAPES = [(2, 3, 37, 40, 9, 0), (3, 5, 2500, 2501, 12, 0)]
_cases = {}


def case(shape):
    if shape not in _cases:
        _cases[shape] = Case(*shape).upload()
    return _cases[shape]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_matches_reference_bit_for_bit(shape, M):
    c = case(shape)
    for ngram in (0, 1, 2, 3):
        counts = R.new_counts()
        for di in range(c.max_len):
            want = c.want(di, M, ngram, counts)
            rc, got = c.run(di, M, ngram)
            assert rc == 0
            for m in range(M):
                assert got[m].tobytes() == want[m].tobytes(), (shape, M, ngram, di, m)
                assert np.isnan(got[m][:, c.V:]).all()
        print("branch rows", shape, "ngram", ngram, counts)
        for name in R.BRANCHES:
            assert counts[name] >= 3, (shape, ngram, name, counts)
        if ngram:
            assert counts["ngram"][ngram] >= 3, (shape, ngram, counts)


def test_empty_constraint_set_changes_nothing():
    c = case(SHAPES[0])
    for di in (0, 4):
        rc, got = c.run(di, 3, 0, full=False)
        assert rc == 0
        for m in range(3):
            assert got[m].tobytes() == c.rows[m][:c.n_rows(di)].tobytes()


def test_device_index_form():
    for shape in SHAPES:
        c = case(shape)
        for di in (0, 1, c.max_len // 2, c.max_len - 1):
            state = torch.tensor([di, 0], dtype=I32, device="cuda")
            rc, got = c.run(di, 3, 2, di_state=state)
            assert rc == 0 and state.cpu().tolist() == [di, 0]
            rc, want = c.run(di, 3, 2)
            assert rc == 0
            for m in range(3):
                assert got[m].tobytes() == want[m].tobytes(), (shape, di, m)
            assert any(g.tobytes() != a[:c.n_rows(di)].tobytes() for g, a in zip(got, c.rows))       # (it did write)
        state = torch.tensor([c.max_len, 0], dtype=I32, device="cuda")                               # past the end: nothing
        rc, got = c.run(1, 3, 2, di_state=state)
        assert rc == 0 and state.cpu().tolist() == [c.max_len, 0]
        for m in range(3):
            assert got[m].tobytes() == c.rows[m].tobytes()


def test_abi_argument_errors_launch_nothing():
    B, k, V, ldl, max_len = 2, 3, 37, 40, 9
    c = case(SHAPES[0])
    logp = [torch.full((B * k, ldl), 0.25, device="cuda") for _ in range(2)]
    state = torch.tensor([1, 0], dtype=I32, device="cuda")
    big_beam = torch.zeros(2 * 1025 * B * k, dtype=I64, device="cuda")                                # (for max_len = 1025)

    def call(M=2, lp="ok", ldl_=(ldl, ldl), beam="ok", di=1, max_len_=max_len, B_=B, k_=k, V_=V, prefix="ok", Lp=3, phrases="ok",
             sent="ok", P=6, ngram=2, dev_form=False, state_="ok"):
        lpp = {"ok": pp(logp), None: None, "entry": (C.c_void_p * 2)(logp[0].data_ptr(), None)}[lp]
        bm = {"ok": c.d_beam.data_ptr(), None: None, "big": big_beam.data_ptr()}[beam]
        con = (c.d_prefix.data_ptr() if prefix == "ok" else None, Lp, c.d_phrases.data_ptr() if phrases == "ok" else None,
               c.d_sent.data_ptr() if sent == "ok" else None, P, ngram)
        if dev_form:
            rc = L().vag_beam_constrain_dev(lpp, p64(list(ldl_)) if ldl_ else None, M, bm, state.data_ptr() if state_ == "ok" else None,
                                            max_len_, B_, k_, V_, *con, stream())
        else:
            rc = L().vag_beam_constrain(lpp, p64(list(ldl_)) if ldl_ else None, M, bm, di, max_len_, B_, k_, V_, *con, stream())
        torch.cuda.synchronize()
        return rc, all(bool((t == 0.25).all()) for t in logp)
    bad = [dict(lp=None), dict(ldl_=None), dict(lp="entry"), dict(M=0), dict(M=9), dict(ldl_=(ldl, V - 1)), dict(beam=None),
           dict(B_=0), dict(k_=0), dict(V_=0), dict(max_len_=0), dict(k_=65), dict(max_len_=1025, beam="big"), dict(di=-1),
           dict(di=max_len), dict(dev_form=True, state_=None), dict(Lp=-1), dict(prefix=None), dict(P=-1), dict(P=257),
           dict(phrases=None), dict(sent=None), dict(ngram=-1), dict(ngram=9)]
    for kw in bad:
        assert call(**kw) == (-22, True), kw
    # an empty set is valid whatever its pointers are, and launches nothing; then the good calls go through
    assert call(prefix=None, Lp=0, phrases=None, sent=None, P=0, ngram=0) == (0, True)
    assert call(dev_form=True, prefix=None, Lp=0, phrases=None, sent=None, P=0, ngram=0) == (0, True)
    assert call() == (0, False)
    assert call(dev_form=True)[0] == 0 and state.cpu().tolist() == [1, 0]


def test_whole_search_on_a_table_model():
    """The kernel plus vag_beam_ens_step_opt against the reference search: a prefix, two bans and no-repeat bigrams on
    log-probabilities quantised to 1/8 (ties everywhere: the total order decides)."""
    rng = np.random.default_rng(7)
    B, k, V, steps, H = 2, 6, 50, 8, 4
    max_len = steps
    T = (rng.integers(-96, 1, size=(V, V)) / 8.0).astype(np.float32)
    T[:, EOS] += np.float32(1.5)                                         # some hypotheses finish
    Td = dev(T)
    prefix = np.array([[7, 9, 11], [8, 0, 0]], dtype=np.int64)
    phrases = np.zeros((2, R.MAX_LEN), dtype=np.int64)
    free = R.search(lambda tok: T[tok], B, k, V, max_len, steps, prefix)[0]      # the words a prefix-only search takes next:
    phrases[0, :1] = [free[3, 0, 0]]                                             # banned, so that the bans change the result
    phrases[1, :2] = [8, free[1, 1, 0]]
    sent = np.array([-1, 1], dtype=np.int32)
    counts = R.new_counts()
    want_beam, want_nll = R.search(lambda tok: T[tok], B, k, V, max_len, steps, prefix, phrases, sent, 2, 0, counts)
    assert not np.array_equal(want_beam, free) and counts["forced"] >= 4 and counts["unigram"] > 0 and counts["multiword"] > 0
    beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
    nll = torch.zeros(B, k, device="cuda")
    n_alive = torch.zeros(1, dtype=I32, device="cuda")
    scratch = torch.empty(L().vag_beam_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
    d_prefix, d_phrases, d_sent = dev(prefix), dev(phrases), dev(sent)
    h = [torch.zeros(B, H, device="cuda")]
    for di in range(steps):
        tok = torch.full((B,), R.SOS, dtype=I64, device="cuda") if di == 0 else beam[di - 1].reshape(-1)
        logp = [Td[tok].contiguous()]
        assert L().vag_beam_constrain(pp(logp), p64([V]), 1, beam.data_ptr(), di, max_len, B, k, V, d_prefix.data_ptr(), 3,
                                      d_phrases.data_ptr(), d_sent.data_ptr(), 2, 2, stream()) == 0
        h_out = [torch.empty(B * k, H, device="cuda")]
        assert L().vag_beam_ens_step_opt(pp(logp), p64([V]), 1, nll.data_ptr(), beam.data_ptr(), di, max_len, pp(h), pp(h_out),
                                         p64([H]), B, k, V, n_alive.data_ptr(), scratch.data_ptr(), 0, stream()) == 0
        h = h_out
    assert np.array_equal(beam.cpu().numpy(), want_beam) and nll.cpu().numpy().tobytes() == want_nll.tobytes()
    live = want_nll > -1e4
    assert live.any()
    for b in range(B):
        for j in np.flatnonzero(live[b]):
            hist = R.history(want_beam, max_len, steps, b, int(j))
            assert hist[:3] == [7, 9, 11] if b == 0 else hist[0] == 8


# ------------------------------------------------------------------------------------------------------------------
# models (small random ones, built as tests/test_gpu_diverse.py builds them)
# ------------------------------------------------------------------------------------------------------------------
VS, VT, IM, ML = 70, 503, 64, 10
LENS = [9, 6, 3]
K = 6


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
    m = make_model(request.param, 21)               # (no EOS bias: every hypothesis of these models runs to max_length)
    src, im = make_inputs()
    return request.param, m, src, (im if request.param == "mm" else None)


def nbest(m, src, im, k=K, n=K, lens=LENS, **kw):
    return m.beamsearch_nbest(src, lens, im, k, n, ML, **kw) if im is not None else m.beamsearch_nbest(src, lens, k, n, ML, **kw)


def con(m, src, im, lens=LENS, **kw):
    kw.setdefault("beam_size", K)
    kw.setdefault("n_best", K)
    kw.setdefault("max_length", ML)
    from vagnmt_hip.ensemble import Ensemble
    if im is not None or isinstance(m, Ensemble):
        return m.beamsearch_constrained(src, lens, im, **kw)
    return m.beamsearch_constrained(src, lens, **kw)


def same(a, b):
    return ints(a.hyps) == ints(b.hyps) and torch.equal(bits(a.scores), bits(b.scores))


def live(c):
    """(b, rank, words) of every returned hypothesis that took no -1e5 step."""
    sc = c.scores.cpu().numpy()
    return [(b, r, [int(t) for t in h]) for b, hs in enumerate(c.hyps) for r, h in enumerate(hs) if sc[b, r] > -1e4]


def contains(h, ph):
    return any(h[i:i + len(ph)] == list(ph) for i in range(len(h) - len(ph) + 1))


def bigrams_repeat(h):
    g = list(zip(h, h[1:]))
    return len(set(g)) < len(g)


def second_best_prefixes(hyps, n=3):
    """The first n words of every sentence's second-best hypothesis."""
    return [[int(t) for t in h[1][:n]] for h in hyps]


def a_constraint_set(hyps):
    """Set A of the cache and mode tests, from the unconstrained lists: a prefix, a ban per sentence, a global bigram."""
    best0 = [int(t) for t in hyps[0][0]]
    assert len(best0) >= 2 and all(len(h[0]) >= 1 for h in hyps)
    return dict(prefix=second_best_prefixes(hyps), banned=[best0[:2], [VT - 1]],
                banned_per_sentence=[[[int(h[0][0])]] for h in hyps], no_repeat_ngram=2)


def test_no_constraints_is_beamsearch_nbest(subject):
    _, m, src, im = subject
    for graph in (True, False):
        m.decode_graph = graph
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(m, src, im, k, n)
            c = con(m, src, im, beam_size=k, n_best=n)
            assert ints(c.hyps) == ints(hyps) and torch.equal(bits(c.scores), bits(sc)), (graph, k)
            c = con(m, src, im, beam_size=k, n_best=n, prefix=[[], [], []], banned=[], banned_per_sentence=[[], [], []])
            assert ints(c.hyps) == ints(hyps) and torch.equal(bits(c.scores), bits(sc)), (graph, k)
    m.decode_graph = True


def test_prefix_is_kept(subject):
    _, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    prefix = second_best_prefixes(hyps)
    assert all(len(p) >= 1 for p in prefix)
    for graph in (True, False):
        m.decode_graph = graph
        for form in (prefix, None):
            if form is None:                                        # the tensor form, padded with 0
                form = torch.zeros(3, 5, dtype=I64)
                for b, p in enumerate(prefix):
                    form[b, :len(p)] = torch.tensor(p)
            c = con(m, src, im, prefix=form)
            got = live(c)
            assert {b for b, r, _ in got if r == 0} == {0, 1, 2}             # the best of every sentence is a live hypothesis
            for b, r, h in got:
                assert h[:len(prefix[b])] == prefix[b], (graph, b, r, h, prefix[b])
            sc = c.scores.cpu()
            assert bool((sc[:, 1:] <= sc[:, :-1]).all())
    m.decode_graph = True


def test_scores_are_forced_scores(subject):
    """Every returned hypothesis that ended before max_length without a -1e5 step scores, forced, what the constrained search
    scored it -- the forced words keep the model's own values: relative 2e-4, the bound of the search-vs-scoring test of
    beamsearch_nbest.  Six sentences: 36 hypotheses to find 8 in."""
    kind, _, _, _ = subject
    m = make_model(kind, 23)
    lens = [9, 8, 6, 5, 3, 2]
    src, im = make_inputs(lens, seed=11)
    im = im if kind == "mm" else None
    B = len(lens)
    idx = []
    for extra in (0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0):
        with torch.no_grad():
            m.decoder.out.bias[EOS] += extra
        prefix = second_best_prefixes(nbest(m, src, im, lens=lens)[0])
        c = con(m, src, im, lens=lens, prefix=prefix)
        sc = c.scores.cpu().numpy()
        idx = [(b, r) for b in range(B) for r in range(K) if len(c.hyps[b][r]) < ML - 1 and sc[b, r] > -1e4]
        if len(idx) >= 8:
            break
    assert len(idx) >= 8, len(idx)
    for b, r in idx:
        assert [int(t) for t in c.hyps[b][r][:len(prefix[b])]] == prefix[b]
    flat = [list(c.hyps[b][r]) for b in range(B) for r in range(K)]
    src_n = src.repeat_interleave(K, 0)
    lens_n = [n for n in lens for _ in range(K)]
    forced = m.score_translations(src_n, lens_n, flat, im.repeat_interleave(K, 0)) if kind == "mm" else \
        m.score_translations(src_n, lens_n, flat)
    f = forced.score.cpu().numpy().reshape(B, K)
    rel = max(abs(float(f[b, r]) - float(sc[b, r])) / max(1.0, abs(float(sc[b, r]))) for b, r in idx)
    print("%d finished hypotheses, forced vs constrained search score: max rel err %.3e" % (len(idx), rel))
    assert rel <= 2e-4, rel


def test_bans_are_kept(subject):
    _, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    hyps = ints(hyps)
    assert all(len(h[0]) >= 1 for h in hyps) and len(hyps[0][0]) >= 2
    first = [h[0][0] for h in hyps]
    bigram = hyps[0][0][:2]
    for graph in (True, False):
        m.decode_graph = graph
        c = con(m, src, im, banned=[bigram], banned_per_sentence=[[[w]] for w in first])
        got = live(c)
        assert {b for b, r, _ in got if r == 0} == {0, 1, 2}
        for b, r, h in got:
            assert first[b] not in h and not contains(h, bigram), (graph, b, r, h)
        assert all(ints(c.hyps)[b] != hyps[b] for b in range(3))
    m.decode_graph = True


def test_no_repeat_bigrams(subject):
    """no_repeat_ngram=2 with avoid_double=False.  The models' seed (21) is one whose unconstrained search, under the same
    options, does repeat a bigram in a live hypothesis -- asserted first."""
    _, m, src, im = subject
    hyps, sc = nbest(m, src, im, avoid_double=False)
    sc = sc.cpu().numpy()
    assert any(bigrams_repeat([int(t) for t in h]) for b, hs in enumerate(hyps) for r, h in enumerate(hs) if sc[b, r] > -1e4)
    for graph in (True, False):
        m.decode_graph = graph
        c = con(m, src, im, no_repeat_ngram=2, avoid_double=False)
        got = live(c)
        assert {b for b, r, _ in got if r == 0} == {0, 1, 2}
        for b, r, h in got:
            assert not bigrams_repeat(h), (graph, b, r, h)
    m.decode_graph = True


def test_search_driven_from_the_test_with_the_numpy_mask(subject):
    """Eager Member steps, the reference's mask copied onto the device rows, vag_beam_ens_step_opt and the n-best finish: the
    eager API's result bit for bit."""
    from vagnmt_hip import constrain as CN
    from vagnmt_hip import search
    _, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    kw = a_constraint_set(hyps)
    m.decode_graph = False
    try:
        api = con(m, src, im, **kw)
        packed = CN.pack(3, VT, ML, **kw)
        B, k, V = 3, K, VT
        with torch.no_grad():
            enc, mask, h0 = m._decode_prologue(src, LENS, im)
            mb = search.Member(m, enc, mask, k, ML, None, 0)
            e = search.search_buffer(B, k, V, ML, enc.device)
            beam, nll, n_alive = e["beam"], e["nll"], e["n_alive"]
            tok, h, steps = torch.full((B,), R.SOS, dtype=I64, device="cuda"), h0, 0
            for di in range(ML):
                h2, logp = mb.step(tok, h, 1 if di == 0 else k)
                masked = R.mask([logp.cpu().numpy()], beam.cpu().numpy(), di, ML, B, k, V, packed.prefix, packed.phrases,
                                packed.phrase_sent, packed.ngram)[0]
                logp.copy_(torch.from_numpy(masked))
                h_next = torch.empty(B * k, mb.H, device="cuda")
                assert L().vag_beam_ens_step_opt(pp([logp]), p64([logp.shape[1]]), 1, nll.data_ptr(), beam.data_ptr(), di, ML,
                                                 pp([h2]), pp([h_next]), p64([mb.H]), B, k, V, n_alive.data_ptr(),
                                                 e["scratch"].data_ptr(), 0, stream()) == 0
                h, tok, steps = h_next, beam[di].view(-1), di + 1
                if di % 8 == 7 and int(n_alive.item()) == 0:       # the poll of search.beam
                    break
            out = torch.empty(B, k, ML, dtype=I64, device="cuda")
            sc = torch.empty(B, k, device="cuda")
            assert L().vag_beam_finish_nbest(nll.data_ptr(), beam.data_ptr(), ML, steps, B, k, k, out.data_ptr(), sc.data_ptr(),
                                             stream()) == 0
        assert search.cut_nbest(out.cpu().numpy(), k) == ints(api.hyps) and torch.equal(bits(sc), bits(api.scores))
        assert len(live(api)) >= 3
    finally:
        m.decode_graph = True


def test_graph_and_eager_agree(subject):
    _, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    kw = a_constraint_set(hyps)
    res = []
    for graph in (True, False):
        m.decode_graph = graph
        res.append(con(m, src, im, **kw))
    m.decode_graph = True
    g, e = res
    # two fp32 evaluations of the same sums (graph mode pads the source to 8 positions, which regroups the attention's
    # reductions): the relative 2e-4 the diverse search's test states for this pair; the lists are equal
    rel = ((g.scores - e.scores).abs() / e.scores.abs().clamp(min=1.0)).max().item()
    print("graph vs eager: max rel score diff %.3e" % rel)
    assert ints(g.hyps) == ints(e.hyps) and rel <= 2e-4


def test_static_buffers_hold_nothing_stale(subject):
    """One graph entry serves every constraint set of one no_repeat_ngram: after set A, a smaller set B (a shorter prefix,
    fewer phrases) gives what a fresh model gives on B, bit for bit; two values of no_repeat_ngram have entries of their own."""
    kind, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    A = a_constraint_set(hyps)
    small = dict(prefix=[A["prefix"][0][:1], [], []], banned=[A["banned"][0]], no_repeat_ngram=2)
    other = dict(small, no_repeat_ngram=3)
    m.decode_graph = True
    got = [con(m, src, im, **kw) for kw in (A, small, other, A, small)]
    # the entries of this shape and these options (key: kind, B, k, Tp, max_length, raw logits, hoisted, flags, ...; other tests
    # on this model left entries for other widths and for avoid_double=False): one per no_repeat_ngram, whatever the set
    keys = [key for key in m._decode_cache if isinstance(key, tuple) and "constrain" in key]
    assert keys and all(key[0] == "beam_con" for key in keys)
    ngrams = [key[key.index("constrain") + 1] for key in keys if key[2] == K and key[7] == 0]
    assert ngrams.count(2) == 1 and ngrams.count(3) == 1
    for kw, c in zip((A, small, other, A, small), got):
        fresh = make_model(kind, 21)                                   # the same weights, nothing cached
        assert same(c, con(fresh, src, im, **kw)), sorted(kw.items())
    assert not same(got[0], got[1])


def test_ensemble_of_twins_is_the_model(subject):
    from vagnmt_hip.ensemble import Ensemble
    _, m, src, im = subject
    hyps, _ = nbest(m, src, im)
    A = a_constraint_set(hyps)
    small = dict(prefix=[A["prefix"][0][:1], [], []], no_repeat_ngram=2)
    ens = Ensemble([m, m])
    for graph in (True, False):
        m.decode_graph = ens.decode_graph = graph
        for kw in (A, small, {}):
            c = con(m, src, im, n_best=4, **kw)
            e = con(ens, src, im, n_best=4, **kw)
            assert same(c, e), (graph, sorted(kw))
    assert any(isinstance(key, tuple) and key[0] == "ens_beam_con" and "constrain" in key for key in ens._cache)
    m.decode_graph = True
