"""GPU: beam search with required phrases (vagnmt_hip.require; include/vag_nmt.h: vag_beam_req_step).

1. the expansion against tests/require_ref.py bit for bit -- words, parents, scores, the four state words, n_alive -- at every
   step of whole searches on a quantised table model (values in 1/8: ties everywhere), with a forced prefix on one sentence
   through vag_beam_constrain, for one and three members; every branch of the rule counted on the CPU and asserted;
2. no phrases is vag_beam_ens_step_opt; the device-index form; the ABI's argument errors;
3. the models and Ensemble: no phrases is beamsearch_nbest, complete hypotheses hold their phrases, scores against forced
   scores, a search driven from the test with the NumPy step, graph against eager mode, the static buffers of a graph entry,
   required phrases together with bans and no-repeat bigrams.

Stage 2 of the expansion has two paths by size (csrc/beam.hip: winners kept in registers up to 2048 per sentence, read from the
scratch beyond): the third shape below (k = 16, nine slices: 2304 winners) takes the second."""
import ctypes as C

import numpy as np
import pytest
import torch

import constrain_ref as CR
import require_ref as R

pytestmark = pytest.mark.gpu

EOS, UNK, SOS = 3, 1, 2
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
    """The buffers of one search, driven step by step through the ABI.  The state starts as garbage: step 0 ignores it."""

    def __init__(self, B, k, V, max_len, Hs, table):
        self.B, self.k, self.V, self.max_len, self.Hs = B, k, V, max_len, list(Hs)
        self.beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
        self.nll = torch.zeros(B, k, device="cuda")
        self.n_alive = torch.full((1,), -7, dtype=I32, device="cuda")
        self.scratch = torch.empty(L().vag_beam_req_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        self.tok = torch.full((B * k,), -1, dtype=I64, device="cuda")
        self.di_state = torch.zeros(2, dtype=I32, device="cuda")
        self.state = torch.full((B, k, 4), 0x5a5a5a5a, dtype=I32, device="cuda")
        self.table = dev(table, I64)

    def step(self, logps, h_ins, di, flags=0, device_index=False, table="own", state="own"):
        """One expansion; logps / h_ins: M tensors (rows, ldl) / (rows, H[m]).  Returns (rc, h_outs)."""
        h_outs = [torch.full((self.B * self.k, H), float("nan"), device="cuda") for H in self.Hs]
        ldl = p64([x.shape[1] for x in logps])
        tp = self.table.data_ptr() if table == "own" else table
        sp = self.state.data_ptr() if state == "own" else state
        if device_index:
            rc = L().vag_beam_req_step_dev(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(),
                                           self.di_state.data_ptr(), self.max_len, pp(h_ins), pp(h_outs), p64(self.Hs),
                                           self.tok.data_ptr(), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                           self.scratch.data_ptr(), flags, tp, sp, stream())
        else:
            rc = L().vag_beam_req_step(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(), di, self.max_len,
                                       pp(h_ins), pp(h_outs), p64(self.Hs), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                       self.scratch.data_ptr(), flags, tp, sp, stream())
        return rc, h_outs


def quantised(rng, rows, V, ldl):
    """Log-probabilities on a grid of 1/8 in [-12, 0]; the columns past V hold +100 (a read there would win every selection)."""
    a = np.full((rows, ldl), 100.0, dtype=np.float32)
    a[:, :V] = rng.integers(-96, 1, size=(rows, V)) / 8.0
    return a


def kernel_combined(logps, V):
    """The kernels' own ensemble scores of every (row, word), read back through plain (groups = 1) steps at step 0 on windows
    of at most 64 words (k = the window: the step returns every word of the window with its score, c = 0 + score)."""
    rows = logps[0].shape[0]
    kw = min(64, V)
    starts = list(range(0, V - kw + 1, kw))
    if starts[-1] + kw < V:
        starts.append(V - kw)
    out = np.full((rows, V), np.nan, dtype=np.float32)
    beam = torch.zeros(2, rows, kw, dtype=I64, device="cuda")
    nll = torch.zeros(rows, kw, device="cuda")
    n_alive = torch.zeros(1, dtype=I32, device="cuda")
    scratch = torch.empty(L().vag_beam_div_scratch_bytes(rows, kw, kw, 1), dtype=torch.uint8, device="cuda")
    h = [torch.zeros(rows, 1, device="cuda") for _ in logps]
    for w0 in starts:
        ho = [torch.empty(rows * kw, 1, device="cuda") for _ in logps]
        rc = L().vag_beam_div_step(pp(logps, 4 * w0), p64([x.shape[1] for x in logps]), len(logps), nll.data_ptr(),
                                   beam.data_ptr(), 0, 1, pp(h), pp(ho), p64([1] * len(logps)), rows, kw, kw, n_alive.data_ptr(),
                                   scratch.data_ptr(), 0, 1, 0.0, stream())
        assert rc == 0
        words, vals = beam[0].cpu().numpy(), nll.cpu().numpy()
        assert all(sorted(r) == list(range(kw)) for r in words.tolist())
        np.put_along_axis(out[:, w0:w0 + kw], words, vals, axis=1)
    assert not np.isnan(out).any()
    return out


# ------------------------------------------------------------------------------------------------------------------
# 1. whole searches on a table model against the reference, step by step
# ------------------------------------------------------------------------------------------------------------------
A_, B_, C_, X_, Y_, Z_, U_ = 5, 6, 7, 8, 9, 10, 11
# sentence 0: a one-word phrase, a self-overlapping three-word phrase, an unused entry between used ones, a phrase that shares
# its first word with the second; sentence 1 (where there are three): two phrases around unused entries; the last: none
PHRASES0 = [[C_], [A_, B_, A_], None, [A_, C_]]
PHRASES1 = [[X_, Y_], None, None, [U_]]
PREFIX0 = [Z_, A_, B_]                         # forced on sentence 0 through vag_beam_constrain: it advances a b a to 2
ROWS = 61                                      # rows of the table "model": logp = T[previous word % ROWS]

# (B, k, V, ldl, max_len, seed, EOS bias): a row shorter than a slice; two slices, unaligned rows; stage 2's second path.
# Seeds and biases are chosen on the CPU, with the reference alone, so that over the two M = 1 searches of a shape (flags 0 and
# VAG_BEAM_ALLOW_REPEAT) every branch fires in at least 3 (row, step) pairs -- asserted below.
SHAPES = [(2, 3, 37, 40, 9, 0, 4.0), (3, 5, 2500, 2501, 12, 1, 4.0), (3, 16, 18000, 18000, 6, 14, 8.0)]


def phrase_lists(B):
    return [PHRASES0] + ([PHRASES1] if B > 2 else []) + [[]]


def table_model(B, k, V, ldl, max_len, seed, eos_bias, M):
    """M members' tables (ROWS, ldl): quantised, EOS and the word `a` lifted; members beyond the first off the grid."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(M):
        T = quantised(rng, ROWS, V, ldl)
        T[:, EOS] += np.float32(eos_bias)
        T[:, A_] += np.float32(2.0)
        if m > 0:
            T[:, :V] += np.float32(0.01 * m) * rng.standard_normal((ROWS, V)).astype(np.float32)
        out.append(T)
    return out


def reference_search(shape, tables, flags, counts=None):
    """The reference's records of a whole search of the case `shape` on `tables` (M arrays (ROWS, >= V))."""
    B, k, V, ldl, max_len = shape[:5]
    prefix = np.zeros((B, 3), dtype=np.int64)
    prefix[0] = PREFIX0
    records = []
    R.search(lambda tok: [T[tok % ROWS] for T in tables], B, k, V, max_len, max_len, R.table_of(phrase_lists(B), B), flags, counts,
             prefix=prefix, records=records)
    return records, prefix


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_reference_bit_for_bit(shape, M):
    B, k, V, ldl, max_len, seed, eos_bias = shape
    tables = table_model(B, k, V, ldl, max_len, seed, eos_bias, M)
    Td = [dev(T) for T in tables]
    if M == 1:
        ref_tables = tables
    else:
        # the NumPy restatement of the ensemble score may differ from the device's expf / logf in the last bits: it is checked
        # to a few ulp, and the search is compared exactly on the kernels' own combined values
        comb = kernel_combined(Td, V)
        want = R.ens_combine([T[:, :V] for T in tables])
        assert np.allclose(comb, want, rtol=2e-6, atol=2e-6), np.abs(comb - want).max()
        ref_tables = [comb]
    Hs = [8, 6, 4][:M]
    counts = R.new_counts()
    for flags in (0, R.ALLOW_REPEAT):
        records, prefix = reference_search(shape, ref_tables, flags, counts)
        s = Search(B, k, V, max_len, Hs, R.table_of(phrase_lists(B), B))
        d_prefix = dev(prefix)
        h = [torch.zeros(B, H, device="cuda") for H in Hs]
        for di in range(max_len):
            tok = torch.full((B,), SOS, dtype=I64, device="cuda") if di == 0 else s.beam[di - 1].reshape(-1)
            logps = [T[tok % ROWS].contiguous() for T in Td]
            assert L().vag_beam_constrain(pp(logps), p64([ldl] * M), M, s.beam.data_ptr(), di, max_len, B, k, V,
                                          d_prefix.data_ptr(), 3, None, None, 0, 0, stream()) == 0
            rc, h = s.step(logps, h, di, flags)
            assert rc == 0
            words, parents, nll, state, alive = records[di]
            what = (shape, M, flags, di)
            assert np.array_equal(s.beam[di].cpu().numpy(), words), what
            assert np.array_equal(s.beam[max_len + di].cpu().numpy(), parents), what
            assert s.nll.cpu().numpy().tobytes() == nll.tobytes(), what
            assert np.array_equal(s.state.cpu().numpy(), state), what
            assert int(s.n_alive.item()) == alive, what
    print("branches", shape, "M", M, counts)
    if M == 1:
        for name in R.BRANCHES:
            assert counts[name] >= 3, (shape, name, counts)


# ------------------------------------------------------------------------------------------------------------------
# 2. no phrases, the device-index form, argument errors
# ------------------------------------------------------------------------------------------------------------------
def test_no_phrases_is_the_plain_step_bit_for_bit():
    """All L_c = 0 against vag_beam_ens_step_opt on the same rows at steps 0, 1 and 5, flags 0 and 3: words, parents, score
    bits, hidden states, n_alive; the state stays empty."""
    rng = np.random.default_rng(5)
    B, k, V, max_len, H = 2, 12, 4100, 8, 8
    none = np.zeros((B, 16, 8), dtype=np.int64)
    for di in (0, 1, 5):
        for flags in (0, 3):
            k_in = 1 if di == 0 else k
            logp = [dev(quantised(rng, B * k_in, V, V))]
            h_in = [dev(rng.standard_normal((B * k_in, H)).astype(np.float32))]
            base = dev((rng.integers(-400, 0, size=(B, k)) / 8.0).astype(np.float32))
            prev = rng.integers(0, V, size=(B, k))
            prev[rng.random((B, k)) < 0.3] = EOS
            a = Search(B, k, V, max_len, [H], none)
            a.state.zero_()
            p_beam, p_nll, p_alive = torch.zeros_like(a.beam), base.clone(), torch.zeros(1, dtype=I32, device="cuda")
            a.nll.copy_(base)
            if di > 0:
                a.beam[di - 1].copy_(dev(prev))
                p_beam[di - 1].copy_(dev(prev))
            rc, ha = a.step(logp, h_in, di, flags)
            assert rc == 0
            hp = [torch.empty(B * k, H, device="cuda")]
            scratch = torch.empty(L().vag_beam_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
            assert L().vag_beam_ens_step_opt(pp(logp), p64([V]), 1, p_nll.data_ptr(), p_beam.data_ptr(), di, max_len, pp(h_in),
                                             pp(hp), p64([H]), B, k, V, p_alive.data_ptr(), scratch.data_ptr(), flags,
                                             stream()) == 0
            assert torch.equal(a.beam, p_beam) and torch.equal(a.nll.view(I32), p_nll.view(I32)), (di, flags)
            assert torch.equal(ha[0].view(I32), hp[0].view(I32)) and torch.equal(a.n_alive, p_alive), (di, flags)
            assert not bool(a.state[:, :, 1:].any())                      # no progress, an empty bank


def test_device_index_form():
    """A whole search through the _dev form equals the by-value form, advances di_state once per step, and writes nothing at
    di = max_len."""
    shape = SHAPES[0]
    B, k, V, ldl, max_len, seed, eos_bias = shape
    Td = dev(table_model(B, k, V, ldl, max_len, seed, eos_bias, 1)[0])
    table = R.table_of(phrase_lists(B), B)
    H = 8
    a, d = Search(B, k, V, max_len, [H], table), Search(B, k, V, max_len, [H], table)
    h0 = torch.zeros(B, H, device="cuda")
    for s in (a, d):
        rc, s.h = s.step([Td[torch.full((B,), SOS, dtype=I64, device="cuda") % ROWS].contiguous()], [h0], 0)
        assert rc == 0
    d.di_state.copy_(torch.tensor([1, 0], dtype=I32))
    for di in range(1, max_len):
        rc, a.h = a.step([Td[a.beam[di - 1].reshape(-1) % ROWS].contiguous()], a.h, di)
        assert rc == 0
        rc, d.h = d.step([Td[d.beam[di - 1].reshape(-1) % ROWS].contiguous()], d.h, 0, device_index=True)
        assert rc == 0
        assert d.di_state.cpu().tolist() == [di + 1, 0]
        assert torch.equal(d.tok, d.beam[di].view(-1))
    assert torch.equal(a.beam, d.beam) and torch.equal(a.nll.view(I32), d.nll.view(I32)) and torch.equal(a.h[0], d.h[0])
    assert torch.equal(a.state, d.state) and torch.equal(a.n_alive, d.n_alive) and bool(a.state[0, :, 3].any())
    before = [t.clone() for t in (d.beam, d.nll, d.tok, d.n_alive, d.di_state, d.state)]
    d.n_alive.fill_(-3); before[3].fill_(-3)
    rc, h = d.step([Td[d.beam[max_len - 1].reshape(-1) % ROWS].contiguous()], d.h, 0, device_index=True)
    assert rc == 0
    for t, b in zip((d.beam, d.nll, d.tok, d.n_alive, d.di_state, d.state), before):
        assert torch.equal(t, b)
    assert bool(torch.isnan(h[0]).all())


def test_abi_argument_errors_launch_nothing():
    B, k, V, max_len, H = 2, 6, 50, 4, 8
    s = Search(B, k, V, max_len, [H], np.zeros((B, 16, 8), dtype=np.int64))
    logp = [torch.zeros(B, V, device="cuda")]
    h = [torch.zeros(B, H, device="cuda")]

    def call(k_=k, V_=V, flags=0, M=1, di=0, nll=None, dev_form=False, di_state=True, table="own", state="own", B_=B):
        ho = [torch.full((B * 64, H), float("nan"), device="cuda")]
        nllp = s.nll.data_ptr() if nll is None else nll
        tp = s.table.data_ptr() if table == "own" else table
        sp = s.state.data_ptr() if state == "own" else state
        if dev_form:
            rc = L().vag_beam_req_step_dev(pp(logp), p64([V]), M, nllp, s.beam.data_ptr(), s.di_state.data_ptr() if di_state else None,
                                           max_len, pp(h), pp(ho), p64([H]), s.tok.data_ptr(), B_, k_, V_, s.n_alive.data_ptr(),
                                           s.scratch.data_ptr(), flags, tp, sp, stream())
        else:
            rc = L().vag_beam_req_step(pp(logp), p64([V]), M, nllp, s.beam.data_ptr(), di, max_len, pp(h), pp(ho), p64([H]), B_, k_,
                                       V_, s.n_alive.data_ptr(), s.scratch.data_ptr(), flags, tp, sp, stream())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ho[0]).all())
    bad = [dict(table=None), dict(state=None), dict(dev_form=True, table=None), dict(dev_form=True, state=None), dict(V_=5),
           dict(flags=4), dict(M=0), dict(M=9), dict(k_=65), dict(k_=0), dict(B_=0), dict(di=-1), dict(di=max_len), dict(nll=0),
           dict(dev_form=True, di_state=False), dict(B_=65536 // k + 1)]
    for kw in bad:
        assert call(**kw) == (-22, True), kw
    assert int(s.n_alive.item()) == -7 and not bool(s.beam.any()) and not bool(s.nll.any())
    assert bool((s.state == 0x5a5a5a5a).all())
    assert L().vag_beam_req_step(None, p64([V]), 1, s.nll.data_ptr(), s.beam.data_ptr(), 0, max_len, pp(h), pp(h), p64([H]), B, k, V,
                                 s.n_alive.data_ptr(), s.scratch.data_ptr(), 0, s.table.data_ptr(), s.state.data_ptr(),
                                 stream()) == -22
    assert L().vag_beam_req_scratch_bytes(16, 12, 9391, 80) >= 16 * 12 * 5 * 12 * 8
    assert call() == (0, False)                                             # and the good call goes through
    assert not bool(s.state.any())


# ------------------------------------------------------------------------------------------------------------------
# 3. models (small random ones, built as tests/test_gpu_constrain.py builds them)
# ------------------------------------------------------------------------------------------------------------------
VS, VT, IM, ML = 70, 503, 64, 10
LENS = [8, 6, 3]                # the longest source is a multiple of 8: graph mode pads nothing, so the two modes run the same sums
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


EOS_BIAS = 2.0          # lets hypotheses end before max_length once their phrases are met


@pytest.fixture(scope="module", params=["mm", "text"])
def subject(request):
    """(kind, model, src, im, phrases): the phrases come from the n-best lists of the model WITHOUT an EOS bias (every hypothesis
    runs to max_length there, so a second-best hypothesis has words to take); the bias is added afterwards."""
    m = make_model(request.param, 21)
    src, im = make_inputs()
    im = im if request.param == "mm" else None
    phrases = phrases_from(nbest(m, src, im)[0])
    with torch.no_grad():
        m.decoder.out.bias[EOS] += EOS_BIAS
    return request.param, m, src, im, phrases


def nbest(m, src, im, k=K, n=K, lens=LENS, **kw):
    return m.beamsearch_nbest(src, lens, im, k, n, ML, **kw) if im is not None else m.beamsearch_nbest(src, lens, k, n, ML, **kw)


def req(m, src, im, lens=LENS, **kw):
    kw.setdefault("beam_size", K)
    kw.setdefault("n_best", K)
    kw.setdefault("max_length", ML)
    return m.beamsearch_required(src, lens, im, **kw)


def same(a, b):
    return ints(a.hyps) == ints(b.hyps) and torch.equal(bits(a.scores), bits(b.scores)) and torch.equal(a.met, b.met) and \
        torch.equal(a.complete, b.complete)


def phrases_from(hyps):
    """Per sentence, from its second-best unconstrained hypothesis h2: a bigram of h2 (one the best hypothesis does not contain
    where there is one, and not its opening, so that the search has to change) and a word of h2 outside that bigram where there is one (one the
    best hypothesis lacks where there is one).  Content words only (> 3), no immediate repeat."""
    out = []
    for hs in hyps:
        h1, h2 = [int(t) for t in hs[0]], [int(t) for t in hs[1]]
        big = [h2[i:i + 2] for i in range(len(h2) - 1, 0, -1) if len(h2[i:i + 2]) == 2 and min(h2[i:i + 2]) > 3 and h2[i] != h2[i + 1]]
        assert big, (h1, h2)
        big = [g for g in big if not R.contains(h1, g)] or big
        rest = [w for w in h2 if w > 3 and w not in big[0]] or [big[0][0]]     # (a hypothesis of two words: one of them again)
        single = [w for w in rest if w not in h1] or rest
        out.append([big[0], [single[-1]]])
    return out


def check_required(r, phrases, n=K):
    """What every Required result must satisfy."""
    sc = r.scores.cpu().numpy()
    met, comp = r.met.cpu().numpy(), r.complete.cpu().numpy()
    assert r.met.dtype == I64 and r.complete.dtype == torch.bool and sc.shape == met.shape == comp.shape == (len(phrases), n)
    for b, hs in enumerate(r.hyps):
        assert len(hs) == n
        want = (1 << len(phrases[b])) - 1
        for i, h in enumerate(hs):
            h = [int(t) for t in h]
            for c, ph in enumerate(phrases[b]):
                if (int(met[b, i]) >> c) & 1:
                    assert R.contains(h, ph), (b, i, c, h, ph)               # every set bit is true of the words
            assert bool(comp[b, i]) == (int(met[b, i]) & want == want)
            if comp[b, i]:
                assert all(R.contains(h, ph) for ph in phrases[b]), (b, i, h)
        nc = int(comp[b].sum())
        assert comp[b, :nc].all() and not comp[b, nc:].any(), comp[b]        # complete entries first
        for part in (sc[b, :nc], sc[b, nc:]):
            assert (part[1:] <= part[:-1]).all(), sc[b]                      # scores descend within each part
        assert comp[b, 0], (b, hs[0], phrases[b])                            # the best hypothesis is complete


def test_no_phrases_is_beamsearch_nbest(subject):
    _, m, src, im, _ = subject
    for graph in (True, False):
        m.decode_graph = graph
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(m, src, im, k, n)
            for kw in (dict(), dict(required=[[], [], []], prefix=[[], [], []], banned=[], banned_per_sentence=[[], [], []])):
                r = req(m, src, im, beam_size=k, n_best=n, **kw)
                assert ints(r.hyps) == ints(hyps) and torch.equal(bits(r.scores), bits(sc)), (graph, k)
                assert not bool(r.met.any()) and bool(r.complete.all())
    m.decode_graph = True


def test_complete_hypotheses_hold_their_phrases(subject):
    _, m, src, im, phrases = subject
    hyps, _ = nbest(m, src, im)
    for graph in (True, False):
        m.decode_graph = graph
        r = req(m, src, im, required=phrases)
        check_required(r, phrases)
        assert any(ints(r.hyps)[b][0] != ints(hyps)[b][0] for b in range(3))         # the search did change
        r3 = req(m, src, im, required=phrases, n_best=3)
        assert ints(r3.hyps) == [h[:3] for h in ints(r.hyps)] and torch.equal(bits(r3.scores), bits(r.scores[:, :3]))
    m.decode_graph = True


def test_scores_are_forced_scores(subject):
    """Complete hypotheses that ended before max_length score, forced, what the search scored them: relative 2e-4, the bound of
    the project's search-vs-scoring tests.  Six sentences: 36 hypotheses to find 8 in."""
    kind = subject[0]
    m = make_model(kind, 23)
    lens = [9, 8, 6, 5, 3, 2]
    src, im = make_inputs(lens, seed=11)
    im = im if kind == "mm" else None
    B = len(lens)
    phrases = phrases_from(nbest(m, src, im, lens=lens)[0])              # (before any EOS bias: 9-word hypotheses)
    idx = []
    for extra in (0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0):
        with torch.no_grad():
            m.decoder.out.bias[EOS] += extra
        r = req(m, src, im, lens=lens, required=phrases)
        sc, comp = r.scores.cpu().numpy(), r.complete.cpu().numpy()
        idx = [(b, i) for b in range(B) for i in range(K) if comp[b, i] and len(r.hyps[b][i]) < ML - 1 and sc[b, i] > -1e4]
        if len(idx) >= 8:
            break
    assert len(idx) >= 8, len(idx)
    for b, i in idx:
        assert all(R.contains(r.hyps[b][i], ph) for ph in phrases[b])
    flat = [list(r.hyps[b][i]) for b in range(B) for i in range(K)]
    src_n = src.repeat_interleave(K, 0)
    lens_n = [n for n in lens for _ in range(K)]
    forced = m.score_translations(src_n, lens_n, flat, im.repeat_interleave(K, 0)) if kind == "mm" else \
        m.score_translations(src_n, lens_n, flat)
    f = forced.score.cpu().numpy().reshape(B, K)
    rel = max(abs(float(f[b, i]) - float(sc[b, i])) / max(1.0, abs(float(sc[b, i]))) for b, i in idx)
    print("%d complete finished hypotheses, forced vs required search score: max rel err %.3e" % (len(idx), rel))
    assert rel <= 2e-4, rel


def test_search_driven_from_the_test_with_the_numpy_step(subject):
    """Eager Member steps, require_ref.step on the model's own log-probability rows, the history written by hand, the n-best
    finish: the eager API's words."""
    from vagnmt_hip import require as Q
    from vagnmt_hip import search
    _, m, src, im, phrases = subject
    m.decode_graph = False
    try:
        api = req(m, src, im, required=phrases)
        B, k, V = 3, K, VT
        table = Q.pack(B, V, ML, phrases)
        with torch.no_grad():
            enc, mask, h0 = m._decode_prologue(src, LENS, im)
            mb = search.Member(m, enc, mask, k, ML, None, 0)
            beam = np.zeros((2 * ML, B, k), dtype=np.int64)
            nll = np.zeros((B, k), dtype=np.float32)
            states = [[R.ZERO] * k for _ in range(B)]
            tok, h = torch.full((B,), SOS, dtype=I64, device="cuda"), h0
            for di in range(ML):
                k_in = 1 if di == 0 else k
                h2, logp = mb.step(tok, h, k_in)
                lp = logp.cpu().numpy()[:, :V].reshape(B, k_in, V)
                for b in range(B):
                    w, p, sc, states[b] = R.step([lp[b]], None if di == 0 else nll[b], None if di == 0 else beam[di - 1, b], k,
                                                 table[b], states[b], 0, last=di == ML - 1)
                    beam[di, b], beam[ML + di, b], nll[b] = w, p, sc
                parent = torch.from_numpy(beam[ML + di]).cuda() + torch.arange(B, device="cuda")[:, None] * k_in
                h, tok = h2[parent.view(-1)].contiguous(), torch.from_numpy(beam[di]).cuda().view(-1)
            out = torch.empty(B, k, ML, dtype=I64, device="cuda")
            sc = torch.empty(B, k, device="cuda")
            slots = torch.empty(B, k, dtype=I64, device="cuda")
            d_beam, d_nll = dev(beam), dev(nll)
            assert L().vag_beam_finish_nbest_slots(d_nll.data_ptr(), d_beam.data_ptr(), ML, ML, B, k, k, out.data_ptr(), sc.data_ptr(),
                                                   slots.data_ptr(), stream()) == 0
        state = torch.from_numpy(np.stack([R.pack_states(s) for s in states])).cuda()
        want = Q.assemble(search.cut_nbest(out.cpu().numpy(), k), sc, slots, state, table, k)
        assert ints(want.hyps) == ints(api.hyps)
        assert torch.equal(want.met, api.met) and torch.equal(want.complete, api.complete)
        assert bool(api.complete[:, 0].all())
    finally:
        m.decode_graph = True


def test_graph_and_eager_agree_bit_for_bit(subject):
    _, m, src, im, phrases = subject
    res = []
    for graph in (True, False):
        m.decode_graph = graph
        res.append(req(m, src, im, required=phrases))
    m.decode_graph = True
    assert same(res[0], res[1])


def test_static_buffers_hold_nothing_stale(subject):
    """One graph entry serves every phrase set: after set A, a smaller set (one phrase for one sentence) gives what a fresh
    model gives on it, bit for bit."""
    kind, m, src, im, A = subject
    small = [[A[0][1]], [], []]
    m.decode_graph = True
    got = [req(m, src, im, required=p) for p in (A, small, A, small)]
    keys = [key for key in m._decode_cache if isinstance(key, tuple) and key[0] == "beam_req"]
    assert len([key for key in keys if key[2] == K and key[7] == 0]) == 1
    for p, r in zip((A, small, A, small), got):
        fresh = make_model(kind, 21, eos_bias=EOS_BIAS)                 # the same weights, nothing cached
        assert same(r, req(fresh, src, im, required=p)), p
    assert not same(got[0], got[1])
    check_required(got[1], small)


def test_ensemble_of_twins_is_the_model(subject):
    from vagnmt_hip.ensemble import Ensemble
    _, m, src, im, A = subject
    ens = Ensemble([m, m])
    for graph in (True, False):
        m.decode_graph = ens.decode_graph = graph
        for kw in (dict(required=A), dict(required=A, no_repeat_ngram=2), dict()):
            c = req(m, src, im, n_best=4, **kw)
            e = req(ens, src, im, n_best=4, **kw)
            assert same(c, e), (graph, sorted(kw))
    assert any(isinstance(key, tuple) and key[0] == "ens_beam_req" for key in ens._cache)
    m.decode_graph = True


def test_required_with_bans_and_no_repeat_bigrams(subject):
    """required together with banned and no_repeat_ngram=2: complete hypotheses hold the phrases, and no live hypothesis
    contains a banned phrase or repeats a bigram."""
    _, m, src, im, phrases = subject
    flat = [w for ps in phrases for ph in ps for w in ph]
    best0 = [int(t) for t in req(m, src, im, required=phrases).hyps[0][0]]
    banned = [[w] for w in best0 if w > 3 and w not in flat][:1] + [[VT - 1]]      # a word the required search uses: it must change
    assert len(banned) == 2
    for graph in (True, False):
        m.decode_graph = graph
        r = req(m, src, im, required=phrases, banned=banned, no_repeat_ngram=2)
        check_required(r, phrases)
        sc = r.scores.cpu().numpy()
        for b, hs in enumerate(r.hyps):
            for i, h in enumerate(hs):
                h = [int(t) for t in h]
                if sc[b, i] > -1e4:
                    g = list(zip(h, h[1:]))
                    assert len(set(g)) == len(g) and not any(R.contains(h, ph) for ph in banned), (graph, b, i, h)
    m.decode_graph = True


def test_a_prefix_word_that_advances_a_phrase_counts(subject):
    _, m, src, im, phrases = subject
    prefix = [list(ps[0]) for ps in phrases]                              # every sentence begins with its own bigram
    r = req(m, src, im, required=phrases, prefix=prefix)
    check_required(r, phrases)
    sc, met = r.scores.cpu().numpy(), r.met.cpu().numpy()
    for b, hs in enumerate(r.hyps):
        for i, h in enumerate(hs):
            if sc[b, i] > -1e4:
                assert [int(t) for t in h[:2]] == prefix[b] and int(met[b, i]) & 1, (b, i, h)
