"""GPU: chrF on surface characters (include/vag_nmt.h: vag_surface_expand, vag_chrf_select) against tests/chrf_ref.py.

1. the expansion against Surface.text: the span's rules, empty surfaces, multi-byte characters, rows of exactly C and of C + 1
   characters, L = 1, and a row of more than one 64-token chunk;
2. match counts m_1..m_6 integer-exact (alphabet of three characters: n-grams repeat, the clipping works), at every row length
   where the kernel changes path (0, 1, 5 < the order, 6, 63 / 64 / 65, 128 / 129, the limit), the utility bit for bit against the
   NumPy float32 restatement and within 1e-6 of the float64 value, expected utility in the fixed order, the first arg-max;
3. self-reference, given weights, a tie, determinism;
4. mbr_decode(utility="chrf") on a small golden model and an Ensemble; the pair on which token BLEU and chrF disagree;
5. mrt_step / expected_risk with cost="chrf".

Bounds.  Counts, lengths and best are integers: equality.  The utility is a fixed sequence of IEEE float32 operations, which
NumPy float32 performs identically: equality of bits.  Against float64: u <= 1 comes out of at most 2 x 6 quotients and 2 x 6
partial sums (each <= 6, rounding error <= 2^-22 = 2.4e-7 absolute at worst, then divided by E), two more quotients, two
products and a final quotient, each relative 2^-24 = 6e-8 on values <= 5: in all below 1e-6 absolute, the bound the definition
allows."""
import functools

import numpy as np
import pytest
import torch

import chrf_ref as R

pytestmark = pytest.mark.gpu

EOS = 3
A, Bc, Cc, AB, CA, AE, EMOJI, EMPTY, JOIN, A10, CH0 = 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14
NCH = 8
L_ROW = 80                                     # tokens per row in the counting cases: 16 long words + 63 letters + EOS


@functools.lru_cache(maxsize=None)
def vocab():
    """The table of the kernel cases: the letters a, b, c, words that exercise the surface rules, and eight 64-character words
    over a, b, c (ids CH0 ..), so that a row of any length up to the limit fits 80 tokens."""
    from vagnmt_hip.surface import Surface
    g = np.random.default_rng(1)
    words = ["<pad>", "<unk>", "<s>", "</s>", "a", "b", "c", "ab@@", "c a", "ä", "\U0001F600", "", "@@", "a" * 10]
    words += ["".join(g.choice(list("abc"), size=64)) for _ in range(NCH)]
    return Surface(words)


def cmax():
    from vagnmt_hip import _lib
    return int(_lib.lib().vag_chrf_max_chars())


def row_of(n, g, L=L_ROW):
    """A token row whose surface has exactly n characters over a, b, c: n // 64 long words, n % 64 letters (shuffled), EOS, padding."""
    toks = list(g.integers(CH0, CH0 + NCH, size=n // 64)) + list(g.integers(A, Cc + 1, size=n % 64))
    g.shuffle(toks)
    assert len(toks) < L
    return [int(t) for t in toks] + [EOS] + [0] * (L - len(toks) - 1)


def bits(t):
    return t.contiguous().view(torch.int32)


def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def strings(table, rows):
    return [[table.text(r) for r in sent] for sent in rows]


def check_select(table, hyps, refs=None, weights=None):
    """mbr_select(utility="chrf") on token lists against the restatement: counts, lengths, utilities, expected, best.  Returns
    (Selected, util, matches) for what a caller adds."""
    from vagnmt_hip.mbr import mbr_select
    ht = torch.tensor(hyps, dtype=torch.int64, device="cuda")
    rt = None if refs is None else torch.tensor(refs, dtype=torch.int64, device="cuda")
    sel, (util, matches, lens) = mbr_select(ht, rt, weights, utility="chrf", surface=table, return_utilities=True)
    torch.cuda.synchronize()
    hs = strings(table, hyps)
    rs = hs if refs is None else strings(table, refs)
    Ch, Cr = lens.limit
    assert Ch == min(cmax(), ht.shape[2] * table.max_len) and Cr == (Ch if refs is None else min(cmax(), rt.shape[2] * table.max_len))
    assert lens.hyps.tolist() == [[len(s) for s in sent] for sent in hs]                  # the TRUE counts, cut or not
    assert lens.refs.tolist() == [[len(s) for s in sent] for sent in rs]
    m, u32, u64 = R.pairwise(hs, rs, Ch, Cr)
    B, Nh, Nr = u32.shape
    assert matches.shape == (B, Nh, Nr, 6) and matches.dtype == torch.int32 and util.shape == (B, Nh, Nr)
    assert np.array_equal(matches.cpu().numpy(), m), np.argwhere(matches.cpu().numpy() != m)[:5]
    got = util.cpu().numpy()
    print("[chrf] max |u - float64| %.3e over %d pairs" % (np.abs(got.astype(np.float64) - u64).max(), got.size))
    assert np.array_equal(fbits(got), fbits(u32)), np.argwhere(fbits(got) != fbits(u32))[:5]
    assert np.abs(got.astype(np.float64) - u64).max() <= 1e-6
    if weights is None:
        w = np.full((B, Nr), np.float32(1) / np.float32(Nr), dtype=np.float32)
    else:                                                                                  # as select_args normalises them
        wt = weights.to(torch.float32)
        w = (wt / wt.sum(1, keepdim=True)).cpu().numpy()
    e = R.expected(w, u32)
    assert np.array_equal(fbits(sel.expected.cpu().numpy()), fbits(e))
    assert sel.index.tolist() == R.first_argmax(e)
    assert sel.best == [hyps[b][i][:hyps[b][i].index(EOS)] for b, i in enumerate(sel.index.tolist())]      # from the token rows
    return sel, util, matches


# ------------------------------------------------------------------------------------------------------------------
# 1. the expansion
# ------------------------------------------------------------------------------------------------------------------
def run_expand(table, rows, C):
    t = torch.tensor(rows, dtype=torch.int64, device="cuda")
    out, lens = table.expand(t, C)
    torch.cuda.synchronize()
    assert out.shape == (len(rows), C) and out.dtype == torch.int32 and lens.shape == (len(rows),) and lens.dtype == torch.int32
    out, lens = out.cpu().tolist(), lens.cpu().tolist()
    for r, row in enumerate(rows):
        s = table.text(row)
        assert lens[r] == len(s), (r, row, lens[r], s)
        n = min(len(s), C)
        assert out[r][:n] == [ord(c) for c in s[:n]], (r, row)
    return lens


def test_expansion():
    table = vocab()
    C = 12
    rows = [[EOS, A, Bc, Cc, A, Bc],                # EOS at position 0
            [A, Bc, Cc, AB, CA, AE],                # no EOS: the whole row
            [A, 0, Bc, EOS, Cc, Cc],                # the padding word inside the span: an ordinary token (empty surface here)
            [A, EMPTY, JOIN, Bc, EOS, A],           # tokens with an empty surface
            [AE, EMOJI, A, EOS, 0, 0],              # a 2-byte and a 4-byte UTF-8 character: one code point each
            [A10, Bc, Cc, EOS, 0, 0],               # exactly C characters
            [A10, Bc, Cc, A, EOS, 0],               # C + 1: lens true, content cut
            [1, 2, A, EOS, 0, 0],                   # UNK keeps its string, SOS is empty
            [A10, A10, A10, A10, A10, A10]]         # far beyond C
    lens = run_expand(table, rows, C)
    assert lens == [0, 8, 2, 2, 3, 12, 13, 6, 60]
    assert run_expand(table, [[A], [EOS], [0], [A10]], 4) == [1, 0, 0, 10]      # L = 1
    # more than one chunk of 64 tokens: the running offset crosses chunks, the EOS lies in the second one, long words in both
    g = np.random.default_rng(2)
    long_rows = [[int(t) for t in g.integers(A, CH0 + NCH, size=130)] for _ in range(5)]
    long_rows[1][100] = EOS
    long_rows[2][64] = EOS
    long_rows[3][63] = EOS
    run_expand(table, long_rows, cmax())
    run_expand(table, long_rows, 1)


# ------------------------------------------------------------------------------------------------------------------
# 2. counts, utilities, expected, best
# ------------------------------------------------------------------------------------------------------------------
def test_counts_and_utilities_at_every_length():
    table = vocab()
    g = np.random.default_rng(3)
    M = cmax()
    hl = [[0, 1, 5, 6, 63], [64, 65, 128, 129, M]]
    rl = [[5, 64, M], [0, 129, 65]]
    hyps = [[row_of(n, g) for n in sent] for sent in hl]
    refs = [[row_of(n, g) for n in sent] for sent in rl]
    check_select(table, hyps, refs)
    check_select(table, [s[::-1] for s in hyps[::-1]], [s[::-1] for s in refs])          # every length against the others


def test_clipping_and_truncation():
    table = vocab()
    g = np.random.default_rng(4)
    M = cmax()
    a70 = [A10] * 7 + [EOS] + [0] * (L_ROW - 8)                                            # one character, 70 times
    hyps = [[a70, row_of(10, g), row_of(7, g), row_of(200, g), row_of(M + 1, g)],
            [row_of(M + 1, g), row_of(M - 1, g), a70, row_of(3, g), row_of(66, g)]]
    pad = lambda t: t + [EOS] + [0] * (L_ROW - len(t) - 1)                                 # noqa: E731
    refs = [[pad([A, Bc, A, Cc, A]), pad([A, A, A, Bc]), row_of(30, g)],                   # hold "a" three times
            [row_of(M + 1, g), pad([A, A, A]), row_of(M, g)]]
    sel, util, matches = check_select(table, hyps, refs)
    m = matches.cpu().numpy()
    assert m[0, 0, 0].tolist() == [3, 0, 0, 0, 0, 0] and m[0, 0, 1].tolist() == [3, 2, 1, 0, 0, 0]
    assert m[1, 2, 1].tolist() == [3, 2, 1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------
# 3. self-reference, weights, ties, determinism
# ------------------------------------------------------------------------------------------------------------------
def test_self_reference_weights_ties_and_determinism():
    from vagnmt_hip.mbr import mbr_select
    table = vocab()
    g = np.random.default_rng(5)
    lens = [[0, 1, 7, 64, 130], [5, 6, 65, 129, 300]]
    hyps = [[row_of(n, g) for n in sent] for sent in lens]
    sel, util, matches = check_select(table, hyps)                                        # refs=None: their own references
    m, u = matches.cpu().numpy(), util.cpu().numpy()
    for b in range(2):
        for i, n in enumerate(lens[b]):
            assert m[b, i, i].tolist() == R.totals(n) and u[b, i, i] == (1.0 if n else 0.0)    # the diagonal: m_n = T_n
    assert np.array_equal(m, m.transpose(0, 2, 1, 3))                                     # m_n is symmetric
    # given weights, one of them zero; normalised per sentence by the Python entry
    w = torch.tensor([[0.5, 0.0, 2.0, 0.25, 1.0], [3.0, 1.0, 1.0, 0.125, 0.7]], device="cuda")
    check_select(table, hyps, None, w)
    refs = [[row_of(n, g) for n in (9, 64, 70)] for _ in range(2)]
    check_select(table, hyps, refs, w[:, :3].contiguous())
    # a tie: candidates 1 and 3 are the same row, and the best one: the lowest index wins
    s = row_of(40, g)
    tie_h = [[row_of(40, g), s, row_of(12, g), s, row_of(41, g)], [s, row_of(5, g), s, row_of(40, g), row_of(6, g)]]
    tie_r = [[s, s, s], [s, s, s]]
    sel, util, _ = check_select(table, tie_h, tie_r)
    e = sel.expected.cpu().numpy()
    assert sel.index.tolist() == [1, 0] and e[0, 1] == e[0, 3] == e[0].max() and e[1, 0] == e[1, 2] == e[1].max()
    # two runs give the same bits
    ht = torch.tensor(hyps, dtype=torch.int64, device="cuda")
    a = mbr_select(ht, utility="chrf", surface=table, return_utilities=True)
    b = mbr_select(ht, utility="chrf", surface=table, return_utilities=True)
    assert torch.equal(bits(a[1][0]), bits(b[1][0])) and torch.equal(bits(a[0].expected), bits(b[0].expected))
    assert torch.equal(a[1][1], b[1][1]) and torch.equal(a[0].index, b[0].index)
    # without the per-pair outputs: the same expected and best
    c = mbr_select(ht, utility="chrf", surface=table)
    assert torch.equal(bits(c.expected), bits(a[0].expected)) and torch.equal(c.index, a[0].index) and c.best == a[0].best


def test_token_bleu_and_chrf_choose_differently():
    """Two segmentations of one string: x = "ab@@ c ab@@ c" and y = "a b c a b c" spell "abcabc".  Against the reference y,
    token BLEU prefers z = "a b c a b b" (five of six words) to x (two of four); chrF rates x 1.0 and prefers it."""
    from vagnmt_hip.mbr import mbr_select
    table = vocab()
    x, y, z = [AB, Cc, AB, Cc, EOS, 0, 0], [A, Bc, Cc, A, Bc, Cc, EOS], [A, Bc, Cc, A, Bc, Bc, EOS]
    assert table.text(x) == table.text(y) == "abcabc" and table.text(z) == "abcabb"
    hyps = torch.tensor([[x, z]], dtype=torch.int64, device="cuda")
    refs = torch.tensor([[y]], dtype=torch.int64, device="cuda")
    by_bleu = mbr_select(hyps, refs, utility="bleu")
    by_chrf, (util, matches, _) = mbr_select(hyps, refs, utility="chrf", surface=table, return_utilities=True)
    assert by_bleu.index.tolist() == [1] and by_bleu.best == [z[:6]]
    assert by_chrf.index.tolist() == [0] and by_chrf.best == [x[:4]]
    assert util[0, 0, 0].item() == 1.0 and matches[0, 0, 0].tolist() == [6, 5, 4, 3, 2, 1] and util[0, 1, 0].item() < 1.0
    xy = mbr_select(torch.tensor([[x, y]], dtype=torch.int64, device="cuda"), utility="chrf", surface=table, return_utilities=True)
    assert xy[1][0].flatten().tolist() == [1.0] * 4                                       # they rate each other 1.0
    # the host path refuses an id the table does not hold, on either side, before any launch
    bad = torch.tensor([[[A, table.V, EOS, 0, 0, 0, 0], z]], dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="hyps holds id %d" % table.V):
        mbr_select(bad, refs, utility="chrf", surface=table)
    with pytest.raises(ValueError, match="refs holds id %d" % table.V):
        mbr_select(hyps, bad, utility="chrf", surface=table)
    assert mbr_select(bad, refs, utility="bleu").index.tolist() == [1]                   # (no table, no bound)


# ------------------------------------------------------------------------------------------------------------------
# 4. mbr_decode
# ------------------------------------------------------------------------------------------------------------------
def model_table(V):
    """A surface for a model's V target ids: pseudo-words over five letters, a third of them BPE continuations."""
    from vagnmt_hip.surface import Surface
    g = np.random.default_rng(6)
    words = ["<pad>", "<unk>", "<s>", "</s>"]
    for i in range(4, V):
        w = "".join(g.choice(list("abcde"), size=int(g.integers(1, 7))))
        words.append(w + "@@" if i % 3 == 0 else w)
    return Surface(words)


@pytest.mark.parametrize("name", ["text", "ens3"])
def test_mbr_decode(name):
    from test_gpu_mbr import same, subject
    from test_gpu_stochastic import same as same_sbs
    from vagnmt_hip.mbr import mbr_select
    from vagnmt_hip.sampling import Generator
    ML, n = 10, 6
    obj, src, lens, im, nbest, _ = subject(name)
    table = model_table(getattr(obj, "models", [obj])[0].tgt_size)
    B = src.shape[0]
    kw = dict(n_samples=n, max_length=ML, temperature=0.9, top_k=10, top_p=0.95)
    gen = Generator(77)
    st = gen.get_state()
    drawn = obj.sample_decode(src, lens, im, generator=gen, **kw)
    gen.set_state(st)
    best, sel, smp = obj.mbr_decode(src, lens, im, utility="chrf", surface=table, generator=gen, **kw)       # from_history
    assert gen.get_state() == [st[0], st[1] + 1] and same(drawn, smp)
    want = mbr_select(drawn.hyps, utility="chrf", surface=table)
    assert torch.equal(sel.index, want.index) and best == want.best == sel.best
    assert torch.equal(bits(sel.expected), bits(want.expected)) and sel.expected.shape == (B, n)
    by_bleu = obj.mbr_decode(src, lens, im, utility="bleu", generator=Generator(77), **kw)[1]
    assert not torch.equal(bits(by_bleu.expected), bits(sel.expected))                   # another utility, other numbers
    gen.set_state(st)                                                                     # with the beam's list
    best3, sel3, smp3 = obj.mbr_decode(src, lens, im, utility="chrf", surface=table, beam_size=3, generator=gen, **kw)
    assert same(drawn, smp3) and sel3.expected.shape == (B, n + 3)
    cands = [drawn.hyps[b] + nbest(3, ML)[0][b] for b in range(B)]
    want3 = mbr_select(cands, refs=drawn.hyps, utility="chrf", surface=table)
    assert torch.equal(sel3.index, want3.index) and torch.equal(bits(sel3.expected), bits(want3.expected))
    assert best3 == [cands[b][int(sel3.index[b])] for b in range(B)] == sel3.best
    assert torch.equal(bits(sel3.expected[:, :n]), bits(sel.expected))
    gen.set_state(st)                                                                     # without replacement: importance weights
    s = obj.beamsearch_stochastic(src, lens, im, n_samples=n, max_length=ML, generator=gen)
    gen.set_state(st)
    bestw, selw, drawnw = obj.mbr_decode(src, lens, im, n_samples=n, max_length=ML, without_replacement=True, utility="chrf",
                                         surface=table, generator=gen)
    assert same_sbs(s, drawnw)
    wantw = mbr_select(s.hyps, weights=torch.exp(s.log_weight), utility="chrf", surface=table)
    assert torch.equal(selw.index, wantw.index) and torch.equal(bits(selw.expected), bits(wantw.expected))
    assert bestw == selw.best == [s.hyps[b][int(selw.index[b])] for b in range(B)]


# ------------------------------------------------------------------------------------------------------------------
# 5. minimum-risk training on the chrF cost
# ------------------------------------------------------------------------------------------------------------------
def test_mrt_step_on_the_chrf_cost():
    import mrt_ref
    from test_gpu_golden import close
    from test_gpu_mrt import _golden_driver
    from vagnmt_hip import mrt
    Lc = mrt_ref.LEARN
    meta, z, m, ts, (src, lens, tgt, im) = _golden_driver(Lc["golden"], lr=Lc["lr"], use_graph=False, pad_src=1)
    V = meta["dims"][1]
    table = model_table(V)
    cand_np = mrt_ref.learn_candidates(z["tgt"], V)
    cand = torch.from_numpy(cand_np).to("cuda")
    B = src.shape[0]
    # the costs: 1 - chrF of every packed row against the gold row
    rows, valid, cost, N, src_r, len_r, _ = mrt._prepare(src, lens, tgt, None, cand, 1, table)
    torch.cuda.synchronize()
    rows_np, valid_np = mrt_ref.pack(cand_np, z["tgt"], True)
    assert np.array_equal(rows.cpu().numpy(), rows_np) and np.array_equal(valid.cpu().numpy(), valid_np)
    want_cost = np.zeros(B * N, dtype=np.float32)
    for i, row in enumerate(rows_np):
        h, r = table.text(row), table.text(z["tgt"][i // N])
        want_cost[i] = np.float32(1) - R.utility32(R.matches(h, r), len(h), len(r))
    assert np.array_equal(fbits(cost.cpu().numpy()), fbits(want_cost))
    assert want_cost.reshape(B, N)[:, 0].tolist() == [0.0] * B and 0.0 < want_cost.max() <= 1.0     # gold against itself; the rest costs
    bleu_cost = mrt._prepare(src, lens, tgt, None, cand, 1)[2]
    assert not torch.equal(bits(bleu_cost), bits(cost))
    # the risk: the reference's formula on score_translations' log-probabilities and those costs
    m.eval()
    s = m.score_translations(src_r, [int(v) for v in len_r.tolist()], rows).logp.double().cpu()
    want = float(mrt_ref.risk_torch(s, want_cost, valid_np, N, Lc["alpha"]))
    got = mrt.expected_risk(ts, src, lens, tgt, im, cand, Lc["alpha"], cost="chrf", surface=table)
    print("[chrf mrt] expected_risk %.7f, reference %.7f" % (float(got), want))
    close(got, want, what="expected_risk on the chrF cost")
    # cost="bleu" is the call without the argument, bit for bit
    a = mrt.expected_risk(ts, src, lens, tgt, im, cand, Lc["alpha"])
    b = mrt.expected_risk(ts, src, lens, tgt, im, cand, Lc["alpha"], cost="bleu")
    assert torch.equal(bits(a.reshape(1)), bits(b.reshape(1))) and float(a) != float(got)
    # a step on it reports the risk before its update, and moves it
    out = ts.mrt_step(src, lens, tgt, im, alpha=Lc["alpha"], candidates=cand, cost="chrf", surface=table)
    after = mrt.expected_risk(ts, src, lens, tgt, im, cand, Lc["alpha"], cost="chrf", surface=table)
    torch.cuda.synchronize()
    ts.check()
    assert float(out.risk) == pytest.approx(float(got), abs=2e-6) and float(out.bleu) == pytest.approx(1.0 - float(got), abs=2e-6)
    assert float(after) < float(got)
