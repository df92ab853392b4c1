"""GPU: validation on the device -- vag_corpus_bleu_stats, vagnmt_hip.validate (BleuStats / corpus_bleu, ChrfStats / corpus_chrf,
validate) and TrainStep.eval_loss -- against the plain Python restatement of the definitions (tests/validate_ref.py) and the fixture
recorded from the reference's bleu.py (tests/golden/corpus_bleu.npz).

1. exact stats: per_sentence and totals equal the restatement integer for integer -- Lh, Lr in {1, 3, 4, 63, 64, 65, 80} with
   Lh != Lr (the walk goes in chunks of 64 positions and reads references four tokens at a time), R in {1, 2, 4, 5, 8} (four waves:
   at R = 5 one wave takes two references), N in {1, 3, 33}, n_refs NULL / constant / varying with the unused rows holding copies
   of the hypothesis, the row kinds of test_gpu_mbr.make_rows, and the hand case where the merged clipping differs from every
   single reference;
2. accumulation: totals pre-filled with 7 s come back as 7 + the sums, two adds equal one add of the concatenation, two runs agree
   bitwise, every output keeps its guard margin (every ABI call of this file goes through the guarded helper);
3. the fixture: corpus_bleu gives the recorded integers exactly and the recorded floats within 1e-12 relative (the same doubles
   in the same order; the margin allows for a log / exp that differs in the last place), both smooth values;
4. corpus_chrf equals the restatement's float64 value exactly (the device supplies only integers);
5. -EINVAL at the ABI;
6. eval_loss against the module's own eval-mode forward within test_gpu_golden.close (TOL = 1e-4, the suite's fp32 bound between
   these two paths), eager, captured and replayed; training with and without interleaved eval_loss calls ends bitwise equal;
7. validate on a tiny golden model and a 3-member Ensemble, eager and graph mode."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from conftest import GOLDEN, load_golden
from test_gpu_golden import build, close, criteria
from test_gpu_mbr import golden_model, make_rows

pytestmark = pytest.mark.gpu

EOS = 3
GUARD = 64
LS = [1, 3, 4, 63, 64, 65, 80]
RS = [1, 2, 4, 5, 8]
NS = [1, 3, 33]
RTOL = 1e-12


# ------------------------------------------------------------------------------------------------------------------
# the guarded call
# ------------------------------------------------------------------------------------------------------------------
def stats(hyps, refs, n_refs=None, fill=0, want_ps=True, totals=None):
    """vag_corpus_bleu_stats at the ABI, every output inside a guard margin that must come back untouched.  Returns (per_sentence
    (N, 10) or None, totals (10,)) as CPU tensors; totals start at `fill`, or continue from a guarded buffer of an earlier call."""
    from vagnmt_hip._lib import call, ptr, stream
    h = torch.as_tensor(hyps).cuda().contiguous()
    r = torch.as_tensor(refs).cuda().contiguous()
    n = None if n_refs is None else torch.as_tensor(n_refs, dtype=torch.int32).cuda().contiguous()
    N, Lh = h.shape
    _, Rr, Lr = r.shape
    ps = torch.full((N * 10 + 2 * GUARD,), -77, dtype=torch.int32, device="cuda") if want_ps else None
    tot = torch.full((10 + 2 * GUARD,), -77, dtype=torch.int64, device="cuda")
    tot[GUARD:-GUARD] = fill if totals is None else totals.cuda()
    call("vag_corpus_bleu_stats", ptr(h, torch.int64), ptr(r, torch.int64), ptr(n, torch.int32), N, Lh, Rr, Lr,
         None if ps is None else ps[GUARD:-GUARD].data_ptr(), tot[GUARD:-GUARD].data_ptr(), stream())
    torch.cuda.synchronize()
    for name, v in (("per_sentence", ps), ("totals", tot)):
        if v is not None:
            assert bool((v[:GUARD] == -77).all()) and bool((v[-GUARD:] == -77).all()), "guard of %s overwritten" % name
    return (None if ps is None else ps[GUARD:-GUARD].reshape(N, 10).cpu()), tot[GUARD:-GUARD].cpu()


def corpus(seed, N, Lh, R_, Lr, V, mode):
    """Hypotheses (N, Lh), references (N, R, Lr) of make_rows' kinds over one vocabulary, and n_refs by mode: None, "const" or
    "vary"; the reference rows beyond n_refs hold copies of the hypothesis."""
    hyps = make_rows(seed, N, 1, Lh, V)[:, 0]
    refs = make_rows(seed + 1, N, R_, Lr, V)
    g = np.random.default_rng(seed + 2)
    n_refs = None
    if mode == "const":
        n_refs = np.full(N, max(1, R_ - 1), dtype=np.int32)
    elif mode == "vary":
        n_refs = g.integers(1, R_ + 1, size=N).astype(np.int32)
    if n_refs is not None:
        w = min(Lh, Lr)
        for b in range(N):
            refs[b, n_refs[b]:, :w] = hyps[b, :w]
            if Lr > w:
                refs[b, n_refs[b]:, w] = EOS
    return hyps, refs, n_refs


# ------------------------------------------------------------------------------------------------------------------
# 1. exact stats
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lh", LS)
def test_stats_equal_the_restatement(Lh):
    i = LS.index(Lh)
    combos = unused = 0
    for ri, R_ in enumerate(RS):
        for ni, N in enumerate(NS):
            Lr = LS[(i + 1 + ri + ni) % len(LS)]
            if Lr == Lh:
                Lr = LS[(i + 3) % len(LS)]
            mode = (None, "const", "vary")[(ri + ni + i) % 3]
            V = (2, 6, 30)[(ri + 2 * ni + i) % 3]
            hyps, refs, n_refs = corpus(1000 * Lh + 10 * R_ + N, N, Lh, R_, Lr, V, mode)
            want_ps, want_tot = R.corpus_stats(hyps, refs, n_refs)
            ps, tot = stats(hyps, refs, n_refs)
            assert ps.tolist() == want_ps, (Lh, Lr, R_, N, mode, V)
            assert tot.tolist() == want_tot, (Lh, Lr, R_, N, mode, V)
            unused += n_refs is not None and R.corpus_stats(hyps, refs, None)[1] != want_tot
            combos += 1
    assert combos == 15 and unused >= 1                          # (the rows beyond n_refs would have counted)


@pytest.mark.parametrize("mode", [None, "const", "vary"])
def test_stats_every_n_refs_mode_at_the_chunk_edges(mode):
    """Each n_refs mode at the shapes where the code takes another path: a span that ends on, before and after a chunk of 64, R = 5
    and 8 (a wave with two references), more sentences than one."""
    for Lh, Lr, R_, N, V in ((64, 65, 5, 3, 2), (65, 63, 8, 33, 6), (80, 4, 4, 3, 2), (3, 80, 5, 33, 30), (63, 64, 2, 1, 6)):
        hyps, refs, n_refs = corpus(7 * Lh + Lr + R_, N, Lh, R_, Lr, V, mode)
        want_ps, want_tot = R.corpus_stats(hyps, refs, n_refs)
        ps, tot = stats(hyps, refs, n_refs)
        assert ps.tolist() == want_ps and tot.tolist() == want_tot, (Lh, Lr, R_, N, V)


def test_hand_cases():
    a, b = 4, 5
    # "a a b" against "a a" and "b b": merged clipping gives m_1 = 3, either reference alone 2 or 1
    hyp = np.array([[a, a, b, EOS]])
    refs = np.array([[[a, a, EOS, 0], [b, b, EOS, 0]]])
    ps, tot = stats(hyp, refs)
    assert ps.tolist() == [[3, 1, 0, 0, 3, 2, 1, 0, 3, 2]] == [R.sentence_stats([a, a, b], [[a, a], [b, b]])]
    assert tot.tolist() == ps[0].tolist()
    assert stats(hyp, refs[:, :1])[0][0, :4].tolist() == [2, 1, 0, 0] and stats(hyp, refs[:, 1:])[0][0, :4].tolist() == [1, 0, 0, 0]
    assert stats(hyp, refs, [1])[0].tolist() == stats(hyp, refs[:, :1])[0].tolist()
    # n_refs is clamped to [1, R] at the ABI
    assert stats(hyp, refs, [0])[0].tolist() == stats(hyp, refs, [1])[0].tolist()
    assert stats(hyp, refs, [9])[0].tolist() == ps.tolist()
    # an empty hypothesis, a row without EOS, a 0 inside the span, ids that differ only above bit 31
    ps, _ = stats(np.array([[EOS, a, a], [a, 0, a], [a + (1 << 32), b, EOS]]), np.array([[[a, a, a]], [[a, 0, EOS]], [[a, b + (1 << 33), EOS]]]))
    assert ps.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0, 3], [2, 1, 0, 0, 3, 2, 1, 0, 3, 2], [2, 1, 0, 0, 2, 1, 0, 0, 2, 2]]


# ------------------------------------------------------------------------------------------------------------------
# 2. accumulation, determinism, NULL per_sentence
# ------------------------------------------------------------------------------------------------------------------
def test_totals_accumulate():
    hyps, refs, n_refs = corpus(5, 33, 65, 5, 80, 2, "vary")
    want = R.corpus_stats(hyps, refs, n_refs)[1]
    ps, tot = stats(hyps, refs, n_refs, fill=7)
    assert tot.tolist() == [7 + x for x in want]
    ps2, tot2 = stats(hyps, refs, n_refs, fill=7)
    assert torch.equal(ps, ps2) and torch.equal(tot, tot2)
    none, tot3 = stats(hyps, refs, n_refs, fill=7, want_ps=False)
    assert none is None and torch.equal(tot, tot3)
    _, part = stats(hyps[:20], refs[:20], n_refs[:20])
    _, both = stats(hyps[20:], refs[20:], n_refs[20:], totals=part)
    assert both.tolist() == want
    # the Python layer: two add calls equal one call on the concatenation, per_sentence on request, lists as tensors
    from vagnmt_hip.validate import BleuStats
    h, r, n = torch.from_numpy(hyps).cuda(), torch.from_numpy(refs).cuda(), torch.from_numpy(n_refs).cuda()
    one, two = BleuStats("cuda"), BleuStats("cuda")
    assert one.add(h, r, n) is None
    got_ps = two.add(h[:20], r[:20], n[:20], per_sentence=True)
    two.add(h[20:], r[20:], n[20:])
    assert one.totals.tolist() == two.totals.tolist() == want and got_ps.cpu().tolist() == ps[:20].tolist()
    assert one.result() == two.result() and one.result(True).bleu == R.bleu_finish(want, True)[0]
    lists = BleuStats("cuda")
    lists.add([R.span(x) for x in hyps], [[R.span(x) for x in refs[b, :n_refs[b]]] for b in range(len(hyps))])
    assert lists.totals.tolist() == want
    one.reset()
    with pytest.raises(ValueError):
        one.result()


# ------------------------------------------------------------------------------------------------------------------
# 3. the fixture
# ------------------------------------------------------------------------------------------------------------------
def test_golden_corpora():
    from vagnmt_hip.validate import corpus_bleu
    z = np.load(os.path.join(GOLDEN, "corpus_bleu.npz"))
    for s in range(int(z["n_sets"])):
        h, r, n = (torch.from_numpy(z[k % s]).cuda() for k in ("hyps%d", "refs%d", "nrefs%d"))
        f, i = z["f%d" % s], z["i%d" % s]
        for k, smooth in enumerate((False, True)):
            got = corpus_bleu(h, r, n, smooth=smooth)
            assert (got.translation_length, got.reference_length) == (int(i[0]), int(i[1])), s
            flat = [got.bleu] + list(got.precisions) + [got.bp, got.ratio]
            for a, b in zip(flat, f[k]):
                assert abs(a - b) <= RTOL * abs(b), (s, smooth, flat, f[k])
            assert (got.bleu == 0.0) == (f[k][0] == 0.0)


# ------------------------------------------------------------------------------------------------------------------
# 4. corpus chrF
# ------------------------------------------------------------------------------------------------------------------
def test_corpus_chrf_equals_the_restatement():
    from vagnmt_hip.surface import Surface
    from vagnmt_hip.validate import ChrfStats, corpus_chrf
    g = np.random.default_rng(11)
    letters = "abcdeä"
    words = ["<pad>", "<unk>", "<s>", "</s>"] + ["".join(letters[int(c)] for c in g.integers(0, len(letters), size=1 + k % 9))
                                                   for k in range(36)]
    table = Surface(words)
    assert table.max_len == 9
    V, N, Lh, Lr = len(words), 9, 130, 140
    hyps = g.integers(4, V, size=(N, Lh)).astype(np.int64)
    refs = g.integers(4, V, size=(N, Lr)).astype(np.int64)
    for b in range(N):
        n = int(g.integers(2, 30))
        refs[b, :n] = hyps[b, :n]                              # shared beginnings: matches at every order
        hyps[b, int(g.integers(n, 40))] = EOS
        refs[b, int(g.integers(n, 40))] = EOS
    hyps[0] = 4 + np.argmax([len(w) for w in words[4:]])       # 130 words of 9 letters: 1170 characters, stored 1024
    refs[0] = hyps[0, 0]
    hyps[1, 0] = EOS                                           # an empty hypothesis
    lim_h, lim_r = table.row_chars(Lh), table.row_chars(Lr)
    assert lim_h == lim_r == 1024
    want = R.chrf_totals(hyps, refs, table.surfaces, lim_h, lim_r)
    assert want[6] > 1024 and want[0] > 0 and want[5] > 0
    st = ChrfStats("cuda", table)
    st.add(torch.from_numpy(hyps).cuda(), torch.from_numpy(refs).cuda())
    assert st.totals.tolist() == want
    got = corpus_chrf(torch.from_numpy(hyps).cuda(), torch.from_numpy(refs).cuda(), table)
    assert got == R.chrf_finish(want) == st.result() and 0.0 < got < 1.0
    st.add(torch.from_numpy(hyps[:3]).cuda(), torch.from_numpy(refs[:3, None]).cuda())           # (N, 1, Lr) is one reference each
    assert st.totals.tolist() == [a + b for a, b in zip(want, R.chrf_totals(hyps[:3], refs[:3], table.surfaces, lim_h, lim_r))]
    with pytest.raises(ValueError, match="single-reference"):
        st.add(torch.from_numpy(hyps[:3]).cuda(), torch.zeros(3, 2, 5, dtype=torch.int64, device="cuda"))
    assert corpus_chrf([[4, 5], [6]], [[4, 5], [6]], table) == 1.0


# ------------------------------------------------------------------------------------------------------------------
# 5. -EINVAL
# ------------------------------------------------------------------------------------------------------------------
def test_refused_arguments():
    from vagnmt_hip import _lib
    L = _lib.lib()
    h = torch.full((2, 8), 4, dtype=torch.int64, device="cuda")
    r = torch.full((2, 65, 8), 4, dtype=torch.int64, device="cuda")
    tot = torch.full((10,), 7, dtype=torch.int64, device="cuda")
    ps = torch.full((2, 10), -77, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = L.vag_corpus_bleu_stats
    assert st(None, p(r), None, 2, 8, 1, 8, p(ps), p(tot), None) == -22
    assert st(p(h), None, None, 2, 8, 1, 8, p(ps), p(tot), None) == -22
    assert st(p(h), p(r), None, 2, 8, 1, 8, p(ps), None, None) == -22
    for N, Lh, R_, Lr in ((0, 8, 1, 8), (2, 0, 1, 8), (2, 8, 0, 8), (2, 8, 1, 0), (2, 8, 65, 8), (2, 513, 1, 8), (2, 8, 1, 513),
                          (1 << 31, 8, 1, 8)):
        assert st(p(h), p(r), None, N, Lh, R_, Lr, p(ps), p(tot), None) == -22, (N, Lh, R_, Lr)
    torch.cuda.synchronize()
    assert bool((tot == 7).all()) and bool((ps == -77).all())              # a refused call touched nothing
    assert L.vag_corpus_bleu_supported(512, 64, 512) == 1 and L.vag_corpus_bleu_supported(513, 64, 512) == 0


# ------------------------------------------------------------------------------------------------------------------
# 6. eval_loss
# ------------------------------------------------------------------------------------------------------------------
def _own_forward(meta, P, batch, cm, cv, teacher):
    """The module's own forward in eval mode with the criteria, on a model of its own (the per-operator path)."""
    m = build(meta, P)
    src, lens, tgt, im = batch
    with torch.no_grad():
        if meta["kind"] == "mm":
            out = m(src, lens, tgt, im, 1.0 if teacher else 0.0, criterion_mt=cm, criterion_vse=cv)
            return [float(x) for x in out]
        loss = float(m(src, lens, tgt, 1.0 if teacher else 0.0, criterion=cm))
        return [loss, loss, 0.0]


def _batch(meta, z):
    src, tgt = torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["tgt"]).cuda()
    return src, meta["lengths"], tgt, (torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None)


@pytest.mark.parametrize("smoothed", [False, True], ids=["nll", "label_smoothed"])
@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32"])
def test_eval_loss_matches_the_per_operator_forward(name, smoothed):
    from test_gpu_label_smoothing import _crit, _generic_cls
    from vagnmt_hip.trainer import TrainStep, _FusedBackend
    meta, P, z = load_golden(name)
    cm, cv = criteria(meta)
    cv = cv if meta["kind"] == "mm" else None
    V = meta["dims"][1]
    cm_ref = cm
    if smoothed:
        cm, cm_ref = _crit(V, 0.1), _crit(V, 0.1, _generic_cls())       # the reference side takes the generic criterion path
    batch = _batch(meta, z)
    m = build(meta, P)
    ts = TrainStep(m, cm, cv, use_graph=True, capture_after=1, pad_src=1)
    assert type(ts.backend) is _FusedBackend
    m.train()
    for teacher in (True, False):
        want = _own_forward(meta, P, batch, cm_ref, cv, teacher)
        before = dict(ts.stats)
        flat, grad, count, version = ts.fp.flat.clone(), ts.fp.grad.clone(), int(ts.step_count.item()), getattr(m, "_vag_weights_version", 0)
        got = []
        for visit in range(3):                                 # eager, captured + replayed, replayed
            out = ts.eval_loss(*batch, teacher=teacher)
            got.append([float(x) for x in out])
            assert m.training is True                          # the flag is restored
        print("[eval_loss] %s smoothed=%s teacher=%s: %s vs per-operator %s" % (name, smoothed, teacher, got, want))
        assert ts.stats["eager_steps"] == before["eager_steps"] + 1 and ts.stats["captures"] == before["captures"] + 1 and \
            ts.stats["replays"] == before["replays"] + 2, ts.stats
        for g in got:
            for j, what in enumerate(("loss", "loss_mt", "loss_vse")):
                close(np.float64(g[j]), want[j], what="%s teacher=%s %s" % (name, teacher, what))
        assert got[1] == got[2]
        assert torch.equal(ts.fp.flat, flat) and torch.equal(ts.fp.grad, grad) and int(ts.step_count.item()) == count
        assert getattr(m, "_vag_weights_version", 0) == version
    assert all("eval" in k for k in ts._graphs)
    # an injected or per-operator backend has no eval_loss
    ts2 = TrainStep(build(meta, P), cm_ref if smoothed else cm, cv, use_graph=False, fused=False)
    with pytest.raises(NotImplementedError):
        ts2.eval_loss(*batch)


def _twin(eval_between):
    """Three training steps (eager, captured, replayed) at dropout 0.3 from one seed, optionally an eval_loss on the same shape
    after every step.  The shape is the one test_gpu_label_smoothing documents as reproducible from driver to driver."""
    from test_gpu_label_smoothing import _model_case
    from vagnmt_hip.trainer import TrainStep
    m, batch, V = _model_case("text", dropout=0.3, B=2, Ts=4, Tt=3)
    vw = torch.ones(V, device="cuda")
    vw[0] = 0
    torch.manual_seed(77)                        # the dropout generator's seed is drawn on the first training step
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, use_graph=True, capture_after=1, pad_src=1, ema_decay=0.9)
    losses, evals = [], []
    for i in range(3):
        losses.append(torch.stack([v.clone() for v in ts.step(*batch, teacher=True)]))
        if eval_between:
            assert m.training
            evals.append(torch.stack([v.clone() for v in ts.eval_loss(*batch)]))
            assert m.training
    torch.cuda.synchronize()
    ts.check()
    return m, ts, batch, torch.stack(losses).cpu(), evals


def test_eval_loss_leaves_training_bitwise_alone():
    from test_gpu_label_smoothing import _model_case
    from vagnmt_hip.trainer import TrainStep
    m0, ts0, _, l0, _ = _twin(False)
    m1, ts1, batch, l1, evals = _twin(True)
    assert ts0.stats["captures"] == 1 and ts1.stats["captures"] == 2, (ts0.stats, ts1.stats)      # no graph shared
    assert sorted(len(k) for k in ts1._graphs) == [5, 5] and sum("eval" in k for k in ts1._graphs) == 1
    assert torch.equal(l0, l1) and l0[0, 0] != l0[1, 0]
    for name in ("flat", "m", "v", "ema"):
        a, b = getattr(ts0.fp, name), getattr(ts1.fp, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert int(ts0.step_count.item()) == int(ts1.step_count.item()) == 3
    assert m0._vag_weights_version == m1._vag_weights_version
    # dropout was off in every eval call: the loss after step i is a function of the weights alone, and differs from the training
    # loss of the next step on the same batch (which has dropout on)
    assert not torch.equal(evals[0], evals[1]) and not torch.equal(evals[1].cpu(), l1[2])
    # eval_loss after a captured training step of the same shape == eval_loss of a fresh driver on the same weights, bitwise
    mine = torch.stack([v.clone() for v in ts1.eval_loss(*batch)])
    fresh, _, V = _model_case("text", dropout=0.3, B=2, Ts=4, Tt=3)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m1.state_dict().items()})
    vw = torch.ones(V, device="cuda")
    vw[0] = 0
    tsf = TrainStep(fresh, torch.nn.NLLLoss(weight=vw, reduction="none"), None, use_graph=False, pad_src=1)
    theirs = torch.stack([v.clone() for v in tsf.eval_loss(*batch)])
    assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32)) and torch.equal(mine, evals[2]), (mine, theirs, evals[2])
    # allowed inside averaged_weights(), where it sees the averaged weights; the raw ones come back bit for bit
    flat = ts1.fp.flat.clone()
    with ts1.averaged_weights():
        inside = torch.stack([v.clone() for v in ts1.eval_loss(*batch)])
    assert torch.equal(ts1.fp.flat.view(torch.int32), flat.view(torch.int32)) and not torch.equal(inside, mine)
    assert torch.equal(torch.stack([v.clone() for v in ts1.eval_loss(*batch)]), mine)


# ------------------------------------------------------------------------------------------------------------------
# 7. validate
# ------------------------------------------------------------------------------------------------------------------
def _dev_set(m, kind, Vs, Vt, I, seed=5):
    """5 batches of 3 sentences of different widths; the targets are noisy copies of the model's own beam output, so that the
    n-gram statistics are not all zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(5):
        Ts = 4 + b
        lens = [Ts, max(1, Ts - 2), 2]
        src = torch.zeros(3, Ts, dtype=torch.int64)
        for i, n in enumerate(lens):
            src[i, :n] = torch.randint(4, Vs, (n,), generator=g)
        im = torch.randn(3, I, generator=g).abs().cuda() if kind != "text" else None
        src = src.cuda()
        hyp = m.beamsearch_decode(src, lens, 4, 12) if kind == "text" else m.beamsearch_decode(src, lens, im, 4, 12)
        Tt = 9 + b % 3
        tgt = torch.zeros(3, Tt, dtype=torch.int64)
        for i, row in enumerate(hyp):
            row = [t if float(torch.rand((), generator=g)) < 0.7 else int(torch.randint(4, Vt, (), generator=g)) for t in row][:Tt - 1]
            row = [t for t in row if t != 0] or [5]
            tgt[i, :len(row)] = torch.tensor(row)
            tgt[i, len(row)] = EOS
        out.append((src, lens, tgt.cuda(), im))
    return out


def _decode_lists(obj, kind, batches):
    return [row for src, lens, tgt, im in batches
            for row in (obj.beamsearch_decode(src, lens, 4, 12) if kind == "text" else obj.beamsearch_decode(src, lens, im, 4, 12))]


def _check_bleu(got, lists, batches):
    refs = [[row.tolist()] for _, _, tgt, _ in batches for row in tgt.cpu()]
    want = R.corpus_bleu(lists, refs)
    assert tuple(got) == (want[0], want[1], want[2], want[3], want[4], want[5]), (got, want)
    assert got.translation_length == sum(len(x) for x in lists) > 0 and sum(R.corpus_stats(lists, refs)[1][:2]) > 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["mm", "text"])
def test_validate_a_training_run(kind, graph):
    from vagnmt_hip.surface import Surface
    from vagnmt_hip.trainer import TrainStep
    from vagnmt_hip.validate import validate
    name = "mm_dot_tied_s0_f32" if kind == "mm" else "text_tied_s0_f32"
    meta, _, _ = load_golden(name)
    m, _, _, _ = golden_model(name, eos_bias=1.5 if kind == "mm" else -2.0)      # (the text model ends at once as it is: empty lists)
    m.decode_graph = graph
    Vs, Vt, I = meta["dims"][:3]
    batches = _dev_set(m, kind, Vs, Vt, I)
    cm, cv = criteria(meta)
    ts = TrainStep(m, cm, cv if kind == "mm" else None, lr=1e-2, use_graph=graph, capture_after=1, ema_decay=0.5)
    for _ in range(2):
        ts.step(*batches[0], teacher=True)
    assert m.training
    table = Surface(["<pad>", "<unk>", "<s>", "</s>"] + ["w%d" % (i * i) for i in range(4, Vt)])
    v = validate(ts, batches, beam_size=4, max_length=12, metrics=("loss", "bleu", "chrf"), surface=table, keep_translations=True)
    assert m.training and (v.n_sentences, v.n_batches) == (15, 5)
    m.eval()
    lists = _decode_lists(m, kind, batches)
    assert v.translations == lists
    _check_bleu(v.bleu, lists, batches)
    tgts = [row.tolist() for _, _, tgt, _ in batches for row in tgt.cpu()]
    assert v.chrf == R.chrf_finish(R.chrf_totals(lists, tgts, table.surfaces, 1024, 1024)) and v.chrf > 0.0
    acc = None
    for batch in batches:                                      # the mean of the per-batch values, summed as validate sums them
        out = torch.stack([x.clone() for x in ts.eval_loss(*batch)]).cpu()
        acc = out if acc is None else acc + out
    assert [v.loss, v.loss_mt, v.loss_vse] == [x / 5 for x in acc.tolist()] and v.loss_mt > 0.0
    # without the loss nothing of the step runs; a metric not asked for is None
    v2 = validate(ts, batches, beam_size=4, max_length=12, metrics=("bleu",))
    assert v2.loss is None and v2.chrf is None and v2.translations is None and v2.bleu == v.bleu
    # on the averaged weights: runs, sees other weights, and leaves the raw parameters bitwise intact
    flat = ts.fp.flat.clone()
    with ts.averaged_weights():
        va = validate(ts, batches, beam_size=4, max_length=12)
    assert torch.equal(ts.fp.flat.view(torch.int32), flat.view(torch.int32))
    assert va.loss_mt != v.loss_mt and va.bleu.reference_length == v.bleu.reference_length
    m.train()
    assert np.isfinite(float(ts.step(*batches[1], teacher=True)[0]))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_validate_an_ensemble_and_a_model(graph):
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.validate import validate
    meta, _, _ = load_golden("mm_dot_tied_s0_f32")
    m, _, _, _ = golden_model("mm_dot_tied_s0_f32", eos_bias=1.5)
    ens = Ensemble([m, golden_model("text_tied_s0_f32", eos_bias=-2.0)[0], golden_model("mm_dot_tied_s0_f32", eos_bias=0.5)[0]])
    ens.decode_graph = m.decode_graph = graph
    Vs, Vt, I = meta["dims"][:3]
    batches = _dev_set(m, "mm", Vs, Vt, I, seed=6)
    for obj in (ens, m):
        with pytest.raises(ValueError, match="dev loss"):
            validate(obj, batches, beam_size=4, max_length=12)
        v = validate(obj, batches, beam_size=4, max_length=12, metrics=("bleu",), keep_translations=True)
        lists = _decode_lists(obj, "mm", batches)
        assert v.translations == lists and v.loss is None and (v.n_sentences, v.n_batches) == (15, 5)
        _check_bleu(v.bleu, lists, batches)
    # multi-reference sets: refs yields (refs (B, R, Lr), n_refs) per batch
    multi = []
    for _, _, tgt, _ in batches:
        r = torch.stack([tgt, tgt.roll(1, 0)], 1).contiguous()
        multi.append((r, torch.tensor([2, 1, 2], dtype=torch.int32, device="cuda")))
    v = validate(m, batches, beam_size=4, max_length=12, metrics=("bleu",), refs=multi, keep_translations=True)
    refs = [[r[i, j].tolist() for j in range(int(n[i]))] for r, n in multi for i in range(3)]
    assert tuple(v.bleu) == tuple(R.corpus_bleu(v.translations, refs))
    # greedy (beam_size 1) keeps its rows on the device too
    v1 = validate(m, batches, beam_size=1, max_length=12, metrics=("bleu",), keep_translations=True)
    assert v1.translations == [row for src, lens, tgt, im in batches for row in m.beamsearch_decode(src, lens, im, 1, 12)]
