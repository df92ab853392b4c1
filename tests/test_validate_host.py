"""CPU: the validation layer's host side (vagnmt_hip.validate) -- the restatement (tests/validate_ref.py) and the library's host
finish against the fixture recorded from the reference's bleu.py (tests/golden/corpus_bleu.npz), Monitor against torch's
ReduceLROnPlateau, the new symbols, and the argument checks of the Python layer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from conftest import GOLDEN, ROOT

RTOL = 1e-12        # the same doubles in the same order: the margin only allows for a log / exp that differs in the last place


def golden_sets():
    z = np.load(os.path.join(GOLDEN, "corpus_bleu.npz"))
    return [(z["hyps%d" % s], z["refs%d" % s], z["nrefs%d" % s], z["f%d" % s], z["i%d" % s]) for s in range(int(z["n_sets"]))]


def check_six(got, f, i, what):
    bleu, p, bp, ratio, tl, rl = got
    assert (tl, rl) == (int(i[0]), int(i[1])), (what, tl, rl, i)
    for name, a, b in [("bleu", bleu, f[0]), ("bp", bp, f[5]), ("ratio", ratio, f[6])] + [("p%d" % (n + 1), p[n], f[1 + n]) for n in range(4)]:
        assert abs(a - b) <= RTOL * abs(b), (what, name, a, b)


def test_restatement_and_host_finish_reproduce_the_fixture():
    from vagnmt_hip.validate import CorpusBLEU, bleu_from_totals
    sets = golden_sets()
    assert len(sets) >= 10
    sizes, n_refs_seen, zero_geo = set(), set(), 0
    for s, (hyps, refs, n_refs, f, i) in enumerate(sets):
        sizes.add(len(hyps))
        n_refs_seen.update(int(x) for x in n_refs)
        per, totals = R.corpus_stats(hyps, refs, n_refs)
        assert totals[8] == sum(len(R.span(h)) for h in hyps)
        for k, smooth in enumerate((False, True)):
            check_six(R.bleu_finish(totals, smooth), f[k], i, "restatement set %d smooth %s" % (s, smooth))
            got = bleu_from_totals(totals, smooth)
            assert isinstance(got, CorpusBLEU)
            check_six(got, f[k], i, "bleu_from_totals set %d smooth %s" % (s, smooth))
        zero_geo += f[0][0] == 0.0 and i[0] > 0
    assert min(sizes) == 1 and max(sizes) == 40 and n_refs_seen == {1, 2, 3, 4, 5} and zero_geo >= 2
    # rows beyond n_refs hold copies of the hypothesis: reading them would change the counts of some set
    assert any(R.corpus_stats(h, r, None)[1] != R.corpus_stats(h, r, n)[1] for h, r, n, _, _ in sets)


def test_restatement_hand_cases():
    a, b = 4, 5
    # the merged clipping differs from every single reference: "a a b" against "a a" and "b b"
    assert R.sentence_stats([a, a, b], [[a, a], [b, b]]) == [3, 1, 0, 0, 3, 2, 1, 0, 3, 2]
    assert R.sentence_stats([a, a, b], [[a, a]])[:4] == [2, 1, 0, 0] and R.sentence_stats([a, a, b], [[b, b]])[:4] == [1, 0, 0, 0]
    assert R.sentence_stats([], [[a]]) == [0] * 8 + [0, 1]
    assert R.span([a, 0, b, 3, a, a]) == [a, 0, b] and R.span([a, b]) == [a, b] and R.span([3, a]) == []
    # an identical corpus scores 1; half the length scores bp = exp(1 - 2)
    assert R.corpus_bleu([[4, 5, 6, 7, 8, 3]], [[[4, 5, 6, 7, 8, 3]]])[0] == 1.0
    got = R.corpus_bleu([[4, 5, 6, 7, 3]], [[[4, 5, 6, 7, 8, 9, 10, 11]]])
    assert got[2] == pytest.approx(np.exp(-1.0), rel=1e-15) and got[1] == [1.0] * 4
    # the library's host finish on the same hand statistics, and its packing of the hand case's lists
    from vagnmt_hip.validate import bleu_args, bleu_from_totals
    assert tuple(bleu_from_totals(R.corpus_stats([[4, 5, 6, 7, 3]], [[[4, 5, 6, 7, 8, 9, 10, 11]]])[1])) == tuple(got)
    merged = bleu_from_totals(R.sentence_stats([a, a, b], [[a, a], [b, b]]))
    assert merged.precisions == [1.0, 0.5, 0.0, 0.0] and merged.bleu == 0.0 and (merged.translation_length, merged.reference_length) == (3, 2)
    h, r, n = bleu_args([[a, a, b]], [[[a, a], [b, b]]], device="cpu")
    assert h.tolist() == [[a, a, b, 3]] and r.tolist() == [[[a, a, 3], [b, b, 3]]] and n is None
    assert R.corpus_stats(h.tolist(), r.tolist())[0] == [[3, 1, 0, 0, 3, 2, 1, 0, 3, 2]]


def test_host_finish_errors_and_chrf_finish():
    from vagnmt_hip.validate import bleu_from_totals, chrf_from_totals
    with pytest.raises(ValueError):
        bleu_from_totals([0] * 10)                        # reference length 0: bleu.py divides by zero
    with pytest.raises(ValueError):
        bleu_from_totals([0] * 9)
    assert bleu_from_totals([0, 0, 0, 0, 0, 0, 0, 0, 0, 5]).bleu == 0.0          # only empty hypotheses: ratio 0, bp 0
    with pytest.raises(ValueError):
        chrf_from_totals([0] * 17)
    assert chrf_from_totals([0] * 18) == 0.0
    assert chrf_from_totals([0] * 6 + [5, 4, 3, 2, 1, 0] + [5, 4, 3, 2, 1, 0]) == 0.0           # P + R = 0
    surf = {4: "ab", 5: "cab", 6: ""}
    hyps, refs = [[4, 5, 3], [6, 3], [5, 5, 5, 3]], [[5, 4, 3], [4, 3], [5, 3, 5]]
    t = R.chrf_totals(hyps, refs, surf, 1024, 1024)
    assert t[6] == 5 + 0 + 9 and t[12] == 5 + 2 + 3 and t[11] == 0 + 0 + 4 and t[17] == 0           # "abcab", "", "cabcabcab" / "cabab", "ab", "cab"
    assert chrf_from_totals(t) == R.chrf_finish(t) and 0.0 < R.chrf_finish(t) < 1.0
    same = R.chrf_totals(hyps, hyps, surf, 1024, 1024)
    assert R.chrf_finish(same) == 1.0 == chrf_from_totals(same)
    cut = R.chrf_totals([[5] * 10], [[5] * 10], surf, 7, 1024)                    # a stored row is cut to its limit
    assert cut[6] == 7 and cut[12] == 30


class _Lr:
    """What Monitor.update needs of a TrainStep."""
    def __init__(self, lr):
        self.lr, self.calls = lr, 0

    def set_lr(self, lr):
        self.lr, self.calls = float(lr), self.calls + 1


def _losses():
    g = np.random.default_rng(20261020)
    x, cur = [], 5.0
    for i in range(60):
        kind = i % 6
        if kind == 0:
            cur *= float(g.uniform(0.9, 0.99))                   # a real improvement
        elif kind == 1 and x:
            cur = x[-1]                                          # an equal value
        elif kind == 2:
            cur = min(x) * (1.0 - 0.5e-4)                        # better, but inside the relative threshold 1e-4
        else:
            cur = min(x) * float(g.uniform(1.0, 1.3))            # worse
        x.append(float(cur))
    return x


@pytest.mark.parametrize("lr_patience,factor,min_lr", [(2, 0.2, 0.0), (0, 0.5, 1e-3), (3, 0.1, 1e-5)])
def test_monitor_follows_reduce_lr_on_plateau(lr_patience, factor, min_lr):
    from vagnmt_hip.validate import Monitor, Validation
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.01)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=factor, patience=lr_patience, min_lr=min_lr)
    mon, ts = Monitor(patience=1000, lr_factor=factor, lr_patience=lr_patience, min_lr=min_lr), _Lr(0.01)
    seq = _losses()
    assert any(a == b for a, b in zip(seq, seq[1:])) and len(seq) == 60
    drops, prev = 0, 0.01
    for i, loss in enumerate(seq):
        sched.step(loss)
        v = mon.update(ts, Validation(loss, loss, 0.0, None, None, 3, 1, None))
        want = opt.param_groups[0]["lr"]
        assert v.lr == want == ts.lr, (i, v.lr, want)
        assert mon.num_bad == sched.num_bad_epochs and mon.plateau_best == sched.best, i
        assert v.best_loss == (loss < min(seq[:i] + [float("inf")])) and v.best_bleu is False and v.stop is False
        drops += want < prev
        prev = want
    assert drops >= 2 and ts.calls == 60


def test_monitor_patience_flags_and_state_round_trip():
    from vagnmt_hip.validate import CorpusBLEU, Monitor, Validation
    def val(loss, b):             # noqa: E306
        return Validation(loss, loss, 0.0, CorpusBLEU(b, [0.0] * 4, 1.0, 1.0, 1, 1), None, 3, 1, None)
    bleus = [0.10, 0.20, 0.20, 0.15, 0.25, 0.1, 0.1, 0.1]
    losses = [3.0, 2.0, 2.5, 1.5, 1.5, 1.6, 1.7, 1.8]
    want_bleu = [True, True, False, False, True, False, False, False]
    want_loss = [True, True, False, True, False, False, False, False]
    left = [3, 3, 2, 1, 3, 2, 1, 0]
    mon, ts = Monitor(patience=3, lr_factor=0.5, lr_patience=1), _Lr(1.0)
    verdicts, half, lr_half = [], None, None
    for i in range(8):
        v = mon.update(ts, val(losses[i], bleus[i]))
        assert (v.best_bleu, v.best_loss, mon.patience_left, v.stop) == (want_bleu[i], want_loss[i], left[i], i == 7), i
        verdicts.append(v)
        if i == 3:
            half, lr_half = dict(mon.state_dict()), ts.lr
    assert ts.lr < 1.0                                   # the plateau rule acted (losses 1.5, 1.6, 1.7 after the best 1.5)
    # a resumed run keeps its counters: a monitor built with other settings, loaded at update 4, goes on as the original did
    twin, ts2 = Monitor(patience=99, lr_factor=0.9, lr_patience=7), _Lr(lr_half)
    twin.load_state_dict(half)
    for i in range(4, 8):
        assert twin.update(ts2, val(losses[i], bleus[i])) == verdicts[i], i
    assert twin.state_dict() == mon.state_dict() and ts2.lr == ts.lr
    with pytest.raises(ValueError):
        Monitor().load_state_dict({"patience": 3})
    for bad in (dict(patience=0), dict(lr_factor=1.0), dict(lr_factor=0.0), dict(min_lr=-1.0), dict(lr_patience=-1)):
        with pytest.raises(ValueError):
            Monitor(**bad)
    # without a loss the rate is left alone; without a TrainStep nothing is called
    m = Monitor()
    v = m.update(None, Validation(None, None, None, CorpusBLEU(0.3, [0.0] * 4, 1.0, 1.0, 1, 1), None, 3, 1, None))
    assert v == (False, True, None, False)


def test_symbols_exported_and_declared():
    from vagnmt_hip import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    for name in ("vag_corpus_bleu_supported", "vag_corpus_bleu_stats"):
        assert name in _lib.PROTOS and hasattr(L, name) and ("int %s(" % name) in header, name
    assert L.vag_corpus_bleu_supported(1, 1, 1) == 1 and L.vag_corpus_bleu_supported(512, 64, 512) == 1
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (513, 1, 8), (8, 65, 8), (8, 1, 513)):
        assert L.vag_corpus_bleu_supported(*bad) == 0, bad
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    st = L.vag_corpus_bleu_stats
    # argument errors come back as -EINVAL before anything touches a device (the pointers are never dereferenced)
    assert st(None, p, None, 1, 8, 1, 8, None, p, None) == -22                   # hyps NULL
    assert st(p, None, None, 1, 8, 1, 8, None, p, None) == -22                   # refs NULL
    assert st(p, p, None, 1, 8, 1, 8, p, None, None) == -22                      # totals NULL
    for N, Lh, R_, Lr in ((0, 8, 1, 8), (1, 0, 1, 8), (1, 8, 0, 8), (1, 8, 1, 0), (1, 8, 65, 8), (1, 513, 1, 8), (1, 8, 1, 513),
                          (1 << 31, 8, 1, 8)):
        assert st(p, p, None, N, Lh, R_, Lr, None, p, None) == -22, (N, Lh, R_, Lr)
    import train
    from vagnmt_hip import validate as V
    assert train.validate is V.validate and train.Monitor is V.Monitor


def test_python_layer_argument_errors():
    from vagnmt_hip import validate as V
    from vagnmt_hip.surface import Surface
    cpu = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU tensor"):
        V.bleu_args(cpu, [[4], [5]], device="cpu")
    with pytest.raises(ValueError, match="empty"):
        V.bleu_args([], [], device="cpu")
    # token lists are packed as mbr.pack packs a row; nothing below needs a device
    h, r, n = V.bleu_args([[4, 5], [6]], [[[4, 5], [4]], [[6, 3, 9]]], device="cpu")
    assert h.tolist() == [[4, 5, 3], [6, 3, 0]] and r.shape == (2, 2, 3) and n.tolist() == [2, 1] and n.dtype == torch.int32
    assert r[0].tolist() == [[4, 5, 3], [4, 3, 0]] and r[1].tolist() == [[6, 3, 9], [3, 0, 0]]
    h, r, n = V.bleu_args([[4, 5], [6]], [[4], [6, 7]], device="cpu")
    assert r.shape == (2, 1, 3) and n is None
    assert V.bleu_args([[4], [5]], [[4], [5]], n_refs=1, device="cpu")[2].tolist() == [1, 1]
    for bad in (dict(n_refs=[1]), dict(n_refs=[1, 2]), dict(n_refs=[0, 1]), dict(n_refs=torch.ones(2))):
        with pytest.raises(ValueError, match="n_refs"):
            V.bleu_args([[4], [5]], [[4], [5]], device="cpu", **bad)
    with pytest.raises(ValueError, match="N = 2"):
        V.bleu_args([[4], [5]], [[4]], device="cpu")
    with pytest.raises(ValueError, match="at least one reference"):
        V.bleu_args([[4], [5]], [[[4]], []], device="cpu")
    with pytest.raises(ValueError, match="unsupported shape"):
        V.bleu_args([[4] * 513], [[4]], device="cpu")
    with pytest.raises(ValueError, match="unsupported shape"):
        V.bleu_args([[4]], [[[4]] * 65], device="cpu")
    with pytest.raises(ValueError, match="Surface"):
        V.ChrfStats("cpu", None)
    t = Surface(["<pad>", "<unk>", "<s>", "</s>", "ab", "c"])
    with pytest.raises(ValueError, match="hypotheses"):
        V.ChrfStats("cpu", t).add([[4]], [[4], [5]])
    # validate's own checks come before anything runs
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    m = NMT_Seq2Seq_Beam_V2(20, 20, 8, 8, 16)
    with pytest.raises(ValueError, match="dev loss needs a TrainStep"):
        V.validate(m, [])
    with pytest.raises(ValueError, match="metrics"):
        V.validate(m, [], metrics=("meteor",))
    with pytest.raises(ValueError, match="surface"):
        V.validate(m, [], metrics=("chrf",))
    with pytest.raises(ValueError, match="surface"):
        V.validate(m, [], metrics=("bleu",), surface=t)
    with pytest.raises(ValueError, match="TrainStep, a model or an Ensemble"):
        V.validate(object(), [], metrics=("bleu",))
    with pytest.raises(ValueError, match="no batches"):
        V.validate(m, [], metrics=("bleu",))
    with pytest.raises(ValueError, match="beam_size"):
        V.validate(m, [], metrics=("bleu",), beam_size=0)
