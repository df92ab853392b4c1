"""CPU: diverse beam search's host side -- the argument checks of vagnmt_hip.diverse (and of mbr_decode's beam_groups /
beam_diversity) and the NumPy reference itself (tests/diverse_ref.py), which the GPU tests compare the kernels against."""
import numpy as np
import pytest
import torch

import diverse_ref as R


class _OnGpu(torch.Tensor):
    """A tensor that says it is on a GPU: all the checks look at of src_var, and no device is needed."""
    is_cuda = property(lambda self: True)


@pytest.fixture
def src():
    return torch.zeros(2, 3, dtype=torch.int64).as_subclass(_OnGpu)


def test_diverse_args(src):
    from vagnmt_hip import diverse as D
    assert D.diverse_args(src, 12, 3, 0.5, None, True, False) == (12, 3, 0.5, 12, 0)
    assert D.diverse_args(src, 6, 6, 0, 2, False, True, vocab=6) == (6, 6, 0.0, 2, 3)
    assert D.diverse_args(src, 64, 1, 2.0, 64, True, True) == (64, 1, 2.0, 64, 2)
    bad = [dict(beam_size=0), dict(beam_size=65, n_groups=5), dict(n_groups=0), dict(n_groups=5), dict(n_groups=-3),
           dict(diversity=-0.1), dict(diversity=float("nan")), dict(diversity=float("inf")), dict(n_best=0), dict(n_best=13),
           dict(vocab=11)]
    for kw in bad:
        a = dict(beam_size=12, n_groups=3, diversity=0.5, n_best=None, vocab=None)
        a.update(kw)
        with pytest.raises(ValueError, match="beamsearch_diverse"):
            D.diverse_args(src, a["beam_size"], a["n_groups"], a["diversity"], a["n_best"], True, False, a["vocab"])
    with pytest.raises(ValueError, match="GPU tensor"):
        D.diverse_args(torch.zeros(2, 3, dtype=torch.int64), 12, 3, 0.5, None, True, False)
    with pytest.raises(ValueError, match="GPU tensor"):
        D.diverse_args([[4, 5]], 12, 3, 0.5, None, True, False)
    assert D.Diverse._fields == ("hyps", "scores", "group")


def test_mbr_beam_arguments():
    from vagnmt_hip import diverse as D
    assert D.mbr_beam_args(6, 3, 0.5) == (3, 0.5)
    assert D.mbr_beam_args(6, 1, -7.0) == (1, 0.0)              # one group: today's path, the strength is not looked at
    assert D.mbr_beam_args(0, 1, 0.5) == (1, 0.0)
    for k, G, lam in [(6, 4, 0.5), (6, 0, 0.5), (6, 3, -1.0), (6, 3, float("nan")), (0, 3, 0.5)]:
        with pytest.raises(ValueError, match="mbr_decode"):
            D.mbr_beam_args(k, G, lam)
    # the models and the ensemble take the two arguments with these defaults
    import inspect
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.ensemble import Ensemble
    for cls in (NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2, Ensemble):
        p = inspect.signature(cls.mbr_decode).parameters
        assert p["beam_groups"].default == 1 and p["beam_diversity"].default == 0.5, cls
        p = inspect.signature(cls.beamsearch_diverse).parameters
        assert [(n, p[n].default) for n in list(p)[3:]] == [
            ("im_var", None), ("beam_size", 12), ("n_groups", 3), ("diversity", 0.5), ("n_best", None), ("max_length", 80),
            ("avoid_double", True), ("avoid_unk", False)], cls


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def quantised(rng, R_, V):
    """Log-probabilities on a grid of 1/8 in [-12, 0]: ties everywhere."""
    return (rng.integers(-96, 1, size=(R_, V)) / 8.0).astype(np.float32)


def step_inputs(rng, k, V):
    logp = quantised(rng, k, V)
    base = (rng.integers(-400, 0, size=k) / 8.0).astype(np.float32)
    prev = rng.integers(4, V, size=k)
    prev[rng.random(k) < 0.3] = R.EOS
    return logp, base, prev


def plain_topk(c, k):
    V = c.shape[1]
    order = sorted(range(c.size), key=lambda f: (-float(c[f // V, f % V]), f))[:k]
    return [f % V for f in order], [f // V for f in order], [c[f // V, f % V] for f in order]


def test_one_group_is_a_plain_topk_step():
    rng = np.random.default_rng(1)
    for k, V, flags in [(6, 50, 0), (4, 9, 3), (12, 40, 1)]:
        for first in (True, False):
            if first:
                logp, base, prev = quantised(rng, 1, V), None, None
            else:
                logp, base, prev = step_inputs(rng, k, V)
            w, p, sc = R.step(logp, base, prev, k, 1, 0.5, flags)
            ww, wp, wsc = plain_topk(R.model_values(logp, base, prev, flags), k)
            assert list(w) == ww and list(p) == wp and [x.tobytes() for x in sc] == [np.float32(x).tobytes() for x in wsc]


def test_zero_strength_gives_identical_groups():
    rng = np.random.default_rng(2)
    k, G, V = 6, 3, 30
    g = k // G
    w, p, sc = R.step(quantised(rng, 1, V), None, None, k, G, 0.0)
    for i in range(1, G):
        assert list(w[i * g:(i + 1) * g]) == list(w[:g]) and list(sc[i * g:(i + 1) * g]) == list(sc[:g])
    # a whole search: every group is the width-g search
    T = quantised(rng, V, V)
    beam, nll = R.search(lambda tok: T[tok], 2, k, G, 0.0, V, 6, 6)
    beam1, nll1 = R.search(lambda tok: T[tok], 2, g, 1, 0.0, V, 6, 6)
    for i in range(G):
        assert np.array_equal(beam[:6, :, i * g:(i + 1) * g], beam1[:6])
        assert np.array_equal(beam[6:, :, i * g:(i + 1) * g] - i * g * (np.arange(6)[:, None, None] > 0), beam1[6:])
        assert np.array_equal(nll[:, i * g:(i + 1) * g], nll1)


def test_huge_strength_makes_first_words_disjoint():
    rng = np.random.default_rng(3)
    k, G, V = 12, 4, 40
    g = k // G
    w, _, sc = R.step(quantised(rng, 1, V), None, None, k, G, 1e6)
    groups = [set(w[i * g:(i + 1) * g]) for i in range(G)]
    assert all(len(s) == g for s in groups)
    assert all(not (groups[i] & groups[j]) for i in range(G) for j in range(i))
    assert bool((sc > -100).all())                             # the stored score is the model's, without the penalty


def brute_force(logp, base, prev, k, G, lam, flags):
    """The rule, spelled out candidate by candidate in Python (independent of diverse_ref.step's array code)."""
    c = R.model_values(logp, base, prev, flags)
    Rr, V = c.shape
    g = k // G
    chosen = []                                                # (word, parent finished?) of earlier groups' slots
    out = []
    for i in range(G):
        rows = [0] if Rr == 1 else list(range(i * g, (i + 1) * g))
        cands = []
        for j in rows:
            fin = prev is not None and prev[j] == R.EOS
            for w in range(V):
                cnt = sum(1 for (cw, cf) in chosen if cw == w and not cf)
                s = c[j, w] if fin else np.float32(np.float64(c[j, w]) - np.float64(lam) * cnt)
                cands.append((-float(s), j * V + w))
        cands.sort()
        for _, f in cands[:g]:
            j, w = f // V, f % V
            out.append((w, j, c[j, w].tobytes()))
            chosen.append((w, prev is not None and prev[j] == R.EOS))
    return out


@pytest.mark.parametrize("k,G,V,lam,flags", [(6, 3, 20, 0.5, 0), (4, 4, 9, 2.0, 3), (8, 2, 12, 0.5, 1), (6, 2, 6, 2.0, 2),
                                           (6, 6, 17, 0.375, 0)])
def test_reference_equals_brute_force(k, G, V, lam, flags):
    rng = np.random.default_rng(k * 100 + G)
    for trial in range(6):
        if trial % 2 == 0:
            logp, base, prev = quantised(rng, 1, V), None, None
        else:
            logp, base, prev = step_inputs(rng, k, V)
        w, p, sc = R.step(logp, base, prev, k, G, lam, flags)
        assert [(int(a), int(b), c.tobytes()) for a, b, c in zip(w, p, sc)] == brute_force(logp, base, prev, k, G, lam, flags)


def test_finish_orders_by_score_then_slot_and_reports_slots():
    # two steps, k = 3: slots 0 and 2 tie on the normalised score, slot 1 is better
    max_len = 4
    beam = np.zeros((2 * max_len, 1, 3), dtype=np.int64)
    beam[0, 0] = [5, 6, 7]
    beam[1, 0] = [8, 3, 9]
    beam[max_len + 1, 0] = [2, 0, 1]
    nll = np.array([[-4.0, -1.0, -4.0]], dtype=np.float32)
    out, sc, slots = R.finish(beam, nll, max_len, 2, 3)
    assert slots.tolist() == [[1, 0, 2]] and sc.tolist() == [[-1.0, -2.0, -2.0]]
    assert out[0].tolist() == [[5, 3, 0, 3], [7, 8, 0, 3], [6, 9, 0, 3]]
    assert R.cut(out[0, 0]) == [5]
