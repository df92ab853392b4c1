"""CPU: the host side of stochastic beam search (vagnmt_hip.stochastic) and its yardstick (tests/stochastic_ref.py).

1. sbs_log_weights against a float64 NumPy restatement, k = 1 and logp - kappa large in both directions included;
2. the argument checks of beamsearch_stochastic and of mbr_decode(without_replacement=True), the ABI's -EINVAL without a device;
3. the reference itself: its invariants on the one-step cases of the GPU test (which must leave at most 1 % of them out of the
   set comparison), and whole searches on a 5-word Markov model against the exact distribution -- the statistical test the GPU
   runs is satisfiable, shown here with numpy's own Gumbel noise; sbs_uncondition against its float64 statement."""
import ctypes as C

import numpy as np
import pytest
import torch

import stochastic_ref as R


# ------------------------------------------------------------------------------------------------------------------
# 1. the importance weights
# ------------------------------------------------------------------------------------------------------------------
def log_weights_f64(logp, gumbel):
    """Kool et al.'s estimator in float64: kappa = the sentence's smallest G; log w = logp - log(1 - exp(-exp(logp - kappa))) for
    the others, -inf for the sample that sets kappa; a single sample gets 0.  log q in forms that stay accurate where logp - kappa is far from 0."""
    logp, gumbel = np.asarray(logp, dtype=np.float64), np.asarray(gumbel, dtype=np.float64)
    B, k = logp.shape
    if k == 1:
        return np.zeros((B, 1))
    out = np.empty((B, k))
    for b in range(B):
        last = int(np.argmin(gumbel[b]))
        for i in range(k):
            x = logp[b, i] - gumbel[b, last]
            if x < -30.0:
                log_q = x - np.exp(x) / 2.0                # log(e - e^2/2 + ...) with e = exp(x) below 1e-13
            elif x > 5.0:
                log_q = -np.exp(-np.exp(x))                # log(1 - t), t = exp(-e) below 1e-64
            else:
                log_q = np.log(-np.expm1(-np.exp(x)))
            out[b, i] = -np.inf if i == last else logp[b, i] - log_q
    return out


def test_log_weights_match_float64():
    from vagnmt_hip.stochastic import sbs_log_weights
    rng = np.random.default_rng(0)
    B, k = 64, 12
    logp = -30.0 * rng.random((B, k))
    gum = logp + rng.gumbel(size=(B, k))
    gum = -np.sort(-gum, axis=1)
    # logp - kappa large in both directions: a sample far more and one far less probable than the threshold
    logp[0, 0], logp[0, 1] = -0.001, -250.0
    gum[0, -1] = -60.0
    logp[1, 0], gum[1, -1] = -1.0, -200.0
    want = log_weights_f64(logp, gum)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 4e-6)):
        lp, g = torch.tensor(logp, dtype=dtype), torch.tensor(gum, dtype=dtype)
        got = sbs_log_weights(lp, g)
        assert got.dtype == dtype and got.shape == (B, k)
        w = want if dtype == torch.float64 else log_weights_f64(lp.numpy(), g.numpy())
        got = got.numpy().astype(np.float64)
        assert np.array_equal(np.isneginf(got), np.isneginf(w)) and np.isneginf(got).sum() == B
        fin = np.isfinite(w)
        assert np.isfinite(got[fin]).all()
        err = np.abs(got[fin] - w[fin]) / np.maximum(1.0, np.abs(w[fin]))
        assert err.max() <= tol, (dtype, err.max())
    assert np.isfinite(want[0, :2]).all() and abs(want[0, 0] - (-0.001)) < 1e-9      # q = 1: the weight is p itself
    assert abs(want[0, 1] - (-60.0)) < 1e-9                                           # q = exp(logp - kappa): the weight is exp(kappa)
    # an included sample's weight is at least its probability (q <= 1)
    inc = np.isfinite(want)
    assert (want[inc] >= logp[inc] - 1e-12).all()


def test_log_weights_edge_shapes():
    from vagnmt_hip.stochastic import sbs_log_weights
    one = sbs_log_weights(torch.tensor([[-3.0], [-7.5]]), torch.tensor([[0.25], [-9.0]]))
    assert one.tolist() == [[0.0], [0.0]]
    # the threshold is the smallest G wherever it stands; exactly one sample per sentence is dropped, ties included
    lw = sbs_log_weights(torch.tensor([[-1.0, -2.0, -3.0]]), torch.tensor([[0.5, -4.0, 1.5]]))
    assert torch.isneginf(lw).tolist() == [[False, True, False]]
    lw = sbs_log_weights(torch.tensor([[-1.0, -2.0, -3.0]]), torch.tensor([[0.5, 0.5, 0.5]]))
    assert int(torch.isneginf(lw).sum()) == 1
    with pytest.raises(ValueError, match="sbs_log_weights"):
        sbs_log_weights(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="sbs_log_weights"):
        sbs_log_weights(torch.zeros(3), torch.zeros(3))


# ------------------------------------------------------------------------------------------------------------------
# 2. argument checks
# ------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip import stochastic
    m = NMT_AttentionImagine_Seq2Seq_Beam_V11(30, 40, 24, 8, 8, 16, 12, 0.99).eval()
    t = NMT_Seq2Seq_Beam_V2(30, 40, 8, 8, 16).eval()
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    for obj in (m, t, Ensemble([m, t])):
        for kw, word in ((dict(n_samples=0), "n_samples"), (dict(n_samples=65), "n_samples"), (dict(max_length=0), "max_length"),
                         (dict(n_samples=41), "vocabulary"), (dict(), "GPU tensor")):      # everything in range, but a CPU src_var
            with pytest.raises(ValueError, match="beamsearch_stochastic.*" + word):
                obj.beamsearch_stochastic(src, [5, 5], im, **kw)
        for kw in (dict(temperature=0.9), dict(top_k=10), dict(top_p=0.9)):
            with pytest.raises(ValueError, match="mbr_decode.*without_replacement"):
                obj.mbr_decode(src, [5, 5], im, without_replacement=True, **kw)
        for kw, word in ((dict(beam_size=65), "beam_size"), (dict(utility="chrf"), "utility"), (dict(n_samples=0), "n_samples"),
                         (dict(n_samples=65), "n_samples"), (dict(), "GPU tensor")):
            with pytest.raises(ValueError, match="mbr_decode.*" + word):
                obj.mbr_decode(src, [5, 5], im, without_replacement=True, **kw)
    assert stochastic.stochastic_args(_FakeCuda(), 12, 80, False, False, 9391) == (12, 80, 1)
    assert stochastic.mbr_args(False, 0.9, 10, 0.9) is False and stochastic.mbr_args(True, 1.0, 0, 1.0) is True
    # the defaults: the model's own distribution (a word may repeat), a dozen samples
    import inspect
    for obj in (m, t, Ensemble([m])):
        sig = inspect.signature(obj.beamsearch_stochastic).parameters
        assert sig["avoid_double"].default is False and sig["avoid_unk"].default is False and sig["n_samples"].default == 12
        assert inspect.signature(obj.mbr_decode).parameters["without_replacement"].default is False


class _FakeCuda(torch.Tensor):
    """A tensor that says it is on a GPU: the checks that follow the device check can be reached on the host."""
    @property
    def is_cuda(self):
        return True


def test_entry_points_on_the_host():
    from vagnmt_hip import _lib
    L = _lib.lib()
    assert L.vag_beam_sbs_scratch_bytes(16, 12, 9391, 80) >= 16 * 12 * 5 * 12 * 16
    assert L.vag_beam_sbs_scratch_bytes(16, 12, 9391, 80) > L.vag_beam_div_scratch_bytes(16, 12, 9391, 80)
    # argument errors come back as -EINVAL before anything touches a device (the pointers are never dereferenced)
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    arr = (C.c_void_p * 1)(p)
    one = (C.c_int64 * 1)(50)

    def step(rng=p, gum=p, k=6, V=50, flags=0, M=1, di=0, B=2, nll=p):
        return L.vag_beam_sbs_step(arr, one, M, nll, p, di, 4, arr, arr, one, B, k, V, p, p, flags, rng, gum, None)
    bad = [dict(rng=None), dict(gum=None), dict(k=0), dict(k=65), dict(V=5), dict(flags=4), dict(M=0), dict(M=9), dict(di=-1),
           dict(di=4), dict(B=0), dict(B=10923), dict(nll=None)]
    for kw in bad:
        assert step(**kw) == -22, kw
    assert L.vag_beam_sbs_step_dev(arr, one, 1, p, p, None, 4, arr, arr, one, p, 2, 6, 50, p, p, 0, p, p, None) == -22
    assert L.vag_beam_sbs_step_dev(arr, one, 1, p, p, p, 4, arr, arr, one, p, 2, 6, 50, p, p, 0, None, p, None) == -22


# ------------------------------------------------------------------------------------------------------------------
# 3. the reference
# ------------------------------------------------------------------------------------------------------------------
def test_reference_invariants_on_the_gpu_tests_cases():
    """The cases the GPU test runs, with numpy's noise: G~ never exceeds the parent's G, the arg-max child and the child of a
    finished row inherit it exactly, the chosen are ranked, the stored score is c -- and the seeds leave at most 1 % of the
    (sentence, step) cases undecided within the tolerances (here: none)."""
    total = left = 0
    for case in R.CASES:
        B, k, V, di = case
        c = R.make_case(case)
        rows = 1 if di == 0 else k
        noise = np.random.default_rng(R.case_seed(case) + 1).gumbel(size=(B, rows, V)).astype(np.float32)
        r = R.step(c["logp"], noise, c["base"], c["prev"], c["G"], k, c["flags"])
        total += B
        left += int((~r["comparable"]).sum())
        assert (np.diff(r["gum"], axis=1) <= 0).all(), case
        assert (r["gum"] <= r["parent_G"].astype(np.float64)).all(), case
        ex = r["exact"]
        assert ex.any() and (r["gum"][ex] == r["parent_G"][ex].astype(np.float64)).all(), case
        assert r["exact"][:, 0].all(), case                    # the best of all is some row's best child
        want_c = np.take_along_axis(r["c_all"].reshape(B, -1), r["parents"] * V + r["words"], axis=1)
        assert r["c"].tobytes() == want_c.tobytes() and r["c"].dtype == np.float32
        if di > 0:
            fin = np.take_along_axis(c["prev"] == R.EOS, r["parents"], axis=1)
            assert (r["words"][fin] == R.EOS).all()
            assert (r["c"][fin] == np.take_along_axis(c["base"], r["parents"], axis=1)[fin]).all()
        for b in range(B):
            assert len({(int(p), int(w)) for p, w in zip(r["parents"][b], r["words"][b])}) == k
    assert total == 3 * len(R.CASES) and left * 100 <= total, (left, total)


def test_reference_samples_the_exact_distribution():
    """Whole searches on the 5-word Markov model (V = 5, k = 3, two steps, 16384 replications): slot 0 is a draw from p, the
    sample is a draw without replacement, the weighted estimator is unbiased -- every frequency within five standard errors.
    The estimator takes the perturbed scores as the public call returns them, through sbs_uncondition: the search's own values
    are conditioned on their maximum (the root's G = 0), and weights formed from those are biased -- leaf (0, 0), p = 0.2573,
    was estimated at 0.2276 with a standard error of 0.0021 -- which the last lines pin as well."""
    from vagnmt_hip.stochastic import sbs_log_weights, sbs_uncondition
    T = R.markov_table()
    B, k, steps = 16384, 3, 2
    names, p, incl = R.exact_markov(T, steps, k)
    assert len(names) == 21 and abs(incl.sum() - k) < 1e-9
    rng = np.random.default_rng(11)
    hyps, logp, gum = R.markov_search(T, B, k, steps, rng)
    index = {y: i for i, y in enumerate(names)}
    ids = np.array([[index[tuple(h)] for h in sent] for sent in hyps.tolist()])
    assert (np.sort(ids, axis=1)[:, 1:] != np.sort(ids, axis=1)[:, :-1]).all()            # pairwise distinct
    assert np.abs(logp.astype(np.float64) - np.log(p)[ids]).max() < 1e-5
    assert (gum[:, 0] == 0).all() and (np.diff(gum, axis=1) <= 0).all()                   # the maximum is the root's G
    first = np.bincount(ids[:, 0], minlength=len(names)) / B
    assert (np.abs(first - p) <= 5 * np.sqrt(p * (1 - p) / B)).all()
    inc = np.array([(ids == i).any(axis=1).mean() for i in range(len(names))])
    assert (np.abs(inc - incl) <= 5 * np.sqrt(incl * (1 - incl) / B)).all()
    lp, g = torch.from_numpy(logp.astype(np.float32)), torch.from_numpy(gum.astype(np.float32))
    free = sbs_uncondition(g, torch.from_numpy(rng.gumbel(size=(B, 1)).astype(np.float32)))
    assert bool((free[:, 1:] <= free[:, :-1]).all())                                      # the order is kept
    w = torch.exp(sbs_log_weights(lp, free)).numpy()
    for i in range(len(names)):
        est = (w * (ids == i)).sum(axis=1)
        se = est.std(ddof=1) / np.sqrt(B)
        assert abs(est.mean() - p[i]) <= 5 * se, (names[i], est.mean(), p[i], se)
    biased = (torch.exp(sbs_log_weights(lp, g)).numpy() * (ids == 0)).sum(axis=1)
    assert abs(biased.mean() - p[0]) > 5 * biased.std(ddof=1) / np.sqrt(B)


def test_uncondition_is_the_truncation_coupling():
    """sbs_uncondition against its float64 statement, G' = -log(exp(-top) + exp(-G) - 1) relative to the row's maximum: the
    maximum becomes top, a G far below it stays what it was, the order is kept; float32 and float64."""
    from vagnmt_hip.stochastic import sbs_uncondition
    rng = np.random.default_rng(2)
    G = -np.sort(rng.exponential(2.0, size=(50, 6)), axis=1)
    G[:, 0] = 0.0
    G[0, 1], G[0, 5] = -1e-6, -90.0
    top = rng.gumbel(size=(50, 1))
    want = -np.log(np.exp(-top) + np.expm1(-G))
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        got = sbs_uncondition(torch.tensor(G, dtype=dtype), torch.tensor(top, dtype=dtype)).numpy().astype(np.float64)
        assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), dtype
        assert (np.diff(got, axis=1) <= 0).all()
    assert np.allclose(want[:, 0], top[:, 0]) and abs(want[0, 5] + 90.0) < 1e-9
    shifted = sbs_uncondition(torch.tensor(G + 3.5), torch.tensor(top)).numpy()           # relative to the maximum, whatever it is
    assert np.abs(shifted - want).max() < 1e-9
