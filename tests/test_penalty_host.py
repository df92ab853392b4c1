"""CPU: the host side of the penalised beam search (vagnmt_hip.penalty) and its NumPy yardstick (tests/penalty_ref.py): the tables
against their formulas, the argument checks, penalised_score, the reference against tests/diverse_ref.py, and the table model
tests/test_gpu_penalty.py runs on the device -- with the assertions that make that test non-vacuous."""
import numpy as np
import pytest
import torch

import diverse_ref as D
import penalty_ref as R

EOS = 3
F32 = np.float32


def table_model(seed=11, V=50, Tp=9):
    """A table "model" like test_gpu_diverse's: the row of log-probabilities (quantised to 1/8, EOS raised) and the attention row
    (quantised to 1/64, some exact zeros) depend on the previous word alone.  mask (2, Tp): the second sentence is shorter."""
    rng = np.random.default_rng(seed)
    T = (rng.integers(-96, 1, size=(V, V)) / 8.0).astype(F32)
    T[:, EOS] += F32(1.5)                                           # some hypotheses finish
    A = (rng.integers(0, 24, size=(V, Tp)) / 64.0).astype(F32)
    A[rng.random((V, Tp)) < 0.2] = 0.0
    mask = np.ones((2, Tp), dtype=F32)
    mask[1, Tp - 3:] = 0.0
    return T, A, mask


# the two settings of the table-model tests, here and on the device: (norm, alpha, beta, word_bonus)
LENGTH_1 = ("length", 1.0, 0.25, 0.0)
WORD_COST = ("none", 0.0, 0.25, -2.0)
SEARCH = dict(B=2, k=6, V=50, max_len=8, steps=8)


def run(T, A, mask, cfg, stepwise, trace=None):
    norm, alpha, beta, wb = cfg
    lp, bonus = R.tables(SEARCH["max_len"], norm, alpha, wb)
    return R.search(lambda tok: T[tok], lambda tok: A[tok], mask, lp=lp, bonus=bonus, beta=beta, stepwise=stepwise, trace=trace,
                    **SEARCH), lp, bonus


def test_tables_match_the_formulas_in_fp64():
    from vagnmt_hip import penalty
    ml = 80
    L = np.maximum(np.arange(ml + 1, dtype=np.float64), 1.0)
    for alpha in (0.0, 0.6, 1.0, 1.7):
        lp, bonus = penalty.tables(ml, "gnmt", alpha, 0.35)
        assert lp.dtype == np.float32 and bonus.dtype == np.float32 and lp.shape == bonus.shape == (ml + 1,)
        assert lp.tobytes() == (((5.0 + L) / 6.0) ** alpha).astype(F32).tobytes()
        assert bonus.tobytes() == (0.35 * L).astype(F32).tobytes()
        assert penalty.tables(ml, "length", alpha, 0.0)[0].tobytes() == (L ** alpha).astype(F32).tobytes()
        assert penalty.tables(ml, "none", alpha, 0.0)[0].tobytes() == np.ones(ml + 1, dtype=F32).tobytes()
        for norm in ("gnmt", "length", "none"):
            a, b = penalty.tables(ml, norm, alpha, -0.5), R.tables(ml, norm, alpha, -0.5)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    lp, bonus = penalty.tables(ml, "length", 1.0, 0.0)
    assert lp.tolist() == [float(max(1, n)) for n in range(ml + 1)] and not bonus.any()
    with pytest.raises(ValueError, match="length_norm"):
        penalty.tables(ml, "wu", 1.0, 0.0)


def test_argument_checks_name_the_method():
    from vagnmt_hip import penalty
    src = torch.zeros(2, 3, dtype=torch.int64)
    ok = dict(src_var=src, beam_size=4, n_best=2, max_length=10, length_norm="gnmt", alpha=0.6, beta=0.2, word_bonus=0.0,
              stepwise=False, avoid_double=True, avoid_unk=False, vocab=100)
    bad = [(dict(beam_size=65), "beam_size"), (dict(n_best=5), "n_best"), (dict(n_best=0), "n_best"), (dict(max_length=0), "max_length"),
           (dict(length_norm="wu"), "length_norm"), (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"),
           (dict(beta=-1.0), "beta"), (dict(beta=float("inf")), "beta"), (dict(word_bonus=float("nan")), "word_bonus"),
           (dict(stepwise=2), "stepwise"), (dict(vocab=3), "vocabulary"), ({}, "GPU tensor")]        # {}: src_var is on the CPU
    for change, word in bad:
        with pytest.raises(ValueError, match="beamsearch_penalised: .*" + word):
            penalty.penalised_args(**dict(ok, **change))


def test_penalised_score_in_plain_torch():
    from vagnmt_hip import penalty
    rng = np.random.default_rng(3)
    B, n, T, Ts = 2, 3, 6, 5
    att = (rng.integers(0, 40, size=(B, n, T, Ts)) / 64.0).astype(F32)
    att[:, :, 4:] = 0.0
    mask = np.ones((B, Ts), dtype=F32)
    mask[1, 3:] = 0.0
    logp = -rng.random((B, n)).astype(F32) * 20
    length = rng.integers(0, 6, size=(B, n))
    for norm, alpha, beta, wb in (("gnmt", 0.6, 0.2, 0.0), ("length", 1.0, 0.0, 0.0), ("none", 0.0, 0.5, 0.3)):
        got = penalty.penalised_score(torch.from_numpy(logp), torch.from_numpy(length), torch.from_numpy(att), torch.from_numpy(mask),
                                      norm, alpha, beta, wb)
        cov = att.astype(np.float64).sum(axis=2)
        cp = beta * (np.log(np.clip(cov, 1e-10, 1.0)) * (mask[:, None, :] != 0)).sum(axis=-1)
        L = np.maximum(length, 1).astype(np.float64)
        lp = {"gnmt": ((5 + L) / 6) ** alpha, "length": L ** alpha, "none": np.ones_like(L)}[norm]
        want = (logp + wb * L) / lp + cp
        assert np.allclose(got.coverage_penalty.numpy(), cp, rtol=1e-5, atol=1e-6)
        assert np.allclose(got.score.numpy(), want, rtol=1e-5, atol=1e-5)
        if beta == 0:
            assert not got.coverage_penalty.numpy().any()
    # the plain normalisation: bit for bit logp / max(1, length)
    got = penalty.penalised_score(torch.from_numpy(logp), torch.from_numpy(length), None, None, "length", 1.0, 0.0, 0.0)
    assert got.score.numpy().tobytes() == (logp / np.maximum(length, 1).astype(F32)).astype(F32).tobytes()


def test_reference_without_stepwise_is_the_plain_step():
    """penalty_ref with stepwise=False against diverse_ref at one group, same inputs: words, parents, score bits -- whatever
    the tables, lens and cp_row hold."""
    rng = np.random.default_rng(5)
    lp, bonus = R.tables(8, "gnmt", 0.6, 0.1)
    for k, V in ((6, 50), (12, 300)):
        for di, flags in ((0, 0), (2, 3), (1, 0), (7, 1)):
            k_in = 1 if di == 0 else k
            logp = (rng.integers(-96, 1, size=(k_in, V)) / 8.0).astype(F32)
            base = prev = lens = None
            if di:
                base = (rng.integers(-400, 0, size=k) / 8.0).astype(F32)
                prev = rng.integers(0, V, size=k)
                prev[rng.random(k) < 0.3] = EOS
                prev[0] = 7                                         # (at least one live row: k candidates above the -1e5 range)
                lens = rng.integers(0, 6, size=k)
            cp = -rng.random(k_in).astype(F32)
            w, p, sc, ln, cpn, _ = R.step(logp, base, prev, lens, cp, k, lp, bonus, False, di, 8, flags)
            w2, p2, sc2 = D.step(logp, base, prev, k, 1, 0.0, flags)
            assert w.tolist() == w2.tolist() and p.tolist() == p2.tolist() and sc.tobytes() == sc2.tobytes()
            for r in range(k):
                live = di == 0 or prev[p[r]] != EOS
                assert ln[r] == (0 if di == 0 else lens[p[r]]) + int(w[r] > 3 and live and di < 7)
                assert cpn[r] == cp[p[r]]


def test_plain_tables_give_the_plain_finish():
    T, A, mask = table_model()
    res, lp, bonus = run(T, A, mask, ("length", 1.0, 0.0, 0.0), False)
    beam, nll = D.search(lambda tok: T[tok], SEARCH["B"], SEARCH["k"], 1, 0.0, SEARCH["V"], SEARCH["max_len"], SEARCH["steps"])
    assert np.array_equal(res["beam"], beam) and res["nll"].tobytes() == nll.tobytes()
    k, ml, steps = SEARCH["k"], SEARCH["max_len"], SEARCH["steps"]
    fin = R.finish(res["beam"], res["nll"], res["lens"], res["cpen"], lp, bonus, ml, steps, k)
    out, sc, slots = D.finish(beam, nll, ml, steps, k)
    assert np.array_equal(fin["out"], out) and fin["scores"].tobytes() == sc.tobytes() and np.array_equal(fin["slots"], slots)
    for b in range(SEARCH["B"]):
        for j in range(k):
            assert res["lens"][b, j] == R.walk_length(beam, ml, steps, b, j)
    assert not res["cpen"].any() and not np.signbit(res["cpen"]).any()


def eos_outside_row_best(trace, k):
    """Selections (step, sentence, slot) of an EOS child of a LIVE row that is not among its row's k best by (c desc, w asc)."""
    found = []
    for t in trace:
        if t["prev"] is None:
            continue
        V = t["c"].shape[1]
        for r, (w, p) in enumerate(zip(t["words"], t["parents"])):
            if w != EOS or t["prev"][p] == EOS:
                continue
            best = np.lexsort((np.arange(V), -t["c"][p].astype(np.float64)))[:k]
            if EOS not in best.tolist():
                found.append((t["di"], t["b"], r))
    return found


def test_table_model_separates_stepwise_from_final():
    """What tests/test_gpu_penalty.py's whole-search test relies on, shown by the reference alone.
    (a) "length", alpha = 1: selecting by the normalised score at every step ends in another beam than normalising at the finish.
    (b) an EOS child outside its row's k best by c is selected by key.  No length normalisation can show it on negative scores
        (the EOS child keeps len_j, its siblings get len_j + 1: dividing by more only helps the siblings), a cost per word does:
        with lp = 1 and bonus[L] = -2 L the EOS child is 2 ahead of every sibling above 3.  A stage 1 that kept each row's k best by c
        would lose it."""
    T, A, mask = table_model()
    k = SEARCH["k"]
    on, _, _ = run(T, A, mask, LENGTH_1, True)
    off, lp, bonus = run(T, A, mask, LENGTH_1, False)
    assert not np.array_equal(on["beam"], off["beam"])
    f_on = R.finish(on["beam"], on["nll"], on["lens"], on["cpen"], lp, bonus, SEARCH["max_len"], SEARCH["steps"], 1)
    f_off = R.finish(off["beam"], off["nll"], off["lens"], off["cpen"], lp, bonus, SEARCH["max_len"], SEARCH["steps"], 1)
    assert any(D.cut(a[0]) != D.cut(b[0]) for a, b in zip(f_on["out"], f_off["out"]))
    trace = []
    run(T, A, mask, WORD_COST, True, trace)
    assert eos_outside_row_best(trace, k)
    trace_off = []
    run(T, A, mask, WORD_COST, False, trace_off)
    assert not eos_outside_row_best(trace_off, k)              # (selected by c, a child is always among its row's k best)
    # the coverage term is live in both settings: some penalty is non-zero, and finished rows froze theirs
    assert on["cpen"].any() and (on["cpen"] <= 0).all()
