"""CPU: the n-gram language model of vagnmt_hip.lm on the host against tests/lm_ref.py, and what of the fusion needs no device.

The estimator's trie is the brute-force Kneser-Ney model; every context's distribution sums to 1; ARPA files round-trip; the
constructor rejects malformed tries; the error bound of the GPU tests is honest (the fp32 restatement of the kernel's arithmetic
stays inside it on every case) and sensitive (every defect of the catalogue leaves it); the ABI's argument errors come back
before anything touches a device; the graph key tells betas and models apart."""
import ctypes as C

import numpy as np
import pytest

import lm_ref as R


def LM():
    from vagnmt_hip import lm
    return lm


def corpus(V=40, n=60, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(w) for w in 4 + np.minimum(rng.zipf(1.5, size=int(rng.integers(1, 9))), V - 5)] for _ in range(n)]


def trie_grams(m):
    """{n-gram: (logp, bo)} read back from the trie's arrays (float64 masters)."""
    out = {}
    for l, d in enumerate(m.levels):
        rows = m.rows(l)
        for i in range(rows.shape[0]):
            out[tuple(int(x) for x in rows[i])] = (float(d["logp"][i]), float(d["bo"][i]) if "bo" in d else 0.0)
    return out


@pytest.fixture(scope="module", params=[2, 3, 5])
def trained(request):
    order, V = request.param, 40
    sents = corpus(V)
    return order, V, sents, LM().NgramLM.train(sents, V, order), R.kn_bruteforce(sents, V, order)


# -------------------------------------------------------------------------------------------------------------- the estimator
def test_trained_trie_is_the_brute_force_model(trained):
    order, V, sents, m, ref = trained
    got = trie_grams(m)
    assert set(got) == set(ref)
    worst = max(max(abs(got[g][0] - ref[g][0]), abs(got[g][1] - ref[g][1])) for g in ref)
    assert worst <= 1e-12, worst
    assert m.counts == [sum(1 for g in ref if len(g) == n) for n in range(1, order + 1)]


def test_a_tensor_of_sentences_trains_the_same_model(trained):
    import torch
    order, V, sents, m, _ = trained
    L = max(len(s) for s in sents)
    t = torch.zeros(len(sents), L, dtype=torch.int64)
    for i, s in enumerate(sents):
        t[i, :len(s)] = torch.tensor(s)
    m2 = LM().NgramLM.train(t, V, order)
    assert np.array_equal(m2.host, m.host)
    with pytest.raises(ValueError):
        LM().NgramLM.train([[4, 2, 5]], V, order)                     # SOS inside a sentence
    with pytest.raises(ValueError):
        LM().NgramLM.train([[4, V]], V, order)


def contexts_of(order, sents):
    s = sents[0] + sents[1]
    nc = order - 1
    seen = [R.SOS] + sents[2][:nc - 1] if nc > 1 else [R.SOS]
    return {"empty": [], "sos": [R.SOS], "seen": seen[-nc:], "short": sents[3][:1], "unseen": [38, 37, 36, 35][:nc],
            "last_only": ([38, 37, 36][:nc - 1] + s[:1]), "pad": [-1] * (nc - 1) + sents[4][:1], "after_eos": [R.EOS]}


def test_every_context_sums_to_one(trained):
    order, V, sents, m, ref = trained
    for name, ctx in contexts_of(order, sents).items():
        by_trie = sum(np.exp(m.logprob(w, ctx)[0]) for w in range(V))
        by_dict = sum(np.exp(R.lm64(ref, w, R.clean_ctx(ctx, V, order))[0]) for w in range(V))
        assert abs(by_trie - 1.0) <= 1e-9 and abs(by_dict - 1.0) <= 1e-9, (name, by_trie, by_dict)
        for w in (0, R.UNK, R.SOS, R.EOS, 4, V - 1):
            a, b = m.logprob(w, ctx), R.lm64(ref, w, R.clean_ctx(ctx, V, order))
            assert a[1] == b[1] and abs(a[0] - b[0]) <= 1e-12, (name, w)
    assert min(np.exp(m.logprob(w, [])[0]) for w in range(V)) > 0.0


def test_training_thirty_thousand_sentences_takes_seconds():
    rng = np.random.default_rng(1)
    V = 9391
    sents = (4 + np.minimum(rng.zipf(1.3, size=(30000, 12)), V - 5)).astype(np.int64)
    m = LM().NgramLM.train(sents, V, 3)
    assert m.train_seconds < 30.0 and m.counts[2] > 100000


# ------------------------------------------------------------------------------------------------------------------ files
ARPA = """\\data\\
ngram 1=5
ngram 2=2

\\1-grams:
-1.0\t<unk>\t-0.5
-99\t<s>\t-0.25
-0.7\t</s>
-0.5\tcat\t-0.3
-0.9\tdog

\\2-grams:
-0.2\t<s> cat
-0.4\tcat dog
-0.1\tcat bird

\\end\\
"""


def test_a_hand_written_arpa_file_is_read(tmp_path):
    p = tmp_path / "tiny.arpa"
    p.write_text(ARPA)
    m = LM().NgramLM.from_arpa(str(p), {"cat": 4, "dog": 5}, 7)
    ln10 = np.log(10.0)
    assert m.order == 2 and m.counts == [7, 2]                         # "cat bird": bird is no word of the vocabulary
    assert abs(m.logprob(4, [R.SOS])[0] - -0.2 * ln10) < 1e-12 and m.logprob(4, [R.SOS])[1] == 2
    assert abs(m.logprob(5, [4])[0] - -0.4 * ln10) < 1e-12
    assert abs(m.logprob(5, [R.SOS])[0] - (-0.25 - 0.9) * ln10) < 1e-12 and m.logprob(5, [R.SOS])[1] == 1
    assert abs(m.logprob(6, [4])[0] - (-0.3 - 1.0) * ln10) < 1e-12     # id 6 has no unigram: <unk>'s value
    assert abs(m.logprob(0, [])[0] - -1.0 * ln10) < 1e-12
    assert abs(m.logprob(R.SOS, [])[0] - -99.0 * ln10) < 1e-9
    bad = tmp_path / "bad.arpa"
    bad.write_text(ARPA.replace("-1.0\t<unk>\t-0.5\n", "").replace("ngram 1=5", "ngram 1=4"))
    with pytest.raises(ValueError):
        LM().NgramLM.from_arpa(str(bad), {"cat": 4, "dog": 5}, 7)


def test_arpa_and_npz_round_trips(trained, tmp_path):
    order, V, sents, m, ref = trained
    words = {i: "w%d" % i for i in range(V) if i not in (R.UNK, R.SOS, R.EOS)}
    p = str(tmp_path / "m.arpa")
    m.to_arpa(p, words)
    back = LM().NgramLM.from_arpa(p, {v: k for k, v in words.items()}, V)
    a, b = trie_grams(m), trie_grams(back)
    assert set(a) == set(b)
    assert max(max(abs(a[g][0] - b[g][0]), abs(a[g][1] - b[g][1])) for g in a) <= 1e-12
    q = str(tmp_path / "m.npz")
    m.save(q)
    again = LM().NgramLM.load(q)
    assert again.order == m.order and again.V == m.V and np.array_equal(again.host, m.host)


# ------------------------------------------------------------------------------------------------------------- validation
def levels_of(m):
    return [{k: v.copy() for k, v in d.items()} for d in m.levels]


def test_the_constructor_rejects_malformed_tries(trained):
    order, V, sents, m, _ = trained
    N = LM().NgramLM
    N(order, V, levels_of(m))                                           # the untouched copy is fine

    def broken(change):
        lv = levels_of(m)
        change(lv)
        with pytest.raises(ValueError):
            N(order, V, lv)

    c0 = m.levels[0]["child"]
    node = int(np.flatnonzero(np.diff(c0) >= 2)[0])                     # a unigram with two successors or more
    lo = int(c0[node])

    def swap(lv):
        lv[1]["word"][[lo, lo + 1]] = lv[1]["word"][[lo + 1, lo]]

    def twice(lv):
        lv[1]["word"][lo + 1] = lv[1]["word"][lo]

    def not_monotone(lv):
        lv[0]["child"][node + 1] = lv[0]["child"][node] - 1

    def past_the_level(lv):
        lv[0]["child"][-1] += 1

    def not_from_zero(lv):
        lv[0]["child"][0] = 1

    def word_past_v(lv):
        lv[1]["word"][-1] = V

    def word_negative(lv):
        lv[1]["word"][0] = -1

    def nan_logp(lv):
        lv[1]["logp"][0] = np.nan

    def inf_bo(lv):
        lv[0]["bo"][3] = -np.inf

    def short_array(lv):
        lv[1]["logp"] = lv[1]["logp"][:-1]

    for change in (swap, twice, not_monotone, past_the_level, not_from_zero, word_past_v, word_negative, nan_logp, inf_bo, short_array):
        broken(change)
    for bad_order in (1, 6):
        with pytest.raises(ValueError):
            N(bad_order, V, levels_of(m))
    with pytest.raises(ValueError):
        N(order, V + 1, levels_of(m))
    with pytest.raises(ValueError):
        N.train(sents, V, 6)


# ----------------------------------------------------------------------------------- the case tables, the bound, the defects
def case_setup(case, seed=0):
    name, V, ld, order, M, Rr = case
    grams = R.case_model(V, order, seed)
    ctx = R.case_contexts(V, order, Rr, name)
    rows = R.case_rows(V, ld, M, Rr, seed)
    return grams, ctx, rows


def test_the_case_table_covers_what_the_issue_names():
    cs = R.DENSE_CASES
    assert {c[1] for c in cs} == {37, 503, 2049} and {c[3] for c in cs} == {2, 3, 5}
    assert {c[4] for c in cs} == {1, 3} and {c[5] for c in cs} == {1, 7}
    assert any(c[1] == 503 and c[2] == 504 for c in cs)
    for order in (2, 3, 5):
        grams = R.case_model(503, order)
        nc = order - 1
        ctx = {k: R.clean_ctx(r, 503, order) for k, r in zip(R.KINDS, R.case_contexts(503, order, 7))}
        assert ctx["empty"] == [] and len(ctx["short"]) == 1
        assert tuple(ctx["full"]) in grams and len(R.successors(grams, ctx["full"])) >= 2
        assert all(tuple(ctx["full"][i:]) in grams and R.successors(grams, ctx["full"][i:]) for i in range(nc))
        assert tuple(ctx["leaf"]) in grams and not R.successors(grams, ctx["leaf"])
        assert len(R.successors(grams, ctx["big"])) > 256
        assert not R.successors(grams, ctx["unseen"][-1:])
        assert R.successors(grams, ctx["last_only"][-1:]) and (nc == 1 or tuple(ctx["last_only"][-2:]) not in grams)
        # the orders overlap: some word follows the full context at two orders or more
        if nc > 1:
            assert set(R.successors(grams, ctx["full"])) & set(R.successors(grams, ctx["full"][1:]))


def test_the_trie_of_a_case_model_is_the_dict():
    for order in (2, 3, 5):
        grams = R.case_model(503, order)
        m = LM().NgramLM.from_ngrams(order, 503, *R.to_arrays(grams, order))
        for ctx in R.case_contexts(503, order, 7):
            c = R.clean_ctx(ctx, 503, order)
            for w in range(0, 503, 7):
                a, b = m.logprob(w, c), R.lm64(grams, w, c)
                assert a[1] == b[1] and abs(a[0] - b[0]) <= 1e-12
        assert m.host_array(0, "logp").dtype == np.float32
        assert np.array_equal(m.host_array(0, "logp"), np.array([grams[(w,)][0] for w in range(503)], dtype=np.float32))


BETAS = (0.3, -1.7)


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=[c[0] for c in R.DENSE_CASES])
def test_the_fp32_restatement_stays_inside_eps(case):
    name, V, ld, order, M, Rr = case
    grams, ctx, rows = case_setup(case)
    g32 = R.round_fp32(grams)
    for beta in BETAS:
        for r in range(Rr):
            row = rows[0][:Rr * ld].reshape(Rr, ld)[r, :V]
            want, _, bound = R.fuse_row64(grams, V, order, row, ctx[r], beta)
            got = R.fuse_row_fp32(g32, V, order, row, ctx[r], beta).astype(np.float64)
            assert np.all(np.abs(got - want) <= bound), (name, r, float((np.abs(got - want) / bound).max()))
            # and the bound is tight enough to mean something: a few units in the last place of the result
            assert np.all(bound <= 16 * R.U * (np.abs(want) + 30.0))


def test_every_defect_of_the_catalogue_leaves_eps():
    caught = {}
    for case in R.DENSE_CASES:
        name, V, ld, order, M, Rr = case
        grams, ctx, rows = case_setup(case)
        g32 = R.round_fp32(grams)
        for d in R.DEFECTS[:-1]:
            for r in range(Rr):
                row = rows[0][:Rr * ld].reshape(Rr, ld)[r, :V]
                want, _, bound = R.fuse_row64(grams, V, order, row, ctx[r], 0.3)
                got = R.fuse_row_fp32(g32, V, order, row, ctx[r], 0.3, defect=d).astype(np.float64)
                if np.any(np.abs(got - want) > bound):
                    caught.setdefault(d, []).append((name, r))
    # the walk's defect shows in the contexts it hands to the same arithmetic
    c = R.BEAM_CASE
    beam = R.beam_case()
    for di in c["steps"]:
        good, _ = R.beam_contexts(beam, di, c["B"], c["k"], c["max_len"], 3, c["V"])
        bad, _ = R.beam_contexts(beam, di, c["B"], c["k"], c["max_len"], 3, c["V"], defect="walk_follows_slot")
        if not np.array_equal(good, bad):
            caught.setdefault("walk_follows_slot", []).append(di)
    assert set(caught) == set(R.DEFECTS) and len(R.DEFECTS) >= 7, sorted(set(R.DEFECTS) - set(caught))
    assert 0 not in caught["walk_follows_slot"] and 1 not in caught["walk_follows_slot"]     # (nothing to follow before step 2)


def test_the_beam_case_has_what_the_walk_must_handle():
    c = R.BEAM_CASE
    beam = R.beam_case()
    B, k, ml = c["B"], c["k"], c["max_len"]
    assert beam.shape == (2 * ml, B, k) and (c["B"], c["k"], c["max_len"], c["steps"]) == (3, 6, 10, (0, 1, 2, 7))
    assert beam[ml:].max() >= k and beam[ml:].min() < 0
    ctx, done = R.beam_contexts(beam, 0, B, k, ml, 3, c["V"])
    assert ctx.tolist() == [[-1, R.SOS]] * B and not done.any()
    ctx, done = R.beam_contexts(beam, 1, B, k, ml, 5, c["V"])
    assert ctx.shape == (B * k, 4) and np.all(ctx[:, :2] == -1) and np.all(ctx[:, 2] == R.SOS) and done.sum() == 1
    ctx, done = R.beam_contexts(beam, 7, B, k, ml, 5, c["V"])
    assert np.all(ctx >= 0) and done.sum() == 1
    ctx, done = R.beam_contexts(beam, 2, B, k, ml, 3, c["V"])
    assert done.sum() == 1


# ------------------------------------------------------------------------------------------------ the ABI's argument errors
def test_argument_errors_come_back_before_any_launch():
    """Every call below must fail on its arguments alone: no device exists here, and none is touched."""
    from vagnmt_hip import _lib
    L = _lib.lib()
    fake = 0x1000                                                       # never dereferenced: the checks come first
    m = LM().NgramLM.from_ngrams(3, 37, *R.to_arrays(R.case_model(37, 3), 3)).to("cpu")

    def model(**kw):
        s = _lib.Lm.from_buffer_copy(m.struct())
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def rows(M=1, ld=37):
        return (C.c_void_p * 8)(*[fake] * M), (C.c_int64 * 8)(*[ld] * M)

    def fuse(M=1, R_=2, V=37, lm=None, ctx=fake, beta=0.3, ld=37, r=True):
        p, l = rows(M if 1 <= M <= 8 else 1, ld)
        return L.vag_lm_fuse_rows(p if r else None, l, M, R_, V, C.byref(lm or model()), ctx, beta, None)

    def beam(M=1, di=0, ml=10, B=3, k=6, V=37, lm=None, beta=0.3, ld=37, buf=fake, dev=None):
        p, l = rows(M if 1 <= M <= 8 else 1, ld)
        if dev is not None:
            return L.vag_lm_fuse_beam_dev(p, l, M, buf, dev[0], ml, B, k, V, C.byref(lm or model()), beta, None)
        return L.vag_lm_fuse_beam(p, l, M, buf, di, ml, B, k, V, C.byref(lm or model()), beta, None)

    for bad in (dict(order=1), dict(order=6), dict(V=38), dict(V=0)):
        assert fuse(lm=model(**bad)) == -22 and beam(lm=model(**bad)) == -22, bad
        assert L.vag_lm_query(C.byref(model(**bad)), fake, fake, 4, fake, fake, None) == -22
    s = model()
    s.logp[2] = None
    assert fuse(lm=s) == -22
    s = model()
    s.child[1] = None
    assert beam(lm=s) == -22
    s = model()
    s.count[1] = 1 << 31
    assert fuse(lm=s) == -22
    assert fuse(V=36) == -22 and beam(V=38) == -22                        # V is not the model's
    assert fuse(M=0) == -22 and fuse(M=9) == -22 and beam(M=0) == -22 and beam(M=9) == -22
    assert fuse(ld=36) == -22 and beam(ld=36) == -22
    assert fuse(ctx=None) == -22 and fuse(r=False) == -22 and fuse(R_=0) == -22 and beam(buf=None) == -22
    assert L.vag_lm_fuse_rows(None, None, 1, 2, 37, C.byref(model()), fake, 0.3, None) == -22
    assert L.vag_lm_fuse_rows(*rows(), 1, 2, 37, None, fake, 0.3, None) == -22
    assert beam(k=65) == -22 and beam(ml=1025) == -22 and beam(di=10) == -22 and beam(di=-1) == -22 and beam(B=0) == -22
    assert beam(dev=(None,)) == -22
    for b in (float("nan"), float("inf"), -float("inf")):
        assert fuse(beta=b) == -22 and beam(beta=b) == -22
    for args in ((None, fake, 4, fake, fake), (fake, None, 4, fake, fake), (fake, fake, 0, fake, fake), (fake, fake, 4, None, fake),
                 (fake, fake, 4, fake, None)):
        assert L.vag_lm_query(C.byref(model()), *args, None) == -22
    assert L.vag_lm_query(None, fake, fake, 4, fake, fake, None) == -22
    # beta = 0 with good arguments is valid and launches nothing
    assert fuse(beta=0.0) == 0 and beam(beta=0.0) == 0 and beam(beta=0.0, dev=(fake,)) == 0


def test_python_side_checks_and_the_graph_key():
    lm = LM()
    a = lm.NgramLM.from_ngrams(3, 37, *R.to_arrays(R.case_model(37, 3, seed=0), 3))
    b = lm.NgramLM.from_ngrams(3, 37, *R.to_arrays(R.case_model(37, 3, seed=1), 3))
    with pytest.raises(_vag_error()):
        a.identity()                                                     # not on a device yet
    a.to("cpu")
    b.to("cpu")
    assert lm.graph_key(a, 0.3) != lm.graph_key(a, 0.2) and lm.graph_key(a, 0.3) != lm.graph_key(b, 0.3)
    assert lm.graph_key(a, 0.3) == lm.graph_key(a, 0.3)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lm.check_beta(bad)
    assert lm.check_beta(1) == 1.0 and lm.MAX_ORDER == 5 and lm.MAX_V == 131072
    s = a.struct()
    assert s.order == 3 and s.V == 37 and list(s.count)[:3] == a.counts and s.word[0] is None and s.bo[2] is None
    base = a.buffer.data_ptr()
    assert all((p - base) % 16 == 0 for p in (s.logp[0], s.bo[0], s.child[0], s.word[1], s.logp[2]))

    class FakeModel:
        tgt_size = 36

    with pytest.raises(ValueError):
        lm.check_lm(a, [FakeModel()], "cpu", "beamsearch_lm")
    with pytest.raises(ValueError):
        lm.check_lm("no model", [FakeModel()], "cpu", "beamsearch_lm")


def test_search_beam_refuses_raw_logits_with_a_language_model():
    from vagnmt_hip import search
    with pytest.raises(ValueError):
        search.beam([], [], 6, 10, raw_logits=True, lm=object())


def _vag_error():
    from vagnmt_hip import _lib
    return _lib.VagError
