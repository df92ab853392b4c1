"""CPU: constrained beam search's host side -- the argument checks and the packing of vagnmt_hip.constrain, and the NumPy
reference itself (tests/constrain_ref.py), which the GPU tests compare the kernel against."""
import inspect

import numpy as np
import pytest
import torch

import constrain_ref as R

V, ML = 50, 10


def pack(**kw):
    from vagnmt_hip import constrain as C
    a = dict(prefix=None, banned=None, banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False)
    a.update(kw)
    return C.pack(2, V, ML, **a)


def test_every_value_error_names_its_argument():
    long_phrase = list(range(4, 13))                                    # 9 words
    bad = [
        (dict(banned=[[]]), "banned"),
        (dict(banned=[long_phrase]), "banned"),
        (dict(banned_per_sentence=[[[]], []]), "banned_per_sentence"),
        (dict(banned_per_sentence=[[], [long_phrase]]), "banned_per_sentence"),
        (dict(banned_per_sentence=[[[5]]]), "banned_per_sentence"),     # one list for two sentences
        (dict(banned=[[5 + i % 40] for i in range(200)], banned_per_sentence=[[[7]] * 57, []]), "257 phrases"),
        (dict(banned=[[V]]), "banned"),
        (dict(banned=[[5, -1]]), "banned"),
        (dict(banned=[[5, 0, 6]]), "banned"),                           # the padding word would cut the phrase short
        (dict(banned_per_sentence=[[], [[V + 3]]]), "banned_per_sentence"),
        (dict(prefix=[[5, 0], []]), "prefix"),
        (dict(prefix=[[R.SOS], []]), "prefix"),
        (dict(prefix=[[], [5, R.EOS]]), "prefix"),
        (dict(prefix=[[V], []]), "prefix"),
        (dict(prefix=[[-2], []]), "prefix"),
        (dict(prefix=torch.tensor([[5, 0, 6], [0, 0, 0]])), "prefix"),  # a zero inside a prefix
        (dict(prefix=torch.tensor([[5, 6]])), "prefix"),                # (1, Lp) for two sentences
        (dict(prefix=torch.tensor([[5, 6], [7, 8]], dtype=torch.int32)), "prefix"),
        (dict(prefix=[[5, 6]]), "prefix"),
        (dict(prefix=[list(range(4, 4 + ML)), []]), "prefix"),          # max_length words: longer than max_length - 1
        (dict(no_repeat_ngram=-1), "no_repeat_ngram"),
        (dict(no_repeat_ngram=9), "no_repeat_ngram"),
        (dict(prefix=[[5, 6, 6], []]), "avoid_double"),
        (dict(prefix=[[5, R.UNK], []], avoid_unk=True), "avoid_unk"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name) as err:
            pack(**kw)
        assert "beamsearch_constrained" in str(err.value), kw
    # what the two search options allow when they are off, and UNK as a FIRST word (step 0 applies no penalty)
    assert pack(prefix=[[5, 6, 6], []], avoid_double=False).prefix.tolist() == [[5, 6, 6], [0, 0, 0]]
    assert pack(prefix=[[R.UNK, 5], [5, R.UNK]]).prefix.tolist() == [[1, 5], [5, 1]]
    assert pack(prefix=[[R.UNK, 5], []], avoid_unk=True).prefix.tolist() == [[1, 5], [0, 0]]
    assert pack(prefix=[list(range(4, 4 + ML - 1)), []]).prefix.shape == (2, ML - 1)
    assert pack(banned=[[5]] * 256).phrases.shape == (256, 8) and pack(no_repeat_ngram=8).ngram == 8


def test_packing():
    p = pack(prefix=[[5, 6], []], banned=[[7], [8, 9]], banned_per_sentence=[[], [[4, 4, 4], list(range(10, 18))]],
             no_repeat_ngram=2)
    assert p.prefix.dtype == np.int64 and p.prefix.tolist() == [[5, 6], [0, 0]]
    assert p.phrases.dtype == np.int64 and p.phrases.tolist() == [[7, 0, 0, 0, 0, 0, 0, 0], [8, 9, 0, 0, 0, 0, 0, 0],
                                                                  [4, 4, 4, 0, 0, 0, 0, 0], list(range(10, 18))]
    assert p.phrase_sent.dtype == np.int32 and p.phrase_sent.tolist() == [-1, -1, 1, 1] and p.ngram == 2
    t = pack(prefix=torch.tensor([[5, 6, 0, 0], [0, 0, 0, 0]]))                  # the tensor form, trailing padding dropped
    assert t.prefix.tolist() == [[5, 6], [0, 0]]
    e = pack()
    assert e.prefix.shape == (2, 0) and e.phrases.shape == (0, 8) and e.phrase_sent.shape == (0,) and e.ngram == 0
    assert pack(prefix=[[], []]).prefix.shape == (2, 0) and pack(banned=[], banned_per_sentence=[[], None]).phrases.shape == (0, 8)


def test_flat_buffer_layout_and_padding():
    from vagnmt_hip import constrain as C
    p = pack(prefix=[[5, 6], [7]], banned=[[8, 9]], banned_per_sentence=[[[4]], [[11, 12, 13]]])
    a, b, size = C.flat_layout(2, 2, 3)
    assert (a, b, size) == (4, 4 + 24, 4 + 24 + 2)
    flat = C.flatten(p, 2, 2, 3)
    assert flat[:a].reshape(2, 2).tolist() == [[5, 6], [7, 0]] and flat[a:b].reshape(3, 8).tolist() == p.phrases.tolist()
    assert flat[b:].view(np.int32)[:3].tolist() == [-1, 0, 1]
    # a graph entry's static buffer: padded to (B, max_length) and MAX_PHRASES, every word of it rewritten
    a, b, size = C.flat_layout(2, ML, C.MAX_PHRASES)
    big = C.flatten(p, 2, ML, C.MAX_PHRASES)
    assert big.shape == (size,) and size == 2 * ML + 256 * 8 + 128
    pre, phr = big[:a].reshape(2, ML), big[a:b].reshape(256, 8)
    assert pre[:, :2].tolist() == [[5, 6], [7, 0]] and not pre[:, 2:].any()
    assert phr[:3].tolist() == p.phrases.tolist() and not phr[3:].any()
    assert C.MAX_LEN == R.MAX_LEN == 8 and C.MAX_PHRASES == R.MAX_PHRASES == 256
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "vag_nmt.h")).read()
    assert "#define VAG_CONSTRAIN_MAX_LEN     8" in hdr and "#define VAG_CONSTRAIN_MAX_PHRASES 256" in hdr


def test_public_signatures():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip import constrain as C
    from vagnmt_hip.ensemble import Ensemble
    tail = [("beam_size", 12), ("n_best", 1), ("max_length", 80), ("prefix", None), ("banned", None),
            ("banned_per_sentence", None), ("no_repeat_ngram", 0), ("avoid_double", True), ("avoid_unk", False)]
    for cls, lead in [(NMT_AttentionImagine_Seq2Seq_Beam_V11, ["self", "src_var", "src_lengths", "im_var"]),
                      (NMT_Seq2Seq_Beam_V2, ["self", "src_var", "src_lengths"]),           # no im_var, as beamsearch_nbest
                      (Ensemble, ["self", "src_var", "src_lengths", "im_var"])]:
        p = inspect.signature(cls.beamsearch_constrained).parameters
        assert list(p)[:len(lead)] == lead and [(n, p[n].default) for n in list(p)[len(lead):]] == tail, cls
    assert C.Constrained._fields == ("hyps", "scores")
    from vagnmt_hip import search
    assert inspect.signature(search.beam).parameters["constrain"].default is None
    with pytest.raises(ValueError, match="raw_logits"):
        search.beam([], [], 2, 4, raw_logits=True, constrain=object())


# ---- the reference's own properties ---------------------------------------------------------------------------------------
def table(B=2, k=3, max_len=6):
    """A history by hand: words in rows [0, max_len), back-pointers in rows [max_len, 2 max_len)."""
    beam = np.zeros((2 * max_len, B, k), dtype=np.int64)
    beam[0, 0], beam[1, 0], beam[2, 0] = [4, 5, 6], [7, 8, 3], [9, 4, 5]
    beam[max_len + 1, 0], beam[max_len + 2, 0] = [2, 0, 1], [0, 0, 1]
    beam[0, 1], beam[1, 1], beam[2, 1] = [10, 11, 12], [10, 10, 10], [13, 3, 10]
    beam[max_len + 1, 1], beam[max_len + 2, 1] = [0, 1, 2], [2, 1, 0]
    return beam, max_len


def rows(N, V_, ldl, seed=0):
    a = np.full((N, ldl), np.nan, dtype=np.float32)
    a[:, :V_] = np.random.default_rng(seed).standard_normal((N, V_)).astype(np.float32)
    return a


def test_history_follows_the_back_pointers():
    beam, ml = table()
    assert R.history(beam, ml, 0, 0, 0) == []
    assert R.history(beam, ml, 3, 0, 0) == [6, 7, 9]       # slot 0 <- slot 0 (word 7) <- slot 2 (word 6)
    assert R.history(beam, ml, 3, 0, 1) == [6, 7, 4]
    assert R.history(beam, ml, 3, 0, 2) == [4, 8, 5]
    assert R.history(beam, ml, 2, 0, 2) == [5, 3] and R.history(beam, ml, 3, 1, 0) == [12, 10, 13]


def test_reference_properties():
    beam, ml = table()
    B, k, Vv, ldl = 2, 3, 20, 23
    src = [rows(B * k, Vv, ldl, 1), rows(B * k, Vv, ldl, 2)]
    prefix = np.array([[4, 7, 9, 15], [0, 0, 0, 0]], dtype=np.int64)
    phrases = np.zeros((5, 8), dtype=np.int64)
    phrases[0, :1], phrases[1, :3], phrases[2, :2], phrases[4, :2] = [15], [10, 13, 16], [13, 17], [13, 18]
    sent = np.array([-1, -1, 0, -1, 1], dtype=np.int32)
    c = R.new_counts()
    out = R.mask(src, beam, 3, ml, B, k, Vv, prefix, phrases, sent, 1, c)
    for s, o in zip(src, out):
        assert np.isnan(o[:, Vv:]).all() and not np.isnan(o[:, :Vv]).any()          # columns >= V untouched
        # sentence 0: every live row is forced to 15 -- and ignores the ban on 15 and the n = 1 ban of its history
        for n_ in (0, 1, 2):
            keep = np.ones(Vv, dtype=bool)
            keep[15] = False
            assert (o[n_, :Vv][keep] == R.NEG_PEN).all() and o[n_, 15] == s[n_, 15]
        # sentence 1: slot 1 is finished (previous word EOS): untouched
        assert o[4].tobytes() == s[4].tobytes()
        # slot 0, history [12, 10, 13]: 15 (unigram), 16 (10 13 16), 18 (13 18, its sentence), not 17 (sentence 0's phrase),
        # and the whole history (n = 1); the empty phrase row does nothing
        hit = sorted(np.flatnonzero(o[3, :Vv] == R.NEG_PEN).tolist())
        assert hit == [10, 12, 13, 15, 16, 18]
        rest = np.setdiff1d(np.arange(Vv), hit)
        assert o[3, rest].tobytes() == s[3, rest].tobytes()
        # slot 2, history [10, 10, 10]
        assert sorted(np.flatnonzero(o[5, :Vv] == R.NEG_PEN).tolist()) == [10, 15]
    assert c["forced"] == 3 and c["finished"] == 1 and c["unigram"] == 2 and c["multiword"] == 1 and c["ngram"] == {1: 2}
    assert all(np.isnan(s[:, Vv:]).all() for s in src)                                   # copies: the inputs are what they were
    # n-grams: history [12, 10, 13] then [.., 10]: with n = 2 the context (10) occurred before, followed by 13
    beam[3, 1, 0], beam[ml + 3, 1, 0] = 10, 0
    o = R.mask([src[0]], beam, 4, ml, B, k, Vv, None, (), (), 2)[0]
    assert np.flatnonzero(o[3, :Vv] == R.NEG_PEN).tolist() == [13]
    o = R.mask([src[0]], beam, 4, ml, B, k, Vv, None, (), (), 3)[0]
    assert not (o[3, :Vv] == R.NEG_PEN).any()
    # a banned or forced word outside [0, V) writes nothing; step 0 is constrained too
    far = np.zeros((1, 8), dtype=np.int64)
    far[0, 0] = Vv + 1
    s0 = rows(B, Vv, ldl, 3)
    assert R.mask([s0], beam, 0, ml, B, k, Vv, np.array([[Vv], [0]]), far, np.array([-1], dtype=np.int32), 0)[0].tobytes() == s0.tobytes()
    o = R.mask([s0], beam, 0, ml, B, k, Vv, np.array([[6], [0]]), phrases, sent, 2)[0]
    assert np.flatnonzero(o[0, :Vv] != R.NEG_PEN).tolist() == [6] and np.flatnonzero(o[1, :Vv] == R.NEG_PEN).tolist() == [15]


def test_expansion_order_and_search():
    lp = np.zeros((2, 6), dtype=np.float32)
    lp[0] = [-1, -1, -3, -9, -1, -2]
    lp[1] = [-2, -1, -1, -9, -1, -1]
    w, p, sc = R.expand(lp, np.float32([0.0, 0.0]), np.array([4, 5]), 4)
    # row 0's previous word 4 and row 1's 5 are ruled out; ties go to the lower flat index
    assert w.tolist() == [0, 1, 1, 2] and p.tolist() == [0, 0, 1, 1] and sc.tolist() == [-1, -1, -1, -1]
    w, p, sc = R.expand(lp, np.float32([0.0, -1.0]), np.array([R.EOS, 5]), 3, R.ALLOW_REPEAT | R.AVOID_UNK)
    assert w.tolist() == [R.EOS, 2, 4] and p.tolist() == [0, 1, 1] and sc.tolist() == [0, -2, -2]
    T = (np.random.default_rng(3).integers(-96, 1, size=(12, 12)) / 8.0).astype(np.float32)
    prefix = np.array([[5, 6], [0, 0]], dtype=np.int64)
    beam, nll = R.search(lambda tok: T[tok], 2, 3, 12, 5, 5, prefix, np.array([[7, 0, 0, 0, 0, 0, 0, 0]]), np.array([-1], dtype=np.int32), 2)
    assert beam[0, 0, 0] == 5 and beam[1, 0, 0] == 6 and nll[0, 0] > -1e4
    for b in range(2):
        for j in range(3):
            h = R.history(beam, 5, 5, b, j)
            if nll[b, j] > -1e4:
                assert 7 not in h
                cut = h[:h.index(R.EOS)] if R.EOS in h else h
                grams = list(zip(cut, cut[1:]))
                assert len(set(grams)) == len(grams)
