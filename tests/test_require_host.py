"""CPU: the required-phrase search's host side -- the argument checks and packing of vagnmt_hip.require, and the NumPy reference
itself (tests/require_ref.py), which the GPU tests compare the kernels against."""
import inspect
import itertools

import numpy as np
import pytest

import constrain_ref as CR
import require_ref as R

V, ML = 50, 10


def pack(**kw):
    from vagnmt_hip import require as Q
    a = dict(required=None, banned=None, banned_per_sentence=None, avoid_double=True, avoid_unk=False)
    a.update(kw)
    return Q.pack(2, V, ML, **a)


def test_slot_order_is_the_round_robin_loop():
    """(rho ascending, bank descending) against the literal loop "best unseen of each bank, highest bank first, repeat", on
    random pools with ties in the values (a grid of 1/8), dead candidates and fewer live candidates than slots."""
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        k = int(rng.integers(1, 13))
        vals = (rng.integers(-40, 1, size=n) / 8.0).astype(np.float32)
        vals[rng.random(n) < 0.3] -= np.float32(1e5)
        flat = rng.permutation(1000)[:n]
        banks = rng.integers(0, 5, size=n)
        cands = [(vals[i], int(flat[i]), int(banks[i])) for i in range(n)]
        a, b = R.slot_order(cands, k), R.round_robin(cands, k)
        assert a == b, trial
        assert len(a) == min(n, k)
        live = [t for t in a if t[0] > R.LIVE]
        assert a[:len(live)] == live                                    # no dead candidate before a live one
        if live:
            assert live[0][2] == max(t[2] for t in cands if t[0] > R.LIVE)      # slot 0: the best of the highest bank


def brute_progress(phrase, L, history):
    """The longest prefix of the phrase that is a suffix of the history, L (met) as soon as the phrase occurred."""
    for q in range(min(L, len(history)), 0, -1):
        if history[len(history) - q:] == list(phrase[:q]):
            return q
    return 0


def test_transition_is_exact_substring_matching():
    """Progress kept step by step with R.transition equals, after every word, the brute-force longest border; the phrase is
    met exactly when it occurs.  Random strings over {4, 5, 6}, every phrase of 1 .. 4 letters over it, a a b and a b a b c."""
    a, b, c = 4, 5, 6
    phrases = [list(p) for n in (1, 2, 3, 4) for p in itertools.product((a, b, c), repeat=n)] + [[a, a, b], [a, b, a, b, c]]
    rng = np.random.default_rng(1)
    strings = [list(rng.integers(4, 7, size=12)) for _ in range(40)] + [[a, a, a, b], [a, b, a, b, a, b, c]]
    for ph in phrases:
        L = len(ph)
        for s in strings:
            s = [int(x) for x in s]
            p, met = 0, False
            for t, w in enumerate(s):
                p = R.transition(ph, L, p, w)
                assert p == brute_progress(ph, L, s[:t + 1]), (ph, s, t)
                if p == L:
                    met = True
                    break
            assert met == CR_contains(s, ph), (ph, s)
    assert R.transition([a, a, b], 3, 2, a) == 2 and R.transition([a, a, b], 3, 2, b) == 3
    assert R.transition([a, b, a, b, c], 5, 4, a) == 3 and R.transition([a, b, a, b, c], 5, 4, c) == 5


def CR_contains(s, ph):
    return R.contains(s, ph)


def test_child_state_packs_met_progress_and_bank():
    table = R.table_of([[[4], [5, 6, 7], None, [5, 8]] + [None] * 5 + [[9, 4, 9]]], 1)[0]
    assert R.lengths(table) == [1, 3, 0, 2, 0, 0, 0, 0, 0, 3] + [0] * 6
    s = R.child(R.ZERO, False, 5, table)
    assert s == (0, (1 << 4) | (1 << 12), 0, 2)                         # phrases 1 and 3 share their first word
    s = R.child(s, False, 8, table)
    assert s == (1 << 3, 0, 0, 2)                                       # phrase 3 met, phrase 1 reset
    s = R.child(s, False, 9, table)
    assert s == (1 << 3, 0, 1 << 4, 3)                                  # phrase 9 lives in prog_hi
    s2 = R.child(s, False, 4, table)
    assert s2 == ((1 << 3) | 1, 0, 2 << 4, 5)                           # one word meets phrase 0 and advances phrase 9
    assert R.child(s2, True, 9, table) == s2                            # a finished row keeps its state
    s3 = R.child(s2, False, 9, table)
    assert s3 == ((1 << 3) | 1 | (1 << 9), 0, 0, 6)
    assert R.is_open(s3, False, table) and not R.is_open(s3, True, table)
    assert not R.is_open(R.ZERO, False, np.zeros((16, 8), dtype=np.int64))


def test_reference_without_phrases_is_the_constrained_reference():
    rng = np.random.default_rng(7)
    B, k, Vt, steps = 2, 6, 50, 8
    T = (rng.integers(-96, 1, size=(Vt, Vt)) / 8.0).astype(np.float32)
    T[:, R.EOS] += np.float32(1.5)
    none = np.zeros((B, 16, 8), dtype=np.int64)
    for flags in (0, 3):
        want_beam, want_nll = CR.search(lambda tok: T[tok], B, k, Vt, steps, steps, flags=flags)
        beam, nll, state = R.search(lambda tok: [T[tok]], B, k, Vt, steps, steps, none, flags)
        assert beam.tobytes() == want_beam.tobytes() and nll.tobytes() == want_nll.tobytes()
        assert not state.any()
    # and through the mask: a prefix and a ban
    prefix = np.array([[7, 9, 11], [8, 0, 0]], dtype=np.int64)
    phrases = np.zeros((1, 8), dtype=np.int64)
    phrases[0, :1] = [12]
    sent = np.array([-1], dtype=np.int32)
    want_beam, want_nll = CR.search(lambda tok: T[tok], B, k, Vt, steps, steps, prefix, phrases, sent, 2)
    beam, nll, _ = R.search(lambda tok: [T[tok]], B, k, Vt, steps, steps, none, prefix=prefix, phrases=phrases, phrase_sent=sent,
                            ngram=2)
    assert beam.tobytes() == want_beam.tobytes() and nll.tobytes() == want_nll.tobytes()


def test_reference_search_meets_its_phrases():
    """A whole reference search: the states it carries are what the words say, hypotheses that ended have met everything."""
    rng = np.random.default_rng(3)
    B, k, Vt, steps = 2, 5, 40, 10
    T = (rng.integers(-96, 1, size=(Vt, Vt)) / 8.0).astype(np.float32)
    T[:, R.EOS] += np.float32(3.0)
    lists = [[[30], [31, 32, 31], None, [31, 33]], []]
    table = R.table_of(lists, B)
    counts = R.new_counts()
    beam, nll, state = R.search(lambda tok: [T[tok]], B, k, Vt, steps, steps, table, 0, counts)
    assert counts["completed"] > 0 and counts["eos_ruled_out"] > 0
    ended = 0
    for b in range(B):
        for j in range(k):
            h = CR.history(beam, steps, steps, b, j)
            words = h[:h.index(R.EOS)] if R.EOS in h else h
            met = int(state[b, j, 0])
            for c, ph in enumerate(lists[b]):
                if ph:
                    assert bool((met >> c) & 1) == R.contains(words, ph), (b, j, c, h)
            if R.EOS in h and nll[b, j] > -1e4:
                ended += 1
                assert all(R.contains(words, ph) for ph in lists[b] if ph), (b, j, h)
    assert ended >= 3


def test_every_value_error_names_its_argument():
    long_phrase = list(range(4, 13))                                    # 9 words
    bad = [
        (dict(required=[[[5]] * 17, []]), "required"),
        (dict(required=[[[]], []]), "required"),
        (dict(required=[[long_phrase], []]), "required"),
        (dict(required=[[[V]], []]), "required"),
        (dict(required=[[[0]], []]), "required"),
        (dict(required=[[[5, -1]], []]), "required"),
        (dict(required=[[[R.SOS]], []]), "SOS"),
        (dict(required=[[], [[5, R.EOS]]]), "EOS"),
        (dict(required=[[[5, 6, 6]], []]), "avoid_double"),
        (dict(required=[[[5, R.UNK]], []], avoid_unk=True), "avoid_unk"),
        (dict(required=[[[5, 6, 7]], []], banned=[[6, 7]]), "banned"),
        (dict(required=[[], [[5, 6, 7]]], banned_per_sentence=[[], [[6]]]), "banned"),
        (dict(required=[[[4, 5, 6, 7], [8, 9, 10], [11, 12, 13]], []]), "max_length"),     # 10 words > max_length - 1
        (dict(required=[[[5]]]), "required"),                                                # one list for two sentences
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name) as err:
            pack(**kw)
        assert "beamsearch_required" in str(err.value) and "required" in str(err.value), kw
    # what the options allow when they are off; a ban of another sentence does not concern this one
    assert pack(required=[[[5, 6, 6]], []], avoid_double=False)[0, 0, :3].tolist() == [5, 6, 6]
    assert pack(required=[[[5, R.UNK]], []])[0, 0, :2].tolist() == [5, 1]
    assert pack(required=[[[5, 6, 7]], []], banned_per_sentence=[[], [[6]]])[0, 0, :3].tolist() == [5, 6, 7]
    assert pack(required=[[[4, 5, 6], [7, 8, 9], [10, 11, 12]], []]).shape == (2, 16, 8)       # 9 words = max_length - 1


def test_table_packing():
    from vagnmt_hip import require as Q
    t = pack(required=[[[5], [6, 7, 8], [5]], []])
    assert t.dtype == np.int64 and t.shape == (2, Q.MAX_PHRASES, Q.MAX_LEN) == (2, 16, 8)
    assert t[0, 0].tolist() == [5, 0, 0, 0, 0, 0, 0, 0] and t[0, 1].tolist() == [6, 7, 8, 0, 0, 0, 0, 0]
    assert t[0, 2].tolist() == t[0, 0].tolist()                          # identical phrases are allowed
    assert not t[0, 3:].any() and not t[1].any()
    assert not pack().any() and not pack(required=[[], []]).any() and not pack(required=[None, []]).any()
    assert Q.given_masks(t).tolist() == [0b111, 0]
    assert R.lengths(t[0])[:4] == [1, 3, 1, 0]
    assert Q.pack(2, V, 17, required=[[[5]] * 16, []])[0, :, 0].tolist() == [5] * 16      # 16 words = max_length - 1


def test_public_signatures():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip import require as Q
    want = dict(im_var=None, beam_size=12, n_best=1, max_length=80, required=None, prefix=None, banned=None,
                banned_per_sentence=None, no_repeat_ngram=0, avoid_double=True, avoid_unk=False)
    for cls in (NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2, Ensemble):
        p = inspect.signature(cls.beamsearch_required).parameters
        assert list(p)[:3] == ["self", "src_var", "src_lengths"] and list(p)[3:] == list(want), cls
        for name, default in want.items():
            assert p[name].default == default, (cls, name)
    assert Q.Required._fields == ("hyps", "scores", "met", "complete")
    from vagnmt_hip import constrain, search
    assert "vagnmt_hip.require" in constrain.__doc__ and callable(search.beam_required)
