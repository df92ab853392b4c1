"""CPU: the lexical shortlist's host side (vagnmt_hip.shortlist) and the invariants of its NumPy reference
(tests/shortlist_ref.py): the lexicon builders, the selection rule's own properties on every case of the table, the default
capacity, and the refusals that need no device."""
import numpy as np
import pytest
import torch

import shortlist_ref as R


def SL():
    from vagnmt_hip import shortlist
    return shortlist


# ------------------------------------------------------------------------------------------------------ lexicon
def test_from_counts_keeps_the_best_and_breaks_ties_by_target_id():
    src = [0, 0, 0, 0, 2, 2, 2, 0, 9, 1]
    tgt = [7, 5, 6, 8, 4, 9, 4, 5, 5, 99]
    cnt = [3, 2, 3, 1, 1, 2, 1, 2, 1, 5]           # word 0: 5 -> 4 (summed), 6 and 7 tie at 3, 8 -> 1; word 2: 4 -> 2 ties 9 -> 2
    lex = SL().Lexicon.from_counts(src, tgt, cnt, Vs=4, Vt=10, best=3)           # source 9 and target 99 are out of range
    assert lex.table.dtype == np.int32 and lex.table.shape == (4, 3) and (lex.Vs, lex.K, lex.Vt) == (4, 3, 10)
    assert lex.table.tolist() == [[5, 6, 7], [-1, -1, -1], [4, 9, -1], [-1, -1, -1]]
    one = SL().Lexicon.from_counts(src, tgt, cnt, Vs=4, Vt=10, best=1)
    assert one.table.tolist() == [[5], [-1], [4], [-1]]
    wide = SL().Lexicon.from_counts(src, tgt, cnt, Vs=4, Vt=10, best=100)        # K is the longest row, not `best`
    assert wide.table.tolist() == [[5, 6, 7, 8], [-1] * 4, [4, 9, -1, -1], [-1] * 4]
    empty = SL().Lexicon.from_counts([], [], [], Vs=3, Vt=10)
    assert empty.table.tolist() == [[-1]] * 3
    with pytest.raises(ValueError):
        SL().Lexicon.from_counts([0], [1], [1.0], 4, 10, best=257)
    with pytest.raises(ValueError):
        SL().Lexicon(np.zeros((2, 2), np.int32), Vt=0)


def test_lexicon_npz_round_trip_and_text(tmp_path):
    rng = np.random.default_rng(0)
    lex = SL().Lexicon.from_counts(rng.integers(0, 30, 500), rng.integers(0, 40, 500), rng.integers(1, 5, 500), 30, 40, best=6)
    path = str(tmp_path / "lex.npz")
    lex.save(path)
    back = SL().Lexicon.load(path)
    assert back.Vt == 40 and back.table.dtype == np.int32 and np.array_equal(back.table, lex.table)
    sv = {"<pad>": 0, "<unk>": 1, "<s>": 2, "</s>": 3, "haus": 4, "katze": 5}
    tv = {"<pad>": 0, "<unk>": 1, "<s>": 2, "</s>": 3, "house": 4, "home": 5, "cat": 6}
    text = tmp_path / "lex.txt"
    text.write_text("haus house 0.7\nhaus home 0.2\nkatze cat 0.9\nkatze house 0.01\nhund dog 0.9\nhaus cat notanumber\nbroken line\n"
                    "haus house 0.05\n", encoding="utf-8")
    lex = SL().Lexicon.from_text(str(text), sv, tv, best=2)
    assert (lex.Vs, lex.Vt, lex.K) == (6, 7, 2)
    assert lex.table[4].tolist() == [4, 5] and lex.table[5].tolist() == [6, 4] and (lex.table[:4] == -1).all()


# ------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_reference_invariants(name):
    c = dict(R.cases()[name])
    want_used = c.pop("rank_used", None)
    ids, n, used, f2s = R.select(**c)
    V, cap = c["V"], c["cap"]
    assert ids.shape == (cap,) and f2s.shape == (V,) and 0 <= n <= cap
    live = ids[:n]
    assert (np.diff(live) > 0).all() and (live >= 0).all() and (live < V).all() and (ids[n:] == -1).all()
    assert set(int(w) for w in c["always"] if 0 <= w < V) <= set(live.tolist())
    assert np.array_equal(f2s[live], np.arange(n)) and (f2s >= 0).sum() == n
    assert live[:4].tolist() == [0, 1, 2, 3]                     # the special words keep their ids
    if want_used is not None:
        assert used == want_used
    # the applied ranks are a prefix, and every word comes from `always` or an applied rank
    allowed = set(int(w) for w in c["always"])
    for r in range(used):
        allowed |= R.rank_words(c["src"], c["lengths"], c["lex"], r, V)
    assert set(live.tolist()) == allowed
    if used < c["best"]:                                         # the first dropped rank really would not fit
        assert len(allowed | R.rank_words(c["src"], c["lengths"], c["lex"], used, V)) > cap


def test_reference_gather():
    src = np.arange(20, dtype=np.float32).reshape(5, 4)
    ids = np.array([1, 4, -1, -1], np.int32)
    out = R.gather(ids, 2, 4, src, -1e30)
    assert np.array_equal(out[:2], src[[1, 4]]) and (out[2:] == np.float32(-1e30)).all()
    assert R.gather(ids, 2, 4, src[:, 0].copy(), 0.0).shape == (4, 1)


# ------------------------------------------------------------------------------------------------------ host rules
def test_default_capacity():
    cap = SL().default_capacity
    assert cap(9391, 104, 100) == 6656                           # 104 + 6400 = 6504 -> the next multiple of 256
    assert cap(9391, 104, 10) == 768
    assert cap(40000, 104, 100) == 6656
    assert cap(1000, 104, 100) == 1000                           # never above V
    assert cap(1000, 104, 2) == 256
    assert cap(300, 104, 2) == 256 and cap(250, 104, 2) == 250


def _cpu_model(tied=False, V=40):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(0)
    return NMT_Seq2Seq_Beam_V2(30, V, 8, 8, 8, tied_emb=tied).eval()


def test_refusals_without_a_device():
    S = SL()
    lex = S.Lexicon(np.full((30, 2), -1, np.int32), Vt=40)
    model = _cpu_model()
    with pytest.raises(ValueError, match="GPU"):
        S.Shortlist(model, lex, first=4, capacity=16)
    with pytest.raises(ValueError, match="lexicon"):
        S.Shortlist(model, S.Lexicon(np.full((30, 2), -1, np.int32), Vt=41), first=4, capacity=16)
    with pytest.raises(ValueError, match="lexicon"):
        S.Shortlist(model, np.zeros((30, 2), np.int32))
    with pytest.raises(ValueError, match="always"):
        S.Shortlist(model, lex, always=[0, 1, 2, 4, 5, 6, 7, 8], capacity=16)        # EOS missing
    with pytest.raises(ValueError, match="always"):
        S.Shortlist(model, lex, always=[0, 1, 2, 3, 40], capacity=16)
    with pytest.raises(ValueError, match="capacity"):
        S.Shortlist(model, lex, first=20, capacity=16)                                # 24 always ids
    with pytest.raises(ValueError, match="capacity"):
        S.Shortlist(model, lex, first=4, capacity=41)
    with pytest.raises(NotImplementedError, match="2-byte"):
        S.Shortlist(_cpu_model().half(), lex, first=4, capacity=16)
    with pytest.raises(ValueError, match="not a model"):
        S.Shortlist(torch.nn.Linear(2, 2), lex)
    with pytest.raises(ValueError, match="beam_size 5"):
        S.check_beam_width(5, 8)
    S.check_beam_width(4, 8)
    # nothing was attached to the model on the way
    assert not [k for k in model.__dict__ if "shortlist" in k]
