"""CPU: minimum-Bayes-risk selection without a device -- the float64 restatement (tests/mbr_ref.py) against the fixture recorded
from the reference's bleu.py (tests/golden/mbr_bleu.npz, tools/make_golden_mbr.py), the packing of token lists, and the host side
of the library's entry points."""
import os

import numpy as np
import pytest
import torch

import mbr_ref as R
from conftest import ROOT

EOS = 3


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mbr_bleu.npz"))
    return [(z["tok%d" % s], z["m%d" % s], z["bleu%d" % s]) for s in range(int(z["n_sets"]))]


def test_restatement_reproduces_the_reference():
    pairs = clipped = 0
    for tok, m_gold, u_gold in golden():
        m, lh, lr = R.pairwise(tok)
        u = R.utilities(m, lh, lr, "bleu")
        have = ~np.isnan(u_gold)
        # the fixture skips exactly the pairs with an empty reference span
        assert np.array_equal(have, np.broadcast_to((lr > 0)[:, None, :], have.shape))
        assert np.array_equal(m[have], m_gold[have].astype(np.int64))                     # integer for integer
        assert float(np.abs(u - u_gold)[have].max()) <= 1e-12
        pairs += int(have.sum())
        # clipping occurs: some pair has fewer clipped matches than the candidate's matching positions
        for b in range(tok.shape[0]):
            spans = [R.span(r) for r in tok[b]]
            for i, h in enumerate(spans):
                for j, r in enumerate(spans):
                    clipped += sum(t in r for t in h) > m[b, i, j, 0]
    assert pairs > 200 and clipped > 20


def test_restatement_on_hand_cases():
    a = 7
    assert R.matches([a] * 4, [a] * 2) == [2, 1, 0, 0]                                    # "a a a a" against "a a"
    assert R.matches([a] * 2, [a] * 4) == [2, 1, 0, 0]                                    # symmetric
    assert R.span([5, 0, 6, EOS, 5, 0]) == [5, 0, 6] and R.span([EOS, 5]) == [] and R.span([5, 6]) == [5, 6]
    assert R.bleu([4, 3, 2, 1], 4, 4) == 1.0 and R.bleu([0, 0, 0, 0], 0, 4) == 0.0
    assert R.bleu([0, 0, 0, 0], 2, 0) == pytest.approx((1 / 3 * 1 / 2) ** 0.25)           # an empty reference: bp = 1
    assert R.ngram_f([4, 3, 2, 1], 4, 4) == 1.0 and R.ngram_f([0, 0, 0, 0], 0, 0) == 0.0
    assert R.ngram_f([1, 0, 0, 0], 1, 2) == pytest.approx((2 / 3 + 0) / 2)               # orders 1 and 2 exist, 3 and 4 do not


def test_packing():
    from vagnmt_hip import mbr
    t = mbr.pack([[[5, 6], [7]], [[8, 9, 10], []]])
    assert t.dtype == torch.int64 and t.tolist() == [[[5, 6, EOS, 0], [7, EOS, 0, 0]], [[8, 9, 10, EOS], [EOS, 0, 0, 0]]]
    assert mbr.pack([[[5, EOS, 9]]]).tolist() == [[[5, EOS, 9]]]                          # a list that holds an EOS is kept
    with pytest.raises(ValueError):
        mbr.pack([[[5], [6]], [[7]]])                                                     # ragged N
    with pytest.raises(ValueError):
        mbr.pack([])
    x = torch.zeros(2, 3, 4, dtype=torch.int64)
    assert mbr.pack(x) is x                                                               # a tensor passes through


def test_host_checks():
    from vagnmt_hip import mbr
    with pytest.raises(ValueError, match="no CPU path"):
        mbr.mbr_select(torch.zeros(1, 2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="utility"):
        mbr.mbr_select(torch.zeros(1, 2, 3, dtype=torch.int64), utility="chrf")
    with pytest.raises(ValueError, match="beam_size"):
        mbr.decode_args(4, 10, 65, "bleu")
    with pytest.raises(ValueError, match="utility"):
        mbr.decode_args(4, 10, 0, "meteor")
    with pytest.raises(ValueError, match="unsupported shape"):
        mbr.decode_args(1024, 10, 1, "bleu")                                              # 1025 candidates
    assert mbr.decode_args(16, 80, 4, "ngram_f") == (4, 1)


def test_entry_points_on_the_host():
    import ctypes as C
    from vagnmt_hip import _lib
    L = _lib.lib()
    assert L.vag_mbr_supported(256, 256, 256, 256) == 1 and L.vag_mbr_supported(1, 1, 1, 1) == 1
    assert L.vag_mbr_supported(0, 256, 256, 256) == 0 and L.vag_mbr_supported(256, 256, 256, 0) == 0
    assert L.vag_mbr_supported(1024, 512, 1024, 512) == 1                                 # the limits of include/vag_nmt.h
    assert L.vag_mbr_supported(1025, 512, 1024, 512) == 0 and L.vag_mbr_supported(1024, 513, 1024, 512) == 0
    assert L.vag_mbr_supported(1024, 512, 1025, 512) == 0 and L.vag_mbr_supported(1024, 512, 1024, 513) == 0
    # argument errors come back as -EINVAL before anything touches a device (the pointers are never dereferenced)
    assert L.vag_mbr_select(None, None, None, 1, 2, 3, 2, 3, 0, None, None, None, None, None) == -22
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.vag_mbr_select(p, None, None, 1, 2, 3, 2, 3, 0, None, None, None, p, None) == -22       # expected NULL
    assert L.vag_mbr_select(p, None, None, 1, 2, 3, 2, 3, 0, None, None, p, None, None) == -22       # best NULL
    assert L.vag_mbr_select(p, None, None, 0, 2, 3, 2, 3, 0, None, None, p, p, None) == -22          # a size below 1
    assert L.vag_mbr_select(p, None, None, 1, 2, 0, 2, 0, 0, None, None, p, p, None) == -22
    assert L.vag_mbr_select(p, None, None, 1, 2, 3, 2, 3, 2, None, None, p, p, None) == -22          # an unknown utility
    assert L.vag_mbr_select(p, None, None, 1, 2, 3, 2, 3, -1, None, None, p, p, None) == -22
    assert L.vag_mbr_select(p, None, None, 1, 2, 3, 4, 3, 0, None, None, p, p, None) == -22          # refs NULL: the shapes differ
    assert L.vag_mbr_select(p, p, None, 1, 2, 600, 2, 3, 0, None, None, p, p, None) == -22           # an unsupported shape
    assert L.vag_mbr_select(p, p, None, 1 << 21, 2, 3, 2, 3, 0, None, None, p, p, None) == -22


def test_mbr_decode_argument_checks():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.ensemble import Ensemble
    m = NMT_AttentionImagine_Seq2Seq_Beam_V11(30, 40, 24, 8, 8, 16, 12, 0.99).eval()
    t = NMT_Seq2Seq_Beam_V2(30, 40, 8, 8, 16).eval()
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    for obj in (m, t, Ensemble([m, t])):
        for kw, word in ((dict(beam_size=65), "beam_size"), (dict(utility="chrf"), "utility"), (dict(n_samples=0), "n_samples"),
                         (dict(top_p=0.0), "top_p"), (dict(top_k=65), "top_k"), (dict(max_length=600), "unsupported shape"),
                         (dict(), "GPU tensor")):                                 # everything in range, but a CPU src_var
            with pytest.raises(ValueError, match="mbr_decode.*" + word):
                obj.mbr_decode(src, [5, 5], im, **kw)
