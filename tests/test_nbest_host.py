"""CPU: host-side checks of the n-best search and forced scoring (no device), the C ABI's argument errors of the new entries, and
the option fixture (tests/golden/beam_opts.npz) being able to tell the options apart."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

UNK, EOS = 1, 3


def _v11(Vs=30, Vt=40, H=16, seed=0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, 24, 8, 8, H, 12, 0.99).eval()


def _v2(Vs=30, Vt=40, H=16, seed=0):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    return NMT_Seq2Seq_Beam_V2(Vs, Vt, 8, 8, H).eval()


def test_nbest_argument_checks():
    from vagnmt_hip.ensemble import Ensemble
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    m, t = _v11(), _v2()
    for k, n in [(3, 0), (3, 4), (65, 2), (65, 65), (0, 0)]:
        with pytest.raises(ValueError):
            m.beamsearch_nbest(src, [5, 5], im, k, n, 4)
        with pytest.raises(ValueError):
            t.beamsearch_nbest(src, [5, 5], k, n, 4)
        with pytest.raises(ValueError):
            Ensemble([m, t]).beamsearch_nbest(src, [5, 5], im, k, n, 4)
    # in range, but CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        m.beamsearch_nbest(src, [5, 5], im, 3, 2, 4)
    with pytest.raises(ValueError):
        t.beamsearch_nbest(src, [5, 5], 64, 64, 4)
    with pytest.raises(ValueError):
        Ensemble([t]).beamsearch_nbest(src, [5, 5], None, 1, 1, 4)
    with pytest.raises(ValueError):
        m.score_translations(src, [5, 5], [[4, 5], [6]], im)
    with pytest.raises(ValueError):
        t.score_translations(src, [5, 5], [[4, 5], [6]])
    with pytest.raises(ValueError):
        Ensemble([m, t]).score_translations(src, [5, 5], [[4, 5], [6]], im)


def test_beamsearch_options_are_accepted_on_the_reference_layout():
    """The public beamsearch(...) takes the reference's options with the reference's decoder_input (the (B, 1) SOS tensor): on CPU
    tensors it then fails only for want of a device.  decoder_input=None stays the default-only shorthand it always was."""
    from vagnmt_hip._lib import VagError
    m = _v2()
    enc, mask, h = torch.zeros(5, 2, 32), torch.ones(5, 2), torch.zeros(1, 2, 16)
    sos = torch.full((2, 1), 2, dtype=torch.int64)
    for ad, au in [(False, False), (True, True), (False, True)]:
        with pytest.raises(VagError):
            m.beamsearch(enc, mask, sos, h, 3, 4, avoid_double=ad, avoid_unk=au)
        with pytest.raises(NotImplementedError):
            m.beamsearch(enc, mask, None, h, 3, 4, avoid_double=ad, avoid_unk=au)
    with pytest.raises(ValueError):
        m.beamsearch(enc, mask, sos + 1, h, 3, 4, avoid_unk=True)         # every hypothesis starts from SOS


def test_flags_encoding():
    from vagnmt_hip.scoring import beam_flags
    assert beam_flags() == 0                              # the reference's defaults: today's kernels
    assert beam_flags(avoid_double=False) == 1
    assert beam_flags(avoid_unk=True) == 2
    assert beam_flags(False, True) == 3


def test_targets_list_to_padded_tensor():
    from vagnmt_hip.scoring import targets_tensor
    t = targets_tensor([[5, 6, 7], [8, EOS], [], [9, EOS, 4]], 4)
    assert t.dtype == torch.int64 and t.shape == (4, 4)
    assert t.tolist() == [[5, 6, 7, EOS], [8, EOS, 0, 0], [EOS, 0, 0, 0], [9, EOS, 4, 0]]
    # numpy integers (n-best output) are taken as they are
    t = targets_tensor([np.array([4, 5], dtype=np.int64), [np.int64(6)]], 2)
    assert t.tolist() == [[4, 5, EOS], [6, EOS, 0]]
    x = torch.tensor([[4, 5, EOS, 0]])
    assert targets_tensor(x, 1) is x or torch.equal(targets_tensor(x, 1), x)
    with pytest.raises(ValueError):
        targets_tensor([[4]], 2)                          # one list for two sentences
    with pytest.raises(ValueError):
        targets_tensor(torch.zeros(3, 4, dtype=torch.int64), 2)
    with pytest.raises(ValueError):
        targets_tensor(torch.zeros(2, 4, dtype=torch.int32), 2)


def test_cut_nbest():
    from vagnmt_hip.scoring import cut_nbest
    out = np.array([[[5, 6, EOS, 0], [7, EOS, EOS, EOS], [9, 9, 9, EOS]]])
    assert cut_nbest(out, 2) == [[[5, 6], [7]]]
    assert cut_nbest(out, 3) == [[[5, 6], [7], [9, 9, 9]]]


def test_new_abi_argument_errors_are_negative_codes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    assert L.vag_version() == 330
    # n-best finish: n out of [1, k], k > 64, steps > max_len (every check precedes any launch)
    assert L.vag_beam_finish_nbest(None, None, 10, 5, 2, 3, 1, None, None, None) == -22
    x = C.c_void_p(16)
    for ml, steps, B, k, n in [(10, 5, 2, 3, 0), (10, 5, 2, 3, 4), (10, 5, 2, 65, 2), (10, 11, 2, 3, 1), (10, 5, 0, 3, 1)]:
        assert L.vag_beam_finish_nbest(x, x, ml, steps, B, k, n, x, x, None) == -22, (ml, steps, B, k, n)
    # expansions: a flag bit outside VAG_BEAM_ALLOW_REPEAT | VAG_BEAM_AVOID_UNK
    assert L.vag_beam_step_opt(x, 16, x, x, 0, 10, x, x, 2, 3, 16, 8, x, x, 4, None) == -22
    assert L.vag_beam_step_dev_opt(x, 16, x, x, x, 10, x, x, None, 2, 3, 16, 8, x, x, 8, None) == -22
    assert L.vag_beam_step_logits_dev_opt(x, 4096, x, 1, x, x, x, 10, x, x, None, 2, 3, 4096, 8, x, x, -1, None) == -22
    P1 = (C.c_void_p * 1)(16)
    I1 = (C.c_int64 * 1)(16)
    H1 = (C.c_int64 * 1)(8)
    assert L.vag_beam_ens_step_opt(P1, I1, 1, x, x, 0, 10, P1, P1, H1, 2, 3, 16, x, x, 5, None) == -22
    assert L.vag_beam_ens_step_dev_opt(P1, I1, 1, x, x, x, 10, P1, P1, H1, None, 2, 3, 16, x, x, 16, None) == -22
    # forced scores: M out of [1, VAG_ENS_MAX], NULL arrays / entries, empty shapes
    assert L.vag_forced_score(P1, I1, P1, 0, x, 2, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, I1, P1, 9, x, 2, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(None, I1, P1, 1, x, 2, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, I1, None, 1, x, 2, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, I1, (C.c_void_p * 1)(None), 1, x, 2, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, I1, P1, 1, x, 0, 3, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, I1, P1, 1, x, 2, 0, 16, x, x, x, None) == -22
    assert L.vag_forced_score(P1, (C.c_int64 * 1)(8), P1, 1, x, 2, 3, 16, x, x, x, None) == -22     # ldl < V


def _fixture():
    z = np.load(os.path.join(GOLDEN, "beam_opts.npz"))
    return json.loads(bytes(z["meta"]).decode())


def test_option_fixture_is_discriminative():
    fx = _fixture()
    assert fx["unk"] == UNK and fx["unk_bias"] > 0
    unk_cases = [c for c in fx["cases"] if c["variant"] == "unk"]
    assert len(unk_cases) == 2
    for c in unk_cases:
        for k in (2, 3, 12):
            d = c["decode"]
            default, avoid = d["%d/10" % k], d["%d/11" % k]
            assert default != avoid, (c["fixture"], k)
            assert any(UNK in h for h in default), (c["fixture"], k)
            # avoid_unk: UNK only where the reference allows it, at step 0
            assert all(UNK not in h[1:] for h in avoid), (c["fixture"], k)
            assert all(UNK not in h[1:] for h in d["%d/01" % k]), (c["fixture"], k)
    # avoid_double=False changes some lists of every fixture, and lets a word follow itself
    for c in fx["cases"]:
        assert any(c["decode"]["%d/00" % k] != c["decode"]["%d/10" % k] for k in (2, 3, 12)), c["fixture"]
    rep = lambda h: any(a == b for a, b in zip(h, h[1:]))      # noqa: E731
    assert any(rep(h) for c in fx["cases"] for k in (2, 3, 12) for h in c["decode"]["%d/00" % k])
    assert not any(rep(h) for c in fx["cases"] for k in (2, 3, 12) for h in c["decode"]["%d/10" % k])
