"""CPU: host-side checks of the attention alignments (no device): the new symbols in the header and the binding, the C ABI's
argument errors of the three entry points, the host helpers of vagnmt_hip.align on hand-written cases and the argument checks of
the public methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

UNK, EOS = 1, 3
NEW = ["vag_beam_attn_record", "vag_beam_attn_record_dev", "vag_beam_finish_align", "vag_forced_align"]


def test_new_symbols_in_header_binding_and_library():
    from vagnmt_hip import _lib
    src = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/vag_nmt.h"
        assert name in _lib.PROTOS, name + " is not in the binding table"
        assert hasattr(L, name), "libvagnmt.so does not export " + name


def test_align_abi_argument_errors_are_negative_codes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    x = C.c_void_p(16)
    P1 = (C.c_void_p * 1)(16)
    P9 = (C.c_void_p * 9)(*([16] * 9))
    N1 = (C.c_void_p * 1)(None)
    # record: M out of [1, VAG_ENS_MAX], NULL array / entry / history, k > 64, di outside [0, max_len), empty sizes
    assert L.vag_ens_max_models() == 8
    assert L.vag_beam_attn_record(P1, 0, x, 0, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record(P9, 9, x, 0, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record(None, 1, x, 0, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record(N1, 1, x, 0, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record(P1, 1, None, 0, 10, 2, 3, 8, None) == -22
    for di, ml, B, k, Tp in [(0, 10, 2, 65, 8), (10, 10, 2, 3, 8), (-1, 10, 2, 3, 8), (0, 0, 2, 3, 8), (0, 10, 0, 3, 8),
                             (0, 10, 2, 0, 8), (0, 10, 2, 3, 0)]:
        assert L.vag_beam_attn_record(P1, 1, x, di, ml, B, k, Tp, None) == -22, (di, ml, B, k, Tp)
    # the device-index form: no step word
    assert L.vag_beam_attn_record_dev(P1, 1, x, None, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record_dev(P1, 0, x, x, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record_dev(N1, 1, x, x, 10, 2, 3, 8, None) == -22
    assert L.vag_beam_attn_record_dev(P1, 1, x, x, 10, 2, 65, 8, None) == -22
    assert L.vag_beam_attn_record_dev(P1, 1, x, x, 10, 2, 3, 0, None) == -22
    # aligning finish: everything vag_beam_finish_nbest rejects, and NULL buffers, Ts < 1, Ts > Tp
    assert L.vag_beam_finish_align(None, None, None, 10, 5, 2, 3, 1, 8, 8, None, None, None, None, None) == -22
    for ml, steps, B, k, n in [(10, 5, 2, 3, 0), (10, 5, 2, 3, 4), (10, 5, 2, 65, 2), (10, 11, 2, 3, 1), (10, 5, 0, 3, 1)]:
        assert L.vag_beam_finish_align(x, x, x, ml, steps, B, k, n, 8, 8, x, x, x, x, None) == -22, (ml, steps, B, k, n)
    assert L.vag_beam_finish_align(x, x, None, 10, 5, 2, 3, 1, 8, 8, x, x, x, x, None) == -22
    assert L.vag_beam_finish_align(x, x, x, 10, 5, 2, 3, 1, 8, 8, x, x, None, x, None) == -22
    assert L.vag_beam_finish_align(x, x, x, 10, 5, 2, 3, 1, 8, 8, x, x, x, None, None) == -22
    assert L.vag_beam_finish_align(x, x, x, 10, 5, 2, 3, 1, 8, 0, x, x, x, x, None) == -22
    assert L.vag_beam_finish_align(x, x, x, 10, 5, 2, 3, 1, 8, 9, x, x, x, x, None) == -22
    # forced alignment: M out of range, NULL arrays / entries / outputs, empty shapes
    assert L.vag_forced_align(P1, 0, x, 2, 3, 8, x, x, None) == -22
    assert L.vag_forced_align(P9, 9, x, 2, 3, 8, x, x, None) == -22
    assert L.vag_forced_align(None, 1, x, 2, 3, 8, x, x, None) == -22
    assert L.vag_forced_align(N1, 1, x, 2, 3, 8, x, x, None) == -22
    assert L.vag_forced_align(P1, 1, None, 2, 3, 8, x, x, None) == -22
    assert L.vag_forced_align(P1, 1, x, 2, 3, 8, None, x, None) == -22
    assert L.vag_forced_align(P1, 1, x, 2, 3, 8, x, None, None) == -22
    for B, Tt, Ts in [(0, 3, 8), (2, 0, 8), (2, 3, 0)]:
        assert L.vag_forced_align(P1, 1, x, B, Tt, Ts, x, x, None) == -22, (B, Tt, Ts)


# ------------------------------------------------------------------------------------------------------------------
# host helpers
# ------------------------------------------------------------------------------------------------------------------
SRC_WORDS = [["ein", "Hund", "rennt", "schnell"], ["Zürich", "ist", "schön"]]


def test_unk_links_nbest_form():
    from vagnmt_hip.align import unk_links
    hyps = [[[5, UNK, 7], [UNK, UNK]], [[8, 9], [UNK]]]
    src_pos = torch.tensor([[[0, 1, 2, 3, -1], [3, -1, -1, -1, -1]],
                            [[1, 2, 0, -1, -1], [0, 2, -1, -1, -1]]])
    assert unk_links(hyps, src_pos) == [[[(1, 1)], [(0, 3)]], [[], [(0, 0)]]]       # src_pos -1 ignored; no UNK: no links
    assert unk_links(hyps, src_pos.numpy()) == unk_links(hyps, src_pos) == unk_links(hyps, src_pos.tolist())
    assert unk_links(hyps, src_pos, unk=9) == [[[], []], [[(1, 2)], []]]


def test_unk_links_one_list_per_sentence():
    from vagnmt_hip.align import unk_links
    hyps = [[5, UNK, 7], [UNK]]
    src_pos = np.array([[0, 2, 1, -1], [-1, -1, -1, -1]])
    assert unk_links(hyps, src_pos) == [[(1, 2)], []]
    assert unk_links([[4, 5], [6]], src_pos) == [[], []]


def test_replace_unk():
    from vagnmt_hip.align import replace_unk
    hyps = [[[5, UNK, 7], [UNK, UNK]], [[8, 9], [UNK]]]
    words = [[["a", "<unk>", "runs"], ["<unk>", "<unk>"]], [["it", "is"], ["<unk>"]]]
    src_pos = torch.tensor([[[0, 1, 2, 3, -1], [3, -1, -1, -1, -1]],
                            [[1, 2, 0, -1, -1], [0, 2, -1, -1, -1]]])
    # no lexicon: the source word itself (a name); the UNK at src_pos -1 keeps its word
    assert replace_unk(words, hyps, src_pos, SRC_WORDS) == [[["a", "Hund", "runs"], ["schnell", "<unk>"]],
                                                           [["it", "is"], ["Zürich"]]]
    # a lexicon entry translates, a missing entry copies
    lex = {"Hund": "dog", "schnell": "fast"}
    got = replace_unk(words, hyps, src_pos, SRC_WORDS, lexicon=lex)
    assert got == [[["a", "dog", "runs"], ["fast", "<unk>"]], [["it", "is"], ["Zürich"]]]
    assert words[0][0] == ["a", "<unk>", "runs"]                                    # the input lists are not modified
    # no UNK present: the lists come back as they are
    assert replace_unk([["x", "y"]], [[4, 5]], [[0, 1]], [["p", "q"]]) == [["x", "y"]]
    # the flat form; a position outside the source sentence keeps the word
    assert replace_unk([["<unk>", "b"], ["<unk>"]], [[UNK, 5], [UNK]], [[1, 0], [7]], [["p", "q"], ["r"]],
                       lexicon={"q": "Q"}) == [["Q", "b"], ["<unk>"]]


# ------------------------------------------------------------------------------------------------------------------
# argument checks of the public methods (CPU tensors: there is no CPU path)
# ------------------------------------------------------------------------------------------------------------------
def _v11(Vs=30, Vt=40, H=16, seed=0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, 24, 8, 8, H, 12, 0.99).eval()


def _v2(Vs=30, Vt=40, H=16, seed=0):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    return NMT_Seq2Seq_Beam_V2(Vs, Vt, 8, 8, H).eval()


def test_align_argument_checks():
    from vagnmt_hip.align import Aligned, Alignment
    from vagnmt_hip.ensemble import Ensemble
    assert Aligned._fields == ("hyps", "scores", "attention", "src_pos") and Alignment._fields == ("attention", "src_pos")
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    m, t = _v11(), _v2()
    for k, n in [(3, 0), (3, 4), (65, 2), (65, 65), (0, 0)]:                 # n_best > beam_size among them
        with pytest.raises(ValueError):
            m.beamsearch_align(src, [5, 5], im, k, n, 4)
        with pytest.raises(ValueError):
            t.beamsearch_align(src, [5, 5], k, n, 4)
        with pytest.raises(ValueError):
            Ensemble([m, t]).beamsearch_align(src, [5, 5], im, k, n, 4)
    # in range, but a CPU src_var
    with pytest.raises(ValueError):
        m.beamsearch_align(src, [5, 5], im, 3, 2, 4)
    with pytest.raises(ValueError):
        t.beamsearch_align(src, [5, 5], 64, 64, 4)
    with pytest.raises(ValueError):
        Ensemble([t]).beamsearch_align(src, [5, 5], None, 1, 1, 4)
    with pytest.raises(ValueError):
        m.align_translations(src, [5, 5], [[4, 5], [6]], im)
    with pytest.raises(ValueError):
        t.align_translations(src, [5, 5], [[4, 5], [6]])
    with pytest.raises(ValueError):
        Ensemble([m, t]).align_translations(src, [5, 5], [[4, 5], [6]], im)
    assert not m.training and not t.training
