"""CPU: the reference of word-level confidence (tests/confidence_ref.py) is honest and sensitive, vag_token_conf rejects what its
contract says it rejects (host checks of the cross-compiled library: nothing is launched), the Python functions refuse CPU tensors,
and `calibration` against a case computed by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import confidence_ref as R
from conftest import ROOT

CASES = [(V, None) for V in R.VS] + [(67, 68 + 1)]          # ldl = ceil4(V), and one odd leading dimension (the unaligned path)


def _worst(got, ref):
    """max over span positions of |entropy - reference| / bound"""
    k = ref["keep"]
    return float((np.abs(got["entropy"].astype(np.float64) - ref["entropy"])[k] / ref["bound"][k]).max())


@pytest.mark.parametrize("V,ldl", CASES)
def test_fp32_restatement_is_inside_the_bound_and_every_defect_leaves_it(V, ldl):
    x, lse, tgt = R.tied_case(V, ldl)
    ref = R.reference(x, lse, tgt, V)
    good = R.restate_fp32(x, lse, tgt, V)
    k = ref["keep"]
    assert k.sum() == 3 + 3 + 0 + 1 + 6 and not k[0, 3:].any() and not k[1, 1] and k[1, 3]
    assert (ref["bound"][k] > 0).all() and (ref["bound"][k] <= 1e-5 * np.maximum(1.0, ref["entropy"][k])).all()
    print("[conf host] V=%d ldl=%s: fp32 restatement, worst |dH| / bound %.3f" % (V, ldl, _worst(good, ref)))
    assert _worst(good, ref) <= 1.0
    for name in ("rank", "top", "keep"):
        assert np.array_equal(good[name], ref[name]), name
    assert np.array_equal(good["token_logp"].astype(np.float64), ref["token_logp"])
    assert np.array_equal(good["top_logp"].astype(np.float64), ref["top_logp"])
    # the special rows are what they say
    b, t = R.UNIFORM
    assert abs(good["entropy"][b, t] - np.log(V)) <= ref["bound"][b, t] + R.uniform_slack(V) and ref["rank"][b, t] == tgt[b, t] == 2
    for b, t in (R.PEAKED, R.NEG_INF):
        assert k[b, t] and np.isfinite(good["entropy"][b, t]) and np.isfinite(ref["entropy"][b, t])
    assert ref["top"][R.PEAKED][0] == V // 2 and not np.isfinite(ref["s"][R.NEG_INF[1] * R.B + R.NEG_INF[0], 1])
    # the sentence values of the restatement against the float64 ones from its own per-position values
    want = R.sentence_values(tgt, good["token_logp"], good["entropy"], good["rank"])
    sb = R.sentence_bounds(tgt, good["token_logp"], good["entropy"])
    assert (np.abs(good["sent"].astype(np.float64) - want) <= sb + R.U24 * np.abs(want)).all()
    assert want[2].tolist() == [0.0] * R.SENT and want[:, 2].tolist() == [3, 3, 0, 1, 6]
    # the catalogue: each defect exceeds the entropy's bound, breaks an integer, or leaves the standard deviation's bound
    for defect in ("bits", "padding"):
        bad = R.restate_fp32(x, lse, tgt, V, defect=defect)
        assert _worst(bad, ref) > 10.0, defect
    bad = R.restate_fp32(x, lse, tgt, V, defect="ties_after")
    assert not np.array_equal(bad["rank"], ref["rank"])
    bad = R.restate_fp32(x, lse, tgt, V, defect="past_eos")
    assert bad["rank"][0, 3] >= 0 and ref["rank"][0, 3] == -1 and bad["sent"][0, 2] == 5
    bad = R.restate_fp32(x, lse, tgt, V, defect="ddof")
    assert (np.abs(bad["sent"][:, 3].astype(np.float64) - want[:, 3]) > 10 * sb[:, 3])[[0, 1, 4]].all()


@pytest.mark.parametrize("M", [3, 8])
def test_ensemble_reference_bound_covers_a_perturbed_score(M):
    """M > 1: scores moved by delta_s in the worst direction for every word stay inside the bound (the propagated term is honest),
    and M identical members give the single model's float64 values."""
    V = 67
    x, lse, tgt = R.random_case(V, M)
    ref = R.reference(x, lse, tgt, V)
    k = ref["keep"]
    for sign in (1.0, -1.0):
        s = ref["s"] + sign * 0.5 * R.delta_s(ref["s"]) * np.sign(ref["s"] + 1.0)
        for b, t in zip(*np.nonzero(k)):
            h = -R.entropy_terms(s[t * R.B + b])[0].sum()
            assert abs(h - ref["entropy"][b, t]) <= ref["bound"][b, t]
    xs, ls, _ = R.random_case(V, M, same=True)
    one = R.reference(xs[:1], ls[:1], tgt, V)
    same = R.reference(xs, ls, tgt, V)
    assert np.array_equal(one["rank"], same["rank"]) and np.array_equal(one["top"], same["top"])
    assert np.abs(one["entropy"] - same["entropy"]).max() <= 1e-6


# ---- the library's host checks -----------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it():
    from vagnmt_hip import _lib
    src = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    assert re.search(r"#define\s+VAG_CONF_SENT\s+8\b", src)
    assert re.search(r"\bint\s+vag_token_conf\s*\(", src)
    assert "vag_token_conf" in _lib.PROTOS and len(_lib.PROTOS["vag_token_conf"][1]) == 15
    assert hasattr(_lib.lib(), "vag_token_conf")
    from vagnmt_hip import confidence
    assert confidence.SENT == 8 and len(confidence.SENT_FIELDS) == 8


def test_token_conf_rejects_bad_arguments_without_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    p = 0x1000                                                  # never dereferenced: every call below fails its host checks

    def rc(fn="vag_token_conf", M=1, V=100, B=5, Tt=6, ldl=100, logits=p, lse=p, arrays=(True, True, True), tgt=p, outs=(p,) * 6):
        n = max(1, min(M, 8))
        a = (C.c_void_p * n)(*[logits] * n) if arrays[0] else None
        d = (C.c_int64 * n)(*[ldl] * n) if arrays[1] else None
        s = (C.c_void_p * n)(*[lse] * n) if arrays[2] else None
        return getattr(L, fn)(a, d, s, M, tgt, B, Tt, V, *outs, None)
    # everything vag_forced_score rejects (asked of both)
    for kw in (dict(M=0), dict(M=9), dict(ldl=99), dict(logits=None), dict(lse=None), dict(arrays=(False, True, True)),
               dict(arrays=(True, False, True)), dict(arrays=(True, True, False)), dict(tgt=None), dict(B=0), dict(Tt=0),
               dict(V=0), dict(B=1 << 31), dict(Tt=1 << 31)):
        assert rc("vag_forced_score", outs=(p,) * 3, **kw) == -22, kw
        assert rc(**kw) == -22, kw
    # and its own: V < 2, V >= 2^24, more rows than a grid holds, any NULL output
    for kw in (dict(V=1, ldl=4), dict(V=1 << 24, ldl=1 << 24), dict(B=1 << 16, Tt=1 << 15)):
        assert rc(**kw) == -22, kw
    for i in range(6):
        assert rc(outs=tuple(None if j == i else p for j in range(6))) == -22, i


def test_python_functions_refuse_cpu_tensors():
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    from vagnmt_hip import confidence
    from vagnmt_hip.ensemble import Ensemble
    m = NMT_Seq2Seq_Beam_V2(20, 30, 8, 8, 16)
    src = torch.randint(4, 20, (2, 3))
    tgt = torch.tensor([[5, 6, 3], [7, 3, 0]])
    for f in (lambda: m.token_confidence(src, [3, 3], tgt),
              lambda: Ensemble([m]).token_confidence(src, [3, 3], tgt),
              lambda: confidence.mc_dropout_confidence(m, src, [3, 3], tgt, passes=2),
              lambda: confidence.corpus_perplexity(m, [(src, [3, 3], tgt)])):
        with pytest.raises(ValueError, match="GPU tensor"):
            f()
    with pytest.raises(ValueError, match="GPU tensor"):
        confidence.translation_confidence(m, src, [3, 3], None, beam_size=2)
    with pytest.raises(ValueError):
        confidence.mc_dropout_confidence(m, src, [3, 3], tgt, passes=0)
    with pytest.raises(ValueError):
        confidence.corpus_perplexity(m, [])


def test_calibration_by_hand():
    from vagnmt_hip.confidence import Confidence, calibration
    # five span positions and one outside; first-choice probabilities 0.95, 0.85, 0.35, 0.35, 0.05; the given word is the first choice
    # at the 1st, 3rd and 5th.  Two bins: [0, 0.5) holds 0.35, 0.35, 0.05 (confidence 0.75 / 3, accuracy 2 / 3), [0.5, 1] holds 0.95, 0.85
    # (confidence 0.9, accuracy 1 / 2): ece = 3/5 |2/3 - 0.75/3| + 2/5 |1/2 - 0.9|
    p = torch.tensor([[0.95, 0.85, 0.35], [0.35, 0.05, 1.0]], dtype=torch.float64)
    top_logp = torch.stack([p.log(), (p / 2).log()], -1).float()
    rank = torch.tensor([[0, 3, 0], [1, 0, -1]], dtype=torch.int32)
    conf = Confidence(None, None, None, None, rank, None, top_logp, None)
    ece, bc, ba, n = calibration(conf, bins=2)
    assert n.tolist() == [3.0, 2.0]
    assert torch.allclose(bc, torch.tensor([0.75 / 3, 0.9], dtype=torch.float64), atol=1e-7)
    assert torch.allclose(ba, torch.tensor([2 / 3, 0.5], dtype=torch.float64), atol=1e-12)
    assert abs(float(ece) - (0.6 * abs(2 / 3 - 0.75 / 3) + 0.4 * abs(0.5 - 0.9))) <= 1e-7
    # ten bins: an empty bin reports 0
    ece10, bc10, ba10, n10 = calibration(conf, bins=10)
    assert n10.tolist() == [1, 0, 0, 2, 0, 0, 0, 0, 1, 1] and float(bc10[1]) == 0.0 and float(ba10[1]) == 0.0
    with pytest.raises(ValueError):
        calibration(conf, bins=0)
