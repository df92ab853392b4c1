"""CPU: the label-smoothed translation loss -- the criterion class (the executable definition every GPU test of the option
compares against), its recognition by the fused step, and the argument checks of the `_ls` entry points.

Definition (include/vag_nmt.h: vag_head_ce_seq_fwd_ls):
    nll_eps = w[y] * ( (1 - eps) * (-logp[y]) + eps * mean_j(-logp[j]) )
which with unit weights is torch's cross_entropy(label_smoothing=eps)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)


def _weight(V, dtype=torch.float64):
    w = torch.ones(V, dtype=dtype)
    w[0] = 0          # the reference's vocabulary weight: PAD contributes nothing
    return w


@pytest.mark.parametrize("V", [7, 2049])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.3])
def test_forward_is_cross_entropy_with_label_smoothing_fp64(V, eps):
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    g = torch.Generator().manual_seed(V)
    logits = 3.0 * torch.randn(33, V, dtype=torch.float64, generator=g)
    y = torch.randint(0, V, (33,), generator=g)
    crit = LabelSmoothedNLLLoss(torch.ones(V, dtype=torch.float64), label_smoothing=eps)
    got = crit(F.log_softmax(logits, -1), y)
    want = F.cross_entropy(logits, y, reduction="none", label_smoothing=eps)
    assert got.shape == (33,) and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.3])
def test_reference_weight_vector_zeroes_pad_rows_only(eps):
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    V = 2049
    g = torch.Generator().manual_seed(5)
    logp = F.log_softmax(3.0 * torch.randn(40, V, dtype=torch.float64, generator=g), -1)
    y = torch.randint(1, V, (40,), generator=g)
    y[::7] = 0
    unit = LabelSmoothedNLLLoss(torch.ones(V, dtype=torch.float64), eps)(logp, y)
    got = LabelSmoothedNLLLoss(_weight(V), eps)(logp, y)
    pad = y == 0
    assert pad.any() and (~pad).any()
    assert torch.equal(got[pad], torch.zeros_like(got[pad]))
    assert torch.equal(got[~pad], unit[~pad])
    if eps == 0.0:
        assert torch.equal(got, torch.nn.NLLLoss(weight=_weight(V), reduction="none")(logp, y))


def test_weight_is_a_tensor_attribute_and_follows_the_module():
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    crit = LabelSmoothedNLLLoss(_weight(11, torch.float32))
    assert torch.is_tensor(crit.weight) and crit.weight.shape == (11,) and crit.label_smoothing == 0.1
    assert crit.double().weight.dtype == torch.float64
    # fp32 log-probabilities, fp32 result
    out = LabelSmoothedNLLLoss(_weight(11, torch.float32), 0.2)(F.log_softmax(torch.randn(4, 11), -1), torch.tensor([0, 3, 10, 1]))
    assert out.dtype == torch.float32 and out[0].item() == 0.0 and (out[1:] > 0).all()


@pytest.mark.parametrize("eps", [-0.1, 1.0, float("nan")])
def test_constructor_rejects_smoothing_outside_the_half_open_unit_interval(eps):
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    with pytest.raises(ValueError):
        LabelSmoothedNLLLoss(_weight(7), label_smoothing=eps)


def test_constructor_rejects_missing_weight():
    from machine_translation_vision.losses import LabelSmoothedNLLLoss
    with pytest.raises(ValueError):
        LabelSmoothedNLLLoss(None)


def test_fusable_recognises_the_class_by_exact_type():
    from machine_translation_vision.losses import LabelSmoothedNLLLoss, PairwiseRankingLoss
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.fused import fusable, mt_label_smoothing

    class Sub(LabelSmoothedNLLLoss):
        pass

    mm = NMT_AttentionImagine_Seq2Seq_Beam_V11(20, 24, 16, 8, 8, 8, 8, 0.9)
    txt = NMT_Seq2Seq_Beam_V2(20, 24, 8, 8, 8)
    w = _weight(24, torch.float32)
    for model, cv in ((mm, PairwiseRankingLoss(margin=0.1)), (mm, None), (txt, None)):
        assert fusable(model, LabelSmoothedNLLLoss(w, 0.1), cv)
        assert fusable(model, LabelSmoothedNLLLoss(w, 0.0), cv)
        assert fusable(model, torch.nn.NLLLoss(weight=w, reduction="none"), cv)           # (unchanged)
        assert not fusable(model, Sub(w, 0.1), cv)
    assert mt_label_smoothing(LabelSmoothedNLLLoss(w, 0.25)) == 0.25
    assert mt_label_smoothing(torch.nn.NLLLoss(weight=w, reduction="none")) == 0.0
    assert mt_label_smoothing(Sub(w, 0.25)) is None
    assert mt_label_smoothing(torch.nn.NLLLoss(weight=w)) is None                        # (a reducing NLLLoss: generic path, as before)


def _ls_calls(L, eps):
    """The three `_ls` entry points with an argument list that would pass every other check (non-NULL, aligned, never
    dereferenced: the smoothing is validated before anything is enqueued)."""
    from vagnmt_hip import _lib
    p = 4096          # "valid-looking": non-NULL and 16-byte aligned; a call that got past the eps check would fault, not return
    hw = _lib.HeadW(p, p, p, p, p, p, p, p)
    B, Tt, E, H, V, ldl = 4, 3, 8, 8, 10, 12
    eps = C.c_float(eps)
    return [
        L.vag_head_ce_seq_fwd_ls(p, p, p, hw, p, p, B, Tt, E, H, V, 0.0, None, 0, p, p, ldl, p, p, p, p, eps, None),
        L.vag_head_ce_seq_bwd_ls(p, p, p, hw, p, p, B, Tt, E, H, V, 0.0, None, p, p, ldl, p, p, p, p, p, p, hw, p, eps, None),
        L.vag_head_ce_seq_bwd_data_ls(hw, p, p, B, Tt, E, H, V, 0.0, None, p, p, ldl, p, p, p, p, p, p, p, eps, None),
    ]


def test_ls_entry_points_are_exported_and_bound():
    from vagnmt_hip import _lib
    L = _lib.lib()
    for n in ("vag_head_ce_seq_fwd_ls", "vag_head_ce_seq_bwd_ls", "vag_head_ce_seq_bwd_data_ls"):
        assert n in _lib.PROTOS and hasattr(L, n), n
        base = _lib.PROTOS[n[:-3]][1]
        # the namesake's argument list plus `float label_smoothing` in front of the stream
        assert _lib.PROTOS[n][1] == base[:-1] + [_lib.F, _lib.P], n


@pytest.mark.parametrize("eps", [-0.1, 1.0, float("nan")])
def test_ls_entry_points_reject_bad_smoothing_without_touching_the_device(eps):
    from vagnmt_hip import _lib
    assert _ls_calls(_lib.lib(), eps) == [-22, -22, -22]


def test_ls_entry_points_reject_null_arguments_like_their_namesakes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    hw = _lib.HeadW()
    assert L.vag_head_ce_seq_fwd_ls(None, None, None, hw, None, None, 4, 3, 8, 8, 10, 0.0, None, 0, None, None, 12, None, None,
                                    None, None, 0.1, None) == -22
    assert L.vag_head_ce_seq_bwd_ls(None, None, None, hw, None, None, 4, 3, 8, 8, 10, 0.0, None, None, None, 12, None, None, None,
                                    None, None, None, hw, None, 0.1, None) == -22
    assert L.vag_head_ce_seq_bwd_data_ls(hw, None, None, 4, 3, 8, 8, 10, 0.0, None, None, None, 12, None, None, None, None, None,
                                         None, None, 0.1, None) == -22


def _cfg():
    from vagnmt_hip import _lib
    c = _lib.StepCfg()
    c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = 64, 40, 40, 256, 256, 512, 512, 2048, 9391, 9392
    c.multimodal, c.rank_kind = 1, 0
    return c


def test_step_cfg_field_is_last_and_leaves_the_workspace_alone():
    from vagnmt_hip import _lib
    L = _lib.lib()
    assert _lib.StepCfg._fields_[-1][0] == "label_smoothing" and _lib.StepCfg._fields_[-2][0] == "guard"
    c = _cfg()
    assert c.label_smoothing == 0.0          # zero-initialised callers keep the plain loss
    a = L.vag_step_ws_floats(C.byref(c))
    offs = [L.vag_step_ws_offset(C.byref(c), k) for k in range(9)]
    c.label_smoothing = 0.1
    assert a > 0 and L.vag_step_ws_floats(C.byref(c)) == a
    assert [L.vag_step_ws_offset(C.byref(c), k) for k in range(9)] == offs


@pytest.mark.parametrize("eps", [-0.1, 1.0, float("nan")])
def test_step_cfg_rejects_bad_smoothing(eps):
    from vagnmt_hip import _lib
    L = _lib.lib()
    c = _cfg()
    c.label_smoothing = eps
    assert math.isnan(eps) or c.label_smoothing == C.c_float(eps).value
    assert L.vag_step_ws_floats(C.byref(c)) == -22
    p = 4096
    assert L.vag_train_step(C.byref(c), C.byref(_lib.ModelW()), C.byref(_lib.ModelW()), p, p, p, p, p, None, None, p, p, 7,
                            None) == -22
