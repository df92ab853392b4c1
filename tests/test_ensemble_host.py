"""CPU: the ensemble decoder's host-side validation (no device, no library compute) and the argument checks of its C ABI."""
import ctypes as C

import pytest
import torch


def _v11(Vs=30, Vt=40, H=16, seed=0, attn="dot"):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, 24, 8, 8, H, 12, 0.99, attn_model=attn).eval()


def _v2(Vs=30, Vt=40, H=16, seed=0):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    return NMT_Seq2Seq_Beam_V2(Vs, Vt, 8, 8, H).eval()


def test_constructor_rejects_bad_member_lists():
    from vagnmt_hip.ensemble import Ensemble, MAX_MODELS
    m = _v11()
    with pytest.raises(ValueError):
        Ensemble([])
    with pytest.raises(ValueError):
        Ensemble([m] * (MAX_MODELS + 1))
    with pytest.raises(ValueError):
        Ensemble([m, _v11(Vt=41)])                   # target vocabularies differ
    with pytest.raises(ValueError):
        Ensemble([m, _v2(Vs=31)])                    # source vocabularies differ
    with pytest.raises(ValueError):
        Ensemble([m, _v11(seed=1).to("meta")])       # members on different devices
    with pytest.raises(ValueError):
        Ensemble([m, torch.nn.Linear(3, 3)])         # not a model of this package


def test_constructor_accepts_mixed_members():
    from vagnmt_hip.ensemble import Ensemble, MAX_MODELS
    ens = Ensemble([_v11(H=16), _v11(H=24, seed=1, attn="mlp"), _v2(H=8)])
    assert len(ens) == 3 and ens.multimodal == [True, True, False]
    assert len(Ensemble([_v2()] * MAX_MODELS)) == MAX_MODELS


def test_multimodal_member_needs_im_var():
    from vagnmt_hip.ensemble import Ensemble
    src = torch.randint(4, 30, (2, 5))
    with pytest.raises(ValueError):
        Ensemble([_v11(), _v2()]).beamsearch_decode(src, [5, 5], None, beam_size=3, max_length=4)
    with pytest.raises(ValueError):
        Ensemble([_v11()]).beamsearch_decode(src, [5, 5], beam_size=1, max_length=4)


def test_max_models_matches_library():
    from vagnmt_hip import _lib
    from vagnmt_hip.ensemble import MAX_MODELS
    assert _lib.lib().vag_ens_max_models() == MAX_MODELS


def test_ensemble_abi_argument_errors_are_negative_codes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    fake = 0x1000                          # never dereferenced on the device: every call below fails its argument check first
    P = lambda n: (C.c_void_p * max(n, 1))(*([fake] * max(n, 1)))      # noqa: E731
    I = lambda n, v: (C.c_int64 * max(n, 1))(*([v] * max(n, 1)))       # noqa: E731
    B, k, V, H, ML = 16, 12, 9391, 512, 80
    dev = dict(nll=fake, beam=fake, n_alive=fake, scratch=fake)

    def step(lp, ld, M, hin, hout, hs, **kw):
        a = dict(dev, **kw)
        return L.vag_beam_ens_step(lp, ld, M, a["nll"], a["beam"], 1, ML, hin, hout, hs, B, k, V, a["n_alive"], a["scratch"],
                                   None)

    def step_dev(lp, ld, M, hin, hout, hs, di_state=fake):
        return L.vag_beam_ens_step_dev(lp, ld, M, fake, fake, di_state, ML, hin, hout, hs, None, B, k, V, fake, fake, None)

    for M in (2, 3):
        ok = (P(M), I(M, 9392), M, P(M), P(M), I(M, H))
        # NULL pointer lists
        assert step(None, *ok[1:]) == -22
        assert step(ok[0], None, *ok[2:]) == -22
        assert step(*ok[:3], None, *ok[4:]) == -22
        assert step(*ok[:4], None, ok[5]) == -22
        assert step(*ok[:5], None) == -22
        assert step_dev(None, *ok[1:]) == -22
        assert step_dev(*ok, di_state=None) == -22
        # a NULL entry inside a list, a short leading dimension, a bad hidden size
        lp = P(M)
        lp[M - 1] = None
        assert step(lp, *ok[1:]) == -22
        assert step(ok[0], I(M, V - 1), *ok[2:]) == -22
        assert step(*ok[:5], I(M, 0)) == -22
        # NULL search buffers, k V >= 2^24
        assert step(*ok, nll=None) == -22 and step(*ok, scratch=None) == -22
        assert L.vag_beam_ens_step(ok[0], I(M, 300000), M, fake, fake, 1, ML, *ok[3:], B, 64, 300000, fake, fake, None) == -22
        assert L.vag_ens_argmax(None, I(M, 9392), M, 16, V, fake, None) == -22
        assert L.vag_ens_argmax(P(M), None, M, 16, V, fake, None) == -22
        assert L.vag_ens_argmax(P(M), I(M, 9392), M, 16, V, None, None) == -22
    # M < 1 and M > VAG_ENS_MAX
    mx = L.vag_ens_max_models()
    for M in (0, -1, mx + 1):
        n = max(M, 1)
        assert step(P(n), I(n, 9392), M, P(n), P(n), I(n, H)) == -22
        assert step_dev(P(n), I(n, 9392), M, P(n), P(n), I(n, H)) == -22
        assert L.vag_ens_argmax(P(n), I(n, 9392), M, 16, V, fake, None) == -22
