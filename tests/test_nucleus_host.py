"""CPU: host-side checks of nucleus (top-p) sampling (no device): the two new symbols in the header, the binding and the
library, the C ABI's argument errors for top_p, check_top_p, and the argument checks of sample_decode(top_p=...) on the models
and the Ensemble."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ["vag_sample_step_p", "vag_sample_step_p_dev"]


def test_new_symbols_in_header_binding_and_library():
    from vagnmt_hip import _lib
    src = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/vag_nmt.h"
        assert name in _lib.PROTOS, name + " is not in the binding table"
        assert hasattr(L, name), "libvagnmt.so does not export " + name
    # the plain entry points keep their signatures; the new ones append (top_p, set_size) before the stream
    P = _lib.PROTOS
    for old, new in (("vag_sample_step", "vag_sample_step_p"), ("vag_sample_step_dev", "vag_sample_step_p_dev")):
        assert P[new][0] is P[old][0]
        assert P[new][1] == P[old][1][:-1] + [C.c_float, C.c_void_p] + P[old][1][-1:]
    assert len(P["vag_sample_step"][1]) == 19 and len(P["vag_sample_step_dev"][1]) == 16


def test_nucleus_abi_argument_errors_are_negative_codes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    x = C.c_void_p(16)
    P1, N1 = (C.c_void_p * 1)(16), (C.c_void_p * 1)(None)
    I1, H1 = (C.c_int64 * 1)(16), (C.c_int64 * 1)(8)

    def step(logp=P1, ldl=I1, M=1, toks=x, lps=x, di=0, ml=10, h_in=P1, h_out=P1, H=H1, B=2, n=3, V=16, T=1.0, k=0, rng=x, alive=x,
             p=0.9, size=x):
        return L.vag_sample_step_p(logp, ldl, M, toks, lps, di, ml, h_in, h_out, H, None, B, n, V, T, k, rng, alive, p, size, None)

    def dev(logp=P1, ldl=I1, M=1, toks=x, lps=x, di_state=x, ml=10, B=2, n=3, V=16, T=1.0, k=0, rng=x, alive=x, p=0.9, size=x):
        return L.vag_sample_step_p_dev(logp, ldl, M, toks, lps, di_state, ml, None, B, n, V, T, k, rng, alive, p, size, None)

    for f in (step, dev):
        # top_p outside (0, 1] or NaN: rejected before anything touches a device, with or without a size buffer
        for bad in (0.0, -0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            assert f(p=bad) == -22, bad
            assert f(p=bad, size=None) == -22, bad
        # everything vag_sample_step rejects, with a good top_p
        assert f(logp=None) == -22 and f(ldl=None) == -22 and f(logp=N1) == -22
        assert f(toks=None) == -22 and f(lps=None) == -22 and f(rng=None) == -22 and f(alive=None) == -22
        assert f(k=65) == -22 and f(k=-1) == -22 and f(T=0.0) == -22 and f(T=float("nan")) == -22
        assert f(V=17) == -22 and f(V=0) == -22 and f(B=0) == -22 and f(n=0) == -22 and f(ml=0) == -22
        assert f(M=0) == -22
        assert f(k=10, V=1 << 24, ldl=(C.c_int64 * 1)(1 << 24)) == -22
    assert step(di=10) == -22 and step(di=-1) == -22 and step(h_in=None) == -22 and step(h_out=N1) == -22
    assert dev(di_state=None) == -22
    # NULL everything
    assert L.vag_sample_step_p(None, None, 1, None, None, 0, 10, None, None, None, None, 2, 3, 16, 1.0, 0, None, None, 0.9, None,
                               None) == -22
    assert L.vag_sample_step_p_dev(None, None, 1, None, None, None, 10, None, 2, 3, 16, 1.0, 0, None, None, 0.9, None, None) == -22


def test_check_top_p():
    from vagnmt_hip import sampling
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="top_p"):
            sampling.check_top_p(bad)
    assert sampling.check_top_p(1e-6) == 1e-6 and sampling.check_top_p(1.0) == 1.0 and sampling.check_top_p(1) == 1.0
    assert isinstance(sampling.check_top_p(1), float)
    # check_args keeps its signature and its result
    import inspect
    assert list(inspect.signature(sampling.check_args).parameters) == ["src_var", "n_samples", "max_length", "temperature", "top_k",
                                                                       "what"]
    # top_p = 1 without sizes is the plain decode: nothing is added to the key of its decode state
    assert sampling.nucleus_key(1.0, False) == ()
    assert sampling.nucleus_key(0.9, False) == (0.9, False) and sampling.nucleus_key(1.0, True) == (1.0, True)


def _models():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(0)
    return (NMT_AttentionImagine_Seq2Seq_Beam_V11(30, 40, 24, 8, 8, 16, 12, 0.99).eval(), NMT_Seq2Seq_Beam_V2(30, 40, 8, 8, 16).eval())


def test_sample_decode_top_p_argument_checks():
    from vagnmt_hip.ensemble import Ensemble
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    m, t = _models()
    for obj in (m, t, Ensemble([m, t]), Ensemble([t])):
        for bad in (0.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="top_p"):
                obj.sample_decode(src, [5, 5], im, top_p=bad)
        with pytest.raises(ValueError, match="top_k"):
            obj.sample_decode(src, [5, 5], im, top_p=0.9, top_k=65)
        for kw in (dict(top_p=0.9), dict(top_p=1.0, return_sizes=True), dict(top_p=0.5, top_k=10, temperature=0.7, return_sizes=True)):
            with pytest.raises(ValueError, match="GPU tensor"):                 # everything in range, but a CPU src_var
                obj.sample_decode(src, [5, 5], im, n_samples=2, **kw)
    # an Ensemble checks im_var where a model does, after the variant's own argument checks: the missing im_var must be the
    # call's only fault, so src_var reports is_cuda here
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    with pytest.raises(ValueError, match="im_var"):
        Ensemble([t, m]).sample_decode(src.as_subclass(OnGpu), [5, 5], top_p=0.9)
    with pytest.raises(ValueError, match="im_var"):
        Ensemble([m]).sample_decode(src.as_subclass(OnGpu), [5, 5], None, top_p=0.9)
