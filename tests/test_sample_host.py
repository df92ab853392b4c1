"""CPU: host-side checks of the sampling decoder (no device): the new symbols in the header, the binding and the library, the C
ABI's argument errors, the argument checks of sample_decode on the models and the Ensemble, and the host side of the result
(vagnmt_hip.sampling.assemble: the EOS cut, the span sums and the length normalisation) against a numpy restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

EOS = 3
NEW = ["vag_sample_step", "vag_sample_step_dev", "vag_sample_noise"]


def test_new_symbols_in_header_binding_and_library():
    from vagnmt_hip import _lib
    src = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared in include/vag_nmt.h"
        assert name in _lib.PROTOS, name + " is not in the binding table"
        assert hasattr(L, name), "libvagnmt.so does not export " + name


def test_sample_abi_argument_errors_are_negative_codes():
    from vagnmt_hip import _lib
    L = _lib.lib()
    x = C.c_void_p(16)
    P1, N1 = (C.c_void_p * 1)(16), (C.c_void_p * 1)(None)
    P9 = (C.c_void_p * 9)(*([16] * 9))
    I1, I9, H1 = (C.c_int64 * 1)(16), (C.c_int64 * 9)(*([16] * 9)), (C.c_int64 * 1)(8)

    def step(logp=P1, ldl=I1, M=1, toks=x, lps=x, di=0, ml=10, h_in=P1, h_out=P1, H=H1, B=2, n=3, V=16, T=1.0, k=0, rng=x, alive=x):
        return L.vag_sample_step(logp, ldl, M, toks, lps, di, ml, h_in, h_out, H, None, B, n, V, T, k, rng, alive, None)

    def dev(logp=P1, ldl=I1, M=1, toks=x, lps=x, di_state=x, ml=10, B=2, n=3, V=16, T=1.0, k=0, rng=x, alive=x):
        return L.vag_sample_step_dev(logp, ldl, M, toks, lps, di_state, ml, None, B, n, V, T, k, rng, alive, None)

    for f in (step, dev):
        assert f(k=65) == -22 and f(k=-1) == -22                                # top_k outside [0, 64]
        assert f(T=0.0) == -22 and f(T=-1.0) == -22 and f(T=float("nan")) == -22 and f(T=float("inf")) == -22
        assert f(logp=None) == -22 and f(ldl=None) == -22 and f(logp=N1) == -22       # NULL array / entry
        assert f(M=0) == -22 and f(logp=P9, ldl=I9, M=9) == -22                 # M outside [1, VAG_ENS_MAX]
        assert f(V=17) == -22 and f(V=0) == -22                                 # ldl < V, empty vocabulary
        assert f(toks=None) == -22 and f(lps=None) == -22 and f(rng=None) == -22 and f(alive=None) == -22
        assert f(B=0) == -22 and f(n=0) == -22 and f(ml=0) == -22
        assert f(k=10, V=1 << 24, ldl=(C.c_int64 * 1)(1 << 24)) == -22          # the radix keys hold 24 index bits
    assert step(di=10) == -22 and step(di=-1) == -22                            # di outside [0, max_len)
    assert step(h_in=None) == -22 and step(h_out=N1) == -22 and step(H=(C.c_int64 * 1)(0)) == -22       # step 0 needs the states
    assert dev(di_state=None) == -22
    assert L.vag_sample_noise(None, 0, 4, 16, x, None) == -22
    assert L.vag_sample_noise(x, 0, 4, 16, None, None) == -22
    for di, N, V in [(-1, 4, 16), (0, 0, 16), (0, 4, 0)]:
        assert L.vag_sample_noise(x, di, N, V, x, None) == -22, (di, N, V)


# ------------------------------------------------------------------------------------------------------------------
# argument checks of the public methods (CPU tensors: there is no CPU path)
# ------------------------------------------------------------------------------------------------------------------
def _v11(seed=0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(30, 40, 24, 8, 8, 16, 12, 0.99).eval()


def _v2(seed=0):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    return NMT_Seq2Seq_Beam_V2(30, 40, 8, 8, 16).eval()


def test_sample_decode_argument_checks():
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.sampling import Sampled
    assert Sampled._fields == ("hyps", "token_logp", "logp", "score")
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    m, t = _v11(), _v2()
    for obj in (m, t, Ensemble([m, t]), Ensemble([t])):
        with pytest.raises(ValueError, match="top_k"):
            obj.sample_decode(src, [5, 5], im, top_k=65)
        with pytest.raises(ValueError, match="top_k"):
            obj.sample_decode(src, [5, 5], im, top_k=-1)
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="temperature"):
                obj.sample_decode(src, [5, 5], im, temperature=bad)
        with pytest.raises(ValueError, match="n_samples"):
            obj.sample_decode(src, [5, 5], im, n_samples=0)
        with pytest.raises(ValueError, match="max_length"):
            obj.sample_decode(src, [5, 5], im, max_length=0)
        with pytest.raises(ValueError, match="GPU tensor"):                     # everything in range, but a CPU src_var
            obj.sample_decode(src, [5, 5], im, n_samples=2, temperature=0.7, top_k=64)
    # image mismatch: a multimodal member (or model) without im_var.  An Ensemble checks it where a model does, after the
    # variant's own argument checks: it must be the call's only fault, so src_var reports is_cuda here
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    with pytest.raises(ValueError, match="im_var"):
        Ensemble([t, m]).sample_decode(src.as_subclass(OnGpu), [5, 5])
    with pytest.raises(ValueError, match="im_var"):
        Ensemble([m]).sample_decode(src.as_subclass(OnGpu), [5, 5], None, n_samples=2, top_k=3)
    assert not m.training and not t.training


def test_generator_state_words():
    from vagnmt_hip.sampling import Generator
    g = Generator(1234)
    assert g.get_state() == [1234, 0]
    g.set_state([7, 9])
    assert g.get_state() == [7, 9]
    assert Generator((1 << 64) - 1).get_state() == [-1, 0]                       # seeds are uint64 words, kept as int64 bit patterns
    assert Generator(torch.initial_seed()).get_state()[1] == 0


# ------------------------------------------------------------------------------------------------------------------
# the result: EOS cut, span sums, length normalisation
# ------------------------------------------------------------------------------------------------------------------
def restate(toks, lps, B, n):
    """numpy restatement, row by row: toks / lps (L, B n) time-major."""
    L, N = toks.shape
    hyps, tl, lp, sc = [], np.zeros((N, L), np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    for r in range(N):
        row, acc, words = [], np.float32(0), 0
        for t in range(L):
            w = int(toks[t, r])
            tl[r, t] = lps[t, r]
            acc = np.float32(acc + np.float32(lps[t, r]))
            words += w > 3
            if w == EOS:
                break
            row.append(w)
        hyps.append(row)
        lp[r] = acc
        sc[r] = np.float32(acc / np.float32(max(1, words)))
    return [hyps[b * n:(b + 1) * n] for b in range(B)], tl.reshape(B, n, L), lp.reshape(B, n), sc.reshape(B, n)


def test_assemble_cut_and_length_normalisation():
    from vagnmt_hip.sampling import assemble
    #        ends at step 2      never ends          EOS first      specials only, then EOS    EOS at the last step   a pad word inside
    rows = [[5, 9, EOS, EOS, EOS], [4, 4, 7, 8, 60], [EOS] * 5, [1, 2, EOS, EOS, EOS], [6, 7, 8, 9, EOS], [5, 0, 7, EOS, EOS]]
    toks = np.array(rows, dtype=np.int64).T.copy()                              # (L, N) = (5, 6): B = 3, n = 2
    rng = np.random.RandomState(3)
    lps = -rng.rand(5, 6).astype(np.float32) * 4
    lps[toks == EOS] *= (np.cumsum(toks == EOS, 0) == 1)[toks == EOS]            # a finished row re-emits EOS at 0
    for make in (lambda a: a, torch.from_numpy):
        got = assemble(make(toks), make(lps), 3, 2)
        hyps, tl, lp, sc = restate(toks, lps, 3, 2)
        assert got.hyps == hyps == [[[5, 9], [4, 4, 7, 8, 60]], [[], [1, 2]], [[6, 7, 8, 9], [5, 0, 7]]]
        assert got.token_logp.shape == (3, 2, 5) and got.logp.shape == (3, 2) and got.score.shape == (3, 2)
        assert got.token_logp.dtype == got.logp.dtype == got.score.dtype == torch.float32
        np.testing.assert_array_equal(got.token_logp.numpy(), tl)
        np.testing.assert_array_equal(got.logp.numpy(), lp)
        np.testing.assert_array_equal(got.score.numpy(), sc)
    # words > 3 in the span: 2, 5, 0 -> 1, 0 -> 1, 4, 2 (the pad word does not count)
    np.testing.assert_array_equal(got.score.numpy(), (lp / np.array([[2, 5], [1, 1], [4, 2]], np.float32)).astype(np.float32))
    # nothing after the first EOS leaks in, even if the history held something there
    lps2 = lps.copy()
    lps2[3:, 0] = -7.0
    toks2 = toks.copy()
    toks2[3:, 0] = 11
    again = assemble(toks2, lps2, 3, 2)
    assert again.hyps[0][0] == [5, 9] and float(again.logp[0, 0]) == float(lp[0, 0])
    assert float(again.token_logp[0, 0, 3:].abs().sum()) == 0.0
