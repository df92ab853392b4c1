"""CPU: word-level distillation (vagnmt_hip.distill; vag_kd_targets, vag_kd_head_ce_seq_fwd / _bwd, vag_train_step_kd / vag_kd_cfg): the
float64 reference of tests/distill_ref.py against its own invariants, the ABI's new names (header, binding table, vag_step_cfg and
its ctypes mirror, the library's exports and its -EINVAL answers before anything touches a device) and the argument errors of
distill_step / teacher_targets."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import distill_ref as R
from conftest import ROOT


def _row(seed, V=37, K=5):
    g = np.random.default_rng(seed)
    x = g.normal(size=V) * 2.0
    y = int(g.integers(1, V))
    idx, q = R.synth_targets(g, np.full(6, y), V, K)
    q = q.astype(np.float64)
    return x, y, idx, q / q.sum(1, keepdims=True)              # (synth_targets rounds to float32: normalised again in float64)


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def test_reference_gradient_rows_sum_to_zero_and_match_central_differences():
    for seed, lam in ((1, 0.5), (2, 1.0), (3, 0.25)):
        x, y, idx, q = _row(seed)
        for r in range(6):                                     # rows with y among the words (0, 3) and without
            assert (y in idx[r]) == (r % 3 == 0)
            g = R.dlogits_row(x, y, 0.7, idx[r], q[r], lam)
            assert abs(g.sum()) < 1e-14
            h = 1e-6
            for j in (y, int(idx[r][0]), int(idx[r][-1]), 0):
                up, dn = x.copy(), x.copy()
                up[j] += h
                dn[j] -= h
                num = 0.7 * (R.nll_row(up, y, 1.0, idx[r], q[r], lam) - R.nll_row(dn, y, 1.0, idx[r], q[r], lam)) / (2 * h)
                assert num == pytest.approx(g[j], abs=1e-8), (seed, r, j)


def test_reference_lambda_to_zero_is_the_plain_gradient_and_k1_idx_y_is_plain_for_any_lambda():
    x, y, idx, q = _row(4)
    p = np.exp(x - x.max())
    plain = p / p.sum()
    plain[y] -= 1.0
    lse = x.max() + np.log(np.exp(x - x.max()).sum())
    for r in range(6):
        assert np.abs(R.dlogits_row(x, y, 1.0, idx[r], q[r], 1e-12) - plain).max() < 1e-11
        assert R.nll_row(x, y, 1.0, idx[r], q[r], 1e-12) == pytest.approx(lse - x[y], abs=1e-10)
    for lam in (0.1, 0.7, 1.0):
        assert np.abs(R.dlogits_row(x, y, 1.0, [y], [1.0], lam) - plain).max() < 1e-15
        assert R.nll_row(x, y, 1.0, [y], [1.0], lam) == pytest.approx(lse - x[y], abs=1e-14)
    assert R.nll_row(x, y, 0.0, idx[0], q[0], 0.5) == 0.0       # a PAD row (weight 0): exactly nothing


def test_reference_targets_order_and_normalisation():
    g = np.random.default_rng(5)
    x = np.round(g.normal(size=(4, 50)) * 2) / 2                # quantised: many exact ties
    lse = np.log(np.exp(x).sum(1))
    s = R.scores([x], [lse], fp32=True)
    assert s.dtype == np.float32
    for K, T in ((1, 1.0), (8, 2.0), (50, 1.0)):
        idx, q = R.targets(s, K, T)
        assert idx.shape == (4, K) and np.abs(q.sum(1) - 1).max() < 1e-14
        for r in range(4):
            v = s[r][idx[r]]
            assert all(v[i] > v[i + 1] or (v[i] == v[i + 1] and idx[r][i] < idx[r][i + 1]) for i in range(K - 1))
            rest = np.setdiff1d(np.arange(50), idx[r])
            assert rest.size == 0 or s[r][rest].max() <= v[-1]
        if K == 50:
            assert np.abs(q - np.exp(np.take_along_axis(s.astype(np.float64), idx.astype(np.int64), 1))).max() < 1e-6    # T = 1: the softmax
    # three identical members are the single model
    s3 = R.scores([x, x, x], [lse, lse, lse])
    assert np.abs(s3 - R.scores([x], [lse])).max() < 1e-14


# ------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_the_kd_struct_are_declared_and_mirrored():
    from vagnmt_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("vag_kd_targets", "vag_kd_head_ce_seq_fwd", "vag_kd_head_ce_seq_bwd", "vag_step_kd_check", "vag_train_step_kd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.PROTOS
        assert hasattr(_lib.lib(), name)
    # the head's entry points: the _ls argument lists with (int64 K, float lambda, idx, q) in place of the smoothing
    for d in ("fwd", "bwd"):
        ls = _lib.PROTOS["vag_head_ce_seq_%s_ls" % d][1]
        assert _lib.PROTOS["vag_kd_head_ce_seq_%s" % d][1] == ls[:-2] + [_lib.I64, _lib.F, _lib.P, _lib.P, _lib.P]
    # the step's: vag_train_step's list with the targets' struct behind the configuration
    ts = _lib.PROTOS["vag_train_step"][1]
    assert _lib.PROTOS["vag_train_step_kd"][1] == ts[:1] + [C.POINTER(_lib.KdCfg)] + ts[1:]
    assert _lib.PROTOS["vag_step_kd_check"][1] == [_lib.StepCfgArg, C.POINTER(_lib.KdCfg)]
    # vag_step_cfg is as it was (the targets travel beside it); vag_kd_cfg and its mirror
    body = re.search(r"typedef struct \{([^}]*)\}\s*vag_step_cfg;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip().endswith("const float *mrt_cost, *mrt_valid;") and C.sizeof(_lib.StepCfgMrt) == 176
    kd = re.search(r"typedef struct \{([^}]*)\}\s*vag_kd_cfg;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", kd).strip() == "int32_t k; float lambda; const int32_t* idx; const float* q;"
    assert _lib.KdCfg._fields_ == [("k", C.c_int), ("lambda_", C.c_float), ("idx", C.c_void_p), ("q", C.c_void_p)]
    assert (_lib.KdCfg.k.offset, _lib.KdCfg.lambda_.offset, _lib.KdCfg.idx.offset, _lib.KdCfg.q.offset, C.sizeof(_lib.KdCfg)) == \
        (0, 4, 8, 16, 24)                                                               # the C layout of include/vag_nmt.h
    assert "Kim & Rush" in hdr
    for f in ("Makefile", "asan.mk"):
        assert "distill.hip" in open(os.path.join(ROOT, "vag-nmt_amd", "csrc", f)).read(), f


def test_kd_targets_answers_einval_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    x = C.c_void_p(16)                                         # a non-NULL address nothing may follow
    P1, I1 = (C.c_void_p * 1)(16), (C.c_int64 * 1)(1000)

    def rc(logits=P1, ldl=I1, lse=P1, M=1, R=48, V=1000, K=8, T=1.0, idx=x, q=x):
        return L.vag_kd_targets(logits, ldl, lse, M, R, V, K, T, idx, q, None)
    for K in (0, -1, 65):
        assert rc(K=K) == -22, K
    assert rc(V=7, K=8, ldl=(C.c_int64 * 1)(8)) == -22         # K > V
    assert rc(V=1 << 24, ldl=(C.c_int64 * 1)(1 << 24)) == -22
    for M in (0, 9, -1):
        assert rc(M=M) == -22, M
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert rc(T=T) == -22, T
    assert rc(logits=None) == -22 and rc(ldl=None) == -22 and rc(lse=None) == -22
    assert rc(logits=(C.c_void_p * 1)(None)) == -22 and rc(lse=(C.c_void_p * 1)(None)) == -22
    assert rc(ldl=(C.c_int64 * 1)(999)) == -22                 # ldl < V
    assert rc(idx=None) == -22 and rc(q=None) == -22
    assert rc(R=-1) == -22
    # every cause with NULL buffers as well
    assert L.vag_kd_targets(None, None, None, 1, 48, 1000, 8, 1.0, None, None, None) == -22


def _head_calls(L, _lib, K=8, lam=0.5, idx=16, q=16, logits_ready=0, V=1000, null=False):
    x = None if null else C.c_void_p(16)
    hw = _lib.HeadW() if null else _lib.HeadW(*([16] * 8))
    ldl = (V + 3) // 4 * 4
    ix = None if null else (C.c_void_p(idx) if idx else None)
    qq = None if null else (C.c_void_p(q) if q else None)
    f = L.vag_kd_head_ce_seq_fwd(x, x, x, hw, x, x, 4, 3, 8, 8, V, 0.0, None, logits_ready, x, x, ldl, x, x, x, x, K, lam, ix, qq, None)
    b = L.vag_kd_head_ce_seq_bwd(x, x, x, hw, x, x, 4, 3, 8, 8, V, 0.0, None, x, x, ldl, x, x, x, x, x, x, hw, x, K, lam, ix, qq, None)
    return f, b


def test_kd_head_entry_points_answer_einval_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    for K in (0, -3, 65):
        assert _head_calls(L, _lib, K=K) == (-22, -22), K
    assert _head_calls(L, _lib, K=8, V=4) == (-22, -22)        # K > V
    for lam in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert _head_calls(L, _lib, lam=lam) == (-22, -22), lam
    assert _head_calls(L, _lib, idx=None) == (-22, -22) and _head_calls(L, _lib, q=None) == (-22, -22)
    assert _head_calls(L, _lib, logits_ready=1)[0] == -22
    assert _head_calls(L, _lib, null=True) == (-22, -22)       # what the namesakes refuse
    # the 2-byte storage mode of the calling thread
    try:
        assert L.vag_set_operator_context(C.c_void_p(16), 1) == 0
        assert _head_calls(L, _lib) == (-22, -22)
    finally:
        assert L.vag_set_operator_context(None, 0) == 0


def _cfg():
    from vagnmt_hip import _lib
    c = _lib.StepCfgMrt()
    c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = 8, 9, 7, 32, 32, 64, 32, 48, 61, 64
    c.multimodal, c.rank_kind = 1, 0
    return c


def test_step_combinations_are_refused_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    assert L.vag_step_ws_floats(_cfg().ref()) > 0              # (the workspace is the plain step's: there is no other query)

    def refused(kd=(8, 0.5, 16, 16), **kw):
        d = _cfg()
        for k, v in kw.items():
            setattr(d, k, v)
        k = None if kd is None else C.byref(_lib.KdCfg(*kd))
        p = 4096
        a = L.vag_step_kd_check(d.ref(), k)
        assert a in (0, -22)
        if a == -22:                                           # ... and the step itself says the same, whatever the rest
            assert L.vag_train_step_kd(d.ref(), k, C.byref(_lib.ModelW()), C.byref(_lib.ModelW()), p, p, p, p, p, None, None, p, p,
                                       7, None) == -22
        return a == -22
    assert refused(kd=None)
    assert refused((-1, 0.5, 16, 16)) and refused((0, 0.5, 16, 16)) and refused((65, 0.5, 16, 16)) and refused((62, 0.5, 16, 16))
    for lam in (0.0, -0.1, 1.01, float("nan"), float("inf")):
        assert refused((8, lam, 16, 16)), lam
    assert refused((8, 0.5, None, 16)) and refused((8, 0.5, 16, None))
    assert refused(free_run=1) and refused(label_smoothing=0.1) and refused(storage=1)
    assert refused(mrt_n=4, mrt_alpha=0.5, mrt_scale=1.0, mrt_cost=16, rank_kind=-1)
    assert refused(V=0)                                        # not a valid configuration at all
    assert not refused() and not refused((8, 1.0, 16, 16)) and not refused((61, 0.5, 16, 16)) and not refused((1, 0.5, 16, 16))
    assert not refused(rank_kind=-1)                           # the ranking loss may be on (rank_kind = 0 above) or off
    short = _lib.StepCfg()                                     # the struct of the earlier size reads as mrt_n = 0
    for n, _ in _lib.StepCfg._fields_:
        setattr(short, n, getattr(_cfg(), n))
    assert L.vag_step_kd_check(C.byref(short), C.byref(_lib.KdCfg(8, 0.5, 16, 16))) == 0


# ------------------------------------------------------------------------------------------------------------------
# Python argument errors: raised before any device work
# ------------------------------------------------------------------------------------------------------------------
class _FakeF:
    storage16, label_smoothing, V = False, 0.0, 61


def _fake_ts(**kw):
    from vagnmt_hip.trainer import _FusedBackend

    class TS:
        world, zero1, multimodal, use_graph = 1, False, False, False
    ts = TS()
    ts.backend = _FusedBackend.__new__(_FusedBackend)
    ts.backend.f = _FakeF()
    for k, v in kw.items():
        setattr(ts, k, v)
    return ts


def test_distill_step_and_teacher_targets_argument_errors():
    from vagnmt_hip import distill
    from vagnmt_hip.trainer import TrainStep
    src = torch.zeros(3, 5, dtype=torch.int64)
    tgt = torch.zeros(3, 6, dtype=torch.int64)
    soft = distill.SoftTargets(torch.zeros(6, 3, 8, dtype=torch.int32), torch.zeros(6, 3, 8))

    def bad(match, exc=ValueError, ts=None, **kw):
        a = dict(src=src, lengths=[5, 4, 3], tgt=tgt, im=None, teacher_model=None, soft=soft, kd_lambda=0.5, top_k=8, temperature=1.0)
        a.update(kw)
        with pytest.raises(exc, match=match):
            distill.distill_step(ts or _fake_ts(), **a)
    for lam in (0.0, -0.5, 1.5, float("nan")):
        bad("kd_lambda", kd_lambda=lam)
    for k in (0, 65, 2.5):
        bad("top_k", top_k=k)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        bad("temperature", temperature=t)
    bad("exactly one", soft=None)
    bad("exactly one", teacher_model=object())
    bad("share B", tgt=torch.zeros(2, 6, dtype=torch.int64))
    bad("share B", tgt=torch.zeros(3, 6, dtype=torch.int32))
    bad("GPU")                                                 # everything else in order: CPU tensors are refused last
    # the follow-ups
    bad("autograd path is a follow-up", NotImplementedError, ts=_fake_ts(backend=object()))
    bad("follow-ups", NotImplementedError, ts=_fake_ts(world=2))
    bad("follow-ups", NotImplementedError, ts=_fake_ts(zero1=True))
    f16, ls = _fake_ts(), _fake_ts()
    f16.backend.f = type("F", (_FakeF,), {"storage16": True})()
    ls.backend.f = type("F", (_FakeF,), {"label_smoothing": 0.1})()
    bad("2-byte storage mode is a follow-up", NotImplementedError, ts=f16)
    bad("label-smoothed criterion is a follow-up", NotImplementedError, ts=ls)
    bad("needs im", ts=_fake_ts(multimodal=True))
    # soft targets of the wrong shape / type / content
    with pytest.raises(ValueError, match="int32"):
        distill.check_soft((soft.idx.long(), soft.q), 3, 6, 61)
    with pytest.raises(ValueError, match=r"\(Tt, B, K\)"):
        distill.check_soft(soft, 3, 5, 61)
    with pytest.raises(ValueError, match=r"\(Tt, B, K\)"):
        distill.check_soft(distill.SoftTargets(torch.zeros(6, 3, 65, dtype=torch.int32), torch.zeros(6, 3, 65)), 3, 6, 100)
    with pytest.raises(ValueError, match="GPU"):
        distill.check_soft(soft, 3, 6, 61)
    # teacher_targets
    class Teacher:
        tgt_size = 61
    for kw, match in ((dict(top_k=0), "top_k"), (dict(top_k=65), "top_k"), (dict(temperature=0.0), "temperature"),
                      (dict(vocab_size=60), "vocabulary"), (dict(top_k=62), "exceeds the vocabulary"), (dict(), "GPU")):
        with pytest.raises(ValueError, match=match):
            distill.teacher_targets(Teacher(), src, [5, 4, 3], tgt, **kw)
    # inside averaged_weights() the driver refuses, as step does
    ts = TrainStep.__new__(TrainStep)
    ts._averaged = True
    with pytest.raises(RuntimeError, match="averaged_weights"):
        ts.distill_step(src, [5, 4, 3], tgt, soft=soft)
    assert "follow-up" in distill.__doc__ and "Kim & Rush" in distill.__doc__
