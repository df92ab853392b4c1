"""CPU: minimum-risk training (vagnmt_hip.mrt, vag_mrt_weights / vag_mrt_pack): the float64 reference of tests/mrt_ref.py against
central differences and its own invariants, the pack's rules on the edge rows, mrt_step's argument errors, the ABI's new names
(header, binding table, vag_step_cfg and its ctypes mirror, the library's exports and its -EINVAL answers), and the learning case
of the GPU test in float64 on the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mrt_ref as R
from conftest import ROOT, load_golden


def _case(seed, G, N, Tt, p_valid=0.8):
    g = np.random.default_rng(seed)
    nll = g.uniform(0.0, 3.0, size=(Tt, G * N))
    cost = g.uniform(0.0, 1.0, size=G * N)
    valid = (g.uniform(size=G * N) < p_valid).astype(np.float32)
    valid[::N] = 1.0                                           # at least one valid row per group
    return nll, cost, valid


@pytest.mark.parametrize("N,G,Tt", [(2, 1, 1), (5, 3, 4), (17, 2, 3)])
def test_reference_gradient_is_alpha_q_cost_minus_risk(N, G, Tt):
    """d risk / d s_i = scale / G * alpha Q_i (c_i - R_g) = -inv_cnt[b_i] / B, against central differences in float64."""
    alpha, scale = 0.7, 0.5
    nll, cost, valid = _case(N + G, G, N, Tt)
    inv_cnt, q, risk = R.weights(nll, cost, valid, N, alpha, scale)
    B = G * N
    h = 1e-6
    for b in range(B):
        up, dn = nll.copy(), nll.copy()
        up[0, b] -= h                                          # s = -sum_t nll: s_b + h
        dn[0, b] += h
        num = (R.weights(up, cost, valid, N, alpha, scale)[2] - R.weights(dn, cost, valid, N, alpha, scale)[2]) / (2 * h)
        want = -inv_cnt[b] / B
        g = b // N
        idx = [i for i in range(g * N, g * N + N) if valid[i]]
        Rg = sum(q[i] * cost[i] for i in idx)
        assert want == pytest.approx(scale / G * alpha * q[b] * (cost[b] - Rg) if valid[b] else 0.0, abs=1e-15)
        assert num == pytest.approx(want, abs=1e-9), (b, num, want)
    # the same through autograd on the torch form the GPU test differentiates
    s = torch.tensor(-nll.sum(0), requires_grad=True)
    (scale * R.risk_torch(s, cost, valid, N, alpha)).backward()
    assert np.abs(s.grad.numpy() + inv_cnt / B).max() < 1e-14


def test_coefficients_of_a_group_sum_to_zero_and_q_to_one():
    for seed, (G, N, Tt) in enumerate([(1, 2, 1), (3, 5, 7), (2, 64, 3), (1, 256, 2)]):
        nll, cost, valid = _case(seed, G, N, Tt)
        inv_cnt, q, risk = R.weights(nll, cost, valid, N, 0.3, 1.0)
        for g in range(G):
            sl = slice(g * N, g * N + N)
            assert abs(inv_cnt[sl].sum()) < 1e-12 * N
            assert q[sl].sum() == pytest.approx(1.0, abs=1e-12)
            assert (inv_cnt[sl][valid[sl] == 0] == 0).all() and (q[sl][valid[sl] == 0] == 0).all()
        assert 0.0 <= risk <= 1.0
    # one valid row: Q = 1, coefficient 0, the group's risk is that row's cost
    nll, cost, valid = _case(9, 1, 4, 2)
    valid[:] = 0
    valid[2] = 1
    inv_cnt, q, risk = R.weights(nll, cost, valid, 4, 2.0, 1.0)
    assert q.tolist() == [0, 0, 1, 0] and not inv_cnt.any() and risk == cost[2]


def test_pack_reference_on_the_edge_rows():
    cand, gold, with_gold, without = R.edge_case()
    tgt, valid = R.pack(cand, gold, True)
    assert tgt.shape == (9, 7) and valid.tolist() == with_gold.tolist()
    assert tgt[0].tolist() == [10, 11, 12, 3, 0, 0, 0]                    # the gold row is candidate 0
    assert tgt[1].tolist() == tgt[0].tolist() and valid[1] == 0           # the gold sentence, sampled: removed
    assert tgt[3].tolist() == tgt[2].tolist() and valid[3] == 0           # a repeated sample: removed
    assert tgt[4].tolist() == [30, 31, 32, 33, 34, 35, 3]                 # no EOS at full length: the whole row, then EOS
    assert tgt[5].tolist() == [3, 0, 0, 0, 0, 0, 0] and valid[5] == 1     # an empty span: a valid one-token row
    assert valid[6] == 0                                                  # ... once
    assert tgt[7].tolist() == [40, 0, 41, 3, 0, 0, 0] and valid[7] == 0 and valid[8] == 0       # a span holding 0
    tgt2, valid2 = R.pack(cand, gold, False)
    assert tgt2.shape == (8, 7) and valid2.tolist() == without.tolist() and (tgt2 == tgt[1:]).all()
    # a wider target matrix only adds zeros
    tgt3, valid3 = R.pack(cand, gold, True, Tt=10)
    assert (tgt3[:, :7] == tgt).all() and not tgt3[:, 7:].any() and (valid3 == valid).all()
    # the cost of the gold row is 0, of an empty row 1
    cost = R.bleu_cost(tgt, gold, 9)
    assert cost[0] == 0.0 and cost[1] == 0.0 and cost[5] == 1.0 and (cost >= 0).all() and (cost <= 1).all()


def test_mrt_step_argument_errors():
    from vagnmt_hip import mrt
    src = torch.zeros(3, 5, dtype=torch.int64)
    tgt = torch.zeros(3, 6, dtype=torch.int64)
    ok = dict(n_candidates=4, alpha=0.01, method="stochastic", include_gold=True, max_length=None, candidates=None, max_rows=1024)

    def bad(match, **kw):
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match=match):
            mrt.check_args(a.pop("src", src), a.pop("tgt", tgt), **a)
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        bad("alpha", alpha=alpha)
    bad("method", method="beam")
    bad("1 .. 64", n_candidates=65)
    bad("1 .. 64", n_candidates=0)
    bad("rows per sentence", method="sample", n_candidates=256)
    bad("rows per sentence", method="sample", n_candidates=1, include_gold=False)
    bad("max_length", max_length=0)
    bad("511", max_length=512)
    bad("max_rows", max_rows=4)
    bad("share B", tgt=torch.zeros(2, 6, dtype=torch.int64))
    bad("share B", tgt=torch.zeros(3, 6, dtype=torch.int32))
    bad("candidates", candidates=torch.zeros(2, 4, 5, dtype=torch.int64))
    bad("candidates", candidates=torch.zeros(3, 4, 5, dtype=torch.int32))
    bad("candidates", candidates=[[1, 2]])
    bad("GPU", )                                               # everything else in order: CPU tensors are refused last
    with pytest.raises(ValueError, match="candidates"):
        mrt.expected_risk(None, src, [5, 4, 3], tgt, None, None, 0.5)

    class FakeTS:                                              # not the fused backend / more than one rank
        world, zero1, backend = 2, False, None
    with pytest.raises(NotImplementedError, match="follow-up"):
        mrt._backend(FakeTS(), "mrt_step")
    from vagnmt_hip.trainer import TrainStep
    assert "follow-up" in mrt.__doc__ and callable(TrainStep.mrt_step)


def test_new_symbols_and_step_cfg_fields_are_declared_and_mirrored():
    from vagnmt_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("vag_mrt_weights", "vag_mrt_pack"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.PROTOS
    body = re.search(r"typedef struct \{([^}]*)\}\s*vag_step_cfg;", code, flags=re.S).group(1)
    tail = body[body.index("label_smoothing"):]
    assert re.sub(r"\s+", " ", tail).strip() == ("label_smoothing; int32_t mrt_n; float mrt_alpha, mrt_scale; "
                                                   "const float *mrt_cost, *mrt_valid;")
    names = [n for n, _ in _lib.StepCfgMrt._fields_]
    assert names[-6:] == ["label_smoothing", "mrt_n", "mrt_alpha", "mrt_scale", "mrt_cost", "mrt_valid"]
    # StepCfg, the struct before these fields, is a prefix of it whose zeroed tail padding reads as mrt_n = 0
    assert _lib.StepCfgMrt._fields_[:len(_lib.StepCfg._fields_)] == _lib.StepCfg._fields_
    assert all(getattr(_lib.StepCfgMrt, n).offset == getattr(_lib.StepCfg, n).offset for n, _ in _lib.StepCfg._fields_)
    assert C.sizeof(_lib.StepCfg) == 152 and _lib.StepCfgMrt.mrt_n.offset == 148 and C.sizeof(_lib.StepCfgMrt) == 176
    assert (_lib.StepCfgMrt.mrt_alpha.offset, _lib.StepCfgMrt.mrt_scale.offset, _lib.StepCfgMrt.mrt_cost.offset,
            _lib.StepCfgMrt.mrt_valid.offset) == (152, 156, 160, 168)          # the C layout of include/vag_nmt.h
    kinds = dict(_lib.StepCfgMrt._fields_)
    assert kinds["mrt_n"] is C.c_int and kinds["mrt_alpha"] is C.c_float and kinds["mrt_scale"] is C.c_float
    assert kinds["mrt_cost"] is C.c_void_p and kinds["mrt_valid"] is C.c_void_p
    c = _lib.StepCfgMrt()
    assert c.mrt_n == 0 and c.mrt_alpha == 0.0 and c.mrt_scale == 0.0 and c.mrt_cost is None and c.mrt_valid is None
    assert "Shen et al" in hdr and "V11.py:162-166" in hdr
    for f in ("Makefile", "asan.mk"):
        assert "mrt.hip" in open(os.path.join(ROOT, "vag-nmt_amd", "csrc", f)).read(), f


def _cfg():
    from vagnmt_hip import _lib
    c = _lib.StepCfgMrt()
    c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = 8, 9, 7, 32, 32, 64, 32, 48, 61, 64
    c.multimodal, c.rank_kind = 1, -1
    return c


def test_library_answers_einval_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    one = C.c_void_p(16)                                       # a non-NULL address nothing may follow
    assert L.vag_mrt_weights(None, one, None, 8, 7, 4, 0.5, 1.0, one, None, one, None) == -22
    for N, B in ((1, 8), (257, 514), (3, 8), (0, 8)):
        assert L.vag_mrt_weights(one, one, None, B, 7, N, 0.5, 1.0, one, None, one, None) == -22
    for alpha, scale in ((0.0, 1.0), (-1.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0), (0.5, 0.0), (0.5, float("nan"))):
        assert L.vag_mrt_weights(one, one, None, 8, 7, 4, alpha, scale, one, None, one, None) == -22
    assert L.vag_mrt_weights(one, one, None, 8, 0, 4, 0.5, 1.0, one, None, one, None) == -22
    assert L.vag_mrt_weights(one, one, None, 8, 7, 4, 0.5, 1.0, one, None, None, None) == -22
    assert L.vag_mrt_pack(None, 3, 7, 6, one, 7, 1, one, 7, one, None) == -22
    assert L.vag_mrt_pack(one, 3, 7, 6, None, 7, 1, one, 7, one, None) == -22           # include_gold without gold
    assert L.vag_mrt_pack(one, 3, 7, 6, one, 7, 1, one, 6, one, None) == -22            # Tt < L + 1
    assert L.vag_mrt_pack(one, 3, 7, 6, one, 9, 1, one, 8, one, None) == -22            # Tt < Tg
    assert L.vag_mrt_pack(one, 3, 256, 6, one, 7, 1, one, 7, one, None) == -22          # N = 257
    assert L.vag_mrt_pack(one, 3, 7, 513, one, 7, 0, one, 514, one, None) == -22
    assert L.vag_mrt_pack(one, 0, 7, 6, one, 7, 1, one, 7, one, None) == -22
    assert L.vag_mrt_pack(one, 3, 7, 6, one, 7, 2, one, 7, one, None) == -22
    # the fused step's configuration
    c = _cfg()
    base = L.vag_step_ws_floats(c.ref())
    assert base > 0
    c.mrt_n, c.mrt_alpha, c.mrt_scale, c.mrt_cost = 4, 0.5, 1.0, 16
    assert L.vag_step_ws_floats(c.ref()) == base            # the minimum-risk step needs no workspace of its own
    short = _lib.StepCfg()                                     # the struct of the earlier size: read as "off"
    for n, _ in _lib.StepCfg._fields_:
        setattr(short, n, getattr(_cfg(), n))
    assert L.vag_step_ws_floats(C.byref(short)) == base

    def refused(**kw):
        d = _cfg()
        d.mrt_n, d.mrt_alpha, d.mrt_scale, d.mrt_cost = 4, 0.5, 1.0, 16
        for k, v in kw.items():
            setattr(d, k, v)
        return L.vag_step_ws_floats(d.ref()) == -22
    assert refused(mrt_n=3) and refused(mrt_n=1) and refused(mrt_n=-4) and refused(B=512 + 256, mrt_n=257 + 127)
    assert refused(free_run=1) and refused(label_smoothing=0.1) and refused(storage=1) and refused(rank_kind=0)
    assert refused(mrt_alpha=0.0) and refused(mrt_alpha=float("inf")) and refused(mrt_scale=0.0) and refused(mrt_cost=None)
    assert not refused()


def test_learning_case_falls_at_every_step_in_float64():
    """What tests/test_gpu_mrt.py asserts of five mrt_steps on the GPU, first in float64 on the oracle: at LEARN's rate and seed the
    risk of the fixed candidate set falls at every step, by far more than an fp32 evaluation's error."""
    meta, P, z = load_golden(R.LEARN["golden"])
    cand = R.learn_candidates(z["tgt"], meta["dims"][1])
    risks = R.learn_reference(P, z["src"], meta["lengths"], z["tgt"], cand)
    print("[mrt learns, fp64] " + " ".join("%.6f" % r for r in risks))
    assert len(risks) == R.LEARN["steps"] + 1
    for a, b in zip(risks, risks[1:]):
        assert b < a - 1e-3, risks
