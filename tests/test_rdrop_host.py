"""CPU: R-Drop (vagnmt_hip.rdrop; vag_rdrop_head_ce_seq_fwd / _bwd, vag_train_step_rdrop / vag_rdrop_cfg, vag_rank_loss_fwd's
kind | 2): the float64 reference of tests/rdrop_ref.py against torch fp64 autograd and against direct formulas, the ABI's new names
(header, binding table, the library's exports and its -EINVAL answers before anything touches a device), the argument and refusal
paths of rdrop_step with an injected backend, and the graph key."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rdrop_ref as R
from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def _case(seed, Bt=6, Tt=3, V=37):
    g = np.random.default_rng(seed)
    x = g.normal(size=(Tt * Bt, V)) * 2.0
    tgt = g.integers(1, V, size=(Bt // 2, Tt)).repeat(2, 0)     # twins share their target
    tgt[2:4, 2] = 0                                            # PAD in both rows of a pair
    tgt[4, 1:] = 0                                             # ... and in one row only (a case the definition covers)
    x[Bt:Bt + 2] = x[Bt]                                       # one identical pair (t = 1, rows 0, 1)
    return x, tgt


def _torch_loss(x, tgt, alpha, eps):
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    t = torch.from_numpy(tgt)
    Bt, Tt = t.shape
    V = xt.shape[1]
    lp = torch.log_softmax(xt, -1)
    y = t.t().reshape(-1)
    w = (y != 0).double()
    pair = lp.view(-1, 2, V)
    tw = pair.flip(1).reshape(-1, V)
    kl = (lp.exp() * (lp - tw)).sum(-1)
    both = kl.view(-1, 2).sum(-1).repeat_interleave(2)
    plain = -((1 - eps) * lp.gather(1, y[:, None])[:, 0] + eps / V * lp.sum(-1))
    nll = w * (plain + alpha / 4 * both)
    loss = (nll.view(Tt, Bt).sum(0) / (t != 0).double().sum(-1)).mean()
    loss.backward()
    return float(loss.detach()), nll.detach().numpy(), kl.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("alpha", [1.0, 5.0])
def test_reference_matches_torch_fp64_autograd(alpha, eps):
    x, tgt = _case(1)
    want_loss, want_nll, want_kl, want_g = _torch_loss(x, tgt, alpha, eps)
    nll, kl = R.nll_rows(x, tgt, alpha, eps)
    assert np.abs(kl - want_kl).max() < 1e-13 and np.abs(nll - want_nll).max() < 1e-12
    assert R.loss_mt(nll, tgt) == pytest.approx(want_loss, abs=1e-13)
    g = R.dlogits(x, tgt, alpha, eps)
    assert np.abs(g - want_g).max() < 1e-14, np.abs(g - want_g).max()
    assert np.abs(want_g).max() > 1e-3 and kl.max() > 0.5       # independent twins: KL of order 1
    assert kl[6] == 0.0 and kl[7] == 0.0                        # the identical pair: exactly nothing
    plain = R.dlogits(x, tgt, 1e-300, eps)
    assert np.abs(g[6:8] - plain[6:8]).max() < 1e-16            # ... and the plain gradient
    assert np.abs(g.sum(-1)).max() < 1e-14                      # every row of d(logits) sums to zero
    y = R.rows_targets(tgt)
    both_pad = (y.reshape(-1, 2) == 0).all(1).repeat(2)
    one_pad = (y == 0) & ~both_pad
    assert both_pad.any() and one_pad.any()
    assert np.abs(g[both_pad]).max() == 0.0 and np.abs(g[one_pad]).max() > 0    # a PAD row still carries its twin's KL gradient
    assert (nll[y == 0] == 0).all()


def test_reference_per_sentence_form_is_half_the_papers():
    """mean(CE_1, CE_2) + (alpha / 2) sum_t (KL_12 + KL_21) / 2 / count per sentence, averaged over sentences."""
    g = np.random.default_rng(3)
    Bt, Tt, V, alpha = 4, 3, 11, 5.0
    x = g.normal(size=(Tt * Bt, V))
    tgt = g.integers(1, V, size=(Bt // 2, Tt)).repeat(2, 0)
    tgt[0:2, 2] = 0
    nll, kl = R.nll_rows(x, tgt, alpha)
    lp = R.log_softmax(x).reshape(Tt, Bt, V)
    klm = kl.reshape(Tt, Bt)
    tot = 0.0
    for s in range(Bt // 2):
        n = int((tgt[2 * s] != 0).sum())
        ce = [-sum(lp[t, 2 * s + i, tgt[2 * s, t]] for t in range(n)) / n for i in (0, 1)]
        sym = sum(klm[t, 2 * s] + klm[t, 2 * s + 1] for t in range(n)) / 2
        tot += 0.5 * (ce[0] + ce[1]) + alpha / 2 * sym / n
    assert R.loss_mt(nll, tgt) == pytest.approx(tot / (Bt // 2), abs=1e-13)


@pytest.mark.parametrize("kind", [0, 1])
def test_twin_ranking_loss_against_direct_formulas(kind):
    g = np.random.default_rng(5 + kind)
    Bt, S, margin = 8, 6, 0.1
    nrm = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)      # noqa: E731
    im, s = nrm(g.normal(size=(Bt, S))), nrm(g.normal(size=(Bt, S)))
    loss, G = R.rank_loss_twins(im, s, margin, kind)
    # a vectorised torch statement of the same rule, and its autograd gradient with respect to the scores
    Sc = (torch.from_numpy(im) @ torch.from_numpy(s).t()).requires_grad_(True)
    i = torch.arange(Bt)
    keep = (i[:, None] >> 1) != (i[None, :] >> 1)
    d = torch.diagonal(Sc)
    tl = torch.clamp(margin - d[None, :] + Sc, min=0)[keep].sum()
    if kind == 0:
        tl = tl + torch.clamp(margin - d[:, None] + Sc, min=0)[keep].sum()
    tl.backward()
    assert loss == pytest.approx(float(tl), abs=1e-13) and loss > 0.1
    assert np.abs(G - Sc.grad.numpy()).max() == 0.0
    assert all(G[a, a ^ 1] == 0 for a in range(Bt))
    assert loss < R.rank_loss_plain(im, s, margin, kind)        # the rule removes something here
    # identical twins (no dropout): a quarter of the twin-aware loss on the 2B rows is the plain loss on the B sentences
    im2, s2 = im[:4].repeat(2, 0), s[:4].repeat(2, 0)
    assert 0.25 * R.rank_loss_twins(im2, s2, margin, kind)[0] == pytest.approx(R.rank_loss_plain(im[:4], s[:4], margin, kind), abs=1e-13)
    # one sentence (Bt = 2): nothing is a negative
    l1, G1 = R.rank_loss_twins(im[:2], s[:2], margin, kind)
    assert l1 == 0.0 and not G1.any()


# ------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_the_rdrop_struct_are_declared_and_mirrored():
    from vagnmt_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "vag_nmt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("vag_rdrop_head_ce_seq_fwd", "vag_rdrop_head_ce_seq_bwd", "vag_step_rdrop_check", "vag_train_step_rdrop"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.PROTOS
        assert hasattr(_lib.lib(), name)
    # the head's entry points: the _ls argument lists with (float alpha, kl) between the smoothing and the stream
    for d in ("fwd", "bwd"):
        ls = _lib.PROTOS["vag_head_ce_seq_%s_ls" % d][1]
        assert _lib.PROTOS["vag_rdrop_head_ce_seq_%s" % d][1] == ls[:-1] + [_lib.F, _lib.P, _lib.P]
    ts = _lib.PROTOS["vag_train_step"][1]
    assert _lib.PROTOS["vag_train_step_rdrop"][1] == ts[:1] + [C.POINTER(_lib.RdropCfg)] + ts[1:]
    assert _lib.PROTOS["vag_step_rdrop_check"][1] == [_lib.StepCfgArg, C.POINTER(_lib.RdropCfg)]
    # vag_step_cfg is as it was; vag_rdrop_cfg and its mirror
    body = re.search(r"typedef struct \{([^}]*)\}\s*vag_step_cfg;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip().endswith("const float *mrt_cost, *mrt_valid;") and C.sizeof(_lib.StepCfgMrt) == 176
    rd = re.search(r"typedef struct \{([^}]*)\}\s*vag_rdrop_cfg;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", rd).strip() == "float alpha; float* kl;"
    assert _lib.RdropCfg._fields_ == [("alpha", C.c_float), ("kl", C.c_void_p)]
    assert (_lib.RdropCfg.alpha.offset, _lib.RdropCfg.kl.offset, C.sizeof(_lib.RdropCfg)) == (0, 8, 16)
    assert "Liang et al. 2021" in hdr and "kind | 2" in hdr
    for f in ("Makefile", "asan.mk"):
        path = os.path.join(ROOT, "vag-nmt_amd", "csrc", f)
        if os.path.isfile(path):                               # (asan.mk stays on the CPU box)
            assert "rdrop.hip" in open(path).read(), f


def _head_calls(L, _lib, alpha=5.0, kl=16, B=4, eps=0.1, logits_ready=0, V=1000, null=False):
    x = None if null else C.c_void_p(16)
    hw = _lib.HeadW() if null else _lib.HeadW(*([16] * 8))
    ldl = (V + 3) // 4 * 4
    k = None if (null or not kl) else C.c_void_p(kl)
    f = L.vag_rdrop_head_ce_seq_fwd(x, x, x, hw, x, x, B, 3, 8, 8, V, 0.0, None, logits_ready, x, x, ldl, x, x, x, x, eps, alpha, k, None)
    b = L.vag_rdrop_head_ce_seq_bwd(x, x, x, hw, x, x, B, 3, 8, 8, V, 0.0, None, x, x, ldl, x, x, x, x, x, x, hw, x, eps, alpha, k, None)
    return f, b


def test_rdrop_head_entry_points_answer_einval_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    for a in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert _head_calls(L, _lib, alpha=a) == (-22, -22), a
    assert _head_calls(L, _lib, kl=None) == (-22, -22)
    for B in (3, 1, 5):
        assert _head_calls(L, _lib, B=B) == (-22, -22), B
    assert _head_calls(L, _lib, logits_ready=1)[0] == -22
    assert _head_calls(L, _lib, eps=1.0) == (-22, -22) and _head_calls(L, _lib, eps=-0.1) == (-22, -22)      # the namesakes' refusals
    assert _head_calls(L, _lib, V=0) == (-22, -22)
    assert _head_calls(L, _lib, null=True) == (-22, -22)
    try:                                                        # the 2-byte storage mode of the calling thread
        assert L.vag_set_operator_context(C.c_void_p(16), 1) == 0
        assert _head_calls(L, _lib) == (-22, -22)
    finally:
        assert L.vag_set_operator_context(None, 0) == 0


def test_rank_loss_kind_is_checked_before_anything_is_launched():
    from vagnmt_hip import _lib
    L = _lib.lib()
    x = C.c_void_p(16)
    for kind in (-1, 4, 7):
        assert L.vag_rank_loss_fwd(x, x, 4, 4, 0.1, kind, x, x, x, None) == -22, kind
    for kind in (2, 3):                                         # the twin flag needs whole pairs
        assert L.vag_rank_loss_fwd(x, x, 5, 4, 0.1, kind, x, x, x, None) == -22, kind


def _cfg():
    from vagnmt_hip import _lib
    c = _lib.StepCfgMrt()
    c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = 8, 9, 7, 32, 32, 64, 32, 48, 61, 64
    c.multimodal, c.rank_kind = 1, 0
    return c


def test_step_combinations_are_refused_before_touching_a_device():
    from vagnmt_hip import _lib
    L = _lib.lib()
    ws = L.vag_step_ws_floats(_cfg().ref())
    assert ws > 0                                              # (the workspace is the plain step's: there is no other query)

    def refused(rd=(5.0, 16), **kw):
        d = _cfg()
        for k, v in kw.items():
            setattr(d, k, v)
        r = None if rd is None else C.byref(_lib.RdropCfg(*rd))
        p = 4096
        a = L.vag_step_rdrop_check(d.ref(), r)
        assert a in (0, -22)
        if a == -22:                                           # ... and the step itself says the same, whatever the rest
            assert L.vag_train_step_rdrop(d.ref(), r, C.byref(_lib.ModelW()), C.byref(_lib.ModelW()), p, p, p, p, p, None, None, p, p,
                                          7, None) == -22
        return a == -22
    assert refused(rd=None)
    for a in (0.0, -5.0, float("nan"), float("inf")):
        assert refused((a, 16)), a
    assert refused((5.0, None))
    assert refused(B=7) and refused(B=1)
    assert refused(free_run=1) and refused(storage=1)
    assert refused(mrt_n=4, mrt_alpha=0.5, mrt_scale=1.0, mrt_cost=16, rank_kind=-1)
    assert refused(V=0) and refused(label_smoothing=1.0)       # not a valid configuration at all
    assert not refused() and not refused((1e-3, 16)) and not refused(B=2)
    assert not refused(label_smoothing=0.1)                    # smoothing composes with it
    assert not refused(rank_kind=-1) and not refused(rank_kind=1) and not refused(multimodal=0)
    short = _lib.StepCfg()                                     # the struct of the earlier size reads as mrt_n = 0
    for n, _ in _lib.StepCfg._fields_:
        setattr(short, n, getattr(_cfg(), n))
    assert L.vag_step_rdrop_check(C.byref(short), C.byref(_lib.RdropCfg(5.0, 16))) == 0
    assert L.vag_step_ws_floats(_cfg().ref()) == ws


# ------------------------------------------------------------------------------------------------------------------
# Python: argument errors and refusals before any device work; the graph key
# ------------------------------------------------------------------------------------------------------------------
class _FakeF:
    storage16, label_smoothing, V = False, 0.1, 61


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


def test_rdrop_step_argument_errors_and_refusals():
    from vagnmt_hip import rdrop
    from vagnmt_hip.trainer import TrainStep
    src = torch.zeros(3, 5, dtype=torch.int64)
    tgt = torch.zeros(3, 6, dtype=torch.int64)

    def bad(match, exc=ValueError, ts=None, **kw):
        a = dict(src=src, lengths=[5, 4, 3], tgt=tgt, im=None, alpha=5.0)
        a.update(kw)
        with pytest.raises(exc, match=match):
            rdrop.rdrop_step(ts or _fake_ts(), **a)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        bad("alpha", alpha=a)
    bad("share B", tgt=torch.zeros(2, 6, dtype=torch.int64))
    bad("share B", tgt=torch.zeros(3, 6, dtype=torch.int32))
    bad("GPU")                                                 # everything else in order (smoothing included): CPU tensors are refused last
    bad("autograd path is a follow-up", NotImplementedError, ts=_fake_ts(backend=object()))
    bad("follow-ups", NotImplementedError, ts=_fake_ts(world=2))
    bad("follow-ups", NotImplementedError, ts=_fake_ts(zero1=True))
    f16 = _fake_ts()
    f16.backend.f = type("F", (_FakeF,), {"storage16": True})()
    bad("2-byte storage mode is a follow-up", NotImplementedError, ts=f16)
    bad("needs im", ts=_fake_ts(multimodal=True))
    ts = TrainStep.__new__(TrainStep)
    ts._averaged = True
    with pytest.raises(ValueError, match="averaged_weights"):
        ts.rdrop_step(src, [5, 4, 3], tgt)
    assert "teacher_force_ratio" in TrainStep.rdrop_step.__doc__ and "teacher_force_ratio" in rdrop.rdrop_step.__doc__
    assert "follow-up" in rdrop.__doc__ and "Liang et al. 2021" in rdrop.__doc__
    # mean_kl: the per-token mean over non-PAD positions of the symmetric KL, and its shape check
    kl = torch.arange(12, dtype=torch.float32).view(3, 4)       # (Tt, 2B), B = 2
    t2 = torch.tensor([[5, 6, 0], [7, 0, 0]])
    want = (0.5 * (0 + 1) + 0.5 * (4 + 5) + 0.5 * (2 + 3)) / 3
    assert float(rdrop.mean_kl(rdrop.RDrop(None, None, None, kl), t2)) == pytest.approx(want)
    with pytest.raises(ValueError, match="does not belong"):
        rdrop.mean_kl(kl, torch.zeros(3, 3, dtype=torch.int64))
    assert torch.equal(rdrop.twins(torch.tensor([[1, 2], [3, 4]])), torch.tensor([[1, 2], [1, 2], [3, 4], [3, 4]]))


def test_graph_key_differs_by_alpha_and_the_batch_is_duplicated():
    """_FusedBackend.run(rdrop=(alpha,)) with a recording FusedStep: alpha is part of the key (it is captured by value), the plain
    step's key has no such entry, and rdrop_step hands the backend every row twice in adjacent rows."""
    import collections
    from vagnmt_hip import rdrop
    from vagnmt_hip.trainer import _FusedBackend

    class F:
        storage16, label_smoothing, V, generation = False, 0.0, 61, 0
        rd_kl = torch.zeros(64)

        def __init__(self):
            self.ran, self.loaded = [], []

        def reserve(self, B, Ts, Tt):
            return False

        def load_batch(self, src, lengths, tgt, im):
            self.loaded.append((src.clone(), lengths.clone(), tgt.clone()))

        def run(self, B, Ts, Tt, teacher, phases, mrt=None, kd=None, rdrop=None):
            self.ran.append((B, Ts, Tt, teacher, phases, mrt, kd, rdrop))

    class TS:
        world, zero1, multimodal, use_graph, pad_src, capture_after, max_graphs = 1, False, False, True, 1, 10 ** 9, 4
    ts = TS()
    ts._graphs, ts._seen, ts._opt_graphs = collections.OrderedDict(), collections.OrderedDict(), {}
    ts.stats = {"captures": 0, "evictions": 0, "eager_steps": 0, "replays": 0}
    ts._optimizer = lambda: None
    be = _FusedBackend.__new__(_FusedBackend)
    be.ts, be.f = ts, F()
    src = torch.tensor([[4, 5, 6], [7, 8, 0]])
    lens = torch.tensor([3, 2], dtype=torch.int32)
    tgt = torch.tensor([[9, 3], [3, 0]])
    be.run(src, lens, tgt, None, True, 7, rdrop=(5.0,))
    be.run(src, lens, tgt, None, True, 7, rdrop=(1.0,))
    be.run(src, lens, tgt, None, True, 7, rdrop=(5.0,))
    be.run(src, lens, tgt, None, True, 7)
    keys = [k for k, _ in ts._seen]
    assert len(keys) == 3 and ts._seen[(keys[0], 7)] == 2
    assert keys[0] == (2, 3, 2, True, ("rdrop", 5.0)) and keys[1] == (2, 3, 2, True, ("rdrop", 1.0)) and keys[2] == (2, 3, 2, True)
    assert [r[-1] for r in be.f.ran] == [(5.0,), (1.0,), (5.0,), None]
    # rdrop_step through the same backend: 2B rows, twins adjacent, lengths still sorted, always teacher-forced, kl a (Tt, 2B) view
    ts.backend, ts.model = be, torch.nn.Linear(1, 1)
    be.outputs = lambda: (torch.zeros(()), torch.zeros(()), torch.zeros(()))
    ts.use_graph = False
    ts._run_optimizer = lambda: ts.stats.__setitem__("opt", ts.stats.get("opt", 0) + 1)

    class CudaLike(torch.Tensor):
        is_cuda = True
    out = rdrop.rdrop_step(ts, src.as_subclass(CudaLike), lens, tgt.as_subclass(CudaLike), None, alpha=2.0)
    s2, l2, t2 = be.f.loaded[-1]
    assert torch.equal(torch.as_tensor(s2), src.repeat_interleave(2, 0)) and l2.tolist() == [3, 3, 2, 2]
    assert torch.equal(torch.as_tensor(t2), tgt.repeat_interleave(2, 0))
    assert be.f.ran[-1] == (4, 3, 2, True, 7, None, None, (2.0,)) and ts.stats["opt"] == 1
    assert isinstance(out, rdrop.RDrop) and out.kl.shape == (2, 4) and out.kl.data_ptr() == be.f.rd_kl.data_ptr()
    assert ts.model.training and ts.model._vag_weights_version == 1
