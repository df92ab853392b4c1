"""GPU: averaged weights -- vag_clip_adam_flat_ema / vag_swap_flat at the C ABI on synthetic buffers, and the step driver's
ema_decay / averaged_weights() / checkpoint resume on the golden fixtures.

The bound on the averaged weights everywhere: against an fp64 recurrence e <- e + (1 - d_t) (p - e) fed with the DEVICE's own fp32
parameters after each call, elementwise ``calls * 2**-22 * max|p|``.  Per call the device makes at most three fp32 roundings
(the difference, the product, the sum -- two when the compiler contracts the last two) on values no larger than
2 max(|p|, |e|), i.e. 3 * 2**-24 * 2 max|p| < 2**-22 max|p|, which also covers the fp32 rounding of 1 - d_t; the recurrence is a
convex combination, so |e| <= max|p| as long as it starts there, and the per-call errors add without growing."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_golden import build, criteria, close
from test_gpu_trainer import _inputs

pytestmark = pytest.mark.gpu

SEG_LR = [1e-2, 5e-3, 2e-2]
SEG_WD = [1e-5, 0.0, 1e-3]
BETAS, EPS = (0.9, 0.999), 1e-8
SKIPPED_WORD = 28 // 4          # VAG_ADAM_SCRATCH_SKIPPED_OFFSET


def _seg_off(n):
    """Three segments whose interior boundaries are no multiples of 4 (the kernel indexes by element).  At the largest size the
    middle segment alone is longer than the 4096 x 256 threads of the capped grid, so the stride loop goes round."""
    return {1: [0, 0, 1, 1], 5: [0, 1, 3, 5], 1027: [0, 301, 702, 1027]}.get(n, [0, 1, n - 1, n])


def _d(t, decay, warmup):
    decay = float(np.float32(decay))              # the entry point takes a float
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class Bufs:
    def __init__(self, n, seed, lr_dev=0.5):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, device="cuda", generator=g)
        self.g = torch.randn(n, device="cuda", generator=g)
        self.m = torch.randn(n, device="cuda", generator=g) * 0.1
        self.v = torch.rand(n, device="cuda", generator=g) * 0.01
        self.e = self.p * -0.5                                      # |e| <= |p|, visibly not p
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.norm = torch.zeros(1, device="cuda")
        self.scratch = torch.zeros(512, device="cuda")
        self.lr = torch.full((1,), lr_dev, device="cuda")

    def twin(self):
        t = Bufs.__new__(Bufs)
        t.n = self.n
        for k in ("p", "g", "m", "v", "e", "step", "norm", "scratch", "lr"):
            setattr(t, k, getattr(self, k).clone())
        return t

    def state(self):
        return {k: getattr(self, k).clone() for k in ("p", "g", "m", "v", "e", "step", "norm", "scratch", "lr")}

    def args(self, clip):
        from vagnmt_hip._lib import ptr
        off = _seg_off(self.n)
        ns = len(off) - 1
        return (ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), self.n, ns, (C.c_int64 * (ns + 1))(*off),
                (C.c_float * ns)(*SEG_LR), (C.c_float * ns)(*SEG_WD), float(clip), 1.0, BETAS[0], BETAS[1], EPS, 1,
                ptr(self.step, torch.int32), ptr(self.norm), self.scratch.data_ptr(), ptr(self.lr))


def _flat(b, clip):
    from vagnmt_hip._lib import lib, stream
    return lib().vag_clip_adam_flat(*b.args(clip), stream())


def _ema(b, clip, decay, warmup, ema="own"):
    from vagnmt_hip._lib import lib, stream
    e = b.e.data_ptr() if ema == "own" else ema
    return lib().vag_clip_adam_flat_ema(*b.args(clip), e, float(decay), int(warmup), stream())


# ------------------------------------------------------------------------------------------------------------------
# 1. sizes, three consecutive calls each, warm-up on and off
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("n", [1, 5, 1027, 4096 * 256 + 3])
def test_ema_entry_point_equals_the_plain_one_and_the_fp64_recurrence(n, warmup):
    decay, calls = 0.9, 3
    # clip = 0 at the largest size: more than one block per slot of the norm's partial sums there, whose atomics may order
    # differently from run to run; with clip <= 0 the coefficient does not depend on the norm
    clip = 1.0 if n <= 131072 else 0.0
    a = Bufs(n, seed=n + int(warmup))
    b = a.twin()
    e_ref = a.e.double()
    pmax = 0.0
    gen = torch.Generator(device="cuda").manual_seed(7)
    for t in range(1, calls + 1):
        if t > 1:                                       # (the previous call left the gradient zeroed)
            a.g.copy_(torch.randn(n, device="cuda", generator=gen))
            b.g.copy_(a.g)
        e_prev = a.e.clone()
        assert _ema(a, clip, decay, warmup) == 0
        assert _flat(b, clip) == 0
        torch.cuda.synchronize()
        for k in ("p", "m", "v", "step"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (k, t)
        if clip > 0:
            assert torch.equal(a.norm, b.norm), t
        else:
            assert abs(float(a.norm) - float(b.norm)) <= 1e-5 * float(b.norm)
        assert int(a.step) == t and float(a.g.abs().max()) == 0.0
        om = 1.0 - _d(t, decay, warmup)
        e_ref = e_ref + om * (a.p.double() - e_ref)
        pmax = max(pmax, float(a.p.abs().max()))
        err = float((a.e.double() - e_ref).abs().max())
        print("n=%d warmup=%s t=%d: max |ema - fp64| = %.3e, bound %.3e" % (n, warmup, t, err, t * 2.0 ** -22 * pmax))
        assert err <= t * 2.0 ** -22 * pmax, (t, err)
        # d_t itself, read off the element that moved the farthest: (1 + t) / (10 + t) with warm-up, the decay without
        diff = (a.p - e_prev).double()
        k = int(diff.abs().argmax())
        om_dev = float((a.e[k].double() - e_prev[k].double()) / diff[k])
        # (the bound above on this one element, divided by the distance it is read from, plus the fp32 rounding of 1 - d_t)
        tol = 2.0 ** -22 * max(abs(float(a.p[k])), abs(float(e_prev[k]))) / abs(float(diff[k])) + 2.0 ** -24
        assert abs(om_dev - om) <= tol, (t, om_dev, om, tol)
        assert abs((1.0 - om_dev) - ((1.0 + t) / (10.0 + t) if warmup else decay)) <= tol + 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------
# 2. a void gradient: the optimiser's ordinary skip path
# ------------------------------------------------------------------------------------------------------------------
def test_a_void_gradient_leaves_the_average_alone():
    n, decay = 1027, 0.9
    a = Bufs(n, seed=3)
    a.g[700] = float("nan")
    before = a.state()
    assert _ema(a, 1.0, decay, True) == 0
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "e", "step"):
        assert torch.equal(getattr(a, k), before[k]), k
    words = a.scratch.view(torch.int32)
    assert int(words[SKIPPED_WORD]) == int(before["scratch"].view(torch.int32)[SKIPPED_WORD]) + 1
    assert float(a.g.abs().max()) == 0.0 and bool(torch.isnan(a.norm).all())
    # a following good call applies, with t = 1
    a.g.copy_(torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)))
    b = a.twin()
    assert _ema(a, 1.0, decay, True) == 0 and _flat(b, 1.0) == 0
    torch.cuda.synchronize()
    assert int(a.step) == 1 and int(words[SKIPPED_WORD]) == 1 and bool(torch.isfinite(a.norm).all())
    for k in ("p", "m", "v", "step", "norm"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    e_ref = before["e"].double() + (1.0 - 2.0 / 11.0) * (a.p.double() - before["e"].double())
    assert float((a.e.double() - e_ref).abs().max()) <= 2.0 ** -22 * float(a.p.abs().max())


# ------------------------------------------------------------------------------------------------------------------
# 3. refused arguments: -EINVAL before anything is enqueued
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["null", "misaligned", "zero", "one", "negative", "above", "nan"])
def test_refused_arguments_touch_nothing(case):
    n = 1027
    a = Bufs(n, seed=5)
    spare = torch.zeros(n + 4, device="cuda")
    before, spare_before = a.state(), spare.clone()
    decay = {"zero": 0.0, "one": 1.0, "negative": -0.5, "above": 1.5, "nan": float("nan")}.get(case, 0.9)
    ema = {"null": None, "misaligned": spare.data_ptr() + 4}.get(case, "own")
    assert _ema(a, 1.0, decay, True, ema=ema) == -22
    torch.cuda.synchronize()
    after = a.state()
    for k in before:
        assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), k
    assert torch.equal(spare, spare_before)


# ------------------------------------------------------------------------------------------------------------------
# 4. vag_swap_flat
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2 ** 20 + 3])
def test_swap_flat_is_an_exact_exchange(n):
    from vagnmt_hip._lib import lib, stream
    g = torch.Generator(device="cuda").manual_seed(n)
    pad = (n + 3) // 4 * 4 - n                         # the sentinels follow n directly, wherever n ends
    A = torch.randn(n + 8 + pad, device="cuda", generator=g)
    B = torch.randn(n + 8 + pad, device="cuda", generator=g)
    A[0] = float("nan")                                # bit patterns travel, not values
    B[n - 1] = -0.0
    A0, B0 = A.clone(), B.clone()
    assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
    assert lib().vag_swap_flat(A.data_ptr(), B.data_ptr(), n, stream()) == 0
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32)              # noqa: E731
    assert torch.equal(bits(A[:n]), bits(B0[:n])) and torch.equal(bits(B[:n]), bits(A0[:n]))
    assert torch.equal(bits(A[n:n + 8]), bits(A0[n:n + 8])) and torch.equal(bits(B[n:n + 8]), bits(B0[n:n + 8]))
    assert lib().vag_swap_flat(A.data_ptr(), B.data_ptr(), n, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(A), bits(A0)) and torch.equal(bits(B), bits(B0))
    # a misaligned base, either side, a NULL, two windows of one buffer: refused, nothing moves
    for pa, pb in ((A.data_ptr() + 4, B.data_ptr()), (A.data_ptr(), B.data_ptr() + 4), (None, B.data_ptr()),
                   (A.data_ptr(), A.data_ptr())):
        assert lib().vag_swap_flat(pa, pb, n, stream()) == -22
    torch.cuda.synchronize()
    assert torch.equal(bits(A), bits(A0)) and torch.equal(bits(B), bits(B0))


# ------------------------------------------------------------------------------------------------------------------
# driver level
# ------------------------------------------------------------------------------------------------------------------
FIXTURES = ["text_tied_s0_f32", "mm_dot_tied_mid_f32"]


def _fixture(name):
    meta, P, z = load_golden(name)
    cm, cv = criteria(meta)
    return meta, P, cm, (cv if meta["kind"] == "mm" else None), _inputs(meta, z)


def _six_steps(meta, P, cm, cv, batch, use_graph, ema_decay, lr=4e-4, check=True):
    """Six steps, teacher alternating: two shapes of three visits each -- the first eager, the second captures, so at least two
    steps per shape are replays.  With check: fp.ema against the fp64 recurrence on the step's own fp.flat after every step."""
    from vagnmt_hip.trainer import TrainStep
    src, lens, tgt, im = batch
    m = build(meta, P)
    ts = TrainStep(m, cm, cv, lr=lr, use_graph=use_graph, capture_after=1, ema_decay=ema_decay)
    losses = []
    if ema_decay:
        e_ref, pmax = ts.fp.ema.double(), float(ts.fp.flat.abs().max())
        assert torch.equal(ts.fp.ema, ts.fp.flat)
    for i in range(6):
        out = ts.step(src, lens, tgt, im, teacher=(i % 2 == 0))
        losses.append(float(out[0].item()))
        if ema_decay and check:
            t = i + 1
            d = _d(t, ema_decay, True)
            assert d < 0.9                           # every one of the six is the warm-up's: a frozen d_t cannot pass
            e_ref = e_ref + (1.0 - d) * (ts.fp.flat.double() - e_ref)
            pmax = max(pmax, float(ts.fp.flat.abs().max()))
            err = float((ts.fp.ema.double() - e_ref).abs().max())
            print("%s graph=%s step %d: max |ema - fp64| = %.3e, bound %.3e" % (meta["kind"], use_graph, t, err, 6 * 2.0 ** -22 * pmax))
            assert err <= 6 * 2.0 ** -22 * pmax, (t, err)
    assert int(ts.step_count.item()) == 6 and ts.skipped_steps() == 0
    return m, ts, losses


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_six_steps_keep_the_average_and_change_nothing_else(name, use_graph):
    meta, P, cm, cv, batch = _fixture(name)
    m1, ts1, l1 = _six_steps(meta, P, cm, cv, batch, use_graph, 0.9)
    m0, ts0, l0 = _six_steps(meta, P, cm, cv, batch, use_graph, 0.0)
    assert ts0.fp.ema is None
    assert np.allclose(l1, l0, rtol=2e-4), (l1, l0)
    for (n, p1), (_, p0) in zip(m1.named_parameters(), m0.named_parameters()):
        close(p1, p0.detach().cpu().numpy(), 2e-4, "ema_decay 0.9 vs 0: " + n)
    assert ts1.stats["captures"] == ts0.stats["captures"]
    if use_graph:
        assert ts1.stats["captures"] >= 2 and ts1.stats["replays"] >= 4, ts1.stats
    else:
        assert ts1.stats["captures"] == 0


def _scores(m, meta, batch):
    src, lens, tgt, im = batch
    s = m.score_translations(src, lens, tgt, im) if meta["kind"] == "mm" else m.score_translations(src, lens, tgt)
    return s.token_logp.clone()


@pytest.mark.parametrize("name", FIXTURES)
def test_averaged_weights_block(name):
    meta, P, cm, cv, batch = _fixture(name)
    m, ts, _ = _six_steps(meta, P, cm, cv, batch, True, 0.9, lr=1e-2, check=False)
    fp = ts.fp
    flat0, ema0 = fp.flat.clone(), fp.ema.clone()
    bits = lambda t: t.view(torch.int32)              # noqa: E731
    ptrs = (fp.flat.data_ptr(), fp.ema.data_ptr())
    before = _scores(m, meta, batch)
    version = m._vag_weights_version
    with ts.averaged_weights() as inner:
        assert inner is ts and m._vag_weights_version > version
        assert torch.equal(bits(fp.flat), bits(ema0)) and torch.equal(bits(fp.ema), bits(flat0))
        inside = _scores(m, meta, batch)
        esd = ts.ema_state_dict()                     # (inside the block it still means the averaged weights)
        with pytest.raises(RuntimeError):
            ts.step(*batch, teacher=True)
        with pytest.raises(RuntimeError):
            ts.mrt_step(*batch)
        with pytest.raises(RuntimeError):
            with ts.averaged_weights():
                pass
        assert torch.equal(bits(fp.flat), bits(ema0))          # the refusals moved nothing
    after = _scores(m, meta, batch)
    assert torch.equal(before, after)
    assert torch.equal(bits(fp.flat), bits(flat0)) and torch.equal(bits(fp.ema), bits(ema0))
    assert (fp.flat.data_ptr(), fp.ema.data_ptr()) == ptrs
    # a fresh model loaded from ema_state_dict() scores what the block scored
    sd_out = ts.ema_state_dict()
    for k in esd:
        assert torch.equal(esd[k], sd_out[k]), k
    fresh = build(meta, esd)
    assert torch.equal(_scores(fresh, meta, batch), inside)
    assert not torch.equal(inside, before)
    # an exception inside the block still restores the raw weights
    with pytest.raises(KeyError):
        with ts.averaged_weights():
            raise KeyError("from the block")
    assert torch.equal(bits(fp.flat), bits(flat0)) and torch.equal(bits(fp.ema), bits(ema0))
    assert torch.equal(_scores(m, meta, batch), before)
    # training goes on from the captured graphs
    captures = ts.stats["captures"]
    out = ts.step(*batch, teacher=True)
    assert np.isfinite(float(out[0])) and ts.stats["captures"] == captures and int(ts.step_count.item()) == 7


# ------------------------------------------------------------------------------------------------------------------
# 7. resume
# ------------------------------------------------------------------------------------------------------------------
def test_resume_restores_the_average_in_place(tmp_path):
    from machine_translation_vision.losses import PairwiseRankingLoss
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    from vagnmt_hip.checkpoint import load_checkpoint, save_checkpoint
    from vagnmt_hip.trainer import TrainStep
    Vs, Vt, I, E, H, S, B, Ts, Tt = 90, 100, 64, 32, 48, 40, 6, 9, 7      # (test_checkpoint_resume_equivalence's model)

    def new_model(seed):
        torch.manual_seed(seed)
        return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, 0.99, dropout_ctx=0.5, dropout_emb=0.3,
                                                     dropout_out=0.5, tied_emb=True).cuda()

    def driver(m):
        return TrainStep(m, cm, PairwiseRankingLoss(0.1), use_graph=True, ema_decay=0.9)
    vw = torch.ones(Vt, device="cuda")
    vw[0] = 0
    cm = torch.nn.NLLLoss(weight=vw, reduction="none")
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(6):
        src = torch.randint(4, Vs, (B, Ts), generator=g)
        tgt = torch.randint(4, Vt, (B, Tt), generator=g)
        tgt[:, -1] = 3
        batches.append((src.cuda(), [Ts] * B, tgt.cuda(), torch.randn(B, I, generator=g).abs().cuda()))
    coins = [True, False, True, True, False, True]
    torch.manual_seed(11)
    m_a = new_model(0)
    ts_a = driver(m_a)
    for b, c in zip(batches, coins):
        ts_a.step(*b, teacher=c)
    torch.manual_seed(11)
    m_b = new_model(0)
    ts_b = driver(m_b)
    for b, c in zip(batches[:3], coins[:3]):
        ts_b.step(*b, teacher=c)
    path = str(tmp_path / "resume.pt")
    save_checkpoint(path, m_b, ts_b)
    torch.manual_seed(99)
    m_c = new_model(123)
    ts_c = driver(m_c)
    ts_c.step(*batches[0], teacher=True)          # the resumed driver already holds captured graphs with fp.ema's address
    ts_c.step(*batches[0], teacher=True)
    where = ts_c.fp.ema.data_ptr()
    load_checkpoint(path, m_c, ts_c)
    assert ts_c.fp.ema.data_ptr() == where
    assert torch.equal(ts_c.fp.ema, ts_b.fp.ema) and not torch.equal(ts_c.fp.ema, ts_c.fp.flat)
    for b, c in zip(batches[3:], coins[3:]):
        ts_c.step(*b, teacher=c)
    assert int(ts_c.step_count) == 6
    for (n, pa), (_, pc) in zip(m_a.named_parameters(), m_c.named_parameters()):
        assert (pa - pc).abs().max().item() <= 2e-5 * max(1.0, pa.abs().max().item()), n
    fa, fc = ts_a.fp, ts_c.fp
    for n, p in fa.named:
        o, k = fa.offsets[n], p.numel()
        ea, ec = fa.ema[o:o + k], fc.ema[fc.offsets[n]:fc.offsets[n] + k]
        assert (ea - ec).abs().max().item() <= 2e-5 * max(1.0, ea.abs().max().item()), n


# ------------------------------------------------------------------------------------------------------------------
# 8. fp16 storage: the derived weights are refreshed on the way out
# ------------------------------------------------------------------------------------------------------------------
def test_fp16_storage_step_after_an_averaged_block_equals_its_twin():
    """The shape of the 2-byte storage mode's tests (test_gpu_round3: H = 1024, B = 256).  Two steps at lr = 1e-2 without warm-up,
    so that the averaged weights lag the parameters visibly; then the third step's loss after an averaged_weights() block
    against a twin driver that never entered one, at that mode's tolerance (rtol 1e-3, atol 1e-4: test_wide_fp16_encoder_...).
    The fp16 copies of the weights that the step reads are derived data: left stale (= the averaged weights) the third step
    would run on other weights."""
    from test_gpu_round2 import _fp16_case
    from vagnmt_hip.trainer import TrainStep
    m_of, (src, lens, tgt, im), cm, cv = _fp16_case("wide")
    out = {}
    for block in (False, True):
        m = m_of()
        ts = TrainStep(m, cm, cv, lr=1e-2, use_graph=False, storage="f16", pad_src=1, ema_decay=0.9, ema_warmup=False)
        for _ in range(2):
            ts.step(src, lens, tgt, im, teacher=True)
        assert float((ts.fp.ema - ts.fp.flat).abs().max()) > 5e-3           # the two sets of weights are far apart
        if block:
            with ts.averaged_weights():
                torch.cuda.synchronize()
        out[block] = [float(x) for x in ts.step(src, lens, tgt, im, teacher=True)]
        assert ts.skipped_steps() == 0
    print("fp16 storage, third step: twin %s, after the block %s" % (out[False], out[True]))
    assert np.isfinite(out[True]).all()
    assert np.allclose(out[True], out[False], rtol=1e-3, atol=1e-4), out
