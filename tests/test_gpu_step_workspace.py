"""A training step must not depend on what its workspace held before (step.hip: vag_train_step on FusedStep's one static
workspace, torch.empty-allocated and reused across batch shapes by fused.py: reserve).

The split-K tickets are the last region of the workspace, so their offset moves with (B, Ts, Tt); the step's prologue launch
zeroes them, and the slab form of split-K (gemm.hip: GemmArgs::slab) relies on that.  The multimodal image projection of the
forward pass (VSE_Imagine_Enc.py: im -> S) is a product over K = I = 2048 that leaves the skinny kernels at B > 256; without tanh
(activation_vse = False) it may split.  Whether the planner splits it onto slabs depends on (S, I), so gemm_force_tile = 128 with
gemm_force_splitk = 4 forces that path.

Multimodal V11 models small enough for the float64 CPU oracle (E = H = S = 64, a few hundred words, Ts, Tt <= 8, I = 2048),
teacher-forced steps through TrainStep's fused backend, losses and every gradient against oracle/vag_oracle.py at the
tolerances of test_gpu_edge_and_full.py::run_both, and against a fresh driver at the same shape within the run-to-run bound of
test_gpu_round5.py::test_run_to_run_spread_of_one_cfg2_step_is_bounded."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

Vs, Vt, I, E, H, S, Ts, Tt = 300, 280, 2048, 64, 64, 64, 8, 7
SEQUENCE = (320, 288, 260, 64)
FORCED = {"gemm_force_tile": 128, "gemm_force_splitk": 4}
TOL, GTOL = 1e-4, 3e-4              # run_both: losses relative, gradients relative to the largest entry of the tensor
SPREAD_L, SPREAD_G = 1e-6, 3e-5     # run-to-run spread of one step (losses, gradients)


def _L():
    from vagnmt_hip import _lib
    return _lib


class _Opts:
    """vag_set_option for the duration of a test; every option set here is put back to its default in the finally."""
    DEFAULTS = {"gemm_force_tile": 0, "gemm_force_splitk": 0, "step_fork": 0}

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _L().set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.DEFAULTS.items():
            _L().set_option(k, v)
        return False


def _cpu_model(act):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(23)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, 0.99, activation_vse=act, tied_emb=True).eval()


def _driver(act):
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip.trainer import TrainStep
    m = _cpu_model(act).cuda()
    vw = torch.ones(Vt, device="cuda")
    vw[0] = 0
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), use_graph=False, pad_src=1)
    m.eval()
    return m, ts


def _batch(B):
    g = torch.Generator().manual_seed(B)
    lens = sorted([int(x) for x in torch.randint(1, Ts + 1, (B,), generator=g)], reverse=True)
    lens[0] = Ts
    src = torch.zeros(B, Ts, dtype=torch.long)
    for b, n in enumerate(lens):
        src[b, :n] = torch.randint(4, Vs, (n,), generator=g)
    tgt = torch.randint(4, Vt, (B, Tt), generator=g)
    tgt[:, -1] = 3
    tgt[-1, 2] = 3
    tgt[-1, 3:] = 0
    im = torch.randn(B, I, generator=g).abs()
    return src, lens, tgt, im


_ORACLE = {}


def _oracle(act, B):
    """float64 losses and gradients of the step (cached: the same model and batch serve several tests)."""
    if (act, B) not in _ORACLE:
        from oracle import vag_oracle as O
        src, lens, tgt, im = _batch(B)
        leaves = {n: p.detach().double().clone().requires_grad_(True) for n, p in _cpu_model(act).named_parameters()}
        out = O.model_forward(leaves, src, lens, tgt, im.double(), teacher=True, activation=act)
        out["loss"].backward()
        grads = {n: (v.grad if v.grad is not None else torch.zeros_like(v)) for n, v in leaves.items()}
        _ORACLE[(act, B)] = ([float(out[k].detach()) for k in ("loss", "loss_mt", "loss_vse")], grads)
    return _ORACLE[(act, B)]


def _dev_batch(B):
    src, lens, tgt, im = _batch(B)
    return src.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), tgt.cuda(), im.cuda()


def _step(m, ts, B, poison=False):
    """One teacher-forced forward + backward (phases 7, no optimiser) at batch size B; (losses, gradients)."""
    src, lt, tgt, im = _dev_batch(B)
    if poison:
        _poison(ts, B)
    ts.fp.grad.zero_()
    ts.backend.run(src, lt, tgt, im, True, 7)
    torch.cuda.synchronize()
    f = ts.backend.f
    need = int(_L().lib().vag_step_ws_floats(C.byref(f.cfg(B, Ts, Tt, True))))
    assert int(f.ws.view(torch.int32)[need - 16384:need].abs().max()) == 0, B      # every ticket zeroed, or put back by its tile
    return [float(x) for x in ts.backend.outputs()], {n: p._vag_grad.detach().double().cpu() for n, p in m.named_parameters()}


def _poison(ts, B):
    """After reserve: NaN in the float regions vag_step_ws_offset names (0-3, 5-7) and in the split-K slabs, small non-zero
    integers (what a stale ticket looks like) in the ticket region.  The int64 token matrix (offset 8) and every other region
    the code reads as an index keep their contents."""
    f = ts.backend.f
    f.reserve(B, Ts, Tt)
    cfg = f.cfg(B, Ts, Tt, True)
    lib = _L().lib()
    need = int(lib.vag_step_ws_floats(C.byref(cfg)))
    C2 = 2 * H
    extents = {0: B * Ts * C2, 1: B * Ts, 2: (Tt + 1) * B * H, 3: Tt * B * cfg.ldl, 5: B * Ts * C2, 6: B * S, 7: B * S}
    ws = f.ws
    for which, n in extents.items():
        o = int(lib.vag_step_ws_offset(C.byref(cfg), which))
        assert 0 <= o and o + n <= need
        ws[o:o + n] = float("nan")
    # the slab region lies right before the 16384 tickets (step.hip: step_ws, fp32 storage): 12 x the widest activation,
    # rounded up to 64 floats like every region of the workspace
    R = Tt * B
    widest = max(B * Ts * C2, R * 3 * H, 3 * H * C2, R * E)
    slab = (min(12 * widest, 192 << 20) + 63) // 64 * 64
    ws[need - 16384 - slab:need - 16384] = float("nan")
    tick = ws.view(torch.int32)[need - 16384:need]
    tick.copy_(torch.arange(16384, device=ws.device, dtype=torch.int32) % 3 + 1)


def _check(tag, got, want):
    (gl, gg), (wl, wg) = got, want
    for a, b in zip(gl, wl):
        assert abs(a - b) <= TOL * max(1.0, abs(b)), (tag, gl, wl)
    for n, ref in wg.items():
        err = (gg[n] - ref).abs().max().item()
        assert err <= GTOL * max(ref.abs().max().item(), 1e-3), (tag, n, err, ref.abs().max().item())


def _same_run(tag, got, fresh):
    (gl, gg), (fl, fg) = got, fresh
    for a, b in zip(gl, fl):
        assert abs(a - b) <= SPREAD_L * max(1.0, abs(b)), (tag, gl, fl)
    for n, ref in fg.items():
        err = (gg[n] - ref).abs().max().item()
        assert err <= SPREAD_G * max(ref.abs().max().item(), 1e-12), (tag, n, err)


@pytest.mark.parametrize("forced", [False, True], ids=["planner", "forced_slabs"])
@pytest.mark.parametrize("act", [False, True], ids=["linear_vse", "tanh_vse"])
def test_step_after_other_shapes_matches_oracle_and_a_fresh_driver(act, forced):
    """One driver runs B = 320, 288, 260, 64 (the workspace is sized by the first shape and never reallocated after it): each step
    matches the oracle, and a fresh driver at the same shape within the run-to-run spread."""
    with _Opts(**(FORCED if forced else {})):
        m, ts = _driver(act)
        f = ts.backend.f
        got = {}
        for i, B in enumerate(SEQUENCE):
            got[B] = _step(m, ts, B)
            if i == 0:
                ptr0, gen0 = f.ws.data_ptr(), f.generation
            assert f.ws.data_ptr() == ptr0 and f.generation == gen0, ("workspace reallocated", B)
        del m, ts
        for B in SEQUENCE:
            _check(("stale", act, forced, B), got[B], _oracle(act, B))
            m, ts = _driver(act)
            _same_run(("stale vs fresh", act, forced, B), got[B], _step(m, ts, B))
            del m, ts


@pytest.mark.parametrize("forced", [False, True], ids=["planner", "forced_slabs"])
@pytest.mark.parametrize("act", [False, True], ids=["linear_vse", "tanh_vse"])
def test_step_on_a_poisoned_workspace_matches_oracle(act, forced):
    """NaN in the named float regions and the slabs, stale-looking tickets: the step's own zeroing and writes must cover
    everything it reads (B = 320: the image projection goes through vag_gemm_launch)."""
    with _Opts(**(FORCED if forced else {})):
        m, ts = _driver(act)
        _check(("poisoned", act, forced), _step(m, ts, 320, poison=True), _oracle(act, 320))


@pytest.mark.parametrize("bit", [1, 2, 4])
def test_step_fork_branches_with_forced_slabs_match_oracle(bit):
    """step_fork bits 1 (image projection beside the encoder), 2 (held-back leaves beside the encoder's backward) and 4 (the
    decoder's weight gradients on the side stream), one at a time, with every splittable product forced onto slabs: a launch
    on the side stream must not share the main stream's slabs and tickets."""
    with _Opts(step_fork=bit, **FORCED):
        m, ts = _driver(False)
        _check(("step_fork", bit), _step(m, ts, 288, poison=True), _oracle(False, 288))
