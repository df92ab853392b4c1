"""GPU: the backward recurrences' hand-off rows as bf16 planes (persist.hip: st_planes4 / ld_planes_sc1, option "handoff_planes").

The producer of a handed-off row splits it once into the three bf16 planes every consumer used to derive for itself; the split is
elementwise, so both forms must give the same bits.  Three properties, on the operators called one by one (raw workspaces, as
test_gpu_round3.py::test_standalone_recurrences_zero_their_own_counters does):
 1. handoff_planes = 0 against 1 on the same inputs: torch.equal on the encoder's d_xp and dgh, its embedding and weight
    gradients, and on the decoder's dgi2, dqgh, ds, dgi1, dgh1, d_h0, d_enc, d_pe;
 2. plane buffers full of NaN patterns before the first call: finite outputs, and a second call on the same buffers gives the
    same bits (a slot that is read but never written would show);
 3. the model with planes on against the launch chains and against the fp64 oracle, with the bounds test_gpu_round6.py uses.

What makes torch.equal a fair demand here: everything between the inputs and the compared tensors is deterministic EXCEPT sums
formed with fp32 atomics, whose order changes from run to run.  The inputs are chosen so that those sums are exact:
 * the decoder's forward adds its scores with atomics as well -- it runs ONCE per shape, and every backward call starts from the
   workspace it left;
 * the decoder's d alpha accumulator (phase A: 16 workgroups add into one word) -- the forward call is given all-zero encoder
   states, so the projected keys and with them every addend are zero, while the backward call is given real ones, so that the
   head's share of d alpha (a plain product), ds, dq and everything behind them are ordinary numbers;
 * the encoder's embedding scatter -- the source tokens are all different, one add per row of the gradient;
 * the products run one by one and unsplit (gemm_nogroup, gemm_force_tile / gemm_force_splitk): no split-K partial sums meet in
   memory."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# H, B, Ts, Tt: one partial tile | a second tile with one valid row, ragged lengths | full tiles at the workload's Ts (the decoder's
# LDS is tightest there) | two passes of row tiles (rt0 != 0)
SHAPES = [(256, 3, 5, 3), (512, 17, 7, 3), (512, 64, 40, 2), (512, 112, 4, 3)]
E = 32


def _r64(n):
    return (n + 63) // 64 * 64


def _layout(regions):
    """name -> (offset, size) of regions carved one after the other on 64-float boundaries (kernels.h: WsCarver), and the end"""
    out, off = {}, 0
    for name, n in regions:
        out[name] = (off, n)
        off += _r64(n)
    return out, off


def _enc_layout(B, Ts, H):
    return _layout([("x", Ts * B * E), ("xp", Ts * B * 6 * H), ("hst", 2 * (Ts + 1) * B * H), ("gates", 2 * Ts * 4 * B * H),
                    ("dgh", 2 * Ts * B * 3 * H), ("carry", 4 * B * H), ("dx", Ts * B * E), ("whhT", 6 * H * H), ("gx", 3 * Ts * B * H)])


def _dec_layout(B, Ts, Tt, H):
    C, R = 2 * H, Tt * B
    Q = C + 3 * H
    return _layout([("wcatT", Q * H), ("wpT", 3 * H * C), ("whh1T", 3 * H * H), ("dgi2", R * 3 * H), ("dqgh", R * Q), ("dalpha", B * Ts),
                    ("ds", R * Ts), ("dgi1", R * 3 * H), ("dgh1", R * 3 * H), ("dh1d", B * H), ("carry", B * H), ("de", R * E),
                    ("dvp", (Ts + 7) // 8 * B * C), ("dwp", 3 * H * C), ("dah", R * Ts), ("dencwp", B * Ts * 3 * H), ("pbuf", B * H),
                    ("u_all", R * H), ("du_all", R * H), ("duk", B * Ts * H)])


class _planes:
    """`with _planes(buf):` -- the caller's buffer for the hand-off planes (vag_set_handoff_planes) for the calls inside"""
    def __init__(self, buf):
        self.buf = buf

    def __enter__(self):
        from vagnmt_hip import _lib as L
        L.call("vag_set_handoff_planes", L.ptr(self.buf), self.buf.numel())

    def __exit__(self, *exc):
        from vagnmt_hip import _lib as L
        L.call("vag_set_handoff_planes", None, 0)
        return False


def _inputs(H, B, Ts, Tt):
    C = 2 * H
    Vs, Vt = B * Ts + 4, 60
    g = torch.Generator().manual_seed(1000 * H + B)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).cuda()

    def gru(inp):
        k = H ** -0.5
        return [rnd(3 * H, inp, scale=k), rnd(3 * H, H, scale=k), rnd(3 * H, scale=k), rnd(3 * H, scale=k)]
    lens = sorted([int(x) for x in torch.randint(1, Ts + 1, (B,), generator=g)], reverse=True)
    lens[0] = Ts
    if B > 2:
        lens[-1] = min(lens[-1], Ts - 1)          # some len < Ts whatever the draw
    perm = torch.randperm(B * Ts, generator=g).view(B, Ts) + 4      # all different: the embedding scatter adds once per row
    src = torch.zeros(B, Ts, dtype=torch.long)
    mask = torch.zeros(B, Ts)
    for b, n in enumerate(lens):
        src[b, :n] = perm[b, :n]
        mask[b, :n] = 1
    d = {"lens": lens, "src": src.cuda(), "lt": torch.tensor(lens, dtype=torch.int32, device="cuda"), "mask": mask.cuda(), "Vs": Vs, "Vt": Vt}
    d["emb_s"], d["fw"], d["bw"] = rnd(Vs, E), gru(E), gru(E)
    d["d_enc_in"] = rnd(B, Ts, C)
    d["keys"] = rnd(B, Ts, C, scale=0.5) * d["mask"].unsqueeze(-1)
    d["pe"] = (d["keys"] @ rnd(C, C, scale=C ** -0.5).t()).contiguous()
    d["h0"] = rnd(B, H, scale=0.5)
    tok = torch.randint(4, Vt, (Tt + 1, B), generator=g)
    tok[0] = 2
    d["tok"] = tok.cuda()
    d["emb_t"] = rnd(Vt, E)
    d["dec"] = gru(E) + [rnd(C, H, scale=H ** -0.5), rnd(C, scale=C ** -0.5), rnd(H, C, scale=C ** -0.5)] + gru(H)
    d["d_h2_in"], d["d_c_in"], d["d_e_in"] = rnd(Tt, B, H), rnd(Tt, B, C), rnd(Tt, B, E)
    return d


def _buffers(H, B, Ts, Tt):
    """workspaces with every byte 0xA5 (test_gpu_round3._dirty) and a plane buffer full of 0xFF: every bf16 there is a NaN"""
    from vagnmt_hip import _lib as L
    from test_gpu_round3 import _dirty
    bufs = {"ws_enc": _dirty(L.lib().vag_bigru_ws_floats(B, Ts, E, H)), "ws_dec": _dirty(L.lib().vag_cgru_ws_floats(B, Ts, Tt, E, H)),
            "scratch": _dirty(L.lib().vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H))}
    n = L.lib().vag_handoff_planes_floats(B, Ts, Tt, H)
    assert n > 0
    bufs["planes"] = torch.empty(n, dtype=torch.float32, device="cuda")
    bufs["planes"].view(torch.uint8).fill_(0xFF)
    return bufs


def _dec_w(emb, p):
    from vagnmt_hip._lib import DecW, gru_w, ptr
    return DecW(ptr(emb), gru_w(*p[0:4]), ptr(p[4]), ptr(p[5]), ptr(p[6]), gru_w(*p[7:11]))


def _forward(d, H, B, Ts, Tt, bufs):
    """Both forward recurrences, ONCE per shape: the decoder's forward adds its scores with atomics too, so two forward calls
    do not leave the same attention weights.  Returns what the backward calls start from (the workspaces as the forward left them)."""
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import gru_w, ptr
    from test_gpu_round3 import _dirty
    C = 2 * H
    assert L.lib().vag_recurrence_supported(0, B, Ts, Tt, H) == 1 and L.lib().vag_recurrence_supported(1, B, Ts, Tt, H) == 1
    st = L.stream
    enc, msk = _dirty(B, Ts, C), _dirty(B, Ts)
    L.call("vag_bigru_seq_fwd", ptr(d["src"], torch.int64), ptr(d["lt"], torch.int32), ptr(d["emb_s"]), gru_w(*d["fw"]), gru_w(*d["bw"]),
           0.0, 0.0, None, B, Ts, E, H, ptr(enc), ptr(msk), ptr(bufs["ws_enc"]), st())
    hseq = _dirty(Tt + 1, B, H)
    hseq[0].copy_(d["h0"])
    h2, c, e = hseq[1:], _dirty(Tt, B, C), _dirty(Tt, B, E)
    zero_keys = torch.zeros_like(d["keys"])          # zero projected keys, so the backward's atomic d alpha sums are exact
    L.call("vag_cgru_attn_decode_seq_fwd", ptr(zero_keys), ptr(d["pe"]), ptr(d["mask"]), ptr(hseq[0]), ptr(d["tok"], torch.int64),
           _dec_w(d["emb_t"], d["dec"]), B, Ts, Tt, E, H, d["Vt"], ptr(h2), ptr(c), ptr(e), ptr(bufs["ws_dec"]), 0, None, 0.0, None, None,
           None, 0, st())
    torch.cuda.synchronize()
    return {"ws_enc": bufs["ws_enc"].clone(), "ws_dec": bufs["ws_dec"].clone(), "hseq": hseq, "c": c, "e": e}


def _backward(d, H, B, Ts, Tt, planes, bufs, fwd):
    """Both backward recurrences from the forward's state; the tensors the issue names, cloned.  The plane buffer of `bufs` is left as
    it is (NaN patterns in a fresh one, the previous call's planes otherwise)."""
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import gru_w, ptr
    from test_gpu_round3 import _dirty
    C = 2 * H
    st = L.stream
    out = {}
    L.set_option("handoff_planes", planes)
    for name, value in (("gemm_force_tile", 128), ("gemm_force_splitk", 1), ("gemm_nogroup", 1)):
        L.set_option(name, value)
    try:
        ws = bufs["ws_enc"]
        ws.copy_(fwd["ws_enc"])                               # (the backward writes d_xp over the forward's input projections)
        fw, bw = d["fw"], d["bw"]
        ge = [torch.zeros_like(x) for x in [d["emb_s"]] + fw + bw]
        d_enc = d["d_enc_in"].clone()
        with _planes(bufs["planes"]):
            L.call("vag_bigru_seq_bwd", ptr(d["src"], torch.int64), ptr(d["lt"], torch.int32), gru_w(*fw), gru_w(*bw), 0.0, 0.0, None,
                   B, Ts, E, H, ptr(d_enc), ptr(ws), ptr(ge[0]), gru_w(*ge[1:5]), gru_w(*ge[5:9]), st())
        lay, end = _enc_layout(B, Ts, H)
        sync = _r64(2 * ((B + 15) // 16) * Ts + 64)           # the mirror of the carver above is the library's layout: the two
        assert end + 2 * sync == ws.numel()                   # counter regions follow
        for name in ("xp", "dgh"):
            o, n = lay[name]
            out["enc_d_xp" if name == "xp" else "enc_dgh"] = ws[o:o + n].clone()
        for i, x in enumerate(ge):
            out["enc_grad%d" % i] = x

        ws = bufs["ws_dec"]
        ws.copy_(fwd["ws_dec"])
        hseq, h2 = fwd["hseq"], fwd["hseq"][1:]
        gd = [torch.zeros_like(x) for x in [d["emb_t"]] + d["dec"]]
        d_h2, d_c = d["d_h2_in"].clone(), d["d_c_in"].clone()
        d_keys, d_pe, d_h0 = _dirty(B, Ts, C), _dirty(B, Ts, C), _dirty(B, H)
        scratch = bufs["scratch"]
        with _planes(bufs["planes"]):
            L.call("vag_cgru_attn_decode_seq_bwd", ptr(d["keys"]), ptr(d["pe"]), ptr(d["mask"]), ptr(hseq[0]), ptr(d["tok"], torch.int64),
                   _dec_w(d["emb_t"], d["dec"]), B, Ts, Tt, E, H, d["Vt"], ptr(h2), ptr(fwd["c"]), ptr(fwd["e"]), ptr(d_h2), ptr(d_c),
                   ptr(d["d_e_in"]), ptr(ws), ptr(d_keys), 0, ptr(d_pe), ptr(d_h0), _dec_w(gd[0], gd[1:]), ptr(scratch), st())
        lay, end = _dec_layout(B, Ts, Tt, H)
        assert end == scratch.numel()
        for name in ("dgi2", "dqgh", "ds", "dgi1", "dgh1"):
            o, n = lay[name]
            out["dec_" + name] = scratch[o:o + n].clone()
        out["dec_d_h0"], out["dec_d_enc"], out["dec_d_pe"] = d_h0, d_keys, d_pe
        torch.cuda.synchronize()
    finally:
        L.set_option("handoff_planes", 1)
        for name in ("gemm_force_tile", "gemm_force_splitk", "gemm_nogroup"):
            L.set_option(name, 0)
    return out


_CACHE = {}


def _planes_on(shape):
    """the forward state of a shape and its planes-on backward on NaN-filled plane buffers, computed once for the tests below and
    left unchanged"""
    if shape not in _CACHE:
        d, bufs = _inputs(*shape), _buffers(*shape)
        fwd = _forward(d, *shape, bufs)
        _CACHE[shape] = (d, bufs, fwd, _backward(d, *shape, 1, bufs, fwd))
    return _CACHE[shape]


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_planes_and_fp32_hand_off_give_the_same_bits(H, B, Ts, Tt):
    from vagnmt_hip import _lib as L
    L.lib().vag_persistent_timeouts()
    d, bufs_on, fwd, on = _planes_on((H, B, Ts, Tt))
    bufs_off = _buffers(H, B, Ts, Tt)
    off = _backward(d, H, B, Ts, Tt, 0, bufs_off, fwd)
    # the two arms are what they say: the planes form wrote the caller's buffer, the fp32 form left it alone
    assert int((bufs_on["planes"].view(torch.int32) != -1).sum()) > 0
    assert int((bufs_off["planes"].view(torch.int32) != -1).sum()) == 0
    assert L.lib().vag_persistent_timeouts() == 0
    assert sorted(on) == sorted(off)
    differ = {name: int((on[name] != off[name]).sum()) for name in sorted(on)}
    for name in sorted(on):
        print("%-14s %9d values, %d differ, largest %.3e" % (name, on[name].numel(), differ[name], float(on[name].abs().max())))
    for name in sorted(on):
        assert torch.isfinite(on[name]).all(), name
        assert torch.equal(on[name], off[name]), (name, differ[name])
        assert float(on[name].abs().max()) > 0.0, name              # the comparison is not one of zeros


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_nothing_is_read_from_a_plane_slot_that_was_not_written(H, B, Ts, Tt):
    from vagnmt_hip import _lib as L
    L.lib().vag_persistent_timeouts()
    d, bufs, fwd, first = _planes_on((H, B, Ts, Tt))
    for name in sorted(first):
        assert torch.isfinite(first[name]).all(), name          # the plane buffers were all NaN before that call
    second = _backward(d, H, B, Ts, Tt, 1, bufs, fwd)           # the same buffers again, now holding the first call's planes
    assert L.lib().vag_persistent_timeouts() == 0
    for name in sorted(first):
        assert torch.equal(first[name], second[name]), (name, int((first[name] != second[name]).sum()))


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES[:2])
def test_model_with_planes_against_launch_chains_and_oracle(H, B, Ts, Tt):
    """Bounds of test_gpu_round6.py for the same comparisons: against the chains, losses 2e-6 and every gradient 2e-5 of its tensor's
    largest entry (test_wider_persistent_decoder_equals_launch_chain); against the oracle, losses 1e-4, gradients 3e-4 of the largest
    entry and 2e-4 relative L2 (test_two_pass_recurrences_match_the_oracle: test_gpu_benched_path._check)."""
    from test_gpu_round3 import _model, _batch
    from test_gpu_benched_path import _oracle, _check
    from vagnmt_hip import _lib as L
    from vagnmt_hip.trainer import TrainStep
    from machine_translation_vision.losses import PairwiseRankingLoss
    assert L.lib().vag_recurrence_supported(1, B, Ts, Tt, H) == 1 and L.lib().vag_recurrence_supported(0, B, Ts, 1, H) == 1
    src, lens, tgt, im = _batch(B, Ts, Tt, seed=3)
    vw = torch.ones(333, device="cuda")
    vw[0] = 0
    crit = torch.nn.NLLLoss(weight=vw, reduction="none")
    res = {}
    L.lib().vag_persistent_timeouts()
    for mode in (0, 1):
        L.set_option("persistent", mode)
        try:
            m = _model(H, seed=2)
            loss, loss_mt, _ = m(src, lens, tgt, im, 1.0, criterion_mt=crit, criterion_vse=PairwiseRankingLoss(0.1))
            loss.backward()
            torch.cuda.synchronize()
            res[mode] = (float(loss), float(loss_mt), {n: p.grad.detach().clone() for n, p in m.named_parameters()})
        finally:
            L.set_option("persistent", 1)
    (l0, m0, g0), (l1, m1, g1) = res[0], res[1]
    assert L.lib().vag_persistent_timeouts() == 0
    assert np.isfinite(l1)
    assert abs(l0 - l1) <= 2e-6 * max(1.0, abs(l0)), (l0, l1)
    assert abs(m0 - m1) <= 2e-6 * max(1.0, abs(m0)), (m0, m1)
    for n in g0:
        scale = max(g0[n].abs().max().item(), 1e-3)
        err = (g0[n] - g1[n]).abs().max().item()
        assert err <= 2e-5 * scale, (n, err, scale)
    # the fused step (planes on) against the fp64 oracle
    m = _model(H, seed=2)
    ts = TrainStep(m, crit, PairwiseRankingLoss(margin=0.1), use_graph=False, pad_src=1)
    m.eval()
    lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ts.backend.run(src, lt, tgt, im, True, 7)
    torch.cuda.synchronize()
    assert L.lib().vag_persistent_timeouts() == 0
    losses = [float(x) for x in ts.backend.outputs()]
    grads = {n: p._vag_grad.detach().clone() for n, p in m.named_parameters()}
    want_l, want_g = _oracle(m, (src, lens, tgt, im))
    _check("planes H=%d B=%d" % (H, B), losses, grads, want_l, want_g)
