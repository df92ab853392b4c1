"""The attention energies' hoisted form on the device (csrc/common.h: vag_energy_exp / vag_energy_tanh; dec_fwd_persistent_kernel's
scores, dec_bwd_persistent_kernel's phase B, attn_post_bwd_kernel).

(a) vag_attn_energy_probe on the grid of tests/energy_ref.py (every pair of ~330 log-spaced values of both signs, zeros and
    denormals with |a|, |b| <= 39, and the cancelling pairs (a, -a +- delta), delta = 2^-20 .. 4) against float64 tanh(a + b): every
    element within TANH_ABS = 2^-20 (tests/ground_ref.py), every result in [-1, 1]; beyond the domain, up to 1e4 and +-inf: finite, in
    [-1, 1], the sign right wherever the clamped operands cannot cancel.  This holds the device's own v_exp_f32 / v_rcp_f32 to the
    bound directly -- a score is a sum of C energies whose bound is wider than any one energy's error.
(b) vag_cgru_attn_decode_seq_fwd / _bwd through the C ABI at shapes the one-launch kernels take, (H, B, Ts, Tt) = (256, 3, 5, 3),
    (512, 17, 7, 2) -- two row tiles, the second partial; an odd Ts for the parity halves of phase B -- and (512, 5, 48, 2), the
    largest Ts one launch holds (the backward there runs in one launch where its own LDS need allows, else as the chain; the
    post-pass is the same kernel either way).  The backward runs at the lengths tests/recur_ref.py uses at those widths (Tt <= 2
    at H = 256, 1 at H = 512).  References: recur_ref.cgru_fwd in its one-step form (every step from the device's own previous
    state) and recur_ref.cgru_bwd on it, each output element by element inside the reference's own bound.  Two input scalings:
    recur_ref's, and one with the keys and attn_h scaled so that |pe| and |q| reach 15 - 25 with both signs (asserted), which puts
    energies with large cancelling operands into every sum.  Outputs: alpha (the workspace slot vag_cgru_ws_offset names), c_all,
    h2_all; d_pe, g_attn_v, g_attn_h, d_enc_out (and d_h0).  vag_persistent_timeouts() == 0 after each case; buffers NaN-tailed and
    sentinel-tailed as in tests/test_gpu_recurrences.py, whose helpers this file uses.
(c) the post-pass at Ts = 8, 9 and 17 -- one, two and three chunks of VAG_POST_SC = 8 positions, the last one partial -- through the
    same operator path at H = 256, Tt = 2, both scalings, against the same reference."""
import functools

import numpy as np
import pytest
import torch

import energy_ref as E
import ground_ref as G
import recur_ref as R
import test_gpu_recurrences as TR
from recur_ref import T

pytestmark = pytest.mark.gpu

DEV = TR.DEV
EMB = 64


# ---------------------------------------------------------------------------------------------------------------- (a) the probe
def _probe(a, b):
    L = TR._L()
    n = a.size
    da, db, out = TR._in(a), TR._in(b), TR._Out((n,))
    L.call("vag_attn_energy_probe", L.ptr(da), L.ptr(db), n, L.ptr(out.view), L.stream())
    torch.cuda.synchronize()
    return out.host("probe", n).astype(np.float64)


def test_probe_is_within_the_tanh_bound_on_the_whole_grid():
    a, b = E.grid()
    assert a.size >= 100000 and a.size % 256 != 0                      # (a partial last block)
    got = _probe(a, b)
    err = np.abs(got - E.reference(a, b))
    k = int(err.argmax())
    print("probe: worst %.3f of TANH_ABS at (%r, %r), %d pairs" % (err[k] / G.TANH_ABS, a[k], b[k], a.size))
    assert np.isfinite(got).all()
    assert (np.abs(got) <= 1.0).all()
    assert (err <= G.TANH_ABS).all(), (a[k], b[k], err[k] / G.TANH_ABS, int((err > G.TANH_ABS).sum()))


def test_probe_saturates_outside_the_domain():
    a, b, sign = E.outside()
    got = _probe(a, b)
    assert np.isfinite(got).all()
    assert (np.abs(got) <= 1.0).all()
    asked = sign != 0
    assert (np.sign(got[asked]) == sign[asked]).all()


def test_probe_rejects_bad_arguments():
    L = TR._L()
    x = torch.zeros(4, device=DEV)
    assert L.lib().vag_attn_energy_probe(None, L.ptr(x), 4, L.ptr(x), L.stream()) == -22
    assert L.lib().vag_attn_energy_probe(L.ptr(x), L.ptr(x), 0, L.ptr(x), L.stream()) == -22


# ---------------------------------------------------------------------------------------------------------------- (b), (c) the operators
FWD_SHAPES = [(256, 3, 5, 3), (512, 17, 7, 2), (512, 5, 48, 2)]
POST_SHAPES = [(256, 3, 8, 2), (256, 3, 9, 2), (256, 3, 17, 2)]        # (c): 1, 2, 3 chunks of VAG_POST_SC


def _bwd_len(H, Tt):
    return min(Tt, 2 if H == 256 else 1)                                # recur_ref.DEC_CASES: the backward's lengths by width


CASES = [(H, B, Ts, Tt, False) for (H, B, Ts, Tt) in FWD_SHAPES] + \
        [(H, B, Ts, _bwd_len(H, Tt), True) for (H, B, Ts, Tt) in FWD_SHAPES] + \
        [(H, B, Ts, Tt, True) for (H, B, Ts, Tt) in POST_SHAPES]
BIG_LO, BIG_HI, BIG_AIM = 15.0, 25.0, 20.0


@functools.lru_cache(maxsize=None)
def _inputs(H, B, Ts, Tt, big):
    inp = R.dec_inputs(H, EMB, B, Ts, Tt)
    if not big:
        return inp
    # keys: uniform in +-0.5 -> +-20.  attn_h: by what brings the largest |q| of the unscaled model (fp32 restatement) to 20; the
    # scaled model's own q is asserted below
    q1 = max(float(np.abs(np.asarray(st["q"])).max()) for st in R.cgru_fwd(R.F, inp)["steps"])
    pe = (inp["pe"] * np.float32(2.0 * BIG_AIM)).astype(np.float32)
    attn_h = (inp["w"]["attn_h"] * np.float32(BIG_AIM / q1)).astype(np.float32)
    return dict(inp, pe=pe, w=dict(inp["w"], attn_h=attn_h))


def _reaches(x, what, tag):
    x = np.asarray(x, dtype=np.float64)
    assert BIG_LO <= x.max() <= BIG_HI and -BIG_HI <= x.min() <= -BIG_LO, (what, x.min(), x.max(), tag)


@pytest.mark.parametrize("big", [False, True], ids=["unit", "big"])
@pytest.mark.parametrize("H,B,Ts,Tt,bwd", CASES, ids=lambda x: str(x))
def test_decoder_operators_with_hoisted_energies(H, B, Ts, Tt, bwd, big):
    L = TR._L()
    lib = L.lib()
    C = 2 * H
    inp = _inputs(H, B, Ts, Tt, big)
    tag = "%d-%d-%d-%d-%s-%s" % (H, B, Ts, Tt, "bwd" if bwd else "fwd", "big" if big else "unit")
    assert lib.vag_recurrence_supported(1, B, Ts, Tt, H) == 1, tag
    enc, pe, mask, h0 = TR._in(inp["enc"]), TR._in(inp["pe"]), TR._in(inp["mask"]), TR._in(inp["h0"])
    tok, emb = TR._in(inp["tok"], torch.int64), TR._in(inp["emb"])
    names = R.DEC_W_NAMES[1:]
    wts = [TR._in(inp["w"][n]) for n in names]
    h2, c_all, e_all = TR._Out((Tt, B, H)), TR._Out((Tt, B, C)), TR._Out((Tt, B, EMB))
    ws = TR._Ws(lib.vag_cgru_ws_floats(B, Ts, Tt, EMB, H))
    scratch = TR._Ws(lib.vag_cgru_bwd_scratch_floats(B, Ts, Tt, EMB, H))
    d_h2, d_c, d_e = TR._Out((Tt, B, H), inp["d_h2"]), TR._Out((Tt, B, C), inp["d_c"]), TR._in(inp["d_e"])
    d_enc, d_pe, d_h0 = TR._Out((B, Ts, C)), TR._Out((B, Ts, C)), TR._Out((B, H))
    g_emb = TR._Out((R.DEC_VT, EMB), inp["g_emb0"])
    gs = [TR._Out(inp["g0"][n].shape, inp["g0"][n]) for n in names]
    W = TR._dec_w(L, emb, wts)
    Gd = TR._dec_w(L, g_emb.view, [g.view for g in gs])
    lib.vag_persistent_timeouts()
    with TR._options(persistent=1):
        planes = TR._planes(lib.vag_handoff_planes_floats(B, Ts, Tt, H), tag)
        L.call("vag_cgru_attn_decode_seq_fwd", L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, EMB, H,
               R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(ws.view), 0, None, 0.0, None, None, None, 0, L.stream())
        if bwd:
            L.call("vag_cgru_attn_decode_seq_bwd", L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, EMB,
                   H, R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_h2.view), L.ptr(d_c.view), L.ptr(d_e),
                   L.ptr(ws.view), L.ptr(d_enc.view), 0, L.ptr(d_pe.view), L.ptr(d_h0.view), Gd, L.ptr(scratch.view), L.stream())
        torch.cuda.synchronize()
        TR._no_timeouts(tag)
    ws.check("ws", tag)
    scratch.check("scratch", tag)
    if planes is not None:
        planes.check("hand-off planes", tag)
    h2_32 = h2.host("h2_all", tag)
    assert np.isfinite(h2_32).all(), tag
    rec = R.cgru_fwd(T, inp, h2_given=h2_32)                  # one-step form: every step from the device's own previous state
    if big:
        _reaches(inp["pe"], "pe", tag)
        _reaches(np.stack([st["q"].v for st in rec["steps"]]), "q", tag)
    op = "energy_" + ("big" if big else "unit")
    TR._check(op, "h2_all", h2_32, rec["h2_all"], tag)
    c32 = TR._check(op, "c_all", c_all, rec["c_all"], tag)
    off = lib.vag_cgru_ws_offset(B, Ts, Tt, EMB, H, 0)
    alpha = ws.view[off:off + Tt * B * Ts].cpu().numpy().reshape(Tt, B, Ts)
    TR._check(op, "alpha", alpha, R.cgru_ws_arrays(T, rec)["ws_alpha"], tag)
    if not bwd:
        return
    e32 = e_all.host("e_all", tag)
    ref = R.cgru_bwd(T, inp, rec, c32, e32, 0, True)
    for what, o in (("d_pe", d_pe), ("d_enc_out", d_enc), ("d_h0", d_h0), ("g_attn_v", gs[names.index("attn_v")]),
                    ("g_attn_h", gs[names.index("attn_h")])):
        TR._check(op, what, o, ref[what], tag)
