"""GPU: the decoder backward's hidden-side product dgh2[t] W_hh2 fed by bf16 planes only (persist.hip: dec_bwd_persistent_kernel,
bit 1 of the option "handoff_planes").

cell2_bwd publishes the dgh2 rows as planes beside the fp32 tensor, and every workgroup splits its W_hh2^T slice once per launch
into a region of its own in the caller's plane buffer.  The split is elementwise and the accumulation order is unchanged, so the
forms 0 (fp32 hand-off), 1 (hand-off planes) and 3 (hidden side too) must give the same bits: torch.equal on dgi2, dqgh, ds, dgi1,
dgh1, d_h0, d_enc, d_pe and every decoder weight gradient that is a product (the bias gradients and d attn_v are column sums
finished with atomics: see _colsum_bounds).  tests/test_gpu_handoff_planes.py explains why torch.equal is a fair
demand under its inputs and product options; its helpers build the inputs and the forward state here as well.  One thing more is
needed for the weight gradients: the target tokens are all different (as its source tokens are), so that the embedding scatter adds
once per row of its gradient.

Per shape the forward runs once and the backward five times (form 3 on a NaN-filled plane buffer, form 3 again on the same buffer,
form 1, form 0, form 3 with a buffer one float short of the query); the tests below only compare what those calls left.

The encoder FORWARD hands its state rows off as planes as well (enc_fwd_persistent_kernel, bit 2 of the option, only with a plane
buffer from the caller): enc, the saved states and the saved gates with bit 2 off and on, torch.equal -- nothing in that operator is
summed with atomics."""
import pytest
import torch

from test_gpu_handoff_planes import E, _buffers, _dec_layout, _dec_w, _enc_layout, _forward, _inputs, _planes

pytestmark = pytest.mark.gpu

# H, B, Ts, Tt: the H = 256 form, a partial tile | a second tile with one valid row, ragged lengths | full tiles at the workload's
# Ts (LDS tightest) | two passes of row tiles (rt0 != 0, the W_hh2^T regions are indexed by the block of the LAUNCH) | Tt = 1: only
# the call of cell2_bwd in front of the step loop publishes
SHAPES = [(256, 3, 5, 3), (512, 17, 7, 3), (512, 64, 40, 2), (512, 112, 4, 3), (512, 5, 3, 1)]
DEFAULT = 7
# Gradients that are products with the forward's contexts: the context-to-hidden projection (DecW.c2h) and gru_2's input weights.
# The forward runs on all-zero encoder states here (so that the backward's atomic d alpha sums are exact), its contexts are zero,
# and so may these two be; they are compared like the rest, only not required to hold something.
ZERO_BY_INPUT = ("grad07", "grad08")


def _handoff_floats(H, B, Tt):
    """floats of the dq and dgh1 blocks, the part of the decoder's buffer that form 1 uses (6 bytes per element of a 16-row tile)"""
    return Tt * ((B + 15) // 16) * 16 * 5 * H * 6 // 4


def _decoder_floats(H, B, Tt):
    """... and of the decoder's whole buffer: the dgh2 blocks and 8 x 3H elements for each workgroup of the widest launch a device
    of at most 256 CUs makes (H / 8 workgroups per row tile) follow.  vag_handoff_planes_floats answers the larger of this and the
    encoder's need."""
    RT, wgs = (B + 15) // 16, H // 8
    return _handoff_floats(H, B, Tt) + (Tt * RT * 16 * 3 * H + min(RT, 256 // wgs) * wgs * 8 * 3 * H) * 6 // 4


def _dec_backward(d, H, B, Ts, Tt, form, planes, bufs, fwd):
    """the decoder's backward recurrence and its weight-gradient products from the forward's state, with `planes` as the caller's
    plane buffer; the compared tensors, cloned"""
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import ptr
    from test_gpu_round3 import _dirty
    C = 2 * H
    out = {}
    L.set_option("handoff_planes", form)
    for name, value in (("gemm_force_tile", 128), ("gemm_force_splitk", 1), ("gemm_nogroup", 1)):
        L.set_option(name, value)
    try:
        ws = bufs["ws_dec"]
        ws.copy_(fwd["ws_dec"])
        hseq, h2 = fwd["hseq"], fwd["hseq"][1:]
        gd = [torch.zeros_like(x) for x in [d["emb_t"]] + d["dec"]]
        d_h2, d_c = d["d_h2_in"].clone(), d["d_c_in"].clone()
        d_keys, d_pe, d_h0 = _dirty(B, Ts, C), _dirty(B, Ts, C), _dirty(B, H)
        scratch = bufs["scratch"]
        with _planes(planes):
            L.call("vag_cgru_attn_decode_seq_bwd", ptr(d["keys"]), ptr(d["pe"]), ptr(d["mask"]), ptr(hseq[0]), ptr(d["tok"], torch.int64),
                   _dec_w(d["emb_t"], d["dec"]), B, Ts, Tt, E, H, d["Vt"], ptr(h2), ptr(fwd["c"]), ptr(fwd["e"]), ptr(d_h2), ptr(d_c),
                   ptr(d["d_e_in"]), ptr(ws), ptr(d_keys), 0, ptr(d_pe), ptr(d_h0), _dec_w(gd[0], gd[1:]), ptr(scratch), L.stream())
        lay, end = _dec_layout(B, Ts, Tt, H)
        assert end == scratch.numel()
        for name in ("dgi2", "dqgh", "ds", "dgi1", "dgh1"):
            o, n = lay[name]
            out[name] = scratch[o:o + n].clone()
        out["d_h0"], out["d_enc"], out["d_pe"] = d_h0, d_keys, d_pe
        for i, x in enumerate(gd):
            out["grad%02d" % i] = x
        torch.cuda.synchronize()
    finally:
        L.set_option("handoff_planes", DEFAULT)
        for name in ("gemm_force_tile", "gemm_force_splitk", "gemm_nogroup"):
            L.set_option(name, 0)
    return out


_CACHE = {}


def _case(shape):
    """every call of a shape, made once and left unchanged: name -> (outputs, the plane buffer's words that are not 0xFFFFFFFF in
    the hand-off part and in the hidden side's part)"""
    if shape in _CACHE:
        return _CACHE[shape]
    from vagnmt_hip import _lib as L
    H, B, Ts, Tt = shape
    d = _inputs(*shape)
    g = torch.Generator().manual_seed(77 + B)
    d["Vt"] = (Tt + 1) * B + 4                               # all target tokens different: one add per row of the embedding gradient
    d["tok"] = (torch.randperm((Tt + 1) * B, generator=g).view(Tt + 1, B) + 4).cuda()
    d["emb_t"] = ((torch.rand(d["Vt"], E, generator=g) * 2 - 1)).cuda()
    bufs = _buffers(*shape)
    L.lib().vag_persistent_timeouts()
    fwd = _forward(d, *shape, bufs)
    n, base, need = bufs["planes"].numel(), _handoff_floats(H, B, Tt), _decoder_floats(H, B, Tt)
    # the query covers the decoder's need; where the encoder's is larger (full tiles at Ts = 40, Tt = 2) "one float short" is taken
    # of the decoder's need, or the call would not be short of anything
    assert n == L.lib().vag_handoff_planes_floats(B, Ts, Tt, H) and base < need <= n
    assert need == n or shape == (512, 64, 40, 2)

    def run(form, planes):
        out = _dec_backward(d, H, B, Ts, Tt, form, planes, bufs, fwd)
        w = planes.view(torch.int32) != -1
        return out, int(w[:base].sum()), int(w[base:].sum())

    def fresh():
        return torch.full((n,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    res = {}
    res["3"] = run(3, bufs["planes"])                        # on a buffer full of NaN patterns
    res["3 again"] = run(3, bufs["planes"])                  # on the planes the first call left
    res["1"] = run(1, fresh())
    res["0"] = run(0, fresh())
    res["short"] = run(3, fresh()[:need - 1])
    assert L.lib().vag_persistent_timeouts() == 0
    _CACHE[shape] = res
    return res


def _colsum_bounds(out, H, B, Ts, Tt):
    """The bias gradients and d attn_v are COLUMN SUMS that colsum_kernel (gemm.hip) finishes with fp32 atomics, one add per group
    of rows: the order of those adds changes from run to run, with or without planes, so torch.equal is no fair demand on them (the
    sums formed with atomics are the one exception the module docstring of test_gpu_handoff_planes.py names).  Their ADDENDS are
    compared bit for bit (dgi1, dgh1, dgi2, dqgh, ds), and the sums themselves against the bound of a reordered fp32 sum of n
    addends x_i: any two orders differ by at most 2 (n - 1) 2^-24 sum |x_i|.  name -> that bound per column.
    d attn_v[c] = sum over (t, b, s) of ds[t, b, s] tanh(.): |addend| <= |ds|."""
    C, R, u = 2 * H, Tt * B, 2.0 ** -24
    rows = {"grad03": out["dgi1"].view(R, 3 * H), "grad04": out["dgh1"].view(R, 3 * H), "grad10": out["dgi2"].view(R, 3 * H),
            "grad11": out["dqgh"].view(R, 5 * H)[:, C:]}
    bounds = {name: 2 * (R - 1) * u * x.abs().double().sum(0) for name, x in rows.items()}
    bounds["grad06"] = (2 * (R * Ts - 1) * u * out["ds"].abs().double().sum()).expand(C)
    return bounds


def _same(a, b, what, shape):
    assert sorted(a) == sorted(b)
    differ = {name: int((a[name] != b[name]).sum()) for name in sorted(a)}
    for name in sorted(a):
        print("%-8s %-8s %9d values, %d differ, largest %.3e" % (what, name, a[name].numel(), differ[name], float(a[name].abs().max())))
    bounds = _colsum_bounds(a, *shape)
    for name in sorted(a):
        assert torch.isfinite(a[name]).all() and torch.isfinite(b[name]).all(), (what, name)
        if name in bounds:
            err = (a[name].double() - b[name].double()).abs().view(-1)
            print("%-8s %-8s column sums: largest difference %.3e, bound there %.3e" % (what, name, float(err.max()), float(bounds[name][err.argmax()])))
            assert bool((err <= bounds[name]).all()), (what, name, float(err.max()))
        else:
            assert torch.equal(a[name], b[name]), (what, name, differ[name])
        if name not in ZERO_BY_INPUT:
            assert float(a[name].abs().max()) > 0.0, (what, name)          # the comparison is not one of zeros


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_hidden_planes_give_the_bits_of_the_other_forms(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt))
    # the arms are what they say: form 3 wrote both parts of the buffer, form 1 the hand-off part alone, form 0 nothing
    assert res["3"][1] > 0 and res["3"][2] > 0
    assert res["1"][1] > 0 and res["1"][2] == 0
    assert res["0"][1] == 0 and res["0"][2] == 0
    _same(res["3"][0], res["1"][0], "3 vs 1", (H, B, Ts, Tt))
    _same(res["3"][0], res["0"][0], "3 vs 0", (H, B, Ts, Tt))


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_nothing_is_read_from_a_hidden_plane_slot_that_was_not_written(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt))
    first, second = res["3"][0], res["3 again"][0]
    for name in sorted(first):
        assert torch.isfinite(first[name]).all(), name          # the plane buffer was all NaN before that call
    _same(first, second, "again", (H, B, Ts, Tt))


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_a_buffer_one_float_short_keeps_the_hand_off_planes_alone(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt))
    out, handoff_words, hidden_words = res["short"]
    assert handoff_words > 0 and hidden_words == 0              # the call succeeded in the form of handoff_planes = 1
    _same(out, res["1"][0], "short", (H, B, Ts, Tt))


def _enc_forward(d, H, B, Ts, form, planes):
    """the encoder's forward recurrence with `planes` as the caller's plane buffer: enc, the saved states and gates, cloned"""
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import gru_w, ptr
    from test_gpu_round3 import _dirty
    L.set_option("handoff_planes", form)
    try:
        ws = _dirty(L.lib().vag_bigru_ws_floats(B, Ts, E, H))
        enc, msk = _dirty(B, Ts, 2 * H), _dirty(B, Ts)
        with _planes(planes):
            L.call("vag_bigru_seq_fwd", ptr(d["src"], torch.int64), ptr(d["lt"], torch.int32), ptr(d["emb_s"]), gru_w(*d["fw"]),
                   gru_w(*d["bw"]), 0.0, 0.0, None, B, Ts, E, H, ptr(enc), ptr(msk), ptr(ws), L.stream())
        torch.cuda.synchronize()
        lay, _ = _enc_layout(B, Ts, H)
        out = {"enc": enc, "mask": msk}
        for name in ("hst", "gates"):
            o, n = lay[name]
            out[name] = ws[o:o + n].clone()
    finally:
        L.set_option("handoff_planes", DEFAULT)
    return out


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES[:4])
def test_encoder_forward_state_planes_give_the_same_bits(H, B, Ts, Tt):
    from vagnmt_hip import _lib as L
    L.lib().vag_persistent_timeouts()
    assert L.lib().vag_recurrence_supported(0, B, Ts, Tt, H) == 1
    d = _inputs(H, B, Ts, Tt)
    n = L.lib().vag_handoff_planes_floats(B, Ts, Tt, H)
    used = 2 * Ts * ((B + 15) // 16) * 16 * H * 6 // 4          # [2][Ts][row tiles] blocks of 16 x H elements, 6 bytes each
    assert 0 < used <= n

    def fresh():
        return torch.full((n,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    buf = fresh()
    on = _enc_forward(d, H, B, Ts, 7, buf)                      # on a buffer full of NaN patterns
    assert int((buf.view(torch.int32)[:used] != -1).sum()) > 0 and int((buf.view(torch.int32)[used:] != -1).sum()) == 0
    again = _enc_forward(d, H, B, Ts, 7, buf)                   # on the planes the first call left
    off_buf = fresh()
    off = _enc_forward(d, H, B, Ts, 3, off_buf)
    assert int((off_buf.view(torch.int32) != -1).sum()) == 0    # the fp32 form left the buffer alone
    short = fresh()[:used - 1]
    cut = _enc_forward(d, H, B, Ts, 7, short)                   # a buffer too small: the fp32 form
    assert int((short.view(torch.int32) != -1).sum()) == 0
    assert L.lib().vag_persistent_timeouts() == 0
    for name in sorted(on):
        differ = int((on[name] != off[name]).sum())
        print("%-6s %9d values, %d differ, largest %.3e" % (name, on[name].numel(), differ, float(on[name].abs().max())))
    for name in sorted(on):
        assert torch.isfinite(on[name]).all(), name
        assert float(on[name].abs().max()) > 0.0, name
        assert torch.equal(on[name], off[name]), name
        assert torch.equal(on[name], again[name]), name
        assert torch.equal(on[name], cut[name]), name
