"""The four recurrence operators (vag_bigru_seq_fwd / _bwd, vag_cgru_attn_decode_seq_fwd / _bwd), the GRU cell, the decoding step and
the stand-alone attention through the C ABI (vagnmt_hip._lib.call / ptr / stream / set_option / gru_w / DecW), element by element
against the tracked float64 references of tests/recur_ref.py: |got - value| <= err, err carried by the reference itself (its docstring
derives every rule), nothing relative to a tensor's maximum.  tests/test_recur_ref_host.py shows on the CPU that the bounds hold for an
fp32 restatement of each operator and reject the defect catalogue, at exactly the cases below.
Storage covered here: storage 0; storage 1: test_gpu_storage16.py.

Buffers, as in test_gpu_ground_ops.py: every input is followed by NaN floats (index arrays by impossible indices), every output by a
sentinel tail that must come back bit-identical; outputs documented as written start as NaN; accumulated ones (every g_*, d_enc_out
under accumulate_enc = 1) start from random nonzero values that enter the reference; workspaces, scratch and the hand-off plane buffer
start with every byte 0xA5 and carry a tail of their own.  The backward's arguments h2_all, c_all, e_all are the device forward's own.
Beside the bounds, exactly: mask bit for bit; enc 0.0 past each row's length; e_all bit-equal to the gathered embedding rows; g_emb
row 0 and a row no token names bit-equal to their start; vag_dropout_mask word for word equal to the host restatement; _bwd_loop +
_bwd_weights under the same bounds as the one-call backward (two decoder cases); d_e_all = NULL (one case);
vag_persistent_timeouts() == 0 after every case.  Options are set inside a context manager whose exit restores the defaults
whatever happened; persist_spin_limit is never touched.

The decoder's forward is held to TWO references.  The free-running one (recur_ref.cgru_fwd) carries its own states from step to
step; its bound is sharp for a step or two and then passes the states' range (worst-case propagation through three products per
step).  The one-step one recomputes every step from the DEVICE's own previous state (cgru_fwd(h2_given = the device's h2_all)): its
bound is sharp at every step (below 1e-3 at all cases, asserted on the host), and it is what holds the workgroup-to-workgroup
hand-offs of steps 2, 3, ... -- a step that read a state one step late leaves it (catalogue: stale_h2_at_late_step).  The backward
has no such second reference, so its cases are short (Tt = 1 at H >= 512, <= 2 at H = 256, <= 3 below: recur_ref.DEC_CASES) and the
long cases run the forward only; at every backward case every catalogue defect leaves the bound.

Branch reached by each case (R.ENC_CASES / R.DEC_CASES carry the sentence per case; conditions quoted from the sources, 256 CUs):
  encoder chain      skinny.hip vag_gru_step_launch, nz = 2: `a.K > 256 && wgs <= maxwg` (160) -> gru_step_small_kernel: (512, B = 20) 128
                     workgroups, (1024, B = 16) 128; `a.M >= 128 && a.K > 256 && grid.x * cdiv64(a.M, 32) * nz >= 192` -> two row tiles
                     per workgroup: (512, B = 130), whose last 32-row tile holds rows 128, 129; else `a.K <= 256` -> gru_step_kernel<4>
                     (H = 32, 128, 256: the K = 256 edge) or gru_step_kernel<8> (512, B = 96: 384 workgroups).  Backward,
                     vag_gru_bwd_step_launch with K = 3H: `a.K <= 256` (96) | `<= 512` (384) | `<= 1024` (768) | `<= 1536` (1536) | else
                     (3072); `a.M >= 128 && a.K > 1024 && cdiv64(a.H, 32) * cdiv64(a.M, 32) * nz >= 256` -> the 2 x 2 wide kernel
                     (512, B = 130: 16 * 5 * 2 = 160: not taken; the cell case (256, 1024): 32 * 8 = 256: taken).
  encoder one launch persist.hip vag_enc_persistent_ok: `H == 256 || H == 512 || H == 1024`, passes_ok(cdiv64(B, 16), cus / (2 * (H / 16)), 2):
                     8 / 4 / 2 tiles per pass, a second pass `4 * last >= 3 * tpp` full: (256, 224) 8 + 6; (512, 100) 4 + 3, the last tile
                     with 4 rows; (1024, 64) 2 + 2.  enc_api.hip vag_bigru_seq_bwd: `(H == 512 || H == 256) && vag_enc_persistent_ok(B, Ts, H)`
                     -> H = 1024 runs the chain backward after the one-launch forward; "persistent_enc_bwd" = 0 does the same at 256.
                     `handoff_planes(vag_enc_bwd_planes_floats(B, Ts, H))`: NULL without a vag_set_handoff_planes buffer -> fp32 hand-off.
  decoder chain      skinny.hip vag_attn_dot_side_launch: `W % 512 == 0 && (W == 1024 || W == 1536 || W == 2048 || W == 3072)` ->
                     attn_dot_side_reg_kernel, NJ = W / 512; forward W = C = 2H: H = 512, 768, 1024, 1536 -> NJ = 2, 3, 4, 6; H = 32, 256
                     (C = 512) -> attn_dot_side_kernel, `d.gx = cdiv64(Ts, DS_WAVES)` = 2 at Ts = 9.  `gx = cdiv64(512, N)` clipped to
                     `Ts / (2 * WV)`: (512, B = 5, Ts = 33) -> 2 blocks, the second ragged.  `wide = M >= 128` (B = 130).  Backward W = 3H:
                     1536 and 3072 take the register kernel, 2304 and 4608 the generic one.  VAG_POST_CHUNKS(Ts) = ceil(Ts / 8): 1 (Ts <= 8),
                     2 (9), 3 (17), 5 (33), 7 (49).  Tt = 1: `t == 0` right after the last-step cell backward.
  decoder one launch persist.hip vag_dec_persistent_ok: `H != 512 && H != 256` refused, passes_ok(cdiv64(B, 16), cus / (H / 8), 2): 4 / 8 tiles
                     per pass; `dec_persistent_lds_bytes(Ts) <= 160 * 1024` <=> Ts <= 48 (R.DEC_MAX_TS, from the formula): Ts = 48 runs in
                     one launch, Ts = 49 reports unsupported and runs the chain.  "persistent_dec_bwd" = 0: chain backward on the
                     one-launch forward's workspace.
  cell               vag_gru_step_launch, nz = 1: (5, 64), (17, 256) kernel<4>; (20, 512) 64 workgroups -> small; (96, 512) 192 ->
                     kernel<8>; (130, 512): 32 * 5 = 160 < 192 -> kernel<8>, not the two-tile form.  Backward: above.

Largest |err| / bound per operator and output: fp32 restatement on the CPU (tests/test_recur_ref_host.py -s) | device (this file -s).
  bahdanau         alpha 0.009 | 0.011   ctx 0.006 | 0.006   scores 0.017 | 0.024
  bigru_bwd        g_b_hh 0.376 | 0.376   g_b_ih 0.326 | 0.326   g_emb 0.011 | 0.010   g_w_hh 0.041 | 0.041
                   g_w_ih 0.479 | 0.479
  bigru_fwd        enc 0.153 | 0.141
  cgru_bwd_H<=128  d_enc_out 0.004 | 0.003   d_h0 0.001 | 0.001   d_pe 0.003 | 0.004   g_attn_h 0.048 | 0.048
                   g_attn_v 0.001 | 0.001   g_b_hh1 0.002 | 0.002   g_b_hh2 0.011 | 0.009   g_b_ih1 0.002 | 0.002
                   g_b_ih2 0.019 | 0.015   g_c2h 0.006 | 0.006   g_emb 0.001 | 0.001   g_w_hh1 0.033 | 0.033
                   g_w_hh2 0.052 | 0.050   g_w_ih1 0.011 | 0.011   g_w_ih2 0.065 | 0.065
  cgru_bwd_H=256   d_enc_out 0.000 | 0.000   d_h0 0.000 | 0.000   d_pe 0.001 | 0.000   g_attn_h 0.002 | 0.002
                   g_attn_v 0.000 | 0.000   g_b_hh1 0.012 | 0.012   g_b_hh2 0.034 | 0.034   g_b_ih1 0.014 | 0.012
                   g_b_ih2 0.040 | 0.040   g_c2h 0.026 | 0.026   g_emb 0.000 | 0.000   g_w_hh1 0.343 | 0.343
                   g_w_hh2 0.429 | 0.429   g_w_ih1 0.144 | 0.144   g_w_ih2 0.406 | 0.406
  cgru_bwd_H>=512  d_enc_out 0.000 | 0.000   d_h0 0.000 | 0.000   d_pe 0.001 | 0.000   g_attn_h 0.041 | 0.041
                   g_attn_v 0.000 | 0.000   g_b_hh1 0.000 | 0.000   g_b_hh2 0.003 | 0.002   g_b_ih1 0.000 | 0.000
                   g_b_ih2 0.003 | 0.004   g_c2h 0.001 | 0.000   g_emb 0.000 | 0.000   g_w_hh1 0.001 | 0.001
                   g_w_hh2 0.026 | 0.026   g_w_ih1 0.002 | 0.001   g_w_ih2 0.016 | 0.016
  cgru_fwd         c_all 0.006 | 0.003   h2_all 0.020 | 0.019
  cgru_fwd_step    c_all 0.006 | 0.004   h2_all 0.021 | 0.019
  cgru_step        alpha 0.006 | 0.003   c 0.006 | 0.004   h_out 0.008 | 0.006
  gru_cell_bwd     carry_out 0.421 | 0.081   dgh 0.374 | 0.078   dgi 0.374 | 0.080
  gru_cell_fwd     h_out 0.122 | 0.125   save 0.334 | 0.193
(cgru_fwd: against the free-running reference, all steps of all cases -- its late steps are inside bounds that no longer say anything,
its figure is set by step 0.  cgru_fwd_step: against the one-step reference, sharp at every step.  cgru_bwd by width, because the
backward's lengths differ by width: Tt <= 3, <= 2 and 1.  The encoder and the cells sit at a tenth to a half of their bounds, device
and restatement alike; the decoder's attention path at a hundredth: a worst-case bound widens by sum|w| ~ sqrt(K) / 2 at each of the
products a decoder step puts in a row, and rounding errors do not line up that way.)
Wall time of this file on an MI355X: 12.9 s for its 84 cases, the float64 references included (no case above 2.1 s)."""
import functools

import numpy as np
import pytest
import torch

import recur_ref as R
from recur_ref import T

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e9
DEV = "cuda:0"
TAIL = 64
WORST = {}


def _L():
    from vagnmt_hip import _lib
    return _lib


def _in(x, dtype=torch.float32):
    """A host array on the device followed by TAIL NaN floats (index arrays: TAIL copies of an impossible index)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    pad = torch.full((TAIL,), float("nan")) if dtype == torch.float32 else torch.full((TAIL,), -(2 ** 30), dtype=dtype)
    buf = torch.cat([t.to(dtype), pad]).to(DEV)
    return buf[:t.numel()]


class _Out:
    """An output buffer of `shape`: NaN (written) or `start` (accumulated / consumed), then a sentinel tail."""

    def __init__(self, shape, start=None):
        n = int(np.prod(shape))
        body = torch.full((n,), float("nan")) if start is None else torch.from_numpy(np.ascontiguousarray(start)).reshape(-1).clone()
        self.sent = torch.full((TAIL,), SENTINEL)
        self.buf = torch.cat([body, self.sent]).to(DEV)
        self.view, self.n, self.shape = self.buf[:n], n, tuple(shape)

    def host(self, what, tag):
        out = self.buf.cpu()
        assert torch.equal(out[self.n:], self.sent), ("write past " + what, tag)
        return out[:self.n].view(self.shape).numpy()


class _Ws:
    """A workspace of n floats whose every byte is 0xA5 (counters read 2779096485, floats -2.9e-16), tail included."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.empty(self.n + TAIL, dtype=torch.float32, device=DEV)
        self.buf.view(torch.uint8).fill_(0xA5)
        self.view = self.buf[:self.n]

    def check(self, what, tag):
        assert bool((self.buf[self.n:].view(torch.uint8) == 0xA5).all()), ("write past " + what, tag)


def _check(op, what, out, ref, tag):
    got = out.host(what, tag) if isinstance(out, _Out) else out
    assert np.isfinite(got).all(), (what, "non-finite (a read outside an input, or an output that was never written)", tag)
    q = R.ratio(got, ref)
    WORST[(op, what)] = max(WORST.get((op, what), 0.0), q)
    print("%-16s %-10s %-40s |err|/bound %.3f" % (op, what, tag, q))
    assert q <= 1.0, (op, what, tag, "worst |err| / bound %.3g" % q)
    return got


def _sync():
    torch.cuda.synchronize()


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


class _options:
    """`with _options(persistent=0, ...)`: set, and restore the defaults (all 1) whatever happens."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _L().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            _L().set_option(k, 1)
        _L().call("vag_set_handoff_planes", None, 0)
        return False


def _planes(floats, tag):
    """The caller's buffer for the hand-off planes, named for this thread (restored by _options.__exit__)."""
    if floats <= 0:
        return None
    buf = _Ws(floats)
    _L().call("vag_set_handoff_planes", _L().ptr(buf.view), buf.n)
    return buf


def _rng():
    return torch.tensor(list(R.RNG_STATE), dtype=torch.int64, device=DEV)         # two uint64 words (both below 2^63)


def _no_timeouts(tag):
    assert _L().lib().vag_persistent_timeouts() == 0, ("a wait of a one-launch kernel gave up", tag)


def _case_id(c):
    return "-".join(str(x) for x in c[:-1] if x is not None).replace(" ", "")


# ---------------------------------------------------------------------------------------------------------------- cells
@pytest.mark.parametrize("M,H", R.CELL_FWD_CASES, ids=lambda x: str(x))
def test_gru_cell_fwd_matches_fp64_per_element(M, H):
    L = _L()
    inp = R.cell_inputs(M, H)
    gi, hp, w, b = _in(inp["gi"]), _in(inp["h_prev"]), _in(inp["w_hh"]), _in(inp["b_hh"])
    h_out, save = _Out((M, H)), _Out((4, M, H))
    L.call("vag_gru_cell_fwd", L.ptr(gi), L.ptr(hp), L.ptr(w), L.ptr(b), M, H, L.ptr(h_out.view), L.ptr(save.view), L.stream())
    _sync()
    ref = R.cell_fwd(T, inp)
    _check("gru_cell_fwd", "h_out", h_out, ref["h_out"], (M, H))
    _check("gru_cell_fwd", "save", save, ref["save"], (M, H))


@pytest.mark.parametrize("M,H", R.CELL_BWD_CASES, ids=lambda x: str(x))
def test_gru_cell_bwd_matches_fp64_per_element(M, H):
    L = _L()
    inp = R.cell_inputs(M, H)
    gi, hp, w, b = _in(inp["gi"]), _in(inp["h_prev"]), _in(inp["w_hh"]), _in(inp["b_hh"])
    h_out, save = _Out((M, H)), _Out((4, M, H))
    L.call("vag_gru_cell_fwd", L.ptr(gi), L.ptr(hp), L.ptr(w), L.ptr(b), M, H, L.ptr(h_out.view), L.ptr(save.view), L.stream())
    dgn, wt, carry, d_out = _in(inp["dgh_next"]), _in(inp["w_hh"].T), _in(inp["carry"]), _in(inp["d_out"])
    dgi, dgh, co = _Out((M, 3 * H)), _Out((M, 3 * H)), _Out((M, H))
    L.call("vag_gru_cell_bwd", L.ptr(dgn), L.ptr(wt), L.ptr(carry), L.ptr(d_out), L.ptr(save.view), L.ptr(hp), M, H, L.ptr(dgi.view),
           L.ptr(dgh.view), L.ptr(co.view), L.stream())
    _sync()
    ref = R.gru_cell_bwd(T, inp, save.host("save", (M, H)))               # the device forward's own gates: exact arguments
    for k, o in (("dgi", dgi), ("dgh", dgh), ("carry_out", co)):
        _check("gru_cell_bwd", k, o, ref[k], (M, H))


# ---------------------------------------------------------------------------------------------------------------- encoder
ENC_G = ["w_ih", "w_hh", "b_ih", "b_hh"]


@functools.lru_cache(maxsize=None)
def _enc_ref(key):
    inp = R.enc_inputs(*key)
    fwd = R.bigru_fwd(T, inp)
    return fwd, R.bigru_bwd(T, inp, fwd)


@pytest.mark.parametrize("case", R.ENC_CASES, ids=_case_id)
def test_bigru_seq_matches_fp64_per_element(case):
    L = _L()
    H, E, B, Ts = case.H, case.E, case.B, case.Ts
    key = R.enc_key(case)
    inp = R.enc_inputs(*key)
    tag = _case_id(case)
    sup = L.lib().vag_recurrence_supported(0, B, Ts, 1, H)
    if case.one_launch:
        assert sup == 1, tag
    opts = dict(persistent=case.one_launch)
    if case.opt:
        opts[case.opt] = 0
    drop = case.p_emb > 0 or case.p_ctx > 0
    rng = _rng() if drop else None
    src, lens, emb = _in(inp["src"], torch.int64), _in(inp["lens"], torch.int32), _in(inp["emb"])
    fw, bw = [_in(x) for x in inp["fw"]], [_in(x) for x in inp["bw"]]
    enc, mask = _Out((B, Ts, 2 * H)), _Out((B, Ts))
    d_enc = _Out((B, Ts, 2 * H), inp["d_enc"])
    g_emb = _Out((R.ENC_VS, E), inp["g_emb0"])
    g_fw = [_Out(x.shape, x) for x in inp["g_fw0"]]
    g_bw = [_Out(x.shape, x) for x in inp["g_bw0"]]
    ws = _Ws(L.lib().vag_bigru_ws_floats(B, Ts, E, H))
    with _options(**opts):
        planes = _planes(L.lib().vag_handoff_planes_floats(B, Ts, 1, H), tag) if (case.planes and case.one_launch) else None
        if "hand-off planes" in case.branch:
            assert planes is not None, tag
        if drop:
            for which, m, p in ((1, inp["m_emb"], case.p_emb), (2, inp["m_ctx"], case.p_ctx)):
                got = _Out((m.size,))
                L.call("vag_dropout_mask", L.ptr(rng, torch.int64), which, m.size, p, L.ptr(got.view), L.stream())
                _sync()
                assert _bits(got.host("mask", tag), m.reshape(-1)), ("vag_dropout_mask differs from the host restatement", which, tag)
        L.call("vag_bigru_seq_fwd", L.ptr(src, torch.int64), L.ptr(lens, torch.int32), L.ptr(emb), L.gru_w(*fw), L.gru_w(*bw),
               case.p_emb, case.p_ctx, L.ptr(rng, torch.int64), B, Ts, E, H, L.ptr(enc.view), L.ptr(mask.view), L.ptr(ws.view), L.stream())
        L.call("vag_bigru_seq_bwd", L.ptr(src, torch.int64), L.ptr(lens, torch.int32), L.gru_w(*fw), L.gru_w(*bw), case.p_emb, case.p_ctx,
               L.ptr(rng, torch.int64), B, Ts, E, H, L.ptr(d_enc.view), L.ptr(ws.view), L.ptr(g_emb.view),
               L.gru_w(*[g.view for g in g_fw]), L.gru_w(*[g.view for g in g_bw]), L.stream())
        _sync()
        _no_timeouts(tag)
    ws.check("ws", tag)
    if planes is not None:
        planes.check("hand-off planes", tag)
    d_enc.host("d_enc", tag)                                                 # consumed: only its extent is promised
    fwd, bwd = _enc_ref(key)
    assert _bits(mask.host("mask", tag), fwd["mask"]), ("mask", tag)
    e32 = _check("bigru_fwd", "enc", enc, fwd["enc"], tag)
    for b, n in enumerate(inp["lens"]):
        assert (e32[b, n:] == 0.0).all(), ("enc past the length of row %d" % b, tag)
    got = _check("bigru_bwd", "g_emb", g_emb, bwd["g_emb"], tag)
    for r in (0, R.ENC_NEVER):
        assert _bits(got[r], inp["g_emb0"][r]), ("g_emb row %d was written" % r, tag)
    for name, gs in (("fw", g_fw), ("bw", g_bw)):
        for k, o in zip(ENC_G, gs):
            _check("bigru_bwd", "g_" + k, o, bwd["g_%s_%s" % (name, k)], tag + "/" + name)


# ---------------------------------------------------------------------------------------------------------------- decoder
@functools.lru_cache(maxsize=None)
def _dec_fwd_ref(key):
    return R.cgru_fwd(T, R.dec_inputs(*key))


def _dec_w(L, emb, p):
    return L.DecW(L.ptr(emb), L.gru_w(*p[0:4]), L.ptr(p[4]), L.ptr(p[5]), L.ptr(p[6]), L.gru_w(*p[7:11]))


def _dec_run(case, two_phase):
    L = _L()
    H, E, B, Ts, Tt = case.H, case.E, case.B, case.Ts, case.Tt
    C = 2 * H
    key = R.dec_key(case)
    inp = R.dec_inputs(*key)
    tag = _case_id(case) + ("/two-phase" if two_phase else "")
    sup = L.lib().vag_recurrence_supported(1, B, Ts, Tt, H)
    if case.one_launch:
        assert sup == 1, tag
    if Ts == R.DEC_MAX_TS + 1:
        assert sup == 0 and L.lib().vag_recurrence_supported(1, B, R.DEC_MAX_TS, Tt, H) == 1, tag
    opts = dict(persistent=1 if (case.one_launch or Ts == R.DEC_MAX_TS + 1) else 0)
    if case.opt:
        opts[case.opt] = 0
    enc, pe, mask, h0 = _in(inp["enc"]), _in(inp["pe"]), _in(inp["mask"]), _in(inp["h0"])
    tok, emb = _in(inp["tok"], torch.int64), _in(inp["emb"])
    names = R.DEC_W_NAMES[1:]
    wts = [_in(inp["w"][n]) for n in names]
    h2, c_all, e_all = _Out((Tt, B, H)), _Out((Tt, B, C)), _Out((Tt, B, E))
    ws = _Ws(L.lib().vag_cgru_ws_floats(B, Ts, Tt, E, H))
    scratch = _Ws(L.lib().vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H))
    d_h2, d_c = _Out((Tt, B, H), inp["d_h2"]), _Out((Tt, B, C), inp["d_c"])
    d_e = _in(inp["d_e"]) if case.d_e else None
    d_enc = _Out((B, Ts, C), inp["d_enc0"] if case.acc else None)
    d_pe, d_h0 = _Out((B, Ts, C)), _Out((B, H))
    g_emb = _Out((R.DEC_VT, E), inp["g_emb0"])
    gs = [_Out(inp["g0"][n].shape, inp["g0"][n]) for n in names]
    W = _dec_w(L, emb, wts)
    G = _dec_w(L, g_emb.view, [g.view for g in gs])
    with _options(**opts):
        planes = _planes(L.lib().vag_handoff_planes_floats(B, Ts, Tt, H), tag) if (case.planes and case.one_launch) else None
        if "hand-off planes" in case.branch:
            assert planes is not None, tag
        L.call("vag_cgru_attn_decode_seq_fwd", L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H,
               R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(ws.view), 0, None, 0.0, None, None, None, 0, L.stream())
        common = (L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H, R.DEC_VT, L.ptr(h2.view),
                  L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_h2.view), L.ptr(d_c.view), L.ptr(d_e), L.ptr(ws.view), L.ptr(d_enc.view),
                  case.acc, L.ptr(d_pe.view), L.ptr(d_h0.view))
        if case.fwd_only:
            pass
        elif two_phase:
            L.call("vag_cgru_attn_decode_seq_bwd_loop", *common, L.ptr(scratch.view), L.stream())
            L.call("vag_cgru_attn_decode_seq_bwd_weights", L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H, L.ptr(h2.view),
                   L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_e), L.ptr(ws.view), G, L.ptr(scratch.view), L.stream())
        else:
            L.call("vag_cgru_attn_decode_seq_bwd", *common, G, L.ptr(scratch.view), L.stream())
        _sync()
        _no_timeouts(tag)
    ws.check("ws", tag)
    scratch.check("scratch", tag)
    if planes is not None:
        planes.check("hand-off planes", tag)
    d_h2.host("d_h2_all", tag)                                               # consumed: only their extent is promised
    d_c.host("d_c_all", tag)
    fwd = _dec_fwd_ref(key)
    h2_32 = _check("cgru_fwd", "h2_all", h2, fwd["h2_all"], tag)
    c32 = _check("cgru_fwd", "c_all", c_all, fwd["c_all"], tag)
    e32 = e_all.host("e_all", tag)
    assert _bits(e32, inp["emb"][inp["tok"][:Tt]]), ("e_all is not the gathered embedding rows", tag)
    # the one-step reference: every step recomputed from the device's OWN previous state, a bound that stays sharp at every step --
    # what holds the hand-offs of steps 2, 3, ... where the free-running bound above has long passed the states' range
    rec = R.cgru_fwd(T, inp, h2_given=h2_32)
    _check("cgru_fwd_step", "h2_all", h2_32, rec["h2_all"], tag)
    _check("cgru_fwd_step", "c_all", c32, rec["c_all"], tag)
    if case.fwd_only:
        assert np.isnan(d_pe.host("d_pe", tag)).all(), tag                     # (no backward was run)
        return
    op = "cgru_bwd" + R.dec_group(H)
    bwd = R.cgru_bwd(T, inp, rec, c32, e32, case.acc, case.d_e)
    _check(op, "d_enc_out", d_enc, bwd["d_enc_out"], tag)
    _check(op, "d_pe", d_pe, bwd["d_pe"], tag)
    _check(op, "d_h0", d_h0, bwd["d_h0"], tag)
    got = _check(op, "g_emb", g_emb, bwd["g_emb"], tag)
    for r in (0, R.DEC_NEVER):
        assert _bits(got[r], inp["g_emb0"][r]), ("g.emb row %d was written" % r, tag)
    for n, o in zip(names, gs):
        _check(op, "g_" + n, o, bwd["g_" + n], tag)


@pytest.mark.parametrize("case", R.DEC_CASES, ids=_case_id)
def test_cgru_attn_decode_seq_matches_fp64_per_element(case):
    _dec_run(case, False)


@pytest.mark.parametrize("case", [c for c in R.DEC_CASES if c.two_phase], ids=_case_id)
def test_cgru_bwd_loop_then_weights_satisfies_the_one_call_bounds(case):
    _dec_run(case, True)


# ---------------------------------------------------------------------------------------------------------------- step, attention
@pytest.mark.parametrize("H,rps", R.STEP_CASES, ids=lambda x: str(x))
def test_cgru_attn_decode_step_matches_fp64_per_element(H, rps):
    L = _L()
    inp = R.step_inputs(H, rps)
    E, B, Ts = R.step_e(H), R.STEP_B, R.STEP_TS
    N, C = B * rps, 2 * H
    enc, pe, mask = _in(inp["enc"]), _in(inp["pe"]), _in(inp["mask"])
    tok, h_in, emb = _in(inp["tok1"], torch.int64), _in(inp["h_in"]), _in(inp["emb"])
    wts = [_in(inp["w"][n]) for n in R.DEC_W_NAMES[1:]]
    W = _dec_w(L, emb, wts)
    prep = _Ws(L.lib().vag_cgru_prep_floats(H))
    scratch = _Ws(L.lib().vag_cgru_step_scratch_floats(N, Ts, E, H))
    h_out, c, e, alpha = _Out((N, H)), _Out((N, C)), _Out((N, E)), _Out((N, Ts))
    L.call("vag_cgru_prepare", W, H, L.ptr(prep.view), L.stream())
    L.call("vag_cgru_attn_decode_step", L.ptr(enc), L.ptr(pe), L.ptr(mask), rps, L.ptr(tok, torch.int64), L.ptr(h_in), W, L.ptr(prep.view),
           N, Ts, E, H, L.ptr(h_out.view), L.ptr(c.view), L.ptr(e.view), L.ptr(alpha.view), L.ptr(scratch.view), L.stream())
    _sync()
    tag = (H, rps)
    prep.check("prep", tag)
    scratch.check("scratch", tag)
    ref = R.cgru_step(T, inp, rps)
    for k, o in (("h_out", h_out), ("c", c), ("alpha", alpha)):
        _check("cgru_step", k, o, ref[k], tag)
    assert _bits(e.host("e", tag), ref["e"]), tag


@pytest.mark.parametrize("H,rps,Ts", R.ATTN_CASES, ids=lambda x: str(x))
def test_bahdanau_attn_fwd_matches_fp64_per_element(H, rps, Ts):
    L = _L()
    inp = R.attn_inputs(H, rps, Ts)
    N, C = 2 * rps, 2 * H
    pe, q, v, mask, enc = _in(inp["pe"]), _in(inp["q"]), _in(inp["v"]), _in(inp["mask"]), _in(inp["enc"])
    scores, alpha, ctx = _Out((N, Ts)), _Out((N, Ts)), _Out((N, C))
    L.call("vag_bahdanau_attn_fwd", L.ptr(pe), L.ptr(q), L.ptr(v), L.ptr(mask), L.ptr(enc), N, rps, Ts, C, L.ptr(scores.view),
           L.ptr(alpha.view), L.ptr(ctx.view), L.stream())
    _sync()
    tag = (H, rps, Ts)
    ref = R.bahdanau_attn(T, inp, rps)
    on = np.repeat(inp["mask"], rps, axis=0) != 0
    s32 = scores.host("scores", tag)                                        # (a masked score is the kernel's own stand-in for -inf)
    _check("bahdanau", "scores", s32[on], R.TV(ref["scores"].v[on], ref["scores"].e[on]), tag)
    a32 = _check("bahdanau", "alpha", alpha, ref["alpha"], tag)
    assert (a32[~on] == 0).all(), ("weight on a masked position", tag)
    _check("bahdanau", "ctx", ctx, ref["ctx"], tag)


def test_zz_report_worst_ratios():
    """Runs last in this file: the largest |err| / bound per operator and output on the device (shown with -s)."""
    for op, what in sorted(WORST):
        print("device worst |err| / bound  %-16s %-12s %.3f" % (op.replace(" ", "_"), what, WORST[(op, what)]))
