"""The 2-byte storage mode (vag_set_operator_context(derived, 1)) operator by operator through the C ABI, element by element against the
tracked float64 references of tests/recur_ref.py with storage = 1: |got - value| <= err, err carried by the reference (its docstring
derives the mode's rules: fp16 store or operand, the 2^12-scaled gradient operand, two-plane products), nothing relative to a tensor's
maximum.  tests/test_storage16_ref_host.py shows on the CPU that the bounds hold for the restatement and reject the mode's defect
catalogue at exactly these cases.  tests/test_gpu_recurrences.py is the same at storage 0; its helpers (_in, _Out, _Ws) are reused.

Covered here: vag_derive_weights(with_fp16 = 1), vag_attn_keys_proj, vag_bigru_seq_fwd / _bwd (launch chain and the wide one-launch
kernels), vag_cgru_attn_decode_seq_fwd / _bwd (teacher forced: the launch chain is the mode's only path) and the mode's rejections.

The decoder's forward takes `pe` from vag_attn_keys_proj on the device, in the mode: its fp16 bits enter the reference as exact data
(and are themselves held to the keys reference).  It is held to the free-running reference (cases of up to three steps) and to the
one-step reference -- every step recomputed from the device's OWN previous state -- on h2_all, c_all and on what the step left in the
workspace (vag_cgru_ws_offset: alpha, h1, q): the mode's worst-case softmax bound lets a query formed from the wrong state through on
alpha, its bound on q does not.  The decoder's backward, like the encoder's (below), is held to the reference from the workspace the
device's own forward saved (g1, g2, h1, alpha, q, uk and the fp16 encwp: layout restated from seq_layout.h and checked against
vag_cgru_ws_offset; each saved tensor is itself held to the one-step forward reference).  Its cases are the forward's short shapes at
the lengths at which every catalogue defect leaves the bound (R.DEC16_BWD_CASES: Tt = 3, 2, 2, 1, 1); variants: accumulate_enc both
ways, d_e_all = NULL once, _bwd_loop + _bwd_weights once.

Buffers as in test_gpu_recurrences.py: NaN tails behind inputs, sentinel tails behind outputs, accumulated outputs start from random
values that enter the reference, workspaces and the derived buffer start with every byte 0xA5.  The mode is set inside `_mode`, whose
exit always calls vag_set_operator_context(None, 0) and puts every option back: the context is sticky per thread.  persist_spin_limit
is never touched; vag_persistent_timeouts() == 0 after every case.

The encoder's backward is held to recur_ref.bigru_bwd(fwd = bigru_saved(gates, hst)): the gates and states the device's forward left in
the workspace enter as exact data (layout restated below from seq_layout.h), so the bound is the backward kernels' own; the saved gates
and states are themselves held to the forward reference's tracked steps (recur_ref docstring: backward from the saved workspace).

Branch reached by each encoder case (R.ENC16_CASES carries the sentence; conditions quoted from the sources, 256 CUs):
  chain forward      skinny.hip vag_gru_step_launch(w16), nz = 2: `a.K > 256 && wgs <= maxwg` (160) -> gru_step_small_kernel<8, 8, true>:
                     (512, B = 20) 32 * 2 * 2 = 128; `a.M >= 128 && a.K > 256 && grid.x * cdiv64(a.M, 32) * nz >= 192` ->
                     gru_step_kernel<8, true, 2>: (512, 130) 32 * 5 * 2 = 320, last 32-row tile rows 128, 129; else `a.K <= 256` ->
                     gru_step_kernel<4, true> (H = 40: kper = 32, the second wave's segment k = 32..39 alone passes `k < kend`; H = 256)
                     or gru_step_kernel<8, true> ((512, 96): 384 workgroups; (512, 64) with persistent = 0: 256).
  chain backward     vag_gru_bwd_step_launch(w16), K = 3H: `a.K <= 256` (120: four waves, the last sums k = 96..119) | `<= 1024` (768) |
                     `<= 1536` (1536, via (512, 20) and (512, 130): `cdiv64(a.H, 32) * cdiv64(a.M, 32) * nz >= 256` is 16 * 5 * 2 = 160:
                     not taken); `a.M >= 128 && a.K > 1024 && ..` -> gru_bwd_step_kernel<16, 4, true, 2, 2> at (1024, 130): 32 * 5 * 2 =
                     320, with persistent_enc_bwd = 0 behind the wide one-launch forward.
  one launch         enc_api.hip: `s16 && vag_opt().persistent && vag_enc_wide16_ok(B, Ts, H) && B >= 64` (persist.hip: H == 512 || 1024,
                     2 * cdiv64(B, 64) * (H / 32) workgroups <= CUs): enc_fwd_wide16_kernel<4 | 8>, enc_bwd_wide16_kernel<6 | 12>;
                     (512, 70): the second 64-row group holds 6 rows.  Which path ran is read off the workspace: the forward's counters
                     and the backward's fp16 exchange copy `gx` are written by the one-launch kernels only; `whhT` by fp32 storage only.
  decoder forward    dec_api.hip vag_cgru_attn_decode_seq_fwd: `hoist && !d.s16 && vag_opt().persistent && ..` -> dec_fwd_hoisted_chain with
                     options at their defaults; per step gru_step (nz = 1: (40 | 256, ..) kernel<4, true>; (512, 5 | 20) and (1024, 16)
                     `a.K > 256 && wgs <= 160` -> small<8, 8, true>; (512, 130) 32 * 9 = 288 workgroups, nz = 1: 32 * 5 = 160 < 192 ->
                     kernel<8, true>), skinny_plain_kernel<W, true> for q, skinny.hip vag_attn_dot_side_launch(0, .., s16): `W % 512 == 0 &&
                     (W == 1024 || ..)` -> attn_dot_side_reg_kernel<0, 8, true, NJ, wide>: H = 512 NJ = 2, H = 1024 NJ = 4, `wide = M >= 128`
                     at B = 130, `gx = cdiv64(512, N)` clipped to `Ts / (2 * WV)`: (512, 5, Ts = 33) -> 2 blocks of 17 and 16 positions;
                     H = 40, 256 -> attn_dot_side_kernel<0, 8, true>, `d.gx = cdiv64(Ts, 8)` = 2; attn_ctx_gru_kernel<true> on fp16 encwp.
  decoder backward   dec_api.hip dec_bwd_chain (`persist = !s16 && ..`): vag_attn_dot_side_launch(1, encwp, .., s16) with W = 3H: 120 and
                     768 -> attn_dot_side_kernel<1, 16, true>; 1536 and 3072 -> attn_dot_side_reg_kernel<1, 16 | 8, true, 3 | 6, wide>,
                     `a.a_scale = mode == 1 ? 4096.f : 1.f` on the riding dgh2 W_hh2; attn_dq_kernel<true> and attn_post_bwd_kernel<true> on
                     the fp16 pe; vag_gru_bwd_step_launch(w16), nz = 1, K = C (dq attn_h) and K = 3H (dgh1 W_hh1; `has_cell = 0` at t = 0).
  dense products     recur_ref.family16 / plan16_tile, asserted against vag_gemm_plan product by product in test_zy_*.

Largest |err| / bound per operator and output: restatement on the CPU (tests/test_storage16_ref_host.py -s) | device (this file -s).
  bigru16_bwd    g_b_hh 0.039 | 0.039   g_b_ih 0.039 | 0.039   g_emb 0.023 | 0.023   g_w_hh 0.146 | 0.135
                 g_w_ih 0.092 | 0.092
  bigru16_fwd    enc 0.211 | 0.211   gates 0.315 | 0.315   hst 0.211 | 0.211
  cgru16_bwd     d_enc_out 0.020 | 0.031   d_h0 0.013 | 0.013   d_pe 0.054 | 0.023   g_attn_h 0.098 | 0.098
                 g_attn_v 0.005 | 0.003   g_b_hh1 0.013 | 0.013   g_b_hh2 0.088 | 0.050   g_b_ih1 0.013 | 0.013
                 g_b_ih2 0.070 | 0.056   g_c2h 0.027 | 0.010   g_emb 0.024 | 0.024   g_w_hh1 0.022 | 0.022
                 g_w_hh2 0.300 | 0.290   g_w_ih1 0.036 | 0.036   g_w_ih2 0.323 | 0.334
  cgru16_fwd     c_all 0.000 | 0.000   h2_all 0.149 | 0.149
  cgru16_step    c_all 0.000 | 0.000   h2_all 0.153 | 0.153   ws_alpha 0.001 | 0.001   ws_encwp 0.967 | 0.967
                 ws_g1 0.520 | 0.214   ws_g2 0.256 | 0.256   ws_h1 0.126 | 0.121   ws_q 0.295 | 0.295
                 ws_uk 0.323 | 0.285
  keys_proj      pe 0.979 | 0.988
(keys_proj and ws_encwp sit next to 1: an fp16 store moves a value by up to half an fp16 ulp and the bound allows exactly that, on the
device and in the restatement alike.  cgru16_fwd is the free-running reference, whose figure is set by step 0; cgru16_step the one-step
reference.  The restatement's ws_* figures come from the backward cases' forwards.)
Wall time of this file on an MI355X: 7.7 s for its 38 cases, the float64 references included (no case above 1.1 s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recur_ref as R
import test_gpu_recurrences as G
from recur_ref import T
from test_gpu_recurrences import _in, _Out, _Ws, _bits, _sync, DEV

pytestmark = pytest.mark.gpu

WORST = {}
A5 = 0xA5
OPTIONS = ("persistent", "persistent_enc_bwd", "persistent_dec_bwd")


def _L():
    from vagnmt_hip import _lib
    return _lib


def _check(op, what, got, ref, tag):
    assert np.isfinite(got).all(), (what, "non-finite (a read outside an input, or an output that was never written)", tag)
    q = R.ratio(got, ref)
    WORST[(op, what)] = max(WORST.get((op, what), 0.0), q)
    print("%-14s %-8s %-44s |err|/bound %.3f" % (op, what, tag, q))
    assert q <= 1.0, (op, what, tag, "worst |err| / bound %.3g" % q)
    return got


class _mode:
    """`with _mode(derived, persistent=0, ...)`: the 2-byte storage mode on this thread with `derived` (a _Ws) as the derived buffer, and
    options; the exit restores the default context and every option whatever happened."""

    def __init__(self, derived, **opts):
        self.derived, self.opts = derived, opts

    def __enter__(self):
        L = _L()
        for k, v in self.opts.items():
            L.set_option(k, v)
        L.call("vag_set_operator_context", L.ptr(self.derived.view), 1)

    def __exit__(self, *exc):
        L = _L()
        rc = L.lib().vag_set_operator_context(None, 0)
        for k in OPTIONS:
            L.set_option(k, 1)
        L.call("vag_set_handoff_planes", None, 0)
        assert rc == 0
        return False


def _r64(n):
    return (int(n) + 63) & ~63


def _carve(sizes):
    """kernels.h WsCarver: regions in order, each rounded up to 64 floats -> {name: (offset, floats)}, total."""
    off, out = 0, {}
    for name, n in sizes:
        out[name] = (off, int(n))
        off += _r64(n)
    return out, off


def _halves(n):
    return (2 * int(n) + 3) // 4                                            # WsCarver::take_as<vag_half>: whole floats, rounded up


def _derived_layout(H):
    """seq_layout.h: derived_layout / cgru_prep restated.  Sizes in floats; the *16 regions hold twice as many halves."""
    C2, Q = 2 * H, 5 * H
    prep, prep_total = _carve([("wcat", Q * H), ("bcat", Q), ("wp", 3 * H * C2)])
    lay, total = _carve([("prep", prep_total), ("wcatT", Q * H), ("whh1T", 3 * H * H), ("encT", 6 * H * H),
                         ("wcat16", _halves(Q * H)), ("wcatT16", _halves(Q * H)), ("whh1_16", _halves(3 * H * H)),
                         ("whh1T16", _halves(3 * H * H)), ("enc16", _halves(6 * H * H)), ("encT16", _halves(6 * H * H))])
    for k, (o, n) in prep.items():
        lay[k] = (lay["prep"][0] + o, n)
    del lay["prep"]
    return lay, total


@functools.lru_cache(maxsize=None)
def _weights(H):
    """Decoder and encoder recurrent weights of width H (the decoder generator's, at a tiny shape)."""
    d = R.dec_inputs(H, 16, 1, 1, 1)
    rs = R._rs(31, H)
    return d["emb"], d["w"], R._uni(rs, 3 * H, H, k=H ** -0.5), R._uni(rs, 3 * H, H, k=H ** -0.5)


def _derive(H, emb, w, whh_fw, whh_bw, with_fp16=1):
    """-> (derived _Ws, rc): vag_derive_weights into a 0xA5 buffer; the device copies of the arguments are kept alive by the caller's sync."""
    L = _L()
    derived = _Ws(L.lib().vag_derived_floats(H))
    names = R.DEC_W_NAMES[1:]
    dev = [_in(emb)] + [_in(w[n]) for n in names] + [_in(whh_fw), _in(whh_bw)]
    W = G._dec_w(L, dev[0], dev[1:12])
    rc = L.lib().vag_derive_weights(W, L.ptr(dev[12]), L.ptr(dev[13]), H, with_fp16, L.ptr(derived.view), L.stream())
    _sync()
    return derived, rc


# ---------------------------------------------------------------------------------------------------------------- a. derived weights
@pytest.mark.parametrize("H", [8, 40, 256, 512])
def test_derive_weights_fp16_regions_are_float16_of_the_weights(H):
    L = _L()
    emb, w, fw, bw = _weights(H)
    lay, total = _derived_layout(H)
    assert total == L.lib().vag_derived_floats(H), (H, total)
    derived, rc = _derive(H, emb, w, fw, bw)
    assert rc == 0
    derived.check("derived", H)
    raw = derived.buf.cpu().numpy()[:total]
    C2, Q = 2 * H, 5 * H
    wcat = np.concatenate([w["attn_h"], w["w_hh2"]], 0)                       # (Q,H) = [attn_h ; W_hh2]
    both = lambda a, b: np.stack([a, b], 0)
    want32 = dict(wcat=wcat, bcat=np.concatenate([np.zeros(C2, np.float32), w["b_hh2"]]), wcatT=wcat.T, whh1T=w["w_hh1"].T,
                  encT=both(fw.T, bw.T))
    want16 = dict(wcat16=wcat, wcatT16=wcat.T, whh1_16=w["w_hh1"], whh1T16=w["w_hh1"].T, enc16=both(fw, bw), encT16=both(fw.T, bw.T))
    written = np.zeros(total, bool)
    for k, v in want32.items():
        o, n = lay[k]
        assert v.size == n and _bits(raw[o:o + n], np.ascontiguousarray(v).reshape(-1)), ("fp32 region differs from the weights", k, H)
        written[o:o + n] = True
    for k, v in want16.items():
        o, n = lay[k]
        got = raw[o:o + n].view(np.float16)[:v.size]
        want = np.ascontiguousarray(v, dtype=np.float32).reshape(-1).astype(np.float16)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), ("fp16 region is not numpy.float16 of the weights", k, H)
        written[o:o + n] = True
        assert 2 * n - v.size in (0, 1)
    # everything else -- the padding between regions and wp, which no path reads from a derived buffer -- still holds 0xA5
    assert (raw.view(np.uint8).reshape(-1, 4)[~written] == A5).all(), ("a write between the regions", H)
    assert not written[lay["wp"][0]:lay["wp"][0] + lay["wp"][1]].any()


def test_derive_weights_fp16_rejects_a_width_that_is_no_multiple_of_8():
    emb, w, fw, bw = _weights(12)
    derived, rc = _derive(12, emb, w, fw, bw)
    assert rc == -22
    assert bool((derived.buf.view(torch.uint8) == A5).all()), "a rejected call wrote to the derived buffer"
    derived, rc = _derive(12, emb, w, fw, bw, with_fp16=0)                   # (the fp32 regions alone are fine at H = 12)
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------- b. keys
@functools.lru_cache(maxsize=None)
def _keys_ref(rows, Cw):
    return R.attn_keys_proj(T, R.keys16_inputs(rows, Cw), storage=1)["pe"]


def _keys16(L, enc, attn_e, rows, Cw, tag):
    """vag_attn_keys_proj in the mode -> (the int16 buffer, its first rows * C halves as fp16).  The buffer holds rows * C halves of
    fp16 NaN and then as many halves again of a sentinel: a write of fp32 size lands in the sentinel, not outside the allocation."""
    n = rows * Cw
    buf = torch.cat([torch.full((n,), 0x7E00, dtype=torch.int16), torch.full((n + 64,), 0x5A5A, dtype=torch.int16)]).to(DEV)
    L.call("vag_attn_keys_proj", L.ptr(enc), L.ptr(attn_e), rows, Cw, L.ptr(buf, torch.int16), L.stream())
    _sync()
    host = buf.cpu().numpy()
    assert (host[n:] == 0x5A5A).all(), ("write past rows * C halves", tag)
    return buf, host[:n].view(np.float16).reshape(rows, Cw)


@pytest.mark.parametrize("rows,Cw", R.KEYS16_CASES, ids=lambda x: str(x))
def test_attn_keys_proj_fp16_matches_fp64_per_element(rows, Cw):
    L = _L()
    inp = R.keys16_inputs(rows, Cw)
    enc, attn_e = _in(inp["enc"]), _in(inp["attn_e"])
    derived = _Ws(L.lib().vag_derived_floats(Cw // 2))                        # (named by the context; this operator never reads it)
    plan = (C.c_int * 6)()
    with _mode(derived):
        assert L.lib().vag_gemm_plan(rows, Cw, Cw, 1, 1, 1, 0.0, 0, 1, 0, 0, 0, plan) == 0
        _, pe16 = _keys16(L, enc, attn_e, rows, Cw, (rows, Cw))
    derived.check("derived", (rows, Cw))
    assert bool((derived.buf.view(torch.uint8) == A5).all())
    want = "planes" if R.plan16_tile(rows, Cw, Cw, 0.0, True) == 128 else "exact"
    assert {0: "exact", 2: "planes"}[plan[0]] == want, (list(plan), want)
    assert want == ("planes" if rows == 4200 else "exact")
    _check("keys_proj", "pe", pe16.astype(np.float32), _keys_ref(rows, Cw), (rows, Cw, want))


# ---------------------------------------------------------------------------------------------------------------- c. encoder
ENC_G = ["w_ih", "w_hh", "b_ih", "b_hh"]


@functools.lru_cache(maxsize=None)
def _enc_fwd_ref(key):
    fwd = R.bigru_fwd(T, R.enc16_inputs(*key), storage=1)
    return fwd, R.bigru_ws_arrays(T, fwd)


def _bigru_layout(B, Ts, E, H):
    """seq_layout.h: bigru_ws restated up to the counters (whose count is the library's)."""
    lay, off = _carve([("x", Ts * B * E), ("xp", Ts * B * 6 * H), ("hst", 2 * (Ts + 1) * B * H), ("gates", 2 * Ts * 4 * B * H),
                       ("dgh", 2 * Ts * B * 3 * H), ("carry", 4 * B * H), ("dx", Ts * B * E), ("whhT", 6 * H * H), ("gx", 3 * Ts * B * H)])
    lay["sync"] = (off, 1)
    return lay


def _enc_run(case, storage):
    """One forward + backward of the encoder; storage 1: in the mode.  -> everything the checks read, on the host."""
    L = _L()
    H, E, B, Ts = case.H, case.E, case.B, case.Ts
    key = R.enc_key(case)
    inp = R.enc16_inputs(*key)
    tag = G._case_id(case)
    opts = dict(persistent=case.one_launch)
    if case.opt:
        opts[case.opt] = 0
    drop = case.p_emb > 0 or case.p_ctx > 0
    rng = G._rng() if drop else None
    src, lens, emb = _in(inp["src"], torch.int64), _in(inp["lens"], torch.int32), _in(inp["emb"])
    fw, bw = [_in(x) for x in inp["fw"]], [_in(x) for x in inp["bw"]]
    enc, mask = _Out((B, Ts, 2 * H)), _Out((B, Ts))
    d_enc = _Out((B, Ts, 2 * H), inp["d_enc"])
    g_emb = _Out((R.ENC_VS, E), inp["g_emb0"])
    g_fw = [_Out(x.shape, x) for x in inp["g_fw0"]]
    g_bw = [_Out(x.shape, x) for x in inp["g_bw0"]]
    ws = _Ws(L.lib().vag_bigru_ws_floats(B, Ts, E, H))
    demb, dw, _, _ = _weights(H)
    derived, rc = _derive(H, demb, dw, inp["fw"][1], inp["bw"][1])
    assert rc == 0, tag
    before = derived.buf.clone()

    def both():
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
        assert L.lib().vag_persistent_timeouts() == 0, ("a wait of a one-launch kernel gave up", tag)

    if storage:
        with _mode(derived, **opts):
            both()
    else:
        with G._options(**opts):
            both()
    ws.check("ws", tag)
    derived.check("derived", tag)
    assert torch.equal(derived.buf.view(torch.int32), before.view(torch.int32)), ("an operator wrote to the derived buffer", tag)
    d_enc.host("d_enc", tag)                                                 # consumed: only its extent is promised
    raw = ws.buf.cpu().numpy()
    lay = _bigru_layout(B, Ts, E, H)
    region = lambda k: raw[lay[k][0]:lay[k][0] + lay[k][1]]
    out = dict(inp=inp, tag=tag, key=key, mask=mask.host("mask", tag), enc=enc.host("enc", tag), g_emb=g_emb.host("g_emb", tag),
               gates=region("gates").reshape(2, Ts, 4, B, H), hst=region("hst").reshape(2, Ts + 1, B, H),
               untouched={k: bool((region(k).view(np.uint8) == A5).all()) for k in ("whhT", "gx", "sync")})
    for name, gs in (("fw", g_fw), ("bw", g_bw)):
        for k, o in zip(ENC_G, gs):
            out["g_%s_%s" % (name, k)] = o.host("g_" + k, tag)
    return out


@pytest.mark.parametrize("case", R.ENC16_CASES, ids=G._case_id)
def test_bigru_seq_fp16_storage_matches_fp64_per_element(case):
    H, E, B, Ts = case.H, case.E, case.B, case.Ts
    got = _enc_run(case, 1)
    inp, tag, key = got["inp"], got["tag"], got["key"]
    # which path ran (module docstring: one launch)
    wide_bwd = bool(case.one_launch and not case.opt)
    assert got["untouched"] == dict(whhT=True, gx=not wide_bwd, sync=not case.one_launch), (got["untouched"], tag)
    fwd, (gates_t, hst_t) = _enc_fwd_ref(key)
    assert _bits(got["mask"], fwd["mask"]), ("mask", tag)
    e32 = _check("bigru16_fwd", "enc", got["enc"], fwd["enc"], tag)
    for b, n in enumerate(inp["lens"]):
        assert (e32[b, n:] == 0.0).all(), ("enc past the length of row %d" % b, tag)
    _check("bigru16_fwd", "gates", got["gates"], gates_t, tag)
    _check("bigru16_fwd", "hst", got["hst"], hst_t, tag)
    bwd = R.bigru_bwd(T, inp, R.bigru_saved(T, inp, got["gates"], got["hst"]), storage=1)
    _check("bigru16_bwd", "g_emb", got["g_emb"], bwd["g_emb"], tag)
    for r in (0, R.ENC_NEVER):
        assert _bits(got["g_emb"][r], inp["g_emb0"][r]), ("g_emb row %d was written" % r, tag)
    for name in ("fw", "bw"):
        for k in ENC_G:
            _check("bigru16_bwd", "g_" + k, got["g_%s_%s" % (name, k)], bwd["g_%s_%s" % (name, k)], tag + "/" + name)


# ---------------------------------------------------------------------------------------------------------------- d. decoder
def _cgru_layout(B, Ts, Tt, E, H):
    """seq_layout.h: cgru_ws / cgru_prep restated up to h1 (checked below against vag_cgru_ws_offset where the ABI names a region)."""
    Cw, Q = 2 * H, 5 * H
    prep = _r64(Q * H) + _r64(Q) + _r64(3 * H * Cw)
    lay, _ = _carve([("xp1", Tt * B * 3 * H), ("g1", Tt * 4 * B * H), ("g2", Tt * 4 * B * H), ("qhp", Tt * B * Q), ("scores", B * Ts),
                     ("alpha", Tt * B * Ts), ("tmp", B * E), ("prep", prep), ("encwp", B * Ts * 3 * H), ("uk", B * Ts * H),
                     ("h1", Tt * B * H)])
    return lay


def _dec16_run(case, bwd):
    """The decoder's forward in the mode, checked; with `bwd` (a Dec16Bwd) the backward behind it, checked against the reference from
    the workspace that forward saved."""
    L = _L()
    H, E, B, Ts, Tt = case[:5]
    Cw, Q = 2 * H, 5 * H
    tag = G._case_id(case)
    inp = dict(R.dec16_inputs(H, E, B, Ts, Tt))
    enc, mask, h0 = _in(inp["enc"]), _in(inp["mask"]), _in(inp["h0"])
    tok, emb, attn_e = _in(inp["tok"], torch.int64), _in(inp["emb"]), _in(inp["attn_e"])
    names = R.DEC_W_NAMES[1:]
    wts = [_in(inp["w"][n]) for n in names]
    W = G._dec_w(L, emb, wts)
    h2, c_all, e_all = _Out((Tt, B, H)), _Out((Tt, B, Cw)), _Out((Tt, B, E))
    ws = _Ws(L.lib().vag_cgru_ws_floats(B, Ts, Tt, E, H))
    scratch = _Ws(L.lib().vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H))
    rs = R._rs(32, H)
    derived, rc = _derive(H, inp["emb"], inp["w"], R._uni(rs, 3 * H, H, k=H ** -0.5), R._uni(rs, 3 * H, H, k=H ** -0.5))
    assert rc == 0, tag
    before = derived.buf.clone()
    if bwd:
        d_h2, d_c = _Out((Tt, B, H), inp["d_h2"]), _Out((Tt, B, Cw), inp["d_c"])
        d_e = _in(inp["d_e"]) if bwd.d_e else None
        d_enc = _Out((B, Ts, Cw), inp["d_enc0"] if bwd.acc else None)
        d_pe, d_h0 = _Out((B, Ts, Cw)), _Out((B, H))
        g_emb = _Out((R.DEC_VT, E), inp["g_emb0"])
        gs = [_Out(inp["g0"][n].shape, inp["g0"][n]) for n in names]
        Gd = G._dec_w(L, g_emb.view, [g.view for g in gs])
    with _mode(derived):                                                     # (options at their defaults: `hoist && !d.s16 && ..` alone keeps the chain)
        pe_buf, pe16 = _keys16(L, enc, attn_e, B * Ts, Cw, tag)               # the keys as the mode stores them: (b) on the device
        pe = L.ptr(pe_buf, torch.int16)
        L.call("vag_cgru_attn_decode_seq_fwd", L.ptr(enc), pe, L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W,
               B, Ts, Tt, E, H, R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(ws.view), 0, None, 0.0, None, None,
               None, 0, L.stream())
        _sync()
        saved = ws.buf.cpu().numpy().copy()                                   # the workspace as the backward will read it
        if bwd:
            common = (L.ptr(enc), pe, L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H, R.DEC_VT, L.ptr(h2.view),
                      L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_h2.view), L.ptr(d_c.view), L.ptr(d_e), L.ptr(ws.view), L.ptr(d_enc.view),
                      bwd.acc, L.ptr(d_pe.view), L.ptr(d_h0.view))
            if bwd.two_phase:
                L.call("vag_cgru_attn_decode_seq_bwd_loop", *common, L.ptr(scratch.view), L.stream())
                L.call("vag_cgru_attn_decode_seq_bwd_weights", L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H, L.ptr(h2.view),
                       L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_e), L.ptr(ws.view), Gd, L.ptr(scratch.view), L.stream())
            else:
                L.call("vag_cgru_attn_decode_seq_bwd", *common, Gd, L.ptr(scratch.view), L.stream())
            _sync()
        assert L.lib().vag_persistent_timeouts() == 0, tag
    ws.check("ws", tag)
    scratch.check("scratch", tag)
    derived.check("derived", tag)
    assert torch.equal(derived.buf.view(torch.int32), before.view(torch.int32)), ("an operator wrote to the derived buffer", tag)
    if not bwd:
        assert bool((scratch.buf.view(torch.uint8) == A5).all()), tag
    _check("keys_proj", "pe", pe16.astype(np.float32), R.attn_keys_proj(T, R.dec16_keys_inputs(inp), storage=1)["pe"], tag)
    inp["pe"] = pe16.astype(np.float32).reshape(B, Ts, Cw)                    # its bits: exact data from here on
    h2_32, c32, e32 = h2.host("h2_all", tag), c_all.host("c_all", tag), e_all.host("e_all", tag)
    assert _bits(e32, inp["emb"][inp["tok"][:Tt]]), ("e_all is not the gathered embedding rows", tag)
    if Tt <= 3:                                                              # (the eight-step case: the one-step reference alone)
        fwd = R.cgru_fwd(T, inp, storage=1)
        _check("cgru16_fwd", "h2_all", h2_32, fwd["h2_all"], tag)
        _check("cgru16_fwd", "c_all", c32, fwd["c_all"], tag)
    rec = R.cgru_fwd(T, inp, h2_given=h2_32, storage=1)
    _check("cgru16_step", "h2_all", h2_32, rec["h2_all"], tag)
    _check("cgru16_step", "c_all", c32, rec["c_all"], tag)
    # what the forward left in its workspace, held to the one-step reference and then handed to the backward's reference as exact data
    lay = _cgru_layout(B, Ts, Tt, E, H)
    for which, k in enumerate(("alpha", "h1", "qhp")):
        assert L.lib().vag_cgru_ws_offset(B, Ts, Tt, E, H, which) == lay[k][0], (k, tag)
    region = lambda k: saved[lay[k][0]:lay[k][0] + lay[k][1]]
    dev = dict(g1=region("g1").reshape(Tt, 4, B, H), g2=region("g2").reshape(Tt, 4, B, H), h1=region("h1").reshape(Tt, B, H),
               alpha=region("alpha").reshape(Tt, B, Ts), q=np.ascontiguousarray(region("qhp").reshape(Tt, B, Q)[:, :, :Cw]),
               uk=region("uk").reshape(B, Ts, H),
               encwp=region("encwp").view(np.float16)[:B * Ts * 3 * H].astype(np.float32).reshape(B, Ts, 3 * H))
    want = R.cgru_ws_saved(T, rec)
    for k in sorted(dev):
        _check("cgru16_step", "ws_" + k, dev[k], want[k], tag)
    if not bwd:
        return
    d_h2.host("d_h2_all", tag)                                               # consumed: only their extent is promised
    d_c.host("d_c_all", tag)
    ref = R.cgru_bwd(T, inp, R.cgru_saved(T, inp, h2_32, dev), c32, e32, bwd.acc, bwd.d_e, storage=1)
    _check("cgru16_bwd", "d_enc_out", d_enc.host("d_enc_out", tag), ref["d_enc_out"], tag)
    _check("cgru16_bwd", "d_pe", d_pe.host("d_pe", tag), ref["d_pe"], tag)
    _check("cgru16_bwd", "d_h0", d_h0.host("d_h0", tag), ref["d_h0"], tag)
    got = _check("cgru16_bwd", "g_emb", g_emb.host("g_emb", tag), ref["g_emb"], tag)
    for r in (0, R.DEC_NEVER):
        assert _bits(got[r], inp["g_emb0"][r]), ("g.emb row %d was written" % r, tag)
    for n, o in zip(names, gs):
        _check("cgru16_bwd", "g_" + n, o.host("g_" + n, tag), ref["g_" + n], tag)


@pytest.mark.parametrize("case", R.DEC16_CASES, ids=G._case_id)
def test_cgru_attn_decode_seq_fwd_fp16_storage_matches_fp64_per_element(case):
    _dec16_run(case, None)


@pytest.mark.parametrize("case", R.DEC16_BWD_CASES, ids=G._case_id)
def test_cgru_attn_decode_seq_bwd_fp16_storage_matches_fp64_per_element(case):
    _dec16_run(case, case)


# ---------------------------------------------------------------------------------------------------------------- e. rejections
def _nothing_written(outs, wss, tag):
    for o in outs:
        h = o.buf.cpu()
        assert bool(torch.isnan(h[:o.n]).all()) and torch.equal(h[o.n:], o.sent), ("a rejected call wrote an output", tag)
    for w in wss:
        assert bool((w.buf.view(torch.uint8) == A5).all()), ("a rejected call wrote a workspace", tag)


def _dec_call_args(H, E, B, Ts, Tt):
    """Buffers of one decoder forward / backward-loop call at a shape whose sizes the library can still compute."""
    L = _L()
    Cw = 2 * H
    inp = R.dec_inputs(H, E, B, Ts, Tt)
    dev = dict(enc=_in(inp["enc"]), pe=_in(inp["pe"]), mask=_in(inp["mask"]), h0=_in(inp["h0"]), tok=_in(inp["tok"], torch.int64),
               emb=_in(inp["emb"]), w=[_in(inp["w"][n]) for n in R.DEC_W_NAMES[1:]])
    outs = dict(h2=_Out((Tt, B, H)), c=_Out((Tt, B, Cw)), e=_Out((Tt, B, E)), d_enc=_Out((B, Ts, Cw)), d_pe=_Out((B, Ts, Cw)),
                d_h0=_Out((B, H)))
    wss = dict(ws=_Ws(L.lib().vag_cgru_ws_floats(B, Ts, Tt, E, H)), scratch=_Ws(L.lib().vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H)))
    return inp, dev, outs, wss, G._dec_w(L, dev["emb"], dev["w"])


def _dec_fwd_rc(L, dev, outs, wss, W, shape, free_run=0, head=None, tmid=None, logits=None, ldl=0):
    H, E, B, Ts, Tt = shape
    return L.lib().vag_cgru_attn_decode_seq_fwd(
        L.ptr(dev["enc"]), L.ptr(dev["pe"]), L.ptr(dev["mask"]), L.ptr(dev["h0"]), L.ptr(dev["tok"], torch.int64), W, B, Ts, Tt, E, H,
        R.DEC_VT, L.ptr(outs["h2"].view), L.ptr(outs["c"].view), L.ptr(outs["e"].view), L.ptr(wss["ws"].view), free_run, head, 0.0,
        None, L.ptr(tmid), L.ptr(logits), ldl, L.stream())


def test_mode_rejects_free_running_decoding():
    """dec_api.hip: `VAG_CHECK_ARG(!d.s16 || (hoist && vag_ctx().derived && H % 8 == 0 && ..))` -- with every argument the free-running
    form itself asks for in place, so that this is the check that refuses."""
    L = _L()
    shape = (40, 16, 5, 9, 3)
    H, E, B, Ts, Tt = shape
    inp, dev, outs, wss, W = _dec_call_args(*shape)
    big = [torch.zeros(1 << 16, device=DEV) for _ in range(8)]                # head weights: never read by a rejected call
    head = _L().HeadW(*[L.ptr(t) for t in big])
    tmid, logits = _Out((Tt, B, E)), _Out((Tt, B, 20))
    emb, w, fw, bw = _weights(H)
    derived, rc = _derive(H, emb, w, fw, bw)
    assert rc == 0
    with _mode(derived, persistent=0):
        rc = _dec_fwd_rc(L, dev, outs, wss, W, shape, 1, C.byref(head), tmid.view, logits.view, 20)
        _sync()
    assert rc == -22
    _nothing_written(list(outs.values()) + [tmid, logits], wss.values(), "free_run")


def test_mode_rejects_a_width_that_is_no_multiple_of_8():
    """H = 36 (a multiple of 4: fine at storage 0): enc_api.hip `!vag_ctx().store16 || (vag_ctx().derived && H % 8 == 0)` in both encoder
    entry points, dec_api.hip the forward's check above and the backward loop's `!s16 || (vag_ctx().derived && H % 8 == 0)`."""
    L = _L()
    shape = (36, 16, 5, 4, 2)
    H, E, B, Ts, Tt = shape
    derived = _Ws(L.lib().vag_derived_floats(40))                             # (a buffer to name: vag_derive_weights itself refuses H = 36)
    einp = R.enc_inputs(H, E, B, Ts)
    src, lens, emb = _in(einp["src"], torch.int64), _in(einp["lens"], torch.int32), _in(einp["emb"])
    fw, bw = [_in(x) for x in einp["fw"]], [_in(x) for x in einp["bw"]]
    enc, mask, d_enc = _Out((B, Ts, 2 * H)), _Out((B, Ts)), _Out((B, Ts, 2 * H))
    g_emb, g_fw, g_bw = _Out((R.ENC_VS, E)), [_Out(x.shape) for x in einp["g_fw0"]], [_Out(x.shape) for x in einp["g_bw0"]]
    ews = _Ws(L.lib().vag_bigru_ws_floats(B, Ts, E, H))
    inp, dev, outs, wss, W = _dec_call_args(*shape)
    d_h2, d_c = _Out((Tt, B, H)), _Out((Tt, B, 2 * H))
    with _mode(derived, persistent=0):
        rcs = [L.lib().vag_bigru_seq_fwd(L.ptr(src, torch.int64), L.ptr(lens, torch.int32), L.ptr(emb), L.gru_w(*fw), L.gru_w(*bw), 0.0, 0.0,
                                         None, B, Ts, E, H, L.ptr(enc.view), L.ptr(mask.view), L.ptr(ews.view), L.stream()),
               L.lib().vag_bigru_seq_bwd(L.ptr(src, torch.int64), L.ptr(lens, torch.int32), L.gru_w(*fw), L.gru_w(*bw), 0.0, 0.0, None, B, Ts,
                                         E, H, L.ptr(d_enc.view), L.ptr(ews.view), L.ptr(g_emb.view), L.gru_w(*[g.view for g in g_fw]),
                                         L.gru_w(*[g.view for g in g_bw]), L.stream()),
               _dec_fwd_rc(L, dev, outs, wss, W, shape),
               L.lib().vag_cgru_attn_decode_seq_bwd_loop(
                   L.ptr(dev["enc"]), L.ptr(dev["pe"]), L.ptr(dev["mask"]), L.ptr(dev["h0"]), L.ptr(dev["tok"], torch.int64), W, B, Ts, Tt,
                   E, H, R.DEC_VT, L.ptr(outs["h2"].view), L.ptr(outs["c"].view), L.ptr(outs["e"].view), L.ptr(d_h2.view), L.ptr(d_c.view),
                   None, L.ptr(wss["ws"].view), L.ptr(outs["d_enc"].view), 0, L.ptr(outs["d_pe"].view), L.ptr(outs["d_h0"].view),
                   L.ptr(wss["scratch"].view), L.stream())]
        _sync()
    assert rcs == [-22, -22, -22, -22], rcs
    _nothing_written([enc, mask, d_enc, g_emb, d_h2, d_c] + g_fw + g_bw + list(outs.values()), [ews, derived] + list(wss.values()), "H = 36")


def test_mode_without_a_derived_buffer_is_refused_and_the_operators_stay_at_fp32_storage():
    """api.hip: vag_set_operator_context `VAG_CHECK_ARG(storage == 0 || (storage == 1 && derived))` refuses the pair before it edits the
    context, so the mode cannot be entered without a derived buffer through the ABI: the operators' own conditions for that state
    (decoder: the documented rejection `!d.s16 || (.. vag_ctx().derived ..)`; encoder: `EncSeq::s16 = store16 && derived`, i.e. fp32
    storage) are never met.  What a caller sees: -22, and the next encoder call runs at fp32 storage -- it satisfies the fp32 bounds of
    recur_ref (storage = 0), which no 2^-11-rounded state does, and it transposes W_hh into its own workspace."""
    L = _L()
    try:
        assert L.lib().vag_set_operator_context(None, 1) == -22
        case = R.ENC16_CASES[1]
        got = _enc_run(case, 0)
    finally:
        assert L.lib().vag_set_operator_context(None, 0) == 0
    inp = got["inp"]
    fwd = R.bigru_fwd(T, inp)
    assert got["untouched"]["whhT"] is False
    _check("bigru_fp32", "enc", got["enc"], fwd["enc"], got["tag"])
    bwd = R.bigru_bwd(T, inp, R.bigru_saved(T, inp, got["gates"], got["hst"]))
    for name in ("fw", "bw"):
        for k in ENC_G:
            _check("bigru_fp32", "g_" + k, got["g_%s_%s" % (name, k)], bwd["g_%s_%s" % (name, k)], got["tag"] + "/" + name)
    # ... and the mode's own result at the same case does leave the fp32 bound: the two storages are told apart by it
    assert R.ratio(_enc_run(case, 1)["enc"], fwd["enc"]) > 1.0


# ---------------------------------------------------------------------------------------------------------------- planner, defaults, report
def test_zy_planned_products_take_the_family_the_reference_assumed():
    L = _L()
    for c in R.ENC16_CASES:
        _enc_fwd_ref(R.enc_key(c))
    plan = (C.c_int * 6)()
    derived = _Ws(64)
    with _mode(derived):
        for M, N, K, beta, c_half, tile in sorted(R.PRODUCTS16):
            assert L.lib().vag_gemm_plan(M, N, K, 1, 1, 1, beta, 0, c_half, 0, 0, 0, plan) == 0
            assert (plan[0], plan[1]) == ((0, 64) if tile == 64 else (2, 128)), ((M, N, K, beta, c_half), list(plan), tile)


def test_zz_context_and_options_are_back_at_their_defaults():
    """After everything above, whatever failed: planes 3 (the default context's) is what the planner reads, and a plain encoder call
    at fp32 storage transposes W_hh into its own workspace."""
    L = _L()
    plan2, plan3 = (C.c_int * 6)(), (C.c_int * 6)()
    assert L.lib().vag_gemm_plan(4200, 512, 512, 1, 1, 1, 0.0, 0, 0, 0, 1, 0, plan2) == -22      # row sums need an outer-contiguous A
    assert L.lib().vag_gemm_plan(512, 512, 4200, 0, 0, 1, 1.0, 0, 0, 0, 1, 0, plan2) == 0
    assert L.lib().vag_gemm_plan(512, 512, 4200, 0, 0, 1, 1.0, 0, 0, 0, 1, 3, plan3) == 0
    assert list(plan2) == list(plan3) and plan2[5] == 1                       # rides only on three planes: the context is the default one
    assert L.lib().vag_persistent_timeouts() == 0
    got = _enc_run(R.ENC16_CASES[1], 0)
    assert got["untouched"]["whhT"] is False


def test_zzz_report_worst_ratios():
    """Runs last in this file: the largest |err| / bound per operator and output on the device (shown with -s)."""
    for op, what in sorted(WORST):
        print("device worst |err| / bound  %-14s %-8s %.3f" % (op, what, WORST[(op, what)]))
