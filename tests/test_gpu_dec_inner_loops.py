"""The LDS-resident inner loops of the one-launch decoder recurrences (persist.hip: dec_fwd_persistent_kernel's score shares and projected
context, dec_bwd_persistent_kernel's d-alpha shares of phase A and dq of phase B) read ahead in batches and address their (row, position)
pairs linearly; the one-launch encoder backward forms its context-dropout multipliers in front of the hand-off wait.  Through the C ABI,
as tests/test_gpu_recurrences.py (whose buffer helpers this file uses: NaN-filled outputs, sentinel tails, 0xA5 workspaces and plane
buffers), element by element against the float64 references of tests/recur_ref.py: the forward against the one-step reference
(cgru_fwd with h2_given = the device's own states, sharp at every step), the backward against cgru_bwd, |got - value| <= the bound the
reference carries.  vag_persistent_timeouts() == 0 after every case.

Shapes: the smallest at which the batching can go wrong.  H in {256, 512} (32 / 64 workgroups per row tile: both template widths);
B in {5, 17, 64}: a partial tile, a second tile of one row, full tiles -- the row test of a pair is now `P < (B - m0) Ts`.  Ts:
   1, 2      no batch at all: the quad round of phase A with 16 / 32 pairs, ctx_dot's tails alone
   7, 8, 9   one below, at and one past the eight-position batch of the projected context (7 = four + two + one); dq's two-link batch
             starts at Ts = 7 (half 0) / 8 (half 1)
   16, 17    dq's four-link batch: 15 + half <= Ts; 16 Ts = 256, 272: two and three quad rounds in phase A
   31, 32    16 Ts = 496 (above 384: whole pairs on 496 threads), 512 (exactly one whole round, no quad round)
   33, 40    a whole round and a quad round of 16 / 128 pairs; 40 is the workload's length (five score rounds)
   largest   forward: R.DEC_MAX_TS; backward: the largest Ts <= R.DEC_MAX_TS with vag_recurrence_supported(2, ...), 44 at H = 512
Tt = 2 forward (the second step reads the first one's hand-off); the backward at the lengths recur_ref allows (Tt = 2 at H = 256, 1 at
H = 512: recur_ref.DEC_CASES).  At H = 256 the forward case and the backward case are the same launch pair, run once.

Beside the bounds the same cases run through the launch chain (option "persistent" = 0), which these changes do not touch; the one-launch
results are held to it by the rule of test_wider_persistent_decoder_equals_launch_chain: every tensor to 2e-5 of its largest entry.

Encoder: one backward case per H with p_ctx = 0.5 and ragged lengths and one with p_ctx = 0, as test_bigru_seq_matches_fp64_per_element
runs its own cases (mask words, bounds, sentinels, timeouts)."""
import functools

import numpy as np
import pytest
import torch

import recur_ref as R
import test_gpu_recurrences as G
from recur_ref import T

pytestmark = pytest.mark.gpu

E = 64
TS = [1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 40, "max"]
CASES = [(H, B, Ts) for H in (256, 512) for B in (5, 17, 64) for Ts in TS]
NAMES = R.DEC_W_NAMES[1:]


def _bwd_tt(H):
    return 2 if H == 256 else 1


def _largest_ts(kind, H, B, Tt):
    sup = G._L().lib().vag_recurrence_supported
    return max(ts for ts in range(1, R.DEC_MAX_TS + 1) if sup(kind, B, ts, Tt, H) == 1)


@functools.lru_cache(maxsize=4)
def _run(H, B, Ts, Tt, bwd, persistent):
    """One forward (and backward) through the C ABI; host copies of every output."""
    L = G._L()
    C = 2 * H
    inp = R.dec_inputs(H, E, B, Ts, Tt)
    tag = "H%d-B%d-Ts%d-Tt%d-%s" % (H, B, Ts, Tt, "one-launch" if persistent else "chain")
    _in, _Out, _Ws = G._in, G._Out, G._Ws
    enc, pe, mask, h0 = _in(inp["enc"]), _in(inp["pe"]), _in(inp["mask"]), _in(inp["h0"])
    tok, emb = _in(inp["tok"], torch.int64), _in(inp["emb"])
    wts = [_in(inp["w"][n]) for n in NAMES]
    h2, c_all, e_all = _Out((Tt, B, H)), _Out((Tt, B, C)), _Out((Tt, B, E))
    ws = _Ws(L.lib().vag_cgru_ws_floats(B, Ts, Tt, E, H))
    scratch = _Ws(L.lib().vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H))
    d_h2, d_c = _Out((Tt, B, H), inp["d_h2"]), _Out((Tt, B, C), inp["d_c"])
    d_e = _in(inp["d_e"])
    d_enc, d_pe, d_h0 = _Out((B, Ts, C)), _Out((B, Ts, C)), _Out((B, H))
    g_emb = _Out((R.DEC_VT, E), inp["g_emb0"])
    gs = [_Out(inp["g0"][n].shape, inp["g0"][n]) for n in NAMES]
    W = G._dec_w(L, emb, wts)
    Gw = G._dec_w(L, g_emb.view, [g.view for g in gs])
    L.lib().vag_persistent_timeouts()
    with G._options(persistent=persistent):
        planes = G._planes(L.lib().vag_handoff_planes_floats(B, Ts, Tt, H), tag) if persistent else None
        if persistent:
            assert L.lib().vag_recurrence_supported(1, B, Ts, Tt, H) == 1, tag
            assert planes is not None, tag
            if bwd:
                assert L.lib().vag_recurrence_supported(2, B, Ts, Tt, H) == 1, tag
        L.call("vag_cgru_attn_decode_seq_fwd", L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E, H,
               R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(ws.view), 0, None, 0.0, None, None, None, 0, L.stream())
        if bwd:
            L.call("vag_cgru_attn_decode_seq_bwd", L.ptr(enc), L.ptr(pe), L.ptr(mask), L.ptr(h0), L.ptr(tok, torch.int64), W, B, Ts, Tt, E,
                   H, R.DEC_VT, L.ptr(h2.view), L.ptr(c_all.view), L.ptr(e_all.view), L.ptr(d_h2.view), L.ptr(d_c.view), L.ptr(d_e),
                   L.ptr(ws.view), L.ptr(d_enc.view), 0, L.ptr(d_pe.view), L.ptr(d_h0.view), Gw, L.ptr(scratch.view), L.stream())
        G._sync()
        G._no_timeouts(tag)
    ws.check("ws", tag)
    scratch.check("scratch", tag)
    if planes is not None:
        planes.check("hand-off planes", tag)
    d_h2.host("d_h2_all", tag)                                               # consumed: only their extent is promised
    d_c.host("d_c_all", tag)
    out = dict(h2_all=h2.host("h2_all", tag), c_all=c_all.host("c_all", tag), e_all=e_all.host("e_all", tag))
    if bwd:
        out.update(d_enc_out=d_enc.host("d_enc_out", tag), d_pe=d_pe.host("d_pe", tag), d_h0=d_h0.host("d_h0", tag),
                   g_emb=g_emb.host("g_emb", tag))
        for n, o in zip(NAMES, gs):
            out["g_" + n] = o.host("g_" + n, tag)
    else:
        assert np.isnan(d_pe.host("d_pe", tag)).all(), tag                   # (no backward was run)
    return out


def _equals_chain(one, chain, keys, tag):
    """test_wider_persistent_decoder_equals_launch_chain's rule: every tensor to 2e-5 of its largest entry."""
    for k in keys:
        assert np.isfinite(chain[k]).all(), (k, tag)
        scale = max(float(np.abs(chain[k]).max()), 1e-3)
        err = float(np.abs(one[k] - chain[k]).max())
        print("%-12s %-28s one launch against the chain: %.3g of the largest entry" % (k, tag, err / scale))
        assert err <= 2e-5 * scale, (k, tag, err, scale)


def _fwd_checks(H, B, Ts, Tt, one, tag):
    inp = R.dec_inputs(H, E, B, Ts, Tt)
    assert G._bits(one["e_all"], inp["emb"][inp["tok"][:Tt]]), ("e_all is not the gathered embedding rows", tag)
    rec = R.cgru_fwd(T, inp, h2_given=one["h2_all"])
    G._check("cgru_fwd_step", "h2_all", one["h2_all"], rec["h2_all"], tag)
    G._check("cgru_fwd_step", "c_all", one["c_all"], rec["c_all"], tag)
    return inp, rec


def _fwd_case(H, B, Ts):
    Tt = 2
    bwd = _bwd_tt(H) == Tt                                  # H = 256: the backward case's launches, shared
    if Ts == "max":
        Ts = _largest_ts(2 if bwd else 1, H, B, Tt)
        assert Ts == R.DEC_MAX_TS, Ts
    tag = "fwd-H%d-B%d-Ts%d" % (H, B, Ts)
    one = _run(H, B, Ts, Tt, bwd, 1)
    _fwd_checks(H, B, Ts, Tt, one, tag)
    _equals_chain(one, _run(H, B, Ts, Tt, bwd, 0), ("h2_all", "c_all"), tag)


def _bwd_case(H, B, Ts):
    Tt = _bwd_tt(H)
    if Ts == "max":
        Ts = _largest_ts(2, H, B, Tt)
        assert Ts <= R.DEC_MAX_TS and (Ts == R.DEC_MAX_TS or G._L().lib().vag_recurrence_supported(2, B, Ts + 1, Tt, H) == 0), Ts
        assert Ts > 40, Ts                                  # (a new length, beyond the list's)
    tag = "bwd-H%d-B%d-Ts%d" % (H, B, Ts)
    one = _run(H, B, Ts, Tt, True, 1)
    inp, rec = _fwd_checks(H, B, Ts, Tt, one, tag)
    op = "cgru_bwd" + R.dec_group(H)
    ref = R.cgru_bwd(T, inp, rec, one["c_all"], one["e_all"], 0, True)
    keys = ["d_enc_out", "d_pe", "d_h0", "g_emb"] + ["g_" + n for n in NAMES]
    for k in keys:
        G._check(op, k, one[k], ref[k], tag)
    for r in (0, R.DEC_NEVER):
        assert G._bits(one["g_emb"][r], inp["g_emb0"][r]), ("g.emb row %d was written" % r, tag)
    _equals_chain(one, _run(H, B, Ts, Tt, True, 0), keys, tag)


@pytest.mark.parametrize("H,B,Ts,what", [c + (w,) for c in CASES for w in ("fwd", "bwd")], ids=lambda x: str(x))
def test_dec_inner_loops_match_fp64_and_the_launch_chain(H, B, Ts, what):
    (_fwd_case if what == "fwd" else _bwd_case)(H, B, Ts)


ENC = [R._enc(256, 64, 21, 6, 1, "one launch, ragged lengths, p_ctx = 0.5: enc_bwd_persistent_kernel<3, true>", p=(0.3, 0.5)),
       R._enc(512, 64, 21, 6, 1, "one launch, ragged lengths, p_ctx = 0.5: enc_bwd_persistent_kernel<6, true>; hand-off planes",
              p=(0.3, 0.5)),
       R._enc(512, 64, 21, 6, 1, "the same without dropout: the multipliers stay 1; hand-off planes")]


@pytest.mark.parametrize("case", ENC, ids=G._case_id)
def test_enc_bwd_dropout_multipliers_formed_before_the_wait(case):
    G.test_bigru_seq_matches_fp64_per_element(case)
