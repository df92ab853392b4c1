"""The hoisted decoding step and the per-step output head -- vag_cgru_decode_keys / _tables once per decode call, then
vag_cgru_attn_decode_step_h and one of vag_head_logp_step(_h) / vag_head_logits_step(_h) per step: what every search runs -- through
the C ABI (vagnmt_hip._lib.call / ptr / stream / set_option), element by element against the tracked float64 references of
tests/decode_ref.py: |got - value| <= err, err carried by the reference itself (its docstring derives every rule), nothing relative to
a tensor's maximum.  tests/test_decode_ref_host.py shows on the CPU that the bounds hold for an fp32 restatement of each operator and
reject the defect catalogue, at exactly the cases below.

Buffers, as in test_gpu_recurrences.py (its _in, _Out, _Ws, _options are used): every input is followed by NaN floats (index arrays
by impossible indices), every output by a sentinel tail that must come back bit-identical; outputs start as NaN; scratch and prep start
with every byte 0xA5 and carry a checked tail; the padding columns [V, ldl) of a logp / logits buffer are pre-filled with the sentinel
and must come back unchanged.  `keys` and `tables` are the device's own (vag_cgru_decode_keys / _tables ran first) and enter the step's
reference exactly; the head's tables buffer is laid out on the host with NaN in embp and in the gaps, so a line taken from the wrong
region is not finite.  Beside the bounds, exactly: alpha 0.0 at masked positions, 1.0 / 0.0 for a sentence of length 1; e bit-equal to
the gathered embedding rows; m_i of `parts` bit-equal to the maximum of the device's own 64 logits of group i; argmax the smallest
index attaining the maximum of the device's own logp, with columns made bit-equal (one thread's two columns, two waves, two sweeps);
-22 with every output untouched for N = 257, N % rows_per_src != 0 and tables without tok.  _options restores attn_row to 1 whatever
happens.

Branch reached by each case (conditions quoted from the sources):
  step_h   dec_api.hip vag_cgru_attn_decode_step_h: `vag_attn_row_gru_ok(N, Ts, H, E)`, attn.hip: `vag_opt().attn_row != 0 && H == 512 &&
           W2 == 256 && N > 0 && N < (1ll << 30) && Ts > 0 && Ts <= 32` -> attn_row_gru_kernel<6,1>, else vag_attn_scores_launch +
           vag_attn_ctx_gru_launch (two launches).  (32,16,3,1,5), (256,64,3,3,5), (1024,256,2,2,5): two launches at other widths;
           (512,64,3,3,5): W2 = 64 != 256, two launches; (512,256,3,1,1): fused, Ts = 1, `min(wave + 8 * p, Ts - 1)` clamps all 16
           preloads to position 0; (512,256,2,3,7): fused, fewer positions than waves, `b = blockIdx.x / rps`; (512,256,2,12,16):
           fused, both preloaded positions of every wave real, `for (s0 = wave + 8 * PRE; s0 < Ts; ...)` not entered; (512,256,2,12,17):
           that loop entered by wave 0 alone, score buffer padded 17 -> 20; (512,256,1,5,32): the last fused Ts, every wave enters that loop
           once; (512,256,2,3,33): Ts > 32, two launches at production widths; (512,256,2,3,7) with attn_row = 0: the fused case's
           inputs on the two launches, same bounds; (512,256,16,16,9): fused at N = 256, the limit.  Every case with and without
           tables: `a.s[0].other_idx = tables ? tok : nullptr` (gru_1 reads the line of embp that tok picks) against
           vag_skinny_gather_launch.
  head     head_api.hip vag_head_step: `N <= 256 && aligned16(...)` -> one launch (skinny3), N = 257 -> the four-launch fallback;
           head_pre_step_h: cw as the addend, b2 kept, `embw3 ? nullptr : e` (the line of embw3 as the second addend).
           head.hip vag_lse_nll_launch: `V <= 256 * 8` (19, 2048) -> NV = 8; `V <= 256 * 40` (2049, 10240) -> NV = 40; else (10241)
           the streaming form, three sweeps of 1024 float4, the last of 513 with column 10240 alone in its float4.
  parts    skinny.hip skinny_tall_ok: `M > 96 && M <= 256 && N >= 4096 && K >= 256 && K % 256 == 0`: (97,4096) RT = 4, KS = 2, no
           ragged group; (97,4100), (192,4097), (256,4159): a last group of 4, 1 and 63 real columns; RT = 6, KS = 1 at 192 and RT = 8
           at 256; (96,4100) and (97,4095): count 0.

Largest |err| / bound per operator and output: fp32 restatement on the CPU (tests/test_decode_ref_host.py -s) | device (this file -s).
  decode_keys          encwp 0.056 | 0.057   encw2 0.180 | 0.363
  decode_tables        embp 0.564 | 0.470   embw3 0.682 | 0.551
  cgru_step_h          h_out 0.025 | 0.031   cw 0.003 | 0.004   alpha 0.005 | 0.003   cw against W2 c of the plain reference - | 0.001
  cgru_step_h_tables   h_out 0.027 | 0.031   cw 0.004 | 0.005   alpha 0.006 | 0.002
  cgru_step_plain      (the cross-form run, device only)  h_out 0.008   c 0.003   alpha 0.003
  head_plain           logits 0.028 | 0.015   lse 0.100 | -   logp 0.081 | 0.060
  head_hoisted_e       logits 0.047 | 0.022   lse 0.185 | -   logp 0.139 | 0.057
  head_hoisted_tables  logits 0.059 | 0.037   lse 0.261 | -   logp 0.198 | 0.073
  parts                s 0.081 | 0.103   lse recombined in float64 0.001 | 0.001
(The device's logits are those of the parts cases, the entry points that return them; the host's are all head cases.  The device has
no lse of its own outside the parts: logp holds it.  The tables, one short contraction and one addition, sit highest: at
half their bound, restatement and device alike.  The step sits at a hundredth, as the recurrences' attention path does: a worst-case bound widens by sum|w| at
each product.  Every tie case produced bit-equal maxima on the device: 2, 5 and 6 columns per row at V = 19, 2049, 10241.)
Wall time of this file on an MI355X: 5.2 s for its 81 cases, the float64 references included (no case above 0.5 s)."""
import functools

import numpy as np
import pytest
import torch

import decode_ref as D
from decode_ref import T, TV
from test_gpu_recurrences import _in, _Out, _Ws, _options, _dec_w, _bits, _sync, SENTINEL, DEV, TAIL

pytestmark = pytest.mark.gpu

WORST = {}
EINVAL = -22


def _L():
    from vagnmt_hip import _lib
    return _lib


def _check(op, what, out, ref, tag):
    got = out.host(what, tag) if isinstance(out, _Out) else out
    assert np.isfinite(got).all(), (what, "non-finite (a read outside an input, or an output that was never written)", tag)
    q = D.ratio(got, ref)
    WORST[(op, what)] = max(WORST.get((op, what), 0.0), q)
    print("%-22s %-8s %-44s |err|/bound %.3f" % (op, what, tag, q))
    assert q <= 1.0, (op, what, tag, "worst |err| / bound %.3g" % q)
    return got


def _ids(c):
    return "-".join(str(x) for x in c)


def _weights(inp):
    L = _L()
    emb = _in(inp["emb"])
    wts = [_in(inp["w"][n]) for n in D.R.DEC_W_NAMES[1:]]
    return _dec_w(L, emb, wts), (emb, wts)                                    # (the tensors are kept alive by the caller)


def _prep(W, H):
    L = _L()
    prep = _Ws(L.lib().vag_cgru_prep_floats(H))
    L.call("vag_cgru_prepare", W, H, L.ptr(prep.view), L.stream())
    return prep


def _untouched(out, what, tag):
    assert np.isnan(out.host(what, tag)).all(), (what + " was written by a rejected call", tag)


# ---------------------------------------------------------------------------------------------------------------- once per call
def _device_keys(inp, W, prep, B, Ts, E, H, tag):
    L = _L()
    off, total = D.keys_layout(B, Ts, E, H)
    assert L.lib().vag_cgru_decode_keys_floats(B, Ts, E, H) == total, tag
    enc, w2 = _in(inp["enc"]), _in(inp["w2"])
    keys = _Out((total,))
    L.call("vag_cgru_decode_keys", L.ptr(enc), L.ptr(prep.view), L.ptr(w2), B, Ts, E, H, L.ptr(keys.view), L.stream())
    _sync()
    flat = keys.host("keys", tag)
    return keys, flat[:B * Ts * 3 * H].reshape(B, Ts, 3 * H), flat[off:off + B * Ts * E].reshape(B, Ts, E)


def _device_tables(inp, W, V, E, H, tag):
    L = _L()
    off, total = D.tables_layout(V, E, H)
    assert L.lib().vag_cgru_decode_tables_floats(V, E, H) == total, tag
    w3 = _in(inp["w3"])
    tables = _Out((total,))
    L.call("vag_cgru_decode_tables", W, L.ptr(w3), V, E, H, L.ptr(tables.view), L.stream())
    _sync()
    flat = tables.host("tables", tag)
    return tables, flat[:V * 3 * H].reshape(V, 3 * H), flat[off:off + V * E].reshape(V, E)


@pytest.mark.parametrize("case", D.KEYS_CASES, ids=_ids)
def test_cgru_decode_keys_matches_fp64_per_element(case):
    H, E, B, Ts = case
    inp = D.keys_inputs(*case)
    W, keep = _weights(inp)
    prep = _prep(W, H)
    _, encwp, encw2 = _device_keys(inp, W, prep, B, Ts, E, H, case)
    prep.check("prep", case)
    ref = D.decode_keys(T, inp["enc"], inp["w"], inp["w2"])
    _check("decode_keys", "encwp", encwp, ref[0], case)
    _check("decode_keys", "encw2", encw2, ref[1], case)


@pytest.mark.parametrize("case", D.TABLES_CASES, ids=_ids)
def test_cgru_decode_tables_matches_fp64_per_element(case):
    H, E, V = case
    inp = D.tables_inputs(*case)
    W, keep = _weights(inp)
    _, embp, embw3 = _device_tables(inp, W, V, E, H, case)
    ref = D.decode_tables(T, inp["emb"], inp["w"], inp["w3"])
    _check("decode_tables", "embp", embp, ref[0], case)
    _check("decode_tables", "embw3", embw3, ref[1], case)


# ---------------------------------------------------------------------------------------------------------------- the hoisted step
@functools.lru_cache(maxsize=None)
def _plain_ref(key):
    return D.R.cgru_step(T, D.hstep_inputs(*key), key[3])


@pytest.mark.parametrize("tables", [0, 1], ids=["e", "tables"])
@pytest.mark.parametrize("case", D.HSTEP_CASES, ids=_ids)
def test_cgru_attn_decode_step_h_matches_fp64_per_element(case, tables):
    L = _L()
    H, E, B, rps, Ts, attn_row = case
    key = D.hstep_key(case)
    inp = D.hstep_inputs(*key)
    N, C, V = B * rps, 2 * H, D.HSTEP_V
    tag = _ids(case) + ("/tables" if tables else "")
    W, keep = _weights(inp)
    prep = _prep(W, H)
    kbuf, encwp, encw2 = _device_keys(inp, W, prep, B, Ts, E, H, tag)
    tab = _device_tables(inp, W, V, E, H, tag) if tables else None
    pe, mask, enc = _in(inp["pe"]), _in(inp["mask"]), _in(inp["enc"])
    tok, h_in = _in(inp["tok1"], torch.int64), _in(inp["h_in"])
    scratch = _Ws(L.lib().vag_cgru_step_scratch_floats(N, Ts, E, H))
    h_out, cw, alpha = _Out((N, H)), _Out((N, E)), _Out((N, Ts))
    e = None if tables else _Out((N, E))
    with _options(attn_row=attn_row):
        L.call("vag_cgru_attn_decode_step_h", L.ptr(pe), L.ptr(mask), L.ptr(kbuf.view), L.ptr(tab[0].view) if tables else None, V, rps,
               L.ptr(tok, torch.int64), L.ptr(h_in), W, L.ptr(prep.view), N, Ts, E, H, L.ptr(h_out.view), L.ptr(cw.view),
               None if tables else L.ptr(e.view), L.ptr(alpha.view), L.ptr(scratch.view), L.stream())
        _sync()
    prep.check("prep", tag)
    scratch.check("scratch", tag)
    assert _bits(kbuf.host("keys", tag)[:encwp.size], encwp.reshape(-1)), ("the step wrote its keys", tag)
    ref = D.cgru_step_h(T, inp, rps, (encwp, encw2), (tab[1], tab[2]) if tables else None)
    op = "cgru_step_h" + ("_tables" if tables else "")
    _check(op, "h_out", h_out, ref["h_out"], tag)
    cw32 = _check(op, "cw", cw, ref["cw"], tag)
    a32 = _check(op, "alpha", alpha, ref["alpha"], tag)
    on = np.repeat(inp["mask"], rps, axis=0) != 0
    assert (a32[~on] == 0.0).all(), ("weight on a masked position", tag)
    one = on.sum(1) == 1
    assert (a32[one, 0] == 1.0).all() and (a32[one, 1:] == 0.0).all(), ("a sentence of length 1", tag)
    sums = TV(ref["alpha"].v.sum(1), ref["alpha"].e.sum(1))                  # (the row sums in float64: no summation error of their own)
    assert D.ratio(a32.astype(np.float64).sum(1), sums) <= 1.0, ("a row of alpha does not sum to 1", tag)
    if tables:
        return
    assert _bits(e.host("e", tag), ref["e"]), ("e is not the gathered embedding rows", tag)
    # cross-form: the plain step on the same inputs, each form inside its own reference's bound; cw against W2 c of the plain
    # reference, the two bounds added
    h_p, c_p, e_p, a_p = _Out((N, H)), _Out((N, C)), _Out((N, E)), _Out((N, Ts))
    scr2 = _Ws(scratch.n)
    with _options(attn_row=attn_row):
        L.call("vag_cgru_attn_decode_step", L.ptr(enc), L.ptr(pe), L.ptr(mask), rps, L.ptr(tok, torch.int64), L.ptr(h_in), W,
               L.ptr(prep.view), N, Ts, E, H, L.ptr(h_p.view), L.ptr(c_p.view), L.ptr(e_p.view), L.ptr(a_p.view), L.ptr(scr2.view), L.stream())
        _sync()
    scr2.check("scratch", tag)
    plain = _plain_ref(key)
    for k, o in (("h_out", h_p), ("c", c_p), ("alpha", a_p)):
        _check("cgru_step_plain", k, o, plain[k], tag)
    w2c = T.ein("nc,ec->ne", plain["c"], inp["w2"])
    _check("cgru_step_h", "cw~W2c", cw32, TV(w2c.v, w2c.e + ref["cw"].e), tag)


# ---------------------------------------------------------------------------------------------------------------- the head
def _head_w(inp):
    L = _L()
    w = inp["w"]
    ts = [_in(w[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "out_w", "out_b")]
    return L.HeadW(*[L.ptr(t) for t in ts]), ts


def _rows_out(N, V):
    """A (N, ldl) logp / logits buffer: NaN in the real columns, the sentinel in the padding columns [V, ldl)."""
    start = np.full((N, D.ldl_of(V)), np.nan, dtype=np.float32)
    start[:, V:] = np.float32(SENTINEL)
    return _Out(start.shape, start)


def _rows_host(out, V, what, tag):
    got = out.host(what, tag)
    assert (got[:, V:] == np.float32(SENTINEL)).all(), ("a padding column of " + what + " was written", tag)
    return np.ascontiguousarray(got[:, :V])


def _i64_out(n):
    buf = torch.full((n + TAIL,), -(2 ** 40), dtype=torch.int64, device=DEV)
    return buf


def _head_call(name, inp, N, E, H, V, form, out, extra, scratch):
    """One of the five entry points on head_inputs; extra: argmax (int64 buffer or None) or parts."""
    L = _L()
    HW, keep = _head_w(inp)
    h2 = _in(inp["h2"])
    ldl = D.ldl_of(V)
    xp = (L.ptr(extra, torch.int64) if extra is not None and extra.dtype == torch.int64 else L.ptr(extra))
    if form == "plain":
        c, e = _in(inp["c"]), _in(inp["e"])
        rc = getattr(L.lib(), name)(L.ptr(h2), L.ptr(c), L.ptr(e), HW, N, E, H, V, L.ptr(out.view), ldl, xp, L.ptr(scratch.view), L.stream())
        _sync()                                                              # (the inputs above live until here)
        return rc
    cw = _in(inp["cw"])
    if form == "hoisted_e":
        e = _in(inp["e"])
        rc = getattr(L.lib(), name + "_h")(L.ptr(h2), L.ptr(cw), L.ptr(e), None, None, HW, N, E, H, V, L.ptr(out.view), ldl, xp,
                                          L.ptr(scratch.view), L.stream())
        _sync()
        return rc
    tables, tok = _in(D.tables_flat(inp, H)), _in(inp["tok"], torch.int64)
    rc = getattr(L.lib(), name + "_h")(L.ptr(h2), L.ptr(cw), None, L.ptr(tables), L.ptr(tok, torch.int64), HW, N, E, H, V,
                                      L.ptr(out.view), ldl, xp, L.ptr(scratch.view), L.stream())
    _sync()
    return rc


def _argmax_rule(logp, am, tag):
    want = np.array([int(np.nonzero(row == row.max())[0][0]) for row in logp])
    assert np.array_equal(am, want), ("argmax is not the smallest index attaining the maximum", tag, am, want)


@functools.lru_cache(maxsize=None)
def _head_ref(N, E, H, V, form):
    return D.head_form(T, D.head_inputs(N, E, H, V), H, form)


@pytest.mark.parametrize("case", D.HEAD_STEP_CASES, ids=_ids)
def test_head_logp_step_matches_fp64_per_element(case):
    N, E, H, V, form = case
    inp = D.head_inputs(N, E, H, V)
    logp, am, scratch = _rows_out(N, V), _i64_out(N), _Ws(2 * N * E)
    rc = _head_call("vag_head_logp_step", inp, N, E, H, V, form, logp, am, scratch)
    _sync()
    assert rc == 0, (rc, case)
    scratch.check("scratch", case)
    got = _rows_host(logp, V, "logp", case)
    ref = _head_ref(*case)
    _check("head_" + form, "logp", got, ref["logp"], _ids(case))
    amh = am.cpu().numpy()
    assert (amh[N:] == -(2 ** 40)).all(), ("write past argmax", case)
    _argmax_rule(got, amh[:N], case)


def test_head_argmax_takes_the_smallest_index_of_bit_equal_maxima():
    """Columns made bit-equal and the row's maximum (decode_ref.tie_columns), in the three regimes of lse_nll_kernel; the rule is
    asserted on the device's own output whether or not the copies came out bit-equal, and at least one case must show a real tie."""
    real = 0
    for (N, E, H, V) in D.TIE_CASES:
        for form in ("plain", "hoisted_e"):
            inp = D.head_inputs(N, E, H, V, ties=True)
            logp, am, scratch = _rows_out(N, V), _i64_out(N), _Ws(2 * N * E)
            rc = _head_call("vag_head_logp_step", inp, N, E, H, V, form, logp, am, scratch)
            _sync()
            assert rc == 0, (rc, V, form)
            got = _rows_host(logp, V, "logp", (V, form))
            assert np.isfinite(got).all()
            _argmax_rule(got, am.cpu().numpy()[:N], (V, form))
            ties = (got == got.max(1, keepdims=True)).sum(1)
            print("ties V=%d %s: columns attaining the maximum per row %s" % (V, form, ties.tolist()))
            real += int((ties >= 2).any())
    assert real >= 1, "no case produced two bit-equal maxima: the tie-break rule was not exercised"


@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("N,V", D.PARTS_CASES, ids=lambda x: str(x))
def test_head_logits_step_parts_recombine_to_the_log_sum_exp(N, V, form):
    L = _L()
    E, H = D.PARTS_E, D.PARTS_H
    inp = D.parts_inputs(N, V)
    tag = (N, V, form)
    HW, keep = _head_w(inp)
    cnt = L.lib().vag_head_logits_parts_count(HW, N, E, V)
    assert cnt == (V + 63) // 64, tag
    logits, parts, scratch = _rows_out(N, V), _Out((cnt, N, 2)), _Ws(2 * N * E)
    rc = _head_call("vag_head_logits_step", inp, N, E, H, V, form, logits, parts.view, scratch)
    _sync()
    assert rc == 0, (rc, tag)
    scratch.check("scratch", tag)
    x = _rows_host(logits, V, "logits", tag)
    ref = _head_ref(N, E, H, V, form)
    _check("head_" + form, "logits", x, ref["logits"], str(tag))
    p = parts.host("parts", tag)
    assert np.isfinite(p).all(), tag
    pad = np.full((N, cnt * 64), -np.inf, dtype=np.float32)
    pad[:, :V] = x
    assert _bits(p[..., 0], pad.reshape(N, cnt, 64).max(-1).T), ("m_i is not the maximum of the device's own group", tag)
    _check("parts", "s", p[..., 1], D.parts_sums_ref(x, p[..., 0]), str(tag))
    _check("parts", "lse", D.lse_from_parts(p), T.logsumexp(ref["logits"], D.PARTS_RESCALES), str(tag))


def test_head_logits_parts_count_is_zero_where_the_shape_is_not_taken():
    L = _L()
    for (N, V) in D.PARTS_NOT_TAKEN:
        HW, keep = _head_w(D.parts_inputs(N, V))
        assert L.lib().vag_head_logits_parts_count(HW, N, D.PARTS_E, V) == 0, (N, V)


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_hoisted_forms_refuse_what_they_document():
    L = _L()
    # the heads at N = 257, and tables without tok
    N, E, H, V = D.HEAD_REJECTED
    inp = D.head_inputs(N, E, H, V)
    for form in ("hoisted_e", "hoisted_tables"):
        for name in ("vag_head_logp_step", "vag_head_logits_step"):
            out, scratch = _rows_out(N, V), _Ws(2 * N * E)
            extra = _i64_out(N) if name.endswith("logp_step") else _Out((1, N, 2)).view
            assert _head_call(name, inp, N, E, H, V, form, out, extra, scratch) == EINVAL, (name, form)
            _sync()
            assert np.isnan(_rows_host(out, V, "out", (name, form))).all(), (name, form)
            assert bool((scratch.buf.view(torch.uint8) == 0xA5).all()), (name, form)
    N = 5
    inp = D.head_inputs(N, E, H, V)
    HW, keep = _head_w(inp)
    h2, cw, tables = _in(inp["h2"]), _in(inp["cw"]), _in(D.tables_flat(inp, H))
    out, scratch = _rows_out(N, V), _Ws(2 * N * E)
    rc = L.lib().vag_head_logp_step_h(L.ptr(h2), L.ptr(cw), None, L.ptr(tables), None, HW, N, E, H, V, L.ptr(out.view), D.ldl_of(V), None,
                                      L.ptr(scratch.view), L.stream())
    _sync()
    assert rc == EINVAL and np.isnan(_rows_host(out, V, "logp", "tok NULL")).all()
    # the step at N = 257 (one row per sentence, so that only the limit refuses it) and at N % rows_per_src != 0
    H, E, Ts, V = 32, 16, 5, D.HSTEP_V
    base = D.hstep_inputs(H, E, 3, 1, Ts)
    W, keep2 = _weights(base)
    prep = _prep(W, H)
    for N, rps in ((257, 1), (3, 2)):
        Bs = -(-N // rps)
        z = lambda *s: torch.zeros(*s, device=DEV)
        pe, mask = z(Bs, Ts, 2 * H), torch.ones(Bs, Ts, device=DEV)
        keys = z(D.keys_layout(Bs, Ts, E, H)[1])
        tok, h_in = torch.ones(N, dtype=torch.int64, device=DEV), z(N, H)
        h_out, cw_o, e_o, alpha = _Out((N, H)), _Out((N, E)), _Out((N, E)), _Out((N, Ts))
        scratch = _Ws(L.lib().vag_cgru_step_scratch_floats(N, Ts, E, H))
        rc = L.lib().vag_cgru_attn_decode_step_h(L.ptr(pe), L.ptr(mask), L.ptr(keys), None, V, rps, L.ptr(tok, torch.int64), L.ptr(h_in), W,
                                                 L.ptr(prep.view), N, Ts, E, H, L.ptr(h_out.view), L.ptr(cw_o.view), L.ptr(e_o.view),
                                                 L.ptr(alpha.view), L.ptr(scratch.view), L.stream())
        _sync()
        assert rc == EINVAL, (N, rps, rc)
        for o, what in ((h_out, "h_out"), (cw_o, "cw"), (e_o, "e"), (alpha, "alpha")):
            _untouched(o, what, (N, rps))
        assert bool((scratch.buf.view(torch.uint8) == 0xA5).all()), (N, rps)


def test_zz_report_worst_ratios():
    """Runs last in this file: the largest |err| / bound per operator and output on the device (shown with -s)."""
    for op, what in sorted(WORST):
        print("device worst |err| / bound  %-22s %-8s %.3f" % (op, what, WORST[(op, what)]))
