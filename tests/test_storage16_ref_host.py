"""CPU only: the 2-byte storage mode of tests/recur_ref.py (storage = 1), at exactly the cases of tests/test_gpu_storage16.py.

HONEST: the fp32 restatement F with the mode's roundings (numpy.float16, the two-plane split) lies inside the tracked bound of T for
every output.  SENSITIVE: every entry of the defect catalogue that applies to a case leaves the bound there -- the condition that makes
the mode's looser bounds (2^-11 per rounded operand where fp32 has 2^-24) worth testing against.  IN RANGE: nothing that is rounded to
fp16 passes 65504, gate gradients times 2^12 included, on the reference's own widened values.  UNCHANGED: storage = 0 through the new
argument reproduces the fp32 reference bit for bit.  PLANNED: every dense product the reference planned alone takes, by the library's
host-only vag_gemm_plan in the mode's context, the kernel family whose rule the reference applied.

With -s: the largest |err| / bound per operator and output (the host column of the table in tests/test_gpu_storage16.py) and at how
many cases each defect was rejected.  Wall time of this file: 58 s on 16 CPU threads."""
import ctypes as C

import numpy as np
import pytest

import recur_ref as R
from recur_ref import T, F, ratio

WORST = {}


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _uniq(keys):
    out = []
    for k in keys:
        if k not in out:
            out.append(k)
    return out


ENC_KEYS = _uniq(R.enc_key(c) for c in R.ENC16_CASES)
ENC_OUT = ["g_emb"] + ["g_%s_%s" % (d, p) for d in ("fw", "bw") for p in ("w_ih", "w_hh", "b_ih", "b_hh")]
_ENC_T = {}


def _enc_t(key):
    if key not in _ENC_T:
        inp = R.enc16_inputs(*key)
        R.F16_PEAK[0] = 0.0
        fwd = R.bigru_fwd(T, inp, storage=1)
        fwd_f = R.bigru_fwd(F, inp, storage=1)
        ws = R.bigru_ws_arrays(F, fwd_f)                                     # what the restatement's forward saved: exact from here on
        bwd = R.bigru_bwd(T, inp, R.bigru_saved(T, inp, *ws), storage=1)
        _ENC_T[key] = (inp, fwd, bwd, R.F16_PEAK[0], fwd_f, ws)
    return _ENC_T[key]


def _inside(op, outs_f, outs_t, names, tag):
    for k in names:
        q = ratio(outs_f[k], outs_t[k])
        name = (op, k.replace("g_fw_", "g_").replace("g_bw_", "g_"))
        WORST[name] = max(WORST.get(name, 0.0), q)
        assert q <= 1.0, (op, k, tag, "restatement outside the bound: %.3g" % q)


def _leaves(outs_f, outs_t, names):
    return max(ratio(outs_f[k], outs_t[k]) for k in names)


# ---------------------------------------------------------------------------------------------------------------- the rules themselves
def test_f16_rule_on_exact_and_on_tracked_values():
    x = np.array([0.1, -0.3, 1.0, 3.0e-5, 6.0e-8, 2.0 ** -14, 1000.5, 0.0], dtype=np.float32)
    t = T.f16(x)                                                             # exact data: the fp16 value, bound 0
    assert (t.e == 0).all() and np.array_equal(t.v, x.astype(np.float16).astype(np.float64))
    assert np.array_equal(F.f16(x), x.astype(np.float16).astype(np.float32))
    e = np.abs(x.astype(np.float64)) * 2.0 ** -20 + 1e-12                   # a tracked quantity: value kept, half an fp16 ulp more
    t = T.f16(R.TV(x, e))
    assert np.array_equal(t.v, x.astype(np.float64))
    assert np.array_equal(t.e, e + np.maximum(2.0 ** -11 * (np.abs(x) + e), 2.0 ** -25))
    rs = np.random.RandomState(5)
    for scale in (1.0, R.GSCALE):                                            # any fp32 within e of v rounds to within the new bound
        v = (rs.randn(4096) * 10.0 ** rs.uniform(-9, 0, 4096)).astype(np.float32)
        err = np.abs(v.astype(np.float64)) * 2.0 ** -12
        seen = (v.astype(np.float64) + err * rs.uniform(-1, 1, 4096)).astype(np.float32)
        ok = np.abs(seen.astype(np.float64) - v) <= err
        assert ratio(F.f16(seen, scale)[ok], R.TV(v[ok], T.f16(R.TV(v, err), scale).e[ok])) <= 1.0
    tiny = np.float32(3.0e-9)                                                # the scale keeps what the unscaled rounding flushes
    assert F.f16(tiny) == 0.0 and abs(float(F.f16(tiny, R.GSCALE)) - 3.0e-9) < 3.0e-9 * 2.0 ** -10


def test_two_plane_rule_holds_the_split_and_rejects_one_plane():
    rs = np.random.RandomState(6)
    a, b = R._uni(rs, 70, 300), R._uni(rs, 90, 300)
    x1, x2 = R._bf16_planes(a)
    assert (np.abs(a - x1) <= 2.0 ** -8 * np.abs(a)).all() and (np.abs(a.astype(np.float64) - x1 - x2) <= 2.0 ** -16 * np.abs(a)).all()
    assert ((x1.view(np.uint32) | x2.view(np.uint32)) & 0xFFFF == 0).all()
    t = T.ein2p("mk,nk->mn", a, b)
    assert ratio(F.ein2p("mk,nk->mn", a, b), t) <= 1.0
    assert ratio(F.ein("mk,nk->mn", x1, R._bf16(b)), t) > 1.0                # one plane per operand is outside
    assert ratio(F.ein2p("mk,nk->mn", a, b), T.ein("mk,nk->mn", a, b)) > 1.0  # ... and two planes are outside the fp32 rule


def test_storage0_through_the_new_argument_is_the_fp32_reference_bit_for_bit():
    for c in (R.ENC_CASES[0], R.ENC_CASES[7]):
        inp = R.enc_inputs(*R.enc_key(c))
        for A in (T, F):
            a, b = R.bigru_fwd(A, inp), R.bigru_fwd(A, inp, storage=0)
            ga, gb = R.bigru_bwd(A, inp, a), R.bigru_bwd(A, inp, b, storage=0)
            gs = R.bigru_bwd(A, inp, R.bigru_saved(A, inp, *R.bigru_ws_arrays(A, a)))        # the saved form changes nothing either
            for k in ENC_OUT:
                assert np.array_equal(A.value(ga[k]), A.value(gs[k]))
            for x, y in [(a["enc"], b["enc"])] + [(ga[k], gb[k]) for k in ENC_OUT]:
                for p, q in ((x.v, y.v), (x.e, y.e)) if A is T else ((x, y),):
                    assert p.dtype == q.dtype and np.array_equal(p.view(np.uint8), q.view(np.uint8))
    inp = R.keys16_inputs(48, 64)
    plain = T.ein("rc,dc->rd", inp["enc"], inp["attn_e"])
    got = R.attn_keys_proj(T, inp, storage=0)["pe"]
    assert np.array_equal(got.v, plain.v) and np.array_equal(got.e, plain.e)


# ---------------------------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize("rows,C", R.KEYS16_CASES, ids=_ids(R.KEYS16_CASES))
def test_keys_restatement_inside_defects_outside_in_range(rows, C):
    inp = R.keys16_inputs(rows, C)
    R.F16_PEAK[0] = 0.0
    t = R.attn_keys_proj(T, inp, storage=1)
    assert 0.0 < R.F16_PEAK[0] < R.F16_MAX
    _inside("keys_proj", R.attn_keys_proj(F, inp, storage=1), t, ["pe"], (rows, C))
    for d in R.KEYS16_DEFECTS:
        assert _leaves(R.attn_keys_proj(F, inp, storage=1, defect=d), t, ["pe"]) > 1.0, (d, rows, C)


# ---------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("key", ENC_KEYS, ids=_ids(ENC_KEYS))
def test_bigru16_restatement_inside_in_range_and_inputs_as_claimed(key):
    inp, fwd_t, bwd_t, peak, fwd_f, ws = _enc_t(key)
    H, E, B, Ts, p_emb, p_ctx, full = key
    assert 0.0 < peak < R.F16_MAX, (key, peak)
    _inside("bigru16_fwd", fwd_f, fwd_t, ["enc"], key)
    gates_t, hst_t = R.bigru_ws_arrays(T, fwd_t)
    _inside("bigru16_fwd", dict(gates=ws[0], hst=ws[1]), dict(gates=gates_t, hst=hst_t), ["gates", "hst"], key)
    _inside("bigru16_bwd", R.bigru_bwd(F, inp, R.bigru_saved(F, inp, *ws), storage=1), bwd_t, ENC_OUT, key)
    lens = inp["lens"]
    assert lens[0] == Ts and (np.diff(lens) <= 0).all() and (lens == 1).any()
    if B > 64:
        assert lens[63] != lens[B - 1]
    for b, n in enumerate(lens):
        assert (fwd_t["enc"].v[b, n:] == 0).all() and (fwd_t["enc"].e[b, n:] == 0).all()
    # the gate gradients the kernels scale are small enough for the scale to matter, and far from fp16's top once scaled
    for steps in fwd_t["steps"]:
        for g in (0, 1):
            vals = np.concatenate([st["save"][g].v[st["live"][:, 0]].ravel() for st in steps])
            assert ((vals > 0.1) & (vals < 0.9)).mean() >= 0.2
    assert np.abs(inp["d_enc"]).max() <= R.GRAD16 < 2.0 ** -14


@pytest.mark.parametrize("defect", _uniq(R.ENC16_FWD_DEFECTS + R.ENC16_BWD_DEFECTS))
def test_bigru16_defects_leave_the_bound(defect):
    keys = R.enc16_defect_cases(defect)
    seen = 0
    for key in keys:
        inp, fwd_t, bwd_t, _, fwd_f, ws = _enc_t(key)
        if defect in R.ENC16_FWD_DEFECTS:
            q = _leaves(R.bigru_fwd(F, inp, defect, storage=1), fwd_t, ["enc"])
            assert q > 1.0, (defect, "forward", key, q)
        if defect in R.ENC16_BWD_DEFECTS:
            q = _leaves(R.bigru_bwd(F, inp, R.bigru_saved(F, inp, *ws), defect, storage=1), bwd_t, ENC_OUT)
            assert q > 1.0, (defect, "backward", key, q)
        seen += 1
    print("%-32s rejected at all %d cases where it changes a result" % (defect, seen))
    assert seen == len(keys) and seen >= 1, defect


def test_no_case_is_left_out_of_the_defect_check():
    every = set(ENC_KEYS)
    for d in ("blend_swapped", "bhn_outside", "k_tail_segment_dropped", "carry_dropped_at_step", "g_overwritten", "grad_scale_missing",
              "fp16_copy_transposed_wrong"):
        assert set(R.enc16_defect_cases(d)) == every, d
    assert any(k[2] > 64 for k in R.enc16_defect_cases("group_tail_takes_len_of_row63"))
    assert any(k[2] > 16 for k in R.enc16_defect_cases("tile2_takes_len_of_row15"))


# ---------------------------------------------------------------------------------------------------------------- decoder forward
DEC_KEYS = _uniq([c[:5] for c in R.DEC16_CASES] + [c[:5] for c in R.DEC16_BWD_CASES])
DEC_OUT = ["h2_all", "c_all"] + R.DEC_WS
_DEC = {}


def _with_ws(A, fwd):
    return dict(fwd, **R.cgru_ws_arrays(A, fwd))


def _dec(key):
    if key not in _DEC:
        inp = dict(R.dec16_inputs(*key))
        B, Ts, Cw = inp["enc"].shape
        R.F16_PEAK[0] = 0.0
        inp["pe"] = R.attn_keys_proj(F, R.dec16_keys_inputs(inp), storage=1)["pe"].reshape(B, Ts, Cw)    # the restatement's own stored keys
        fwd_f = _with_ws(F, R.cgru_fwd(F, inp, storage=1))
        rec_t = _with_ws(T, R.cgru_fwd(T, inp, h2_given=fwd_f["h2_all"], storage=1))
        peak = R.F16_PEAK[0]                                                 # (the one-step reference's: its values are sharp at every step)
        fwd_t = R.cgru_fwd(T, inp, storage=1)
        _DEC[key] = (inp, fwd_f, fwd_t, rec_t, peak)
    return _DEC[key]


@pytest.mark.parametrize("key", DEC_KEYS, ids=_ids(DEC_KEYS))
def test_cgru16_forward_restatement_inside_and_in_range(key):
    H, E, B, Ts, Tt = key
    inp, fwd_f, fwd_t, rec_t, peak = _dec(key)
    assert 0.0 < peak < R.F16_MAX, (key, peak)
    assert np.array_equal(inp["pe"], inp["pe"].astype(np.float16).astype(np.float32))
    _inside("cgru16_fwd", fwd_f, fwd_t, ["h2_all", "c_all"], key)
    assert np.array_equal(fwd_f["e_all"], fwd_t["e_all"])
    _inside("cgru16_step", fwd_f, rec_t, DEC_OUT, key)
    # the one-step bound stays a small part of a state's range at every step, where the free-running one passes it
    assert max(float(rec_t["h2_all"].e[t].max()) for t in range(Tt)) < 0.02, key
    lens = inp["mask"].sum(1)
    assert lens[0] == Ts and (lens == 1).any()


@pytest.mark.parametrize("defect", R.DEC16_FWD_DEFECTS)
def test_cgru16_forward_defects_leave_the_one_step_bound(defect):
    keys = R.dec16_defect_cases(defect)
    for key in keys:
        inp, fwd_f, fwd_t, rec_t, _ = _dec(key)
        bad = _with_ws(F, R.cgru_fwd(F, inp, defect=defect, storage=1))
        ref = _with_ws(T, R.cgru_fwd(T, inp, h2_given=bad["h2_all"], storage=1))
        q = _leaves(bad, ref, DEC_OUT)
        assert q > 1.0, (defect, key, q)
    print("%-32s rejected at all %d cases where it changes a result" % (defect, len(keys)))
    assert len(keys) >= 4 and (defect == "stale_h2_at_late_step" or len(keys) == len(R.DEC16_CASES))


def test_storage0_decoder_is_unchanged_by_the_new_argument():
    for c in (R.DEC_CASES[0], R.DEC_CASES[4]):
        inp = R.dec_inputs(*R.dec_key(c))
        for A in (T, F):
            a, b = R.cgru_fwd(A, inp), R.cgru_fwd(A, inp, storage=0)
            for k in ("h2_all", "c_all"):
                assert np.array_equal(A.value(a[k]), A.value(b[k])) and (A is F or np.array_equal(a[k].e, b[k].e))
            h2, c_all, e_all = (R.F.value(R.cgru_fwd(F, inp)[k]).astype(np.float32) for k in ("h2_all", "c_all", "e_all"))
            ga = R.cgru_bwd(A, inp, R.cgru_fwd(A, inp, h2_given=h2), c_all, e_all)
            gb = R.cgru_bwd(A, inp, R.cgru_fwd(A, inp, h2_given=h2, storage=0), c_all, e_all, storage=0)
            for k in DEC_BWD_OUT:
                assert np.array_equal(A.value(ga[k]), A.value(gb[k])) and (A is F or np.array_equal(ga[k].e, gb[k].e))


# ---------------------------------------------------------------------------------------------------------------- decoder backward
DEC_BWD_OUT = ["d_enc_out", "d_pe", "d_h0", "g_emb"] + ["g_" + n for n in R.DEC_W_NAMES[1:]]
_DECB = {}


def _decb(c):
    if c not in _DECB:
        inp, fwd_f, _, rec_t, _ = _dec(c[:5])
        ws = R.cgru_ws_saved(F, fwd_f)                                       # what the restatement's forward saved: exact from here on
        R.F16_PEAK[0] = 0.0
        bwd_t = R.cgru_bwd(T, inp, R.cgru_saved(T, inp, fwd_f["h2_all"], ws), fwd_f["c_all"], fwd_f["e_all"], c.acc, c.d_e, storage=1)
        _DECB[c] = (inp, fwd_f, ws, bwd_t, R.F16_PEAK[0], rec_t)
    return _DECB[c]


def _decb_f(c, defect=None):
    inp, fwd_f, ws, _, _, _ = _decb(c)
    return R.cgru_bwd(F, inp, R.cgru_saved(F, inp, fwd_f["h2_all"], ws), fwd_f["c_all"], fwd_f["e_all"], c.acc, c.d_e, defect=defect, storage=1)


@pytest.mark.parametrize("case", R.DEC16_BWD_CASES, ids=_ids([c[:8] for c in R.DEC16_BWD_CASES]))
def test_cgru16_backward_restatement_inside_and_in_range(case):
    inp, fwd_f, ws, bwd_t, peak, rec_t = _decb(case)
    assert 0.0 < peak < R.F16_MAX, (case, peak)
    _inside("cgru16_bwd", _decb_f(case), bwd_t, DEC_BWD_OUT, case[:8])
    saved_t = R.cgru_ws_saved(T, rec_t)                                      # the saved tensors are held to the one-step forward reference
    _inside("cgru16_step", {"ws_" + k: v for k, v in ws.items()}, {"ws_" + k: v for k, v in saved_t.items()}, ["ws_" + k for k in ws], case[:8])
    got = bwd_t["g_emb"]
    for r in (0, R.DEC_NEVER):
        assert np.array_equal(got.v[r], inp["g_emb0"][r].astype(np.float64)) and (got.e[r] == 0).all()
    assert max(np.abs(inp[k]).max() for k in ("d_h2", "d_c", "d_e")) <= R.GRAD16


@pytest.mark.parametrize("defect", R.DEC16_BWD_DEFECTS)
def test_cgru16_backward_defects_leave_the_bound(defect):
    cases = R.dec16_bwd_defect_cases(defect)
    for c in cases:
        q = _leaves(_decb_f(c, defect), _decb(c)[3], DEC_BWD_OUT)
        assert q > 1.0, (defect, c[:8], q)
    print("%-32s rejected at all %d cases where it changes a result" % (defect, len(cases)))
    always = defect not in ("carry_dropped_at_step", "g_emb0_touched", "accumulate_enc_ignored", "d_e_all_ignored")
    assert len(cases) >= 2 and (not always or len(cases) == len(R.DEC16_BWD_CASES))


# ---------------------------------------------------------------------------------------------------------------- planner
def test_zy_planned_products_take_the_family_the_reference_assumed():
    """Runs after the cases above have filled R.PRODUCTS16 (and fills it itself when run alone)."""
    from vagnmt_hip import _lib
    L = _lib.lib()
    for key in ENC_KEYS:
        _enc_t(key)
    for c in R.KEYS16_CASES:
        R.attn_keys_proj(T, R.keys16_inputs(*c), storage=1)
    for key in DEC_KEYS:
        _dec(key)
    out = (C.c_int * 6)()
    assert L.vag_set_operator_context(C.c_void_p(4096), 1) == 0              # (never dereferenced by the planner)
    try:
        for M, N, K, beta, c_half, tile in sorted(R.PRODUCTS16):
            assert L.vag_gemm_plan(M, N, K, 1, 1, 1, beta, 0, c_half, 0, 0, 0, out) == 0
            assert (out[0], out[1]) == ((0, 64) if tile == 64 else (2, 128)), ((M, N, K, beta, c_half), list(out), tile)
    finally:
        assert L.vag_set_operator_context(None, 0) == 0
    tiles = {p[5] for p in R.PRODUCTS16}
    assert tiles == {64, 128}                                                # both families are reached by products planned alone
    assert any(p[4] == 1 and p[5] == 128 for p in R.PRODUCTS16)              # ... the fp16 epilogue on the plane kernel among them


def test_zz_report_worst_ratios():
    for op, what in sorted(WORST):
        print("restatement worst |err| / bound  %-16s %-12s %.3f" % (op, what, WORST[(op, what)]))
