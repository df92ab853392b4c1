"""CPU only: the tracked references of tests/recur_ref.py are HONEST (the fp32 restatement of every operator lies inside the bound, at
exactly the cases of tests/test_gpu_recurrences.py), SENSITIVE (every entry of the defect catalogue -- the restatement with one subtle
mistake -- leaves the bound at each case listed for it: the guard against a bound that the time steps have made vacuous), and their
inputs have the properties the cases claim (lengths, unmasked positions, no one-hot softmax row, gates in their active range).

Wall time of this file: 50 s on 16 CPU threads.  With -s it prints the largest |err| / bound per operator and output (the CPU column
of the table in tests/test_gpu_recurrences.py) and at how many cases each defect changes a result (it leaves the bound at all of them)."""
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


ENC_KEYS = _uniq(R.enc_key(c) for c in R.ENC_CASES)
DEC_KEYS = _uniq(R.dec_key(c) for c in R.DEC_CASES)


def _inside(op, outs_f, outs_t, names, tag):
    for k in names:
        q = ratio(outs_f[k], outs_t[k])
        name = (op, k.replace("g_fw_", "g_").replace("g_bw_", "g_"))
        WORST[name] = max(WORST.get(name, 0.0), q)
        assert q <= 1.0, (op, k, tag, "fp32 restatement outside the bound: %.3g" % q)


def _leaves(outs_f, outs_t, names):
    return max(ratio(outs_f[k], outs_t[k]) for k in names)


# ---------------------------------------------------------------------------------------------------------------- cells
@pytest.mark.parametrize("M,H", R.CELL_FWD_CASES, ids=_ids(R.CELL_FWD_CASES))
def test_gru_cell_fwd_restatement_inside_defects_outside(M, H):
    inp = R.cell_inputs(M, H)
    t = R.cell_fwd(T, inp)
    _inside("gru_cell_fwd", R.cell_fwd(F, inp), t, ["h_out", "save"], (M, H))
    for d in R.CELL_DEFECTS:
        assert _leaves(R.cell_fwd(F, inp, d), t, ["h_out"]) > 1.0, (d, M, H)
    r, z = t["save"].v[0], t["save"].v[1]
    for g in (r, z):
        assert ((g > 0.1) & (g < 0.9)).mean() >= 0.2


@pytest.mark.parametrize("M,H", R.CELL_BWD_CASES, ids=_ids(R.CELL_BWD_CASES))
def test_gru_cell_bwd_restatement_inside_defects_outside(M, H):
    inp = R.cell_inputs(M, H)
    save = R.cell_fwd(F, inp)["save"]
    t = R.gru_cell_bwd(T, inp, save)
    _inside("gru_cell_bwd", R.gru_cell_bwd(F, inp, save), t, ["dgi", "dgh", "carry_out"], (M, H))
    assert _leaves(R.gru_cell_bwd(F, inp, save, "carry_dropped"), t, ["dgi", "carry_out"]) > 1.0


# ---------------------------------------------------------------------------------------------------------------- encoder
ENC_OUT = ["g_emb"] + ["g_%s_%s" % (d, p) for d in ("fw", "bw") for p in ("w_ih", "w_hh", "b_ih", "b_hh")]
_ENC_T = {}


def _enc_t(key):
    if key not in _ENC_T:
        inp = R.enc_inputs(*key)
        fwd = R.bigru_fwd(T, inp)
        _ENC_T[key] = (inp, fwd, R.bigru_bwd(T, inp, fwd))
    return _ENC_T[key]


@pytest.mark.parametrize("key", ENC_KEYS, ids=_ids(ENC_KEYS))
def test_bigru_restatement_inside_and_inputs_as_claimed(key):
    inp, fwd_t, bwd_t = _enc_t(key)
    H, E, B, Ts, p_emb, p_ctx, full = key
    fwd_f = R.bigru_fwd(F, inp)
    _inside("bigru_fwd", fwd_f, fwd_t, ["enc"], key)
    _inside("bigru_bwd", R.bigru_bwd(F, inp, fwd_f), bwd_t, ENC_OUT, key)
    lens = inp["lens"]
    assert lens[0] == Ts and (np.diff(lens) <= 0).all() and ((inp["src"] != 0).sum(1) == lens).all()
    if B > 1 and Ts > 1 and not full:
        assert (lens == 1).any() and (B < 4 or (np.bincount(lens) >= 2).any()), lens
    assert R.ENC_NEVER not in inp["src"] and R.ENC_VS - 1 in inp["src"]
    for b, n in enumerate(lens):                                             # exactly 0, with a bound of 0, past a row's length
        assert (fwd_t["enc"].v[b, n:] == 0).all() and (fwd_t["enc"].e[b, n:] == 0).all()
        assert (fwd_f["enc"][b, n:] == 0).all()
    for steps in fwd_t["steps"]:
        for g in (0, 1):
            vals = np.concatenate([st["save"][g].v[st["live"][:, 0]].ravel() for st in steps])
            assert ((vals > 0.1) & (vals < 0.9)).mean() >= 0.2


@pytest.mark.parametrize("defect", R.ENC_FWD_DEFECTS + R.ENC_BWD_DEFECTS)
def test_bigru_defects_leave_the_bound(defect):
    keys = R.enc_defect_cases(defect)
    seen = 0
    for key in keys:
        inp, fwd_t, bwd_t = _enc_t(key)
        if defect in R.ENC_FWD_DEFECTS:
            q = _leaves(R.bigru_fwd(F, inp, defect), fwd_t, ["enc"])
        else:
            q = _leaves(R.bigru_bwd(F, inp, R.bigru_fwd(F, inp), defect), bwd_t, ENC_OUT)
        seen += 1
        assert q > 1.0, (defect, key, q)
    print("%-28s rejected at all %d cases where it changes a result" % (defect, seen))
    assert seen == len(keys) and seen >= 1, defect


def test_bigru_scatter_into_the_pad_row_would_add_zeros_only():
    """Why "g_emb[0] is touched" is a decoder entry of the catalogue only: the encoder's padded steps carry dgi = 0."""
    for key in ENC_KEYS[:4]:
        inp, fwd_t, bwd_t = _enc_t(key)
        ff = R.bigru_fwd(F, inp)
        a, b = R.bigru_bwd(F, inp, ff)["g_emb"], R.bigru_bwd(F, inp, ff, "g_emb0_touched")["g_emb"]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and (inp["src"] == 0).any() == (key[2] > 1 and key[3] > 1)


def test_dropout_words_are_multipliers_at_the_stated_rate():
    m = R.drop_mask(R.RNG_STATE, 2, 1 << 16, 0.5)
    assert set(np.unique(m)) == {np.float32(0.0), np.float32(2.0)} and abs((m == 0).mean() - 0.5) < 0.01
    m = R.drop_mask(R.RNG_STATE, 1, 1 << 16, 0.3)
    assert abs((m == 0).mean() - 0.3) < 0.01 and m.max() == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    assert (R.drop_mask(R.RNG_STATE, 1, 64, 0.3) != R.drop_mask(R.RNG_STATE, 2, 64, 0.3)).any()


# ---------------------------------------------------------------------------------------------------------------- decoder
FWD_ONLY = {R.dec_key(c) for c in R.DEC_CASES if c.fwd_only}
DEC_OUT = ["d_enc_out", "d_pe", "d_h0", "g_emb"] + ["g_" + n for n in R.DEC_W_NAMES[1:]]
_DEC = {}


def _dec(key, acc=0, with_d_e=True):
    k = (key, acc, with_d_e)
    if k not in _DEC:
        inp = R.dec_inputs(*key)
        fwd_f = R.cgru_fwd(F, inp)
        fwd_t = R.cgru_fwd(T, inp)
        h2, c, e = fwd_f["h2_all"], fwd_f["c_all"], fwd_f["e_all"]          # the forward's own outputs: exact arguments of the backward
        rec_t = R.cgru_fwd(T, inp, h2_given=h2)
        bwd_t = None if key in FWD_ONLY else R.cgru_bwd(T, inp, rec_t, c, e, acc, with_d_e)
        _DEC[k] = (inp, fwd_f, fwd_t, bwd_t, rec_t)
    return _DEC[k]


def _dec_bwd_f(inp, fwd_f, acc=0, with_d_e=True, defect=None):
    rec = R.cgru_fwd(F, inp, h2_given=fwd_f["h2_all"])
    return R.cgru_bwd(F, inp, rec, fwd_f["c_all"], fwd_f["e_all"], acc, with_d_e, defect)


@pytest.mark.parametrize("key", DEC_KEYS, ids=_ids(DEC_KEYS))
def test_cgru_restatement_inside_and_inputs_as_claimed(key):
    H, E, B, Ts, Tt = key
    variants = _uniq((c.acc, c.d_e) for c in R.DEC_CASES if R.dec_key(c) == key)
    for acc, with_d_e in variants:
        inp, fwd_f, fwd_t, bwd_t, rec_t = _dec(key, acc, with_d_e)
        _inside("cgru_fwd", fwd_f, fwd_t, ["h2_all", "c_all"], key)
        assert np.array_equal(fwd_f["e_all"], fwd_t["e_all"])
        _inside("cgru_fwd_step", fwd_f, rec_t, ["h2_all", "c_all"], key)        # each step from the forward's own previous state
        if bwd_t is not None:
            _inside("cgru_bwd" + R.dec_group(H), _dec_bwd_f(inp, fwd_f, acc, with_d_e), bwd_t, DEC_OUT, key + (acc, with_d_e))
    lens = inp["mask"].sum(1)
    assert lens[0] == Ts and (lens >= 1).all()                               # every attention row has an unmasked position
    if B > 1 and Ts > 1:
        assert (lens == 1).any() and (B < 4 or (np.bincount(lens.astype(int)) >= 2).any())
    for st in fwd_t["steps"]:
        a32 = st["alpha"].v.astype(np.float32)
        many = lens > 1
        assert (a32[many].max(1) < 1.0).all(), "a softmax row that is one-hot to fp32"
        for s in (st["s1"], st["s2"]):
            for g in (0, 1):
                assert ((s[g].v > 0.1) & (s[g].v < 0.9)).mean() >= 0.2
    # the one-step bound is sharp at every step: never more than a tenth of a state's range, where the free-running one passes it
    assert max(float(rec_t["h2_all"].e[t].max()) for t in range(Tt)) < 1e-3, key
    if bwd_t is None:
        return
    got = bwd_t["g_emb"].v
    assert np.array_equal(got[R.DEC_NEVER], inp["g_emb0"][R.DEC_NEVER].astype(np.float64)) and (bwd_t["g_emb"].e[R.DEC_NEVER] == 0).all()
    assert np.array_equal(got[0], inp["g_emb0"][0].astype(np.float64)) and (bwd_t["g_emb"].e[0] == 0).all()


@pytest.mark.parametrize("defect", R.DEC_FWD_DEFECTS + R.DEC_BWD_DEFECTS)
def test_cgru_defects_leave_the_bound(defect):
    keys = R.dec_defect_cases(defect)
    seen = 0
    for key in keys:
        acc = 1 if defect == "accumulate_enc_ignored" else 0
        inp, fwd_f, fwd_t, bwd_t, rec_t = _dec(key, acc, True)
        if defect in R.DEC_FWD_DEFECTS:
            bad = R.cgru_fwd(F, inp, defect=defect)
            if defect == "stale_h2_at_late_step":                            # wrong from step 2 on only: the one-step reference's to catch
                q = _leaves(bad, R.cgru_fwd(T, inp, h2_given=bad["h2_all"]), ["h2_all", "c_all"])
            else:                                                            # the others show in step 0: the free-running reference
                q = _leaves(bad, fwd_t, ["h2_all", "c_all"])
        else:
            q = _leaves(_dec_bwd_f(inp, fwd_f, acc, True, defect), bwd_t, DEC_OUT)
        seen += 1
        assert q > 1.0, (defect, key, q)
    print("%-28s rejected at all %d cases where it changes a result" % (defect, seen))
    assert seen == len(keys) and seen >= 1, defect


# ---------------------------------------------------------------------------------------------------------------- step, attention
@pytest.mark.parametrize("H,rps", R.STEP_CASES, ids=_ids(R.STEP_CASES))
def test_cgru_step_restatement_inside_defects_outside(H, rps):
    inp = R.step_inputs(H, rps)
    t = R.cgru_step(T, inp, rps)
    names = ["h_out", "c", "alpha"]
    _inside("cgru_step", R.cgru_step(F, inp, rps), t, names, (H, rps))
    for d in R.STEP_DEFECTS:
        if d == "source_row_not_divided" and rps == 1:
            continue
        assert _leaves(R.cgru_step(F, inp, rps, d), t, names) > 1.0, (d, H, rps)
    # the two associations of one product: the value of the sequence operator's gi2 path and of the step's agree to float64 rounding
    w = inp["w"]
    c = t["c"].v
    a = (c @ w["c2h"].astype(np.float64).T) @ w["w_ih2"].astype(np.float64).T
    b = c @ (w["w_ih2"].astype(np.float64) @ w["c2h"].astype(np.float64)).T
    assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("H,rps,Ts", R.ATTN_CASES, ids=_ids(R.ATTN_CASES))
def test_bahdanau_attn_restatement_inside_defects_outside(H, rps, Ts):
    inp = R.attn_inputs(H, rps, Ts)
    t = R.bahdanau_attn(T, inp, rps)
    names = ["scores", "alpha", "ctx"]
    f = R.bahdanau_attn(F, inp, rps)
    on = np.repeat(inp["mask"], rps, axis=0) != 0
    _inside("bahdanau", f, t, ["alpha", "ctx"], (H, rps, Ts))
    _inside("bahdanau", dict(scores=f["scores"][on]), dict(scores=R.TV(t["scores"].v[on], t["scores"].e[on])), ["scores"],
            (H, rps, Ts))                                                    # (a masked score is the kernel's own stand-in for -inf)
    assert (t["alpha"].v[~on] == 0).all()
    if Ts > 1:
        assert _leaves(R.bahdanau_attn(F, inp, rps, "mask_ignored_row"), t, ["alpha", "ctx"]) > 1.0
        assert (t["alpha"].v.astype(np.float32).max(1) < 1.0).all()


def test_mark_budget_is_one_unit_in_the_last_place():
    x = np.array([0.5, -0.3, 1.0, 1e-3, 0.75 + 2.0 ** -23], dtype=np.float32)
    m = F.mark(x)
    assert (m.view(np.uint32) & 1 == 1).all()
    assert ratio(m, T.mark(x)) <= 1.0 and (np.abs(m.astype(np.float64) - x) <= R.ULP * np.abs(x)).all()
    assert (T.mark(x).e == R.ULP * np.abs(x.astype(np.float64))).all()


def test_lds_limit_of_the_one_launch_decoder_is_the_case_tables():
    assert R.DEC_MAX_TS == 48 and R.dec_lds_bytes(48) <= 160 * 1024 < R.dec_lds_bytes(49)
    assert any(c.Ts == R.DEC_MAX_TS and c.one_launch for c in R.DEC_CASES)
    assert any(c.Ts == R.DEC_MAX_TS + 1 and not c.one_launch for c in R.DEC_CASES)


def test_zz_report_worst_ratios():
    for op, what in sorted(WORST):
        print("fp32 restatement worst |err| / bound  %-16s %-12s %.3f" % (op.replace(" ", "_"), what, WORST[(op, what)]))
