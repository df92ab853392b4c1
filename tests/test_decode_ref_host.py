"""CPU only: the tracked references of tests/decode_ref.py are HONEST (the fp32 restatement of every operator lies inside the bound, at
exactly the cases of tests/test_gpu_decode_step.py), SENSITIVE (every entry of the defect catalogue -- the restatement with one
mistake -- leaves the bound at each case at which it changes a result; no case is excused because its bound has grown), and their
inputs have the properties the cases claim (a sentence of length 1 and one of full length, lines 0 and V - 1 among the tokens, a shared
token, different tokens and states within one source sentence, tie columns that are bit-equal and the row's maximum).

Where a defect changes a result (decode_ref.hstep_defect_cases / head_defect_cases): keys_of_row_n at rows_per_src > 1 with more than
one sentence; mask_ignored_row where a position is masked (B > 1, Ts > 1); cw_from_scores at Ts > 1; the table defects with tables;
cw_without_b2 in the hoisted forms; lse_without_max_shift_of_tail in the streaming form (V = 10241), where the inputs raise
out_b[V - 1] so that the last column is the maximum of its thread's partial group (decode_ref's docstring) -- the one case whose inputs
were shaped for a defect; parts_count_padding at V % 64 != 0; everything else at every case.

With -s it prints the largest |err| / bound per operator and output (the CPU column of the table in tests/test_gpu_decode_step.py)."""
import numpy as np
import pytest

import decode_ref as D
from decode_ref import T, F, ratio

WORST = {}


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _uniq(keys):
    out = []
    for k in keys:
        if k not in out:
            out.append(k)
    return out


def _inside(op, f, t, names, tag):
    for k in names:
        q = ratio(f[k], t[k])
        WORST[(op, k)] = max(WORST.get((op, k), 0.0), q)
        assert q <= 1.0, (op, k, tag, "fp32 restatement outside the bound: %.3g" % q)


def _leaves(f, t, names):
    return max(ratio(f[k], t[k]) for k in names)


# ---------------------------------------------------------------------------------------------------------------- keys, tables
@pytest.mark.parametrize("case", D.KEYS_CASES, ids=_ids(D.KEYS_CASES))
def test_decode_keys_restatement_inside(case):
    inp = D.keys_inputs(*case)
    t = dict(zip(("encwp", "encw2"), D.decode_keys(T, inp["enc"], inp["w"], inp["w2"])))
    f = dict(zip(("encwp", "encw2"), D.decode_keys(F, inp["enc"], inp["w"], inp["w2"])))
    _inside("decode_keys", f, t, ["encwp", "encw2"], case)
    # the value is the definition's W_ih2 (W_c2h enc) whichever product is formed first
    w = {k: v.astype(np.float64) for k, v in inp["w"].items()}
    other = (inp["enc"].astype(np.float64) @ w["c2h"].T) @ w["w_ih2"].T
    assert np.abs(other - t["encwp"].v).max() <= 1e-12


@pytest.mark.parametrize("case", D.TABLES_CASES, ids=_ids(D.TABLES_CASES))
def test_decode_tables_restatement_inside(case):
    inp = D.tables_inputs(*case)
    t = dict(zip(("embp", "embw3"), D.decode_tables(T, inp["emb"], inp["w"], inp["w3"])))
    f = dict(zip(("embp", "embw3"), D.decode_tables(F, inp["emb"], inp["w"], inp["w3"])))
    _inside("decode_tables", f, t, ["embp", "embw3"], case)
    assert _leaves(dict(embp=F.ein("ve,ge->vg", inp["emb"], inp["w"]["w_ih1"])), t, ["embp"]) > 1.0          # b_ih1 left out


# ---------------------------------------------------------------------------------------------------------------- the hoisted step
HKEYS = _uniq(D.hstep_key(c) for c in D.HSTEP_CASES)
HOUT = ["h_out", "cw", "alpha"]
_H = {}


def _hstep(key):
    if key not in _H:
        H, E, B, rps, Ts = key
        inp = D.hstep_inputs(*key)
        keys = D.decode_keys(F, inp["enc"], inp["w"], inp["w2"])             # the arguments of the step: fp32, exact
        tables = D.decode_tables(F, inp["emb"], inp["w"], inp["w3"])
        _H[key] = (inp, keys, tables, {tb: D.cgru_step_h(T, inp, rps, keys, tables if tb else None) for tb in (0, 1)})
    return _H[key]


@pytest.mark.parametrize("key", HKEYS, ids=_ids(HKEYS))
def test_cgru_step_h_restatement_inside_and_inputs_as_claimed(key):
    H, E, B, rps, Ts = key
    inp, keys, tables, t = _hstep(key)
    N, V = B * rps, D.HSTEP_V
    lens = inp["mask"].sum(1).astype(int)
    assert lens[0] == Ts and (lens >= 1).all()
    if B > 1 and Ts > 1:
        assert (lens == 1).sum() == 1
    tok = inp["tok1"]
    assert tok[0] == 0 and (N < 2 or V - 1 in tok) and (N < 3 or (tok == 0).sum() == 2) and tok.min() >= 0 and tok.max() < V
    if rps > 1:
        for b in range(B):
            rows = slice(b * rps, (b + 1) * rps)
            assert len(set(tok[rows])) > 1 and not (inp["h_in"][rows] == inp["h_in"][b * rps]).all()
    for tb in (0, 1):
        f = D.cgru_step_h(F, inp, rps, keys, tables if tb else None)
        _inside("cgru_step_h" + ("_tables" if tb else ""), f, t[tb], HOUT, key)
        if tb == 0:
            assert np.array_equal(f["e"], inp["emb"][tok])
        one = np.repeat(lens, rps) == 1
        for a in (f["alpha"], t[tb]["alpha"].v):                            # a sentence of length 1: exactly 1.0 and 0.0
            assert (a[one, 0] == 1.0).all() and (a[one, 1:] == 0.0).all()
        off = np.repeat(inp["mask"], rps, axis=0) == 0
        assert (f["alpha"][off] == 0.0).all() and (t[tb]["alpha"].e[off] == 0.0).all()
        # the bound still says something: every output's bound far below the output's own range
        assert float(t[tb]["h_out"].e.max()) < 1e-3 and float(t[tb]["cw"].e.max()) < 1e-3, key
    # the other association: the hoisted gi2 path's value is the plain step's, W_p (sum alpha enc), to float64 rounding of fp32 keys
    plain = D.R.cgru_step(T, inp, rps)
    assert np.abs(plain["alpha"].v - t[0]["alpha"].v).max() <= 1e-12
    assert np.abs(plain["h_out"].v - t[0]["h_out"].v).max() <= 1e-4


@pytest.mark.parametrize("defect", D.HSTEP_DEFECTS + D.HSTEP_TABLE_DEFECTS)
def test_cgru_step_h_defects_leave_the_bound(defect):
    keys_ = D.hstep_defect_cases(defect)
    seen = 0
    for key in keys_:
        inp, keys, tables, t = _hstep(key)
        for tb in ((1,) if defect in D.HSTEP_TABLE_DEFECTS else (0, 1)):
            bad = D.cgru_step_h(F, inp, key[3], keys, tables if tb else None, defect)
            q = _leaves(bad, t[tb], HOUT)
            seen += 1
            assert q > 1.0, (defect, key, tb, q)
    print("%-28s rejected at all %d cases where it changes a result" % (defect, seen))
    assert seen >= 1 and seen == len(keys_) * (1 if defect in D.HSTEP_TABLE_DEFECTS else 2)


# ---------------------------------------------------------------------------------------------------------------- the head
HEAD_OUT = ["logits", "lse", "logp"]
_HD = {}


def _head_t(case):
    if case not in _HD:
        N, E, H, V, form = case
        _HD[case] = D.head_form(T, D.head_inputs(N, E, H, V), H, form)
    return _HD[case]


@pytest.mark.parametrize("case", D.HEAD_STEP_CASES, ids=_ids(D.HEAD_STEP_CASES))
def test_head_step_restatement_inside(case):
    N, E, H, V, form = case
    inp = D.head_inputs(N, E, H, V)
    t = _head_t(case)
    f = D.head_form(F, inp, H, form)
    _inside("head_" + form, f, t, HEAD_OUT, case)
    # the bound still says something about a log-probability: 3e-5 at the narrow head, 1.1e-4 at E = 256, H = 512 (worst-case
    # propagation of tmid's error through sum|out_w| ~ sqrt(E) / 2: the restatement sits at a few hundredths of it)
    assert float(t["logp"].e.max()) < 2e-4, case
    assert (np.exp(t["logp"].v).sum(-1) - 1.0).__abs__().max() < 1e-12
    tok = inp["tok"]
    assert 0 in tok and V - 1 in tok and (tok == 0).sum() == 2
    if V > 10240:                                                           # the streaming restatement against the plain one
        g = F.logsumexp(f["logits"], streaming=False)
        assert np.abs(g.astype(np.float64) - f["lse"]).max() <= 1e-5


@pytest.mark.parametrize("defect", D.HEAD_DEFECTS)
def test_head_step_defects_leave_the_bound(defect):
    cases = D.head_defect_cases(defect)
    for case in cases:
        N, E, H, V, form = case
        q = _leaves(D.head_form(F, D.head_inputs(N, E, H, V), H, form, defect), _head_t(case), ["logp", "lse"])
        assert q > 1.0, (defect, case, q)
    print("%-28s rejected at all %d cases where it changes a result" % (defect, len(cases)))
    assert len(cases) >= 1


@pytest.mark.parametrize("N,E,H,V", D.TIE_CASES, ids=_ids(D.TIE_CASES))
def test_tie_columns_are_bit_equal_and_the_row_maximum(N, E, H, V):
    inp = D.head_inputs(N, E, H, V, ties=True)
    x = D.head_form(F, inp, H, "plain")["logits"]
    cols = D.tie_columns(V)
    assert len(cols) >= 2 and (x[:, cols] == x[:, cols[:1]]).all() and (x.argmax(-1) == cols[0]).all()
    rest = np.delete(x, cols, axis=1)
    assert (rest.max(-1) < x[:, cols[0]]).all()


# ---------------------------------------------------------------------------------------------------------------- parts
@pytest.mark.parametrize("N,V", D.PARTS_CASES, ids=_ids(D.PARTS_CASES))
def test_parts_recombine_to_the_log_sum_exp(N, V):
    inp = D.parts_inputs(N, V)
    for form in ("plain", "hoisted_e"):
        f = D.head_form(F, inp, D.PARTS_H, form)
        t = D.head_form(T, inp, D.PARTS_H, form)
        lse_t = T.logsumexp(t["logits"], D.PARTS_RESCALES)
        parts = D.parts_of(f["logits"])
        assert parts.shape == ((V + 63) // 64, N, 2)
        q = ratio(D.lse_from_parts(parts), lse_t)
        WORST[("parts", "lse")] = max(WORST.get(("parts", "lse"), 0.0), q)
        assert q <= 1.0, (N, V, form, q)
        q = ratio(parts[..., 1], D.parts_sums_ref(f["logits"], parts[..., 0]))
        WORST[("parts", "s")] = max(WORST.get(("parts", "s"), 0.0), q)
        assert q <= 1.0, (N, V, form, q)
        assert ratio(D.lse_from_parts(parts, "parts_merged_without_rescale"), lse_t) > 1.0, (N, V, form)
        if V % 64:
            bad = D.parts_of(f["logits"], "parts_count_padding")
            assert ratio(D.lse_from_parts(bad), lse_t) > 1.0, (N, V, form)
            assert ratio(bad[..., 1], D.parts_sums_ref(f["logits"], bad[..., 0])) > 1.0, (N, V, form)


def test_layouts_and_rescale_counts():
    assert D.keys_layout(1, 1, 16, 32) == (128, 192) and D.tables_layout(19, 16, 32) == (1856, 1856 + 320)
    assert [D.stream_rescales(V) for V in (19, 10240, 10241, 4096 * 3 + 1)] == [0, 0, 4, 5]
    assert D.ldl_of(19) == 20 and D.ldl_of(2048) == 2048 and D.ldl_of(10241) == 10244


def test_zz_report_worst_ratios():
    for op, what in sorted(WORST):
        print("fp32 restatement worst |err| / bound  %-22s %-8s %.3f" % (op, what, WORST[(op, what)]))
