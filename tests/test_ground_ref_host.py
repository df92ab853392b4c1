"""CPU: the tracked float64 references of tests/ground_ref.py, at every case tests/test_gpu_ground_ops.py runs on the device.

  * honest bound    -- the fp32 restatement of each operator (the same formula in np.float32) lies inside the tracked bound,
                       element by element;
  * sensitive bound -- every entry of the defect catalogue (the restatement with one subtle mistake) leaves the bound on at least
                       one element of at least one case of its operator;
  * input conditions, asserted on the reference alone: ranking-loss cases with B >= 16 have 20 .. 80 % of their hinges active and no
    case has an ambiguous hinge (|argument| <= its own tracked bound); every attention row has an unmasked position; no softmax
    input lies outside [-30, 30].

The largest |fp32 restatement - value| / err per operator is printed by the last test (`-s`) and recorded, next to the device's, in
the docstring of tests/test_gpu_ground_ops.py."""
import functools

import numpy as np
import pytest

import ground_ref as R

WORST = {}


def _note(op, name, got, ref):
    q = R.ratio(got, ref)
    WORST[op] = max(WORST.get(op, 0.0), q)
    assert q <= 1.0, (op, name, "fp32 restatement outside the tracked bound: |err| / bound = %.3g" % q)


def _outside(got, ref):
    return R.ratio(got, ref) > 1.0


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("E,n", R.EMBED_CASES, ids=_ids(R.EMBED_CASES))
def test_embedding_bound_is_honest(E, n):
    inp = R.embed_inputs(E, n)
    ref = R.embed_bwd_ref(inp)
    _note("embed_bwd", "g_W", R.embed_bwd_f32(inp), ref)
    assert (ref.e[0] == 0).all() and (ref.e[R.EMBED_NEVER] == 0).all()          # the pad row and the unnamed row: exact
    assert (inp["idx"] == 0).sum() >= (3 if n > 1 else 0) and (n < 300 or np.bincount(inp["idx"]).max() >= 64)


@pytest.mark.parametrize("defect", R.EMBED_DEFECTS)
def test_embedding_bound_is_sensitive(defect):
    hits = [c for c in R.EMBED_CASES if _outside(R.embed_bwd_f32(R.embed_inputs(*c), defect), R.embed_bwd_ref(R.embed_inputs(*c)))]
    assert hits, defect


# ---------------------------------------------------------------------------------------------------------------- l2norm, projections
def _l2_run(B, S, defect=None):
    inp = R.l2_inputs(B, S)
    n32, o32 = R.l2norm_fwd(R.F32, inp["x"])
    fwd = R.l2norm_fwd(R.Tr, inp["x"])
    bwd = R.l2norm_bwd(R.Tr, inp["x"], n32, o32, inp["d_out"], 0)
    return inp, (n32, o32), fwd, bwd, R.l2norm_bwd(R.F32, inp["x"], n32, o32, inp["d_out"], 0, defect)


@pytest.mark.parametrize("B,S", R.L2_CASES, ids=_ids(R.L2_CASES))
def test_l2norm_bound_is_honest(B, S):
    inp, (n32, o32), (nrm, out), bwd, dy32 = _l2_run(B, S)
    _note("l2norm_fwd", "nrm", n32, nrm)
    _note("l2norm_fwd", "out", o32, out)
    _note("l2norm_bwd", "dx", dy32, bwd)
    if B > 1:                                                                   # the all-zero row: exact expectations
        z = R.L2_ZERO_ROW
        assert nrm.v[z] == float(np.float32(1e-12)) and nrm.e[z] == 0 and (out.v[z] == 0).all() and (out.e[z] == 0).all()
        assert np.allclose(bwd.v[z], inp["d_out"][z].astype(np.float64) / float(np.float32(1e-12)), rtol=1e-12)
        assert n32[4] == np.float32(1e-12) and (o32[4] != 0).all()              # the row below the clamp that is not zero


@pytest.mark.parametrize("defect", R.L2_DEFECTS)
def test_l2norm_bound_is_sensitive(defect):
    hits = []
    for c in R.L2_CASES:
        _, _, _, bwd, dy32 = _l2_run(*c, defect=defect)
        if _outside(dy32, bwd):
            hits.append(c)
    assert hits, defect


def _proj_run(B, K, S, act, defect=None):
    inp = R.proj_inputs(B, K, S, act)
    f32 = R.proj_fwd(R.F32, inp, act)
    return inp, f32, R.proj_fwd(R.Tr, inp, act), R.proj_bwd(R.Tr, inp, f32, act), R.proj_bwd(R.F32, inp, f32, act, defect)


@pytest.mark.parametrize("B,K,S,act", R.PROJ_CASES, ids=_ids(R.PROJ_CASES))
def test_projection_bound_is_honest(B, K, S, act):
    inp, f32, fwd, bwd, b32 = _proj_run(B, K, S, act)
    for k in ("y", "nrm", "out"):
        _note("img_proj_l2_fwd", k, f32[k], fwd[k])
    for k in ("dy", "d_x", "g_W", "g_b"):
        _note("img_proj_l2_bwd", k, b32[k], bwd[k])
    if B > 1 and not act:
        z = R.L2_ZERO_ROW
        assert fwd["nrm"].v[z] == float(np.float32(1e-12)) and (fwd["out"].v[z] == 0).all() and (fwd["out"].e[z] == 0).all()


@pytest.mark.parametrize("defect", ["projection_scaled"])
def test_projection_bound_is_sensitive(defect):
    hits = []
    for c in R.PROJ_CASES[:8]:
        _, _, _, bwd, b32 = _proj_run(*c, defect=defect)
        if any(_outside(b32[k], bwd[k]) for k in bwd):
            hits.append(c)
    assert hits, defect


# ---------------------------------------------------------------------------------------------------------------- grounding attention
@functools.lru_cache(maxsize=None)
def _attn_ref(case):
    method, row, B, Ts, C, S, acc = case
    inp = R.attn_inputs(*case)
    f32 = R.attn_fwd(R.F32, inp, method)
    return inp, f32, R.attn_fwd(R.Tr, inp, method), R.attn_bwd(R.Tr, inp, f32["alpha"], method, acc)


# one reference per distinct input (attn_row only steers the device's kernels)
ATTN_HOST_CASES = sorted({(m, 1, B, Ts, C, S, acc) for (m, _, B, Ts, C, S, acc) in R.ATTN_CASES})


@pytest.mark.parametrize("case", ATTN_HOST_CASES, ids=_ids(ATTN_HOST_CASES))
def test_attention_bound_is_honest_and_inputs_are_sound(case):
    method, row, B, Ts, C, S, acc = case
    inp, f32, fwd, bwd = _attn_ref(case)
    on = inp["mask"] != 0
    assert on.any(1).all(), "an attention row without an unmasked position"
    sc = fwd["scores"].v[on]
    assert sc.min() >= -30.0 and sc.max() <= 30.0, (sc.min(), sc.max())
    assert (fwd["alpha"].v[~on] == 0).all() and (fwd["alpha"].e[~on] == 0).all()
    assert (np.abs(fwd["alpha"].v.sum(1) - 1.0) <= fwd["alpha"].e.sum(1) + 1e-15).all()
    for k in ("alpha", "ctx"):
        _note("imagine_attn_ctx_fwd", k, f32[k], fwd[k])
    b32 = R.attn_bwd(R.F32, inp, f32["alpha"], method, acc)
    for k in bwd:
        _note("imagine_attn_ctx_bwd", k, b32[k], bwd[k])


def test_attention_cases_reach_every_value():
    for pos, vals in ((2, {1, 2, 3}), (5, {4, 20}), (6, {0, 1})):
        for fam in ((0, 1), (0, 0), (1, 1), (1, 0)):
            got = {c[pos] for c in R.ATTN_CASES if c[:2] == fam}
            assert got >= vals - {2}, (pos, fam, got)
    assert any(c[2] > 1 and 1 in R.attn_lengths(c[2], c[3]) for c in R.ATTN_CASES)


@pytest.mark.parametrize("defect", R.ATTN_FWD_DEFECTS + R.ATTN_BWD_DEFECTS + R.ATTN_MLP_DEFECTS)
def test_attention_bound_is_sensitive(defect):
    hits = []
    for case in ATTN_HOST_CASES:
        method, row, B, Ts, C, S, acc = case
        if C > 1024 or (defect in R.ATTN_MLP_DEFECTS and method == 0) or (defect == "dw_position_missing" and method == 1):
            continue
        inp, f32, fwd, bwd = _attn_ref(case)
        if defect in R.ATTN_FWD_DEFECTS:
            bad = R.attn_fwd(R.F32, inp, method, defect)
            out = any(_outside(bad[k], fwd[k]) for k in ("alpha", "ctx"))
        else:
            bad = R.attn_bwd(R.F32, inp, f32["alpha"], method, acc, defect)
            out = any(_outside(bad[k], bwd[k]) for k in bwd)
        if out:
            hits.append(case)
    assert hits, defect
    if defect == "mlp_w_last_chunk_missing":                                    # at every chunk edge: Ts = 7, 8, 9, 17
        assert {c[3] for c in hits} == {7, 8, 9, 17}, hits


# ---------------------------------------------------------------------------------------------------------------- ranking loss
@functools.lru_cache(maxsize=None)
def _rank_ref(B, S, kind):
    inp = R.rank_inputs(B, S)
    return inp, R.rank_fwd(R.Tr, inp, R.rank_margin(S), kind), R.rank_fwd(R.F32, inp, R.rank_margin(S), kind)


@pytest.mark.parametrize("B,S,kind", R.RANK_CASES, ids=_ids(R.RANK_CASES))
def test_ranking_loss_inputs_and_bound(B, S, kind):
    inp, fwd, f32 = _rank_ref(B, S, kind)
    assert fwd["ambiguous"] == 0, "a hinge whose sign the fp32 product may not decide"
    if B >= 16:
        frac = fwd["active"] / fwd["hinges"]
        assert 0.2 <= frac <= 0.8, frac
    assert np.array_equal(f32["G"], fwd["G"])                                   # no ambiguous hinge: the same small integers
    assert fwd["G"].sum() == 0                                                  # every hinge adds +1 off and -1 on the diagonal
    _note("rank_loss_fwd", "loss", f32["loss"], fwd["loss"])
    G32 = fwd["G"].astype(np.float32)
    bwd, b32 = R.rank_bwd(R.Tr, inp, G32, R.RANK_D_LOSS), R.rank_bwd(R.F32, inp, G32, R.RANK_D_LOSS)
    for k in bwd:
        _note("rank_loss_bwd", k, b32[k], bwd[k])


@pytest.mark.parametrize("defect", R.RANK_FWD_DEFECTS + R.RANK_BWD_DEFECTS)
def test_ranking_loss_bound_is_sensitive(defect):
    hits = []
    for (B, S, kind) in R.RANK_CASES:
        if B > 32:
            continue
        inp, fwd, _ = _rank_ref(B, S, kind)
        if defect in R.RANK_FWD_DEFECTS:
            bad = R.rank_fwd(R.F32, inp, R.rank_margin(S), kind, defect)
            out = not np.array_equal(bad["G"], fwd["G"]) or _outside(bad["loss"], fwd["loss"])
        else:
            G32 = fwd["G"].astype(np.float32)
            ref, bad = R.rank_bwd(R.Tr, inp, G32, R.RANK_D_LOSS), R.rank_bwd(R.F32, inp, G32, R.RANK_D_LOSS, defect)
            out = any(_outside(bad[k], ref[k]) for k in ref)
        if out:
            hits.append((B, S, kind))
    assert hits, defect
    if defect == "twin_not_skipped":
        assert all(k & 2 for (_, _, k) in hits)


# ---------------------------------------------------------------------------------------------------------------- initial state
def _init_run(case, fdef=None, bdef=None):
    B, Ts, C, H, mode, split, acc = case
    inp = R.init_inputs(*case)
    good = R.init_fwd(R.F32, inp, mode, split)
    f32 = R.init_fwd(R.F32, inp, mode, split, fdef)
    return inp, f32, R.init_fwd(R.Tr, inp, mode, split), R.init_bwd(R.Tr, inp, good, mode, split, acc), \
        R.init_bwd(R.F32, inp, good, mode, split, acc, bdef)


@pytest.mark.parametrize("case", R.INIT_CASES, ids=_ids(R.INIT_CASES))
def test_initial_state_bound_is_honest(case):
    inp, f32, fwd, bwd, b32 = _init_run(case)
    for k in fwd:
        _note("dec_init_fwd", k, f32[k], fwd[k])
    for k in bwd:
        _note("dec_init_bwd", k, b32[k], bwd[k])
    assert ("d_ctx" in bwd) == (case[4] == "ctx")


@pytest.mark.parametrize("defect", R.INIT_FWD_DEFECTS + R.INIT_BWD_DEFECTS)
def test_initial_state_bound_is_sensitive(defect):
    hits = []
    for case in R.INIT_CASES:
        fdef, bdef = (defect, None) if defect in R.INIT_FWD_DEFECTS else (None, defect)
        _, f32, fwd, bwd, b32 = _init_run(case, fdef, bdef)
        if any(_outside(f32[k], fwd[k]) for k in fwd) or any(_outside(b32[k], bwd[k]) for k in bwd):
            hits.append(case)
    assert hits, defect
    if defect == "accumulate_overwrites":
        assert all(c[6] == 1 for c in hits)


# ---------------------------------------------------------------------------------------------------------------- riders, arithmetic
def test_retrieval_ranks_reference_is_a_stable_descending_sort():
    sc = np.array([[1.0, 1.0, 0.5], [2.0, 1.0, 2.0], [3.0, 3.0, 3.0]])
    assert R.retrieval_ranks_ref(sc).tolist() == [0, 2, 2]


def test_tracked_arithmetic_basics():
    a = R.TV([1.0, -2.0], [0.5, 0.0])
    s = R.Tr.add(a, a)
    assert np.allclose(s.v, [2.0, -4.0]) and (s.e >= [1.0, 0.0]).all()
    sm = R.Tr.softmax(np.array([[0.0, 5.0, -3.0]]), np.array([[1.0, 0.0, 1.0]]))
    assert sm.v[0, 1] == 0 and sm.e[0, 1] == 0 and abs(sm.v.sum() - 1) < 1e-15
    with pytest.raises(AssertionError):
        R.Tr.softmax(np.zeros((1, 2)), np.zeros((1, 2)))
    with pytest.raises(AssertionError):                                         # a norm the clamp cannot be decided for
        R.l2norm_fwd(R.Tr, R.TV([[1e-12]], [[1e-13]]))
    assert R.ratio(np.array([1.0]), R.TV([1.0], [0.0])) == 0.0 and R.ratio(np.array([1.5]), R.TV([1.0], [0.0])) == np.inf


def test_zz_report_worst_ratios():
    """Runs last in this file: the largest |fp32 restatement - value| / err per operator (shown with -s)."""
    for op in sorted(WORST):
        print("host worst |err| / bound  %-24s %.3f" % (op, WORST[op]))
        assert WORST[op] <= 1.0
