"""CPU: the references and bounds of kNN-MT (tests/knn_ref.py) and the argument checks of vagnmt_hip.knn that need no device.

The bounds are honest (the fp32 restatement of the kernel's arithmetic stays inside them on the GPU tests' inputs) and sensitive
(every defect of the catalogue leaves them); the lam -> 0 and K = 1 properties hold; a mixed row sums to 1; the premises of the
GPU cases hold, so that the case tables are chosen with the reference alone."""
import numpy as np
import pytest

import knn_ref as R


# ------------------------------------------------------------------------------------------------------ premises of the GPU cases
@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=[c[0] for c in R.SEARCH_CASES])
def test_case_table_leaves_a_gap_at_the_kth_place_and_the_restatement_stays_inside_eps(case):
    name, N, Rr, D, K, ldq, seed = case
    q, bits, norm = R.search_case(N, Rr, D, K, ldq, seed)
    assert np.all(np.isnan(q[:, D:])) and q.shape == (Rr, ldq)
    q = q[:, :D]
    gap, eps = R.kth_gap(q, bits, norm, K)
    assert np.all(gap > 4 * eps), (name, float((gap / eps).min()))
    # honest: the fp32 restatement lies within eps of the float64 scores, entry by entry, and passes the GPU test's acceptance
    s64 = R.scores64(q, bits, norm)
    s32 = R.scores_fp32(q, bits, norm).astype(np.float64)
    e = R.score_eps(q, bits, s64)
    assert np.all(np.abs(s32 - s64) <= e), float((np.abs(s32 - s64) / e).max())
    Kp = min(K, N)
    got_s = np.full((Rr, K), -np.inf)
    got_i = np.full((Rr, K), -1, dtype=np.int32)
    for r in range(Rr):
        o = R.rank_order(s32[r])[:Kp]
        got_s[r, :Kp], got_i[r, :Kp] = s32[r, o], o
    assert not R.check_search(got_s, got_i, q, bits, norm, K)
    assert np.array_equal(got_i, R.search(q, bits, norm, K)[1])


def test_case_table_covers_the_sizes_the_kernel_branches_on():
    Ns, Rs, Ds, Ks = ({c[i] for c in R.SEARCH_CASES} for i in (1, 2, 3, 4))
    assert {1, R.SLICE - 1, R.SLICE + 1, 3 * R.SLICE + 17} <= Ns and any(c[1] == c[4] - 1 for c in R.SEARCH_CASES)
    assert {1, 12, R.ROW_TILE + 1, 192} <= Rs and {8, 40, 256, 512} <= Ds and {1, 8, 32} <= Ks
    assert any(c[5] > c[3] for c in R.SEARCH_CASES)


def test_duplicate_case_premise():
    c = R.DUP_CASE
    q, bits, norm = R.duplicate_case()
    s = R.scores64(q, bits, norm)
    dup = set(c["a"] + c["b"])
    slices = lambda idx: {i // R.SLICE for i in idx}        # noqa: E731
    assert slices(c["a"]) == {0, 1, 2} and slices(c["b"]) == {0, 1, 2} and c["N"] % R.SLICE != 0 and c["R"] > R.ROW_TILE
    for r in range(c["R"]):
        o = R.rank_order(s[r])
        assert set(o[:10].tolist()) == dup                                       # the ten copies are the ten best
        assert (o[c["K"] - 1] in c["a"]) == (o[c["K"]] in c["a"])                  # K-th and (K+1)-th: copies of one key
        assert s[r, o[c["K"] - 1]] == s[r, o[c["K"]]] and o[c["K"] - 1] < o[c["K"]]
        for g in (c["a"], c["b"]):
            assert len(set(s[r, g].tolist())) == 1
    # the restatement gives identical keys identical scores, whatever slice they lie in
    s32 = R.scores_fp32(q[:3], bits[sorted(dup)], norm[sorted(dup)])
    order = sorted(dup)
    for g in (c["a"], c["b"]):
        cols = [order.index(i) for i in g]
        assert all(len(set(s32[r, cols].view(np.int32).tolist())) == 1 for r in range(3))


@pytest.mark.parametrize("kind", ["one_word", "distinct", "mixed", "underflow", "short"])
@pytest.mark.parametrize("V", [5, 2500])
def test_mix_case_premises(V, kind):
    K = 8
    for raw in (False, True):
        for m in R.mix_case(V, V + 3, 2, K, kind, V + 2, raw):
            assert np.all(np.isnan(m["row"][:, V:])) and (m["lse"] is not None) == raw
            for r in range(m["row"].shape[0]):
                idx = m["nb_index"][r]
                words = [int(m["values"][i]) for i in idx if i >= 0]
                if kind == "one_word":
                    assert len(set(words)) == 1 and len(words) == K
                if kind == "distinct":
                    assert len(set(words)) == len(words) == min(K, V)
                if kind == "short":
                    assert len(words) == 3 and np.all(np.isneginf(m["nb_score"][r, 3:]))
                if kind == "underflow":
                    x = m["row"][r, words[0]] - (m["lse"][r] if raw else 0.0)
                    assert abs(x - R.NEG) < 1.0


# ------------------------------------------------------------------------------------------------------------- properties
def a_row(V=40, K=8, seed=0, T=10.0):
    rng = np.random.default_rng(seed)
    logits = 2.0 * rng.standard_normal(V)
    row = (logits - np.log(np.sum(np.exp(logits)))).astype(np.float32)
    values = rng.integers(0, V, size=30).astype(np.int32)
    idx = rng.permutation(30)[:K].astype(np.int32)
    sc = (-np.sort(rng.uniform(0, 40, K)) - 50).astype(np.float32)
    return row, sc, idx, values


def test_a_mixed_row_sums_to_one():
    for seed in range(5):
        row, sc, idx, values = a_row(seed=seed)
        for lam in (0.1, 0.5, 0.9):
            out = R.mix_row(row, sc, idx, values, 40, lam, 10.0)
            assert abs(np.sum(np.exp(out)) - 1.0) < 1e-6


def test_lam_to_zero_is_the_model_and_k_1_is_one_word():
    row, sc, idx, values = a_row()
    out = R.mix_row(row, sc, idx, values, 40, 1e-13, 10.0)
    assert np.all(np.abs(out - row.astype(np.float64)) < 1e-9)
    lam = 0.3
    out = R.mix_row(row, sc[:1], idx[:1], values, 40, lam, 10.0)
    w = int(values[idx[0]])
    want = row.astype(np.float64) + np.log1p(-lam)
    want[w] = np.log((1 - lam) * np.exp(float(row[w])) + lam)
    assert np.all(np.abs(out - want) < 1e-12)
    # the temperature does not matter with one neighbour; the ranking by score is the ranking by squared distance
    assert np.array_equal(out, R.mix_row(row, sc[:1], idx[:1], values, 40, lam, 0.01))
    q, bits, norm = R.search_case(200, 3, 16, 4, 16, 7)
    k = R.bf16_value(bits).astype(np.float64)
    d = ((q[:, None, :].astype(np.float64) - k[None]) ** 2).sum(-1)
    norm64 = (k ** 2).sum(1)
    s = R.scores64(q, bits, norm64)
    assert np.array_equal(np.argsort(d, axis=1, kind="stable")[:, :4], np.argsort(-s, axis=1, kind="stable")[:, :4])
    assert np.allclose(s.max(1)[:, None] - s, d - d.min(1)[:, None], atol=1e-9)


# ---------------------------------------------------------------------------------------------------- the bounds are sensitive
def test_every_defect_of_the_catalogue_leaves_the_bounds():
    seen = set()
    # the norm taken from the unrounded key
    rng = np.random.default_rng(1)
    h2 = rng.standard_normal((4, 3, 40)).astype(np.float32)
    tgt = rng.integers(4, 50, size=(3, 4))
    ref, bad = R.store_rows(h2, tgt), R.store_rows(h2, tgt, defect="norm_unrounded")
    assert np.any(np.abs(bad["norm"] - ref["norm"]) > R.norm_bound(ref["norm"], 40))
    seen.add("norm_unrounded")
    # a tie broken by index descending
    q, bits, norm = R.duplicate_case()
    assert not np.array_equal(R.search(q, bits, norm, 8, defect="tie_desc")[1], R.search(q, bits, norm, 8)[1])
    seen.add("tie_desc")
    # the mix
    row, sc, idx, values = a_row()
    values[idx[1]] = values[idx[0]]                           # two neighbours carry one word
    lam, T, V = 0.4, 10.0, 40
    ref = R.mix_row(row, sc, idx, values, V, lam, T)
    bound = R.mix_bound(row, sc, V, lam, T)
    for d in ("one_by_one", "no_log1m"):
        out = R.mix_row(row, sc, idx, values, V, lam, T, defect=d)
        assert np.any(np.abs(out - ref) > bound), d
        seen.add(d)
    far = (sc.astype(np.float64) * 40).astype(np.float32)      # scores near -3000 at T = 1: exp underflows without the shift
    ref = R.mix_row(row, far, idx, values, V, lam, 1.0)
    out = R.mix_row(row, far, idx, values, V, lam, 1.0, defect="no_max_shift")
    assert np.all(np.isfinite(ref)) and not np.all(np.abs(out - ref) <= R.mix_bound(row, far, V, lam, 1.0))
    seen.add("no_max_shift")
    wide = np.concatenate([row, np.float32([0.25, np.nan])])
    out = R.mix_row(wide, sc, idx, values, V, lam, T, defect="past_v")
    assert out[V] != wide[V] and R.mix_row(wide, sc, idx, values, V, lam, T)[V] == wide[V]
    seen.add("past_v")
    assert seen == set(R.DEFECTS)


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, 65504.0], dtype=np.float32)
    got = R.bf16_round(x)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == np.float32(1.015625) and got[3] == -1.0    # ties go to the even neighbour
    import torch
    y = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(R.bf16_bits(y), torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    p1, p2, p3 = R.split3(y)
    assert np.all(np.abs(y.astype(np.float64) - p1.astype(np.float64) - p2 - p3) <= 2.0 ** -27 * np.abs(y))


def test_span_end_is_the_forced_span():
    assert R.span_end([5, 6, 3, 7, 0]) == 2 and R.span_end([5, 6, 7, 0, 0]) == 2 and R.span_end([0, 0, 0]) == -1
    assert R.span_end([5, 0, 7, 0]) == 2 and R.span_end([3]) == 0


# --------------------------------------------------------------------------------- vagnmt_hip.knn: checks that need no device
def test_argument_checks_of_knn_py():
    from vagnmt_hip import knn
    assert knn.check_params(8, 10, 0.5) == (8, 10.0, 0.5) and knn.check_params(1, 0.1, 0) == (1, 0.1, 0.0)
    for bad in [(0, 10.0, 0.5), (33, 10.0, 0.5), (8, 0.0, 0.5), (8, -1.0, 0.5), (8, float("inf"), 0.5), (8, 10.0, 1.0),
                (8, 10.0, -0.1)]:
        with pytest.raises(ValueError):
            knn.check_params(*bad)
    for D in (0, 4, 12, 1032):
        with pytest.raises(ValueError):
            knn.Datastore(D, "cpu")
    s = knn.Datastore(40, "cpu")
    assert len(s) == 0
    inv_T, log_lam, log1m = knn.mix_scalars(10.0, 0.5)
    ref = R.host_scalars(0.5, 10.0)
    assert (np.float32(inv_T), np.float32(log_lam), np.float32(log1m)) == ref
    assert knn.MAX_K == R.MAX_K and knn.SLICE == R.SLICE
    with pytest.raises(ValueError):
        knn.search_args([object(), object()], [s], 8, 10.0, 0.5)
    with pytest.raises(ValueError):
        knn.search_args([object()], ["not a store"], 8, 10.0, 0.5)
    assert knn.graph_key([], 8, 10.0, 0.5) != knn.graph_key([], 8, 10.0, 0.25)
