"""GPU: kNN-MT (vagnmt_hip.knn; include/vag_nmt.h: vag_knn_store_rows, vag_knn_search, vag_knn_mix).

1. the three kernels through the ABI by hand against tests/knn_ref.py: the search on the case table of knn_ref (every row's set
   must equal the reference's: the table's seeds leave a gap of more than 4 eps at the K-th place, asserted here again), exact
   duplicates, the store, the mix, the ABI's argument errors;
2. the models and Ensemble: lam = 0 is beamsearch_nbest, scores against knn_score_translations, graph against eager mode and
   stale graphs, memorisation of a translation memory, the reported neighbours, save / load, knn_sweep."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import knn_ref as R

pytestmark = pytest.mark.gpu

EOS = 3
I32, I64 = torch.int32, torch.int64


def L():
    from vagnmt_hip import _lib
    return _lib.lib()


def stream():
    from vagnmt_hip import _lib
    return _lib.stream()


def pp(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def p64(vals):
    return (C.c_int64 * len(vals))(*vals)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def keys_dev(bits):
    """uint16 bf16 bit patterns -> a torch.bfloat16 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def run_search(q, bits, norm, K, D):
    Rr, ldq = q.shape
    N = bits.shape[0]
    qd, kd, nd = dev(q), keys_dev(bits), dev(norm)
    out_s = torch.full((Rr, K), 7.0, device="cuda")
    out_i = torch.full((Rr, K), 7, dtype=I32, device="cuda")
    nb = L().vag_knn_scratch_bytes(Rr, N, K)
    assert nb == Rr * ((N + R.SLICE - 1) // R.SLICE) * K * 8
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = L().vag_knn_search(qd.data_ptr(), ldq, Rr, D, kd.data_ptr(), nd.data_ptr(), N, K, out_s.data_ptr(), out_i.data_ptr(),
                            scratch.data_ptr(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ search
def test_geometry_constants():
    assert L().vag_knn_slice() == R.SLICE
    assert L().vag_knn_row_tile(512) == R.ROW_TILE and L().vag_knn_row_tile(640) == 32 and L().vag_knn_row_tile(1024) == 16
    assert L().vag_knn_row_tile(12) == 0 and L().vag_knn_scratch_bytes(4, 0, 8) == 0 and L().vag_knn_scratch_bytes(4, 9, 33) == 0


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=[c[0] for c in R.SEARCH_CASES])
def test_search_matches_reference(case):
    name, N, Rr, D, K, ldq, seed = case
    q, bits, norm = R.search_case(N, Rr, D, K, ldq, seed)
    gap, eps = R.kth_gap(q[:, :D], bits, norm, K)
    assert np.all(gap > 4 * eps), "the case table's premise: every row's gap at the K-th place exceeds 4 eps"
    got_s, got_i = run_search(q, bits, norm, K, D)
    bad = R.check_search(got_s, got_i, q[:, :D], bits, norm, K)
    assert not bad, bad[:5]
    ref_s, ref_i = R.search(q[:, :D], bits, norm, K)
    Kp = min(K, N)
    # no row is excused: with the gap above, the device's set IS the reference's
    assert all(set(got_i[r, :Kp].tolist()) == set(ref_i[r, :Kp].tolist()) for r in range(Rr))
    s64 = R.scores64(q[:, :D], bits, norm)
    err = np.abs(got_s[:, :Kp].astype(np.float64) - np.take_along_axis(s64, got_i[:, :Kp].astype(np.int64), 1))
    print("%s: max |score - s64| = %.3e, smallest eps of a row = %.3e" % (name, err.max(), eps.min()))


def test_search_at_depth_1024_uses_the_small_row_tile():
    """D = 1024 (row tile 16) and D = 648 (a depth that is no multiple of 16, row tile 16), more rows than one tile."""
    for D, seed in ((1024, 0), (648, 1)):
        q, bits, norm = R.search_case(300, 19, D, 4, D, seed)
        got_s, got_i = run_search(q, bits, norm, 4, D)
        assert not R.check_search(got_s, got_i, q, bits, norm, 4)


def test_exact_duplicates_are_ranked_by_index_with_identical_scores():
    c = R.DUP_CASE
    q, bits, norm = R.duplicate_case()
    got_s, got_i = run_search(q, bits, norm, c["K"], c["D"])
    ref_s, ref_i = R.search(q, bits, norm, c["K"])
    dup = set(c["a"] + c["b"])
    assert all(set(r) <= dup for r in ref_i.tolist())                          # the premise: the copies are the best of every row
    assert np.array_equal(got_i, ref_i)
    group = np.isin(got_i, c["a"])
    for r in range(c["R"]):
        for g in (group[r], ~group[r]):
            v = got_s[r][g].view(np.int32)
            assert len(set(v.tolist())) == 1, (r, got_s[r], got_i[r])           # one stored key, one bit pattern
        # the K-th and the (K+1)-th place of the reference are copies of one key
        full = R.rank_order(R.scores64(q, bits, norm)[r])
        assert (full[c["K"] - 1] in c["a"]) == (full[c["K"]] in c["a"])


# ------------------------------------------------------------------------------------------------------------------- store
def store_case(B, Tt, H, seed):
    rng = np.random.default_rng(seed)
    h2 = rng.standard_normal((Tt, B, H)).astype(np.float32)
    tgt = rng.integers(4, 60, size=(B, Tt)).astype(np.int64)
    if B > 1 and Tt > 1:
        tgt[0, Tt // 2] = EOS                       # an EOS in the middle: the rest of the row is not stored
        tgt[1, :] = 0                               # an all-pad row: nothing
        tgt[2, Tt - 3:] = 0                         # no EOS: up to the last non-pad word
        tgt[3, 2] = 0                               # (a pad inside the words is a word position like any other)
    return h2, tgt


@pytest.mark.parametrize("B,Tt", [(1, 1), (1, 9), (5, 1), (5, 9)])
def test_store_rows(B, Tt):
    H = 40
    h2, tgt = store_case(B, Tt, H, 5)
    ref = R.store_rows(h2, tgt, sent_base=11)
    cap = B * Tt + 3
    keys = torch.full((cap, H), 7.0, dtype=torch.bfloat16, device="cuda")
    norm = torch.full((cap,), 7.0, device="cuda")
    val, sen, pos = (torch.full((cap,), 7, dtype=I32, device="cuda") for _ in range(3))
    cnt = torch.zeros(1, dtype=I32, device="cuda")
    hd, td = dev(h2), dev(tgt)
    rc = L().vag_knn_store_rows(hd.data_ptr(), td.data_ptr(), B, Tt, H, 11, cap, keys.data_ptr(), norm.data_ptr(),
                                val.data_ptr(), sen.data_ptr(), pos.data_ptr(), cnt.data_ptr(), stream())
    assert rc == 0
    n = int(cnt.item())
    assert n == ref["count"]
    assert np.array_equal(keys[:n].view(torch.int16).cpu().numpy().view(np.uint16), ref["keys"])      # bit for bit
    assert np.all(np.abs(norm[:n].cpu().numpy().astype(np.float64) - ref["norm"]) <= R.norm_bound(ref["norm"], H))
    assert np.array_equal(val[:n].cpu().numpy(), ref["value"]) and np.array_equal(sen[:n].cpu().numpy(), ref["sentence"])
    assert np.array_equal(pos[:n].cpu().numpy(), ref["position"])
    assert bool((norm[n:] == 7.0).all()) and bool((val[n:] == 7).all())                                # nothing past the count


# --------------------------------------------------------------------------------------------------------------------- mix
def run_mix(members, V, K, lam, T):
    inv_T, log_lam, log1m = R.host_scalars(lam, T)
    rows = [dev(m["row"]) for m in members]
    lses = [None if m["lse"] is None else dev(m["lse"]) for m in members]
    sc, ix, vals = [dev(m["nb_score"]) for m in members], [dev(m["nb_index"]) for m in members], [dev(m["values"]) for m in members]
    rc = L().vag_knn_mix(pp(rows), p64([r.shape[1] for r in rows]), len(members), rows[0].shape[0], V, pp(sc), pp(ix), K, pp(vals),
                         p64([len(m["values"]) for m in members]), pp(lses) if lses[0] is not None else None, float(inv_T),
                         float(log_lam), float(log1m), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in rows]


@pytest.mark.parametrize("raw", [False, True], ids=["logp", "logits_lse"])
@pytest.mark.parametrize("kind", ["one_word", "distinct", "mixed", "underflow", "short"])
@pytest.mark.parametrize("V,M", [(5, 1), (2500, 3), (2500, 1), (5, 3)])
def test_mix_matches_reference(V, M, kind, raw):
    K, lam, T, ldl = 8, 0.4, 10.0, V + 3
    members = R.mix_case(V, ldl, M, K, kind, V + M, raw)
    got = run_mix(members, V, K, lam, T)
    for m, g in zip(members, got):
        for r in range(m["row"].shape[0]):
            lse = 0.0 if m["lse"] is None else m["lse"][r]
            ref = R.mix_row(m["row"][r], m["nb_score"][r], m["nb_index"][r], m["values"], V, lam, T, lse)
            bound = R.mix_bound(m["row"][r], m["nb_score"][r], V, lam, T, lse)
            assert np.all(np.isnan(g[r, V:])), "columns past V must stay"
            assert np.all(np.abs(g[r, :V].astype(np.float64) - ref[:V]) <= bound), (kind, r, np.abs(g[r, :V] - ref[:V]).max())
            # the probabilities sum to what the reference's do within the bound -- and that is 1, up to the fp32 rounding of the
            # given row itself (2^-23 (|x| + |lse| + 1) per word), unless a word of the row was ruled out (-1e5: its mass is gone)
            total, want = np.sum(np.exp(g[r, :V].astype(np.float64))), np.sum(np.exp(ref[:V]))
            assert abs(total - want) <= np.sum(np.exp(ref[:V]) * bound) + 1e-12, (total, want)
            if kind != "underflow":
                given = 2.0 ** -23 * (np.abs(m["row"][r, :V].astype(np.float64)) + abs(float(lse)) + 1.0)
                assert abs(total - 1.0) <= np.sum(np.exp(ref[:V]) * (bound + given)) + 1e-12, total


def test_abi_argument_errors_launch_nothing():
    t = torch.zeros(64, device="cuda")
    i = torch.zeros(64, dtype=I32, device="cuda")
    p, ip = t.data_ptr(), i.data_ptr()
    S = L().vag_knn_search
    assert S(None, 8, 1, 8, p, p, 1, 1, p, ip, p, stream()) == -22
    assert S(p, 8, 1, 12, p, p, 1, 1, p, ip, p, stream()) == -22              # D no multiple of 8
    assert S(p, 8, 1, 1032, p, p, 1, 1, p, ip, p, stream()) == -22
    assert S(p, 4, 1, 8, p, p, 1, 1, p, ip, p, stream()) == -22               # ldq < D
    assert S(p, 8, 1, 8, p, p, 0, 1, p, ip, p, stream()) == -22
    assert S(p, 8, 1, 8, p, p, 1 << 31, 1, p, ip, p, stream()) == -22
    assert S(p, 8, 1, 8, p, p, 1, 33, p, ip, p, stream()) == -22
    assert S(p, 8, 0, 8, p, p, 1, 1, p, ip, p, stream()) == -22
    assert S(p, 8, 1, 8, p + 2, p, 1, 1, p, ip, p, stream()) == -22           # misaligned keys
    St = L().vag_knn_store_rows
    assert St(None, p, 1, 1, 8, 0, 1, p, p, ip, ip, ip, ip, stream()) == -22
    assert St(p, p, 1, 1, 12, 0, 1, p, p, ip, ip, ip, ip, stream()) == -22
    assert St(p, p, 0, 1, 8, 0, 1, p, p, ip, ip, ip, ip, stream()) == -22
    assert St(p, p, 1, 1, 8, -1, 1, p, p, ip, ip, ip, ip, stream()) == -22
    Mx = L().vag_knn_mix
    one = pp([t])
    onei = pp([i])
    ok = dict(inv_T=0.1, ll=math.log(0.5), l1=math.log1p(-0.5))
    assert Mx(None, p64([8]), 1, 1, 5, one, onei, 4, onei, p64([4]), None, ok["inv_T"], ok["ll"], ok["l1"], stream()) == -22
    assert Mx(one, p64([4]), 1, 1, 5, one, onei, 4, onei, p64([4]), None, ok["inv_T"], ok["ll"], ok["l1"], stream()) == -22   # ldl < V
    assert Mx(one, p64([8]), 9, 1, 5, one, onei, 4, onei, p64([4]), None, ok["inv_T"], ok["ll"], ok["l1"], stream()) == -22
    assert Mx(one, p64([8]), 1, 1, 5, one, onei, 33, onei, p64([4]), None, ok["inv_T"], ok["ll"], ok["l1"], stream()) == -22
    assert Mx(one, p64([8]), 1, 1, 5, one, onei, 4, onei, p64([4]), None, 0.0, ok["ll"], ok["l1"], stream()) == -22
    assert Mx(one, p64([8]), 1, 1, 5, one, onei, 4, onei, p64([4]), None, ok["inv_T"], 0.0, ok["l1"], stream()) == -22
    assert Mx(one, p64([8]), 1, 1, 5, one, onei, 4, onei, p64([4]), None, ok["inv_T"], ok["ll"], 0.5, stream()) == -22
    assert Mx(one, p64([8]), 1, 1, 5, pp([None]), onei, 4, onei, p64([4]), None, ok["inv_T"], ok["ll"], ok["l1"], stream()) == -22
    torch.cuda.synchronize()
    assert bool((t == 0).all()) and bool((i == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# the models and Ensemble
# ------------------------------------------------------------------------------------------------------------------
VS, VT, IM, ML, H = 70, 503, 64, 10, 64
LENS = [9, 6, 3]
KB = 6                      # beam size
KN, TEMP = 4, 10.0          # neighbours, temperature


def make_model(kind, seed, eos_bias=0.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    if kind == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(VS, VT, IM, 32, 32, H, 48, 0.99, attn_model="dot", tied_emb=True)
    else:
        m = NMT_Seq2Seq_Beam_V2(VS, VT, 32, 32, H, tied_emb=True)
    with torch.no_grad():
        m.decoder.out.bias[EOS] += eos_bias
    return m.cuda().eval()


def make_inputs(lens=LENS, seed=9):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        src[b, :n] = torch.randint(4, VS, (n,), generator=g)
    return src.cuda(), torch.randn(len(lens), IM, generator=g).abs().cuda()


def memory(seed=3, n=8):
    """A translation memory of n pairs: sources, lengths, images, and targets of 3 .. 8 words without an immediate repeat, EOS
    appended, as a (n, ML) int64 tensor padded with 0."""
    rng = np.random.default_rng(seed)
    lens = sorted((int(x) for x in rng.integers(2, 10, size=n)), reverse=True)
    src, im = make_inputs(lens, seed=seed + 1)
    tgt = np.zeros((n, ML), dtype=np.int64)
    for b in range(n):
        L_ = int(rng.integers(3, 9))
        row = [int(rng.integers(4, VT))]
        while len(row) < L_:
            w = int(rng.integers(4, VT))
            if w != row[-1]:
                row.append(w)
        tgt[b, :L_] = row
        tgt[b, L_] = EOS
    return src, lens, im, torch.from_numpy(tgt).cuda()


def build_store(m, kind, seed=3):
    from vagnmt_hip import knn
    return knn.Datastore.build(m, split(memory(seed), 5, kind != "text"), chunk_rows=32)


def split(mem, at, with_im):
    """The memory as two batches (src_var, src_lengths, tgt, im_var), each source trimmed to its longest sentence."""
    src, lens, im, tgt = mem
    return [(src[a:b, :max(lens[a:b])].contiguous(), lens[a:b], tgt[a:b].contiguous(), im[a:b].contiguous() if with_im else None)
            for a, b in ((0, at), (at, len(lens)))]


def ints(hyps):
    return [[[int(t) for t in r] for r in h] for h in hyps]


def bits(t):
    return t.detach().cpu().contiguous().view(I32)


def same(a, b):
    return ints(a.hyps) == ints(b.hyps) and torch.equal(bits(a.scores), bits(b.scores))


@pytest.fixture(scope="module", params=["mm", "text", "ens"])
def subject(request):
    """(kind, searcher, members, stores, src, im): a multimodal model, a text-only one, an Ensemble of two multimodal ones; the
    models carry an EOS bias so that hypotheses end before max_length."""
    kind = request.param
    src, im = make_inputs()
    if kind == "ens":
        from vagnmt_hip.ensemble import Ensemble
        ms = [make_model("mm", 31, 5.0), make_model("mm", 32, 5.0)]
        return kind, Ensemble(ms), ms, [build_store(m, "mm") for m in ms], src, im
    m = make_model(kind, 31, 5.0)
    return kind, m, [m], build_store(m, kind), src, (im if kind == "mm" else None)


def nbest(s, src, im, k=KB, n=KB, lens=LENS):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    if isinstance(s, NMT_Seq2Seq_Beam_V2):
        return s.beamsearch_nbest(src, lens, k, n, ML)
    return s.beamsearch_nbest(src, lens, im, k, n, ML)


def knn_search(s, src, im, store, lens=LENS, **kw):
    kw.setdefault("beam_size", KB)
    kw.setdefault("n_best", KB)
    kw.setdefault("max_length", ML)
    kw.setdefault("k", KN)
    kw.setdefault("temperature", TEMP)
    return s.beamsearch_knn(src, lens, im, store, **kw)


def set_graph(s, members, on):
    s.decode_graph = on
    for m in members:
        m.decode_graph = on


def test_store_holds_the_memory_and_round_trips(subject, tmp_path):
    from vagnmt_hip import knn
    kind, s, members, stores, src, im = subject
    store = stores[0] if kind == "ens" else stores
    _, _, _, tgt = memory()
    t = tgt.cpu().numpy()
    spans = [R.span_end(r) + 1 for r in t]
    assert len(store) == sum(spans) and store.keys.shape == (len(store), H) and store.keys.dtype == torch.bfloat16
    assert store.values.cpu().tolist() == [int(t[b, i]) for b in range(8) for i in range(spans[b])]
    assert store.sentence.cpu().tolist() == [b for b in range(8) for _ in range(spans[b])]
    assert store.position.cpu().tolist() == [i for b in range(8) for i in range(spans[b])]
    k64 = store.keys.float().double()
    assert torch.all((store.norm.double() - (k64 * k64).sum(1)).abs().cpu() <= torch.from_numpy(R.norm_bound((k64 * k64).sum(1).cpu().numpy(), H)))
    path = str(tmp_path / "store.pt")
    store.save(path)
    back = knn.Datastore.load(path)
    assert len(back) == len(store)
    for f in ("keys", "norm", "values", "sentence", "position"):
        assert torch.equal(getattr(back, f).cpu().view(-1).view(torch.uint8) if f == "keys" else getattr(back, f).cpu(),
                           getattr(store, f).cpu().view(-1).view(torch.uint8) if f == "keys" else getattr(store, f).cpu()), f
    if kind != "ens":
        a, b = knn_search(s, src, im, store, lam=0.5), knn_search(s, src, im, back, lam=0.5)
        assert same(a, b)
        # a store that does not fit the model is refused
        with pytest.raises(ValueError):
            knn_search(s, src, im, knn.Datastore(32, "cuda"), lam=0.5)
        bad = knn.Datastore.load(path)
        bad._chunks[0]["values"][0] = VT
        with pytest.raises(ValueError):
            knn_search(s, src, im, bad, lam=0.5)
        with pytest.raises(ValueError):
            knn_search(s, src, im, [store, store], lam=0.5)


def test_lam_0_is_beamsearch_nbest_and_launches_nothing(subject, monkeypatch):
    from vagnmt_hip import knn
    kind, s, members, stores, src, im = subject
    seen = []
    real = knn.call
    monkeypatch.setattr(knn, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    for graph in (True, False):
        set_graph(s, members, graph)
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(s, src, im, k, n)
            r = knn_search(s, src, im, stores, beam_size=k, n_best=n, lam=0.0)
            assert ints(r.hyps) == ints(hyps) and torch.equal(bits(r.scores), bits(sc)), (graph, k)
    assert not [x for x in seen if x.startswith("vag_knn")], seen
    r = knn_search(s, src, im, stores, lam=0.5)
    assert "vag_knn_search" in seen and "vag_knn_mix" in seen and not same(r, knn_search(s, src, im, stores, lam=0.0))
    set_graph(s, members, True)


def forced_eps(members, stores, src_n, lens_n, flat, im_n):
    """The largest score bound eps over the forced rows of the given hypotheses and every entry of the members' stores."""
    from vagnmt_hip import knn, scoring
    stores = stores if isinstance(stores, list) else [stores]
    worst = 0.0
    with torch.no_grad():
        for m, st in zip(members, stores):
            mm = hasattr(m, "vse_imagine")
            tgt, tok = scoring.forced_args([m], [mm], src_n, flat, im_n if mm else None)
            h2 = knn.member_forced(m, src_n, lens_n, im_n if mm else None, tok, tgt, head=False)
            q = h2.reshape(-1, h2.shape[2]).cpu().numpy()
            kb = st.keys.view(torch.int16).cpu().numpy().view(np.uint16)
            nm = st.norm.cpu().numpy()
            worst = max(worst, float(R.score_eps(q, kb, R.scores64(q, kb, nm)).max()))
    return worst


def test_scores_are_knn_forced_scores(subject):
    """Every returned hypothesis that ended before max_length scores, forced under the mixed distribution, what the search scored
    it.  Tolerance: relative 2e-4, the bound tests/test_gpu_constrain.py uses for its search-score against forced-score
    comparison, plus the neighbour term's margin: the search and the forced path each hold every neighbour's score within eps
    of the exact one (knn_ref.score_eps, the largest over the forced rows and the store), so the arguments (s_j - s_max) / T of
    the two paths differ by at most 4 eps / T, log p_knn by as much, and a mixed log-probability -- 1-Lipschitz in it -- too
    (knn_ref.mix_bound_from_search); a length-normalised score is a mean of those, so the margin is 4 eps / T, not widened."""
    kind, s, members, stores, src, im = subject
    lam = 0.5
    r = knn_search(s, src, im, stores, lam=lam)
    sc = r.scores.cpu().numpy()
    B = len(LENS)
    idx = [(b, j) for b in range(B) for j in range(KB) if len(r.hyps[b][j]) < ML - 1]
    assert len(idx) >= 4, len(idx)
    flat = [list(r.hyps[b][j]) for b in range(B) for j in range(KB)]
    src_n = src.repeat_interleave(KB, 0)
    lens_n = [n for n in LENS for _ in range(KB)]
    im_n = im.repeat_interleave(KB, 0) if im is not None else None
    f = s.knn_score_translations(src_n, lens_n, flat, im_n, stores, KN, TEMP, lam).score.cpu().numpy().reshape(B, KB)
    margin = R.mix_bound_from_search(forced_eps(members, stores, src_n, lens_n, flat, im_n), TEMP)
    worst = max((abs(float(f[b, j]) - float(sc[b, j])) - margin) / max(1.0, abs(float(sc[b, j]))) for b, j in idx)
    print("%s: %d finished hypotheses, margin 4 eps / T = %.3e, worst relative excess %.3e" % (kind, len(idx), margin, worst))
    assert worst <= 2e-4, worst
    # and lam = 0 of the scoring is score_translations bit for bit
    z = s.knn_score_translations(src_n, lens_n, flat, im_n, stores, KN, TEMP, 0.0)
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    p = s.score_translations(src_n, lens_n, flat) if isinstance(s, NMT_Seq2Seq_Beam_V2) else s.score_translations(src_n, lens_n, flat, im_n)
    assert torch.equal(bits(z.score), bits(p.score)) and torch.equal(bits(z.token_logp), bits(p.token_logp))


def test_graph_equals_eager_and_no_stale_graph(subject):
    kind, s, members, stores, src, im = subject
    other = [build_store(m, "mm", seed=5) for m in members] if kind == "ens" else build_store(members[0], kind, seed=5)
    runs = [(stores, 0.5), (stores, 0.2), (other, 0.5), (stores, 0.5)]
    set_graph(s, members, False)
    eager = [knn_search(s, src, im, st, lam=lam) for st, lam in runs]
    set_graph(s, members, True)
    graph = [knn_search(s, src, im, st, lam=lam) for st, lam in runs]
    for e, g in zip(eager, graph):
        assert same(e, g)
    assert not same(eager[0], eager[1]) and not same(eager[0], eager[2])       # another lam, another store: other results
    # the constraints still win over a neighbour
    w = next(int(h[0]) for hs in eager[0].hyps for h in hs if len(h))
    c = knn_search(s, src, im, stores, lam=0.5, banned=[[w]])
    live = [(b, j) for b in range(len(LENS)) for j in range(KB) if float(c.scores[b, j]) > -1e4]
    assert live and all(w not in [int(t) for t in c.hyps[b][j]] for b, j in live)


def test_memorisation_and_reported_neighbours(subject):
    """A store built from 8 pairs makes a greedy kNN search return exactly those targets.  The premise is checked with the
    reference first: with the forced states from the device, the mixed arg-max at every gold prefix is the gold word."""
    from vagnmt_hip import knn, scoring
    kind, s, members, stores, _, _ = subject
    src, lens, im, tgt = memory()
    im_ = im if kind != "text" else None
    lam, T, K = 0.9, 0.05, 4
    gold = tgt.cpu().numpy()
    spans = [R.span_end(r) + 1 for r in gold]
    own = nbest(s, src, im_, 1, 1, lens)[0]
    assert all([int(t) for t in own[b][0]] != gold[b, :spans[b] - 1].tolist() for b in range(8))     # not what the model says anyway
    # the premise, with knn_ref on the device's forced states and logits
    store_list = stores if isinstance(stores, list) else [stores]
    probs = []
    ref_nb = []
    with torch.no_grad():
        for m, st in zip(members, store_list):
            mm = hasattr(m, "vse_imagine")
            tg, tok = scoring.forced_args([m], [mm], src, tgt, im if mm else None)
            logits, lse, h2 = knn.member_forced(m, src, lens, im if mm else None, tok, tg)
            q = h2.reshape(-1, H).cpu().numpy()
            kb, nm = st.keys.view(torch.int16).cpu().numpy().view(np.uint16), st.norm.cpu().numpy()
            rs, ri = R.search(q, kb, nm, K)
            ref_nb.append((q, kb, nm, ri.reshape(ML, 8, K)))
            vals = st.values.cpu().numpy()
            lg, ls = logits.cpu().numpy(), lse.cpu().numpy()
            probs.append(np.stack([np.exp(R.mix_row(lg[i], rs[i], ri[i], vals, VT, lam, T, ls[i])[:VT]) for i in range(ML * 8)]))
    mean = np.mean(probs, axis=0).reshape(ML, 8, VT)
    for b in range(8):
        for t in range(spans[b]):
            assert int(mean[t, b].argmax()) == int(gold[b, t]), (b, t)
            assert np.sort(mean[t, b])[-1] > 2 * np.sort(mean[t, b])[-2]       # (by a wide margin: no near tie decides)
    for graph in (True, False):
        set_graph(s, members, graph)
        r = s.beamsearch_knn(src, lens, im_, stores, beam_size=1, n_best=1, max_length=ML, k=K, temperature=T, lam=lam,
                             return_neighbours=True)
        assert [[int(t) for t in r.hyps[b][0]] for b in range(8)] == [gold[b, :spans[b] - 1].tolist() for b in range(8)], graph
    # the neighbours reported along the returned hypotheses are the entries the reference finds
    nbs = r.neighbours if isinstance(r.neighbours, list) else [r.neighbours]
    off = np.concatenate([[0], np.cumsum(spans)])
    for nb, (q, kb, nm, ri), st in zip(nbs, ref_nb, store_list):
        got_i, got_s = nb.index.cpu().numpy(), nb.score.cpu().numpy()
        assert got_i.shape[:2] == (8, 1) and got_i.shape[3] == K
        for b in range(8):
            for t in range(spans[b]):
                assert got_i[b, 0, t, 0] == ri[t, b, 0] == off[b] + t                   # the nearest entry is the position's own
                assert int(nb.value[b, 0, t, 0]) == int(gold[b, t])
                assert not R.check_search(got_s[b, 0, t][None], got_i[b, 0, t][None], q[t * 8 + b][None], kb, nm, K)
            assert np.all(got_i[b, 0, spans[b]:] == -1)
    set_graph(s, members, True)


def test_knn_sweep_is_the_grid_of_separate_scorings(subject):
    from vagnmt_hip import knn
    kind, s, members, stores, _, _ = subject
    src, lens, im, tgt = memory(seed=7)
    batches = split((src, lens, im, tgt), 3, kind != "text")
    lams, temps = [0.0, 0.3, 0.8], [1.0, 20.0]
    grid = knn.knn_sweep(s, stores, batches, lams, temps, k=KN)
    assert tuple(grid.shape) == (3, 2)
    words = sum(R.span_end(r) + 1 for r in tgt.cpu().numpy())
    for i, lam in enumerate(lams):
        for j, t in enumerate(temps):
            total = sum(float(s.knn_score_translations(a, b, c, d, stores, KN, t, lam).logp.double().sum()) for a, b, c, d in batches)
            assert abs(float(grid[i, j]) - math.exp(-total / words)) <= 1e-6 * math.exp(-total / words), (lam, t)
    assert float(grid[0, 0]) == float(grid[0, 1])                                 # lam = 0: the model's own perplexity
