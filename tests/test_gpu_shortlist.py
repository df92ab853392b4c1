"""GPU: lexical shortlists (vagnmt_hip.shortlist; include/vag_nmt.h: vag_shortlist_*).

1. vag_shortlist_select against tests/shortlist_ref.py on every case of its table, all integer outputs exactly, two runs bitwise
   equal, and the entry's refusals;
2. vag_shortlist_gather: widths 1 / 3 / 32 / 36, a source 4 bytes off a 16-byte boundary, pads, an untouched source, a refill
   with a smaller n;
3. vag_shortlist_map in both directions on 1-D and 3-D tensors, absent words counted, the round trip;
4. the equivalence: a model whose three vocabulary-sized tensors were cut down BY HAND in torch (index_select with the
   reference's ids, pad rows of 0 / -1e30) decodes token for token and bit for bit in the scores like the shortlist path -- text,
   multimodal, tied_emb, an Ensemble of two, eager and graph mode, forced scores, device rows, sampling;
5. refill under a captured graph: batch A, batch B, batch A again on ONE Shortlist;
6. the identity: always = every word, capacity V is the plain model bit for bit;
7. nothing else moved: the wrapped model's parameters and its own search;
8. a constrained search through sl.view with to_short / to_full; the refusals."""
import copy

import numpy as np
import pytest
import torch

import shortlist_ref as R

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64
VS, VT, E, IM = 50, 120, 32, 48
CAP, BEST, K_LEX = 40, 3, 4
BEAM, NBEST, MAXLEN = 3, 3, 8
ALWAYS = np.arange(8, dtype=np.int32)


def L():
    from vagnmt_hip import _lib
    return _lib.lib()


def stream():
    from vagnmt_hip import _lib
    return _lib.stream()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ------------------------------------------------------------------------------------------------------------------
# 1. select
# ------------------------------------------------------------------------------------------------------------------
def run_select(c, poison=7):
    src, lengths, lex, always = dev(c["src"]), dev(c["lengths"]), dev(c["lex"]), dev(c["always"])
    V, cap = c["V"], c["cap"]
    ids = torch.full((cap,), poison, dtype=I32, device="cuda")
    f2s = torch.full((V,), poison, dtype=I32, device="cuda")
    cnt = torch.full((2,), poison, dtype=I32, device="cuda")
    rc = L().vag_shortlist_select(src.data_ptr(), lengths.data_ptr(), src.shape[0], src.shape[1], lex.data_ptr(), lex.shape[0],
                                  lex.shape[1], c["best"], always.data_ptr(), always.shape[0], V, cap, ids.data_ptr(),
                                  cnt[0:1].data_ptr(), cnt[1:2].data_ptr(), f2s.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), int(cnt[0]), int(cnt[1]), f2s.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_select_matches_the_reference(name):
    c = dict(R.cases()[name])
    want_used = c.pop("rank_used", None)
    ids, n, used, f2s = R.select(**c)
    assert L().vag_shortlist_supported(c["V"], c["lex"].shape[0], c["lex"].shape[1], c["cap"]) == 1
    rc, g_ids, g_n, g_used, g_f2s = run_select(c)
    assert rc == 0
    assert (g_n, g_used) == (n, used) and (want_used is None or g_used == want_used)
    assert np.array_equal(g_ids, ids) and np.array_equal(g_f2s, f2s)
    rc, h_ids, h_n, h_used, h_f2s = run_select(c, poison=-3)
    assert rc == 0 and (h_n, h_used) == (g_n, g_used) and np.array_equal(h_ids, g_ids) and np.array_equal(h_f2s, g_f2s)


def test_select_refusals():
    lib = L()
    assert lib.vag_shortlist_supported(131072, 300, 8, 512) == 1
    assert lib.vag_shortlist_supported(131073, 300, 8, 512) == 0
    assert lib.vag_shortlist_supported(7, 300, 8, 7) == 0 and lib.vag_shortlist_supported(100, 300, 257, 50) == 0
    assert lib.vag_shortlist_supported(100, 300, 0, 50) == 0 and lib.vag_shortlist_supported(100, 300, 8, 101) == 0
    assert lib.vag_shortlist_supported(100, 300, 8, 7) == 0 and lib.vag_shortlist_supported(100, 0, 8, 50) == 0
    c = dict(R.cases()["largest_V"])
    assert run_select(dict(c, V=131073))[0] == -22                       # (the buffers are sized for it: nothing is launched)
    small = dict(R.cases()["V1000"])
    assert run_select(dict(small, best=7))[0] == -22                     # best > K
    assert run_select(dict(small, always=np.arange(small["cap"] + 1, dtype=np.int32)))[0] == -22      # A > cap
    assert run_select(dict(small, cap=1001))[0] == -22
    assert lib.vag_shortlist_select(None, None, 1, 1, None, 10, 2, 1, None, 0, 100, 16, None, None, None, None, None) == -22


# ------------------------------------------------------------------------------------------------------------------
# 2. gather
# ------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().contiguous().view(I32).cpu().numpy()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", [1, 3, 32, 36])
def test_gather(W, offset):
    V, cap, n = 50, 16, 9
    rng = np.random.default_rng(W * 2 + offset)
    ids_np = np.full(cap, -1, np.int32)
    ids_np[:n] = np.sort(rng.choice(V, n, replace=False))
    ids_np[0], ids_np[n - 1] = 0, V - 1                                   # the first and the last row of the source
    ids_np[:n] = np.sort(ids_np[:n])
    base = torch.randn(V * W + 4, device="cuda")
    base[offset + 2 * W] = float("nan")                                   # bit for bit: a NaN travels too
    src = base[offset:offset + V * W].view(V, W)                          # offset 1: 4 bytes off a 16-byte boundary
    assert src.data_ptr() % 16 == 4 * offset
    before = bits(base)
    pad = -1e30 if W == 1 else 0.0
    ids, cnt = dev(ids_np), dev(np.array([n], np.int32))
    out = torch.full((cap, W), 123.0, device="cuda")

    def run():
        rc = L().vag_shortlist_gather(ids.data_ptr(), cnt.data_ptr(), cap, src.data_ptr(), V, W, W, pad, out.data_ptr(), stream())
        torch.cuda.synchronize()
        return rc

    assert run() == 0
    want = np.full((cap, W), np.float32(pad), np.float32)
    src_bits = bits(base)[offset:offset + V * W].reshape(V, W)
    assert np.array_equal(bits(out)[:n], src_bits[ids_np[:n]])
    assert np.array_equal(out.cpu().numpy()[n:], want[n:])
    assert np.array_equal(bits(base), before)                             # the source is only read
    cnt.fill_(4)                                                          # a refill with a smaller n: the former rows become pads
    assert run() == 0
    assert np.array_equal(bits(out)[:4], src_bits[ids_np[:4]]) and np.array_equal(out.cpu().numpy()[4:], want[4:])
    assert L().vag_shortlist_gather(ids.data_ptr(), cnt.data_ptr(), cap, src.data_ptr(), V, W, W - 1, pad, out.data_ptr(),
                                    stream()) == -22
    assert L().vag_shortlist_gather(None, cnt.data_ptr(), cap, src.data_ptr(), V, W, W, pad, out.data_ptr(), stream()) == -22


def test_gather_with_a_row_stride():
    V, W, ld, cap, n = 20, 8, 12, 8, 5
    src = torch.randn(V, ld, device="cuda")
    ids_np = np.array([1, 3, 4, 10, 19, -1, -1, -1], np.int32)
    ids, cnt = dev(ids_np), dev(np.array([n], np.int32))
    out = torch.empty(cap, W, device="cuda")
    assert L().vag_shortlist_gather(ids.data_ptr(), cnt.data_ptr(), cap, src.data_ptr(), V, W, ld, 0.0, out.data_ptr(), stream()) == 0
    assert torch.equal(out[:n], src[torch.as_tensor(ids_np[:n]).long().cuda(), :W]) and bool((out[n:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# models, batches and the copies cut down by hand
# ------------------------------------------------------------------------------------------------------------------
def text_model(seed, tied=False, H=32):
    from machine_translation_vision.models import NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    return NMT_Seq2Seq_Beam_V2(VS, VT, E, E, H, tied_emb=tied).cuda().eval()


def mm_model(seed, tied=True, H=64):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(VS, VT, IM, E, E, H, 24, 0.99, tied_emb=tied).cuda().eval()


def make_batch(seed, lens):
    rng = np.random.default_rng(seed)
    B, Ts = len(lens), max(lens)
    src = np.zeros((B, Ts), np.int64)
    for b, n in enumerate(lens):
        src[b, :n] = rng.integers(4, VS, n)
    im = torch.from_numpy(rng.standard_normal((B, IM)).astype(np.float32)).abs().cuda()
    return dict(src_np=src, lens=list(lens), src=dev(src), im=im)


@pytest.fixture(scope="module")
def lex_np():
    return np.random.default_rng(5).integers(4, VT, size=(VS, K_LEX)).astype(np.int32)


@pytest.fixture(scope="module")
def batch_a():
    return make_batch(1, [7, 5, 3])


@pytest.fixture(scope="module")
def batch_b():
    return make_batch(2, [6, 6, 2])


def lexicon(lex_np):
    from vagnmt_hip.shortlist import Lexicon
    return Lexicon(lex_np, VT)


def shortlist(obj, lex_np, **kw):
    from vagnmt_hip.shortlist import Shortlist
    kw.setdefault("always", ALWAYS)
    kw.setdefault("capacity", CAP)
    kw.setdefault("best", BEST)
    return Shortlist(obj, lexicon(lex_np), **kw)


def ref_selection(batch, lex_np, always=ALWAYS, cap=CAP, best=BEST):
    return R.select(batch["src_np"], np.asarray(batch["lens"]), lex_np, best, always, VT, cap)


def hand_copy(model, ids, n, cap=CAP):
    """A deep copy of the model whose three vocabulary-sized tensors are cut down in torch: index_select with the reference's
    ids, then pad rows of 0 / -1e30 up to the capacity."""
    c = copy.deepcopy(model)
    d = c.decoder
    idx = torch.as_tensor(ids[:n].astype(np.int64)).cuda()
    tied = d.out.weight is d.embedding.weight

    def cut(t, pad):
        rows = t.detach().index_select(0, idx)
        tail = torch.full((cap - n,) + tuple(t.shape[1:]), pad, device=t.device)
        return torch.nn.Parameter(torch.cat([rows, tail], 0), requires_grad=False)

    d.embedding.weight = cut(d.embedding.weight, 0.0)
    d.out.weight = d.embedding.weight if tied else cut(d.out.weight, 0.0)
    d.out.bias = cut(d.out.bias, -1e30)
    c.tgt_size = cap
    c.decode_graph = model.decode_graph
    return c


def full_lists(x, ids):
    return [full_lists(v, ids) for v in x] if isinstance(x, list) else int(ids[int(x)])


def short_lists(x, f2s):
    if isinstance(x, list):
        return [short_lists(v, f2s) for v in x]
    return int(f2s[int(x)]) if f2s[int(x)] >= 0 else 1


def nbest_args(model, batch):
    a = [batch["src"], batch["lens"]]
    if hasattr(model, "vse_imagine") or hasattr(model, "models"):
        a.append(batch["im"])
    return a + [BEAM, NBEST]


def check_nbest(sl, obj_copy, batch, ids):
    hyps, scores = sl.beamsearch_nbest(*nbest_args(sl.obj, batch), max_length=MAXLEN)
    w_hyps, w_scores = obj_copy.beamsearch_nbest(*nbest_args(sl.obj, batch), max_length=MAXLEN)
    assert hyps == full_lists(w_hyps, ids)
    assert torch.equal(scores, w_scores)
    assert bool(torch.isfinite(scores).all()) and float(scores.min()) > -1e4          # no pad word surfaced
    return hyps, scores


# ------------------------------------------------------------------------------------------------------------------
# 3. map
# ------------------------------------------------------------------------------------------------------------------
def test_map_both_directions(lex_np, batch_a):
    sl = shortlist(text_model(3), lex_np)
    sel = sl.select(batch_a["src"], batch_a["lens"])
    ids, n, used, f2s = ref_selection(batch_a, lex_np)
    assert int(sel.n) == n and int(sel.rank_used) == used and np.array_equal(sel.ids.cpu().numpy(), ids)
    assert np.array_equal(sl.full2short.cpu().numpy(), f2s)
    rng = np.random.default_rng(0)
    for shape in [(23,), (2, 3, 5)]:
        x = rng.integers(0, VT, size=shape)
        absent = torch.zeros(1, dtype=I32, device="cuda")
        got = sl.to_short(dev(x), absent)
        want = np.where(f2s[x] >= 0, f2s[x], 1)
        assert got.shape == shape and got.dtype == I64 and np.array_equal(got.cpu().numpy(), want)
        assert int(absent) == int((f2s[x] < 0).sum()) > 0
        back = sl.to_full(got).cpu().numpy()
        present = f2s[x] >= 0
        assert np.array_equal(back[present], x[present]) and (back[~present] == 1).all()
        y = rng.integers(0, n, size=shape)                                            # compact -> full -> compact
        assert np.array_equal(sl.to_short(sl.to_full(dev(y))).cpu().numpy(), y)
    pad_slot = sl.to_full(dev(np.array([n, CAP - 1, CAP, -1, 10 ** 9])))             # pad slots and ids outside the table: UNK
    assert pad_slot.cpu().tolist() == [1] * 5
    lists = [[int(ids[5]), int(ids[n - 1])], [], [[3, int(ids[4])]]]
    assert sl.to_full(sl.to_short(lists)) == lists
    missing = int(np.nonzero(f2s < 0)[0][0])
    assert sl.to_short([missing, 0, 3]) == [1, 0, 3]
    with pytest.raises(ValueError):
        sl.to_short(torch.zeros(3, dtype=I64))                                        # a CPU tensor
    with pytest.raises(ValueError):
        sl.select(batch_a["src"].cpu(), batch_a["lens"])
    assert L().vag_shortlist_map(None, 4, sl.ids.data_ptr(), CAP, 0, None, None, stream()) == -22
    assert L().vag_shortlist_map(None, 0, sl.ids.data_ptr(), CAP, 0, None, None, stream()) == 0
    assert L().vag_shortlist_map(None, 4, None, CAP, 0, None, None, stream()) == -22


# ------------------------------------------------------------------------------------------------------------------
# 4. the equivalence
# ------------------------------------------------------------------------------------------------------------------
def build(kind):
    if kind == "text":
        return text_model(11)
    if kind == "text_tied":
        return text_model(12, tied=True)
    if kind == "multimodal":
        return mm_model(13)
    from vagnmt_hip.ensemble import Ensemble
    return Ensemble([mm_model(14), text_model(15, H=64)])


def copy_of(obj, ids, n):
    if hasattr(obj, "models"):
        from vagnmt_hip.ensemble import Ensemble
        e = Ensemble([hand_copy(m, ids, n) for m in obj.models])
        e.decode_graph = obj.decode_graph
        return e
    return hand_copy(obj, ids, n)


def set_graph(obj, on):
    obj.decode_graph = on
    for m in getattr(obj, "models", []):
        m.decode_graph = on


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["text", "text_tied", "multimodal", "ensemble"])
def test_equivalence_with_a_model_cut_down_by_hand(kind, graph, lex_np, batch_a):
    obj = build(kind)
    set_graph(obj, graph)
    ids, n, used, f2s = ref_selection(batch_a, lex_np)
    assert 8 < n <= CAP and used < BEST                                               # the cap rule is in play
    sl = shortlist(obj, lex_np)
    cp = copy_of(obj, ids, n)
    check_nbest(sl, cp, batch_a, ids)
    # forced scores of targets with and without words outside the shortlist
    outside = [int(w) for w in np.nonzero(f2s < 0)[0][:2]]
    tgt = [[int(ids[9]), outside[0], int(ids[n - 1])], [int(ids[8])], [outside[1], outside[0], int(ids[10]), 3]]
    extra = [batch_a["im"]] if kind in ("multimodal", "ensemble") else []
    got = sl.score_translations(batch_a["src"], batch_a["lens"], tgt, *extra)
    want = cp.score_translations(batch_a["src"], batch_a["lens"], short_lists(tgt, f2s), *extra)
    assert int(got.absent) == 3
    for a, b in zip(got[:3], want):
        assert torch.equal(a, b)
    assert abs(sl.coverage([(batch_a["src"], batch_a["lens"], tgt)]) - 0.7) < 1e-12   # 10 words, EOS included; 3 outside


def test_equivalence_of_device_rows_and_sampling(lex_np, batch_a):
    from vagnmt_hip.sampling import Generator
    obj = text_model(16)
    ids, n, used, f2s = ref_selection(batch_a, lex_np)
    sl, cp = shortlist(obj, lex_np), hand_copy(obj, ids, n)
    t_ids = torch.as_tensor(ids.astype(np.int64)).cuda()
    for beam in (1, BEAM):
        rows = sl.beamsearch_decode(batch_a["src"], batch_a["lens"], beam_size=beam, max_length=MAXLEN, device_rows=True)
        want = cp._decode(batch_a["src"], batch_a["lens"], None, beam, MAXLEN, None, device_rows=True)
        assert rows.is_cuda and rows.dtype == I64 and torch.equal(rows, t_ids[want])
        lists = sl.beamsearch_decode(batch_a["src"], batch_a["lens"], beam_size=beam, max_length=MAXLEN)
        assert lists == full_lists(cp.beamsearch_decode(batch_a["src"], batch_a["lens"], beam_size=beam, max_length=MAXLEN), ids)
    got = sl.sample_decode(batch_a["src"], batch_a["lens"], n_samples=3, max_length=MAXLEN, generator=Generator(7))
    want = cp.sample_decode(batch_a["src"], batch_a["lens"], n_samples=3, max_length=MAXLEN, generator=Generator(7))
    assert got.hyps == full_lists(want.hyps, ids)
    assert torch.equal(got.token_logp, want.token_logp) and torch.equal(got.logp, want.logp)
    assert bool(torch.isfinite(got.logp).all()) and float(got.token_logp.min()) > -1e4          # no pad word was drawn


# ------------------------------------------------------------------------------------------------------------------
# 5. refill under a captured graph
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text_tied", "multimodal"])
def test_refill_under_a_captured_graph(kind, lex_np, batch_a, batch_b):
    obj = build(kind)
    set_graph(obj, True)
    sl = shortlist(obj, lex_np)
    sel_a, sel_b = ref_selection(batch_a, lex_np), ref_selection(batch_b, lex_np)
    assert sel_a[1] != sel_b[1] and not np.array_equal(sel_a[0], sel_b[0])            # another n: pad rows move
    first = check_nbest(sl, copy_of(obj, sel_a[0], sel_a[1]), batch_a, sel_a[0])
    check_nbest(sl, copy_of(obj, sel_b[0], sel_b[1]), batch_b, sel_b[0])
    again = check_nbest(sl, copy_of(obj, sel_a[0], sel_a[1]), batch_a, sel_a[0])
    assert again[0] == first[0] and torch.equal(again[1], first[1])
    states = [st for st in sl.view._decode_cache.values() if isinstance(st, dict)]
    assert len(states) == 1 and states[0]["graph"] is not None                        # one shape, one key, one captured graph


# ------------------------------------------------------------------------------------------------------------------
# 6. the identity, 7. nothing else moved
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_identity_with_every_word_always_present(graph, lex_np, batch_a):
    model = mm_model(21)
    set_graph(model, graph)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    args = [batch_a["src"], batch_a["lens"], batch_a["im"]]
    before = model.beamsearch_nbest(*args, BEAM, NBEST, max_length=MAXLEN)
    sl = shortlist(model, lex_np, always=np.arange(VT), capacity=VT)
    hyps, scores = sl.beamsearch_nbest(*args, BEAM, NBEST, max_length=MAXLEN)
    assert int(sl.last.n) == VT and hyps == before[0] and torch.equal(scores, before[1])
    for beam in (1, BEAM):
        assert sl.beamsearch_decode(*args, beam_size=beam, max_length=MAXLEN) == \
            model.beamsearch_decode(*args, beam_size=beam, max_length=MAXLEN)
    # 7. the wrapped model: its parameters bit for bit, its own search bit for bit, and nothing shared with the view's vocabulary
    small = shortlist(model, lex_np)
    small.beamsearch_nbest(*args, BEAM, NBEST, max_length=MAXLEN)
    after = model.beamsearch_nbest(*args, BEAM, NBEST, max_length=MAXLEN)
    assert after[0] == before[0] and torch.equal(after[1], before[1])
    now = model.state_dict()
    assert sorted(now) == sorted(params)
    for k, v in params.items():
        assert torch.equal(now[k], v), k
    assert model.tgt_size == VT and model.decoder.out.bias.shape[0] == VT and model.training is False
    v = small.view
    assert isinstance(v, type(model)) and v is not model and v.tgt_size == CAP and v.decoder.out.bias.shape[0] == CAP
    assert v.encoder is model.encoder and v.decoder.gru_1 is model.decoder.gru_1 and v.decoder.W1 is model.decoder.W1
    assert v.decoder.out.weight is v.decoder.embedding.weight                         # tied: one compact buffer


# ------------------------------------------------------------------------------------------------------------------
# 8. another search through the view; the refusals
# ------------------------------------------------------------------------------------------------------------------
def test_constrained_search_through_the_view(lex_np, batch_a):
    model = text_model(31)
    ids, n, used, f2s = ref_selection(batch_a, lex_np)
    sl, cp = shortlist(model, lex_np), hand_copy(model, ids, n)
    free, _ = sl.beamsearch_nbest(batch_a["src"], batch_a["lens"], BEAM, 1, max_length=MAXLEN)
    banned = [[free[0][0][0] if free[0][0] else int(ids[8])]]                         # sentence 0's first word, nowhere
    prefix = [[], [int(ids[n - 2]), int(ids[9])], []]
    sl.select(batch_a["src"], batch_a["lens"])
    kw = dict(beam_size=BEAM, n_best=2, max_length=MAXLEN)
    got = sl.to_full(sl.view.beamsearch_constrained(batch_a["src"], batch_a["lens"], prefix=sl.to_short(prefix),
                                                    banned=sl.to_short(banned), **kw))
    want = cp.beamsearch_constrained(batch_a["src"], batch_a["lens"], prefix=short_lists(prefix, f2s),
                                     banned=short_lists(banned, f2s), **kw)
    assert type(got).__name__ == "Constrained" and got.hyps == full_lists(want.hyps, ids) and torch.equal(got.scores, want.scores)
    assert got.hyps[1][0][:2] == prefix[1]
    assert all(banned[0][0] not in h for sent in got.hyps for h in sent if h)


def test_refusals(lex_np, batch_a):
    from vagnmt_hip.ensemble import Ensemble
    model = text_model(41)
    sl = shortlist(model, lex_np)
    a = [batch_a["src"], batch_a["lens"]]
    with pytest.raises(ValueError, match="beam_size 5"):
        sl.beamsearch_nbest(*a, 5, 1, max_length=MAXLEN)                              # 8 always ids carry a beam of 4
    with pytest.raises(ValueError, match="beam_size 5"):
        sl.beamsearch_decode(*a, beam_size=5, max_length=MAXLEN)
    with pytest.raises(ValueError, match="beam_size 6"):
        sl.view.beamsearch_diverse(*a, beam_size=6, n_groups=2, max_length=MAXLEN)
    with pytest.raises(NotImplementedError, match="full target ids"):
        sl.view.beamsearch_lm(*a, lm=None)
    with pytest.raises(NotImplementedError, match="full target ids"):
        sl.view.beamsearch_knn(*a, datastore=None)
    with pytest.raises(NotImplementedError, match="decode-only"):
        sl.view(batch_a["src"], batch_a["lens"], batch_a["src"])
    ens = shortlist(Ensemble([model, text_model(42)]), lex_np)
    with pytest.raises(ValueError, match="beam_size 5"):
        ens.beamsearch_nbest(*a, None, 5, 1, max_length=MAXLEN)
    with pytest.raises(NotImplementedError, match="full target ids"):
        ens.view.beamsearch_lm(*a, lm=None)
    hyps, scores = sl.beamsearch_nbest(*a, 4, 1, max_length=MAXLEN)                   # the widest beam the always ids carry
    assert len(hyps) == 3 and bool(torch.isfinite(scores).all())
