"""GPU: attention alignments of the beam search and of forced decoding (vagnmt_hip.align) on the golden fixtures.

1. the search is unchanged: beamsearch_align returns beamsearch_nbest's token lists and scores bit for bit;
2. the attention of every returned hypothesis against the oracle's decoder step, teacher-forced on the hypothesis's own tokens
   (1e-4 absolute: the tolerance of test_gpu_round2.py for attention across kernels), including hypotheses whose ancestor slot
   changes between steps (the back-pointer walk);
3. shape rules: zero rows after the EOS row and from the steps run on, live rows sum to 1, masked columns are 0, src_pos is
   numpy.argmax of the returned rows;
4. forced alignment against the golden alpha_steps, and against the search's attention of the same hypothesis;
5. ensembles: two identical members give the member bit for bit, two different ones the mean of two oracle attentions;
6. the graph cache keeps aligning and plain searches apart."""
import numpy as np
import pytest
import torch

from test_gpu_nbest_score import FLAGS, golden_model, ints_nb, span_mask

pytestmark = pytest.mark.gpu

EOS = 3
FIXTURES = ["mm_dot_tied_s0_f32", "mm_mlp_untied_s1_f32", "text_tied_s0_f32", "mm_dot_tied_mid_f32"]
TOL = 1e-4


def inputs(meta, z):
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
    return src, meta["lengths"], im


def margs(m, src, lens, im):
    """(src, lengths[, im]): the leading arguments of a model's beamsearch_nbest / beamsearch_align."""
    return (src, lens, im) if hasattr(m, "vse_imagine") else (src, lens)


def oracle_attention(m, meta, src, lens, im, toks):
    """(L, B, Ts) attention of the oracle's decoder step, teacher-forced on toks (B, L), with the model's weights on the CPU."""
    from oracle import vag_oracle as O
    P = {n: p.detach().cpu().float() for n, p in m.named_parameters()}
    with torch.no_grad():
        enc, mask, h = O._decode_prologue(P, src.cpu(), lens, im.cpu() if meta["kind"] == "mm" else None, meta["init_split"],
                                          meta.get("attn", "dot"), True)
        tok = torch.full((src.shape[0],), 2, dtype=torch.long)
        out = []
        for t in range(toks.shape[1]):
            _, h, aux = O.decoder_step(P, tok, h, enc, mask)
            out.append(aux["alpha"])
            tok = toks[:, t]
    return torch.stack(out)


def forced_rows(hyps, j, max_length):
    """Hypothesis j of every sentence + EOS as a padded (B, L) tensor, and the lengths with the EOS."""
    rows = [list(h[j]) + [EOS] for h in hyps]
    assert all(len(r) <= max_length for r in rows)
    L = max(len(r) for r in rows)
    t = torch.zeros(len(rows), L, dtype=torch.long)
    for b, r in enumerate(rows):
        t[b, :len(r)] = torch.tensor(r)
    return t, [len(r) for r in rows]


def check_against_oracle(a, oracle, src, max_length, what):
    """Every returned hypothesis: attention[b, j, :len+1] against oracle(tokens of rank j) (L, B, Ts)."""
    att = a.attention.cpu()
    n = att.shape[1]
    worst = 0.0
    for j in range(n):
        toks, lens1 = forced_rows(a.hyps, j, max_length)
        ref = oracle(toks)
        for b, L1 in enumerate(lens1):
            err = (att[b, j, :L1] - ref[:L1, b]).abs().max().item()
            worst = max(worst, err)
            assert err <= TOL, (what, b, j, L1, err)
    print("%s: %d hypotheses, attention vs oracle max abs err %.3e" % (what, n * att.shape[0], worst))


def check_shape_rules(a, lens, max_length, steps, what):
    att = a.attention.cpu()
    pos = a.src_pos.cpu()
    B, n, ML, Ts = att.shape
    assert ML == max_length and pos.shape == (B, n, ML) and pos.dtype == torch.int64 and att.dtype == torch.float32
    for b in range(B):
        for j in range(n):
            live = min(len(a.hyps[b][j]) + 1, ML)            # the words and the row that produced EOS
            assert live <= steps or live == ML, (what, b, j, live, steps)
            assert bool((att[b, j, live:] == 0).all()) and bool((pos[b, j, live:] == -1).all()), (what, b, j)
            assert bool((att[b, j, steps:] == 0).all()) and bool((pos[b, j, steps:] == -1).all()), (what, b, j)
            live = min(live, steps)
            assert bool(((att[b, j, :live].sum(-1) - 1).abs() <= TOL).all()), (what, b, j, att[b, j, :live].sum(-1))
            assert bool((att[b, j, :, lens[b]:] == 0).all()), (what, b, j)             # masked source positions
            assert bool((pos[b, j, :live] >= 0).all()) and bool((pos[b, j, :live] < lens[b]).all()), (what, b, j)
            assert np.array_equal(pos[b, j, :live].numpy(), np.argmax(att[b, j, :live].numpy(), axis=-1)), (what, b, j)


def lift_eos(m, by):
    with torch.no_grad():
        m.decoder.out.bias[EOS] += by


def align_entry(m):
    """The decode-cache entry of the model's aligning beam search (graph mode)."""
    es = [st for key, st in m._decode_cache.items() if isinstance(key, tuple) and "align" in key]
    assert len(es) == 1, len(es)
    return es[0]


def slot_changes(st, max_length, steps):
    """Final slots (b, j) whose chain of ancestor slots is not constant: the parent of the slot at some step t >= 1 is another
    slot (read from the back-pointer half of the search buffer)."""
    par = st["beam"][max_length:max_length + steps].cpu().numpy()            # (steps, B, k)
    _, B, k = par.shape
    moved = []
    for b in range(B):
        for j in range(k):
            p, ch = j, False
            for t in range(steps - 1, 0, -1):
                q = int(par[t, b, p])
                ch = ch or q != p
                p = q
            if ch:
                moved.append((b, j))
    return moved


# ------------------------------------------------------------------------------------------------------------------
# 1. the search is unchanged
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_align_returns_the_nbest_search_bit_for_bit(name):
    m, meta, z = golden_model(name)
    src, lens, im = inputs(meta, z)
    lift_eos(m, 2.0)                                         # hypotheses end at mixed lengths
    ml = 10
    for graph in (True, False):
        m.decode_graph = graph
        for k in (1, 3, 12):
            for n in sorted({1, k}):
                for ad, au in FLAGS:
                    args = margs(m, src, lens, im) + (k, n, ml)
                    hyps, sc = m.beamsearch_nbest(*args, avoid_double=ad, avoid_unk=au)
                    a = m.beamsearch_align(*args, avoid_double=ad, avoid_unk=au)
                    assert ints_nb(a.hyps) == ints_nb(hyps), (name, graph, k, n, ad, au)
                    assert torch.equal(a.scores, sc), (name, graph, k, n, ad, au)
                    assert a.attention.shape == (src.shape[0], n, ml, src.shape[1]) and a.attention.is_cuda
                    assert a.src_pos.shape == (src.shape[0], n, ml) and a.src_pos.is_cuda
                    check_shape_rules(a, lens, ml, m.last_decode_steps, (name, graph, k, n, ad, au))


# ------------------------------------------------------------------------------------------------------------------
# 2. attention against the reference path (+ 3. shape rules)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eos_bias", [0.0, 2.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_attention_matches_oracle_along_every_hypothesis(name, eos_bias):
    """eos_bias 0: the fixture's weights as they are (random weights rarely end a sentence: every row is live); 2: the same
    weights with the EOS bias lifted on both sides, so that hypotheses end at mixed lengths."""
    m, meta, z = golden_model(name)
    src, lens, im = inputs(meta, z)
    lift_eos(m, eos_bias)
    ml = 12
    oracle = lambda toks: oracle_attention(m, meta, src, lens, im, toks)      # noqa: E731
    for graph in (True, False):
        m.decode_graph = graph
        for k, n in [(12, 12), (3, 2), (1, 1)]:
            a = m.beamsearch_align(*(margs(m, src, lens, im) + (k, n, ml)))
            steps = m.last_decode_steps
            check_against_oracle(a, oracle, src, ml, (name, eos_bias, graph, k))
            check_shape_rules(a, lens, ml, steps, (name, eos_bias, graph, k))
            if graph and k == 12:
                # the slot-0 chain alone would not exercise the back-pointer walk: some returned hypothesis (n = k: all of
                # them are returned) must descend from another slot than its own
                moved = slot_changes(align_entry(m), ml, steps)
                print("%s eos_bias %.1f: %d of %d hypotheses change their ancestor slot" % (name, eos_bias, len(moved),
                                                                                            src.shape[0] * k))
                assert len(moved) > 0, name


def test_rows_from_the_steps_run_on_are_zero_after_an_early_stop():
    """Once every hypothesis has emitted EOS the search stops (polled per chunk of steps): rows >= steps are zero."""
    m, meta, z = golden_model("mm_dot_tied_mid_f32")
    src, lens, im = inputs(meta, z)
    ml, steps = 40, 40
    for extra in (4.0, 4.0, 8.0, 16.0):                     # raise the EOS bias until the search ends early
        lift_eos(m, extra)
        a = m.beamsearch_align(src, lens, im, 12, 12, ml)
        steps = m.last_decode_steps
        if steps < ml:
            break
    assert steps < ml, steps
    check_shape_rules(a, lens, ml, steps, "early stop")
    assert bool((a.attention[:, :, steps:] == 0).all()) and bool((a.src_pos[:, :, steps:] == -1).all())
    oracle = lambda toks: oracle_attention(m, meta, src, lens, im, toks)      # noqa: E731
    check_against_oracle(a, oracle, src, ml, "early stop")
    hyps, sc = m.beamsearch_nbest(src, lens, im, 12, 12, ml)
    assert ints_nb(hyps) == ints_nb(a.hyps) and torch.equal(sc, a.scores)


# ------------------------------------------------------------------------------------------------------------------
# 4. forced alignment
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_forced_alignment_matches_golden_alpha(name):
    m, meta, z = golden_model(name)
    src, lens, im = inputs(meta, z)
    tgt = torch.from_numpy(z["tgt"]).cuda()
    m.train()                                                # (align_translations runs without dropout whatever the mode)
    f = m.align_translations(src, lens, tgt, im)
    assert m.training
    m.eval()
    B, Tt = tgt.shape
    assert f.attention.shape == (B, Tt, src.shape[1]) and f.src_pos.shape == (B, Tt) and f.src_pos.dtype == torch.int64
    want = torch.from_numpy(z["alpha_steps"]).permute(1, 0, 2)               # (Tt, B, Ts) -> (B, Tt, Ts)
    att, pos = f.attention.cpu(), f.src_pos.cpu()
    # the span rule of score_translations: up to and including the first EOS (to the last non-pad word if there is none)
    tgt_c = tgt.cpu()
    keep = torch.zeros(B, Tt, dtype=torch.bool)
    for b in range(B):
        row = tgt_c[b].tolist()
        end = row.index(EOS) if EOS in row else max([t for t, w in enumerate(row) if w != 0], default=-1)
        keep[b, :end + 1] = True
    err = ((att - want).abs() * keep.unsqueeze(-1)).max().item()
    print("%s: forced attention vs golden alpha_steps max abs err %.3e" % (name, err))
    assert err <= TOL, (name, err)
    assert bool((att[~keep] == 0).all()) and bool((pos[~keep] == -1).all())
    assert np.array_equal(pos[keep].numpy(), np.argmax(att[keep].numpy(), axis=-1))
    # a sentence with words after its first EOS, one without EOS
    t2 = tgt.clone()
    t2[0, 2] = EOS
    t2[1, :] = torch.where(t2[1] == EOS, torch.zeros_like(t2[1]), t2[1])
    f2 = m.align_translations(src, lens, t2, im)
    a2 = f2.attention.cpu()
    assert bool((a2[0, 3:] == 0).all()) and bool((f2.src_pos.cpu()[0, 3:] == -1).all())
    assert (a2[0, :3] - want[0, :3]).abs().max().item() <= TOL
    last = max(t for t, w in enumerate(t2[1].tolist()) if w != 0)
    assert bool((a2[1, last + 1:] == 0).all()) and bool((a2[1, :last + 1].sum(-1) > 0.5).all())
    assert (a2[1, :last + 1] - want[1, :last + 1]).abs().max().item() <= TOL
    # token lists (EOS appended) give what the padded tensor gives
    lists = [[int(w) for w in r[:r.index(EOS)]] if EOS in r else [int(w) for w in r if w != 0] for r in tgt_c.tolist()]
    f3 = m.align_translations(src, lens, lists, im)
    L3 = f3.attention.shape[1]
    assert (f3.attention.cpu() - att[:, :L3]).abs().max().item() <= TOL


@pytest.mark.parametrize("name", FIXTURES)
def test_forced_alignment_of_a_search_hypothesis_is_its_attention(name):
    m, meta, z = golden_model(name)
    src, lens, im = inputs(meta, z)
    lift_eos(m, 2.0)
    ml, k = 12, 12
    a = m.beamsearch_align(*(margs(m, src, lens, im) + (k, k, ml)))
    att = a.attention.cpu()
    worst = 0.0
    for j in range(k):
        lists = [h[j] for h in a.hyps]
        f = m.align_translations(src, lens, lists, im)
        L = f.attention.shape[1]
        assert L <= ml
        err = (f.attention.cpu() - att[:, j, :L]).abs().max().item()
        worst = max(worst, err)
        assert err <= TOL, (name, j, err)
        assert bool((att[:, j, L:] == 0).all())
    print("%s: forced vs search attention max abs err %.3e" % (name, worst))


# ------------------------------------------------------------------------------------------------------------------
# 5. ensembles
# ------------------------------------------------------------------------------------------------------------------
def test_ensemble_of_identical_members_is_the_member_bit_for_bit():
    from vagnmt_hip.ensemble import Ensemble
    for name in ("mm_dot_tied_s0_f32", "mm_dot_tied_mid_f32"):
        m, meta, z = golden_model(name)
        src, lens, im = inputs(meta, z)
        lift_eos(m, 2.0)
        ens = Ensemble([m, m])
        for graph in (True, False):
            m.decode_graph = ens.decode_graph = graph
            for k, n in [(12, 12), (3, 1)]:
                a = m.beamsearch_align(src, lens, im, k, n, 12)
                e = ens.beamsearch_align(src, lens, im, k, n, 12)
                assert ints_nb(a.hyps) == ints_nb(e.hyps) and torch.equal(a.scores, e.scores), (name, graph, k)
                assert torch.equal(a.attention, e.attention) and torch.equal(a.src_pos, e.src_pos), (name, graph, k)
        tgt = torch.from_numpy(z["tgt"]).cuda()
        f, g = m.align_translations(src, lens, tgt, im), ens.align_translations(src, lens, tgt, im)
        assert torch.equal(f.attention, g.attention) and torch.equal(f.src_pos, g.src_pos), name


def test_ensemble_attention_is_the_mean_of_the_members():
    from vagnmt_hip.ensemble import Ensemble
    m1, meta1, z = golden_model("mm_dot_tied_s0_f32")
    m2, meta2, _ = golden_model("mm_mlp_untied_s1_f32")          # same vocabularies, other weights and attention method
    m3, meta3, _ = golden_model("text_tied_s0_f32")
    src, lens, im = inputs(meta1, z)
    for m in (m1, m2, m3):
        lift_eos(m, 2.0)
    for members, metas in [((m1, m2), (meta1, meta2)), ((m1, m2, m3), (meta1, meta2, meta3))]:
        ens = Ensemble(list(members))

        def oracle(toks):
            return torch.stack([oracle_attention(m, mt, src, lens, im, toks) for m, mt in zip(members, metas)]).mean(0)
        for graph in (True, False):
            ens.decode_graph = graph
            a = ens.beamsearch_align(src, lens, im, 12, 12, 12)
            check_against_oracle(a, oracle, src, 12, ("ensemble", len(members), graph))
            check_shape_rules(a, lens, 12, ens.last_decode_steps, ("ensemble", len(members), graph))
            hyps, sc = ens.beamsearch_nbest(src, lens, im, 12, 12, 12)
            assert ints_nb(hyps) == ints_nb(a.hyps) and torch.equal(sc, a.scores)
        # forced: the mean of the members' forced attentions
        tgt = torch.from_numpy(z["tgt"]).cuda()
        f = ens.align_translations(src, lens, tgt, im)
        singles = [m.align_translations(src, lens, tgt, im) for m in members]
        want = torch.stack([s.attention for s in singles]).mean(0)
        assert (f.attention - want).abs().max().item() <= 1e-6
        assert bool(((f.attention.cpu() != 0).any(-1) <= (span_mask(tgt) > 0)).all())


# ------------------------------------------------------------------------------------------------------------------
# 6. graph cache
# ------------------------------------------------------------------------------------------------------------------
def test_graph_cache_keeps_aligning_and_plain_searches_apart():
    from vagnmt_hip.ensemble import Ensemble
    m, meta, z = golden_model("mm_dot_tied_mid_f32")
    src, lens, im = inputs(meta, z)
    lift_eos(m, 2.0)
    m.decode_graph = True
    k, ml = 12, 12
    h1, s1 = m.beamsearch_nbest(src, lens, im, k, k, ml)
    s1 = s1.clone()
    plain_keys = [key for key in m._decode_cache if isinstance(key, tuple)]
    assert len(plain_keys) == 1
    a = m.beamsearch_align(src, lens, im, k, k, ml)
    h2, s2 = m.beamsearch_nbest(src, lens, im, k, k, ml)
    assert ints_nb(h1) == ints_nb(h2) == ints_nb(a.hyps) and torch.equal(s1, s2) and torch.equal(s1, a.scores)
    keys = [key for key in m._decode_cache if isinstance(key, tuple)]
    assert len(keys) == 2 and plain_keys[0] in keys
    plain = m._decode_cache[plain_keys[0]]
    assert "attn_hist" not in plain and "alpha" not in plain and plain["graph"] is not None
    st = align_entry(m)
    assert st is not plain and st["graph"] is not None and st["graph"] is not plain["graph"]
    assert st["attn_hist"].shape == (ml, src.shape[0] * k, st["mask"].shape[1]) and st["alpha"].shape == st["attn_hist"].shape[1:]
    # a second aligning call replays the same graph on the same buffers
    hist, graph = st["attn_hist"], st["graph"]
    b = m.beamsearch_align(src, lens, im, k, k, ml)
    st2 = align_entry(m)
    assert st2["graph"] is graph and st2["attn_hist"] is hist
    assert torch.equal(a.attention, b.attention) and torch.equal(a.src_pos, b.src_pos) and ints_nb(a.hyps) == ints_nb(b.hyps)
    # the ensemble's cache: the same separation
    ens = Ensemble([m])
    e1, es1 = ens.beamsearch_nbest(src, lens, im, k, k, ml)
    es1 = es1.clone()
    ea = ens.beamsearch_align(src, lens, im, k, k, ml)
    e2, es2 = ens.beamsearch_nbest(src, lens, im, k, k, ml)
    assert ints_nb(e1) == ints_nb(e2) == ints_nb(ea.hyps) and torch.equal(es1, es2)
    ents = {key: e for key, e in ens._cache.items() if isinstance(key, tuple)}
    assert len(ents) == 2
    for key, e in ents.items():
        assert ("attn_hist" in e) == ("align" in key), key
    assert torch.equal(ea.attention, a.attention)


# ------------------------------------------------------------------------------------------------------------------
# configs[3]'s decode shape: the raw-logits form of the captured steps records too
# ------------------------------------------------------------------------------------------------------------------
def test_raw_logits_and_log_probability_forms_record_the_same_attention():
    """At this shape the decode path sums with fp32 atomics (test_gpu_round5.py: run-to-run spread): two calls of the SAME search
    differ in the last bits of their scores, so the comparisons here are at 1e-4 -- the attention tolerance of this file, and
    what test_gpu_nbest_score.py allows a token's log-probability -- not bit for bit as on the fixtures above."""
    from test_gpu_nbest_score import CFG3, LENS3, _cfg3_model, set_modes
    c = CFG3
    m, src, im = _cfg3_model(eos_bias=6.0)
    out = {}
    for graph, raw in [(True, True), (True, False), (False, True)]:
        set_modes(m, graph, True, raw)
        hyps, sc = m.beamsearch_nbest(src, LENS3, im, c["K"], 3, c["ML"])
        a = m.beamsearch_align(src, LENS3, im, c["K"], 3, c["ML"])
        assert ints_nb(a.hyps) == ints_nb(hyps), (graph, raw)
        err = (a.scores - sc).abs().max().item()
        print("configs[3] graph %s raw %s: align vs nbest scores max abs diff %.3e" % (graph, raw, err))
        assert err <= TOL, (graph, raw, err)
        check_shape_rules(a, LENS3, c["ML"], m.last_decode_steps, ("configs[3]", graph, raw))
        out[(graph, raw)] = a
    ref = out[(True, False)]
    for key, a in out.items():
        assert ints_nb(a.hyps) == ints_nb(ref.hyps), key
        err = (a.attention - ref.attention).abs().max().item()
        print("configs[3] %s: attention vs the log-probability form max abs diff %.3e" % (key, err))
        assert err <= TOL, (key, err)
        assert torch.equal(a.src_pos == -1, ref.src_pos == -1), key
