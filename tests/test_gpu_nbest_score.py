"""GPU: the beam search's options (avoid_double / avoid_unk), n-best lists and forced-decoding scores.

1. the options against the reference's own token lists (tests/golden/beam_opts.npz, tools/make_golden_beam_opts.py), under every
   combination of decode_graph / decode_hoisted / decode_raw_logits;
2. the options at configs[3]'s decode shape (V 9391: the raw-logits expansion runs there) and the decode caches' keys;
3. n-best: n = 1 is beamsearch_decode + last_beam_scores bit for bit (model, Ensemble M = 1 and 2), n = k is ordered;
4. score_translations against a float64 restatement from the oracle's decoder step; ensembles against the ens_score formula;
5. search <-> scoring: every finished n-best hypothesis scores, forced, what the search scored it."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

EOS, UNK = 3, 1
FLAGS = [(True, False), (False, False), (True, True), (False, True)]


def golden_model(name, unk_bias=0.0):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    meta, P, z = load_golden(name)
    Vs, Vt, I, E, H, S, B, Ts, Tt = meta["dims"]
    if meta["kind"] == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, meta["loss_w"], attn_model=meta["attn"],
                                                  tied_emb=meta["tied"], init_split=meta["init_split"])
    else:
        m = NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, tied_emb=meta["tied"])
    m.load_state_dict(P, strict=False)
    with torch.no_grad():
        m.decoder.out.bias[UNK] += unk_bias
    return m.cuda().eval(), meta, z


def make_model(kind, Vs, Vt, E, H, seed, attn="dot", tied=True, I=64, S=48):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    if kind == "mm":
        m = NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, 0.99, attn_model=attn, tied_emb=tied)
    else:
        m = NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, tied_emb=tied)
    return m.cuda().eval()


def make_inputs(Vs, B, Ts, I, lens, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(B, Ts, dtype=torch.long)
    for b, L in enumerate(lens):
        src[b, :L] = torch.randint(4, Vs, (L,), generator=g)
    return src.cuda(), torch.randn(B, I, generator=g).abs().cuda()


def ints(h):
    return [[int(t) for t in r] for r in h]


def public_beamsearch(m, src, lens, im, k, ml, ad, au):
    """The reference's public beamsearch(...) entry, fed from the model's own prologue in the reference's argument layout
    (time-major, decoder_input = the (B, 1) SOS tensor, as beamsearch_decode builds it: V11.py:186-188)."""
    with torch.no_grad():
        if hasattr(m, "vse_imagine"):
            enc, mask, _, h0 = m._prologue(src, lens, im, None, None)
        else:
            enc, mask, h0 = m._prologue(src, lens, None)
    sos = torch.full((src.shape[0], 1), 2, dtype=torch.int64, device="cuda")
    return ints(m.beamsearch(enc.transpose(0, 1), mask.t(), sos, h0.unsqueeze(0), k, ml, avoid_double=ad, avoid_unk=au))


def set_modes(m, graph, hoisted, raw):
    m.decode_graph, m.decode_hoisted, m.decode_raw_logits = graph, hoisted, raw


# ------------------------------------------------------------------------------------------------------------------
# 1. the options against the reference
# ------------------------------------------------------------------------------------------------------------------
def _beam_opts():
    z = np.load(os.path.join(GOLDEN, "beam_opts.npz"))
    return json.loads(bytes(z["meta"]).decode())


@pytest.mark.parametrize("modes", [(g, h, r) for g in (True, False) for h in (True, False) for r in (True, False)])
def test_options_match_reference(modes):
    fx = _beam_opts()
    for case in fx["cases"]:
        m, meta, z = golden_model(case["fixture"], fx["unk_bias"] if case["variant"] == "unk" else 0.0)
        set_modes(m, *modes)
        src = torch.from_numpy(z["src"]).cuda()
        im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
        for key, want in case["decode"].items():
            k, opt = key.split("/")
            k, ad, au = int(k), opt[0] == "1", opt[1] == "1"
            got = public_beamsearch(m, src, meta["lengths"], im, k, case["max_len"], ad, au)
            assert got == want, (case["fixture"], case["variant"], key, modes, got, want)
            # the n-best entry point runs the same search: its first list is the public one's
            args = (src, meta["lengths"]) + ((im,) if im is not None else ())
            hyps, _ = m.beamsearch_nbest(*args, beam_size=k, n_best=1, max_length=case["max_len"], avoid_double=ad,
                                         avoid_unk=au)
            assert [h[0] for h in ints_nb(hyps)] == want, (case["fixture"], key, modes)


def ints_nb(hyps):
    return [[[int(t) for t in r] for r in h] for h in hyps]


def test_public_beamsearch_options_need_the_reference_layout():
    """The options run on the reference's argument layout (decoder_input = the SOS tensor); decoder_input=None, this port's
    shorthand for it, stays the default search only and raises NotImplementedError with an option, as before."""
    fx = _beam_opts()
    for name in ("mm_dot_tied_s0_f32", "text_tied_s0_f32"):
        m, meta, z = golden_model(name)
        src = torch.from_numpy(z["src"]).cuda()
        im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
        case = [c for c in fx["cases"] if c["fixture"] == name and c["variant"] == "plain"][0]
        for key in ("2/11", "3/00", "12/01"):
            k, opt = key.split("/")
            got = public_beamsearch(m, src, meta["lengths"], im, int(k), case["max_len"], opt[0] == "1", opt[1] == "1")
            assert got == case["decode"][key], (name, key)
        with torch.no_grad():
            if im is not None:
                enc, mask, _, h0 = m._prologue(src, meta["lengths"], im, None, None)
            else:
                enc, mask, h0 = m._prologue(src, meta["lengths"], None)
        for ad, au in [(False, False), (True, True), (False, True)]:
            with pytest.raises(NotImplementedError):
                m.beamsearch(enc.transpose(0, 1), mask.t(), None, h0.unsqueeze(0), 2, 5, avoid_double=ad, avoid_unk=au)
        got = ints(m.beamsearch(enc.transpose(0, 1), mask.t(), None, h0.unsqueeze(0), 2, case["max_len"]))
        assert got == case["decode"]["2/10"], name                   # the default search with the shorthand, as before


# ------------------------------------------------------------------------------------------------------------------
# 2. configs[3]'s decode shape: the raw-logits expansion, and the cache keys of captured graphs
# ------------------------------------------------------------------------------------------------------------------
CFG3 = dict(Vs=8507, V=9391, I=2048, E=256, H=512, S=512, B=16, Ts=40, K=12, ML=80)
LENS3 = [40, 33, 30, 27, 25, 22, 20, 18, 17, 15, 13, 11, 9, 7, 5, 3]


def _cfg3_model(seed=31, unk_bias=0.0, eos_bias=0.0):
    c = CFG3
    m = make_model("mm", c["Vs"], c["V"], c["E"], c["H"], seed, I=c["I"], S=c["S"])
    with torch.no_grad():
        m.decoder.out.bias[UNK] += unk_bias
        m.decoder.out.bias[EOS] += eos_bias
    src, im = make_inputs(c["Vs"], c["B"], c["Ts"], c["I"], LENS3, seed + 100)
    return m, src, im


def _unk_bias_for(m, src, im):
    """A UNK bias under which UNK wins most of the first step's rows (the search then picks UNK unless it is masked)."""
    with torch.no_grad():
        sc = m.score_translations(src, LENS3, torch.full((src.shape[0], 1), UNK, dtype=torch.int64, device="cuda"), im)
    # token_logp of UNK at step 0 is log p(UNK); lifting the bias by -median(log p) makes p(UNK) ~ 1/2 on half the rows
    return float(-sc.token_logp[:, 0].median()) + 1.0


def test_options_raw_logits_and_cache_keys_at_config3():
    c = CFG3
    m, src, im = _cfg3_model()
    bias = _unk_bias_for(m, src, im)
    with torch.no_grad():
        m.decoder.out.bias[UNK] += bias
    out = {}
    for ad, au in FLAGS:
        for raw in (True, False):
            set_modes(m, True, True, raw)
            hyps, sc = m.beamsearch_nbest(src, LENS3, im, c["K"], 1, c["ML"], avoid_double=ad, avoid_unk=au)
            out[(ad, au, raw)] = ([h[0] for h in ints_nb(hyps)], sc.cpu().numpy().copy())
        assert out[(ad, au, True)][0] == out[(ad, au, False)][0], (ad, au)
        if au:                                                    # no UNK after step 0 under avoid_unk
            assert all(UNK not in h[1:] for h in out[(ad, au, True)][0]), (ad, au)
    assert out[(True, True, True)][0] != out[(True, False, True)][0]          # the bias makes avoid_unk matter
    assert sum(h.count(UNK) for h in out[(True, False, True)][0]) > 10
    # defaults -> avoid_unk -> defaults with graphs on, each against its eager run: a graph captured for one option set must
    # not be replayed for another (flags are part of _decode_state's key)
    for raw in (True, False):
        seq = []
        for ad, au in [(True, False), (True, True), (True, False), (False, True)]:
            set_modes(m, True, True, raw)
            g = public_beamsearch(m, src, LENS3, im, c["K"], c["ML"], ad, au)
            set_modes(m, False, True, raw)
            e = public_beamsearch(m, src, LENS3, im, c["K"], c["ML"], ad, au)
            assert g == e, (raw, ad, au)
            seq.append(g)
        assert seq[0] == seq[2] and seq[0] != seq[1]
    # defaults are today's decode
    set_modes(m, True, True, True)
    plain = ints(m.beamsearch_decode(src, LENS3, im, c["K"], c["ML"]))
    assert plain == out[(True, False, True)][0]


def test_ensemble_options_and_cache_key():
    from vagnmt_hip.ensemble import Ensemble
    fx = _beam_opts()
    case = [cs for cs in fx["cases"] if cs["fixture"] == "mm_dot_tied_s0_f32" and cs["variant"] == "unk"][0]
    m, meta, z = golden_model(case["fixture"], fx["unk_bias"])
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda()
    ens = Ensemble([m])
    for graph in (True, False):
        ens.decode_graph = graph
        for key in ["12/10", "12/11", "12/10", "3/01", "3/00", "2/11"]:
            k, opt = key.split("/")
            hyps, _ = ens.beamsearch_nbest(src, meta["lengths"], im, int(k), 1, case["max_len"], avoid_double=opt[0] == "1",
                                           avoid_unk=opt[1] == "1")
            assert [h[0] for h in ints_nb(hyps)] == case["decode"][key], (graph, key)


# ------------------------------------------------------------------------------------------------------------------
# 3. n-best
# ------------------------------------------------------------------------------------------------------------------
def test_nbest_top1_is_beamsearch_decode_and_lists_are_ordered():
    from vagnmt_hip.ensemble import Ensemble
    m, meta, z = golden_model("mm_dot_tied_mid_f32")
    Vs, Vt, I, E, H, S = meta["dims"][:6]
    m2 = make_model("mm", Vs, Vt, E, H, seed=5, I=I, S=S)
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda()
    lens, ml = meta["lengths"], 20
    for obj in (m, Ensemble([m]), Ensemble([m, m2])):
        for graph in (True, False):
            obj.decode_graph = graph
            for k in (1, 3, 12):
                if k > 1:
                    want = ints(obj.beamsearch_decode(src, lens, im, k, ml))
                    want_sc = obj.last_beam_scores.cpu().clone()
                    hyps, sc = obj.beamsearch_nbest(src, lens, im, k, 1, ml)
                    assert [h[0] for h in ints_nb(hyps)] == want
                    assert torch.equal(sc[:, 0].cpu(), want_sc)                      # bit for bit
                hyps, sc = obj.beamsearch_nbest(src, lens, im, k, k, ml)
                sc = sc.cpu()
                assert sc.shape == (src.shape[0], k) and all(len(h) == k for h in hyps)
                assert bool((sc[:, 1:] <= sc[:, :-1]).all()), sc
                if k > 1:
                    assert [h[0] for h in ints_nb(hyps)] == want and torch.equal(sc[:, 0], want_sc)


def test_nbest_argument_errors():
    m, meta, z = golden_model("text_tied_s0_f32")
    src = torch.from_numpy(z["src"]).cuda()
    for k, n in [(3, 0), (3, 4), (65, 2)]:
        with pytest.raises(ValueError):
            m.beamsearch_nbest(src, meta["lengths"], k, n, 10)


# ------------------------------------------------------------------------------------------------------------------
# 4. forced scores against a float64 restatement
# ------------------------------------------------------------------------------------------------------------------
def restate_token_logp(m, src, lens, im, tgt):
    """float64 log p(y_t) per position from the oracle's prologue and decoder step (teacher forced), 0 at pad / after EOS."""
    from oracle import vag_oracle as O
    P = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
    mm = hasattr(m, "vse_imagine")
    src, tgt = src.cpu(), tgt.cpu()
    with torch.no_grad():
        enc, mask, h = O._decode_prologue(P, src, lens, im.cpu().double() if mm else None, 0.5, getattr(m, "attn_model", "dot"),
                                          True)
        pe = enc.transpose(0, 1) @ P["decoder.attn.attn_e.weight"].t()
        B, Tt = tgt.shape
        tok = torch.full((B,), 2, dtype=torch.long)
        out = torch.zeros(B, Tt, dtype=torch.float64)
        for t in range(Tt):
            logp, h, _ = O.decoder_step(P, tok, h, enc, mask, pe=pe)
            out[:, t] = logp.gather(1, tgt[:, t:t + 1]).squeeze(1)
            tok = tgt[:, t]
    return span_mask(tgt) * out


def span_mask(tgt):
    tgt = tgt.cpu()
    B, Tt = tgt.shape
    keep = torch.zeros(B, Tt, dtype=torch.float64)
    for b in range(B):
        row = tgt[b].tolist()
        end = row.index(EOS) if EOS in row else max([t for t, w in enumerate(row) if w != 0], default=-1)
        for t in range(end + 1):
            keep[b, t] = 1.0 if row[t] != 0 else 0.0
    return keep


def restate_scores(tok_lp, tgt):
    keep = span_mask(tgt)
    logp = tok_lp.sum(1)
    words = ((tgt.cpu() > 3).double() * keep).sum(1).clamp(min=1)
    return logp / words, logp


def check_scores(got, tok_lp, tgt, tol, what):
    score, logp = restate_scores(tok_lp, tgt)
    e_tok = (got.token_logp.cpu().double() - tok_lp).abs().max().item()
    e_lp = (got.logp.cpu().double() - logp).abs().max().item()
    e_sc = (got.score.cpu().double() - score).abs().max().item()
    print("%s: max abs err token_logp %.2e logp %.2e score %.2e" % (what, e_tok, e_lp, e_sc))
    assert e_tok <= tol and e_lp <= tol * tgt.shape[1] and e_sc <= tol * tgt.shape[1], (what, e_tok, e_lp, e_sc)
    assert bool(((got.token_logp.cpu() != 0) <= (span_mask(tgt) > 0)).all())          # exactly 0 outside the span


@pytest.mark.parametrize("name", ["mm_dot_tied_s0_f32", "text_tied_s0_f32", "mm_dot_tied_mid_f32", "mm_mlp_untied_s1_f32"])
def test_scores_match_oracle_golden(name):
    m, meta, z = golden_model(name)
    src = torch.from_numpy(z["src"]).cuda()
    im = torch.from_numpy(z["im"]).cuda() if meta["kind"] == "mm" else None
    tgt = torch.from_numpy(z["tgt"]).cuda()
    tgt[0, 2] = EOS                                        # a sentence with words after its first EOS (they do not count)
    tgt[1, :] = torch.where(tgt[1] == EOS, torch.zeros_like(tgt[1]), tgt[1])           # one without EOS
    args = (src, meta["lengths"], tgt) + ((im,) if im is not None else ())
    m.train()                                              # (score_translations runs without dropout whatever the mode)
    got = m.score_translations(*args)
    assert m.training
    m.eval()
    check_scores(got, restate_token_logp(m, src, meta["lengths"], im, tgt), tgt, 1e-4, name)
    # a list of token lists: EOS appended, padded with 0 -- the same scores as the padded tensor
    lists = [[int(w) for w in r if w != 0] for r in tgt.cpu()]
    lists = [r[:r.index(EOS)] if EOS in r else r for r in lists]
    t2 = torch.zeros_like(tgt)
    for b, r in enumerate(lists):
        t2[b, :len(r) + 1] = torch.tensor(r + [EOS])
    got_l = m.score_translations(*((src, meta["lengths"], lists) + ((im,) if im is not None else ())))
    got_t = m.score_translations(*((src, meta["lengths"], t2) + ((im,) if im is not None else ())))
    assert torch.equal(got_l.score, got_t.score) and torch.equal(got_l.logp, got_t.logp)


@pytest.mark.timeout(1500)
def test_scores_match_oracle_at_config1():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    Vs, V, I, B, T = 8507, 9391, 2048, 64, 40
    m = make_model("mm", Vs, V, 256, 512, seed=41, I=I, S=512)
    g = torch.Generator().manual_seed(42)
    lens = sorted([int(x) for x in torch.randint(3, T + 1, (B,), generator=g)], reverse=True)
    lens[0] = T
    src, im = make_inputs(Vs, B, T, I, lens, 43)
    tgt = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        L = int(torch.randint(2, T + 1, (1,), generator=g))
        tgt[b, :L - 1] = torch.randint(4, V, (L - 1,), generator=g)
        tgt[b, L - 1] = EOS
    tgt = tgt.cuda()
    got = m.score_translations(src, lens, tgt, im)
    check_scores(got, restate_token_logp(m, src, lens, im, tgt), tgt, 2e-4, "configs[1]")


def _ens_combine(tok_lps):
    x = torch.stack([t.double() for t in tok_lps])
    mx = x.max(0).values
    return mx + torch.log(torch.exp(x - mx).sum(0) / len(tok_lps))


@pytest.mark.parametrize("M", [2, 3])
def test_ensemble_scores(M):
    from vagnmt_hip.ensemble import Ensemble
    Vs, Vt = 70, 503
    ms = [make_model("mm", Vs, Vt, 32, 64, seed=51, attn="dot"), make_model("mm", Vs, Vt, 40, 96, seed=52, attn="mlp", tied=False),
          make_model("text", Vs, Vt, 24, 48, seed=53)][:M]
    lens = [12, 10, 7, 5, 2]
    src, im = make_inputs(Vs, 5, 12, 64, lens, seed=54)
    g = torch.Generator().manual_seed(55)
    tgt = torch.randint(4, Vt, (5, 9), generator=g)
    tgt[0, 8] = EOS
    tgt[2, 4] = EOS
    tgt[3, 6:] = 0
    tgt = tgt.cuda()
    singles = [m.score_translations(src, lens, tgt, im) if hasattr(m, "vse_imagine") else m.score_translations(src, lens, tgt)
               for m in ms]
    got = Ensemble(ms).score_translations(src, lens, tgt, im)
    want_tok = _ens_combine([s.token_logp.cpu() for s in singles]) * span_mask(tgt)
    check_scores(got, want_tok, tgt, 2e-6, "ensemble M=%d" % M)
    # M identical members: the single model bit for bit
    same = Ensemble([ms[0]] * M).score_translations(src, lens, tgt, im)
    for a, b in zip(same, singles[0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 5. search <-> scoring at configs[3]'s decode shape
# ------------------------------------------------------------------------------------------------------------------
def _finished(obj, src, im):
    c = CFG3
    hyps, sc = obj.beamsearch_nbest(src, LENS3, im, c["K"], c["K"], c["ML"])
    sc = sc.cpu().numpy()
    idx = [(b, r) for b in range(len(hyps)) for r in range(c["K"])
           if len(hyps[b][r]) < c["ML"] - 1 and sc[b, r] > -1e4]           # emitted EOS before max_length, no penalty step
    return hyps, sc, idx


def _search_vs_scoring(obj, members, src, im, what):
    c = CFG3
    # raise the EOS bias of untrained members step by step until enough hypotheses end inside max_length at mixed lengths
    for extra in (0.5, 0.5, 1.0, 1.0, 1.0, 2.0):
        for m in members:
            with torch.no_grad():
                m.decoder.out.bias[EOS] += extra
        hyps, sc, idx = _finished(obj, src, im)
        if len(idx) >= 24 and len(set(len(hyps[b][r]) for b, r in idx)) >= 4:
            break
    assert len(idx) >= 24, (what, len(idx))
    B, n = len(hyps), c["K"]
    # repeat each source row n times (repeat_interleave keeps the descending length order), score all B n lists at once
    src_n = src.repeat_interleave(n, 0)
    im_n = im.repeat_interleave(n, 0)
    lens_n = [L for L in LENS3 for _ in range(n)]
    flat = [list(hyps[b][r]) for b in range(B) for r in range(n)]
    got = obj.score_translations(src_n, lens_n, flat, im_n)
    f = got.score.cpu().numpy().reshape(B, n)
    err = max(abs(float(f[b, r]) - float(sc[b, r])) for b, r in idx)
    rel = max(abs(float(f[b, r]) - float(sc[b, r])) / max(1.0, abs(float(sc[b, r]))) for b, r in idx)
    print("%s: %d finished hypotheses, forced vs search score: max abs err %.3e, max rel err %.3e" % (what, len(idx), err, rel))
    assert rel <= 2e-4, (what, err, rel)


def _models(seeds):
    ms = [_cfg3_model(seed=s) for s in seeds]
    return [x[0] for x in ms], ms[0][1], ms[0][2]


@pytest.mark.timeout(1500)
def test_search_scores_match_forced_scores_single():
    ms, src, im = _models([61])
    _search_vs_scoring(ms[0], ms, src, im, "single model")


@pytest.mark.timeout(1500)
def test_search_scores_match_forced_scores_ensemble():
    from vagnmt_hip.ensemble import Ensemble
    ms, src, im = _models([61, 62, 63])
    _search_vs_scoring(Ensemble(ms), ms, src, im, "ensemble M=3")
