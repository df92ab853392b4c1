"""GPU: ensemble decoding (vagnmt_hip.ensemble, vag_beam_ens_step*, vag_ens_argmax) against the single model and against a
float64 restatement built from the oracle's decoder step.

The ensemble's score of word w for hypothesis n is s = mx + log(sum_m exp(x_m - mx) / M), mx = max_m x_m, x_m = member m's
log_softmax row; the search rules are those of models/...V11.py:207-226 (greedy) and :233-337 (beam) applied to s."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EOS = 3


def make_model(kind, Vs, Vt, E, H, seed, attn="dot", tied=True, I=64, S=48):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    torch.manual_seed(seed)
    if kind == "mm":
        return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, 0.99, attn_model=attn, tied_emb=tied)
    return NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, tied_emb=tied)


def make_inputs(Vs, B, Ts, I, lens, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.zeros(B, Ts, dtype=torch.long)
    for b, L in enumerate(lens):
        src[b, :L] = torch.randint(4, Vs, (L,), generator=g)
    im = torch.randn(B, I, generator=g).abs()
    return src, im


def combine(xs):
    """The ensemble's score, in the form the kernels compute it (float64 here)."""
    if len(xs) == 1:
        return xs[0]
    x = torch.stack(xs)
    mx = x.max(0).values
    return mx + torch.log(torch.exp(x - mx).sum(0) / len(xs))


class _Restated:
    """One member in float64 on the CPU: the oracle's prologue and decoder step."""

    def __init__(self, m, src, lens, im):
        from oracle import vag_oracle as O
        self.O = O
        self.P = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
        mm = hasattr(m, "vse_imagine")
        self.enc, self.mask, self.h = O._decode_prologue(self.P, src, lens, im.double() if mm else None, 0.5,
                                                         getattr(m, "attn_model", "dot"), True)
        self.pe = self.enc.transpose(0, 1) @ self.P["decoder.attn.attn_e.weight"].t()       # (B,Ts,C): hoisted W_e enc

    def step(self, tok, rows=None):
        enc, mask, pe = self.enc, self.mask, self.pe
        if rows is not None:
            enc, mask, pe = enc[:, rows], mask[:, rows], pe[rows]
        logp, self.h, _ = self.O.decoder_step(self.P, tok, self.h, enc, mask, pe=pe)
        return logp


def restate_greedy(models, src, lens, im, steps):
    with torch.no_grad():
        mem = [_Restated(m, src, lens, im) for m in models]
        B = src.shape[0]
        tok = torch.full((B,), 2, dtype=torch.long)
        out = []
        for _ in range(steps):
            s = combine([r.step(tok) for r in mem])
            mxv = s.max(1, keepdim=True).values
            idx = torch.arange(s.shape[1]).expand_as(s)
            tok = torch.where(s == mxv, idx, s.shape[1]).min(1).values          # ties: the lowest word index
            out.append(tok)
        rows = torch.stack(out, 1).tolist()
    return [r[:r.index(EOS)] if EOS in r else r for r in rows]


def restate_beam(models, src, lens, im, k, max_length):
    """V11.py:233-337 on the ensemble's scores, selection under (score desc, flat index asc), history as back-pointers."""
    with torch.no_grad():
        mem = [_Restated(m, src, lens, im) for m in models]
        B = src.shape[0]
        V = mem[0].P["decoder.out.bias"].shape[0]
        tok = torch.full((B,), 2, dtype=torch.long)
        words, parents = [], []
        nll = None
        tile = torch.arange(B * k) // k
        for di in range(max_length):
            if di == 0:
                s = combine([r.step(tok) for r in mem])                                    # (B, V)
                cand = s
            else:
                cur = words[-1].reshape(-1)
                if bool((cur == EOS).all()):
                    break                                                                     # :266-269
                xs = []
                for r in mem:
                    r.h = r.h[tile]                                                           # :273
                    xs.append(r.step(cur, torch.arange(B * k) // k))
                s = combine(xs).clone()
                s[torch.arange(B * k), cur] = -1e5                                            # :279-280
                fin = cur == EOS
                s[fin] = -1e5                                                                 # :291-294
                s[fin, EOS] = 0.0
                cand = (nll.reshape(-1, 1) + s).reshape(B, k * V)                             # :297
            vals, idx = torch.sort(cand, dim=1, descending=True, stable=True)
            nll, idx = vals[:, :k], idx[:, :k]
            words.append(idx % V)
            parents.append(idx // V)
            k_in = 1 if di == 0 else k
            tile = (parents[-1] + torch.arange(B).unsqueeze(1) * k_in).reshape(-1)
        steps = len(words)
        hyps, scores = [], []
        for b in range(B):
            best, best_j, best_row = None, None, None
            for j in range(k):
                p, row, ln = j, [], 0
                for t in range(steps - 1, -1, -1):
                    w = int(words[t][b, p])
                    row.append(w)
                    if t < max_length - 1 and w > 3:
                        ln += 1
                    p = int(parents[t][b, p])
                row = row[::-1] + [0] * (max_length - steps)
                row[max_length - 1] = EOS
                sc = float(nll[b, j]) / max(ln, 1)
                if best is None or sc > best:
                    best, best_j, best_row = sc, j, row
            hyps.append(best_row[:best_row.index(EOS)])
            scores.append(best)
    return hyps, np.array(scores)


def _decode(obj, src, lens, im, k, ml, graph):
    obj.decode_graph = graph
    args = (src.cuda(), lens) + ((im.cuda(),) if im is not None else ())
    hyps = [[int(t) for t in h] for h in obj.beamsearch_decode(*args, beam_size=k, max_length=ml)]
    sc = obj.last_beam_scores.cpu().numpy().copy() if k > 1 else None
    return hyps, sc


# ------------------------------------------------------------------------------------------------------------------
# 1. M = 1 is the model itself
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mm", "text"])
def test_single_member_equals_model(kind):
    from vagnmt_hip.ensemble import Ensemble
    Vs, Vt, B, Ts, I = 60, 157, 5, 11, 64
    m = make_model(kind, Vs, Vt, 32, 48, seed=3).cuda().eval()
    with torch.no_grad():
        m.decoder.out.bias[EOS] += 1.0
    m.decode_raw_logits = False
    m.decode_persistent = False
    src, im = make_inputs(Vs, B, Ts, I, [11, 9, 7, 4, 2], seed=4)
    imv = im if kind == "mm" else None
    ens = Ensemble([m])
    for graph in (True, False):
        for k in (12, 1):
            if kind == "mm":
                m.decode_graph = graph
                want = [[int(t) for t in h] for h in m.beamsearch_decode(src.cuda(), [11, 9, 7, 4, 2], im.cuda(), k, 14)]
            else:
                m.decode_graph = graph
                want = [[int(t) for t in h] for h in m.beamsearch_decode(src.cuda(), [11, 9, 7, 4, 2], k, 14)]
            want_sc = m.last_beam_scores.cpu().numpy().copy() if k > 1 else None
            got, sc = _decode(ens, src, [11, 9, 7, 4, 2], imv, k, 14, graph)
            assert got == want, (kind, graph, k)
            if k > 1:
                assert np.array_equal(sc.view(np.int32), want_sc.view(np.int32)), (kind, graph, sc, want_sc)
                assert ens.last_decode_steps == m.last_decode_steps


# ------------------------------------------------------------------------------------------------------------------
# 2. M identical copies are the single model, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def test_identical_copies_equal_one_model():
    from vagnmt_hip.ensemble import Ensemble
    Vs, Vt, B, Ts, I = 60, 211, 5, 10, 64
    m = make_model("mm", Vs, Vt, 32, 64, seed=5).cuda().eval()
    with torch.no_grad():
        m.decoder.out.bias[EOS] += 1.0
    m.decode_raw_logits = False
    m.decode_persistent = False
    copies = [copy.deepcopy(m) for _ in range(3)]
    ptrs = {p.data_ptr() for c in copies for p in c.parameters()}
    assert len(ptrs) == 3 * len(list(m.parameters()))              # separate parameter storage
    src, im = make_inputs(Vs, B, Ts, I, [10, 8, 6, 5, 1], seed=6)
    lens = [10, 8, 6, 5, 1]
    ens = Ensemble(copies)
    for graph in (True, False):
        for k in (12, 1):
            want, want_sc = _decode(m, src, lens, im, k, 16, graph)
            got, sc = _decode(ens, src, lens, im, k, 16, graph)
            assert got == want, (graph, k)
            if k > 1:
                assert np.array_equal(sc.view(np.int32), want_sc.view(np.int32)), (graph, sc, want_sc)


# ------------------------------------------------------------------------------------------------------------------
# 3. distinct members against the float64 restatement
# ------------------------------------------------------------------------------------------------------------------
def _distinct(case):
    Vs, Vt = 70, 503
    if case == "m2":
        ms = [make_model("mm", Vs, Vt, 32, 256, seed=11, attn="dot"),
              make_model("mm", Vs, Vt, 48, 512, seed=12, attn="mlp", tied=False)]
    else:
        ms = [make_model("mm", Vs, Vt, 32, 64, seed=13, attn="dot"),
              make_model("mm", Vs, Vt, 40, 96, seed=14, attn="mlp", tied=False),
              make_model("text", Vs, Vt, 24, 48, seed=15)]
    for m in ms:
        m.eval()
        with torch.no_grad():
            m.decoder.out.bias[EOS] += 1.0            # let some hypotheses finish inside max_length (finished-beam rules)
    lens = [12, 10, 7, 5, 2]
    src, im = make_inputs(Vs, 5, 12, 64, lens, seed=16)
    return ms, src, lens, im


@pytest.mark.parametrize("case", ["m2", "m3_mixed"])
def test_distinct_members_match_restatement(case):
    from vagnmt_hip.ensemble import Ensemble
    ms, src, lens, im = _distinct(case)
    want = {k: restate_beam(ms, src, lens, im, k, 20) for k in (3, 5)}
    want_g = restate_greedy(ms, src, lens, im, 20)
    ens = Ensemble([m.cuda() for m in ms])
    finished_early = False
    for graph in (True, False):
        for k in (3, 5):
            got, sc = _decode(ens, src, lens, im, k, 20, graph)
            assert got == want[k][0], (case, graph, k, got, want[k][0])
            assert np.allclose(sc, want[k][1], rtol=0, atol=1e-4), (case, graph, k, np.abs(sc - want[k][1]).max())
            finished_early |= any(len(h) < 19 for h in got)
        got_g, _ = _decode(ens, src, lens, im, 1, 20, graph)
        assert got_g == want_g, (case, graph)
    assert finished_early                              # the finished-hypothesis rules were exercised


# ------------------------------------------------------------------------------------------------------------------
# 4. configs[3] size: V = 9391, H = 512, B = 16, beam 12, max_length 80, M = 3
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1500)
def test_three_members_at_config_size():
    from vagnmt_hip.ensemble import Ensemble
    Vs, Vt, I = 8507, 9391, 2048
    lens = [40, 33, 30, 27, 25, 22, 20, 18, 17, 15, 13, 11, 9, 7, 5, 3]
    ms = [make_model("mm", Vs, Vt, 256, 512, seed=21 + i, attn="dot" if i != 1 else "mlp", I=I, S=512) for i in range(3)]
    for m in ms:
        m.eval()
        with torch.no_grad():
            m.decoder.out.bias[EOS] += 0.5          # (mixed lengths at this size: some sentences end early, some run 80 steps)
    src, im = make_inputs(Vs, 16, 40, I, lens, seed=22)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want, want_sc = restate_beam(ms, src, lens, im, 12, 80)
    ens = Ensemble([m.cuda() for m in ms])
    got, sc = _decode(ens, src, lens, im, 12, 80, True)
    same = [a == b for a, b in zip(got, want)]
    for b, ok in enumerate(same):
        if not ok:
            print("sentence %d differs: score gap %.3e" % (b, abs(sc[b] - want_sc[b])))
            assert abs(sc[b] - want_sc[b]) < 1e-4
    assert sum(same) >= 15, [b for b, ok in enumerate(same) if not ok]
    assert np.allclose(sc, want_sc, rtol=2e-4, atol=2e-4), np.abs(sc - want_sc).max()      # (the single-model test's bound)


# ------------------------------------------------------------------------------------------------------------------
# 5. the expansion kernel itself: selection under the total order, M hidden states re-ordered
# ------------------------------------------------------------------------------------------------------------------
def _ens_scores_ref(xs):
    """The combined scores in float64 from the fp32 inputs, rounded to fp32.  The device's expf / logf may differ from this by an
    ulp, so scores are compared to 1e-6; candidates whose M inputs are equal tie exactly on both sides (M identical rows give
    s == x bit for bit), so the order among ties is compared exactly."""
    x = torch.stack([t.double() for t in xs])
    mx = x.max(0).values
    return (mx + torch.log(torch.exp(x - mx).sum(0) / len(xs))).float()


def _logp_rows(M, N, V, ldl, g, case):
    """M log-probability matrices padded with NaN columns (never read).  "random": distinct rows; "ties": M copies of one
    quantised matrix (thousands of exact ties on every value)."""
    xs = []
    for i in range(M):
        if case == "random" or i == 0:
            x = torch.log_softmax(torch.randn(N, V, generator=g) * 3, dim=1)
            if case == "ties":
                x = (x * 2).round() / 2
        xp = torch.full((N, ldl), float("nan"))
        xp[:, :V] = x
        xs.append(xp.cuda().contiguous())
    return xs


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("case", ["random", "ties"])
def test_ens_expansion_selection_matches_total_order(M, case):
    import ctypes as C
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import call, ptr
    B, V, ML = 5, 9391, 10
    ldl = (V + 3) // 4 * 4
    Hs = [32, 20, 48][:M]
    g = torch.Generator().manual_seed(7 + M)
    for k in (1, 5, 12):
        for di in (0, 2):
            k_in = 1 if di == 0 else k
            N = B * k_in
            xs = _logp_rows(M, N, V, ldl, g, case)
            nll = torch.randn(B * k, generator=g)
            if case == "ties":
                nll = nll.round()
            nll = nll.cuda()
            beam = torch.zeros(2 * ML, B, k, dtype=torch.int64)
            if di > 0:
                beam[di - 1] = torch.randint(4, V, (B, k), generator=g)
                beam[di - 1, 0, 0] = EOS                              # a finished hypothesis
                beam[di - 1, 1, :] = EOS                              # a sentence whose hypotheses have all finished
            beam = beam.cuda()
            h_in = [torch.randn(N, H, generator=g).cuda() for H in Hs]
            h_out = [torch.zeros(B * k, H, device="cuda") for H in Hs]
            n_alive = torch.zeros(1, dtype=torch.int32, device="cuda")
            scratch = torch.empty(L.lib().vag_beam_scratch_bytes(B, k, V, ML), dtype=torch.uint8, device="cuda")
            nll_in = nll.clone()
            P = lambda ts: (C.c_void_p * M)(*[ptr(t) for t in ts])      # noqa: E731
            I64 = lambda v: (C.c_int64 * M)(*v)                       # noqa: E731
            call("vag_beam_ens_step", P(xs), I64([ldl] * M), M, ptr(nll), ptr(beam, torch.int64), di, ML, P(h_in), P(h_out),
                 I64(Hs), B, k, V, ptr(n_alive, torch.int32), scratch.data_ptr(), L.stream())
            torch.cuda.synchronize()
            # restatement: the combined scores, penalties (V11.py:279-280, :291-294), the k best under (score desc, flat index asc)
            s = _ens_scores_ref([x[:, :V].cpu() for x in xs])
            if case == "ties":
                assert torch.equal(s, xs[0][:, :V].cpu())             # identical rows: s == x exactly
            if di > 0:
                prev = beam[di - 1].reshape(-1).cpu()
                s[torch.arange(N), prev] = -1e5
                fin = prev == EOS
                s[fin] = -1e5
                s[fin, EOS] = 0.0
                cand = (nll_in.cpu().reshape(-1, 1) + s).reshape(B, k_in * V)
            else:
                cand = s.reshape(B, V)
            cand = cand.numpy()
            got_nll = nll.cpu().numpy().reshape(B, k)
            for b in range(B):
                order = np.lexsort((np.arange(cand.shape[1]), -cand[b].astype(np.float64)))[:k]
                assert np.array_equal(beam[di, b].cpu().numpy(), order % V), (M, case, k, di, b)
                assert np.array_equal(beam[ML + di, b].cpu().numpy(), order // V), (M, case, k, di, b)
                if case == "ties":
                    assert np.array_equal(got_nll[b], cand[b][order]), (M, case, k, di, b)
                else:
                    assert np.allclose(got_nll[b], cand[b][order], rtol=1e-6, atol=1e-6), (M, case, k, di, b)
            par = beam[ML + di].cpu()
            rows = (par + torch.arange(B).unsqueeze(1) * k_in).reshape(-1).cuda()
            for hi, ho in zip(h_in, h_out):
                assert torch.equal(ho, hi.index_select(0, rows)), (M, case, k, di)
            assert int(n_alive.item()) == int((beam[di] != EOS).sum().item())


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("case", ["random", "ties"])
def test_ens_argmax_matches_total_order(M, case):
    import ctypes as C
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import call, ptr
    N, V = 37, 9391
    ldl = V + 1
    g = torch.Generator().manual_seed(31)
    xs = _logp_rows(M, N, V, ldl, g, case)
    if case == "ties":
        for x in xs:
            x[0, :V] = -1.0                                           # a row that ties everywhere: word 0
    out = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    call("vag_ens_argmax", (C.c_void_p * M)(*[ptr(x) for x in xs]), (C.c_int64 * M)(*[ldl] * M), M, N, V, ptr(out, torch.int64),
         L.stream())
    s = _ens_scores_ref([x[:, :V].cpu() for x in xs])
    want = torch.where(s == s.max(1, keepdim=True).values, torch.arange(V).expand_as(s), V).min(1).values
    assert torch.equal(out.cpu(), want)
    if case == "ties":
        assert int(out[0]) == 0
