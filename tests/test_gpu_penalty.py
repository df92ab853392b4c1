"""GPU: beam search with length and coverage penalties (vagnmt_hip.penalty; include/vag_nmt.h: vag_beam_cover, vag_beam_pen_step,
vag_beam_finish_pen).

1. vag_beam_cover against tests/penalty_ref.py: cov_row bit for bit on attention quantised to 1/64, cp_row against fp64;
2. vag_beam_pen_step against the reference, exactly -- words, parents, score bits, lengths, penalties, coverage rows, hidden
   states, n_alive, tok_out, di_state -- on log-probabilities quantised to 1/8 (ties everywhere) with arbitrary lengths, penalties
   and tables; stepwise = 0 against vag_beam_ens_step_opt; the device-index form;
3. a whole search on the table model of tests/test_penalty_host.py through vag_beam_finish_pen; the ABI's argument errors;
4. the models and Ensemble."""
import numpy as np
import pytest
import torch

import diverse_ref as D
import penalty_ref as R
from test_gpu_diverse import (EOS, I32, I64, L, LENS, ML, bits, dev, ints, kernel_combined, make_inputs, make_model, nbest, p64, pp,
                              quantised, stream)
from test_penalty_host import LENGTH_1, SEARCH, WORD_COST, eos_outside_row_best, table_model

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------
# the ABI by hand
# ------------------------------------------------------------------------------------------------------------------
def quantised_attention(rng, rows, Tp, top=24):
    a = (rng.integers(0, top, size=(rows, Tp)) / 64.0).astype(F32)
    a[rng.random((rows, Tp)) < 0.2] = 0.0
    return a


def run_cover(alphas, mask, cov, beam, di, max_len, B, k, Tp, beta, di_state=None):
    rows = B if di == 0 else B * k
    cov_row = torch.full((B * k, Tp), float("nan"), device="cuda")
    cp_row = torch.full((B * k,), float("nan"), device="cuda")
    if di_state is None:
        rc = L().vag_beam_cover(pp(alphas), len(alphas), mask.data_ptr(), cov.data_ptr(), beam.data_ptr(), di, max_len, B, k, Tp, beta,
                                cov_row.data_ptr(), cp_row.data_ptr(), stream())
    else:
        rc = L().vag_beam_cover_dev(pp(alphas), len(alphas), mask.data_ptr(), cov.data_ptr(), beam.data_ptr(), di_state.data_ptr(),
                                    max_len, B, k, Tp, beta, cov_row.data_ptr(), cp_row.data_ptr(), stream())
    assert rc == 0
    return cov_row.cpu().numpy(), cp_row.cpu().numpy(), rows


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 6, 64])
@pytest.mark.parametrize("Tp", [1, 3, 9, 40, 104])
def test_cover_matches_reference(Tp, k, M):
    """cov_row bit for bit; cp_row against fp64 to 1e-5 max(1, |cp|): logf is within 2 ulp plus one rounding per term, all terms
    have one sign, at most 104 additions follow: about 6.4e-6 relative."""
    rng = np.random.default_rng(1000 * Tp + 10 * k + M)
    B, max_len, beta = 2, 4, 0.375
    mask = np.ones((B, Tp), dtype=F32)
    if Tp > 1:
        mask[1, Tp - max(1, Tp // 3):] = 0.0                              # masked columns
    for di in (0, 2):
        rows = B if di == 0 else B * k
        al = [quantised_attention(rng, rows, Tp) for _ in range(M)]
        cov = (rng.integers(0, 100, size=(B, k, Tp)) / 64.0).astype(F32)   # some sums beyond 1, some exact zeros
        cov[rng.random(cov.shape) < 0.15] = 0.0
        prev = rng.integers(4, 50, size=(B, k))
        prev[rng.random((B, k)) < 0.4] = EOS                              # finished rows
        if k > 1:
            prev[0, 0], prev[0, 1] = EOS, 5
        beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
        if di:
            beam[di - 1].copy_(dev(prev))
        alphas = [dev(a) for a in al]
        ds = torch.tensor([di, 0], dtype=I32, device="cuda") if di else None
        got_row, got_cp, _ = run_cover(alphas, dev(mask), dev(cov), beam, di, max_len, B, k, Tp, beta, ds)
        want_row, want_cp = R.cover(al, np.repeat(mask, rows // B, axis=0), None if di == 0 else cov.reshape(B * k, Tp),
                                    None if di == 0 else prev.reshape(-1), beta)
        assert got_row[:rows].tobytes() == want_row.tobytes(), (Tp, k, M, di)
        err = np.abs(got_cp[:rows].astype(np.float64) - want_cp) / np.maximum(1.0, np.abs(want_cp))
        assert err.max() <= 1e-5, (Tp, k, M, di, err.max())
        assert np.isnan(got_row[rows:]).all() and np.isnan(got_cp[rows:]).all()     # nothing past the step's rows
        if di:
            fin = prev.reshape(-1) == EOS
            assert got_row[:rows][fin].tobytes() == cov.reshape(B * k, Tp)[fin].tobytes()      # a finished row is frozen
            assert ds.cpu().tolist() == [di, 0]                                               # the index is read, not advanced


def test_cover_scalar_and_vector_paths_agree_and_beta_zero_does_nothing():
    rng = np.random.default_rng(4)
    B, k, Tp, max_len, di = 2, 6, 40, 4, 1
    al = quantised_attention(rng, B * k, Tp)
    cov = (rng.integers(0, 100, size=(B, k, Tp)) / 64.0).astype(F32)
    mask = np.ones((B, Tp), dtype=F32)
    mask[0, 30:] = 0
    beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
    beam[0, 0, 2] = EOS
    row, cp, _ = run_cover([dev(al)], dev(mask), dev(cov), beam, di, max_len, B, k, Tp, 0.2)
    shifted = torch.zeros(B * k * Tp + 1, device="cuda")
    shifted[1:].copy_(dev(al).view(-1))                                   # the same rows, 4 bytes off a 16-byte boundary
    row2, cp2, _ = run_cover([shifted[1:].view(B * k, Tp)], dev(mask), dev(cov), beam, di, max_len, B, k, Tp, 0.2)
    assert row.tobytes() == row2.tobytes() and cp.tobytes() == cp2.tobytes()
    # beta = 0: cp_row is +0 and nothing else is read or written
    cp_row = torch.full((B * k,), float("nan"), device="cuda")
    assert L().vag_beam_cover(None, 1, None, None, beam.data_ptr(), di, max_len, B, k, Tp, 0.0, None, cp_row.data_ptr(), stream()) == 0
    assert cp_row.cpu().numpy().tobytes() == np.zeros(B * k, dtype=F32).tobytes()


class PenSearch:
    """The buffers of one penalised search, driven step by step through the ABI."""

    def __init__(self, B, k, V, max_len, Hs, Tp, cover=True):
        self.B, self.k, self.V, self.max_len, self.Hs, self.Tp = B, k, V, max_len, list(Hs), Tp
        self.beam = torch.zeros(2 * max_len, B, k, dtype=I64, device="cuda")
        self.nll = torch.zeros(B, k, device="cuda")
        self.n_alive = torch.full((1,), -7, dtype=I32, device="cuda")
        self.scratch = torch.empty(L().vag_beam_pen_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        self.tok = torch.full((B * k,), -1, dtype=I64, device="cuda")
        self.di_state = torch.zeros(2, dtype=I32, device="cuda")
        self.lens = torch.full((B, k), 77, dtype=I32, device="cuda")       # (step 0 ignores the contents)
        self.cpen = torch.zeros(B, k, device="cuda")
        self.cp_row = torch.zeros(B * k, device="cuda")
        self.cov = torch.zeros(B, k, Tp, device="cuda") if cover else None
        self.cov_row = torch.zeros(B * k, Tp, device="cuda") if cover else None
        self.tabs = torch.ones(2, max_len + 1, device="cuda")

    def set_tables(self, lp, bonus):
        self.tabs.copy_(dev(np.stack([lp, bonus])))

    def step(self, logps, h_ins, di, stepwise, flags=0, device_index=False):
        h_outs = [torch.full((self.B * self.k, H), float("nan"), device="cuda") for H in self.Hs]
        ldl = p64([x.shape[1] for x in logps])
        ptr = lambda t: None if t is None else t.data_ptr()             # noqa: E731
        pen = (self.lens.data_ptr(), self.cp_row.data_ptr(), self.cpen.data_ptr(), ptr(self.cov_row), ptr(self.cov), self.Tp,
               self.tabs[0].data_ptr(), self.tabs[1].data_ptr(), stepwise)
        if device_index:
            rc = L().vag_beam_pen_step_dev(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(),
                                           self.di_state.data_ptr(), self.max_len, pp(h_ins), pp(h_outs), p64(self.Hs),
                                           self.tok.data_ptr(), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                           self.scratch.data_ptr(), flags, *pen, stream())
        else:
            rc = L().vag_beam_pen_step(pp(logps), ldl, len(logps), self.nll.data_ptr(), self.beam.data_ptr(), di, self.max_len,
                                       pp(h_ins), pp(h_outs), p64(self.Hs), self.B, self.k, self.V, self.n_alive.data_ptr(),
                                       self.scratch.data_ptr(), flags, *pen, stream())
        return rc, h_outs


def random_tables(rng, max_len):
    """Arbitrary tables: any positive divisor, any reward -- the step indexes them, it does not know their formulas."""
    return (0.5 + 2.5 * rng.random(max_len + 1)).astype(F32), (2.0 * rng.random(max_len + 1) - 1.0).astype(F32)


def check_step(B, k, V, ldl, M, di, stepwise, flags, seed, Hs, Tp):
    rng = np.random.default_rng(seed)
    k_in = 1 if di == 0 else k
    rows = B * k_in
    max_len = 4
    lp = [quantised(rng, rows, V, ldl) for _ in range(M)]
    if M > 1:                                     # members that disagree, off the grid
        lp = [a + np.float32(0.01 * m) * rng.standard_normal(a.shape).astype(np.float32) for m, a in enumerate(lp)]
        for a in lp:
            a[:, V:] = 100.0
    s = PenSearch(B, k, V, max_len, Hs, Tp)
    tlp, tbonus = random_tables(rng, max_len)
    s.set_tables(tlp, tbonus)
    base = prev = lens = None
    if di > 0:
        base = (rng.integers(-400, 0, size=(B, k)) / 8.0).astype(np.float32)
        prev = rng.integers(0, V, size=(B, k))
        prev[rng.random((B, k)) < 0.3] = EOS
        prev[:, k - 1] = prev[:, 0]               # two rows with the same previous word
        lens = rng.integers(0, max_len - 1, size=(B, k)).astype(np.int32)
        s.nll.copy_(dev(base))
        s.beam[di - 1].copy_(dev(prev))
        s.lens.copy_(dev(lens))
    cp_row = (-rng.integers(0, 64, size=rows) / 16.0).astype(F32)
    cov_row = rng.random((rows, Tp)).astype(F32)
    s.cp_row[:rows].copy_(dev(cp_row))
    s.cov_row[:rows].copy_(dev(cov_row))
    h_in = [rng.standard_normal((rows, H)).astype(np.float32) for H in Hs]
    logps = [dev(a) for a in lp]
    if M == 1:
        comb = lp[0][:, :V]
    else:
        # NumPy's ens_score may differ from the device's expf / logf in the last bits: checked to a few ulp, and the selection is
        # compared exactly on the kernels' own combined values (test_gpu_diverse.kernel_combined)
        comb = kernel_combined(logps, V)
        want = D.ens_combine([a[:, :V] for a in lp])
        assert np.allclose(comb, want, rtol=2e-6, atol=2e-6), np.abs(comb - want).max()
    s.di_state.copy_(torch.tensor([di, 0], dtype=I32))
    rc, h_out = s.step(logps, [dev(h) for h in h_in], di, stepwise, flags, device_index=di > 0)
    assert rc == 0
    words, parents = s.beam[di].cpu().numpy(), s.beam[max_len + di].cpu().numpy()
    nll, got_lens, got_cpen, got_cov = s.nll.cpu().numpy(), s.lens.cpu().numpy(), s.cpen.cpu().numpy(), s.cov.cpu().numpy()
    alive = 0
    for b in range(B):
        sl = slice(b * k_in, (b + 1) * k_in)
        w, p, sc, ln, cpn, _ = R.step(comb[sl], None if di == 0 else base[b], None if di == 0 else prev[b],
                                      None if di == 0 else lens[b], cp_row[sl], k, tlp, tbonus, stepwise, di, max_len, flags)
        what = (B, k, V, M, di, stepwise, flags, b)
        assert words[b].tolist() == w.tolist(), what
        assert parents[b].tolist() == p.tolist(), what
        assert nll[b].tobytes() == sc.tobytes(), what
        assert got_lens[b].tolist() == ln.tolist(), what
        assert got_cpen[b].tobytes() == cpn.tobytes(), what
        assert got_cov[b].tobytes() == cov_row[sl][p].tobytes(), what
        for m, H in enumerate(Hs):
            got = h_out[m].cpu().numpy()[b * k:(b + 1) * k]
            assert got.tobytes() == h_in[m][b * k_in + p].tobytes(), what
        alive += int((w != EOS).sum())
    assert int(s.n_alive.item()) == alive
    if di > 0:
        assert s.tok.cpu().numpy().tolist() == words.reshape(-1).tolist()
        assert s.di_state.cpu().tolist() == [di + 1, 0]


SHAPES = [(3, 6, 50, 50), (2, 4, 2500, 2504), (1, 12, 4100, 4100), (2, 64, 70, 70), (2, 12, 10000, 10000)]


@pytest.mark.parametrize("B,k,V,ldl", SHAPES)
def test_step_matches_reference_exactly(B, k, V, ldl):
    seed = 0
    for stepwise in (0, 1):
        for flags in (0, 3):
            for di in (0, 2, 3):                  # 3 = max_len - 1: no word counts any more
                seed += 1
                check_step(B, k, V, ldl, 1, di, stepwise, flags, 1000 * V + seed, [8] if seed % 2 else [6], 8 if seed % 2 else 5)


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("B,k,V,ldl", [SHAPES[0], SHAPES[-1]])
def test_ensemble_step_matches_reference_exactly(B, k, V, ldl, M):
    for n, (stepwise, flags, di) in enumerate([(1, 0, 0), (1, 3, 1), (0, 3, 2), (1, 0, 3)]):
        check_step(B, k, V, ldl, M, di, stepwise, flags, 77 * V + 10 * M + n, [8, 6, 4][:M], 7)


def test_without_stepwise_is_the_plain_step_bit_for_bit():
    """stepwise = 0 against vag_beam_ens_step_opt on the same inputs: words, parents, score bits, hidden states, n_alive."""
    rng = np.random.default_rng(5)
    B, k, V, max_len, H, Tp = 2, 12, 4100, 4, 8, 8
    for di, flags in [(0, 0), (2, 3), (1, 0)]:
        k_in = 1 if di == 0 else k
        logp = [dev(quantised(rng, B * k_in, V, V))]
        h_in = [dev(rng.standard_normal((B * k_in, H)).astype(np.float32))]
        base = dev((rng.integers(-400, 0, size=(B, k)) / 8.0).astype(np.float32))
        prev = rng.integers(0, V, size=(B, k))
        prev[rng.random((B, k)) < 0.3] = EOS
        a = PenSearch(B, k, V, max_len, [H], Tp)
        a.set_tables(*random_tables(rng, max_len))
        a.cp_row.copy_(dev(-rng.random(B * k).astype(F32)))
        a.lens.copy_(dev(rng.integers(0, 3, size=(B, k)).astype(np.int32)))
        p = PenSearch(B, k, V, max_len, [H], Tp)
        for s in (a, p):
            s.nll.copy_(base)
            if di > 0:
                s.beam[di - 1].copy_(dev(prev))
        rc, ha = a.step(logp, h_in, di, 0, flags)
        assert rc == 0
        hp = [torch.empty(B * k, H, device="cuda")]
        scratch = torch.empty(L().vag_beam_scratch_bytes(B, k, V, max_len), dtype=torch.uint8, device="cuda")
        assert L().vag_beam_ens_step_opt(pp(logp), p64([V]), 1, p.nll.data_ptr(), p.beam.data_ptr(), di, max_len, pp(h_in), pp(hp),
                                         p64([H]), B, k, V, p.n_alive.data_ptr(), scratch.data_ptr(), flags, stream()) == 0
        assert torch.equal(a.beam, p.beam) and torch.equal(bits(a.nll), bits(p.nll)), (di, flags)
        assert torch.equal(ha[0], hp[0]) and torch.equal(a.n_alive, p.n_alive)


def test_device_index_form():
    rng = np.random.default_rng(6)
    B, k, V, max_len, H, Tp = 3, 6, 50, 3, 8, 5
    lps = [dev(quantised(rng, B * (1 if di == 0 else k), V, V)) for di in range(3)]
    cps = [dev((-rng.integers(0, 64, size=B * k) / 16.0).astype(F32)) for _ in range(3)]
    cvs = [dev(rng.random((B * k, Tp)).astype(F32)) for _ in range(3)]
    h0 = dev(rng.standard_normal((B, H)).astype(np.float32))
    a, d = PenSearch(B, k, V, max_len, [H], Tp), PenSearch(B, k, V, max_len, [H], Tp)
    tabs = random_tables(rng, max_len)

    def feed(s, di):
        s.cp_row.copy_(cps[di]); s.cov_row.copy_(cvs[di])
    for s in (a, d):
        s.set_tables(*tabs)
        feed(s, 0)
        rc, h = s.step([lps[0]], [h0], 0, 1)
        assert rc == 0
        s.h = h
    for di in (1, 2):
        feed(a, di)
        rc, a.h = a.step([lps[di]], a.h, di, 1)
        assert rc == 0
    d.di_state.copy_(torch.tensor([1, 0], dtype=I32))
    for di in (1, 2):
        feed(d, di)
        rc, d.h = d.step([lps[di]], d.h, 0, 1, device_index=True)
        assert rc == 0
    assert d.di_state.cpu().tolist() == [3, 0]
    assert torch.equal(a.beam, d.beam) and torch.equal(bits(a.nll), bits(d.nll)) and torch.equal(a.h[0], d.h[0])
    assert torch.equal(a.lens, d.lens) and torch.equal(bits(a.cpen), bits(d.cpen)) and torch.equal(bits(a.cov), bits(d.cov))
    assert torch.equal(a.n_alive, d.n_alive) and torch.equal(d.tok, d.beam[2].view(-1))
    # at di >= max_len the launches write nothing
    state = (d.beam, d.nll, d.tok, d.n_alive, d.di_state, d.lens, d.cpen, d.cov)
    d.n_alive.fill_(-3)
    before = [t.clone() for t in state]
    rc, h = d.step([lps[2]], d.h, 0, 1, device_index=True)
    assert rc == 0
    for t, b in zip(state, before):
        assert torch.equal(t, b)
    assert bool(torch.isnan(h[0]).all())
    crow, cprow = torch.full((B * k, Tp), float("nan"), device="cuda"), torch.full((B * k,), float("nan"), device="cuda")
    assert L().vag_beam_cover_dev(pp([cvs[0]]), 1, torch.ones(B, Tp, device="cuda").data_ptr(), d.cov.data_ptr(), d.beam.data_ptr(),
                                  d.di_state.data_ptr(), max_len, B, k, Tp, 0.5, crow.data_ptr(), cprow.data_ptr(), stream()) == 0
    assert bool(torch.isnan(crow).all()) and bool(torch.isnan(cprow).all())


def device_search(T, A, mask, lp, bonus, beta, stepwise):
    """Three launches per step on the table model; returns the search and every step's (cov_row, cp_row) as the device wrote them."""
    B, k, V, max_len, steps = (SEARCH[n] for n in ("B", "k", "V", "max_len", "steps"))
    Tp, H = mask.shape[1], 4
    Td, Ad, md = dev(T), dev(A), dev(mask)
    s = PenSearch(B, k, V, max_len, [H], Tp, cover=beta > 0)
    s.set_tables(lp, bonus)
    h = [torch.zeros(B, H, device="cuda")]
    rows_seen, cps_seen = [], []
    for di in range(steps):
        tok = torch.full((B,), D.SOS, dtype=I64, device="cuda") if di == 0 else s.beam[di - 1].reshape(-1)
        if beta > 0:
            assert L().vag_beam_cover(pp([Ad[tok].contiguous()]), 1, md.data_ptr(), s.cov.data_ptr(), s.beam.data_ptr(), di, max_len,
                                      B, k, Tp, beta, s.cov_row.data_ptr(), s.cp_row.data_ptr(), stream()) == 0
            n = tok.shape[0]
            rows_seen.append(s.cov_row[:n].cpu().numpy()); cps_seen.append(s.cp_row[:n].cpu().numpy())
        else:
            cps_seen.append(np.zeros(tok.shape[0], dtype=F32))
        rc, h = s.step([Td[tok].contiguous()], h, di, int(stepwise))
        assert rc == 0
    return s, rows_seen, cps_seen


def finish_pen(s, steps, n):
    B, k, ml = s.B, s.k, s.max_len
    out = torch.empty(B, n, ml, dtype=I64, device="cuda")
    sc, logp, cp = (torch.empty(B, n, device="cuda") for _ in range(3))
    slots, length = torch.empty(B, n, dtype=I64, device="cuda"), torch.empty(B, n, dtype=I32, device="cuda")
    assert L().vag_beam_finish_pen(s.nll.data_ptr(), s.beam.data_ptr(), s.lens.data_ptr(), s.cpen.data_ptr(), s.tabs[0].data_ptr(),
                                   s.tabs[1].data_ptr(), ml, steps, B, k, n, out.data_ptr(), sc.data_ptr(), slots.data_ptr(),
                                   logp.data_ptr(), length.data_ptr(), cp.data_ptr(), stream()) == 0
    return dict(out=out.cpu().numpy(), scores=sc.cpu().numpy(), slots=slots.cpu().numpy(), logp=logp.cpu().numpy(),
                length=length.cpu().numpy(), cp=cp.cpu().numpy())


@pytest.mark.parametrize("cfg", [LENGTH_1, WORD_COST], ids=["length1", "wordcost"])
@pytest.mark.parametrize("stepwise", [False, True])
def test_whole_search_on_a_table_model(cfg, stepwise):
    """The table model of tests/test_penalty_host.py (which asserts that these settings separate stepwise from final selection
    and select an EOS child outside its row's k best by c).  The reference is fed the device's own cp_row values -- NumPy cannot
    restate logf bit for bit -- after they were checked against fp64; everything else is exact."""
    T, A, mask = table_model()
    norm, alpha, beta, wb = cfg
    k, ml, steps, B = SEARCH["k"], SEARCH["max_len"], SEARCH["steps"], SEARCH["B"]
    lp, bonus = R.tables(ml, norm, alpha, wb)
    s, rows_seen, cps_seen = device_search(T, A, mask, lp, bonus, beta, stepwise)
    trace = []
    want = R.search(lambda tok: T[tok], lambda tok: A[tok], mask, lp=lp, bonus=bonus, beta=beta, stepwise=stepwise, cp_rows=cps_seen,
                    trace=trace, **SEARCH)
    for di in range(steps):
        assert rows_seen[di].tobytes() == want["cov_rows"][di].tobytes(), di
        rows = np.minimum(np.maximum(rows_seen[di], R.COV_FLOOR), F32(1.0)).astype(np.float64)
        cp64 = beta * np.where(np.repeat(mask, 1 if di == 0 else k, axis=0) != 0, np.log(rows), 0.0).sum(axis=1)
        assert (np.abs(cps_seen[di] - cp64) <= 1e-5 * np.maximum(1.0, np.abs(cp64))).all(), di
    assert np.array_equal(s.beam.cpu().numpy(), want["beam"]) and s.nll.cpu().numpy().tobytes() == want["nll"].tobytes()
    assert np.array_equal(s.lens.cpu().numpy(), want["lens"]) and s.cpen.cpu().numpy().tobytes() == want["cpen"].tobytes()
    assert s.cov.cpu().numpy().tobytes() == want["cov"].tobytes()
    if stepwise and cfg is WORD_COST:
        assert eos_outside_row_best(trace, k)                             # the device selected such a child too (same history)
    got = finish_pen(s, steps, k)
    fin = R.finish(want["beam"], want["nll"], want["lens"], want["cpen"], lp, bonus, ml, steps, k)
    assert np.array_equal(got["out"], fin["out"]) and np.array_equal(got["slots"], fin["slots"])
    for name in ("scores", "logp", "cp"):
        assert got[name].tobytes() == fin[name].tobytes(), name
    assert np.array_equal(got["length"], fin["length"])
    for b in range(B):                                                    # the carried lengths are what the finish's walk counts
        for j in range(k):
            assert want["lens"][b, j] == R.walk_length(want["beam"], ml, steps, b, j)


def test_plain_tables_are_the_plain_search_and_finish():
    """"length" / 1 / 0 / 0: history, out and scores are vag_beam_ens_step_opt's and vag_beam_finish_nbest's bit for bit."""
    T, A, mask = table_model()
    k, ml, steps, B, V = SEARCH["k"], SEARCH["max_len"], SEARCH["steps"], SEARCH["B"], SEARCH["V"]
    lp, bonus = R.tables(ml, "length", 1.0, 0.0)
    s, _, _ = device_search(T, A, mask, lp, bonus, 0.0, True)           # (stepwise on plain tables: length-normalised selection)
    p, _, _ = device_search(T, A, mask, lp, bonus, 0.0, False)
    beam, nll = D.search(lambda tok: T[tok], B, k, 1, 0.0, V, ml, steps)
    assert np.array_equal(p.beam.cpu().numpy(), beam) and p.nll.cpu().numpy().tobytes() == nll.tobytes()
    assert not np.array_equal(s.beam.cpu().numpy(), beam)
    got = finish_pen(p, steps, k)
    out, sc = torch.empty(B, k, ml, dtype=I64, device="cuda"), torch.empty(B, k, device="cuda")
    assert L().vag_beam_finish_nbest(p.nll.data_ptr(), p.beam.data_ptr(), ml, steps, B, k, k, out.data_ptr(), sc.data_ptr(),
                                     stream()) == 0
    assert np.array_equal(got["out"], out.cpu().numpy()) and got["scores"].tobytes() == sc.cpu().numpy().tobytes()
    assert got["cp"].tobytes() == np.zeros((B, k), dtype=F32).tobytes()


def test_abi_argument_errors_launch_nothing():
    B, k, V, max_len, H, Tp = 2, 6, 50, 4, 8, 8
    s = PenSearch(B, k, V, max_len, [H], Tp)
    logp = [torch.zeros(B, V, device="cuda")]
    h = [torch.zeros(B, H, device="cuda")]
    NULL = object()

    def call(k_=k, V_=V, flags=0, M=1, di=0, Tp_=Tp, stepwise=1, dev_form=False, state=True, **null):
        ho = [torch.full((B * 64, H), float("nan"), device="cuda")]
        g = lambda name, t: None if null.get(name) is NULL else t.data_ptr()          # noqa: E731
        pen = (g("lens", s.lens), g("cp_row", s.cp_row), g("cpen", s.cpen), g("cov_row", s.cov_row), g("cov", s.cov), Tp_,
               g("lp", s.tabs[0]), g("bonus", s.tabs[1]), stepwise)
        if dev_form:
            rc = L().vag_beam_pen_step_dev(pp(logp), p64([V]), M, g("nll", s.nll), s.beam.data_ptr(),
                                           s.di_state.data_ptr() if state else None, max_len, pp(h), pp(ho), p64([H]),
                                           s.tok.data_ptr(), B, k_, V_, s.n_alive.data_ptr(), s.scratch.data_ptr(), flags, *pen, stream())
        else:
            rc = L().vag_beam_pen_step(pp(logp), p64([V]), M, g("nll", s.nll), s.beam.data_ptr(), di, max_len, pp(h), pp(ho),
                                       p64([H]), B, k_, V_, s.n_alive.data_ptr(), s.scratch.data_ptr(), flags, *pen, stream())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(ho[0]).all())
    bad = [dict(V_=5), dict(flags=4), dict(M=0), dict(M=9), dict(k_=65), dict(k_=0), dict(di=-1), dict(di=max_len), dict(nll=NULL),
           dict(dev_form=True, state=False), dict(Tp_=0), dict(stepwise=2), dict(stepwise=-1), dict(lens=NULL), dict(cp_row=NULL),
           dict(cpen=NULL), dict(lp=NULL), dict(bonus=NULL), dict(cov=NULL), dict(cov_row=NULL)]
    for kw in bad:
        assert call(**kw) == (-22, True), kw
    assert int(s.n_alive.item()) == -7 and not bool(s.beam.any()) and not bool(s.nll.any())
    assert bool((s.lens == 77).all()) and not bool(s.cpen.any()) and not bool(s.cov.any())
    # the coverage launch
    al = [torch.zeros(B * k, Tp, device="cuda")]
    mask = torch.ones(B, Tp, device="cuda")
    crow, cprow = torch.full((B * k, Tp), float("nan"), device="cuda"), torch.full((B * k,), float("nan"), device="cuda")

    def cover(beta=0.2, k_=k, Tp_=Tp, M=1, di=0, alpha=True, **null):
        g = lambda name, t: None if null.get(name) is NULL else t.data_ptr()          # noqa: E731
        rc = L().vag_beam_cover(pp(al) if alpha else None, M, g("mask", mask), g("cov", s.cov), g("beam", s.beam), di, max_len, B, k_,
                                Tp_, beta, g("cov_row", crow), g("cp_row", cprow), stream())
        torch.cuda.synchronize()
        return rc
    for kw in [dict(beta=-0.1), dict(beta=float("nan")), dict(beta=float("inf")), dict(k_=65), dict(Tp_=0), dict(M=0), dict(M=9),
               dict(di=-1), dict(di=max_len), dict(alpha=False), dict(mask=NULL), dict(cov=NULL), dict(beam=NULL), dict(cov_row=NULL),
               dict(cp_row=NULL)]:
        assert cover(**kw) == -22, kw
    assert bool(torch.isnan(crow).all()) and bool(torch.isnan(cprow).all())
    assert L().vag_beam_cover_dev(pp(al), 1, mask.data_ptr(), s.cov.data_ptr(), s.beam.data_ptr(), None, max_len, B, k, Tp, 0.2,
                                  crow.data_ptr(), cprow.data_ptr(), stream()) == -22
    # the finish
    out = torch.zeros(B, k, max_len, dtype=I64, device="cuda")
    f = [torch.zeros(B, k, device="cuda") for _ in range(3)]
    sl, ln = torch.zeros(B, k, dtype=I64, device="cuda"), torch.zeros(B, k, dtype=I32, device="cuda")

    def finish(n=k, k_=k, steps=2, **null):
        g = lambda name, t: None if null.get(name) is NULL else t.data_ptr()          # noqa: E731
        rc = L().vag_beam_finish_pen(g("nll", s.nll), s.beam.data_ptr(), g("lens", s.lens), g("cpen", s.cpen), g("lp", s.tabs[0]),
                                     g("bonus", s.tabs[1]), max_len, steps, B, k_, n, g("out", out), g("scores", f[0]),
                                     g("slots", sl), g("logp", f[1]), g("length", ln), g("cp", f[2]), stream())
        torch.cuda.synchronize()
        return rc
    for kw in [dict(n=k + 1), dict(n=0), dict(k_=65), dict(steps=0), dict(steps=max_len + 1)] + \
            [{name: NULL} for name in ("nll", "lens", "cpen", "lp", "bonus", "out", "scores", "slots", "logp", "length", "cp")]:
        assert finish(**kw) == -22, kw
    assert not bool(out.any()) and not any(bool(t.any()) for t in f) and not bool(sl.any()) and not bool(ln.any())
    assert L().vag_beam_pen_scratch_bytes(16, 12, 9391, 80) >= 16 * 12 * 5 * 12 * 12
    assert L().vag_beam_pen_scratch_bytes(16, 65, 9391, 80) == -22 and L().vag_beam_pen_scratch_bytes(16, 12, 5, 80) == -22
    assert call() == (0, False) and cover() == 0 and finish() == 0          # and the good calls go through


# ------------------------------------------------------------------------------------------------------------------
# models (small random ones, as tests/test_gpu_diverse.py builds them: VS 70, VT 503, H 64, lens [9, 6, 3], ML 10)
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["mm", "text"])
def subject(request):
    m = make_model(request.param, 21, eos_bias=2.0)
    src, im = make_inputs()
    return request.param, m, src, (im if request.param == "mm" else None)


def pen(m, src, im, lens=LENS, **kw):
    kw.setdefault("max_length", ML)
    return m.beamsearch_penalised(src, lens, im, **kw)


def aligned(m, src, im, k, n, lens=LENS):
    return m.beamsearch_align(src, lens, im, k, n, ML) if im is not None else m.beamsearch_align(src, lens, k, n, ML)


def recomputed(p, norm, alpha, wb):
    from vagnmt_hip import penalty
    lp, bonus = penalty.tables(ML, norm, alpha, wb)
    return R.score(p.logp.cpu().numpy(), p.length.cpu().numpy(), p.coverage_penalty.cpu().numpy(), lp, bonus)


def test_plain_settings_are_beamsearch_nbest(subject):
    _, m, src, im = subject
    for graph in (True, False):
        m.decode_graph = graph
        for k, n in [(6, 6), (12, 5)]:
            hyps, sc = nbest(m, src, im, k, n)
            p = pen(m, src, im, beam_size=k, n_best=n, length_norm="length", alpha=1, beta=0, word_bonus=0, stepwise=False)
            assert ints(p.hyps) == ints(hyps) and torch.equal(bits(p.scores), bits(sc)), (graph, k)
            assert p.length.dtype == I32 and p.scores.shape == p.logp.shape == p.length.shape == p.coverage_penalty.shape == (3, n)
            assert bits(p.coverage_penalty).tolist() == [[0] * n] * 3
    m.decode_graph = True


def test_final_penalties_rerank_the_nbest_list(subject):
    """stepwise=False at n_best = k: the same (tokens, logp bits) as beamsearch_nbest(k, k), re-ordered; scores are the fp32
    recomputation from the returned parts bit for bit; length is the count of words above 3; the coverage penalty is what
    penalised_score gives on beamsearch_align's attention of the same hypotheses (relative 2e-4, two fp32 evaluations of the same
    sums: every hypothesis is compared)."""
    from vagnmt_hip import penalty
    _, m, src, im = subject
    k = 6
    mask = (src != 0).float()
    for graph in (True, False):
        m.decode_graph = graph
        p = pen(m, src, im, beam_size=k, n_best=k, alpha=0.6, beta=0.2)
        al = aligned(m, src, im, k, k)
        plain = (p.logp.cpu().numpy() / np.maximum(p.length.cpu().numpy(), 1).astype(F32)).astype(F32)
        asc = al.scores.cpu().numpy()
        got = sorted((tuple(h), int(s.view(np.int32))) for b in range(3) for h, s in zip(p.hyps[b], plain[b]))
        want = sorted((tuple(h), int(s.view(np.int32))) for b in range(3) for h, s in zip(al.hyps[b], asc[b]))
        assert got == want, graph
        assert recomputed(p, "gnmt", 0.6, 0.0).tobytes() == p.scores.cpu().numpy().tobytes()
        sc = p.scores.cpu()
        assert bool((sc[:, 1:] <= sc[:, :-1]).all())
        assert p.length.cpu().tolist() == [[sum(t > 3 for t in h) for h in hs] for hs in p.hyps]
        # the attention of the same hypotheses, looked up by (tokens, plain score bits)
        rows = {(b, tuple(h), int(s.view(np.int32))): r for b in range(3) for r, (h, s) in enumerate(zip(al.hyps[b], asc[b]))}
        order = torch.tensor([[rows[(b, tuple(h), int(s.view(np.int32)))] for h, s in zip(p.hyps[b], plain[b])] for b in range(3)])
        att = al.attention.cpu()[torch.arange(3)[:, None], order]
        ref = penalty.penalised_score(p.logp.cpu(), p.length.cpu(), att, mask.cpu(), "gnmt", 0.6, 0.2, 0.0, ML)
        cp, want_cp = p.coverage_penalty.cpu().numpy(), ref.coverage_penalty.numpy()
        rel = (np.abs(cp - want_cp) / np.maximum(1.0, np.abs(want_cp))).max()
        print("coverage penalty vs penalised_score on beamsearch_align's attention: max rel err %.3e" % rel)
        assert rel <= 2e-4 and (cp < 0).any()
        rel = (np.abs(sc.numpy() - ref.score.numpy()) / np.maximum(1.0, np.abs(ref.score.numpy()))).max()
        assert rel <= 2e-4
    m.decode_graph = True


def test_logp_is_the_forced_logp(subject):
    """logp agrees with score_translations to relative 2e-4 on hypotheses that ended before max_length without a -1e5 step; the
    EOS-bias ladder of test_gpu_diverse.test_scores_are_forced_scores, six sentences, at least 8 such hypotheses."""
    kind, _, _, _ = subject
    m = make_model(kind, 23)
    lens = [9, 8, 6, 5, 3, 2]
    src, im = make_inputs(lens, seed=11)
    im = im if kind == "mm" else None
    k, B = 6, len(lens)
    idx = []
    for extra in (0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0):
        with torch.no_grad():
            m.decoder.out.bias[EOS] += extra
        p = pen(m, src, im, lens, beam_size=k, n_best=k, stepwise=True)
        lg = p.logp.cpu().numpy()
        idx = [(b, r) for b in range(B) for r in range(k) if len(p.hyps[b][r]) < ML - 1 and lg[b, r] > -1e4]
        if len(idx) >= 8:
            break
    assert len(idx) >= 8, len(idx)
    flat = [list(p.hyps[b][r]) for b in range(B) for r in range(k)]
    src_n = src.repeat_interleave(k, 0)
    lens_n = [n for n in lens for _ in range(k)]
    forced = m.score_translations(src_n, lens_n, flat, im.repeat_interleave(k, 0)) if kind == "mm" else \
        m.score_translations(src_n, lens_n, flat)
    f = forced.logp.cpu().numpy().reshape(B, k)
    rel = max(abs(float(f[b, r]) - float(lg[b, r])) / max(1.0, abs(float(lg[b, r]))) for b, r in idx)
    print("%d finished hypotheses, forced vs search logp: max rel err %.3e" % (len(idx), rel))
    assert rel <= 2e-4, rel


def test_graph_and_eager_agree_and_the_cache_keeps_settings_apart(subject):
    kind, m, src, im = subject
    res = {}
    settings = [(0.2, False, 0.6, 0.0), (0.2, True, 0.6, 0.0), (0.5, True, 0.6, 0.0), (0.2, True, 1.0, 0.3), (0.0, True, 0.6, 0.0),
                (0.2, True, 0.6, 0.0)]
    for graph in (True, False):
        m.decode_graph = graph
        for beta, stepwise, alpha, wb in settings:     # a graph captured for one (beta, stepwise) is not another's
            kw = dict(beam_size=6, n_best=6, alpha=alpha, beta=beta, word_bonus=wb, stepwise=stepwise)
            p = pen(m, src, im, **kw)
            fresh = make_model(kind, 21, eos_bias=2.0)                     # the same weights, nothing cached
            fresh.decode_graph = graph
            f = pen(fresh, src, im, **kw)
            assert ints(p.hyps) == ints(f.hyps), (graph, kw)
            for a, b in zip(p[1:], f[1:]):
                assert torch.equal(bits(a), bits(b)), (graph, kw)
            assert recomputed(p, "gnmt", alpha, wb).tobytes() == p.scores.cpu().numpy().tobytes()
            res.setdefault((beta, stepwise, alpha, wb), []).append(p)
    # one entry per (beta, stepwise) at this shape; alpha and word_bonus share an entry
    keys = [key for key in m._decode_cache if isinstance(key, tuple) and key[0] == "beam_pen" and key[2] == 6 and "constrain" not in key]
    pens = [key[key.index("penalty") + 1:key.index("penalty") + 3] for key in keys]
    f32 = lambda x: float(np.float32(x))                                  # noqa: E731
    assert len(pens) == len(set(pens)) and {(f32(0.2), False), (f32(0.2), True), (f32(0.5), True), (0.0, True)} <= set(pens)
    for key, ps in res.items():
        g, e = ps[0], ps[-1]
        rel = ((g.scores - e.scores).abs() / e.scores.abs().clamp(min=1.0)).max().item()
        print("graph vs eager", key, "max rel score diff %.3e" % rel)
        assert ints(g.hyps) == ints(e.hyps) and torch.equal(g.length, e.length) and rel <= 2e-4, key
    m.decode_graph = True


def test_ensemble_of_twins_is_the_model(subject):
    from vagnmt_hip.ensemble import Ensemble
    _, m, src, im = subject
    ens = Ensemble([m, m])
    for graph in (True, False):
        m.decode_graph = ens.decode_graph = graph
        for stepwise in (False, True):
            kw = dict(beam_size=6, n_best=4, alpha=0.6, beta=0.2, stepwise=stepwise)
            p, e = pen(m, src, im, **kw), pen(ens, src, im, **kw)
            assert ints(p.hyps) == ints(e.hyps)
            for a, b in zip(p[1:], e[1:]):
                assert torch.equal(bits(a), bits(b)), (graph, stepwise)
    m.decode_graph = True


def test_no_repeat_ngram(subject):
    _, m, src, im = subject
    for graph in (True, False):
        m.decode_graph = graph
        p = pen(m, src, im, beam_size=6, n_best=6, stepwise=True, no_repeat_ngram=2)
        for hs, sc in zip(p.hyps, p.logp.cpu().tolist()):
            for h, s in zip(hs, sc):
                grams = list(zip(h, h[1:]))
                assert s <= -1e4 or len(grams) == len(set(grams)), h
    m.decode_graph = True
    with pytest.raises(ValueError, match="beamsearch_penalised"):
        pen(m, src, im, no_repeat_ngram=9)
    with pytest.raises(ValueError, match="beamsearch_penalised"):
        pen(m, src, im, length_norm="wu")


def test_stepwise_changes_a_best_hypothesis(subject):
    """stepwise=True, length_norm="length", alpha=1 against stepwise=False on this model, eos_bias 2.0 (the fixture's value: with it
    beamsearch_nbest's best hypotheses are visibly short -- the empty translation for two or three of the three sentences): at
    least one sentence's best hypothesis changes.  beta stays at the method's default 0.2: the empty hypothesis has L = max(0, 1)
    = 1, so no length normalisation alone can make it lose to anything -- its coverage penalty is what does, and selecting by
    the penalised score at every step is what keeps the long hypotheses in the beam until then."""
    _, m, src, im = subject
    kw = dict(beam_size=6, n_best=1, length_norm="length", alpha=1.0)
    on, off = pen(m, src, im, stepwise=True, **kw), pen(m, src, im, stepwise=False, **kw)
    print("best lengths, final:", [len(h[0]) for h in off.hyps], "stepwise:", [len(h[0]) for h in on.hyps])
    assert any(a[0] != b[0] for a, b in zip(on.hyps, off.hyps))
