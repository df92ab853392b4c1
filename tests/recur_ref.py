"""Float64 references WITH THEIR OWN ERROR BOUND for the recurrences -- the bi-GRU encoder, the conditional-GRU decoder with Bahdanau
attention, and the cell / step / attention operators they are made of -- written from the definitions in include/vag_nmt.h and the
reference lines it cites (layers/Encoder.py:36-66, layers/NMT_Decoder.py:27-51, 109-131), in the manner of tests/ground_ref.py:

    vag_gru_cell_fwd / _bwd           "gi (M,3H) = W_ih x + b_ih (already projected); computes W_hh h_prev + b_hh, the gates and the
                                       blend ... save: NULL or [4][M][H] (r,z,n,hn)";  "dh = dgh_next W_hh + carry + d_out ... dgi, dgh =
                                       cell backward of THIS step ... carry_out (M,H) = z * dh".  Gate order r, z, n (torch):
                                       r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r (W_hn h + b_hn)),
                                       h' = (1 - z) n + z h.
    vag_bigru_seq_fwd / _bwd          "Writes enc (B,Ts,2H) (forward direction in [:H], reverse in [H:], zeros past each row's length)
                                       and mask (B,Ts) = (src != 0).  p_emb / p_ctx: dropout on the embedded input / on the output";
                                       packed-sequence semantics (Encoder.py:55-60): the state of row b is frozen on steps t >= len[b],
                                       so the reverse direction of a short row starts from zero at t = len[b] - 1.
                                      "d_enc (B,Ts,2H) is consumed (overwritten).  Accumulates g_emb (Vs,E; pad row untouched) and both GRUs."
    vag_cgru_attn_decode_seq_fwd/_bwd teacher-forced, per step (NMT_Decoder.py:118-129): e_t = emb[tok_t]; h1 = gru_1(e_t, h2_{t-1});
                                       q = attn_h h1; alpha = softmax_s(v . tanh(pe_s + q)) over unmasked positions; c = alpha . enc;
                                       h2 = gru_2(W_c2h c, h1).  "Outputs for the head: h2_all (Tt,B,H), c_all (Tt,B,C), e_all (Tt,B,E)."
                                      "Inputs: gradients w.r.t. the three outputs (d_h2_all, d_c_all are consumed; d_e_all may be NULL).
                                       Writes d_enc_out (B,Ts,C) (accumulate_enc: adds), d_pe (B,Ts,C), d_h0 (B,H); accumulates the parameter
                                       gradients in g (g.emb: pad row untouched)."
    vag_cgru_attn_decode_step         "Hypothesis n attends over source sentence n / rows_per_src ... h_in (N,H) -> h_out (N,H), c (N,C),
                                       e (N,E)" (+ alpha (N,Ts)).
    vag_bahdanau_attn_fwd             "alpha[n,:] = softmax_s(v . tanh(pe[n/rows_per_src,s] + q[n])) with masked positions at -inf;
                                       ctx = alpha . enc."

Every operator is written ONCE over an arithmetic `A` (ground_ref's docstring): A = T, tracked (value, err) pairs, |fp32 result - value|
<= err for any fp32 evaluation of the formula; A = F, the fp32 restatement.  T and F extend ground_ref's Tr and F32 without changing
a rule of theirs that ground_ref's operators use; `ein` is the same rule evaluated through BLAS.  The additions, u = 2^-24:

  sigmoid   common.h: vag_sigmoid = rcp(1 + __expf(-x)).  With E = exp(-x) and s = 1 / (1 + E): ground_ref's exp rule gives E a relative
            error of d + (|x| + 2) 2^-23 for an argument error d; the sum 1 + E rounds once (ULP (1 + E) allows the fused form), the
            reciprocal is RCP_REL.  ds/dE = -s^2 and s^2 E = s (1 - s), so
                err = e sup sigma' + s (1 - s) (|x| + 2) 2^-23 + s (ULP + RCP_REL),
            the first term the argument's own error e through sigma' = s (1 - s), taken at the point of the interval [x - e, x + e]
            nearest 0, where sigma' is largest (mean-value theorem); |x| in the second term at the far end of the interval.  At x = 0
            this is e / 4 + 2^-24 + 1.5 * 2^-23: a little under 2^-21.
  tanh      ground_ref's rule is err_a + TANH_ABS with |tanh'| <= 1.  A recurrence applies it once per step to a state that the next
            step's product widens by ~sqrt(H) / 2, so the slope matters here: err = e sup (1 - tanh^2) + TANH_ABS, the supremum over
            [x - e, x + e] at the point nearest 0 (mean-value theorem again: never larger than ground_ref's rule, equal to it at 0).
  range caps
            a sigmoid and a softmax weight lie in [0, 1] and a tanh in [-1, 1] whatever their argument -- the device's rcp forms pass
            the ends by a few ulp at most -- so their errors are capped at 1 + 2^-20 and twice that.  Without the caps the bound of a
            late step overflows (exp of a score whose own bound has grown past 700); with them it is merely uninformative there, and
            the elements of the early steps keep their sharp bounds: every bound is per element.
  two associations of one product
            vag_cgru_attn_decode_seq_fwd documents "the teacher-forced sequence operators apply context2hid and gru_2.w_ih to the keys
            one after the other": encwp = (enc W_c2h^T) W_ih2^T, gi2 = sum_s alpha_s encwp_s + b_ih2 -- three tracked contractions in that
            order.  vag_cgru_attn_decode_step documents "gru_2.w_ih . context2hid folded: decoding steps ... read it": Wp = W_ih2 W_c2h,
            gi2 = Wp (sum_s alpha_s enc_s) + b_ih2 -- three contractions in THAT order.  The value is the definition's
            W_ih2 (W_c2h c) + b_ih2 either way (float64 makes the difference 1e-16); the error is the documented association's.
            The backward of the sequence operator goes the same way round: du = dgi2 W_ih2, d_uk = sum_t alpha_t du_t, d_enc += d_uk W_c2h,
            and d alpha takes gru_2's share as encwp . dgi2.
  mark      the one-launch decoder stores h1 and h2 with the lowest significand bit forced to 1 (persist.hip, tag1: the bit is how a
            consumer tells a written word from an unwritten one).  |x| 2^-23 is the weight of that bit at most, so `mark` adds exactly
            ULP |h| at each such store -- h1 and h2 of every step of vag_cgru_attn_decode_seq_fwd, h2_all included -- and changes no value.
            F.mark sets the bit.  The encoder, the cells, the decoding step and the stand-alone attention do not mark and are not given
            the budget.  (The launch chain of the same operator does not mark either; it is held to the same bound, one ulp looser than
            it needs.)
  scores    e_s = v . tanh(pe_s + q) is summed over shards of C with atomics in free order: C terms of one size and of mixed sign,
            the kind ground_ref's EPS convention describes -- `ein` under EPS, no worst_case anywhere in this module.
  scatter   g_emb rows are sums of atomics in free order of known length k: gamma_k (|g0| + sum|terms|) as in ground_ref.embed_bwd_ref.

Backward inputs: what the backward reads from its private workspace (gates, h1, alpha, q and W_hh2 h1 + b, the input projections) is
recomputed here and carries its tracked error; the arguments h2_all, c_all and e_all are the fp32 arrays the forward under test produced
and enter exactly (h2_all also as the previous state the recomputation of each step starts from).
Dropout: multipliers 0 or 1 / (1 - p) from vag_dropout_mask (`which` 1: (Ts,B,E) time-major, 2: (B,Ts,2H)); exact data here.
drop_mask() restates common.h's counter-based generator on the host so that the host test has the same masks; the device test asserts
that vag_dropout_mask gives the same words.

The case tables of tests/test_gpu_recurrences.py, the input generators and the defect catalogue live here, so that
tests/test_recur_ref_host.py checks the bounds at exactly the shapes and inputs the device is tested at."""
import collections
import functools

import numpy as np

from ground_ref import TV, Tr, F32, ratio, gamma, U24, ULP, EPS, TANH_ABS, RCP_REL, _rs, _f32   # noqa: F401 (re-exported)


# ---------------------------------------------------------------------------------------------------------------- the two arithmetics
UNIT_CAP = 1.0 + 2.0 ** -20        # (module docstring: range caps)


class T(Tr):
    """ground_ref.Tr with sigmoid, the slope-aware tanh, mark and a few shape helpers (module docstring)."""

    @staticmethod
    def ein(spec, a, b, worst_case=False):
        assert not worst_case                                               # (module docstring: scores)
        a, b = Tr.lift(a), Tr.lift(b)
        av, bv = np.abs(a.v), np.abs(b.v)
        es = lambda x, y: np.einsum(spec, x, y, optimize=True)
        e = EPS * es(av, bv)
        if a.e.any():
            e = e + es(a.e, bv)
        if b.e.any():
            e = e + es(av, b.e)
        if a.e.any() and b.e.any():
            e = e + es(a.e, b.e)
        return TV(es(a.v, b.v), e)

    @staticmethod
    def sigmoid(a):
        a = Tr.lift(a)
        sg = lambda x: 1.0 / (1.0 + np.exp(-x))
        s = sg(a.v)
        near = sg(np.maximum(np.abs(a.v) - a.e, 0.0))
        e = a.e * near * (1.0 - near) + s * (1.0 - s) * (np.abs(a.v) + a.e + 2.0) * 2.0 ** -23 + s * (ULP + RCP_REL)
        return TV(s, np.minimum(e, UNIT_CAP))

    @staticmethod
    def tanh(a):
        a = Tr.lift(a)
        near = np.tanh(np.maximum(np.abs(a.v) - a.e, 0.0))
        return TV(np.tanh(a.v), np.minimum(a.e * (1.0 - near * near) + TANH_ABS, 2.0 * UNIT_CAP))

    @staticmethod
    def softmax(x, mask):
        with np.errstate(over="ignore", invalid="ignore"):
            r = Tr.softmax(x, mask)
        on = np.asarray(mask) != 0
        return TV(r.v, np.where(on, np.minimum(np.where(np.isnan(r.e), np.inf, r.e), UNIT_CAP), 0.0))

    @staticmethod
    def mark(a):
        a = Tr.lift(a)
        return TV(a.v, a.e + ULP * np.abs(a.v))

    @staticmethod
    def cat(xs, axis):
        xs = [Tr.lift(x) for x in xs]
        return TV(np.concatenate([x.v for x in xs], axis), np.concatenate([x.e for x in xs], axis))

    @staticmethod
    def stack(xs, axis):
        xs = [Tr.lift(x) for x in xs]
        return TV(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))

    @staticmethod
    def scatter_rows(g0, idx, rows, skip0=True):
        """g0 (V,E) + rows (n,E) added at idx (n), index 0 skipped: atomics in free order (module docstring: scatter)."""
        rows = Tr.lift(rows)
        v = np.asarray(g0, dtype=np.float64).copy()
        mag, e, k = np.abs(v), np.zeros_like(v), np.zeros(v.shape[0])
        keep = (idx != 0) if skip0 else np.ones(len(idx), bool)
        np.add.at(v, idx[keep], rows.v[keep])
        np.add.at(mag, idx[keep], np.abs(rows.v[keep]))
        np.add.at(e, idx[keep], rows.e[keep])
        np.add.at(k, idx[keep], 1.0)
        return TV(v, e + gamma(k)[:, None] * mag)


class F(F32):
    """ground_ref.F32 with the same additions; products through BLAS in fp32 (one more fp32 summation order)."""

    @staticmethod
    def ein(spec, a, b):
        return np.einsum(spec, F32.lift(a), F32.lift(b), optimize=True).astype(np.float32)

    @staticmethod
    def sigmoid(a):
        with np.errstate(over="ignore"):
            return (np.float32(1.0) / (np.float32(1.0) + np.exp(-F32.lift(a), dtype=np.float32))).astype(np.float32)

    @staticmethod
    def mark(a):
        return (np.ascontiguousarray(F32.lift(a)).view(np.uint32) | np.uint32(1)).view(np.float32)

    @staticmethod
    def cat(xs, axis):
        return np.concatenate([F32.lift(x) for x in xs], axis)

    @staticmethod
    def stack(xs, axis):
        return np.stack([F32.lift(x) for x in xs], axis)

    @staticmethod
    def scatter_rows(g0, idx, rows, skip0=True):
        g = np.array(g0, dtype=np.float32)
        keep = (idx != 0) if skip0 else np.ones(len(idx), bool)
        np.add.at(g, idx[keep], F32.lift(rows)[keep])
        return g


def _one(x):
    return np.ones(np.shape(x.v if isinstance(x, TV) else x))


def _zeros(A, shape):
    return A.lift(np.zeros(shape))


# ---------------------------------------------------------------------------------------------------------------- dropout words
def _mix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def drop_mask(rng, which, n, p):
    """common.h: vag_drop_mul for indices 0 .. n - 1 -- the multiplier, 0 or 1 / (1 - p) (fp32 division)."""
    if p <= 0.0:
        return np.ones(n, dtype=np.float32)
    with np.errstate(over="ignore"):
        seed, step = np.uint64(rng[0]), np.uint64(rng[1])
        key = _mix64(np.array([seed ^ (step * np.uint64(0xD1342543DE82EF95)) ^ (np.uint64(which) << np.uint64(56))], dtype=np.uint64))
        r = _mix64(key + np.arange(n, dtype=np.uint64))
    u = (r >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)


RNG_STATE = (0x1234567, 3)


# ---------------------------------------------------------------------------------------------------------------- GRU cell
CELL_DEFECTS = ["blend_swapped", "bhn_outside"]


def gru_cell_fwd(A, gi, h, w_hh, b_hh, defect=None):
    """-> h' (M,H), save = [r, z, n, W_hn h + b_hn]."""
    H = np.shape(w_hh)[1]
    gh = A.ein("mk,gk->mg", h, w_hh)
    if defect == "bhn_outside":                                              # b_hn added outside r * (...)
        b_in = np.concatenate([b_hh[:2 * H], np.zeros(H, np.float32)])
        gh = A.add(gh, b_in[None, :])
    else:
        gh = A.add(gh, b_hh[None, :])
    r = A.sigmoid(A.add(gi[:, :H], gh[:, :H]))
    z = A.sigmoid(A.add(gi[:, H:2 * H], gh[:, H:2 * H]))
    hn = gh[:, 2 * H:]
    pre = A.add(gi[:, 2 * H:], A.mul(r, hn))
    if defect == "bhn_outside":
        pre = A.add(pre, b_hh[None, 2 * H:])
    n = A.tanh(pre)
    omz = A.sub(_one(z), z)
    if defect == "blend_swapped":
        out = A.add(A.mul(z, n), A.mul(omz, h))
    else:
        out = A.add(A.mul(omz, n), A.mul(z, h))
    return out, [r, z, n, hn]


def gru_cell_grads(A, dh, save, h_prev):
    """The cell backward for the output gradient dh -> dgi (M,3H), dgh (M,3H), z * dh."""
    r, z, n, hn = save
    dn = A.mul(dh, A.sub(_one(z), z))
    dz = A.mul(dh, A.sub(h_prev, n))
    dpn = A.mul(dn, A.sub(_one(n), A.mul(n, n)))
    dr = A.mul(dpn, hn)
    dpr = A.mul(dr, A.mul(r, A.sub(_one(r), r)))
    dpz = A.mul(dz, A.mul(z, A.sub(_one(z), z)))
    return A.cat([dpr, dpz, dpn], -1), A.cat([dpr, dpz, A.mul(dpn, r)], -1), A.mul(z, dh)


def gru_cell_bwd(A, inp, save, defect=None):
    """vag_gru_cell_bwd: dh = dgh_next W_hh + carry + d_out, then the cell backward.  save: the forward's fp32 [4][M][H], exact."""
    dh = A.ein("mg,gh->mh", inp["dgh_next"], inp["w_hh"])
    if defect != "carry_dropped":
        dh = A.add(dh, inp["carry"])
    dh = A.add(dh, inp["d_out"])
    dgi, dgh, co = gru_cell_grads(A, dh, list(save), inp["h_prev"])
    return dict(dgi=dgi, dgh=dgh, carry_out=co)


CELL_FWD_CASES = [(5, 64), (17, 256), (20, 512), (96, 512), (130, 512)]
# vag_gru_bwd_step_launch (skinny.hip), K = 3H: `K <= 256` (H = 64) | 384 | 768 | 1536 | 3072 | the 2 x 2 wide kernel
CELL_BWD_CASES = [(5, 64), (17, 128), (17, 256), (20, 512), (16, 1024), (256, 1024)]


def _uni(rs, *shape, k=1.0):
    return _f32((rs.rand(*shape) * 2.0 - 1.0) * k)


def _gru_params(rs, inp, H):
    k = H ** -0.5
    return [_uni(rs, 3 * H, inp, k=k), _uni(rs, 3 * H, H, k=k), _uni(rs, 3 * H, k=k), _uni(rs, 3 * H, k=k)]


@functools.lru_cache(maxsize=None)
def cell_inputs(M, H):
    rs = _rs(21, M, H)
    k = H ** -0.5
    return dict(gi=_uni(rs, M, 3 * H), h_prev=_uni(rs, M, H, k=0.5), w_hh=_uni(rs, 3 * H, H, k=k), b_hh=_uni(rs, 3 * H, k=k),
                dgh_next=_uni(rs, M, 3 * H), carry=_uni(rs, M, H), d_out=_uni(rs, M, H))


def cell_fwd(A, inp, defect=None):
    out, save = gru_cell_fwd(A, A.lift(inp["gi"]), A.lift(inp["h_prev"]), inp["w_hh"], inp["b_hh"], defect)
    return dict(h_out=out, save=A.stack(save, 0))


# ---------------------------------------------------------------------------------------------------------------- lengths
def lengths_for(B, Ts, full=False):
    """Descending (the packed-sequence contract); a row of length Ts, a row of length 1 where Ts > 1, two rows of equal length;
    `full`: every row of length Ts (the case that is about that).  Exactly ONE row has length 1, the last: in a batch of 17 it is the
    only row of the second 16-row tile, and its length differs from row 15's."""
    if full or B == 1 or Ts == 1:
        return np.full(B, Ts, dtype=np.int32)
    rs = _rs(22, B, Ts)
    lens = list(rs.randint(2, Ts + 1, size=B))
    lens[0], lens[1] = Ts, 1
    if B >= 4:
        lens[2] = lens[3] = max(2, (Ts + 1) // 2)
    return np.array(sorted(lens, reverse=True), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- bi-GRU encoder
EncCase = collections.namedtuple("EncCase", "H E B Ts one_launch opt p_emb p_ctx planes full branch")


def _enc(H, E, B, Ts, one_launch, branch, opt=None, p=(0.0, 0.0), planes=True, full=False):
    return EncCase(H, E, B, Ts, one_launch, opt, p[0], p[1], planes, full, branch)


ENC_CASES = [
    # launch chain (persistent = 0)
    _enc(32, 16, 5, 4, 0, "gru_step_kernel<4>; backward K = 3H <= 256"),
    _enc(128, 32, 17, 3, 0, "backward K = 384"),
    _enc(256, 64, 17, 5, 0, "K = 256 edge; backward K = 768"),
    _enc(512, 64, 20, 3, 0, "gru_step_small_kernel (<= 160 workgroups); backward K = 1536"),
    _enc(512, 64, 96, 2, 0, "gru_step_kernel<8>"),
    _enc(512, 64, 130, 2, 0, "two row tiles per workgroup (M >= 128); last 32-row tile has 2 rows"),
    _enc(1024, 64, 16, 2, 0, "backward K = 3072"),
    _enc(256, 64, 17, 5, 0, "chain with p_emb = 0.3, p_ctx = 0.5 (vag_dropout_apply_launch on enc)", p=(0.3, 0.5)),
    # one launch
    _enc(256, 64, 1, 1, 1, "one row, one step"),
    _enc(256, 64, 17, 5, 1, "second tile of one row"),
    _enc(256, 64, 224, 2, 1, "two passes: 14 tiles, 8 + 6"),
    _enc(512, 64, 37, 7, 1, "ragged batch at H = 512; hand-off planes"),
    _enc(512, 64, 64, 3, 1, "all lengths full", full=True),
    _enc(512, 64, 100, 2, 1, "two passes: 4 + 3 tiles, last tile of 4 rows"),
    _enc(1024, 64, 20, 3, 1, "forward enc_fwd_persistent_kernel<4>; backward the chain (enc_api.hip: H == 512 || H == 256)"),
    _enc(1024, 64, 64, 2, 1, "two passes of two tiles"),
    _enc(256, 64, 17, 5, 1, "one-launch forward feeding the chain backward", opt="persistent_enc_bwd"),
    _enc(512, 64, 37, 7, 1, "fp32 hand-off (no vag_set_handoff_planes buffer)", planes=False),
    _enc(256, 64, 17, 5, 1, "one launch with p_emb = 0.3, p_ctx = 0.5 (mask applied as enc is written, recomputed in backward)",
         p=(0.3, 0.5)),
]
ENC_VS = 23
ENC_NEVER = 21                  # an embedding row no source token names (the LAST row, 22, is named)


def enc_key(c):
    """What the inputs and the reference depend on."""
    return (c.H, c.E, c.B, c.Ts, c.p_emb, c.p_ctx, c.full)


@functools.lru_cache(maxsize=None)
def enc_inputs(H, E, B, Ts, p_emb=0.0, p_ctx=0.0, full=False):
    rs = _rs(23, H, E, B, Ts)
    lens = lengths_for(B, Ts, full)
    src = np.zeros((B, Ts), dtype=np.int64)
    for b, n in enumerate(lens):
        src[b, :n] = rs.choice([t for t in range(1, ENC_VS) if t != ENC_NEVER], size=n)
    src[0, 0] = ENC_VS - 1
    d = dict(src=src, lens=lens, emb=_uni(rs, ENC_VS, E), fw=_gru_params(rs, E, H), bw=_gru_params(rs, E, H),
             d_enc=_uni(rs, B, Ts, 2 * H), g_emb0=_uni(rs, ENC_VS, E), g_fw0=_gru_params(rs, E, H), g_bw0=_gru_params(rs, E, H),
             m_emb=drop_mask(RNG_STATE, 1, Ts * B * E, p_emb).reshape(Ts, B, E),
             m_ctx=drop_mask(RNG_STATE, 2, B * Ts * 2 * H, p_ctx).reshape(B, Ts, 2 * H), p_emb=p_emb, p_ctx=p_ctx)
    return d


ENC_FWD_DEFECTS = ["rev_runs_over_padding", "enc_pad_holds_state", "tile2_takes_len_of_row15", "blend_swapped", "bhn_outside",
                   "ctx_mask_indexed_TsB"]
ENC_BWD_DEFECTS = ["carry_dropped_at_step", "pad_step_into_dxp", "g_overwritten"]


def bigru_fwd(A, inp, defect=None):
    """-> enc (B,Ts,2H), mask (B,Ts) and, for the backward and the input conditions, x, the states and the gates per direction."""
    src, lens = inp["src"], inp["lens"].copy()
    B, Ts = src.shape
    H = inp["fw"][1].shape[1]
    if defect == "tile2_takes_len_of_row15" and B > 16:
        lens[16:] = lens[15]
    x = A.lift(inp["emb"][src])                                              # (B,Ts,E): a gather, exact
    if inp["p_emb"] > 0:
        x = A.mul(x, np.transpose(inp["m_emb"], (1, 0, 2)))
    sides, saved = [], []
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate((inp["fw"], inp["bw"])):
        xp = A.add(A.ein("bte,ge->btg", x, w_ih), b_ih[None, None, :])
        h = _zeros(A, (B, H))
        outs, steps = [None] * Ts, []
        for t in (range(Ts) if d == 0 else range(Ts - 1, -1, -1)):
            live = (t < lens)[:, None]
            run = np.ones_like(live) if (defect == "rev_runs_over_padding" and d == 1) else live
            hn, save = gru_cell_fwd(A, xp[:, t], h, w_hh, b_hh, defect if defect in CELL_DEFECTS else None)
            steps.append(dict(t=t, h_prev=h, save=save, live=live))
            h = A.where(run, hn, h)
            outs[t] = h if defect == "enc_pad_holds_state" else A.where(live, h, np.zeros((B, H)))
        sides.append(A.stack(outs, 1))
        saved.append(steps)
    enc = A.cat(sides, -1)
    if inp["p_ctx"] > 0:
        m = inp["m_ctx"]
        if defect == "ctx_mask_indexed_TsB":
            m = np.transpose(m.reshape(Ts, B, 2 * H), (1, 0, 2))
        enc = A.mul(enc, m)
    return dict(enc=enc, mask=(src != 0).astype(np.float32), x=x, steps=saved)


def bigru_bwd(A, inp, fwd, defect=None):
    """fwd: bigru_fwd(A, inp) -- the workspace, recomputed.  -> g_emb and the four gradients of each direction, accumulated."""
    src, lens = inp["src"], inp["lens"]
    B, Ts = src.shape
    H = inp["fw"][1].shape[1]
    dE = A.lift(inp["d_enc"])
    if inp["p_ctx"] > 0:
        dE = A.mul(dE, inp["m_ctx"])
    out, dx = {}, None
    for d, name in enumerate(("fw", "bw")):
        w_ih, w_hh, b_ih, b_hh = inp[name]
        dh = _zeros(A, (B, H))
        dgis, dghs, hps = [None] * Ts, [], []
        steps = fwd["steps"][d]
        for k in range(Ts - 1, -1, -1):
            st = steps[k]
            t, live = st["t"], st["live"]
            tot = A.add(dh, dE[:, t, d * H:(d + 1) * H])
            dgi, dgh, carry = gru_cell_grads(A, tot, st["save"], st["h_prev"])
            if defect == "carry_dropped_at_step" and k == Ts // 2:
                carry = _zeros(A, (B, H))
            nxt = A.add(A.ein("bg,gh->bh", dgh, w_hh), carry)
            z3 = np.zeros((B, 3 * H))
            dgis[t] = dgi if defect == "pad_step_into_dxp" else A.where(live, dgi, z3)
            dghs.append(A.where(live, dgh, z3))
            hps.append(st["h_prev"])
            dh = A.where(live, nxt, dh)
        dgi_all, dgh_all, hp_all = A.stack(dgis, 1), A.stack(dghs, 1), A.stack(hps, 1)
        g0 = inp["g_" + name + "0"]
        acc = (lambda g, v: v) if defect == "g_overwritten" and d == 1 else (lambda g, v: A.add(g, v))
        out["g_%s_w_ih" % name] = A.add(g0[0], A.ein("btg,bte->ge", dgi_all, fwd["x"]))
        out["g_%s_w_hh" % name] = acc(g0[1], A.ein("btg,bth->gh", dgh_all, hp_all))
        out["g_%s_b_ih" % name] = A.add(g0[2], A.sum(A.sum(dgi_all, 1), 0))
        out["g_%s_b_hh" % name] = A.add(g0[3], A.sum(A.sum(dgh_all, 1), 0))
        part = A.ein("btg,ge->bte", dgi_all, w_ih)
        dx = part if dx is None else A.add(dx, part)
    if inp["p_emb"] > 0:
        dx = A.mul(dx, np.transpose(inp["m_emb"], (1, 0, 2)))
    E = inp["emb"].shape[1]
    rows = dx[:, :, :]
    flat = TV(rows.v.reshape(-1, E), rows.e.reshape(-1, E)) if isinstance(rows, TV) else rows.reshape(-1, E)
    # ("g_emb0_touched" is not in ENC_BWD_DEFECTS: dgi is zero on a row's padded steps, so a scatter that does not skip index 0 adds 0.0
    # there and changes no result -- tests/test_recur_ref_host.py asserts exactly that; the decoder, whose padding tokens sit on live steps, lists it)
    out["g_emb"] = A.scatter_rows(inp["g_emb0"], src.reshape(-1), flat, skip0=defect != "g_emb0_touched")
    return out


# ---------------------------------------------------------------------------------------------------------------- attention, decoder
def attn_scores(A, pe, q, v, rows_per_src=1):
    """e[n,s] = v . tanh(pe[n / rows_per_src, s] + q[n]) -> (e, th)."""
    Ts = np.shape(pe.v if isinstance(pe, TV) else pe)[1]
    if rows_per_src != 1:
        pe = np.repeat(np.asarray(pe), rows_per_src, axis=0)
    th = A.tanh(A.add(pe, A.expand(q, 1, Ts)))
    return A.ein("nsc,c->ns", th, v), th


ATTN_WIDTHS = [32, 256, 512]
ATTN_CASES = [(H, rps, Ts) for H in ATTN_WIDTHS for (rps, Ts) in ((1, 7), (3, 7), (3, 1))]


@functools.lru_cache(maxsize=None)
def attn_inputs(H, rps, Ts):
    """B = 2 sources, N = 2 rps hypotheses; source 1 has a fully masked tail (length (Ts + 1) // 2)."""
    rs = _rs(24, H, rps, Ts)
    B, C = 2, 2 * H
    mask = np.ones((B, Ts), dtype=np.float32)
    mask[1, (Ts + 1) // 2:] = 0.0
    return dict(pe=_uni(rs, B, Ts, C, k=0.5), enc=_uni(rs, B, Ts, C, k=0.5), mask=mask, q=_uni(rs, B * rps, C, k=0.5),
                v=_uni(rs, C, k=4.0 * C ** -0.5))


def bahdanau_attn(A, inp, rps, defect=None):
    sc, _ = attn_scores(A, inp["pe"], A.lift(inp["q"]), inp["v"], rps)
    mask = np.repeat(inp["mask"], rps, axis=0)
    if defect == "mask_ignored_row":
        mask = mask.copy()
        mask[-1] = 1.0
    alpha = A.softmax(sc, mask)
    return dict(scores=sc, alpha=alpha, ctx=A.ein("ns,nsc->nc", alpha, np.repeat(inp["enc"], rps, axis=0)))


ATTN_DEFECTS = ["mask_ignored_row"]

DecCase = collections.namedtuple("DecCase", "H E B Ts Tt one_launch opt acc planes d_e two_phase fwd_only branch")


def _dec(H, E, B, Ts, Tt, one_launch, branch, opt=None, acc=0, planes=True, d_e=True, two_phase=False, fwd_only=False):
    return DecCase(H, E, B, Ts, Tt, one_launch, opt, acc, planes, d_e, two_phase, fwd_only, branch)


# How long a case may be is decided by its bounds (module end, "which defect where").  The FORWARD is held to two references: the
# free-running one, whose bound is sharp for the first step or two, and the one-step one -- each step recomputed from the device's own
# previous state -- whose bound is sharp at EVERY step; so forward cases keep the issue's Tt.  The BACKWARD carries its gradient through
# every step and has one reference only: its cases run Tt = 1 at H >= 512, Tt <= 2 at H = 256 and Tt <= 3 below -- the lengths at which
# every catalogue defect still leaves the bound -- and the longer cases are `fwd_only`.
DEC_CASES = [
    # launch chain (persistent = 0)
    _dec(32, 16, 5, 4, 3, 0, "generic attention kernels, W % 512 != 0"),
    _dec(64, 16, 17, 9, 3, 0, "generic kernels on two row tiles, three steps"),
    _dec(128, 32, 17, 9, 2, 0, "the same at H = 128, two steps"),
    _dec(256, 64, 17, 9, 3, 0, "C = 512 not in the register-kernel list; cdiv(Ts, 8) = 2 ragged score blocks", fwd_only=True),
    _dec(256, 64, 17, 9, 2, 0, "the same with its backward: VAG_POST_CHUNKS = 2; _bwd_loop + _bwd_weights", two_phase=True),
    _dec(512, 64, 5, 33, 2, 0, "attn_dot_side_reg_kernel, NJ = 2, gx = 2 with a ragged second block", fwd_only=True),
    _dec(512, 64, 5, 33, 1, 0, "the same with its backward, Tt = 1: only the last-step branch; five post-backward chunks"),
    _dec(512, 64, 20, 17, 2, 0, "two row tiles at NJ = 2", fwd_only=True),
    _dec(512, 64, 20, 17, 1, 0, "three post-backward chunks"),
    _dec(512, 64, 130, 3, 2, 0, "wide side product on 32 x 64 tiles", fwd_only=True),
    _dec(512, 64, 130, 3, 1, 0, "wide side product in the backward"),
    _dec(768, 64, 5, 4, 2, 0, "NJ = 3", fwd_only=True),
    _dec(768, 64, 5, 4, 1, 0, "NJ = 3; backward W = 2304: generic kernel"),
    _dec(1024, 64, 16, 5, 2, 0, "NJ = 4", fwd_only=True),
    _dec(1024, 64, 16, 5, 1, 0, "NJ = 4; backward W = 3072: register kernel"),
    _dec(1536, 64, 4, 3, 2, 0, "NJ = 6", fwd_only=True),
    _dec(1536, 64, 4, 3, 1, 0, "NJ = 6; backward W = 4608: generic kernel"),
    _dec(32, 16, 5, 4, 3, 0, "accumulate_enc = 1", acc=1),
    _dec(32, 16, 5, 4, 1, 0, "Tt = 1: only the last-step branch; d_h0 from step 0 alone"),
    _dec(256, 64, 16, 49, 2, 0, "one past the largest Ts whose keys fit the LDS: reports unsupported, runs the chain"),
    # one launch
    _dec(256, 64, 1, 1, 1, 1, "one row, one step"),
    _dec(256, 64, 17, 5, 3, 1, "second tile of one row, three steps", fwd_only=True),
    _dec(256, 64, 17, 5, 2, 1, "second tile of one row; d_e_all = NULL; hand-off planes; _bwd_loop + _bwd_weights", d_e=False,
         two_phase=True),
    _dec(256, 64, 17, 5, 2, 1, "one-launch forward feeding the chain backward", opt="persistent_dec_bwd"),
    _dec(256, 64, 17, 5, 2, 1, "fp32 hand-off (no vag_set_handoff_planes buffer)", planes=False),
    _dec(256, 64, 16, 48, 2, 1, "largest Ts whose keys fit the LDS by dec_persistent_lds_bytes; accumulate_enc = 1", acc=1),
    _dec(256, 64, 224, 3, 2, 1, "two passes at H = 256"),
    _dec(512, 64, 37, 9, 7, 1, "ragged batch at H = 512, seven steps", fwd_only=True),
    _dec(512, 64, 64, 12, 5, 1, "full batch of one pass, five steps", fwd_only=True),
    _dec(512, 64, 100, 4, 2, 1, "two passes", fwd_only=True),
    _dec(512, 64, 37, 9, 1, 1, "ragged batch at H = 512 with its backward; hand-off planes"),
    _dec(512, 64, 64, 12, 1, 1, "full batch of one pass with its backward"),
    _dec(512, 64, 100, 4, 1, 1, "two passes with their backward"),
    _dec(256, 64, 17, 5, 1, 1, "Tt = 1 in one launch, two tiles"),
    _dec(512, 64, 37, 9, 1, 1, "one-launch forward feeding the chain backward at H = 512", opt="persistent_dec_bwd"),
    _dec(512, 64, 37, 9, 1, 1, "fp32 hand-off at H = 512 (no vag_set_handoff_planes buffer)", planes=False),
]
DEC_VT = 19
DEC_NEVER = 17


def dec_group(H):
    """The three groups the ratio table reports the decoder's backward in (their backward lengths differ: DEC_CASES)."""
    return " H<=128" if H <= 128 else " H=256" if H == 256 else " H>=512"


def dec_key(c):
    return (c.H, c.E, c.B, c.Ts, c.Tt)


def dec_lds_bytes(Ts):
    """persist.hip: dec_persistent_lds_bytes(Ts) -- the one-launch decoder wants it <= 160 KiB."""
    return 4 * (6144 + 16 * Ts * 16 + 16 * Ts * 24 + 16 * Ts + 16 * 24 + 16 * 24 + 80 + 256 + 1024 + 16 * Ts + 256)


DEC_MAX_TS = max(ts for ts in range(1, 513) if dec_lds_bytes(ts) <= 160 * 1024)


@functools.lru_cache(maxsize=None)
def dec_inputs(H, E, B, Ts, Tt):
    rs = _rs(25, H, E, B, Ts, Tt)
    C = 2 * H
    lens = lengths_for(B, Ts)
    mask = (np.arange(Ts)[None, :] < lens[:, None]).astype(np.float32)
    tok = rs.choice([t for t in range(1, DEC_VT) if t != DEC_NEVER], size=(Tt + 1, B)).astype(np.int64)
    tok[0] = 2
    if B > 1 and Tt > 1:
        tok[1:, B - 1] = 0                                                   # a finished sentence: padding from step 1 on
    tok[Tt - 1, 0] = DEC_VT - 1
    gp = lambda: [_gru_params(rs, E, H), _uni(rs, C, H, k=H ** -0.5), _uni(rs, C, k=C ** -0.5), _uni(rs, H, C, k=C ** -0.5),
                  _gru_params(rs, H, H)]
    P = gp()
    G = gp()
    names = ["w_ih1", "w_hh1", "b_ih1", "b_hh1", "attn_h", "attn_v", "c2h", "w_ih2", "w_hh2", "b_ih2", "b_hh2"]
    flat = lambda p: dict(zip(names, p[0] + [p[1], p[2], p[3]] + p[4]))
    d = dict(enc=_uni(rs, B, Ts, C, k=0.5), pe=_uni(rs, B, Ts, C, k=0.5), mask=mask, h0=_uni(rs, B, H, k=0.5), tok=tok,
             emb=_uni(rs, DEC_VT, E), w=flat(P), g0=flat(G), g_emb0=_uni(rs, DEC_VT, E),
             d_h2=_uni(rs, Tt, B, H), d_c=_uni(rs, Tt, B, C), d_e=_uni(rs, Tt, B, E), d_enc0=_uni(rs, B, Ts, C))
    return d


DEC_W_NAMES = ["emb", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "attn_h", "attn_v", "c2h", "w_ih2", "w_hh2", "b_ih2", "b_hh2"]
DEC_FWD_DEFECTS = ["gru2_blends_h2_prev", "query_from_h2_prev", "mask_ignored_row", "blend_swapped", "bhn_outside",
                   "stale_h2_at_late_step"]
DEC_BWD_DEFECTS = ["softmax_bwd_without_sum", "dalpha_without_gru2", "carry_dropped_at_step", "d_h0_without_carry", "g_overwritten",
                   "accumulate_enc_ignored", "g_emb0_touched", "d_e_all_ignored"]


def cgru_fwd(A, inp, h2_given=None, defect=None):
    """-> h2_all (Tt,B,H), c_all (Tt,B,C), e_all (Tt,B,E) and the per-step workspace.  h2_given: fp32 (Tt,B,H), the states the
    recomputation of each step starts from (the backward's argument h2_all, exact)."""
    w, tok = inp["w"], inp["tok"]
    Tt = tok.shape[0] - 1
    B, Ts, C = inp["enc"].shape
    cd = defect if defect in CELL_DEFECTS else None
    e_all = inp["emb"][tok[:Tt]]                                             # a gather: exact
    xp1 = A.add(A.ein("tbe,ge->tbg", e_all, w["w_ih1"]), w["b_ih1"][None, None, :])
    uk = A.ein("bsc,hc->bsh", inp["enc"], w["c2h"])                           # context2hid on the keys, then W_ih2 on the result
    encwp = A.ein("bsh,gh->bsg", uk, w["w_ih2"])
    mask = inp["mask"]
    if defect == "mask_ignored_row":
        mask = mask.copy()
        mask[np.argmin(mask.sum(1))] = 1.0
    h2 = A.lift(inp["h0"])
    steps, h2s, cs = [], [], []
    for t in range(Tt):
        hprev = h2 if (h2_given is None or t == 0) else A.lift(h2_given[t - 1])
        if defect == "stale_h2_at_late_step" and t >= 2:                        # a hand-off read one step late: h2_{t-2}
            hprev = h2s[t - 2]
        h1, s1 = gru_cell_fwd(A, xp1[t], hprev, w["w_hh1"], w["b_hh1"], cd)
        h1 = A.mark(h1)
        q = A.ein("bh,ch->bc", hprev if defect == "query_from_h2_prev" else h1, w["attn_h"])
        sc, th = attn_scores(A, inp["pe"], q, w["attn_v"])
        alpha = A.softmax(sc, mask)
        gi2 = A.add(A.ein("bs,bsg->bg", alpha, encwp), w["b_ih2"][None, :])
        h2, s2 = gru_cell_fwd(A, gi2, hprev if defect == "gru2_blends_h2_prev" else h1, w["w_hh2"], w["b_hh2"], cd)
        h2 = A.mark(h2)
        c = A.ein("bs,bsc->bc", alpha, inp["enc"])
        steps.append(dict(hprev=hprev, h1=h1, s1=s1, s2=s2, th=th, alpha=alpha, scores=sc))
        h2s.append(h2)
        cs.append(c)
    return dict(h2_all=A.stack(h2s, 0), c_all=A.stack(cs, 0), e_all=e_all, steps=steps, uk=uk, encwp=encwp)


def cgru_bwd(A, inp, fwd, c_all, e_all, acc=0, with_d_e=True, defect=None):
    """fwd: cgru_fwd(A, inp, h2_given = the device's h2_all) -- the workspace, recomputed; c_all, e_all: the forward's fp32 outputs, exact.
    -> d_enc_out, d_pe, d_h0 and the twelve accumulated parameter gradients g_*."""
    w, tok = inp["w"], inp["tok"]
    Tt = tok.shape[0] - 1
    B, Ts, C = inp["enc"].shape
    H = C // 2
    enc, encwp, v = inp["enc"], fwd["encwp"], w["attn_v"]
    carry_in = _zeros(A, (B, H))
    d_pe = _zeros(A, (B, Ts, C))
    per = dict(dgi1=[None] * Tt, dgh1=[None] * Tt, dgi2=[None] * Tt, dgh2=[None] * Tt, dq=[None] * Tt, ds=[None] * Tt)
    g_v = None
    for t in range(Tt - 1, -1, -1):
        st = fwd["steps"][t]
        dh2 = A.add(carry_in, inp["d_h2"][t])
        dgi2, dgh2, carry2 = gru_cell_grads(A, dh2, st["s2"], st["h1"])
        dalpha = A.ein("bsc,bc->bs", enc, inp["d_c"][t])
        if defect != "dalpha_without_gru2":
            dalpha = A.add(dalpha, A.ein("bsg,bg->bs", encwp, dgi2))
        alpha = st["alpha"]
        if defect == "softmax_bwd_without_sum":
            ds = A.mul(alpha, dalpha)
        else:
            ds = A.mul(alpha, A.sub(dalpha, A.expand(A.sum(A.mul(alpha, dalpha), -1), -1, Ts)))
        th = st["th"]
        dth = A.mul(A.expand(ds, -1, C), A.mul(A.sub(_one(th), A.mul(th, th)), v[None, None, :]))
        d_pe = A.add(d_pe, dth)
        dq = A.sum(dth, 1)
        gv_t = A.ein("bs,bsc->c", ds, th)
        g_v = gv_t if g_v is None else A.add(g_v, gv_t)
        dh1 = A.add(A.add(A.ein("bc,ch->bh", dq, w["attn_h"]), A.ein("bg,gh->bh", dgh2, w["w_hh2"])), carry2)
        dgi1, dgh1, carry1 = gru_cell_grads(A, dh1, st["s1"], st["hprev"])
        if defect == "carry_dropped_at_step" and t == Tt // 2:
            carry1 = _zeros(A, (B, H))
        if defect == "d_h0_without_carry" and t == 0:
            carry1 = _zeros(A, (B, H))
        carry_in = A.add(A.ein("bg,gh->bh", dgh1, w["w_hh1"]), carry1)
        for k, x in (("dgi1", dgi1), ("dgh1", dgh1), ("dgi2", dgi2), ("dgh2", dgh2), ("dq", dq), ("ds", ds)):
            per[k][t] = x
    S = {k: A.stack(x, 0) for k, x in per.items()}
    alpha_all = A.stack([st["alpha"] for st in fwd["steps"]], 0)               # (Tt,B,Ts)
    h1_all = A.stack([st["h1"] for st in fwd["steps"]], 0)
    hp_all = A.stack([st["hprev"] for st in fwd["steps"]], 0)
    du = A.ein("tbg,gh->tbh", S["dgi2"], w["w_ih2"])
    d_enc = A.add(A.ein("tbs,tbc->bsc", alpha_all, inp["d_c"]), A.ein("bsh,hc->bsc", A.ein("tbs,tbh->bsh", alpha_all, du), w["c2h"]))
    if acc and defect != "accumulate_enc_ignored":
        d_enc = A.add(inp["d_enc0"], d_enc)
    u_all = A.ein("tbs,bsh->tbh", alpha_all, fwd["uk"])
    g0 = inp["g0"]
    tsum = lambda x: A.sum(A.sum(x, 0), 0)
    out = dict(d_enc_out=d_enc, d_pe=d_pe, d_h0=carry_in)
    out["g_w_hh2"] = A.add(g0["w_hh2"], A.ein("tbg,tbh->gh", S["dgh2"], h1_all))
    out["g_b_hh2"] = A.add(g0["b_hh2"], tsum(S["dgh2"]))
    out["g_attn_h"] = A.add(g0["attn_h"], A.ein("tbc,tbh->ch", S["dq"], h1_all))
    out["g_attn_v"] = A.add(g0["attn_v"], g_v)
    out["g_w_ih2"] = A.add(g0["w_ih2"], A.ein("tbg,tbh->gh", S["dgi2"], u_all))
    out["g_b_ih2"] = A.add(g0["b_ih2"], tsum(S["dgi2"]))
    out["g_c2h"] = A.add(g0["c2h"], A.ein("tbh,tbc->hc", du, c_all))
    prod = A.ein("tbg,tbh->gh", S["dgh1"], hp_all)
    out["g_w_hh1"] = prod if defect == "g_overwritten" else A.add(g0["w_hh1"], prod)
    out["g_b_hh1"] = A.add(g0["b_hh1"], tsum(S["dgh1"]))
    out["g_w_ih1"] = A.add(g0["w_ih1"], A.ein("tbg,tbe->ge", S["dgi1"], e_all))
    out["g_b_ih1"] = A.add(g0["b_ih1"], tsum(S["dgi1"]))
    de = A.ein("tbg,ge->tbe", S["dgi1"], w["w_ih1"])
    if with_d_e and defect != "d_e_all_ignored":
        de = A.add(inp["d_e"], de)
    E = inp["emb"].shape[1]
    flat = TV(de.v.reshape(-1, E), de.e.reshape(-1, E)) if isinstance(de, TV) else de.reshape(-1, E)
    out["g_emb"] = A.scatter_rows(inp["g_emb0"], tok[:Tt].reshape(-1), flat, skip0=defect != "g_emb0_touched")
    return out


# ---------------------------------------------------------------------------------------------------------------- decoding step
STEP_CASES = [(H, rps) for H in ATTN_WIDTHS for rps in (1, 3)]
STEP_TS, STEP_B = 5, 3


def step_e(H):
    return 16 if H == 32 else 64


@functools.lru_cache(maxsize=None)
def step_inputs(H, rps):
    d = dict(dec_inputs(H, step_e(H), STEP_B, STEP_TS, 1))
    rs = _rs(26, H, rps)
    N = STEP_B * rps
    d["tok1"] = rs.choice([t for t in range(1, DEC_VT)], size=N).astype(np.int64)
    d["h_in"] = _uni(rs, N, H, k=0.5)
    return d


STEP_DEFECTS = ["gru2_blends_h2_prev", "query_from_h2_prev", "source_row_not_divided"]


def cgru_step(A, inp, rps, defect=None):
    """vag_cgru_attn_decode_step: one step for N = B rps hypotheses; the context enters gru_2 through the folded W_ih2 W_c2h (module
    docstring: two associations of one product); no mark."""
    w = inp["w"]
    N = inp["h_in"].shape[0]
    srow = np.arange(N) // rps
    if defect == "source_row_not_divided":
        srow = np.arange(N) % (N // rps)
    e = inp["emb"][inp["tok1"]]
    h_in = A.lift(inp["h_in"])
    xp1 = A.add(A.ein("ne,ge->ng", e, w["w_ih1"]), w["b_ih1"][None, :])
    h1, _ = gru_cell_fwd(A, xp1, h_in, w["w_hh1"], w["b_hh1"])
    q = A.ein("nh,ch->nc", h_in if defect == "query_from_h2_prev" else h1, w["attn_h"])
    sc, _ = attn_scores(A, inp["pe"][srow], q, w["attn_v"])
    alpha = A.softmax(sc, inp["mask"][srow])
    c = A.ein("ns,nsc->nc", alpha, inp["enc"][srow])
    wp = A.ein("gh,hc->gc", w["w_ih2"], w["c2h"])
    gi2 = A.add(A.ein("nc,gc->ng", c, wp), w["b_ih2"][None, :])
    h2, _ = gru_cell_fwd(A, gi2, h_in if defect == "gru2_blends_h2_prev" else h1, w["w_hh2"], w["b_hh2"])
    return dict(h_out=h2, c=c, e=e, alpha=alpha)


# ---------------------------------------------------------------------------------------------------------------- which defect where
# A defect is listed at EVERY case at which it changes a result, and the host test asserts that it leaves the bound at each: no case
# is excused because its bound has grown.  That is what sets the lengths of the cases: the worst-case propagation through a product
# over K terms widens an error by up to sum|w| ~ sqrt(K) / 2, three or four products deep per decoder step, so a carried quantity's
# bound passes the quantity itself after two or three steps at H >= 256 (measured at the issue's own (512, 64, 37, 9, 7): the median
# bound of every backward output 1e7 and more times its median size).  The forward escapes through its one-step reference (DEC_CASES);
# the backward does not, and its cases are as short as DEC_CASES says.  The encoder's products are one deep per step and its cases keep
# the issue's lengths: at (512, 64, 37, 7) the least-rejected defect still leaves the bound by a factor of 2.
def enc_defect_cases(defect):
    keys = []
    for c in ENC_CASES:
        k = enc_key(c)
        if k in keys:
            continue
        ragged = c.B > 1 and c.Ts > 1 and not c.full
        if defect in ("rev_runs_over_padding", "enc_pad_holds_state", "pad_step_into_dxp") and not ragged:
            continue
        if defect == "tile2_takes_len_of_row15" and not (c.B > 16 and ragged):
            continue
        if defect == "ctx_mask_indexed_TsB" and not (c.p_ctx > 0):
            continue
        if defect == "carry_dropped_at_step" and c.Ts < 2:
            continue
        keys.append(k)
    return keys


def dec_defect_cases(defect):
    keys = []
    for c in DEC_CASES:
        k = dec_key(c)
        if k in keys:
            continue
        if defect in ("mask_ignored_row", "query_from_h2_prev") and not (c.B > 1 and c.Ts > 1):      # (Ts = 1: alpha = 1 whatever q is)
            continue
        if defect == "carry_dropped_at_step" and c.Tt < 2:
            continue
        if defect == "g_emb0_touched" and not (c.B > 1 and c.Tt > 1):                             # (no padding token otherwise)
            continue
        if defect in ("softmax_bwd_without_sum", "dalpha_without_gru2") and c.Ts == 1:            # (d alpha has no effect: alpha = 1)
            continue
        if defect == "accumulate_enc_ignored" and not c.acc:
            continue
        if defect in DEC_BWD_DEFECTS and c.fwd_only:
            continue
        if defect == "stale_h2_at_late_step" and c.Tt < 3:
            continue
        keys.append(k)
    return keys
