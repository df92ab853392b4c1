"""Float64 references WITH THEIR OWN ERROR BOUND for the HOISTED decoding step and the per-step output head -- what every search
runs once per decode call and once per step -- written from the definitions in include/vag_nmt.h, in the manner of tests/recur_ref.py:

    vag_cgru_decode_keys          "the keys as gru_2 sees them and the head's share of them are projected once per decode call
                                   (vag_cgru_decode_keys: keys = [(W_ih2 W_c2h) enc (B,Ts,3H) | enc W2^T (B,Ts,E)],
                                   vag_cgru_decode_keys_floats floats; prep from vag_cgru_prepare, w2 = head W2 (E,C))"
    vag_cgru_decode_tables        "tables (optional, NULL: none): [emb W_ih1^T + b_ih1 (V,3H) | emb W3^T (V,E)] from
                                   vag_cgru_decode_tables, once per call (w3 = head W3): a step then has no embedding / input-projection
                                   launch, `e` is not produced (may be NULL) and the head reads its share of the embedded token from the
                                   table line `tok` picks."
    vag_cgru_attn_decode_step_h   "a step is then four launches and returns cw (N,E) = W2 c instead of the context c, which
                                   vag_head_logp_step_h / vag_head_logits_step_h take in its place.  N <= 256 hypotheses, rows_per_src
                                   divides N."  Hypothesis n attends over source sentence n / rows_per_src; h_in (N,H) -> h_out (N,H).
    vag_head_logp_step (_h)       "Single step, inference: logp (N,V) = log_softmax(out(tanh(...))) and argmax (int64[N], may be NULL)";
                                   "t = tanh(W1 h2 + W2 c + W3 e + b1+b2+b3); ... logits = t out_w^T + out_b; log_softmax".
    vag_head_logits_step (_h)     "the vocabulary product of vag_head_logits_step leaves, per row, vag_head_logits_parts_count (max,
                                   sum exp) pairs -- the pieces of the row's log-sum-exp -- in `parts` (count, N, 2)".

Every operator is written ONCE over an arithmetic `A` (ground_ref's docstring): A = T, tracked (value, err) pairs; A = F, the fp32
restatement.  T and F here extend recur_ref's without changing a rule that recur_ref's or ground_ref's operators use.

What enters exactly.  `keys` and `tables` are ARGUMENTS of vag_cgru_attn_decode_step_h and of the _h heads: the fp32 arrays that the
device's own vag_cgru_decode_keys / _tables produced (on the host: the restatement's).  They carry no error inside the step; their own
error is held by decode_keys / decode_tables.  The head's h2, c, cw, e are arguments too.

Associations.  decode_keys forms Wp = W_ih2 W_c2h first (what vag_cgru_prepare stores) and applies it to enc: two tracked contractions
in that order.  The hoisted step forms gi2 = sum_s alpha_s encwp_s + b_ih2 and cw = sum_s alpha_s encw2_s: alpha-weighted sums of key
rows, one contraction each with the keys exact; recur_ref.cgru_step restates the plain step's Wp (sum_s alpha_s enc_s).  The hoisted
head adds cw where the plain head has W2 c, and KEEPS b2: pre = W1 h2 + b1 + b2 + b3 + cw + (W3 e | the line of embw3 that tok picks).

The one new tracked rule, u = 2^-24:

  logsumexp  head.hip lse_nll_kernel: l = m + __logf(sum_j __expf(x_j - m)), m the row's maximum; skinny.hip's epilogue leaves
             per 64 columns (m_i, sum_j exp(x_j - m_i)), merged as sum exp(m_i - M).  The value is shift invariant, so the error of m
             cancels (softmax rule).  With p_j = exp(x_j - m) / S the softmax weights and d_j = m - x_j >= 0:
               argument      an error e_j of x_j moves term j by a relative exp(e_j) - 1 (second order kept, as in the softmax rule);
               exponential   ground_ref's exp rule: the subtraction x_j - m rounds, ULP d_j, and __expf adds (d_j + 2) 2^-23: the
                             issue's (|x_j - m| + 2) 2^-23 per term; d_j is taken at the far end of its interval, d_j + e_j + e_max;
               rescaling     the streaming form keeps a running (max, sum) per thread and multiplies the sum by exp(m_old - m_new)
                             whenever a group of 16 values raises the maximum, and once more by exp(m_thread - m) at the end; the parts
                             merge does the same twice inside the kernel (the two 32-column halves, the two lane halves).  The
                             shifts a term passes through add up to at most d_j (m_first >= x_j and the last maximum is m), each
                             shift's subtraction and exponential are relative ULP + 2^-23 per unit of shift, and each of the k steps
                             adds the exponential's 2 * 2^-23, one product and one addition (ULP each):
                             d_j 2^-22 + k 2^-21 per term.  k = 0 in the register forms (V <= 10240), ceil(ceil(V / 4) / 1024) + 1 in
                             the streaming form (one rescale per sweep of 1024 float4, one at the end), 2 for the parts (what follows,
                             lse_from_parts, is float64);
               summation     EPS, the suite's convention for an fp32 sum in any order;
             so S carries the relative error rel = sum_j p_j (exp(e_j + ULP d_j + (d_j + 2) 2^-23 + d_j 2^-22 + k 2^-21) - 1) + EPS and
             log S moves by at most -log(1 - rel);
               logarithm     __logf is the native form: v_log_f32 (log2, 1 ulp) times ln 2 -- one more rounding and the rounded
                             constant: 2^-22 |log S| relative in all; S >= 1 (the maximum's own term), and next to 1 the hardware's
                             result is good to an ulp of its argument's spacing, an absolute 2^-24: |log S| 2^-22 + 2^-24;
               final sum     m + log S: ULP (|m| + |log S|).
             err = -log(1 - rel) + |log S| 2^-22 + 2^-24 + ULP (|m| + |log S|).  logp = x - lse by T.sub.
  exp        for the parts' own sums (s_i against sum_j exp(x_j - m_i) over the group's real columns, x the device's own logits and
             m_i their own maximum: the difference is exact or rounds by ULP d): ground_ref's exp rule as a function, relative
             exp(e) - 1 + (|x| + 2) 2^-23, then T.sum, then the two rescaling steps above as a relative d 2^-22 + 2 * 2^-21 of the sum.

The case tables of tests/test_gpu_decode_step.py, the input generators and the defect catalogue live here, so that
tests/test_decode_ref_host.py checks the bounds at exactly the shapes and inputs the device is tested at.  Inputs: the recurrences'
(recur_ref.dec_inputs: ragged lengths from lengths_for, a sentence of full length and -- B > 1, Ts > 1 -- exactly one of length 1, keys
that stay nonzero past a row's length so that an ignored mask shows) plus h_in, the tokens and the head's W2, W3.  tok holds line 0 and
line V - 1, rows 0 and N - 1 share line 0, and with rows_per_src > 1 the rows of one sentence differ in token and in h_in.  The head's
out_b[V - 1] is raised by 3: the last column is then the maximum of its thread's last, partial group of 16 in the streaming form, so a
tail that is merged without its rescaling step moves the row's log-sum-exp (catalogue: lse_without_max_shift_of_tail)."""
import functools

import numpy as np

import recur_ref as R
from recur_ref import T as _T, F as _F, TV, ratio, gru_cell_fwd, attn_scores, dec_inputs, _uni, _rs   # noqa: F401 (re-exported)
from ground_ref import ULP, EPS, U24

LOG_REL = 2.0 ** -22            # (module docstring: logarithm)
RESCALE_STEP = 2.0 ** -21       # (module docstring: rescaling, per step)
RESCALE_SHIFT = 2.0 ** -22      # (the same, per unit of shift)
EXP_REL = 2.0 ** -23


def stream_rescales(V):
    """Rescaling steps a term of lse_nll_kernel passes through: none in the register forms, one per sweep and one at the end."""
    return 0 if V <= 10240 else -(-((V + 3) // 4) // 1024) + 1


PARTS_RESCALES = 2


# ---------------------------------------------------------------------------------------------------------------- the two arithmetics
class T(_T):
    """recur_ref.T with exp (as a function) and logsumexp (module docstring)."""

    @staticmethod
    def exp(a):
        a = _T.lift(a)
        v = np.exp(a.v)
        return TV(v, v * (np.expm1(a.e) + (np.abs(a.v) + a.e + 2.0) * EXP_REL))

    @staticmethod
    def logsumexp(x, rescales=0):
        """Rows of x (.., V) -> lse (..)."""
        x = _T.lift(x)
        m = x.v.max(-1, keepdims=True)
        e_max = np.take_along_axis(x.e, x.v.argmax(-1)[..., None], -1)
        d = m - x.v
        p = np.exp(-d)
        S = p.sum(-1, keepdims=True)
        df = d + x.e + e_max
        with np.errstate(over="ignore"):
            r = np.expm1(x.e + ULP * df + (df + 2.0) * EXP_REL + df * RESCALE_SHIFT + rescales * RESCALE_STEP)
            rel = ((p * r).sum(-1, keepdims=True) / S + EPS)[..., 0]
        logS, m = np.log(S)[..., 0], m[..., 0]
        dlog = np.where(rel < 0.5, -np.log1p(-np.minimum(rel, 0.5)), np.inf)       # (a bound that has passed 1/2 says nothing)
        return TV(m + logS, dlog + np.abs(logS) * LOG_REL + U24 + ULP * (np.abs(m) + np.abs(logS)))


class F(_F):
    """recur_ref.F with the same additions: the register form of lse_nll_kernel, its streaming form thread by thread."""

    @staticmethod
    def exp(a):
        return np.exp(_F.lift(a), dtype=np.float32)

    @staticmethod
    def logsumexp(x, streaming=False, defect=None):
        x = _F.lift(x)
        f = np.float32
        if not streaming:
            m = x.max(-1, keepdims=True)
            s = np.exp(x - m, dtype=f).sum(-1, dtype=f)
            return (m[..., 0] + np.log(s, dtype=f)).astype(f)
        # thread t of 256 takes the float4 i0 = t + 256 u + 1024 k (u < 4) in sweep k: 16 values per thread and sweep
        lead, V = x.shape[:-1], x.shape[-1]
        sweeps = -(-((V + 3) // 4) // 1024)
        pad = np.full(lead + (sweeps * 4096,), -np.inf, dtype=f)
        pad[..., :V] = x
        g = np.moveaxis(pad.reshape(lead + (sweeps, 4, 256, 4)), -2, -4).reshape(lead + (256, sweeps, 16))
        mx = np.full(lead + (256,), -np.inf, dtype=f)
        sm = np.zeros(lead + (256,), dtype=f)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(sweeps):
                e = g[..., k, :]
                gm = np.maximum(mx, e.max(-1))
                live = gm > -np.inf
                part = np.where(live, np.exp(e - np.where(live, gm, f(0))[..., None], dtype=f).sum(-1, dtype=f), f(0))
                scale = np.where(mx > -np.inf, np.exp(mx - gm, dtype=f), f(0))
                if defect == "lse_without_max_shift_of_tail":             # the partial group: some of its 16 values lie past V
                    partial = np.isinf(e).any(-1) & ~np.isinf(e).all(-1)
                    scale = np.where(partial & (mx > -np.inf), f(1), scale)
                sm = np.where(live, (sm * scale).astype(f) + part, sm).astype(f)
                mx = np.where(live, gm, mx)
            bm = mx.max(-1, keepdims=True)
            tot = np.where(mx > -np.inf, sm * np.exp(mx - bm, dtype=f), f(0)).astype(f).sum(-1, dtype=f)
        return (bm[..., 0] + np.log(tot, dtype=f)).astype(f)


def round64(n):
    return (int(n) + 63) // 64 * 64


def keys_layout(B, Ts, E, H):
    """kernels.h WsCarver: every region starts on a multiple of 64 floats -> (offset of encw2, total)."""
    return round64(B * Ts * 3 * H), round64(B * Ts * 3 * H) + round64(B * Ts * E)


def tables_layout(V, E, H):
    return round64(V * 3 * H), round64(V * 3 * H) + round64(V * E)


# ---------------------------------------------------------------------------------------------------------------- once per call
def decode_keys(A, enc, w, w2):
    """-> encwp (B,Ts,3H) = enc (W_ih2 W_c2h)^T, the product formed first; encw2 (B,Ts,E) = enc W2^T."""
    wp = A.ein("gh,hc->gc", w["w_ih2"], w["c2h"])
    return A.ein("bsc,gc->bsg", enc, wp), A.ein("bsc,ec->bse", enc, w2)


def decode_tables(A, emb, w, w3):
    """-> embp (V,3H) = emb W_ih1^T + b_ih1; embw3 (V,E) = emb W3^T."""
    return A.add(A.ein("ve,ge->vg", emb, w["w_ih1"]), w["b_ih1"][None, :]), A.ein("ve,fe->vf", emb, w3)


HPAIRS = [(32, 16), (256, 64), (512, 64), (512, 256), (1024, 256)]
KEYS_CASES = [(H, E, B, Ts) for (H, E) in HPAIRS for (B, Ts) in ((1, 1), (2, 5), (6, 11))]            # B Ts = 1, 10, 66
TABLES_CASES = [(H, E, 19) for (H, E) in HPAIRS] + [(512, 256, 4100)]


@functools.lru_cache(maxsize=None)
def keys_inputs(H, E, B, Ts):
    """The recurrences' decoder weights and keys (a whole vag_dec_w: vag_cgru_prepare reads it) and the head's W2."""
    rs = _rs(31, H, E, B, Ts)
    d = dec_inputs(H, E, B, Ts, 1)
    return dict(enc=d["enc"], emb=d["emb"], w=d["w"], w2=_uni(rs, E, 2 * H, k=(2 * H) ** -0.5))


@functools.lru_cache(maxsize=None)
def tables_inputs(H, E, V):
    rs = _rs(32, H, E, V)
    return dict(emb=_uni(rs, V, E), w3=_uni(rs, E, E, k=E ** -0.5), w=dec_inputs(H, E, 1, 1, 1)["w"])


# ---------------------------------------------------------------------------------------------------------------- the hoisted step
# (H, E, B, rps, Ts, attn_row)
HSTEP_CASES = [
    (32, 16, 3, 1, 5, 1), (256, 64, 3, 3, 5, 1), (512, 64, 3, 3, 5, 1), (512, 256, 3, 1, 1, 1), (512, 256, 2, 3, 7, 1),
    (512, 256, 2, 12, 16, 1), (512, 256, 2, 12, 17, 1), (512, 256, 1, 5, 32, 1), (512, 256, 2, 3, 33, 1), (512, 256, 2, 3, 7, 0),
    (512, 256, 16, 16, 9, 1), (1024, 256, 2, 2, 5, 1),
]
HSTEP_V = R.DEC_VT


def hstep_key(c):
    """What the inputs and the reference depend on (attn_row chooses the kernel, not the result)."""
    return tuple(c[:5])


@functools.lru_cache(maxsize=None)
def hstep_inputs(H, E, B, rps, Ts):
    d = dict(dec_inputs(H, E, B, Ts, 1))
    rs = _rs(33, H, E, B, rps, Ts)
    N, C, V = B * rps, 2 * H, HSTEP_V
    tok = rs.randint(1, V - 1, size=N).astype(np.int64)
    tok[0] = 0
    if N > 1:
        tok[1] = V - 1
    if N > 2:
        tok[N - 1] = 0
    d.update(tok1=tok, h_in=_uni(rs, N, H, k=0.5), w2=_uni(rs, E, C, k=C ** -0.5), w3=_uni(rs, E, E, k=E ** -0.5))
    return d


HSTEP_DEFECTS = ["gi2_without_b_ih2", "keys_of_row_n", "cw_from_scores", "last_position_dropped", "mask_ignored_row", "gru2_blends_h_in"]
HSTEP_TABLE_DEFECTS = ["table_line_of_neighbour_row"]


def cgru_step_h(A, inp, rps, keys, tables=None, defect=None):
    """keys = (encwp, encw2), tables = None or (embp, embw3): fp32 arrays, exact.  -> h_out (N,H), cw (N,E), e (N,E; None with tables),
    alpha (N,Ts)."""
    w = inp["w"]
    N = inp["h_in"].shape[0]
    srow = np.arange(N) // rps
    krow = np.arange(N) % (N // rps) if defect == "keys_of_row_n" else srow
    tok = inp["tok1"]
    h_in = A.lift(inp["h_in"])
    if tables is None:
        e = inp["emb"][tok]                                                  # a gather: exact
        gi1 = A.add(A.ein("ne,ge->ng", e, w["w_ih1"]), w["b_ih1"][None, :])
    else:
        e = None
        line = tok[np.minimum(np.arange(N) ^ 1, N - 1)] if defect == "table_line_of_neighbour_row" else tok
        gi1 = A.lift(tables[0][line])                                        # the line of embp that tok picks: exact
    h1, _ = gru_cell_fwd(A, gi1, h_in, w["w_hh1"], w["b_hh1"])
    q = A.ein("nh,ch->nc", h1, w["attn_h"])
    sc, _ = attn_scores(A, inp["pe"][srow], q, w["attn_v"])
    mask = inp["mask"][srow]
    if defect == "mask_ignored_row":
        mask = mask.copy()
        mask[-1] = 1.0
    alpha = A.softmax(sc, mask)
    wts = alpha
    if defect == "cw_from_scores":                                           # the numerators exp(e_s - max), not divided by their sum
        x = np.where(mask != 0, sc, np.float32(-np.inf))
        wts = np.exp(x - x.max(-1, keepdims=True), dtype=np.float32)
    wk = alpha
    if defect == "last_position_dropped":
        wk = wts = np.concatenate([alpha[:, :-1], np.zeros((N, 1), np.float32)], 1)
    gi2 = A.ein("ns,nsg->ng", wk, keys[0][krow])
    if defect != "gi2_without_b_ih2":
        gi2 = A.add(gi2, w["b_ih2"][None, :])
    cw = A.ein("ns,nse->ne", wts, keys[1][krow])
    h2, _ = gru_cell_fwd(A, gi2, h_in if defect == "gru2_blends_h_in" else h1, w["w_hh2"], w["b_hh2"])
    return dict(h_out=h2, cw=cw, e=e, alpha=alpha)


def hstep_defect_cases(defect):
    """The keys of HSTEP_CASES at which a defect changes a result (with tables for the table defects)."""
    keys = []
    for c in HSTEP_CASES:
        H, E, B, rps, Ts = k = hstep_key(c)
        if k in keys:
            continue
        if defect == "keys_of_row_n" and not (rps > 1 and B > 1):             # (one sentence, or one row per sentence: the same key)
            continue
        if defect == "mask_ignored_row" and not (B > 1 and Ts > 1):           # (no masked position otherwise)
            continue
        if defect == "cw_from_scores" and Ts == 1:                            # (one position: its numerator is 1, as its weight)
            continue
        keys.append(k)
    return keys


# ---------------------------------------------------------------------------------------------------------------- the head of a step
FORMS = ["plain", "hoisted_e", "hoisted_tables"]
HEAD_VS = [19, 2048, 2049, 10240, 10241]
# (N, E, H, V, form)
HEAD_STEP_CASES = [(5, 64, 32, V, f) for V in HEAD_VS for f in FORMS] + [(17, 256, 512, 2049, f) for f in FORMS] + \
                  [(256, 64, 32, 19, "plain"), (257, 64, 32, 19, "plain")]
HEAD_REJECTED = (257, 64, 32, 19)                 # the hoisted forms: -22, every output untouched
PARTS_CASES = [(97, 4096), (97, 4100), (192, 4097), (256, 4159)]
PARTS_NOT_TAKEN = [(96, 4100), (97, 4095)]
PARTS_E, PARTS_H = 256, 512
TIE_CASES = [(5, 64, 32, 19), (5, 64, 32, 2049), (5, 64, 32, 10241)]
HEAD_DEFECTS = ["cw_without_b2", "embw3_line_from_embp", "lse_without_max_shift_of_tail"]
PARTS_DEFECTS = ["parts_count_padding", "parts_merged_without_rescale"]


def ldl_of(V):
    return (V + 3) // 4 * 4


def tie_columns(V):
    """Columns made bit-equal and the row's maximum: two of one thread (j, j + 256), of two waves (j, j + 70), and -- streaming form --
    of two sweeps of 1024 float4 (j, j + 4096 + 4), also 1024 columns apart."""
    return [j for j in (3, 7, 3 + 70, 3 + 256, 3 + 1024, 3 + 4096 + 4) if j < V]


@functools.lru_cache(maxsize=None)
def head_inputs(N, E, H, V, ties=False):
    rs = _rs(34, N, E, H, V)
    C = 2 * H
    tok = rs.randint(1, V - 1, size=N).astype(np.int64)
    tok[0], tok[1], tok[N - 1] = 0, V - 1, 0
    out_w, out_b = _uni(rs, V, E, k=E ** -0.5), _uni(rs, V)
    out_b[V - 1] += np.float32(3.0)                                          # (module docstring: the streaming form's tail)
    if ties:
        cols = tie_columns(V)
        out_w[cols] = out_w[cols[0]]
        out_b[cols] = np.float32(2.0 * E ** 0.5 + 5.0)                       # |t . w| <= sum|w| <= sqrt(E): above every other logit
    return dict(h2=_uni(rs, N, H, k=0.5), c=_uni(rs, N, C, k=0.5), cw=_uni(rs, N, E, k=0.5), e=_uni(rs, N, E), tok=tok,
                embp=_uni(rs, V, 3 * H), embw3=_uni(rs, V, E, k=0.5),
                w=dict(w1=_uni(rs, E, H, k=H ** -0.5), b1=_uni(rs, E, k=H ** -0.5), w2=_uni(rs, E, C, k=C ** -0.5),
                       b2=_uni(rs, E, k=C ** -0.5), w3=_uni(rs, E, E, k=E ** -0.5), b3=_uni(rs, E, k=E ** -0.5), out_w=out_w, out_b=out_b))


def tables_flat(inp, H):
    """The tables buffer as the device lays it out: [embp (V,3H) | embw3 (V,E)], regions on multiples of 64 floats, gaps NaN."""
    V, E = inp["embw3"].shape
    off, total = tables_layout(V, E, H)
    flat = np.full(total, np.nan, dtype=np.float32)
    flat[:V * 3 * H] = inp["embp"].reshape(-1)
    flat[off:off + V * E] = inp["embw3"].reshape(-1)
    return flat


def head_step(A, h2, c_or_cw, e_or_line, w, hoisted, defect=None, rescales=0, streaming=False):
    """plain: tanh(W1 h2 + b1 + W2 c + b2 + W3 e + b3); hoisted: cw in place of W2 c (b2 kept), e_or_line the embedded token e (then
    W3 e is formed) or, 2-d and of width E with `hoisted == "tables"`, the line of embw3.  -> tmid, logits, lse, logp."""
    pre = A.add(A.ein("nh,eh->ne", h2, w["w1"]), w["b1"][None, :])
    if not hoisted:
        pre = A.add(pre, A.add(A.ein("nc,ec->ne", c_or_cw, w["w2"]), w["b2"][None, :]))
    else:
        if defect != "cw_without_b2":
            pre = A.add(pre, w["b2"][None, :])
        pre = A.add(pre, c_or_cw)
    if hoisted == "tables":
        pre = A.add(A.add(pre, w["b3"][None, :]), e_or_line)
    else:
        pre = A.add(pre, A.add(A.ein("nf,ef->ne", e_or_line, w["w3"]), w["b3"][None, :]))
    tmid = A.tanh(pre)
    logits = A.add(A.ein("ne,ve->nv", tmid, w["out_w"]), w["out_b"][None, :])
    if A is T:
        lse = T.logsumexp(logits, rescales)
    else:
        lse = F.logsumexp(logits, streaming, defect)
    V = np.shape(w["out_w"])[0]
    return dict(tmid=tmid, logits=logits, lse=lse, logp=A.sub(logits, A.expand(lse, -1, V)))


def head_form(A, inp, H, form, defect=None):
    """One of FORMS on head_inputs: what the three entry points are given."""
    V = inp["embw3"].shape[0]
    kw = dict(defect=defect, rescales=stream_rescales(V), streaming=V > 10240)
    if form == "plain":
        return head_step(A, inp["h2"], inp["c"], inp["e"], inp["w"], False, **kw)
    if form == "hoisted_e":
        return head_step(A, inp["h2"], inp["cw"], inp["e"], inp["w"], "e", **kw)
    E = inp["embw3"].shape[1]
    if defect == "embw3_line_from_embp":                                     # the line taken at region offset 0: a stretch of embp
        line = tables_flat(inp, H)[:V * E].reshape(V, E)[inp["tok"]]
    else:
        line = inp["embw3"][inp["tok"]]
    return head_step(A, inp["h2"], inp["cw"], line, inp["w"], "tables", **kw)


def head_defect_cases(defect):
    """(N, E, H, V, form) of HEAD_STEP_CASES at which a defect changes a result."""
    out = []
    for c in HEAD_STEP_CASES:
        N, E, H, V, form = c
        if defect == "cw_without_b2" and form == "plain":
            continue
        if defect == "embw3_line_from_embp" and form != "hoisted_tables":
            continue
        if defect == "lse_without_max_shift_of_tail" and V <= 10240:         # (the register forms have no running pair)
            continue
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- parts
def lse_from_parts(parts, defect=None):
    """parts (count, N, 2) of (m_i, s_i) -> lse (N) in float64: M = max_i m_i, lse = M + log sum_i s_i exp(m_i - M)."""
    parts = np.asarray(parts, dtype=np.float64)
    m, s = parts[..., 0], parts[..., 1]
    M = m.max(0)
    if defect == "parts_merged_without_rescale":
        return M + np.log(s.sum(0))
    return M + np.log((s * np.exp(m - M[None, :])).sum(0))


def parts_of(x, defect=None):
    """The fp32 pieces of rows x (N,V) in 64-column groups: (cdiv(V,64), N, 2)."""
    x = np.asarray(x, dtype=np.float32)
    N, V = x.shape
    cnt = (V + 63) // 64
    fill = np.float32(0.0) if defect == "parts_count_padding" else np.float32(-np.inf)      # (padding columns hold 0 and are summed)
    pad = np.full((N, cnt * 64), fill, dtype=np.float32)
    pad[:, :V] = x
    g = pad.reshape(N, cnt, 64)
    m = g.max(-1)
    s = np.exp(g - m[..., None], dtype=np.float32).sum(-1, dtype=np.float32)
    return np.ascontiguousarray(np.transpose(np.stack([m, s], -1), (1, 0, 2)))


def parts_sums_ref(x, m):
    """x (N,V): the device's own fp32 logits, exact; m (count,N): their group maxima -> tracked s (count,N) = sum_j exp(x_j - m_i) over
    the real columns of group i, with the two rescaling steps of the kernel's merge (module docstring: exp)."""
    x = np.asarray(x, dtype=np.float64)
    N, V = x.shape
    cnt = (V + 63) // 64
    on = np.zeros((N, cnt * 64), bool)
    on[:, :V] = True
    pad = np.zeros((N, cnt * 64))
    pad[:, :V] = x
    g, on = pad.reshape(N, cnt, 64), on.reshape(N, cnt, 64)
    mm = np.transpose(np.asarray(m, dtype=np.float64))[..., None]            # (N,cnt,1)
    d = np.where(on, mm - g, 0.0)
    t = T.exp(TV(-d, ULP * d))
    t = TV(np.where(on, t.v, 0.0), np.where(on, t.e + t.v * (d * RESCALE_SHIFT + PARTS_RESCALES * RESCALE_STEP), 0.0))
    s = T.sum(t, -1)
    return TV(s.v.T, s.e.T)


@functools.lru_cache(maxsize=None)
def parts_inputs(N, V):
    return head_inputs(N, PARTS_E, PARTS_H, V)
