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

The 2-byte storage mode (vag_set_operator_context(derived, 1)) -- `storage = 1` of bigru_fwd / bigru_bwd,
cgru_fwd / cgru_bwd and attn_keys_proj; tests/test_gpu_storage16.py holds the device to it, tests/test_storage16_ref_host.py the restatement.  h = 2^-11 is
the unit roundoff of fp16 (11 significand bits, round to nearest even), 2^-24 its subnormal spacing:

  f16       an fp16 store or operand: gemm_shared.h pack_f16 `(_Float16)a` (v_cvt, round to nearest even), gemm_epilogue16
            `ch[..] = (vag_half)v`, elem.hip jobs_kernel kinds 3 / 4 `dh[..] = (vag_half)v`.  On EXACT data (err = 0: the weights, the
            device's own stored keys) device and reference round the same fp32 number: the value becomes numpy.float16 of it, err
            stays 0.  On a tracked quantity the device rounds ITS fp32 number x', |x' - v| <= e: the rounding moves it by at most half
            an fp16 ulp of a number in [|v| - e, |v| + e], i.e. by h (|v| + e) where that is normal and by 2^-25 (half the subnormal
            spacing) below 2^-14 -- the value is kept, err = e + max(h (|v| + e), 2^-25).  F.f16 rounds with numpy.float16.
  f16(x, s) the scaled gradient operand: skinny.hip skinny_mma_h16 `pack_f16(x.x * a_scale, ..)` with a_scale = 4096 (gru_bwd_step_kernel)
            and `acc * inv` on the fp32 sum; persist.hip enc_bwd_wide16_kernel `st_sc1_h4(.., gh * GSCALE, ..)` and `acc * (1.f / GSCALE)`.
            s is a power of two, so x s and (sum) / s are exact and the rule is f16's on the scaled value:
            err = e + max(h (|v| + e), 2^-25 / s).
  products of fp16 operands
            an fp16 x fp16 product has 22 significand bits: exact in the fp32 accumulator of v_mfma_f32_16x16x32_f16.  What is left
            is the fp32 accumulation: `ein` under EPS on the rounded operands, as for every other product here.
  two-plane products (ein2p)
            gemm_shared.h split3 / sp_store<.., PL = 2>: x1 = bf16(x), x2 = bf16(x - x1), both round to nearest even, the subtraction
            exact in fp32.  bf16 keeps 8 significand bits: |x - x1| <= 2^-8 |x|, |x2| <= 2^-8 (1 + 2^-8) |x| and the dropped rest
            r = x - x1 - x2 has |r| <= 2^-8 |x - x1| <= 2^-16 |x| ("x = x1 + x2 exactly to 16 significand bits").  sp_compute<PL = 2>
            forms a1 b1 + a1 b2 + a2 b1 (each exact in fp32) and leaves a2 b2 out:
                a b - (a1 b1 + a1 b2 + a2 b1) = a2 b2 + ra b + a rb - ra rb,   |.| <= |a b| (2^-16 (1 + 2^-8)^2 + 2 * 2^-16 + 2^-32)
            which PL2_REL = 3 * 2^-16 + 2^-22 covers; it multiplies the magnitudes the device splits, (|a| + ea)(|b| + eb), and comes
            on top of ein's own terms (the fp32 accumulation of the three products is of ein's kind).  F.ein2p performs the split.
  which product takes the planes
            gemm.hip gemm_product / gemm_plan_single with VagCallCtx::gemm_planes = 2: a product queued into an open group bracket
            (`bracket && .. M > 64 && N > 64 && K >= 256`, two or more of one layout) runs on the 128 x 128 plane kernel; every other one is
            planned alone: `t == 128 && (M <= 64 || N <= 64)` is never tried, so those run on the exact f32-input 64 x 64 kernel, and above
            that the cost model decides.  plan16_tile restates that cost model; both new test files assert, product by product
            (PRODUCTS16, filled by the reference as it runs), that the host-only vag_gemm_plan picks the same family.
  range     nothing a kernel rounds to fp16 may leave fp16's finite range (65504; gate gradients times 2^12 likewise).  T.f16 keeps the
            largest (|v| + e) s it has seen in F16_PEAK; the host test resets and reads it per case.  The gradient inputs of the mode's
            cases (d_enc and the accumulators' starting values) are scaled by GRAD16 = 2^-18: gate gradients of a trained model are that
            small -- it is why the kernels scale them -- and only then does an unscaled fp16 rounding (defect grad_scale_missing) land in
            fp16's subnormal range and leave the bound.
  backward from the saved workspace
            The mode's forward bound is 2^-11-grade, and a backward recomputed from it inherits that: at H = 1024 a dropped K segment of
            the BACKWARD product stays inside such a bound (0.6 of it at (1024, 130, 3)).  So the mode's backward is held to
            bigru_bwd(fwd = bigru_saved(gates, hst)): the gates and states the forward of the same call left in the workspace
            (seq_layout.h: BiGruWs, offsets pinned by tests/golden/ws_layout.json) enter as exact data, and the bound that remains is
            the backward kernels' own -- every catalogue defect leaves it at every case.  The saved gates and states themselves are
            held, element by element, to bigru_fwd's tracked steps: a wrong saved gate cannot hide behind a right output.
            The decoder the same way: cgru_bwd(fwd = cgru_saved(h2_all, workspace)) with g1, g2, h1, alpha, q, uk and the stored
            fp16 encwp as exact data, each of them held to the one-step forward reference (cgru_ws_saved).  Its backward still
            puts three fp16-operand products in a row per step, so its cases keep the lengths at which every defect leaves the
            bound (DEC16_BWD_CASES).
Where the kernels round: the recurrent weights once (vag_derive_weights(with_fp16 = 1): w16); the state as it enters the recurrent
product, the blend z h reading the fp32 state (gru_step_kernel: `hp[q] = sd.hprev[..]` beside skinny_mma_h16 on sd.A); the gate
gradients as they enter dgh W_hh (f16(x, 2^12)); the keys as stored (gemm_epilogue16).  The wide one-launch encoder kernels exchange
exactly these rounded operands (enc_fwd_wide16_kernel: `st_sc1_h4(hx + .., ho..)`, "what an fp16-operand product would round it to
anyway") and keep the carried state, the saved gates and the outputs in fp32, so chain and one launch share ONE reference.

The case tables of tests/test_gpu_recurrences.py and tests/test_gpu_storage16.py, the input generators and the defect catalogue live
here, so that tests/test_recur_ref_host.py and tests/test_storage16_ref_host.py check the bounds at exactly the shapes and inputs the
device is tested at."""
import collections
import functools

import numpy as np

from ground_ref import TV, Tr, F32, ratio, gamma, U24, ULP, EPS, TANH_ABS, RCP_REL, _rs, _f32   # noqa: F401 (re-exported)


# ---------------------------------------------------------------------------------------------------------------- the two arithmetics
UNIT_CAP = 1.0 + 2.0 ** -20        # (module docstring: range caps)
F16_MAX = 65504.0                  # (module docstring: the 2-byte storage mode)
F16_REL = 2.0 ** -11
F16_SUB = 2.0 ** -25
GSCALE = 4096.0
PL2_REL = 3.0 * 2.0 ** -16 + 2.0 ** -22
GRAD16 = 2.0 ** -18
F16_PEAK = [0.0]                   # largest (|v| + e) * scale that T.f16 has rounded since the last reset


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
    def f16(a, scale=1.0):
        """An fp16 store or operand, of a * scale for a power of two `scale` (module docstring: f16, f16(x, s))."""
        a = Tr.lift(a)
        wide = np.abs(a.v) + a.e
        if wide.size:
            F16_PEAK[0] = max(F16_PEAK[0], float(wide.max()) * scale)
        with np.errstate(over="ignore"):
            r = (a.v * scale).astype(np.float16).astype(np.float64) / scale
        exact = a.e == 0
        return TV(np.where(exact, r, a.v), np.where(exact, 0.0, a.e + np.maximum(F16_REL * wide, F16_SUB / scale)))

    @staticmethod
    def ein2p(spec, a, b):
        """A product on two bf16 planes per operand (module docstring: two-plane products)."""
        a, b = Tr.lift(a), Tr.lift(b)
        r = T.ein(spec, a, b)
        return TV(r.v, r.e + PL2_REL * np.einsum(spec, np.abs(a.v) + a.e, np.abs(b.v) + b.e, optimize=True))

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
    def f16(a, scale=1.0):
        with np.errstate(over="ignore"):
            return ((F32.lift(a) * np.float32(scale)).astype(np.float16).astype(np.float32) / np.float32(scale)).astype(np.float32)

    @staticmethod
    def ein2p(spec, a, b):
        """gemm_shared.h split3 with two planes kept, then sp_compute<2>: smallest terms first, all in fp32."""
        a1, a2 = _bf16_planes(F32.lift(a))
        b1, b2 = _bf16_planes(F32.lift(b))
        return ((F.ein(spec, a1, b2) + F.ein(spec, a2, b1)).astype(np.float32) + F.ein(spec, a1, b1)).astype(np.float32)

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


# ---------------------------------------------------------------------------------------------------------------- 2-byte storage mode
def _bf16(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32: gemm_shared.h pack_bf16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def _bf16_planes(x):
    x1 = _bf16(x)
    return x1, _bf16((x - x1).astype(np.float32))


def w16(w):
    """A weight as the derived buffer holds it in the mode: rounded to fp16 once (vag_derive_weights(with_fp16 = 1)); exact data."""
    return np.asarray(w, dtype=np.float32).astype(np.float16).astype(np.float32)


def _cdiv(a, b):
    return -(-a // b)


def plan16_tile(M, N, K, beta=0.0, c_half=False):
    """gemm.hip gemm_plan_single's tile choice restated, for planes = 2 and the default options (no slabs, no force hook, bf16 MFMA):
    64 -> the exact f32-input kernel, 128 -> the plane kernel.  act = none."""
    can_split = beta in (0.0, 1.0) and not c_half
    best, tile = 1e30, 64
    for t in (64, 128):
        if t == 128 and (M <= 64 or N <= 64):
            continue
        eff = 0.64 if t == 128 else 0.42
        base = _cdiv(M, t) * _cdiv(N, t)
        sp = 1
        while sp <= 64:
            if sp > 1 and (not can_split or K // sp < 128):
                break
            kper = _cdiv(_cdiv(K, sp), 32) * 32
            blocks = base * sp
            if t == 128:
                full, rem = divmod(blocks, 512)
                rounds = 1.5 * float(full) + (0.0 if rem == 0 else (1.0 if rem <= 256 else 1.5))
            else:
                rounds = float(_cdiv(blocks, 256))
            t_mfma = rounds * float(kper) * float(t * t) * 2.0 / (256.0 * eff) / 2400.0
            nbytes = float(M) * float(N) * 4.0
            if sp > 1:
                t_out = sp * nbytes / 3.0e6 + (nbytes / 4.0e6 + 2.0 if beta == 0.0 else 0.0)
            else:
                t_out = nbytes * (2.0 if beta != 0.0 else 1.0) / 4.0e6
            if t_mfma + t_out < best:
                best, tile = t_mfma + t_out, t
            sp += 1 if sp < 16 else 4 if sp < 32 else 8
    return tile


PRODUCTS16 = set()                 # (M, N, K, beta, c_half) of every product the mode's references planned alone, and the tile


def family16(M, N, K, beta=0.0, c_half=False, bracket=False):
    """"planes" or "exact" for a dense product of the mode (module docstring: which product takes the planes).  bracket: the call
    site holds an open group bracket AND queues a second product of the same layout (both encoder directions)."""
    if bracket and M > 64 and N > 64 and K >= 256 and beta in (0.0, 1.0):
        return "planes"
    t = plan16_tile(M, N, K, beta, c_half)
    PRODUCTS16.add((M, N, K, float(beta), int(c_half), t))
    return "planes" if t == 128 else "exact"


def _prod(A, spec, a, b, fam=None):
    return A.ein2p(spec, a, b) if fam == "planes" else A.ein(spec, a, b)


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
CELL16_DEFECTS = CELL_DEFECTS + ["k_tail_segment_dropped"]


def gru_cell_fwd(A, gi, h, w_hh, b_hh, defect=None, h_op=None):
    """-> h' (M,H), save = [r, z, n, W_hn h + b_hn].  h_op: the state as the recurrent product reads it (2-byte storage mode: rounded
    to fp16; the blend reads h itself)."""
    H = np.shape(w_hh)[1]
    if defect == "k_tail_segment_dropped":                                    # the last 8-wide K segment is not summed
        gh = A.ein("mk,gk->mg", (h if h_op is None else h_op)[:, :H - 8], w_hh[:, :H - 8])
    else:
        gh = A.ein("mk,gk->mg", h if h_op is None else h_op, w_hh)
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


def bigru_fwd(A, inp, defect=None, storage=0):
    """-> enc (B,Ts,2H), mask (B,Ts) and, for the backward and the input conditions, x, the states and the gates per direction.
    storage = 1: the 2-byte storage mode (module docstring), launch chain and wide one-launch kernel alike."""
    src, lens = inp["src"], inp["lens"].copy()
    B, Ts = src.shape
    H = inp["fw"][1].shape[1]
    E = inp["emb"].shape[1]
    if defect == "tile2_takes_len_of_row15" and B > 16:
        lens[16:] = lens[15]
    if defect == "group_tail_takes_len_of_row63" and B > 64:                   # the wide kernels' last 64-row group
        lens[64:] = lens[63]
    x = A.lift(inp["emb"][src])                                              # (B,Ts,E): a gather, exact
    if inp["p_emb"] > 0:
        x = A.mul(x, np.transpose(inp["m_emb"], (1, 0, 2)))
    sides, saved = [], []
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate((inp["fw"], inp["bw"])):
        if storage:
            xp = A.add(_prod(A, "bte,ge->btg", x, w_ih, family16(Ts * B, 3 * H, E)), b_ih[None, None, :])
            w_hh = w16(w_hh)
        else:
            xp = A.add(A.ein("bte,ge->btg", x, w_ih), b_ih[None, None, :])
        h = _zeros(A, (B, H))
        outs, steps = [None] * Ts, []
        for t in (range(Ts) if d == 0 else range(Ts - 1, -1, -1)):
            live = (t < lens)[:, None]
            run = np.ones_like(live) if (defect == "rev_runs_over_padding" and d == 1) else live
            if storage:
                hn, save = gru_cell_fwd(A, xp[:, t], h, w_hh, b_hh, defect if defect in CELL16_DEFECTS else None, h_op=A.f16(h))
            else:
                hn, save = gru_cell_fwd(A, xp[:, t], h, w_hh, b_hh, defect if defect in CELL_DEFECTS else None)
            steps.append(dict(t=t, h_prev=h, save=save, live=live))
            h = A.where(run, hn, h)
            steps[-1]["h_next"] = h
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


def bigru_saved(A, inp, gates, hst):
    """The forward's workspace as the backward of the SAME call reads it (seq_layout.h: BiGruWs): gates [2][Ts][r,z,n,hn][B][H] and
    hst [2][Ts + 1][B][H] in processing order, fp32 arrays that enter exactly -- the `fwd` argument of bigru_bwd whose bounds then hold
    the backward kernels alone, sharp at every step (the forward's own error is held by bigru_fwd's bounds on enc, gates and hst)."""
    src, lens = inp["src"], inp["lens"]
    B, Ts = src.shape
    x = A.lift(inp["emb"][src])
    if inp["p_emb"] > 0:
        x = A.mul(x, np.transpose(inp["m_emb"], (1, 0, 2)))
    saved = []
    for d in range(2):
        steps = []
        for k in range(Ts):
            t = k if d == 0 else Ts - 1 - k
            steps.append(dict(t=t, h_prev=A.lift(hst[d, k]), save=[A.lift(gates[d, k, g]) for g in range(4)], live=(t < lens)[:, None]))
        saved.append(steps)
    return dict(x=x, steps=saved)


def bigru_ws_arrays(A, fwd):
    """(gates, hst) of a forward in arithmetic A, in the workspace's layout (T: as tracked arrays)."""
    gates = A.stack([A.stack([A.stack(st["save"], 0) for st in steps], 0) for steps in fwd["steps"]], 0)
    hst = A.stack([A.stack([st["h_prev"] for st in steps] + [steps[-1]["h_next"]], 0) for steps in fwd["steps"]], 0)
    return gates, hst


def bigru_bwd(A, inp, fwd, defect=None, storage=0):
    """fwd: bigru_fwd(A, inp) -- the workspace, recomputed.  -> g_emb and the four gradients of each direction, accumulated.
    storage = 1: fwd from bigru_fwd(.., storage = 1); the gate gradients enter dgh W_hh as fp16 x 2^12 against the fp16 W_hh^T."""
    src, lens = inp["src"], inp["lens"]
    B, Ts = src.shape
    H = inp["fw"][1].shape[1]
    E, R = inp["emb"].shape[1], B * Ts
    dE = A.lift(inp["d_enc"])
    if inp["p_ctx"] > 0:
        dE = A.mul(dE, inp["m_ctx"])
    out, dx = {}, None
    for d, name in enumerate(("fw", "bw")):
        w_ih, w_hh, b_ih, b_hh = inp[name]
        if storage:
            w_hh = w16(w_hh)
            if defect == "fp16_copy_transposed_wrong":                         # encT16 (H,3H) read where enc16 (3H,H) lies
                w_hh = np.ascontiguousarray(w_hh.reshape(H, 3 * H).T)
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
            if storage:
                g16 = A.f16(dgh) if defect == "grad_scale_missing" else A.f16(dgh, GSCALE)
                if defect == "k_tail_segment_dropped":
                    nxt = A.add(A.ein("bg,gh->bh", g16[:, :3 * H - 8], w_hh[:3 * H - 8]), carry)
                else:
                    nxt = A.add(A.ein("bg,gh->bh", g16, w_hh), carry)
            else:
                nxt = A.add(A.ein("bg,gh->bh", dgh, w_hh), carry)
            z3 = np.zeros((B, 3 * H))
            dgis[t] = dgi if defect == "pad_step_into_dxp" else A.where(live, dgi, z3)
            dghs.append(A.where(live, dgh, z3))
            hps.append(st["h_prev"])
            dh = A.where(live, nxt, dh)
        dgi_all, dgh_all, hp_all = A.stack(dgis, 1), A.stack(dghs, 1), A.stack(hps, 1)
        g0 = inp["g_" + name + "0"]
        acc = (lambda g, v: v) if defect == "g_overwritten" and d == 1 else (lambda g, v: A.add(g, v))
        f_ih = family16(3 * H, E, R, 1.0, bracket=True) if storage else None   # (enc_api.hip: grp1 holds both directions' products)
        f_hh = family16(3 * H, H, R, 1.0, bracket=True) if storage else None
        out["g_%s_w_ih" % name] = A.add(g0[0], _prod(A, "btg,bte->ge", dgi_all, fwd["x"], f_ih))
        out["g_%s_w_hh" % name] = acc(g0[1], _prod(A, "btg,bth->gh", dgh_all, hp_all, f_hh))
        out["g_%s_b_ih" % name] = A.add(g0[2], A.sum(A.sum(dgi_all, 1), 0))
        out["g_%s_b_hh" % name] = A.add(g0[3], A.sum(A.sum(dgh_all, 1), 0))
        part = _prod(A, "btg,ge->bte", dgi_all, w_ih, family16(R, E, 3 * H, 1.0, bracket=True) if storage else None)
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


def cgru_fwd(A, inp, h2_given=None, defect=None, storage=0):
    """-> h2_all (Tt,B,H), c_all (Tt,B,C), e_all (Tt,B,E) and the per-step workspace.  h2_given: fp32 (Tt,B,H), the states the
    recomputation of each step starts from (the backward's argument h2_all, exact).
    storage = 1 (teacher forced; the launch chain is the only path): inp["pe"] holds the fp16 keys vag_attn_keys_proj stored in the
    mode, as exact data; W_hh1, attn_h and W_hh2 are rounded once; hprev and h1 are rounded as they enter W_hh1 hprev, attn_h h1 and
    W_hh2 h1 (skinny.hip: gru_step_kernel<.., true>, skinny_plain_kernel<W, true>, the side product of attn_dot_side*_kernel<0, .., true>);
    encwp is rounded as gemm_epilogue16 stores it (dec_api.hip dec_project_keys: c_half = d.s16) and read back by attn_ctx_gru_kernel<true>."""
    w, tok = inp["w"], inp["tok"]
    Tt = tok.shape[0] - 1
    B, Ts, C = inp["enc"].shape
    H, E = C // 2, inp["emb"].shape[1]
    cd = defect if defect in (CELL16_DEFECTS if storage else CELL_DEFECTS) else None
    e_all = inp["emb"][tok[:Tt]]                                             # a gather: exact
    pe = inp["pe"]
    if storage:
        # (dec_api.hip: xp1 and uk share a bracket but only uk can be queued, alone: both are planned alone; encwp has its own bracket)
        xp1 = A.add(_prod(A, "tbe,ge->tbg", e_all, w["w_ih1"], family16(Tt * B, 3 * H, E)), w["b_ih1"][None, None, :])
        uk = _prod(A, "bsc,hc->bsh", inp["enc"], w["c2h"], family16(B * Ts, H, C))
        encwp = A.f16(_prod(A, "bsh,gh->bsg", uk, w["w_ih2"], family16(B * Ts, 3 * H, H, 0.0, True)))
        w = dict(w, w_hh1=w16(w["w_hh1"]), attn_h=w16(w["attn_h"]), w_hh2=w16(w["w_hh2"]))
        op = A.f16
        if defect == "keys_row_shifted":                                     # fp16 pe and encwp read one source position late
            late = np.minimum(np.arange(Ts) + 1, Ts - 1)
            pe, encwp = pe[:, late], encwp[:, late]
    else:
        xp1 = A.add(A.ein("tbe,ge->tbg", e_all, w["w_ih1"]), w["b_ih1"][None, None, :])
        uk = A.ein("bsc,hc->bsh", inp["enc"], w["c2h"])                       # context2hid on the keys, then W_ih2 on the result
        encwp = A.ein("bsh,gh->bsg", uk, w["w_ih2"])
        op = lambda x: x
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
        h1, s1 = gru_cell_fwd(A, xp1[t], hprev, w["w_hh1"], w["b_hh1"], cd, h_op=op(hprev))
        h1 = A.mark(h1)
        q = A.ein("bh,ch->bc", op(hprev if defect == "query_from_h2_prev" else h1), w["attn_h"])
        sc, th = attn_scores(A, pe, q, w["attn_v"])
        alpha = A.softmax(sc, mask)
        gi2 = A.add(A.ein("bs,bsg->bg", alpha, encwp), w["b_ih2"][None, :])
        hside = hprev if defect == "gru2_blends_h2_prev" else h1
        h2, s2 = gru_cell_fwd(A, gi2, hside, w["w_hh2"], w["b_hh2"], cd, h_op=op(hside))
        h2 = A.mark(h2)
        c = A.ein("bs,bsc->bc", alpha, inp["enc"])
        steps.append(dict(hprev=hprev, h1=h1, s1=s1, s2=s2, th=th, alpha=alpha, scores=sc, q=q))
        h2s.append(h2)
        cs.append(c)
    return dict(h2_all=A.stack(h2s, 0), c_all=A.stack(cs, 0), e_all=e_all, steps=steps, uk=uk, encwp=encwp)


DEC_WS = ["ws_alpha", "ws_h1", "ws_q"]


def cgru_ws_arrays(A, fwd):
    """What the forward leaves in its workspace per step, as vag_cgru_ws_offset names it: alpha (Tt,B,Ts), h1 (Tt,B,H) and the q half
    of [q | W_hh2 h1 + b] (Tt,B,C).  The mode's device test holds them to the one-step reference beside h2_all and c_all: a query
    formed from the wrong state moves alpha by less than the mode's worst-case softmax bound, but never q itself."""
    st = fwd["steps"]
    return dict(ws_alpha=A.stack([x["alpha"] for x in st], 0), ws_h1=A.stack([x["h1"] for x in st], 0), ws_q=A.stack([x["q"] for x in st], 0))


def cgru_saved(A, inp, h2_all, ws):
    """The forward's workspace as the backward of the same call reads it (seq_layout.h: CgruWs), as exact data: ws = dict(g1, g2
    (Tt,4,B,H), h1 (Tt,B,H), alpha (Tt,B,Ts), q (Tt,B,C), uk (B,Ts,H), encwp (B,Ts,3H)) -- the `fwd` argument of cgru_bwd whose bounds
    then hold the backward kernels alone.  th = tanh(pe + q) is recomputed (attn_dq_kernel and attn_post_bwd_kernel do) and tracked."""
    Tt, B, Ts = ws["alpha"].shape
    steps = []
    for t in range(Tt):
        q = A.lift(ws["q"][t])
        th = A.tanh(A.add(inp["pe"], A.expand(q, 1, Ts)))
        steps.append(dict(hprev=A.lift(inp["h0"] if t == 0 else h2_all[t - 1]), h1=A.lift(ws["h1"][t]), s1=[A.lift(ws["g1"][t, g]) for g in range(4)],
                          s2=[A.lift(ws["g2"][t, g]) for g in range(4)], th=th, alpha=A.lift(ws["alpha"][t]), q=q))
    return dict(steps=steps, uk=A.lift(ws["uk"]), encwp=A.lift(ws["encwp"]))


def cgru_ws_saved(A, fwd):
    """The same dict from a forward in arithmetic A (the host test: from the restatement's own forward)."""
    st = fwd["steps"]
    stk = lambda f: A.stack([f(x) for x in st], 0)
    return dict(g1=stk(lambda x: A.stack(x["s1"], 0)), g2=stk(lambda x: A.stack(x["s2"], 0)), h1=stk(lambda x: x["h1"]),
                alpha=stk(lambda x: x["alpha"]), q=stk(lambda x: x["q"]), uk=fwd["uk"], encwp=fwd["encwp"])


def cgru_bwd(A, inp, fwd, c_all, e_all, acc=0, with_d_e=True, defect=None, storage=0):
    """fwd: cgru_fwd(A, inp, h2_given = the device's h2_all) -- the workspace, recomputed; c_all, e_all: the forward's fp32 outputs, exact.
    -> d_enc_out, d_pe, d_h0 and the twelve accumulated parameter gradients g_*.
    storage = 1 (fwd: cgru_saved of the mode's forward): dgh2, dq and dgh1 enter dgh2 W_hh2, dq attn_h and dgh1 W_hh1 as fp16 x 2^12
    against the fp16 transposes (skinny.hip vag_attn_dot_side_launch `a.a_scale = mode == 1 ? 4096.f : 1.f`, gru_bwd_step_kernel);
    everything else the backward does in the mode is fp32 arithmetic on the stored fp16 keys."""
    w, tok = inp["w"], inp["tok"]
    Tt = tok.shape[0] - 1
    B, Ts, C = inp["enc"].shape
    H = C // 2
    R_, E_ = Tt * B, inp["emb"].shape[1]
    if storage:
        w = dict(w, w_hh1=w16(w["w_hh1"]), attn_h=w16(w["attn_h"]), w_hh2=w16(w["w_hh2"]))
        if defect == "fp16_copy_transposed_wrong":                             # whh1T16 (H,3H) read where whh1_16 (3H,H) lies
            w["w_hh1"] = np.ascontiguousarray(w["w_hh1"].reshape(H, 3 * H).T)
        gop = (lambda x: A.f16(x)) if defect == "grad_scale_missing" else (lambda x: A.f16(x, GSCALE))
        fam = lambda M, N, K, beta, bracket=False: family16(M, N, K, beta, False, bracket)
        kcut = 8 if defect == "k_tail_segment_dropped" else 0
    else:
        gop = lambda x: x
        fam = lambda *a, **k: None
        kcut = 0
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
        if kcut:
            dh1 = A.add(A.add(A.ein("bc,ch->bh", gop(dq)[:, :C - kcut], w["attn_h"][:C - kcut]),
                              A.ein("bg,gh->bh", gop(dgh2)[:, :3 * H - kcut], w["w_hh2"][:3 * H - kcut])), carry2)
        else:
            dh1 = A.add(A.add(A.ein("bc,ch->bh", gop(dq), w["attn_h"]), A.ein("bg,gh->bh", gop(dgh2), w["w_hh2"])), carry2)
        dgi1, dgh1, carry1 = gru_cell_grads(A, dh1, st["s1"], st["hprev"])
        if defect == "carry_dropped_at_step" and t == Tt // 2:
            carry1 = _zeros(A, (B, H))
        if defect == "d_h0_without_carry" and t == 0:
            carry1 = _zeros(A, (B, H))
        carry_in = A.add(A.ein("bg,gh->bh", gop(dgh1)[:, :3 * H - kcut], w["w_hh1"][:3 * H - kcut]), carry1) if kcut else \
            A.add(A.ein("bg,gh->bh", gop(dgh1), w["w_hh1"]), carry1)
        for k, x in (("dgi1", dgi1), ("dgh1", dgh1), ("dgi2", dgi2), ("dgh2", dgh2), ("dq", dq), ("ds", ds)):
            per[k][t] = x
    S = {k: A.stack(x, 0) for k, x in per.items()}
    alpha_all = A.stack([st["alpha"] for st in fwd["steps"]], 0)               # (Tt,B,Ts)
    h1_all = A.stack([st["h1"] for st in fwd["steps"]], 0)
    hp_all = A.stack([st["hprev"] for st in fwd["steps"]], 0)
    du = _prod(A, "tbg,gh->tbh", S["dgi2"], w["w_ih2"], fam(R_, H, 3 * H, 0.0))
    d_enc = A.add(A.ein("tbs,tbc->bsc", alpha_all, inp["d_c"]),
                  _prod(A, "bsh,hc->bsc", A.ein("tbs,tbh->bsh", alpha_all, du), w["c2h"], fam(B * Ts, C, H, 1.0)))
    if acc and defect != "accumulate_enc_ignored":
        d_enc = A.add(inp["d_enc0"], d_enc)
    u_all = A.ein("tbs,bsh->tbh", alpha_all, fwd["uk"])
    g0 = inp["g0"]
    tsum = lambda x: A.sum(A.sum(x, 0), 0)
    out = dict(d_enc_out=d_enc, d_pe=d_pe, d_h0=carry_in)
    # (dec_api.hip: the weight gradients share the bracket grp3; g_w_hh1 goes out as two products over B and (Tt - 1) B rows, held to
    # the looser rule of the two)
    f_hh1 = "planes" if storage and "planes" in (fam(3 * H, H, B, 1.0, True), fam(3 * H, H, max(R_ - B, 1), 1.0, True)) else None
    out["g_w_hh2"] = A.add(g0["w_hh2"], _prod(A, "tbg,tbh->gh", S["dgh2"], h1_all, fam(3 * H, H, R_, 1.0, True)))
    out["g_b_hh2"] = A.add(g0["b_hh2"], tsum(S["dgh2"]))
    out["g_attn_h"] = A.add(g0["attn_h"], _prod(A, "tbc,tbh->ch", S["dq"], h1_all, fam(C, H, R_, 1.0, True)))
    out["g_attn_v"] = A.add(g0["attn_v"], g_v)
    out["g_w_ih2"] = A.add(g0["w_ih2"], _prod(A, "tbg,tbh->gh", S["dgi2"], u_all, fam(3 * H, H, R_, 1.0, True)))
    out["g_b_ih2"] = A.add(g0["b_ih2"], tsum(S["dgi2"]))
    out["g_c2h"] = A.add(g0["c2h"], _prod(A, "tbh,tbc->hc", du, c_all, fam(H, C, R_, 1.0, True)))
    prod = _prod(A, "tbg,tbh->gh", S["dgh1"], hp_all, f_hh1)
    out["g_w_hh1"] = prod if defect == "g_overwritten" else A.add(g0["w_hh1"], prod)
    out["g_b_hh1"] = A.add(g0["b_hh1"], tsum(S["dgh1"]))
    out["g_w_ih1"] = A.add(g0["w_ih1"], _prod(A, "tbg,tbe->ge", S["dgi1"], e_all, fam(3 * H, E_, R_, 1.0, True)))
    out["g_b_ih1"] = A.add(g0["b_ih1"], tsum(S["dgi1"]))
    de = _prod(A, "tbg,ge->tbe", S["dgi1"], w["w_ih1"], fam(R_, E_, 3 * H, 1.0 if with_d_e else 0.0, True))
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


# ---------------------------------------------------------------------------------------------------------------- 2-byte storage mode: cases
# (H, E, B, Ts): launch chain with persistent = 0 unless one_launch; branch sentences quoted in tests/test_gpu_storage16.py
ENC16_CASES = [
    _enc(40, 16, 5, 4, 0, "gru_step_kernel<4, true>, K = 40: one full and one 8-wide K segment; backward K = 120"),
    _enc(256, 64, 17, 5, 0, "gru_step_kernel<4, true> at the K = 256 edge, second 16-row tile of one row; backward K = 768"),
    _enc(512, 64, 20, 3, 0, "gru_step_small_kernel<8, 8, true>; backward K = 1536"),
    _enc(512, 64, 96, 3, 0, "gru_step_kernel<8, true>"),
    _enc(512, 64, 130, 3, 0, "gru_step_kernel<8, true, 2>, last 32-row tile of 2 rows; backward K = 1536, 16 x 16 tiles"),
    _enc(1024, 64, 130, 3, 1, "wide fp16 forward in one launch; backward chain gru_bwd_step_kernel<16, 4, true, 2, 2>",
         opt="persistent_enc_bwd"),
    _enc(512, 64, 64, 3, 1, "enc_fwd_wide16_kernel<4> / enc_bwd_wide16_kernel<6>, one full 64-row group"),
    _enc(512, 64, 70, 3, 1, "the same, second 64-row group of 6 rows"),
    _enc(1024, 64, 64, 3, 1, "enc_fwd_wide16_kernel<8> / enc_bwd_wide16_kernel<12>"),
    _enc(512, 64, 64, 3, 0, "the launch chain under the one-launch case's reference"),
    _enc(256, 64, 17, 5, 0, "chain with p_emb = 0.3, p_ctx = 0.5", p=(0.3, 0.5)),
]
ENC16_FWD_DEFECTS = ENC_FWD_DEFECTS + ["k_tail_segment_dropped", "group_tail_takes_len_of_row63"]
ENC16_BWD_DEFECTS = ENC_BWD_DEFECTS + ["k_tail_segment_dropped", "grad_scale_missing", "fp16_copy_transposed_wrong"]


@functools.lru_cache(maxsize=None)
def enc16_inputs(H, E, B, Ts, p_emb=0.0, p_ctx=0.0, full=False):
    """enc_inputs with the gradient side scaled by GRAD16 (a power of two: exact; module docstring: range)."""
    d = dict(enc_inputs(H, E, B, Ts, p_emb, p_ctx, full))
    d["d_enc"] = _f32(d["d_enc"] * GRAD16)
    d["g_emb0"] = _f32(d["g_emb0"] * GRAD16)
    for k in ("g_fw0", "g_bw0"):
        d[k] = [_f32(g * GRAD16) for g in d[k]]
    return d


def enc16_defect_cases(defect):
    keys = []
    for c in ENC16_CASES:
        k = enc_key(c)
        if k in keys:
            continue
        ragged = c.B > 1 and c.Ts > 1 and not c.full
        if defect in ("rev_runs_over_padding", "enc_pad_holds_state", "pad_step_into_dxp") and not ragged:
            continue
        if defect == "tile2_takes_len_of_row15" and not (c.B > 16 and ragged):
            continue
        if defect == "group_tail_takes_len_of_row63" and not (c.B > 64 and ragged):
            continue
        if defect == "ctx_mask_indexed_TsB" and not (c.p_ctx > 0):
            continue
        keys.append(k)
    return keys


# vag_attn_keys_proj in the mode: rows x C.  The first four are the issue's; gemm_plan_single sends all four to the exact 64 x 64 kernel
# (at 200 x 1024 its cost model prices 4 x 16 small tiles at 32 us against 2 x 8 plane tiles at 85 us), so the plane kernel's fp16
# epilogue is reached by the fifth: 33 x 4 plane tiles in one round against 66 x 8 = 528 small ones in three, last row tile of 104 rows.
KEYS16_CASES = [(48, 64), (35, 512), (130, 512), (200, 1024), (4200, 512)]
KEYS16_DEFECTS = ["keys_row_shifted", "k_tail_segment_dropped"]


@functools.lru_cache(maxsize=None)
def keys16_inputs(rows, C):
    rs = _rs(27, rows, C)
    return dict(enc=_uni(rs, rows, C, k=0.5), attn_e=_uni(rs, C, C, k=C ** -0.5))


def attn_keys_proj(A, inp, storage=0, defect=None):
    """vag_attn_keys_proj: pe (rows,C) = enc attn_e^T (NMT_Decoder.py:47 hoisted).  storage = 1: the product by its family, then the
    fp16 store of gemm_epilogue16 (the device test decodes the halves; on a tracked value f16 keeps the value and widens the bound)."""
    enc, w = inp["enc"], inp["attn_e"]
    rows, C = enc.shape
    if defect == "k_tail_segment_dropped":
        enc, w = enc[:, :C - 8], w[:, :C - 8]
    pe = _prod(A, "rc,dc->rd", enc, w, family16(rows, C, C, 0.0, True) if storage else None)
    if storage:
        pe = A.f16(pe)
    if defect == "keys_row_shifted":                                          # every row read one source position late
        idx = np.minimum(np.arange(rows) + 1, rows - 1)
        pe = pe[idx]
    return dict(pe=pe)


# The decoder's forward in the mode: (H, E, B, Ts, Tt), launch chain (`hoist && !d.s16 && ..` keeps the one-launch kernel out).
Dec16Case = collections.namedtuple("Dec16Case", "H E B Ts Tt branch")
DEC16_CASES = [
    Dec16Case(40, 16, 5, 9, 3, "generic attn_dot_side_kernel<0, 8, true> (W = 80), gru_step_kernel<4, true>, K = 40"),
    Dec16Case(256, 64, 17, 9, 3, "generic kernel at C = 512: d.gx = cdiv64(9, 8) = 2 ragged score blocks; second row tile of one row"),
    Dec16Case(512, 64, 5, 33, 3, "attn_dot_side_reg_kernel<0, 8, true, 2, false>: gx = min(cdiv64(512, 5), 33 / 16) = 2, second block ragged"),
    Dec16Case(512, 64, 130, 9, 2, "attn_dot_side_reg_kernel<0, 8, true, 2, true>: wide side product on 32 x 64 tiles"),
    Dec16Case(1024, 64, 16, 9, 1, "NJ = 4"),
    Dec16Case(512, 64, 20, 17, 8, "eight steps, held to the one-step reference from the device's own h2_all"),
]
DEC16_FWD_DEFECTS = DEC_FWD_DEFECTS + ["k_tail_segment_dropped", "keys_row_shifted"]
DEC16_BWD_DEFECTS = DEC_BWD_DEFECTS + ["k_tail_segment_dropped", "grad_scale_missing", "fp16_copy_transposed_wrong"]
# The backward carries its gradient through three fp16-operand products per step, so even from the saved workspace its worst-case
# bound grows with the steps: at (256, .., Tt = 3) and (512, .., Tt = 3) d_h0_without_carry stays inside (0.25, 0.03 of the bound).
# Its cases are therefore the forward's short shapes at the lengths at which every catalogue defect leaves the bound.
Dec16Bwd = collections.namedtuple("Dec16Bwd", "H E B Ts Tt acc d_e two_phase branch")
DEC16_BWD_CASES = [
    Dec16Bwd(40, 16, 5, 9, 3, 1, True, False, "W = 3H = 120: attn_dot_side_kernel<1, 16, true>; accumulate_enc = 1"),
    Dec16Bwd(256, 64, 17, 9, 2, 0, False, True, "W = 768: generic kernel; d_e_all = NULL; _bwd_loop + _bwd_weights"),
    Dec16Bwd(512, 64, 5, 33, 2, 0, True, False, "W = 1536: attn_dot_side_reg_kernel<1, 16, true, 3, false>"),
    Dec16Bwd(512, 64, 130, 9, 1, 1, True, False, "W = 1536, M >= 128: <1, 8, true, 3, true>; accumulate_enc = 1; only the last-step branch"),
    Dec16Bwd(1024, 64, 16, 9, 1, 0, True, False, "W = 3072: NJ = 6"),
]


@functools.lru_cache(maxsize=None)
def dec16_inputs(H, E, B, Ts, Tt):
    """dec_inputs and the key projection's weight; "pe" is put in by the caller: the fp16 keys the mode's vag_attn_keys_proj stored
    (device test: the device's own; host test: the restatement's own), decoded to fp32, exact from there on."""
    d = dict(dec_inputs(H, E, B, Ts, Tt))
    d["attn_e"] = _uni(_rs(28, H, B, Ts), 2 * H, 2 * H, k=(2 * H) ** -0.5)
    del d["pe"]
    for k in ("d_h2", "d_c", "d_e", "d_enc0", "g_emb0"):                     # the gradient side at GRAD16 (module docstring: range)
        d[k] = _f32(d[k] * GRAD16)
    d["g0"] = {k: _f32(g * GRAD16) for k, g in d["g0"].items()}
    return d


def dec16_keys_inputs(inp):
    B, Ts, C = inp["enc"].shape
    return dict(enc=inp["enc"].reshape(B * Ts, C), attn_e=inp["attn_e"])


def dec16_defect_cases(defect):
    keys = []
    for c in DEC16_CASES:
        if defect == "stale_h2_at_late_step" and c.Tt < 3:
            continue
        keys.append(c[:5])
    return keys


def dec16_bwd_defect_cases(defect):
    """The backward cases at which the defect changes a result."""
    out = []
    for c in DEC16_BWD_CASES:
        if defect in ("carry_dropped_at_step", "g_emb0_touched") and c.Tt < 2:
            continue
        if defect == "accumulate_enc_ignored" and not c.acc:
            continue
        if defect == "d_e_all_ignored" and not c.d_e:
            continue
        out.append(c)
    return out
