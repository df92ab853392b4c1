"""Float64 references WITH THEIR OWN ERROR BOUND for the operators around the dense products: the embeddings, the shared-space
projections, the image-conditioned attention, the ranking loss and the decoder's initial state, written from the definitions in
include/vag_nmt.h:

    vag_embed_fwd / _bwd        "embedding (nn.Embedding(padding_idx=0) ...)": out = W[idx]; g_W[idx[i]] += d_out[i], row 0 never
    vag_l2norm_fwd / _bwd       "a8 alone: out = x / max(||x||, 1e-12) per row"
    vag_img_proj_l2_fwd / _bwd  "out = l2norm(act(x W^T + b)); x (B,K), W (S,K).  y (B,S) = activation output and nrm (B) are saved."
                                "d_out is consumed.  d_x may be NULL; g_W, g_b accumulated."
    vag_imagine_attn_ctx_*      "method 0 = 'dot' (score_dot), 1 = 'mlp' (score_mlp; mlp_w (C)).  im_emb (B,S), enc (B,Ts,C), mask (B,Ts).
                                 Outputs alpha (B,Ts), ctx (B,C). ... 'dot' uses e[b,t] = enc[b,t] . (W_cc^T (W_ec im_emb[b]))"
                                "d_ctx (B,C) in.  d_enc (B,Ts,C) is written or added to (accumulate_enc); d_im_emb (B,S) written."
    vag_rank_loss_fwd / _bwd    "kind 0 = pairwise (both directions), 1 = image retrieval (cost_s only).  im, s (B,S).  loss (1).
                                 G (B,B) = d loss / d scores ... kind | 2 (B even): rows 2 p and 2 p + 1 are twins ... every entry (i, j)
                                 with i != j and i >> 1 == j >> 1 is skipped by both hinges and its G is 0."
    vag_dec_init_fwd / _bwd     "x = split*ctx + (1-split)*sum_t enc/sum_t mask (ctx NULL: text-only, x = mean);  h0 = tanh(W x + b)."
                                "d_h0 consumed.  d_enc written or added; d_ctx (may be NULL) written."
    vag_retrieval_ranks         "ranks[i] = 0-based position of key i in the descending sort of scores[i,:]"
    vag_gather_rows_i64         "out[i, 0:w] = in[idx[i], 0:w]"

Every operator is written ONCE, over an arithmetic `A`:
  * A = Tr   -- tracked values: a pair (value, err) of float64 arrays, err >= 0 a bound on |fp32 result - value| for ANY fp32
                evaluation of the same formula, whatever its summation order.  This is the reference the device is held to,
                element by element: |got - value| <= err.  No bound is relative to the maximum of a whole tensor.
  * A = F32  -- the same formula in np.float32 (every sum pairwise, numpy's order): the "fp32 restatement".  tests/test_ground_ref_host.py
                asserts that it lies inside the tracked bound (the bound is honest) and that each entry of the defect catalogue --
                the restatement with ONE subtle mistake, `defect=` -- leaves it (the bound is sensitive).

Tracked operations and their constants (u = 2^-24 is the unit roundoff of fp32):
  ein / mm   a bilinear contraction (matrix product, batched dot product, weighted sum, outer product):
             err = EPS (|a| |b|) + |a| err_b + err_a |b| + err_a err_b, EPS = 2^-21 -- the suite's convention for an fp32
             accumulation of any order on this device (tests/test_gpu_gemm_paths.py), bf16x6 matrix pipes included
             worst_case: max(EPS, gamma_n) in place of EPS, n the number of terms, gamma_n = n u / (1 - n u) -- the theorem for
             n terms added in ANY order (each of the n - 1 additions rounds a partial sum no larger than sum|terms|, each product
             once).  EPS = 8 u is that theorem for n <= 8 and an observation beyond: it holds when the terms are of one size and
             of mixed sign, so that partial sums stay near sqrt(k) of them.  The ranking loss's backward is not of that kind:
             a row of G is ~B entries of 1 or 2 and a diagonal of about -B, so one term of the B carries most of sum|terms| and the
             ~B additions after it each round at ITS size -- a random walk of ~0.3 u sqrt(B) |term|, whose largest of 65536
             elements passes 8 u sum|terms| from B ~ 100 on.  Measured with EPS at B = 128, 130, 144: 1.57 x the bound on the
             device (the one-launch kernel and the two products alike), 1.67 x for a sequential fp32 sum on the CPU, 0.69 x for a
             pairwise one; B <= 32 stayed below 0.5.  rank_bwd therefore asks for worst_case; nothing else does.
  sum        err = EPS sum|a| + sum err_a
  mul, scale (by an exact fp32 constant), div by an exact array: first-order propagation plus ULP = 2^-23 = 2 u of the result's
             magnitude per operation (one rounding is u; the factor 2 covers a fused multiply-add taken or not taken)
  add, sub   err_a + err_b + ULP (|a| + |b|): chains of these are accumulations whose association the device is free to choose
             (old + p u + r w in one kernel, old + p u and a product on top in another); a three-term sum in any order rounds
             twice, u |partial| + u |total| <= 2 u sum|terms|
  tanh       |tanh'| <= 1: err = err_a + TANH_ABS, TANH_ABS = 2^-20 (tests/test_gpu_gemm_paths.py; common.h: vag_tanh =
             1 - 2 rcp(exp(2x) + 1): the exponential's relative error r = (|2x| + 2) 2^-23 enters as 2 e r / (e + 1)^2 <= 2^-23 at
             x = 0 and decays with |x|; the reciprocal and the final subtraction add 2^-23 + 2^-24: < 3 * 2^-23 in all)
  exp        common.h / attn.hip use __expf = exp2(x log2 e): the product x log2 e is rounded (relative 2^-24 of an argument of
             size |x| log2 e, i.e. |x| 2^-24 log2 e ln 2 = |x| 2^-24 relative in the result) and v_exp_f32 is good to 1 ulp; with an
             argument error d the relative error is at most d + (|x| + 2) 2^-23
  softmax    alpha_t = exp(x_t - m) / sum: shift invariant, so the error of m cancels.  Relative error of a numerator
             r_t = d_t + ULP |x_t - m| + (|x_t - m| + 2) 2^-23; of the sum, sum_t p_t r_t / sum + EPS; the reciprocal RCP_REL; the
             product ULP.  err = alpha (exp(total) - 1) (second order included).  Masked positions: value 0, err 0.
  rcp, sqrt  RCP_REL = SQRT_REL = 2^-22: "a few ulp" -- v_rcp_f32 is 1 ulp (common.h), 1.f / n compiles to an IEEE division or to
             the reciprocal, sqrtf is correctly rounded; 2 ulp of 2^-23 allows either.
Sums whose ORDER is free and whose length is known (the embedding backward's atomics) use gamma_k = k u / (1 - k u) sum|terms|.

Inputs of a backward that the forward SAVED (nrm, out, y, alpha, xmix, h0, G) are taken as the fp32 arrays the forward produced --
they are arguments of the backward call -- and enter exactly; what a backward reads from a private workspace (the attention's u, w,
pre) is recomputed here and carries its tracked error.

The cases of tests/test_gpu_ground_ops.py live here too (EMBED_CASES ... INIT_CASES and the *_inputs generators), so that the host
test checks the bound at exactly the shapes and inputs the device is tested at."""
import numpy as np

U24 = 2.0 ** -24
ULP = 2.0 ** -23
EPS = 2.0 ** -21
TANH_ABS = 2.0 ** -20
RCP_REL = 2.0 ** -22
SQRT_REL = 2.0 ** -22
L2_EPS = np.float32(1e-12)


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U24 / (1.0 - k * U24)


# ---------------------------------------------------------------------------------------------------------------- tracked values
class TV:
    """(value, err): float64 arrays of one shape, err >= 0."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    shape = property(lambda self: self.v.shape)

    def __getitem__(self, k):
        return TV(self.v[k], self.e[k])


class Tr:
    """The tracked arithmetic (module docstring)."""
    name = "tracked"

    @staticmethod
    def lift(x):
        return x if isinstance(x, TV) else TV(np.asarray(x, dtype=np.float64))

    @staticmethod
    def ein(spec, a, b, worst_case=False):
        a, b = Tr.lift(a), Tr.lift(b)
        av, bv = np.abs(a.v), np.abs(b.v)
        eps = EPS
        if worst_case:                                                     # (module docstring: ein, worst_case)
            ins, out = spec.split("->")
            dims = dict(zip(ins.replace(",", ""), a.v.shape + b.v.shape))
            eps = max(EPS, float(gamma(np.prod([dims[k] for k in set(dims) - set(out)]))))
        e = eps * np.einsum(spec, av, bv) + np.einsum(spec, av, b.e) + np.einsum(spec, a.e, bv) + np.einsum(spec, a.e, b.e)
        return TV(np.einsum(spec, a.v, b.v), e)

    @staticmethod
    def add(a, b):
        a, b = Tr.lift(a), Tr.lift(b)
        return TV(a.v + b.v, a.e + b.e + ULP * (np.abs(a.v) + np.abs(b.v)))

    @staticmethod
    def sub(a, b):
        a, b = Tr.lift(a), Tr.lift(b)
        return TV(a.v - b.v, a.e + b.e + ULP * (np.abs(a.v) + np.abs(b.v)))

    @staticmethod
    def mul(a, b):
        a, b = Tr.lift(a), Tr.lift(b)
        v = a.v * b.v
        return TV(v, np.abs(a.v) * b.e + a.e * np.abs(b.v) + a.e * b.e + ULP * np.abs(v))

    @staticmethod
    def scale(a, c):
        a = Tr.lift(a)
        c = float(np.float32(c))
        v = c * a.v
        return TV(v, abs(c) * a.e + ULP * np.abs(v))

    @staticmethod
    def div_exact(a, c):
        a = Tr.lift(a)
        c = np.asarray(c, dtype=np.float64)
        v = a.v / c
        return TV(v, a.e / np.abs(c) + ULP * np.abs(v))

    @staticmethod
    def sum(a, axis):
        a = Tr.lift(a)
        return TV(a.v.sum(axis), EPS * np.abs(a.v).sum(axis) + a.e.sum(axis))

    @staticmethod
    def tanh(a):
        a = Tr.lift(a)
        return TV(np.tanh(a.v), a.e + TANH_ABS)

    @staticmethod
    def rcp(a):
        a = Tr.lift(a)
        assert (np.abs(a.v) > a.e).all(), "reciprocal of a value that may be zero"
        v = 1.0 / a.v
        return TV(v, np.abs(v) * (a.e / (np.abs(a.v) - a.e) + RCP_REL))

    @staticmethod
    def sqrt(a):
        a = Tr.lift(a)
        v = np.sqrt(a.v)
        lo = np.sqrt(np.maximum(a.v - a.e, 0.0))
        hi = np.sqrt(a.v + a.e)
        return TV(v, np.maximum(hi - v, v - lo) + SQRT_REL * v)

    @staticmethod
    def softmax(x, mask):
        """Rows of x (.., T) with mask (.., T) of 0 / 1; every row has an unmasked position."""
        x = Tr.lift(x)
        on = np.asarray(mask) != 0
        assert on.any(-1).all(), "an attention row without an unmasked position"
        xv = np.where(on, x.v, -np.inf)
        d = xv.max(-1, keepdims=True) - xv                                  # x_t - m, as a magnitude
        d = np.where(on, d, 0.0)
        p = np.where(on, np.exp(-d), 0.0)
        r = np.where(on, x.e + ULP * d + (d + 2.0) * 2.0 ** -23, 0.0)
        s = p.sum(-1, keepdims=True)
        rs = (p * r).sum(-1, keepdims=True) / s + EPS
        alpha = p / s
        return TV(alpha, alpha * np.expm1(r + rs + RCP_REL + ULP))

    @staticmethod
    def expand(a, axis, n):
        a = Tr.lift(a)
        return TV(np.repeat(np.expand_dims(a.v, axis), n, axis), np.repeat(np.expand_dims(a.e, axis), n, axis))

    @staticmethod
    def where(c, a, b):
        a, b = Tr.lift(a), Tr.lift(b)
        return TV(np.where(c, a.v, b.v), np.where(c, a.e, b.e))

    @staticmethod
    def value(a):
        return Tr.lift(a).v


class F32:
    """The same operations in np.float32 (numpy's summation order; the device forms of tanh and exp restated)."""
    name = "fp32"
    f = np.float32

    @staticmethod
    def lift(x):
        return np.asarray(x, dtype=np.float32)

    @staticmethod
    def ein(spec, a, b):
        """The products in fp32, then numpy's pairwise fp32 sum over the contracted indices (moved last, flattened)."""
        ins, out = spec.split("->")
        red = "".join(sorted(set(ins.replace(",", "")) - set(out)))
        prod = np.ascontiguousarray(np.einsum(ins + "->" + out + red, F32.lift(a), F32.lift(b)), dtype=np.float32)
        if not red:
            return prod
        return prod.reshape(prod.shape[:len(out)] + (-1,)).sum(-1, dtype=np.float32)

    @staticmethod
    def add(a, b):
        return (F32.lift(a) + F32.lift(b)).astype(np.float32)

    @staticmethod
    def sub(a, b):
        return (F32.lift(a) - F32.lift(b)).astype(np.float32)

    @staticmethod
    def mul(a, b):
        return (F32.lift(a) * F32.lift(b)).astype(np.float32)

    @staticmethod
    def scale(a, c):
        return (np.float32(c) * F32.lift(a)).astype(np.float32)

    @staticmethod
    def div_exact(a, c):
        return (F32.lift(a) / np.asarray(c, dtype=np.float32)).astype(np.float32)

    @staticmethod
    def sum(a, axis):
        return F32.lift(a).sum(axis, dtype=np.float32)

    @staticmethod
    def tanh(a):
        with np.errstate(over="ignore"):                                 # common.h: vag_tanh; exp -> inf gives 1 - 0
            e = np.exp(np.float32(2.0) * F32.lift(a), dtype=np.float32)
            return (np.float32(1.0) - np.float32(2.0) / (e + np.float32(1.0))).astype(np.float32)

    @staticmethod
    def rcp(a):
        return (np.float32(1.0) / F32.lift(a)).astype(np.float32)

    @staticmethod
    def sqrt(a):
        return np.sqrt(F32.lift(a), dtype=np.float32)

    @staticmethod
    def softmax(x, mask, leak=None):
        x = F32.lift(x)
        on = np.asarray(mask) != 0
        xv = np.where(on, x, np.float32(-np.inf))
        m = xv.max(-1, keepdims=True)
        if leak is not None:                                               # (defect catalogue: a finite score at a masked position)
            xv = np.where(on, xv, m + np.float32(leak))
        p = np.exp(xv - m, dtype=np.float32)
        return (p * (np.float32(1.0) / p.sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)

    @staticmethod
    def expand(a, axis, n):
        return np.repeat(np.expand_dims(F32.lift(a), axis), n, axis)

    @staticmethod
    def where(c, a, b):
        return np.where(c, F32.lift(a), F32.lift(b)).astype(np.float32)

    @staticmethod
    def value(a):
        return np.asarray(a, dtype=np.float64)


def ratio(got, ref):
    """Largest |got - value| / err over the elements of a tracked reference (0 / 0 = 0, x / 0 = inf)."""
    ref = Tr.lift(ref)
    d = np.abs(np.asarray(got, dtype=np.float64) - ref.v)
    if d.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / ref.e)
    q = np.where(np.isnan(np.asarray(got, dtype=np.float64)), np.inf, q)
    return float(q.max())


def _rs(*key):
    return np.random.RandomState(np.array([abs(int(k)) % (2 ** 31) for k in key], dtype=np.uint32))


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- embedding
EMBED_V = 11
EMBED_NEVER = 9            # a row no index names; the LAST row (10) is named, so that a write past E would land in the guard tail
EMBED_CASES = [(E, n) for E in (4, 60, 64, 68, 256) for n in (1, 7, 300)]


def embed_inputs(E, n):
    rs = _rs(11, E, n)
    if n == 1:
        idx = np.array([10])
    elif n == 7:
        idx = np.array([0, 3, 0, 10, 3, 0, 1])
    else:
        idx = rs.choice([0, 1, 2, 3, 5, 6, 7, 8, 10], size=n)
        idx[rs.permutation(n)[:70]] = 4                                    # one index at least 64 times
        idx[:5] = [0, 10, 0, 4, 0]
    assert EMBED_NEVER not in idx
    return dict(idx=idx.astype(np.int64), W=_f32(rs.randn(EMBED_V, E)), d_out=_f32(rs.randn(n, E)), g0=_f32(rs.randn(EMBED_V, E)))


def embed_fwd_ref(inp):
    return inp["W"][inp["idx"]]                                            # a gather: bitwise


def embed_bwd_ref(inp):
    """g_W = g0 + scatter-add of d_out, row 0 untouched; err = gamma_k sum|terms| with k the row's multiplicity (0: exact)."""
    idx, d = inp["idx"], inp["d_out"].astype(np.float64)
    v = inp["g0"].astype(np.float64).copy()
    mag = np.abs(v)
    k = np.zeros(EMBED_V)
    for i, r in enumerate(idx):
        if r != 0:
            v[r] += d[i]
            mag[r] += np.abs(d[i])
            k[r] += 1
    return TV(v, gamma(k)[:, None] * mag)


def embed_bwd_f32(inp, defect=None):
    idx, d = inp["idx"], inp["d_out"]
    g = inp["g0"].copy()
    rows = list(enumerate(idx))
    if defect == "duplicate_dropped":                                      # the last occurrence of the most frequent index is lost
        top = np.bincount(idx[idx != 0]).argmax()
        rows.remove((int(np.nonzero(idx == top)[0][-1]), top))
    for i, r in rows:
        if r != 0 or defect == "pad_row_written":
            g[r] = g[r] + d[i]
    return g


EMBED_DEFECTS = ["duplicate_dropped", "pad_row_written"]


# ---------------------------------------------------------------------------------------------------------------- l2norm, projections
# rows: scale 1, an all-zero row, 1e-3, 1e3, and a row whose norm is below the clamp without being zero (2e-14 sqrt(S) < 1e-12: the
# eps branch of the backward with out != 0)
L2_CASES = [(B, S) for B in (1, 5) for S in (1, 4, 257, 512, 1000)]
PROJ_CASES = [(B, K, S, act) for B in (1, 5) for S in (1, 4, 257, 512, 1000) for K in (8, 100) for act in (0, 1)] + \
             [(3, 2048, 8, 0), (3, 2048, 8, 1)]
L2_ZERO_ROW = 1


def _row_scales(B, tiny):
    return np.array([1.0, 0.0, 1e-3, 1e3, 1e-14 if tiny else 1.0][:B]) if B > 1 else np.array([1.0])


def _dout_scales(B, tiny):
    """d_out of the rows whose norm is the clamp is of size 1e-12, so that dy = d_out / 1e-12 stays of size 1 next to the other rows."""
    return np.array([1.0, 1e-12, 1.0, 1.0, 1e-12 if tiny else 1.0][:B]) if B > 1 else np.array([1.0])


def l2_inputs(B, S):
    rs = _rs(12, B, S)
    x = _f32(rs.randn(B, S) * _row_scales(B, True)[:, None])
    return dict(x=x, d_out=_f32(rs.randn(B, S) * _dout_scales(B, True)[:, None]))


def proj_inputs(B, K, S, act):
    """act = 0: zero bias, so that the all-zero row of x gives an all-zero y (exact); act = 1: a bias, and no zero row."""
    rs = _rs(13, B, K, S, act)
    sc = _row_scales(B, False).copy()
    if act and B > 1:
        sc[L2_ZERO_ROW] = 1.0
    x = _f32(rs.randn(B, K) * sc[:, None])
    W = _f32(rs.randn(S, K) * K ** -0.5)
    b = _f32(rs.randn(S) if act else np.zeros(S))
    return dict(x=x, W=W, b=b, d_out=_f32(rs.randn(B, S) * (_dout_scales(B, False) if not act else np.ones(B))[:, None]), gW0=_f32(rs.randn(S, K)), gb0=_f32(rs.randn(S)))


def l2norm_fwd(A, y):
    """out = y / max(||y||, 1e-12) per row -> (nrm, out).  The clamp must be decidable from the tracked sum of squares."""
    y = A.lift(y)
    ss = A.sum(A.mul(y, y), -1)
    n = A.sqrt(ss)
    if A is Tr:
        small = n.v + n.e < float(L2_EPS)
        assert (small | (n.v - n.e > float(L2_EPS))).all(), "a row norm too close to the clamp to call"
        n = Tr.where(small, TV(np.full(n.shape, float(L2_EPS))), n)
    else:
        n = np.maximum(n, L2_EPS)
    inv = A.rcp(n)
    return n, A.mul(y, A.expand(inv, -1, y.shape[-1]))


def l2norm_bwd(A, y, nrm, out, d_out, act, defect=None):
    """dy = (d_out - out (out . d_out)) / nrm, the projection term absent where nrm is the clamp; times (1 - y^2) with act.
    y, nrm, out: the forward's saved fp32 arrays, exact."""
    S = np.shape(out)[-1]
    dot = A.sum(A.mul(out, d_out), -1)
    clamp = ~(np.asarray(nrm) > L2_EPS)
    if defect != "eps_branch_ignored":
        dot = A.where(clamp, np.zeros(np.shape(nrm)), dot)
    proj = A.mul(out, A.expand(dot, -1, S))
    if defect == "projection_scaled":
        proj = A.scale(proj, 1.0 - 2.0 ** -10)
    g = A.mul(A.sub(d_out, proj), A.expand(A.rcp(nrm), -1, S))
    if act:
        g = A.mul(g, A.sub(np.ones(np.shape(y)), A.mul(y, y)))
    return g


L2_DEFECTS = ["projection_scaled", "eps_branch_ignored"]


def proj_fwd(A, inp, act):
    y = A.add(A.ein("bk,sk->bs", inp["x"], inp["W"]), inp["b"][None, :])
    if act:
        y = A.tanh(y)
    nrm, out = l2norm_fwd(A, y)
    return dict(y=y, nrm=nrm, out=out)


def proj_bwd(A, inp, saved, act, defect=None):
    """saved: y, nrm, out as fp32 arrays.  -> dy (what d_out holds afterwards), d_x, g_W, g_b (accumulated onto gW0, gb0)."""
    dy = l2norm_bwd(A, saved["y"], saved["nrm"], saved["out"], inp["d_out"], act, defect)
    return dict(dy=dy, d_x=A.ein("bs,sk->bk", dy, inp["W"]), g_W=A.add(inp["gW0"], A.ein("bs,bk->sk", dy, inp["x"])),
                g_b=A.add(inp["gb0"], A.sum(dy, 0)))


# ---------------------------------------------------------------------------------------------------------------- grounding attention
def _attn_cases():
    """(method, attn_row, B, Ts, C, S, accumulate_enc).  B, S and accumulate_enc cycle over {1, 3}, {4, 20} and {0, 1} along each list
    with different periods, so that every value meets every kernel family."""
    shapes = []
    shapes += [(0, 1, Ts, C) for C in (512, 1024) for Ts in (1, 16, 17, 32, 33, 48, 49, 64)]     # register kernel, 1..4 groups
    shapes += [(0, 1, 65, 512), (0, 1, 5, 8), (0, 1, 5, 260), (0, 1, 3, 4096)]                   # generic row kernel, its branches
    shapes += [(0, 0, Ts, C) for C in (8, 260, 512) for Ts in (3, 21)]                           # scores / softmax-bwd / attn_ctx
    shapes += [(1, row, Ts, C) for row in (1, 0) for C in (8, 260, 512) for Ts in (7, 8, 9, 17)]  # mlp: chunk edges
    out = []
    for i, (method, row, Ts, C) in enumerate(shapes):
        B = 2 if C == 4096 else (3, 1, 3)[i % 3]
        out.append((method, row, B, Ts, C, (4, 20)[(i // 3 + i) % 2], (i // 2 + i // 3) % 2))
    return out


ATTN_CASES = _attn_cases()


def attn_lengths(B, Ts):
    """Ragged, with a length-1 row when there is more than one row; row 0 is full."""
    return [Ts, 1, (Ts + 1) // 2, max(1, Ts - 1)][:B]


def attn_inputs(method, row, B, Ts, C, S, acc):
    rs = _rs(14, method, B, Ts, C, S)
    im = rs.randn(B, S)
    im /= np.sqrt((im * im).sum(1, keepdims=True))                           # an l2-normalised embedding
    mask = np.zeros((B, Ts))
    for b, n in enumerate(attn_lengths(B, Ts)):
        mask[b, :n] = 1.0
    # scores of a few units: the dot method's e = enc . w has C terms, the mlp's is bounded by sum|mlp_w|
    enc = rs.randn(B, Ts, C) * (2.0 * C ** -0.5 if method == 0 else 1.0)      # (masked positions keep finite values: the mask decides)
    d = dict(im_emb=_f32(im), enc=_f32(enc), mask=_f32(mask), ctx2ctx=_f32(rs.randn(C, C) * C ** -0.5), emb2ctx=_f32(rs.randn(C, S)),
             mlp_w=_f32(rs.randn(C) * 2.0 * C ** -0.5), d_ctx=_f32(rs.randn(B, C)), d_enc0=_f32(rs.randn(B, Ts, C)),
             g_cc0=_f32(rs.randn(C, C)), g_ec0=_f32(rs.randn(C, S)), g_mlp0=_f32(rs.randn(C)))
    return d


def _attn_common(A, inp, method):
    u = A.ein("bs,cs->bc", inp["im_emb"], inp["emb2ctx"])                     # emb2ctx(image_vec)
    if method == 0:
        return u, A.ein("bi,ij->bj", u, inp["ctx2ctx"]), None               # w = W_cc^T u
    return u, None, A.ein("btj,ij->bti", inp["enc"], inp["ctx2ctx"])          # pre = ctx2ctx(enc)


def attn_fwd(A, inp, method, defect=None):
    """-> alpha (B,Ts), ctx (B,C), scores (B,Ts; for the input conditions)."""
    u, w, pre = _attn_common(A, inp, method)
    Ts = inp["enc"].shape[1]
    if method == 0:
        e = A.ein("btc,bc->bt", inp["enc"], w)
    else:
        e = A.ein("btc,c->bt", A.tanh(A.add(pre, A.expand(u, 1, Ts))), inp["mlp_w"])
    alpha = F32.softmax(e, inp["mask"], leak=-20.0) if defect == "mask_leak" else A.softmax(e, inp["mask"])
    enc = inp["enc"]
    if defect == "ctx_last_position_missing":
        alpha_c, enc = alpha[:, :-1], enc[:, :-1]
    else:
        alpha_c = alpha
    return dict(alpha=alpha, ctx=A.ein("bt,btc->bc", alpha_c, enc), scores=e)


def attn_bwd(A, inp, alpha, method, acc, defect=None):
    """alpha: the forward's fp32 output, exact.  -> d_enc, d_im_emb, g_ctx2ctx, g_emb2ctx, g_mlp_w (method 1)."""
    u, w, pre = _attn_common(A, inp, method)
    enc, d_ctx = inp["enc"], inp["d_ctx"]
    B, Ts, C = enc.shape
    dalpha = A.ein("btc,bc->bt", enc, d_ctx)
    dot = A.sum(A.mul(alpha, dalpha), -1)
    if defect == "softmax_bwd_sum_scaled":
        dot = A.scale(dot, 1.0 - 2.0 ** -10)
    de = A.mul(alpha, A.sub(dalpha, A.expand(dot, -1, Ts)))
    d_enc = A.ein("bt,bc->btc", alpha, d_ctx)
    out = {}
    if method == 0:
        d_enc = A.add(d_enc, A.ein("bt,bc->btc", de, w))
        dw = A.ein("bt,btc->bc", de[:, 1:], enc[:, 1:]) if defect == "dw_position_missing" else A.ein("bt,btc->bc", de, enc)
        du = A.ein("bj,ij->bi", dw, inp["ctx2ctx"])
        out["g_ctx2ctx"] = A.add(inp["g_cc0"], A.ein("bi,bj->ij", u, dw))
    else:
        th = A.tanh(A.add(pre, A.expand(u, 1, Ts)))
        dth = A.mul(A.expand(de, -1, C), A.sub(np.ones((B, Ts, C)), A.mul(th, th)))          # de (1 - th^2)
        dpre = A.mul(dth, inp["mlp_w"][None, None, :])
        last = 8 * ((Ts + 7) // 8 - 1)
        keep = slice(0, last) if defect == "mlp_w_last_chunk_missing" else slice(0, Ts)
        out["g_mlp_w"] = A.add(inp["g_mlp0"], A.ein("bt,btc->c", de[:, keep], th[:, keep]))
        du = A.sum(dpre, 1)
        d_enc = A.add(d_enc, A.ein("bti,ij->btj", dpre, inp["ctx2ctx"]))
        out["g_ctx2ctx"] = A.add(inp["g_cc0"], A.ein("bti,btj->ij", dpre, enc))
    if acc:
        d_enc = A.add(inp["d_enc0"], d_enc)
    out.update(d_enc=d_enc, d_im_emb=A.ein("bc,cs->bs", du, inp["emb2ctx"]),
               g_emb2ctx=A.add(inp["g_ec0"], A.ein("bc,bs->cs", du, inp["im_emb"])))
    return out


ATTN_FWD_DEFECTS = ["mask_leak", "ctx_last_position_missing"]
ATTN_BWD_DEFECTS = ["softmax_bwd_sum_scaled", "dw_position_missing"]            # dw: the dot method only
ATTN_MLP_DEFECTS = ["mlp_w_last_chunk_missing"]


# ---------------------------------------------------------------------------------------------------------------- ranking loss
RANK_SHAPES = [(1, 4), (2, 8), (16, 4), (16, 64), (17, 60), (32, 6), (128, 512), (130, 68), (144, 512)]
# the seed of each shape's inputs: the first one under which no hinge of any kind is ambiguous (tests/test_ground_ref_host.py asserts
# it, and the 20 .. 80 % active hinges, rather than searching)
RANK_SEEDS = {(1, 4): 0, (2, 8): 0, (16, 4): 0, (16, 64): 0, (17, 60): 0, (32, 6): 0, (128, 512): 0, (130, 68): 0, (144, 512): 1}
RANK_CASES = [(B, S, kind) for (B, S) in RANK_SHAPES for kind in (0, 1, 2, 3) if not (kind & 2 and B % 2)]
RANK_D_LOSS = np.float32(0.37)


def rank_margin(S):
    return np.float32(0.15 if S == 512 else 0.3)


def rank_inputs(B, S, seed=None):
    rs = _rs(15, B, S, RANK_SEEDS[(B, S)] if seed is None else seed)
    im = rs.randn(B, S)
    s = im + (6.0 if S == 512 else 3.0) * rs.randn(B, S)
    im /= np.sqrt((im * im).sum(1, keepdims=True))
    s /= np.sqrt((s * s).sum(1, keepdims=True))
    return dict(im=_f32(im), s=_f32(s))


def rank_fwd(A, inp, margin, kind, defect=None):
    """-> loss (scalar), G (B,B) small integers, and for the input conditions: hinges (their count), active, ambiguous."""
    B = inp["im"].shape[0]
    sc = A.ein("is,js->ij", inp["im"], inp["s"])
    i, j = np.indices((B, B))
    live = i != j
    if kind & 2 and defect != "twin_not_skipped":
        live &= (i >> 1) != (j >> 1)
    diag = sc[np.arange(B), np.arange(B)]
    m = np.full((B, B), np.float32(margin))
    terms = [A.add(A.sub(m, A.expand(diag, 0, B)), sc)]                        # cost_s: margin - d_j + S_ij
    if (kind & 1) == 0:
        terms.append(A.add(A.sub(m, A.expand(diag, 1, B)), sc))               # cost_im: margin - d_i + S_ij
    G = np.zeros((B, B))
    loss = None
    stats = dict(hinges=0, active=0, ambiguous=0)
    for k, c in enumerate(terms):
        cv = A.value(c)
        on = live & (cv > 0)
        stats["hinges"] += int(live.sum())
        stats["active"] += int(on.sum())
        if A is Tr:
            stats["ambiguous"] += int((live & (np.abs(c.v) <= c.e)).sum())
        G += on
        cnt = on.sum(0) if k == 0 else on.sum(1)                               # d / d d_j of cost_s, d / d d_i of cost_im
        G[np.arange(B), np.arange(B)] -= cnt
        part = A.sum(A.where(on, c, np.zeros((B, B))), (0, 1))
        loss = part if loss is None else A.add(loss, part)
    if defect == "diagonal_count_missing" and stats["active"]:
        r = int(np.argmin(np.diag(G)))
        G[r, r] += 1
    return dict(loss=loss, G=G, **stats)


def rank_bwd(A, inp, G, d_loss, defect=None):
    """G: the forward's fp32 output, exact.  d_im = d_loss G s, d_s = d_loss G^T im."""
    kw = dict(worst_case=True) if A is Tr else {}                           # (module docstring: one dominant term per row of G)
    d_im = A.ein("ij,js->is", G, inp["s"], **kw)
    d_s = A.ein("ij,is->js", G.T if defect == "G_not_transposed" else G, inp["im"], **kw)
    if defect != "d_loss_not_applied":
        d_im, d_s = A.scale(d_im, d_loss), A.scale(d_s, d_loss)
    return dict(d_im=d_im, d_s=d_s)


RANK_FWD_DEFECTS = ["diagonal_count_missing", "twin_not_skipped"]
RANK_BWD_DEFECTS = ["G_not_transposed", "d_loss_not_applied"]


# ---------------------------------------------------------------------------------------------------------------- initial state
# mode: ("ctx", split) or ("text", 0.5) -- ctx NULL with split = 0.5 passed anyway: x is the plain mean, the backward's coefficient 1
INIT_SHAPES = [(1, 1, 8, 5), (5, 7, 48, 24), (128, 3, 8, 8), (130, 3, 8, 8)]
INIT_MODES = [("ctx", 0.0), ("ctx", 0.5), ("ctx", 1.0), ("text", 0.5)]
INIT_CASES = [(B, Ts, C, H, mode, split, acc) for (B, Ts, C, H) in INIT_SHAPES for (mode, split) in INIT_MODES for acc in (0, 1)]


def init_inputs(B, Ts, C, H, mode, split, acc):
    rs = _rs(16, B, Ts, C, H)
    lens = np.concatenate([[Ts], rs.randint(1, Ts + 1, size=B - 1)])
    mask = (np.arange(Ts)[None, :] < lens[:, None]).astype(np.float64)
    return dict(enc=_f32(rs.randn(B, Ts, C)), mask=_f32(mask), ctx=_f32(rs.randn(B, C)), W=_f32(rs.randn(H, C) * C ** -0.5),
                b=_f32(rs.randn(H)), d_h0=_f32(rs.randn(B, H)), d_enc0=_f32(rs.randn(B, Ts, C)), gW0=_f32(rs.randn(H, C)),
                gb0=_f32(rs.randn(H)))


def init_fwd(A, inp, mode, split, defect=None):
    """x = split ctx + (1 - split) sum_t enc / sum_t mask (every t of enc: the encoder leaves zeros past a row's length, the formula
    does not ask); text: x = the mean.  -> xmix, h0."""
    B, Ts, C = inp["enc"].shape
    cnt = np.full((B, 1), float(Ts)) if defect == "mean_over_Ts" else inp["mask"].astype(np.float64).sum(1, keepdims=True)
    mean = A.div_exact(A.sum(inp["enc"], 1), cnt)
    if mode == "ctx":
        xmix = A.add(A.scale(inp["ctx"], split), A.scale(mean, np.float32(1.0) - np.float32(split)))
    else:
        xmix = mean
    return dict(xmix=xmix, h0=A.tanh(A.add(A.ein("bc,hc->bh", xmix, inp["W"]), inp["b"][None, :])))


def init_bwd(A, inp, saved, mode, split, acc, defect=None):
    """saved: xmix, h0 as fp32 arrays.  -> d_enc (every position: coef dx / sum_t mask), d_ctx (ctx form), g_W, g_b."""
    B, Ts, C = inp["enc"].shape
    h0 = saved["h0"]
    dpre = A.mul(inp["d_h0"], A.sub(np.ones(np.shape(h0)), A.mul(h0, h0)))
    dx = A.ein("bh,hc->bc", dpre, inp["W"])
    cnt = inp["mask"].astype(np.float64).sum(1, keepdims=True)
    coef = np.float32(1.0) - np.float32(split) if mode == "ctx" else np.float32(1.0)
    d_enc = A.expand(A.div_exact(A.scale(dx, coef), cnt), 1, Ts)
    if acc and defect != "accumulate_overwrites":
        d_enc = A.add(inp["d_enc0"], d_enc)
    out = dict(d_enc=d_enc, g_W=A.add(inp["gW0"], A.ein("bh,bc->hc", dpre, saved["xmix"])), g_b=A.add(inp["gb0"], A.sum(dpre, 0)))
    if mode == "ctx":
        out["d_ctx"] = dx if defect == "d_ctx_without_split" else A.scale(dx, split)
    return out


INIT_FWD_DEFECTS = ["mean_over_Ts"]
INIT_BWD_DEFECTS = ["d_ctx_without_split", "accumulate_overwrites"]


# ---------------------------------------------------------------------------------------------------------------- small riders
def retrieval_ranks_ref(scores):
    """Position of key i in the STABLE descending sort of scores[i, :]."""
    scores = np.asarray(scores)
    N = scores.shape[0]
    order = np.argsort(-scores, axis=1, kind="stable")
    return np.array([int(np.nonzero(order[i] == i)[0][0]) for i in range(N)], dtype=np.int32)


def gather_rows_ref(mat, idx, w):
    return np.asarray(mat)[np.asarray(idx), :w]
