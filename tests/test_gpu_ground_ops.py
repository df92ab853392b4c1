"""The operators around the dense products -- embeddings, shared-space projections, image-conditioned attention, ranking loss,
decoder initial state, and two small riders -- through the C ABI (vagnmt_hip._lib.call / ptr / stream / set_option), element by
element against the tracked float64 references of tests/ground_ref.py: |got - value| <= err, err carried by the reference itself
(its docstring derives every constant).  tests/test_ground_ref_host.py shows on the CPU that these bounds hold for an fp32
restatement of each operator and reject every entry of the defect catalogue, at exactly the cases below.

Guard bands, as in test_gpu_gemm_paths.py: every input is followed by NaN floats (an over-read shows as NaN), every output by a
sentinel tail that must come back bit-identical; outputs documented as written start as NaN, accumulated ones (g_W, g_b, g_ctx2ctx,
g_emb2ctx, g_mlp_w, d_enc with accumulate_enc) from random nonzero values that enter the reference.  Saved tensors a backward takes
as arguments (nrm, out, y, alpha, xmix, h0, G) are the device forward's own; the reference takes them as exact inputs.

Kernel reached by each case (dispatch conditions quoted from api.hip / attn.hip / vse.hip / elem.hip):
  vag_embed_fwd / _bwd        embed_gather_kernel (float4 per thread, E % 4 == 0); embed_scatter_kernel: one wave per (row, 64-float
                              block), `if (tok == 0 || e >= E) continue` -- E = 4, 60 (one ragged block), 64, 68 (a full and a ragged
                              block), 256; n = 300 has one index 70 times (atomics on one row), the LAST row is indexed so that a
                              write past E lands in the guard tail, row 9 never is.
  vag_l2norm_* / img_proj_l2  l2norm_fwd_kernel / l2norm_bwd_kernel, one 256-thread block per row: S = 1, 4 (one wave partly idle),
                              257 (one past the block), 512, 1000; `fmaxf(sqrtf(ss), 1e-12f)` and `if (!(n > 1e-12f)) dot = 0.f` with an
                              all-zero row and a row of norm ~1e-13; the projection through linear_fwd (M <= 256: skinny kernels by
                              K <= 256 / more: K = 8, 100, 2048), gemm_nn, gemm_tn_acc and colsum.
  vag_imagine_attn_ctx_*      method 0, attn_row 1 -> vag_attn_dot_row_launch: `np = ceil(Ts/16) <= 4 && (C == 1024 || C == 512)`
                              -> attn_dot_row_reg_kernel<BWD, NC = C/256, NP = np> (Ts = 1, 16 | 17, 32 | 33, 48 | 49, 64 at both
                              widths: NP = 1..4 at both edges); Ts = 65 at C = 512 -> attn_dot_row_kernel (np = 5); C = 8, 260 ->
                              attn_dot_row_kernel with `G = ROW_THREADS / nc4` = 512 and 15 (65 does not divide 1024: 49 idle
                              threads); C = 4096 -> `G == 1`.  method 0, attn_row 0 -> vag_attn_scores_launch(1), vag_attn_ctx_launch,
                              vag_softmax_bwd_launch, vag_attn_ctx_launch(0) for dw.  method 1 -> linear_fwd for pre,
                              vag_attn_scores_launch(0), vag_attn_ctx_launch; backward: attn_row 1 -> attn_dot_row_kernel<true>
                              without a sum, attn_row 0 -> scores + softmax_bwd; then vag_attn_post_bwd_launch with
                              `VAG_POST_CHUNKS(Ts) = ceil(Ts/8)` chunk rows (Ts = 7, 8 -> 1; 9 -> 2; 17 -> 3) summed by colsum into
                              g_mlp_w, vag_attn_dq_launch, two products.  vag_outer2_launch writes or accumulates d_enc.
  vag_rank_loss_fwd / _bwd    linear_fwd + rank_loss_kernel (one 1024-thread block); backward `B <= 128 && B % 16 == 0 && S % 4 == 0`
                              -> rank_bwd_kernel: (16, 4), (16, 64), (128, 512) -- its B = 16 and B = 128 ends; otherwise two
                              products + vag_scale_by_dev_launch: (17, 60) by B % 16, (130, 68) and (144, 512) by B > 128, (32, 6)
                              by S % 4, (1, 4) and (2, 8) by B % 16.  kind | 2 with an odd B is -EINVAL.
  vag_dec_init_fwd / _bwd     meanpool_mix_kernel + linear_fwd(tanh); backward: tanh_bwd, gemm_tn_acc, colsum, then
                              `ride = d_ctx && B <= 128` -> vag_skinny_nn_launch with the d_ctx rider: B = 1, 5, 128 with ctx;
                              B = 130, or ctx NULL -> gemm_nn (+ vag_axpy_launch for d_ctx); meanpool_bwd_kernel with
                              `s_eff = d_ctx ? split : 0`: ctx NULL is the text-only form, coefficient 1 whatever split says.
  vag_retrieval_ranks         vag_gemm_launch + retrieval_rank_kernel, `(v > d) || (v == d && j < i)`: exact ties from integer inputs.
  vag_gather_rows_i64         gather_rows_i64_kernel with w < ld, repeated and out-of-order rows.

Largest |err| / bound per operator: fp32 restatement on the CPU (tests/test_ground_ref_host.py -s) | device (this file -s):
  embed_bwd 0.99 | 0.99      l2norm_fwd 0.18 | 0.18      l2norm_bwd 0.24 | 0.24
  img_proj_l2_fwd 0.20 | 0.20      img_proj_l2_bwd 0.49 | 0.49
  imagine_attn_ctx_fwd 0.04 | 0.04      imagine_attn_ctx_bwd 0.49 | 0.49
  rank_loss_fwd 0.02 | 0.04      rank_loss_bwd 0.16 | 0.16
  dec_init_fwd 0.20 | 0.20      dec_init_bwd 0.34 | 0.34
(Where both columns agree the worst element is one whose error is the final rounding alone: the same on any machine.  rank_loss_bwd is
measured under the worst-case sum bound gamma_B that ground_ref.rank_bwd asks for; under EPS it was 1.57 on the device, 1.67 for a
sequential and 0.69 for a pairwise fp32 sum on the CPU, all at B >= 128 -- ground_ref's docstring, "worst_case", has the reason.)
Wall time of this file's 186 cases on an MI355X: 3 s."""
import numpy as np
import pytest
import torch

import ground_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e9
DEV = "cuda:0"
TAIL = 64
WORST = {}


def _L():
    from vagnmt_hip import _lib
    return _lib


def _in(x, dtype=torch.float32):
    """A host array on the device followed by TAIL NaN floats (int64: TAIL copies of an impossible index)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    pad = torch.full((TAIL,), float("nan")) if dtype == torch.float32 else torch.full((TAIL,), -(2 ** 40), dtype=dtype)
    buf = torch.cat([t.to(dtype), pad]).to(DEV)
    return buf[:t.numel()]


class _Out:
    """An output buffer of `shape`: NaN (written) or `start` (accumulated), then a sentinel tail."""

    def __init__(self, shape, start=None, dtype=torch.float32):
        n = int(np.prod(shape))
        body = torch.full((n,), float("nan")) if start is None else torch.from_numpy(np.ascontiguousarray(start)).reshape(-1).clone()
        if dtype != torch.float32:
            body = torch.full((n,), -1, dtype=dtype)
        self.sent = torch.full((TAIL,), SENTINEL if dtype == torch.float32 else -77).to(dtype)
        self.buf = torch.cat([body.to(dtype), self.sent]).to(DEV)
        self.view, self.n, self.shape = self.buf[:n], n, tuple(shape)

    def host(self, what, tag):
        out = self.buf.cpu()
        assert torch.equal(out[self.n:], self.sent), ("write past " + what, tag)
        return out[:self.n].view(self.shape).numpy()


def _check(op, what, out, ref, tag):
    got = out.host(what, tag) if isinstance(out, _Out) else out
    assert np.isfinite(got).all(), (what, "non-finite (a read outside an input, or an output that was never written)", tag)
    q = R.ratio(got, ref)
    WORST[op] = max(WORST.get(op, 0.0), q)
    print("%-22s %-10s %-44s |err|/bound %.3f" % (op, what, tag, q))
    assert q <= 1.0, (op, what, tag, "worst |err| / bound %.3g" % q)
    return got


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("E,n", R.EMBED_CASES, ids=_ids(R.EMBED_CASES))
def test_embedding_gather_is_bitwise_and_scatter_within_gamma_k(E, n):
    L = _L()
    inp = R.embed_inputs(E, n)
    idx, W, d_out = _in(inp["idx"], torch.int64), _in(inp["W"]), _in(inp["d_out"])
    out, gW = _Out((n, E)), _Out((R.EMBED_V, E), inp["g0"])
    L.call("vag_embed_fwd", L.ptr(idx, torch.int64), n, L.ptr(W), E, L.ptr(out.view), L.stream())
    L.call("vag_embed_bwd", L.ptr(idx, torch.int64), n, L.ptr(d_out), E, L.ptr(gW.view), L.stream())
    _sync()
    tag = (E, n)
    assert np.array_equal(out.host("out", tag).view(np.int32), R.embed_fwd_ref(inp).view(np.int32)), tag
    got = _check("embed_bwd", "g_W", gW, R.embed_bwd_ref(inp), tag)       # (the tail after V rows: columns past E stay untouched)
    for r in (0, R.EMBED_NEVER):
        assert np.array_equal(got[r].view(np.int32), inp["g0"][r].view(np.int32)), ("row %d was written" % r, tag)


# ---------------------------------------------------------------------------------------------------------------- l2norm, projections
@pytest.mark.parametrize("B,S", R.L2_CASES, ids=_ids(R.L2_CASES))
def test_l2norm_matches_fp64_per_element(B, S):
    L = _L()
    inp = R.l2_inputs(B, S)
    x, d_out = _in(inp["x"]), _in(inp["d_out"])
    nrm, out, dx = _Out((B,)), _Out((B, S)), _Out((B, S))
    L.call("vag_l2norm_fwd", L.ptr(x), B, S, L.ptr(nrm.view), L.ptr(out.view), L.stream())
    L.call("vag_l2norm_bwd", L.ptr(x), L.ptr(nrm.view), L.ptr(out.view), L.ptr(d_out), B, S, L.ptr(dx.view), L.stream())
    _sync()
    tag = (B, S)
    rn, ro = R.l2norm_fwd(R.Tr, inp["x"])
    n32 = _check("l2norm_fwd", "nrm", nrm, rn, tag)
    o32 = _check("l2norm_fwd", "out", out, ro, tag)
    _check("l2norm_bwd", "dx", dx, R.l2norm_bwd(R.Tr, inp["x"], n32, o32, inp["d_out"], 0), tag)
    if B > 1:                                          # the all-zero row: nrm is the clamp itself, out is 0 (bounds of 0 above)
        z = R.L2_ZERO_ROW
        assert n32[z] == np.float32(1e-12) and (o32[z] == 0).all() and rn.e[z] == 0 and (ro.e[z] == 0).all(), tag
        assert n32[4] == np.float32(1e-12) and (o32[4] != 0).all(), tag          # below the clamp without being zero


@pytest.mark.parametrize("B,K,S,act", R.PROJ_CASES, ids=_ids(R.PROJ_CASES))
def test_img_proj_l2_matches_fp64_per_element(B, K, S, act):
    L = _L()
    inp = R.proj_inputs(B, K, S, act)
    x, W, b = _in(inp["x"]), _in(inp["W"]), _in(inp["b"])
    y, nrm, out = _Out((B, S)), _Out((B,)), _Out((B, S))
    L.call("vag_img_proj_l2_fwd", L.ptr(x), L.ptr(W), L.ptr(b), B, K, S, act, L.ptr(y.view), L.ptr(nrm.view), L.ptr(out.view),
           L.stream())
    _sync()
    tag = (B, K, S, act)
    ref = R.proj_fwd(R.Tr, inp, act)
    saved = {k: _check("img_proj_l2_fwd", k, o, ref[k], tag) for k, o in (("y", y), ("nrm", nrm), ("out", out))}
    if B > 1 and not act:
        z = R.L2_ZERO_ROW
        assert saved["nrm"][z] == np.float32(1e-12) and (saved["out"][z] == 0).all() and (saved["y"][z] == 0).all(), tag
    rb = R.proj_bwd(R.Tr, inp, saved, act)
    for with_dx in (True, False):
        d_out, d_x = _Out((B, S), inp["d_out"]), _Out((B, K))
        gW, gb = _Out((S, K), inp["gW0"]), _Out((S,), inp["gb0"])
        L.call("vag_img_proj_l2_bwd", L.ptr(x), L.ptr(W), L.ptr(y.view), L.ptr(nrm.view), L.ptr(out.view), L.ptr(d_out.view), B, K, S,
               act, L.ptr(d_x.view) if with_dx else None, L.ptr(gW.view), L.ptr(gb.view), L.stream())
        _sync()
        t2 = tag + (("d_x" if with_dx else "no d_x"),)
        _check("img_proj_l2_bwd", "dy", d_out, rb["dy"], t2)
        _check("img_proj_l2_bwd", "g_W", gW, rb["g_W"], t2)
        _check("img_proj_l2_bwd", "g_b", gb, rb["g_b"], t2)
        if with_dx:
            _check("img_proj_l2_bwd", "d_x", d_x, rb["d_x"], t2)
        else:
            assert np.isnan(d_x.host("d_x", t2)).all(), t2


# ---------------------------------------------------------------------------------------------------------------- grounding attention
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=_ids(R.ATTN_CASES))
def test_imagine_attn_ctx_matches_fp64_per_element(case):
    method, row, B, Ts, C, S, acc = case
    L = _L()
    inp = R.attn_inputs(*case)
    im, enc, mask = _in(inp["im_emb"]), _in(inp["enc"]), _in(inp["mask"])
    cc, ec, d_ctx = _in(inp["ctx2ctx"]), _in(inp["emb2ctx"]), _in(inp["d_ctx"])
    mw = _in(inp["mlp_w"]) if method == 1 else None
    nws = int(L.lib().vag_imagine_ws_floats(B, Ts, C, S, method))
    ws = _Out((nws,))
    alpha, ctx = _Out((B, Ts)), _Out((B, C))
    d_enc = _Out((B, Ts, C), inp["d_enc0"] if acc else None)
    d_im = _Out((B, S))
    g_cc, g_ec = _Out((C, C), inp["g_cc0"]), _Out((C, S), inp["g_ec0"])
    g_mw = _Out((C,), inp["g_mlp0"]) if method == 1 else None
    try:
        L.set_option("attn_row", row)
        L.call("vag_imagine_attn_ctx_fwd", L.ptr(im), L.ptr(enc), L.ptr(mask), L.ptr(cc), L.ptr(ec), L.ptr(mw), method, B, Ts, C, S,
               L.ptr(alpha.view), L.ptr(ctx.view), L.ptr(ws.view), L.stream())
        L.call("vag_imagine_attn_ctx_bwd", L.ptr(im), L.ptr(enc), L.ptr(mask), L.ptr(cc), L.ptr(ec), L.ptr(mw), method, B, Ts, C, S,
               L.ptr(alpha.view), L.ptr(d_ctx), L.ptr(ws.view), L.ptr(d_enc.view), acc, L.ptr(d_im.view), L.ptr(g_cc.view),
               L.ptr(g_ec.view), L.ptr(g_mw.view) if g_mw else None, L.stream())
        _sync()
    finally:
        L.set_option("attn_row", 1)
    tag = case
    ws.host("ws", tag)                                                           # (the workspace's own extent)
    fwd = R.attn_fwd(R.Tr, inp, method)
    a32 = _check("imagine_attn_ctx_fwd", "alpha", alpha, fwd["alpha"], tag)
    on = inp["mask"] != 0
    assert (a32[~on] == 0).all(), ("weight on a masked position", tag)
    assert (np.abs(a32.astype(np.float64).sum(1) - 1.0) <= fwd["alpha"].e.sum(1) + Ts * R.U24).all(), ("rows of alpha do not sum to 1", tag)
    _check("imagine_attn_ctx_fwd", "ctx", ctx, fwd["ctx"], tag)
    bwd = R.attn_bwd(R.Tr, inp, a32, method, acc)
    outs = dict(d_enc=d_enc, d_im_emb=d_im, g_ctx2ctx=g_cc, g_emb2ctx=g_ec)
    if method == 1:
        outs["g_mlp_w"] = g_mw
    assert set(outs) == set(bwd)
    for k, o in outs.items():
        _check("imagine_attn_ctx_bwd", k, o, bwd[k], tag)


# ---------------------------------------------------------------------------------------------------------------- ranking loss
@pytest.mark.parametrize("B,S,kind", R.RANK_CASES, ids=_ids(R.RANK_CASES))
def test_rank_loss_matches_fp64_and_G_is_exact(B, S, kind):
    L = _L()
    inp = R.rank_inputs(B, S)
    margin = float(R.rank_margin(S))
    im, s = _in(inp["im"]), _in(inp["s"])
    scores, G, loss = _Out((B, B)), _Out((B, B)), _Out((1,))
    d_im, d_s = _Out((B, S)), _Out((B, S))
    d_loss = _in(np.array([R.RANK_D_LOSS], dtype=np.float32))
    L.call("vag_rank_loss_fwd", L.ptr(im), L.ptr(s), B, S, margin, kind, L.ptr(scores.view), L.ptr(G.view), L.ptr(loss.view), L.stream())
    L.call("vag_rank_loss_bwd", L.ptr(im), L.ptr(s), L.ptr(G.view), L.ptr(d_loss), B, S, L.ptr(d_im.view), L.ptr(d_s.view), L.stream())
    _sync()
    tag = (B, S, kind)
    fwd = R.rank_fwd(R.Tr, inp, R.rank_margin(S), kind)
    assert fwd["ambiguous"] == 0
    scores.host("scores", tag)
    G32 = G.host("G", tag)
    assert np.array_equal(G32.astype(np.float64), fwd["G"]), ("G differs at %d entries" % int((G32 != fwd["G"]).sum()), tag)
    _check("rank_loss_fwd", "loss", loss, R.TV(fwd["loss"].v.reshape(1), fwd["loss"].e.reshape(1)), tag)
    bwd = R.rank_bwd(R.Tr, inp, G32, R.RANK_D_LOSS)                              # d_loss = 0.37, applied once on either path
    _check("rank_loss_bwd", "d_im", d_im, bwd["d_im"], tag)
    _check("rank_loss_bwd", "d_s", d_s, bwd["d_s"], tag)


@pytest.mark.parametrize("kind", [2, 3])
def test_rank_loss_twin_flag_refuses_an_odd_batch(kind):
    L = _L()
    inp = R.rank_inputs(17, 60)
    im, s = _in(inp["im"]), _in(inp["s"])
    scores, G, loss = _Out((17, 17)), _Out((17, 17)), _Out((1,))
    rc = L.lib().vag_rank_loss_fwd(L.ptr(im), L.ptr(s), 17, 60, 0.3, kind, L.ptr(scores.view), L.ptr(G.view), L.ptr(loss.view), L.stream())
    _sync()
    assert rc == -22
    assert np.isnan(G.host("G", kind)).all() and np.isnan(loss.host("loss", kind)).all()      # refused before anything was launched


# ---------------------------------------------------------------------------------------------------------------- initial state
@pytest.mark.parametrize("case", R.INIT_CASES, ids=_ids(R.INIT_CASES))
def test_dec_init_matches_fp64_per_element(case):
    B, Ts, C, H, mode, split, acc = case
    L = _L()
    inp = R.init_inputs(*case)
    enc, mask, W, b = _in(inp["enc"]), _in(inp["mask"]), _in(inp["W"]), _in(inp["b"])
    ctx = _in(inp["ctx"]) if mode == "ctx" else None
    xmix, h0 = _Out((B, C)), _Out((B, H))
    L.call("vag_dec_init_fwd", L.ptr(enc), L.ptr(mask), L.ptr(ctx), split, L.ptr(W), L.ptr(b), B, Ts, C, H, L.ptr(xmix.view),
           L.ptr(h0.view), L.stream())
    _sync()
    tag = case
    fwd = R.init_fwd(R.Tr, inp, mode, split)
    saved = dict(xmix=_check("dec_init_fwd", "xmix", xmix, fwd["xmix"], tag), h0=_check("dec_init_fwd", "h0", h0, fwd["h0"], tag))
    d_h0 = _Out((B, H), inp["d_h0"])
    d_enc = _Out((B, Ts, C), inp["d_enc0"] if acc else None)
    d_ctx = _Out((B, C)) if mode == "ctx" else None
    gW, gb, scratch = _Out((H, C), inp["gW0"]), _Out((H,), inp["gb0"]), _Out((B, C))
    L.call("vag_dec_init_bwd", L.ptr(mask), L.ptr(xmix.view), L.ptr(h0.view), split, L.ptr(W), L.ptr(d_h0.view), B, Ts, C, H,
           L.ptr(d_enc.view), acc, L.ptr(d_ctx.view) if d_ctx else None, L.ptr(gW.view), L.ptr(gb.view), L.ptr(scratch.view), L.stream())
    _sync()
    bwd = R.init_bwd(R.Tr, inp, saved, mode, split, acc)
    d_h0.host("d_h0", tag)
    scratch.host("scratch", tag)
    _check("dec_init_bwd", "d_enc", d_enc, bwd["d_enc"], tag)                    # every position, past a row's length included
    _check("dec_init_bwd", "g_W", gW, bwd["g_W"], tag)
    _check("dec_init_bwd", "g_b", gb, bwd["g_b"], tag)
    if mode == "ctx":
        _check("dec_init_bwd", "d_ctx", d_ctx, bwd["d_ctx"], tag)


# ---------------------------------------------------------------------------------------------------------------- small riders
def test_retrieval_ranks_with_exact_ties_follow_a_stable_sort():
    L = _L()
    N, S = 9, 8
    rs = np.random.RandomState(5)
    q = rs.randint(-2, 3, size=(N, S)).astype(np.float32)                        # small integers: every score is exact
    k = rs.randint(-2, 3, size=(N, S)).astype(np.float32)
    k[5] = k[3]                                                                 # query 5 ties its own key with key 3 (before it),
    k[7] = k[8]                                                                 # query 7 with key 8 (after it: not counted)
    qd, kd = _in(q), _in(k)
    scores, ranks = _Out((N, N)), _Out((N,), dtype=torch.int32)
    L.call("vag_retrieval_ranks", L.ptr(qd), L.ptr(kd), N, S, L.ptr(scores.view), L.ptr(ranks.view, torch.int32), L.stream())
    _sync()
    sc = scores.host("scores", "ranks")
    want = q.astype(np.float64) @ k.astype(np.float64).T
    assert np.array_equal(sc.astype(np.float64), want)
    assert want[5, 5] == want[5, 3] and want[7, 7] == want[7, 8]
    assert ranks.host("ranks", "ranks").tolist() == R.retrieval_ranks_ref(want).tolist()


def test_gather_rows_i64_repeated_and_out_of_order():
    L = _L()
    N, ld, w = 6, 7, 5
    mat = np.arange(N * ld, dtype=np.int64).reshape(N, ld) * 1000003 + 7
    idx = np.array([4, 1, 4, 0, 5, 1, 1], dtype=np.int64)
    md, idd = _in(mat, torch.int64), _in(idx, torch.int64)
    out = _Out((len(idx), w), dtype=torch.int64)
    L.call("vag_gather_rows_i64", L.ptr(md, torch.int64), ld, L.ptr(idd, torch.int64), len(idx), w, L.ptr(out.view, torch.int64), L.stream())
    _sync()
    assert np.array_equal(out.host("out", "gather"), R.gather_rows_ref(mat, idx, w))


def test_zz_report_worst_ratios():
    """Runs last in this file: the largest |err| / bound per operator on the device (shown with -s)."""
    for op in sorted(WORST):
        print("device worst |err| / bound  %-24s %.3f" % (op, WORST[op]))
