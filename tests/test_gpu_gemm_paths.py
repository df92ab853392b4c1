"""Every path of the dense-product dispatcher (gemm.hip: vag_gemm_launch; skinny.hip: vag_skinny_launch, vag_skinny_nn_launch) against a
float64 product of the same fp32 inputs, element by element, through the public ABI only: vag_gemm_f32, vag_linear_fwd and
vag_linear_bwd, with the path steered by vag_set_option ("gemm_force_tile", "gemm_force_splitk", "gemm_f32mfma").

Error bound, per element: |got - ref| <= 2^-21 * (|alpha| (|A||B|) + |beta| |C0| + |bias|) -- an fp32 dot product of length K
(the bound test_gpu_round4.py::test_tall_skinny_vocabulary_product_is_fp32_grade uses); no bound relative to max|ref|, which
would hide errors on small elements.  With act = tanh the device tanh (common.h: vag_tanh, 1 - 2 rcp(exp(2x) + 1) on the fast
exp and reciprocal) adds its own absolute error: a few ulp of 1 (about 2^-23, from the final 1 - ...); TANH_ABS allows 2^-20.
tanh' <= 1, so the argument's error passes through unscaled.

Guard bands catch reads and writes outside the logical extents:
  * C is (M + 2) x ldc with ldc = N + 5; the pad columns and the two extra rows hold a sentinel and must come back bit-identical;
  * A and B have a leading dimension larger than the logical one (rounded up to a multiple of 4, plus 4, so that the vectorised
    path stays reachable) and one extra row / column; every pad float is NaN, so an unmasked over-read shows up as NaN;
  * beta = 0: the live part of C starts as NaN (the kernel must not read it) and the result must be finite.

Kernels the planner sends a product to (vag_gemm_launch; an ABI call never queues into a group bracket and has no slab scratch):
  T = 64                     gemm_tiled_kernel<64, 64, AKC, BKC, VEC, 256>   exact f32-input MFMA, split-K through fp32 atomics
  T = 128, gemm_f32mfma 0    gemm_split_kernel<AKC, BKC, VEC, 3>           bf16x6 three-plane MFMA, split-K through atomics
  T = 128, gemm_f32mfma 1    gemm_tiled_kernel<128, 128, AKC, BKC, VEC, 512> exact f32-input MFMA
  VEC = both operands 16-byte aligned and both leading dimensions % 4 == 0; a one-float offset forces the scalar loads.
vag_linear_fwd (api.hip: linear_fwd): M <= 256 -> vag_skinny_launch, which takes skinny_tall_kernel (M > 96, N >= 4096,
K % 256 == 0, no activation), the tiled kernels (K % 4 != 0, misaligned x, M > 64 with M N K > 350e6) or skinny_plain_go
(skinny_plain_mn_kernel for M >= 128, 256 < K <= 1024 and >= 192 tiles of 32 x 64; else skinny_plain_kernel<4 / 8 / 16> by
K <= 256 / <= 1024 / more); M > 256 -> vag_gemm_launch.
vag_linear_bwd: d_x through gemm_nn: M <= 128 -> vag_skinny_nn_launch, skinny_bt_kernel<4 / 8 / 16> by the reduction length
(the layer's N) <= 256 / <= 1024 / more, or the tiled kernels when N % 4 != 0; M > 128 -> vag_gemm_launch.  g_W through
vag_gemm_launch with beta = 1, g_b through colsum_kernel.
The mapping of each case below to its kernel follows the dispatch conditions in gemm.hip, skinny.hip and api.hip quoted above.  Where
the planner decides (no forced tile), tests/test_gemm_plan_host.py asserts its choice through vag_gemm_plan (no device needed), A and
B k-contiguous: d_1x1x1, d_63x64x31, d_64x65x32, d_65x63x33, d_127x128x255, d_128x127x1 -> T = 64, one slice; d_129x257x257 ->
T = 64, 2 slices; d_257x129x2560 -> T = 64, 16 slices; f32_default_129x128x255 -> T = 64, one slice; off_default_129x65x2560 ->
T = 64, 20 slices; tanh_forced_split_129x127x255 -> T = 64, one slice (the forced pair is ignored under tanh).  The forced cases
print their forced pair (t128s7_k31 included: 7 requested, one k-tile of work).  vag_linear_fwd: 257x4096x256 -> T = 128,
2 slices; 65x4096x2048 -> T = 128, 16 slices; 257x130x64 tanh, 64x100x63, 97x4096x255, misaligned 65x130x64 and 200x4096x256
-> T = 64, one slice; the skinny cases print nothing (they never reach vag_gemm_launch)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -21
TANH_ABS = 2.0 ** -20
SENTINEL = -7.25e9             # pad value of C: exactly representable, never a result here
DEV = "cuda:0"


def _L():
    from vagnmt_hip import _lib
    return _lib


class _Opts:
    """vag_set_option for the duration of a case; every option is put back to its default in the finally."""
    DEFAULTS = {"gemm_force_tile": 0, "gemm_force_splitk": 0, "gemm_f32mfma": 0}

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _L().set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.DEFAULTS.items():
            _L().set_option(k, v)
        return False


def _ld(n):
    return (n + 3) // 4 * 4 + 4


def _padded(mat, outer, inner, off):
    """mat (outer, inner) into a flat NaN buffer: `outer + 1` rows of ld = _ld(inner), starting `off` floats in.
    Returns (whole buffer, pointer-view at the first element, ld)."""
    ld = _ld(inner)
    buf = torch.full((off + (outer + 1) * ld,), float("nan"), dtype=torch.float32)
    buf[off:off + outer * ld].view(outer, ld)[:, :inner] = torch.from_numpy(np.ascontiguousarray(mat))
    buf = buf.to(DEV)
    return buf, buf[off:], ld


def _run_gemm(M, N, K, a_kc, b_kc, alpha=1.0, beta=0.0, bias=False, act=0, off=0, seed=0, **opts):
    L = _L()
    rs = np.random.RandomState(seed * 7919 + M * 31 + N * 7 + K)
    A = rs.randn(M, K).astype(np.float32)
    Bm = rs.randn(K, N).astype(np.float32)
    C0 = rs.randn(M, N).astype(np.float32)
    bv = rs.randn(N).astype(np.float32) if bias else None
    # A(m, k) = A[m sam + k sak]; B(k, n) = B[k sbk + n sbn]
    if a_kc:
        _, Ap, lda = _padded(A, M, K, off)
        sam, sak = lda, 1
    else:
        _, Ap, lda = _padded(A.T, K, M, off)
        sam, sak = 1, lda
    if b_kc:
        _, Bp, ldb = _padded(Bm.T, N, K, off)
        sbk, sbn = 1, ldb
    else:
        _, Bp, ldb = _padded(Bm, K, N, off)
        sbk, sbn = ldb, 1
    ldc = N + 5
    Ch = torch.full((M + 2, ldc), SENTINEL, dtype=torch.float32)
    Ch[:M, :N] = torch.from_numpy(C0) if beta != 0.0 else float("nan")
    Ct = Ch.to(DEV)
    bt = torch.from_numpy(bv).to(DEV) if bias else None
    with _Opts(**opts):
        L.call("vag_gemm_f32", M, N, K, alpha, L.ptr(Ap), sam, sak, L.ptr(Bp), sbk, sbn, beta, L.ptr(Ct), ldc, L.ptr(bt), act,
               L.stream())
        torch.cuda.synchronize()
    out = Ct.cpu()
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    ref = alpha * (A64 @ B64)
    bound = abs(alpha) * (np.abs(A64) @ np.abs(B64))
    if beta != 0.0:
        ref = ref + beta * C0
        bound = bound + abs(beta) * np.abs(C0)
    if bias:
        ref = ref + bv
        bound = bound + np.abs(bv)
    bound = EPS * bound
    if act:
        ref = np.tanh(ref)
        bound = bound + TANH_ABS
    got = out[:M, :N].double().numpy()
    tag = dict(M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc, alpha=alpha, beta=beta, bias=bias, act=act, off=off, **opts)
    assert np.isfinite(got).all(), ("non-finite result (read outside A / B, or C read with beta = 0)", tag)
    err = np.abs(got - ref)
    assert (err <= bound).all(), ("worst err / bound %.3g" % float((err / bound).max()), tag)
    pad = torch.cat([out[:M, N:].reshape(-1), out[M:, :].reshape(-1)])
    assert bool((pad == SENTINEL).all()), ("write outside C", tag)


LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]

# (id, M, N, K, keyword arguments of _run_gemm) -- the kernel each case targets in the comment
GEMM_CASES = [
    # planner default
    ("d_1x1x1", 1, 1, 1, {}),                                            # gemm_tiled 64 (M, N <= 64: the 128 tile is never planned)
    ("d_63x64x31", 63, 64, 31, {}),                                      # gemm_tiled 64, M / N / K one short of a tile
    ("d_64x65x32", 64, 65, 32, {}),                                      # gemm_tiled 64, N one past a tile
    ("d_65x63x33", 65, 63, 33, dict(bias=True)),                         # gemm_tiled 64, bias
    ("d_127x128x255", 127, 128, 255, {}),                                # gemm_tiled 64 (planner's choice at 127 x 128)
    ("d_129x257x257", 129, 257, 257, dict(alpha=0.5, beta=1.0)),         # gemm_tiled 64, 2 atomic slices onto C, alpha / beta
    ("d_257x129x2560", 257, 129, 2560, {}),                              # gemm_tiled 64, 16 slices: fill2d over NaN C + atomics
    ("d_128x127x1", 128, 127, 1, dict(bias=True)),                       # gemm_tiled 64, K = 1
    # forced tile / split-K
    ("t64s1_127x129x33", 127, 129, 33, dict(gemm_force_tile=64, gemm_force_splitk=1)),              # gemm_tiled 64
    ("t64s3_65x257x255", 65, 257, 255, dict(gemm_force_tile=64, gemm_force_splitk=3)),              # gemm_tiled 64, 3 slices: fill + atomics
    ("t64s3_bias_63x129x257", 63, 129, 257, dict(bias=True, gemm_force_tile=64, gemm_force_splitk=3)),  # bias added once over 3 slices
    ("t64s3_acc_129x65x2560", 129, 65, 2560, dict(alpha=0.5, beta=1.0, gemm_force_tile=64, gemm_force_splitk=3)),  # atomics onto C
    ("t128s1_129x127x257", 129, 127, 257, dict(gemm_force_tile=128, gemm_force_splitk=1)),          # gemm_split (bf16x6), one slice
    ("t128s1_1x257x32", 1, 257, 32, dict(bias=True, gemm_force_tile=128, gemm_force_splitk=1)),     # gemm_split with one live row
    ("t128s2_257x257x2560", 257, 257, 2560, dict(alpha=0.5, beta=1.0, gemm_force_tile=128, gemm_force_splitk=2)),  # gemm_split, 2 atomic slices onto C
    ("t128s2_bias_128x64x255", 128, 64, 255, dict(bias=True, gemm_force_tile=128, gemm_force_splitk=2)),  # gemm_split, bias once
    ("t128s7_128x129x2560", 128, 129, 2560, dict(bias=True, gemm_force_tile=128, gemm_force_splitk=7)),  # gemm_split, 7 slices, bias once
    ("t128s7_k31_64x63x31", 64, 63, 31, dict(gemm_force_tile=128, gemm_force_splitk=7)),            # K < one k-tile: 7 collapses to 1
    # exact f32-input MFMA
    ("f32_default_129x128x255", 129, 128, 255, dict(gemm_f32mfma=1)),                               # planner with f32mfma: gemm_tiled 64
    ("f32_t128s1_257x65x33", 257, 65, 33, dict(bias=True, gemm_f32mfma=1, gemm_force_tile=128, gemm_force_splitk=1)),  # gemm_tiled 128 f32
    ("f32_t128s3_257x129x2560", 257, 129, 2560, dict(gemm_f32mfma=1, gemm_force_tile=128, gemm_force_splitk=3)),  # gemm_tiled 128 f32 + split-K
    ("f32_t128s2_acc_128x128x257", 128, 128, 257, dict(alpha=0.5, beta=1.0, gemm_f32mfma=1, gemm_force_tile=128,
                                                        gemm_force_splitk=2)),                       # f32 128, atomics onto C
    ("f32_t64s3_65x127x255", 65, 127, 255, dict(gemm_f32mfma=1, gemm_force_tile=64, gemm_force_splitk=3)),  # gemm_tiled 64
    # tanh: never split (a forced split is ignored, the forced tile with it)
    ("tanh_65x64x33", 65, 64, 33, dict(bias=True, act=1)),                                           # gemm_tiled 64 + tanh
    ("tanh_forced_split_129x127x255", 129, 127, 255, dict(bias=True, act=1, gemm_force_tile=128, gemm_force_splitk=4)),  # -> gemm_tiled 64
    ("tanh_t128s1_acc_257x129x257", 257, 129, 257, dict(alpha=0.5, beta=1.0, bias=True, act=1, gemm_force_tile=128,
                                                       gemm_force_splitk=1)),                        # gemm_split + tanh
    # operands one float off 16-byte alignment: the scalar (non-VEC) loads
    ("off_t64s1_127x129x33", 127, 129, 33, dict(off=1, gemm_force_tile=64, gemm_force_splitk=1)),   # gemm_tiled 64, !VEC
    ("off_t128s2_257x257x255", 257, 257, 255, dict(off=1, bias=True, gemm_force_tile=128, gemm_force_splitk=2)),  # gemm_split, !VEC
    ("off_default_129x65x2560", 129, 65, 2560, dict(off=1, alpha=0.5, beta=1.0)),                 # gemm_tiled 64, !VEC, 20 slices onto C
    ("off_f32_t128s1_128x129x32", 128, 129, 32, dict(off=1, gemm_f32mfma=1, gemm_force_tile=128, gemm_force_splitk=1)),  # f32 128, !VEC
]


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS, ids=["AkBk", "AkBn", "AmBk", "AmBn"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_f32_path_matches_fp64_per_element(case, a_kc, b_kc):
    _, M, N, K, kw = case
    _run_gemm(M, N, K, a_kc, b_kc, **kw)


def _flat(host, off, tail, fill=float("nan")):
    """host tensor into a flat device buffer `off` floats in, followed by `tail` floats of `fill`; (buffer, view at the data)."""
    n = host.numel()
    buf = torch.full((off + n + tail,), fill, dtype=torch.float32)
    buf[off:off + n] = host.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf[off:off + n]


# (M, N, K, act, x offset, kernel) for vag_linear_fwd; y = act(x W^T + b)
LINEAR_FWD_CASES = [
    (1, 48, 64, 0, 0),              # skinny_plain_kernel<4>
    (64, 200, 512, 1, 0),           # skinny_plain_kernel<8>, tanh
    (65, 100, 2048, 0, 0),          # skinny_plain_kernel<16>
    (96, 4096, 256, 0, 0),          # skinny_plain_kernel<4>: M = 96 is below the tall-skinny switch
    (97, 4096, 256, 0, 0),          # skinny_tall_kernel: M > 96, N >= 4096
    (97, 4096, 256, 1, 0),          # tanh: never the tall kernel -> skinny_plain_kernel<4>
    (255, 1536, 512, 0, 0),         # skinny_plain_mn_kernel (M >= 128, 256 < K <= 1024, 24 x 8 tiles)
    (256, 4100, 512, 0, 0),         # skinny_tall_kernel at M = 256, ragged N
    (257, 4096, 256, 0, 0),         # M > 256: vag_gemm_launch
    (257, 130, 64, 1, 0),           # M > 256: vag_gemm_launch with tanh
    (64, 100, 63, 0, 0),            # K % 4 != 0: tiled gemm_tiled 64
    (97, 4096, 255, 0, 0),          # K % 4 != 0 at the tall shape: tiled
    (65, 130, 64, 0, 1),            # x misaligned: tiled, !VEC
    (200, 4096, 256, 0, 1),         # x misaligned at the tall shape: tiled
    (64, 4096, 2048, 0, 0),         # M <= 64: skinny_plain_kernel<16> whatever M N K
    (65, 4096, 2048, 0, 0),         # M > 64, M N K = 545e6 > 350e6: tiled
]


@pytest.mark.parametrize("M,N,K,act,off", LINEAR_FWD_CASES)
def test_linear_fwd_path_matches_fp64_per_element(M, N, K, act, off):
    L = _L()
    g = torch.Generator().manual_seed(M * 1009 + N * 13 + K + act)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    _, xp = _flat(x, off, K)                 # one NaN row past x and W: an over-read turns into NaN
    _, Wp = _flat(W, 0, K)
    bt = b.to(DEV)
    ybuf, yp = _flat(torch.full((M, N), float("nan")), 0, 257, fill=SENTINEL)
    L.call("vag_linear_fwd", M, N, K, L.ptr(xp), L.ptr(Wp), L.ptr(bt), act, L.ptr(yp), L.stream())
    torch.cuda.synchronize()
    out = ybuf.cpu()
    got = out[:M * N].view(M, N).double()
    x64, W64, b64 = x.double(), W.double(), b.double()
    ref = x64 @ W64.t() + b64
    bound = EPS * (x64.abs() @ W64.abs().t() + b64.abs())
    if act:
        ref = torch.tanh(ref)
        bound = bound + TANH_ABS
    assert bool(torch.isfinite(got).all()), (M, N, K, act, off)
    assert bool(((got - ref).abs() <= bound).all()), (M, N, K, act, off, float(((got - ref).abs() / bound).max()))
    assert bool((out[M * N:] == SENTINEL).all()), ("write past y", M, N, K)


# (M rows, N layer outputs = d_x's reduction length, K layer inputs, act, accumulate_dx, with d_x) for vag_linear_bwd
LINEAR_BWD_CASES = [
    (64, 256, 100, 1, 0, True),      # skinny_bt_kernel<4> (N <= 256), tanh: dy rewritten in place
    (128, 1024, 60, 0, 1, True),     # skinny_bt_kernel<8> (N <= 1024) at M = 128, accumulating d_x
    (33, 1028, 48, 1, 1, True),      # skinny_bt_kernel<16> (N > 1024)
    (37, 1030, 52, 0, 0, True),      # N % 4 != 0: tiled
    (129, 256, 100, 1, 0, True),     # M > 128: tiled
    (129, 1024, 65, 0, 1, True),     # M > 128, accumulating
    (1, 20, 12, 1, 0, True),         # one row
    (70, 300, 90, 1, 0, False),      # d_x = NULL: g_W, g_b only
]


@pytest.mark.parametrize("M,N,K,act,acc,with_dx", LINEAR_BWD_CASES)
def test_linear_bwd_path_matches_fp64_autograd(M, N, K, act, acc, with_dx):
    L = _L()
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    dx0 = torch.randn(M, K, generator=g) if acc else torch.full((M, K), float("nan"))
    gW0 = torch.randn(N, K, generator=g)
    gb0 = torch.randn(N, generator=g)
    # fp64 autograd from the fp32 values the kernel sees (y: the forward's output rounded to fp32)
    x64 = x.double().requires_grad_(True)
    W64 = W.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    pre = x64 @ W64.t() + b64
    y32 = (torch.tanh(pre) if act else pre).detach().float()
    # d(pre) = dy (1 - y^2) at the fp32 y the kernel reads (what tanh's backward computes from the saved output), then autograd
    dpre_ref = dy.double() * (1.0 - y32.double() ** 2) if act else dy.double()
    pre.backward(dpre_ref)
    _, xp = _flat(x, 0, K)
    _, Wp = _flat(W, 0, K)
    _, yp = _flat(y32, 0, N)
    _, dyp = _flat(dy, 0, N)
    dxbuf, dxp = _flat(dx0, 0, 64, fill=SENTINEL)
    gWbuf, gWp = _flat(gW0, 0, 64, fill=SENTINEL)
    gbbuf, gbp = _flat(gb0, 0, 64, fill=SENTINEL)
    L.call("vag_linear_bwd", M, N, K, L.ptr(xp), L.ptr(Wp), L.ptr(yp), L.ptr(dyp), act, L.ptr(dxp) if with_dx else None, acc,
           L.ptr(gWp), L.ptr(gbp), L.stream())
    torch.cuda.synchronize()
    tag = (M, N, K, act, acc, with_dx)
    # dy: rewritten in place as dy (1 - y^2) with act, untouched without
    dy_got = dyp.cpu().view(M, N).double()
    if act:
        assert bool(((dy_got - dpre_ref).abs() <= EPS * dy.double().abs()).all()), tag
    else:
        assert torch.equal(dy_got.float(), dy), tag
    # (|dy| bounds |dy (1 - y^2)|: the rounding of 1 - y^2 near |y| = 1 is absolute, not relative)
    ady = dy.double().abs()
    checks = [("g_W", gWbuf, gW0.double() + W64.grad, gW0.double().abs() + ady.t() @ x64.detach().abs(), N * K),
              ("g_b", gbbuf, gb0.double() + b64.grad, gb0.double().abs() + ady.sum(0), N)]
    if with_dx:
        base = dx0.double() if acc else torch.zeros(M, K, dtype=torch.float64)
        checks.append(("d_x", dxbuf, base + x64.grad, base.abs() + ady @ W64.detach().abs(), M * K))
    for name, buf, want, mag, n in checks:
        out = buf.cpu()
        got = out[:n].view_as(want).double()
        assert bool(torch.isfinite(got).all()), (name, tag)
        assert bool(((got - want).abs() <= EPS * mag).all()), (name, tag, float(((got - want).abs() / (EPS * mag)).max()))
        assert bool((out[n:] == SENTINEL).all()), ("write past " + name, tag)
