"""CPU: the single-product planner (gemm.hip: gemm_plan_single) through its host-only ABI view vag_gemm_plan.

tests/golden/gemm_plans.json holds the (T, split-K) pairs the library printed under vag_set_option("gemm_debug", 1) BEFORE the planner
became a function of its own (tools/record_gemm_plans.py against the `make LAB=1` library of that commit): every GEMM_CASES entry of
tests/test_gpu_gemm_paths.py with its options in all four operand layouts, and the dense products of one configs[1] training step
with beta 0 and 1, in the fp32 and in the 2-byte storage context.  The planner must still choose exactly those."""
import ctypes as C
import json
import os

import pytest

from conftest import ROOT

OPTS = ("gemm_force_tile", "gemm_force_splitk", "gemm_f32mfma")
TILED64, TILED128_F32, SPLIT128, BIG256 = 0, 1, 2, 3          # include/vag_nmt.h: VAG_GEMM_*


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")) as f:
        return json.load(f)


GOLDEN = _golden()


@pytest.fixture
def lib():
    from vagnmt_hip import _lib
    L = _lib.lib()
    yield L
    for k in OPTS:
        L.vag_set_option(k.encode(), 0)
    L.vag_set_operator_context(None, 0)


def _plan(L, e, planes=0, rowsum=0):
    for k in OPTS:
        assert L.vag_set_option(k.encode(), e["opts"].get(k, 0)) == 0
    assert L.vag_set_operator_context(C.c_void_p(4096) if e["storage"] else None, e["storage"]) == 0      # (never dereferenced)
    out = (C.c_int * 6)()
    rc = L.vag_gemm_plan(e["M"], e["N"], e["K"], e["a_kc"], e["b_kc"], e["vec"], e["beta"], e["act"], 0, 0, rowsum, planes, out)
    assert rc == 0, (rc, e)
    return dict(zip(("family", "T", "splitk", "slices", "kchunk", "rides"), out))


def test_golden_covers_what_it_should():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gemm_paths", os.path.join(ROOT, "tests", "test_gpu_gemm_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    have = {(e["id"], e["a_kc"], e["b_kc"]) for e in GOLDEN if not e["id"].startswith("step_")}
    assert have == {(c[0], int(a), int(b)) for c in mod.GEMM_CASES for a, b in mod.LAYOUTS}
    step = [e for e in GOLDEN if e["id"].startswith("step_")]
    assert {(e["storage"], e["beta"]) for e in step} == {(0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0)}
    assert len({e["id"] for e in step}) == 10


def test_planner_reproduces_every_recorded_choice(lib):
    for e in GOLDEN:
        p = _plan(lib, e)
        assert (p["T"], p["splitk"]) == (e["T"], e["splitk"]), (e, p)
        # what is launched: ceil(K / kchunk) slices of a whole number of 32-deep k-tiles, never more than the model asked for
        assert p["kchunk"] > 0 and p["kchunk"] % 32 == 0 and p["slices"] == -(-e["K"] // p["kchunk"]), (e, p)
        assert p["rides"] == 0
        if p["family"] != BIG256:
            assert p["slices"] <= p["splitk"] and p["family"] == {64: TILED64, 128: TILED128_F32 if e["opts"].get("gemm_f32mfma") else SPLIT128}[p["T"]], (e, p)


def _one(name, a_kc=1, b_kc=1):
    return next(e for e in GOLDEN if e["id"] == name and e["a_kc"] == a_kc and e["b_kc"] == b_kc)


def test_choices_quoted_in_the_gemm_paths_docstring(lib):
    """The planner's choices tests/test_gpu_gemm_paths.py relies on for its case -> kernel mapping (A and B k-contiguous)."""
    want = {"d_1x1x1": (64, 1), "d_63x64x31": (64, 1), "d_64x65x32": (64, 1), "d_65x63x33": (64, 1), "d_127x128x255": (64, 1),
            "d_128x127x1": (64, 1), "d_129x257x257": (64, 2), "d_257x129x2560": (64, 16), "f32_default_129x128x255": (64, 1),
            "off_default_129x65x2560": (64, 20), "tanh_forced_split_129x127x255": (64, 1)}
    for name, (T, slices) in want.items():
        p = _plan(lib, _one(name))
        assert (p["T"], p["slices"], p["family"]) == (T, slices, TILED64), (name, p)
    # the forced cases print their forced pair; seven slices over K = 31 are one k-tile of work
    for e in GOLDEN:
        if e["opts"].get("gemm_force_tile") and e["act"] == 0:
            p = _plan(lib, e)
            assert (p["T"], p["splitk"]) == (e["opts"]["gemm_force_tile"], e["opts"]["gemm_force_splitk"]), (e, p)
    p = _plan(lib, _one("t128s7_k31_64x63x31"))
    assert (p["T"], p["splitk"], p["slices"], p["family"]) == (128, 7, 1, SPLIT128)
    # vag_linear_fwd's products that reach the planner: y = x W^T, both k-contiguous
    fwd = {(257, 4096, 256, 0, 1): (128, 2), (65, 4096, 2048, 0, 1): (128, 16), (257, 130, 64, 1, 1): (64, 1), (64, 100, 63, 0, 0): (64, 1),
           (97, 4096, 255, 0, 0): (64, 1), (65, 130, 64, 0, 0): (64, 1), (200, 4096, 256, 0, 0): (64, 1)}
    for (M, N, K, act, vec), (T, slices) in fwd.items():
        e = dict(M=M, N=N, K=K, a_kc=1, b_kc=1, vec=vec, beta=0.0, act=act, storage=0, opts={})
        p = _plan(lib, e)
        assert (p["T"], p["slices"]) == (T, slices), (e, p)


def test_family_and_row_sums_by_planes(lib):
    """Which kernel family a plan names and whether A's row sums ride on it: the three-plane 128 x 128 kernel and the one-plane
    256 x 256 kernel carry them, everything else leaves them to a column-sum launch."""
    g = dict(M=2560, N=512, K=2560, a_kc=0, b_kc=0, vec=1, beta=1.0, act=0, storage=0, opts={})      # g_W += dY^T X
    p = _plan(lib, g, planes=3, rowsum=1)
    assert (p["family"], p["rides"]) == (SPLIT128, 1)
    assert _plan(lib, g, planes=2, rowsum=1)["rides"] == 0 and _plan(lib, g, planes=2)["family"] == SPLIT128
    for planes in (1, 11):
        p = _plan(lib, g, planes=planes, rowsum=1)
        assert (p["family"], p["rides"]) == (BIG256, 1) and p["slices"] == -(-g["K"] // p["kchunk"])
    assert _plan(lib, dict(g, vec=0), planes=1, rowsum=1)["family"] == SPLIT128          # unaligned operands: no 256 x 256 tile
    assert _plan(lib, dict(g, M=191), planes=1, rowsum=1)["rides"] == 0                  # below the 256-tile threshold
    assert _plan(lib, dict(g, opts={"gemm_f32mfma": 1}), planes=3, rowsum=1) ["family"] == TILED128_F32
    small = dict(g, M=64, N=64, K=64)
    assert (_plan(lib, small, planes=3, rowsum=1)["family"], _plan(lib, small, planes=3, rowsum=1)["rides"]) == (TILED64, 0)
    # the context's planes when none are given: 2 in the 2-byte storage context
    assert _plan(lib, dict(g, storage=1), rowsum=1)["rides"] == 0 and _plan(lib, g, rowsum=1)["rides"] == 1


def test_bad_arguments_are_einval(lib):
    out = (C.c_int * 6)()
    ok = (256, 256, 256, 1, 1, 1, 0.0, 0, 0, 0, 0, 3)
    assert lib.vag_gemm_plan(*ok, out) == 0
    assert lib.vag_gemm_plan(*ok, None) == -22
    for i, bad in ((0, 0), (1, -1), (2, 0), (0, 1 << 30), (11, 4), (7, 7)):
        a = list(ok)
        a[i] = bad
        assert lib.vag_gemm_plan(*a, out) == -22, a
    assert lib.vag_gemm_plan(256, 256, 256, 1, 1, 1, 1.0, 0, 1, 0, 0, 3, out) == -22      # fp16 output never accumulates
    assert lib.vag_gemm_plan(256, 256, 256, 1, 1, 1, 0.0, 0, 0, 0, 1, 3, out) == -22      # row sums need an outer-contiguous A
    assert lib.vag_gemm_plan(256, 256, 256, 1, 0, 1, 0.0, 0, 0, 1, 0, 3, out) == -22      # a bf16-stored A: one bf16 plane only
    assert lib.vag_gemm_plan(256, 256, 256, 1, 0, 1, 0.0, 0, 0, 1, 0, 1, out) == 0
    assert lib.vag_gemm_plan(64, 64, 256, 1, 0, 1, 0.0, 0, 0, 1, 0, 1, out) == -22        # ... and no 64 x 64 kernel takes it
