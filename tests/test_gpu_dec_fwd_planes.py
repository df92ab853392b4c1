"""GPU: the teacher-forced decoder forward hands h1 and h2 off as MARKED bf16 planes (persist.hip: dec_fwd_persistent_kernel<.., PL>,
st_planes2_marked / ld_planes_marked, bit 3 of the option "handoff_planes").

The producer splits its values once; the split is elementwise and the accumulation order is unchanged, so the plane form must give
the bits of the fp32 form.  What makes torch.equal a fair demand: the forward's scores are sums of fp32 atomics, so two runs of ONE
form differ in the last bits -- the bit-for-bit tests therefore run with the attention vector v = 0.  Every share is then exactly 0
and alpha exactly 1 / len, while q, hp2, both cells and both hand-offs are ordinary numbers; q is compared directly through qhp.

 1. mask 31 against mask 23 (bit 3 off), same inputs, a plane buffer full of 0xFF each: torch.equal on h1, h2_all, g1, g2, qhp, alpha
    and c_all, no give-up of a wait; the arms are what they say (mask 31 wrote exactly the decoder forward's region, mask 23 nothing);
 2. the zero-word path, deterministic: z-gate biases of both cells + 40, so that vag_sigmoid returns exactly 1 and h1 = h2 = h0 at
    every step, and h0 from {0, +-1/8, +-1/4, +-1/2}: plane 2 of every word is zero and all planes are where h0 = 0 -- every one of
    those words travels as 0x80008000;
 3. a second call on the same buffer (now full of the first call's marks) gives the same bits: the library zeroes the region itself;
    a buffer one float short of vag_handoff_planes_floats succeeds in the fp32 form with the same bits;
 4. with the real v: the decoder-forward checks of tests/test_gpu_recurrences.py (its case table, _dec_run and bounds against the
    fp64 references) for every one-launch case that sets a plane buffer, with bit 3 on.

Per shape and input kind every call is made once and left unchanged; the tests only compare what the calls left."""
import pytest
import torch

from test_gpu_handoff_planes import E, _dec_w, _inputs, _planes

pytestmark = pytest.mark.gpu

# H, B, Ts, Tt: WGS = 32, KS = 1, 13 rows past the batch | a second tile with one valid row | full tiles at the workload's Ts | two
# passes of row tiles (rt0 != 0) | Tt = 1: no h2 block is ever consumed
SHAPES = [(256, 3, 5, 3), (512, 17, 7, 3), (512, 64, 40, 2), (512, 112, 4, 3), (512, 5, 3, 1)]
DEFAULT = 15
ON, OFF = 31, 23
NAMES = ("h1", "h2_all", "g1", "g2", "qhp", "alpha", "c_all")


def _r64(n):
    return (n + 63) // 64 * 64


def _region(H, B, Ts, Tt):
    """(first float, floats) of the decoder forward's region: [2][Tt][row tiles] blocks of 16 x H values, 6 bytes each, behind the
    encoder forward's [2][Ts][row tiles] blocks"""
    RT = (B + 15) // 16
    return 2 * Ts * RT * 16 * H * 6 // 4, 2 * Tt * RT * 16 * H * 6 // 4


def _dec_inputs(H, B, Ts, Tt, kind):
    d = _inputs(H, B, Ts, Tt)
    d["dec"][5] = torch.zeros_like(d["dec"][5])                 # v = 0: every score share is exactly 0, alpha exactly 1 / len
    if kind == "zero words":
        g = torch.Generator().manual_seed(5 + B)
        for b_hh in (d["dec"][3], d["dec"][10]):                 # b_hh of gru_1 and of gru_2: z = vag_sigmoid(>= 30) = 1 exactly
            b_hh[H:2 * H] = 40.0
        levels = torch.tensor([0.0, 0.125, -0.125, 0.25, -0.25, 0.5, -0.5])
        d["h0"] = levels[torch.randint(0, len(levels), (B, H), generator=g)].cuda()
        d["h0"][0, :8] = 0.0                                     # whole 8-byte pieces of zeros, whatever the draw
    return d


def _forward(d, H, B, Ts, Tt, mask, planes):
    """the decoder's forward with `planes` as the caller's buffer: the compared tensors, cloned"""
    from vagnmt_hip import _lib as L
    from vagnmt_hip._lib import ptr
    from test_gpu_round3 import _dirty
    C = 2 * H
    lib = L.lib()
    L.set_option("handoff_planes", mask)
    # the input projections in front of the recurrence run one by one and unsplit: no split-K partial sums meet in memory
    for name, value in (("gemm_force_tile", 128), ("gemm_force_splitk", 1), ("gemm_nogroup", 1)):
        L.set_option(name, value)
    try:
        ws = _dirty(lib.vag_cgru_ws_floats(B, Ts, Tt, E, H))
        hseq = _dirty(Tt + 1, B, H)
        hseq[0].copy_(d["h0"])
        h2, c, e = hseq[1:], _dirty(Tt, B, C), _dirty(Tt, B, E)
        with _planes(planes):
            L.call("vag_cgru_attn_decode_seq_fwd", ptr(d["keys"]), ptr(d["pe"]), ptr(d["mask"]), ptr(hseq[0]), ptr(d["tok"], torch.int64),
                   _dec_w(d["emb_t"], d["dec"]), B, Ts, Tt, E, H, d["Vt"], ptr(h2), ptr(c), ptr(e), ptr(ws), 0, None, 0.0, None, None,
                   None, 0, L.stream())
        torch.cuda.synchronize()
    finally:
        L.set_option("handoff_planes", DEFAULT)
        for name in ("gemm_force_tile", "gemm_force_splitk", "gemm_nogroup"):
            L.set_option(name, 0)
    R = Tt * B
    g1 = _r64(R * 3 * H)                                         # kernels.h WsCarver: xp1 | g1 | g2 | qhp | ...
    g2 = g1 + _r64(4 * R * H)
    off = {"alpha": lib.vag_cgru_ws_offset(B, Ts, Tt, E, H, 0), "h1": lib.vag_cgru_ws_offset(B, Ts, Tt, E, H, 1),
           "qhp": lib.vag_cgru_ws_offset(B, Ts, Tt, E, H, 2), "g1": g1, "g2": g2}
    assert off["qhp"] == g2 + _r64(4 * R * H)                    # the mirror above is the library's layout
    size = {"alpha": R * Ts, "h1": R * H, "qhp": R * 5 * H, "g1": 4 * R * H, "g2": 4 * R * H}
    out = {name: ws[off[name]:off[name] + size[name]].clone() for name in off}
    out["h2_all"], out["c_all"] = h2.clone(), c.clone()
    return out


_CACHE = {}


def _case(shape, kind):
    """name of a call -> (outputs, words of the plane buffer that are not 0xFFFFFFFF: in front of the region, in it, behind it)"""
    if (shape, kind) in _CACHE:
        return _CACHE[(shape, kind)]
    from vagnmt_hip import _lib as L
    H, B, Ts, Tt = shape
    assert L.lib().vag_recurrence_supported(1, B, Ts, Tt, H) == 1
    d = _dec_inputs(H, B, Ts, Tt, kind)
    n = L.lib().vag_handoff_planes_floats(B, Ts, Tt, H)
    first, floats = _region(H, B, Ts, Tt)
    assert floats == L.lib().vag_dec_fwd_planes_floats(B, Tt, H) and 0 < first + floats <= n
    L.lib().vag_persistent_timeouts()

    def fresh():
        return torch.full((n,), -1, dtype=torch.int32, device="cuda").view(torch.float32)

    def run(mask, planes):
        out = _forward(d, H, B, Ts, Tt, mask, planes)
        w = planes.view(torch.int32) != -1
        return out, (int(w[:first].sum()), int(w[first:first + floats].sum()), int(w[first + floats:].sum()))
    res = {}
    buf = fresh()
    res["on"] = run(ON, buf)
    res["off"] = run(OFF, fresh())
    if kind == "ordinary":
        res["off again"] = run(OFF, fresh())                     # the demand is fair: the fp32 form repeats its own bits
        res["on again"] = run(ON, buf)                           # on the marks the first call left
        res["short"] = run(ON, fresh()[:n - 1])
    res["timeouts"] = L.lib().vag_persistent_timeouts()
    res["region floats"] = floats
    _CACHE[(shape, kind)] = res
    return res


def _same(a, b, what):
    differ = {name: int((a[name] != b[name]).sum()) for name in NAMES}
    for name in NAMES:
        print("%-10s %-7s %9d values, %d differ, largest %.3e" % (what, name, a[name].numel(), differ[name], float(a[name].abs().max())))
    for name in NAMES:
        assert torch.isfinite(a[name]).all() and torch.isfinite(b[name]).all(), (what, name)
        assert torch.equal(a[name], b[name]), (what, name, differ[name])
        assert float(a[name].abs().max()) > 0.0, (what, name)    # the comparison is not one of zeros


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_marked_planes_give_the_bits_of_the_fp32_hand_off(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt), "ordinary")
    assert res["timeouts"] == 0
    # the arms are what they say: every word of the region was written (rows past the batch and the last step's h2 included), and
    # nothing else of the buffer; the fp32 form left the buffer alone
    assert res["on"][1] == (0, res["region floats"], 0)
    assert res["off"][1] == (0, 0, 0)
    _same(res["off again"][0], res["off"][0], "23 vs 23")         # v = 0 and unsplit products: nothing is summed in a changing order
    _same(res["on"][0], res["off"][0], "31 vs 23")
    alpha = res["on"][0]["alpha"].view(Tt, B, Ts)
    assert torch.equal(alpha[0], alpha[-1]) and float((alpha[0].sum(1) - 1).abs().max()) < 1e-6      # v = 0: 1 / len at every step


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_words_of_zeros_travel_as_marked_zeros(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt), "zero words")
    assert res["timeouts"] == 0
    assert res["on"][1] == (0, res["region floats"], 0)
    on, off = res["on"][0], res["off"][0]
    _same(on, off, "zero words")
    # the inputs did what they are for: both states of every step are h0 with the mark bit of the hand-off
    h0 = _dec_inputs(H, B, Ts, Tt, "zero words")["h0"]
    marked = (h0.view(torch.int32) | 1).view(torch.float32)
    for name in ("h1", "h2_all"):
        assert torch.equal(on[name].view(Tt, B, H), marked.expand(Tt, B, H)), name
    assert int((h0 == 0).sum()) >= 8


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES)
def test_a_second_call_and_a_short_buffer_give_the_same_bits(H, B, Ts, Tt):
    res = _case((H, B, Ts, Tt), "ordinary")
    assert res["timeouts"] == 0
    assert res["on again"][1] == (0, res["region floats"], 0)
    _same(res["on again"][0], res["on"][0], "again")
    assert res["short"][1] == (0, 0, 0)                          # one float short of the query: the fp32 form, the buffer left alone
    _same(res["short"][0], res["on"][0], "short")


def _plane_cases():
    import recur_ref as R
    return [c for c in R.DEC_CASES if c.one_launch and c.planes and not c.opt]


def _id(c):
    return "-".join(str(x) for x in c[:-1] if x is not None).replace(" ", "")


@pytest.mark.parametrize("case", _plane_cases(), ids=_id)
def test_plane_form_with_the_real_v_against_the_fp64_references(case):
    """tests/test_gpu_recurrences.py's own run of a decoder case -- the forward against the free-running and the one-step fp64
    reference, the backward (where the case has one) against its own -- with bit 3 of the option on.  Its `planes` cases set a buffer
    of vag_handoff_planes_floats, so the forward takes the plane form."""
    from vagnmt_hip import _lib as L
    from test_gpu_recurrences import _dec_run
    L.set_option("handoff_planes", ON)
    try:
        _dec_run(case, False)
    finally:
        L.set_option("handoff_planes", DEFAULT)
