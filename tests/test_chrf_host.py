"""CPU: the surface table, the host-side checks of the chrF utility (mbr_select / mbr_decode / mrt_step), the library's argument
checks, and the Python restatement of the definition (tests/chrf_ref.py) on cases whose value is known."""
import ctypes as C

import numpy as np
import pytest
import torch

import chrf_ref as R

WORDS = ["<pad>", "<unk>", "<s>", "</s>", "Haus", "tür@@", "en", "@@", "x@@@@", "@@y", "a b\tc", "ä", "\U0001F600", "", "ab@@ "]


def table():
    from vagnmt_hip.surface import Surface
    return Surface(WORDS)


def test_surface_construction():
    t = table()
    s = t.surfaces
    assert t.V == len(WORDS)
    assert s[0] == s[2] == s[3] == "" and s[1] == "<unk>"                 # padding, SOS, EOS are empty; UNK keeps its string
    assert s[4] == "Haus" and s[5] == "tür" and s[6] == "en"              # one trailing join marker stripped
    assert s[7] == "" and s[8] == "x@@" and s[9] == "@@y"                 # once, and only at the end
    assert s[10] == "abc"                                                 # whitespace dropped
    assert s[14] == "ab@@"                                                # "ab@@ " does not END in the marker: only the blank goes
    assert len(s[11]) == 1 and len(s[12]) == 1                            # multi-byte characters count once
    assert len("ä".encode()) == 2 and len("\U0001F600".encode()) == 4
    off, chars = t.host()
    assert off.dtype == torch.int32 and chars.dtype == torch.int32 and off.shape == (t.V + 1,)
    lens = [len(x) for x in s]
    assert off.tolist() == [0] + list(np.cumsum(lens))
    assert chars[:-1].tolist() == [ord(c) for x in s for c in x] and chars.shape == (sum(lens) + 1,)
    assert int(chars[off[12]]) == 0x1F600 and int(chars[off[11]]) == 0xE4
    assert t.max_len == 5 == len("<unk>")
    assert t.text([4, 5, 6, 3, 4]) == "Haustüren"                        # cut at EOS; BPE joins need nothing more
    assert t.text([0, 4, 0, 13]) == "Haus" and t.text([3, 4]) == "" and t.text([]) == ""


def test_surface_options_and_errors():
    from vagnmt_hip.surface import Surface
    t = Surface(["a@@", "b##", "c", "d"], join="##", empty=())
    assert t.surfaces == ["a@@", "b", "c", "d"]
    assert Surface(["a@@", "b"], join="", empty=()).surfaces == ["a@@", "b"]
    assert Surface(["x", "y", "z", "w"]).max_len == 1 and Surface(["x"]).max_len == 0
    for bad in ([], ["a", 3]):
        with pytest.raises(ValueError):
            Surface(bad)
    with pytest.raises(ValueError):
        Surface(["a"], join=None)


def test_select_args_checks():
    from vagnmt_hip import mbr
    t = table()
    x = torch.zeros(1, 2, 3, dtype=torch.int64)
    assert mbr.UTILITIES["chrf"] == 2 and mbr.UTILITIES["bleu"] == 0 and mbr.UTILITIES["ngram_f"] == 1
    with pytest.raises(ValueError, match="chrf.*surface"):
        mbr.mbr_select(x, utility="chrf")                                 # "chrf" without a surface
    with pytest.raises(ValueError, match="surface.*chrf"):
        mbr.mbr_select(x, utility="bleu", surface=t)                      # a surface with another utility
    with pytest.raises(ValueError, match="surface.*chrf"):
        mbr.select_args(x, utility="ngram_f", surface=t)
    with pytest.raises(ValueError, match="surface"):
        mbr.mbr_select(x, utility="chrf", surface=WORDS)                  # not a table
    with pytest.raises(ValueError, match="utility must be one of"):
        mbr.mbr_select(x, utility="meteor")                               # unknown names as before
    with pytest.raises(ValueError, match="utility must be one of"):
        mbr.mbr_select(x, utility="meteor", surface=t)
    # with a table the name is accepted, and the next check is the one every utility meets
    with pytest.raises(ValueError, match="no CPU path"):
        mbr.mbr_select(x, utility="chrf", surface=t)


def test_decode_args_checks():
    from vagnmt_hip import mbr
    t = table()
    assert mbr.decode_args(16, 80, 4, "chrf", t) == (4, 2)
    assert mbr.decode_args(16, 80, 4, "chrf", t, len(WORDS)) == (4, 2)
    assert mbr.decode_args(16, 80, 4, "ngram_f") == (4, 1)
    with pytest.raises(ValueError, match="mbr_decode.*chrf.*surface"):
        mbr.decode_args(16, 80, 4, "chrf")
    with pytest.raises(ValueError, match="mbr_decode.*surface.*chrf"):
        mbr.decode_args(16, 80, 4, "bleu", t)
    with pytest.raises(ValueError, match="mbr_decode.*utility must be one of"):
        mbr.decode_args(16, 80, 4, "meteor", t)
    with pytest.raises(ValueError, match="mbr_decode.*surface holds"):
        mbr.decode_args(16, 80, 4, "chrf", t, len(WORDS) + 1)             # ids the table does not cover
    with pytest.raises(ValueError, match="unsupported shape"):
        mbr.decode_args(1024, 10, 1, "chrf", t)


def test_mbr_decode_surface_checks_on_the_models():
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11, NMT_Seq2Seq_Beam_V2
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.surface import Surface
    m = NMT_AttentionImagine_Seq2Seq_Beam_V11(30, 40, 24, 8, 8, 16, 12, 0.99).eval()
    t = NMT_Seq2Seq_Beam_V2(30, 40, 8, 8, 16).eval()
    src = torch.randint(4, 30, (2, 5))
    im = torch.rand(2, 24)
    full, short = Surface(["w%d" % i for i in range(40)]), Surface(["w%d" % i for i in range(39)])
    for obj in (m, t, Ensemble([m, t])):
        for kw, word in ((dict(utility="chrf"), "chrf.*surface"), (dict(surface=full), "surface.*chrf"),
                         (dict(utility="chrf", surface=short), "surface holds 39"),
                         (dict(utility="chrf", surface=full), "GPU tensor")):       # everything in range, but a CPU src_var
            with pytest.raises(ValueError, match="mbr_decode.*" + word):
                obj.mbr_decode(src, [5, 5], im, **kw)


def test_mrt_check_args():
    from vagnmt_hip import mrt
    t = table()
    V = len(WORDS)
    src = torch.randint(4, 30, (2, 5))
    tgt = torch.tensor([[4, 5, 6, 3], [4, 3, 0, 0]])
    cand = torch.randint(4, V, (2, 3, 4))
    args = lambda tg, c: (src, tg, 3, 0.5, "sample", True, None, c, 1024, "mrt_step")      # noqa: E731
    with pytest.raises(ValueError, match="mrt_step: cost must be one of"):
        mrt.check_args(*args(tgt, cand), "ter", None)
    with pytest.raises(ValueError, match="mrt_step: cost 'chrf' needs surface"):
        mrt.check_args(*args(tgt, cand), "chrf", None)
    with pytest.raises(ValueError, match="mrt_step: surface goes with cost 'chrf' only"):
        mrt.check_args(*args(tgt, cand), "bleu", t)
    bad = cand.clone()
    bad[1, 2, 0] = V
    with pytest.raises(ValueError, match="candidates must hold ids in \\[0, %d\\)" % V):
        mrt.check_args(*args(tgt, bad), "chrf", t)
    badt = tgt.clone()
    badt[0, 0] = V + 5
    with pytest.raises(ValueError, match="tgt must hold ids"):
        mrt.check_args(*args(badt, cand), "chrf", t)
    # in range: the checks of every cost follow (CPU tensors are refused last), with or without the new arguments
    for extra in (("chrf", t), ("bleu", None), ()):
        with pytest.raises(ValueError, match="GPU tensors"):
            mrt.check_args(*args(tgt, cand), *extra)
    with pytest.raises(ValueError, match="expected_risk: cost 'chrf' needs surface"):
        mrt.expected_risk(None, src, [5, 5], tgt, None, cand, 0.5, cost="chrf")


def test_entry_points_on_the_host():
    from vagnmt_hip import _lib
    L = _lib.lib()
    Cmax = L.vag_chrf_max_chars()
    assert Cmax >= 1024
    assert L.vag_chrf_supported(1, 1, 1, 1) == 1 and L.vag_chrf_supported(1024, Cmax, 1024, Cmax) == 1
    for bad in ((0, 8, 2, 8), (2, 0, 2, 8), (2, 8, 0, 8), (2, 8, 2, 0), (1025, 8, 2, 8), (2, 8, 1025, 8), (2, Cmax + 1, 2, 8),
                (2, 8, 2, Cmax + 1)):
        assert L.vag_chrf_supported(*bad) == 0, bad
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    # argument errors come back as -EINVAL before anything touches a device (the pointers are never dereferenced)
    sel = lambda *a: L.vag_chrf_select(*a)      # noqa: E731
    assert sel(None, p, None, None, None, 1, 2, 8, 2, 8, None, None, p, p, None) == -22             # hchars NULL
    assert sel(p, None, None, None, None, 1, 2, 8, 2, 8, None, None, p, p, None) == -22             # hlens NULL
    assert sel(p, p, None, None, None, 1, 2, 8, 2, 8, None, None, None, p, None) == -22             # expected NULL
    assert sel(p, p, None, None, None, 1, 2, 8, 2, 8, None, None, p, None, None) == -22             # best NULL
    assert sel(p, p, p, None, None, 1, 2, 8, 2, 8, None, None, p, p, None) == -22                   # rchars without rlens
    assert sel(p, p, None, p, None, 1, 2, 8, 2, 8, None, None, p, p, None) == -22
    assert sel(p, p, None, None, None, 0, 2, 8, 2, 8, None, None, p, p, None) == -22                # a size below 1
    assert sel(p, p, None, None, None, 1, 2, 0, 2, 0, None, None, p, p, None) == -22
    assert sel(p, p, None, None, None, 1, 2, 8, 3, 8, None, None, p, p, None) == -22                # refs NULL: the shapes differ
    assert sel(p, p, None, None, None, 1, 2, 8, 2, 9, None, None, p, p, None) == -22
    assert sel(p, p, p, p, None, 1, 2, Cmax + 1, 2, 8, None, None, p, p, None) == -22               # an unsupported shape
    assert sel(p, p, p, p, None, 1, 1025, 8, 2, 8, None, None, p, p, None) == -22
    assert sel(p, p, p, p, None, 1 << 21, 2, 8, 2, 8, None, None, p, p, None) == -22
    exp = lambda *a: L.vag_surface_expand(*a)   # noqa: E731
    assert exp(None, 1, 4, p, p, 10, p, 8, p, None) == -22
    assert exp(p, 1, 4, None, p, 10, p, 8, p, None) == -22
    assert exp(p, 1, 4, p, None, 10, p, 8, p, None) == -22
    assert exp(p, 1, 4, p, p, 10, None, 8, p, None) == -22
    assert exp(p, 1, 4, p, p, 10, p, 8, None, None) == -22
    for R_, L_, V_, C_ in ((0, 4, 10, 8), (1, 0, 10, 8), (1, 4, 0, 8), (1, 4, 10, 0), (1, 513, 10, 8)):
        assert exp(p, R_, L_, p, p, V_, p, C_, p, None) == -22, (R_, L_, V_, C_)


def test_reference_sanity():
    assert R.matches("abcabc", "abcabc") == [6, 5, 4, 3, 2, 1] == R.totals(6)
    for s in ("a", "ab", "abcdef", "Haustüren" * 3):                     # identical strings give 1, in both precisions
        m = R.matches(s, s)
        assert R.utility64(m, len(s), len(s)) == 1.0 and R.utility32(m, len(s), len(s)) == np.float32(1.0), s
    m = R.matches("abcabc", "xyzxyzxyz")                                  # disjoint alphabets give 0
    assert m == [0] * 6 and R.utility64(m, 6, 9) == 0.0 and R.utility32(m, 6, 9) == 0.0
    for h, r in (("", "abc"), ("abc", ""), ("", "")):                     # an empty side gives 0
        m = R.matches(h, r)
        assert m == [0] * 6 and R.utility64(m, len(h), len(r)) == 0.0 and R.utility32(m, len(h), len(r)) == 0.0
    g = np.random.default_rng(0)
    for _ in range(50):                                                   # m_n is symmetric; the utility (beta = 2) is not
        h = "".join(g.choice(list("abc"), size=g.integers(0, 20)))
        r = "".join(g.choice(list("abc"), size=g.integers(0, 20)))
        assert R.matches(h, r) == R.matches(r, h)
        u = R.utility64(R.matches(h, r), len(h), len(r))
        assert 0.0 <= u <= 1.0 and abs(float(R.utility32(R.matches(h, r), len(h), len(r))) - u) <= 1e-6
    # clipping: "a" 70 times against a string that holds it 3 times
    assert R.matches("a" * 70, "abaca") == [3, 0, 0, 0, 0, 0] and R.matches("a" * 70, "aaab") == [3, 2, 1, 0, 0, 0]
    # a hand-computed value: h = "ab", r = "abc": orders 1, 2 effective; P = (2/2 + 1/1) / 2 = 1, R = (2/3 + 1/2) / 2 = 7/12
    assert R.utility64(R.matches("ab", "abc"), 2, 3) == pytest.approx(5 * (7 / 12) / (4 + 7 / 12), abs=1e-15)
    # one BPE segmentation or another: the same characters
    t = table()
    assert t.text([4, 5, 6]) == t.text([4, 5, 6, 3]) == "Haustüren"
