"""CPU: what every exported function of the sequence operators' host layer (csrc/enc_api.hip, csrc/dec_api.hip) answers to an
argument list that breaks ONE of its conditions, pinned against tests/golden/seq_rejections.json (recorded from the library of the
commit before those functions left csrc/api.hip: `VAG_LIB=<that library> python tests/test_seq_args_host.py --record`).

Every call looks valid but for the one condition its name says (non-NULL 16-byte aligned pointers that are never dereferenced on
the host, consistent shapes), as in test_head_args_host.py.  The golden holds the return code per call: -22 where the function
rejects; where it does not check the condition, whatever the launch it then attempts returns on a machine without a device.  That is
why the module runs only without /dev/kfd, and why the only valid calls it makes are of the size and support queries, whose values
are pinned as they are.  `head` points at a real vag_head_w: the free-running forwards read its members on the host.

An entry marked "stricter" is one the branch rejects (-22) where the recorded library had already enqueued work before its check
(the check now stands in front of the first launch)."""
import ctypes as C
import json
import os
import sys

import pytest

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_rejections.json")
pytestmark = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a call that slips through must end in a no-device error")

PTR, OFF = 4096, 4100          # "valid-looking" and misaligned
GRU = ("w_ih", "w_hh", "b_ih", "b_hh")
DEC = ("emb",) + tuple("gru1." + m for m in GRU) + ("attn_h", "attn_v", "c2h") + tuple("gru2." + m for m in GRU)
HEAD = ("w1", "b1", "w2", "b2", "w3", "b3", "out_w", "out_b")
STRUCTS = {"fw": GRU, "bw": GRU, "g_fw": GRU, "g_bw": GRU, "W": DEC, "G": DEC, "head": HEAD}
DIMS = {"B": 4, "Ts": 3, "Tt": 3, "N": 4, "M": 4, "rows": 4, "E": 8, "H": 8, "C": 16, "V": 10, "ldl": 12, "rows_per_src": 1,
        "free_run": 0, "accumulate_enc": 0, "with_fp16": 0}
FLOATS = ("p_emb", "p_ctx", "p_out")
NEVER_SET = ("rng", "stream")          # NULL in every call: no dropout (p = 0), the default stream
SEQ_FWD = "enc pe mask h0 tok W B Ts Tt E H V h2_all c_all e_all ws %s head p_out rng tmid logits ldl %s stream"
SEQ_BWD = "enc pe mask h0 tok W B Ts Tt E H V h2_all c_all e_all d_h2_all d_c_all d_e_all ws d_enc_out accumulate_enc d_pe d_h0 %s scratch stream"
# function (+variant) -> (argument names in ABI order, arguments left NULL in the base call, dimensions the variant changes)
SPECS = {
    "vag_bigru_seq_fwd": ("src lengths emb fw bw p_emb p_ctx rng B Ts E H enc mask ws stream", (), {}),
    "vag_bigru_seq_bwd": ("src lengths fw bw p_emb p_ctx rng B Ts E H d_enc ws g_emb g_fw g_bw stream", (), {}),
    "vag_gru_cell_fwd": ("gi h_prev w_hh b_hh M H h_out save stream", (), {}),
    "vag_gru_cell_bwd": ("dgh_next w_hh_t carry d_out save h_prev M H dgi dgh carry_out stream", (), {}),
    "vag_attn_keys_proj": ("enc attn_e rows C pe stream", (), {}),
    "vag_bahdanau_attn_fwd": ("pe q v mask enc N rows_per_src Ts C scores alpha ctx stream", (), {}),
    "vag_attn_keys_proj_bwd": ("enc attn_e d_pe rows C d_enc accumulate_enc g_attn_e stream", (), {}),
    "vag_cgru_prepare": ("W H prep stream", (), {}),
    "vag_derive_weights": ("W enc_whh_fw enc_whh_bw H with_fp16 derived stream", (), {}),
    "vag_cgru_attn_decode_seq_fwd": (SEQ_FWD % ("free_run", ""), ("head", "tmid", "logits"), {}),
    "vag_cgru_attn_decode_seq_fwd+free": (SEQ_FWD % ("free_run", ""), (), {"free_run": 1}),
    "vag_cgru_attn_decode_free_fwd": (SEQ_FWD % ("", "tables"), (), {}),
    "vag_cgru_attn_decode_seq_bwd": (SEQ_BWD % "G", (), {}),
    "vag_cgru_attn_decode_seq_bwd_loop": (SEQ_BWD % "", (), {}),
    "vag_cgru_attn_decode_seq_bwd_weights": ("h0 tok W B Ts Tt E H h2_all c_all e_all d_e_all ws G scratch stream", (), {}),
    "vag_cgru_attn_decode_step": ("enc pe mask rows_per_src tok h_in W prep N Ts E H h_out c e alpha scratch stream", (), {}),
    "vag_cgru_decode_keys": ("enc prep w2 B Ts E H keys stream", (), {}),
    "vag_cgru_decode_tables": ("W w3 V E H tables stream", (), {}),
    "vag_cgru_attn_decode_step_h": ("pe mask keys tables V rows_per_src tok h_in W prep N Ts E H h_out cw e alpha scratch stream", ("tables",), {}),
    "vag_cgru_attn_decode_step_h+tables": ("pe mask keys tables V rows_per_src tok h_in W prep N Ts E H h_out cw e alpha scratch stream", ("e",), {}),
    "vag_cgru_recurrence_fwd": ("pe mask h0 xp1 W wcat bcat encwp B Ts Tt H h1 g1 qhp alpha h2_all g2 psc sync stream", (), {}),
}
STORE16 = ("vag_bigru_seq_fwd", "vag_bigru_seq_bwd", "vag_attn_keys_proj", "vag_cgru_attn_decode_seq_fwd",
           "vag_cgru_attn_decode_seq_fwd+free", "vag_cgru_attn_decode_seq_bwd", "vag_cgru_attn_decode_seq_bwd_loop")
# host-side queries that moved with them: valid calls, the value itself is pinned (sizes of every layout of seq_layout.h among them)
QUERIES = {
    "vag_bigru_ws_floats": [(5, 7, 16, 24), (64, 20, 256, 512)],
    "vag_cgru_ws_floats": [(5, 7, 6, 16, 24), (64, 20, 21, 256, 512)],
    "vag_cgru_ws_offset": [(5, 7, 6, 16, 24, w) for w in (0, 1, 2, 3)],
    "vag_cgru_bwd_scratch_floats": [(5, 7, 6, 16, 24), (64, 20, 21, 256, 512)],
    "vag_cgru_step_scratch_floats": [(1, 1, 4, 4), (5, 7, 16, 24), (257, 49, 256, 512)],
    "vag_cgru_prep_floats": [(24,), (512,)],
    "vag_derived_floats": [(24,), (512,)],
    "vag_cgru_free_supported": [(5, 7, 6, 16, 24, 60), (64, 20, 21, 256, 512, 8192)],
    "vag_cgru_free_tables_floats": [(5, 7, 6, 16, 24, 60), (64, 20, 21, 256, 512, 8192)],
    "vag_cgru_decode_keys_floats": [(5, 7, 16, 24), (64, 20, 256, 512)],
    "vag_cgru_decode_tables_floats": [(60, 16, 24), (8192, 256, 512)],
}


def _cases(key):
    """(case name, {argument or struct.member: value, "@ctx": (derived, storage)}) for one function: one broken condition each."""
    names, base_null, _ = SPECS[key]
    names = names.split()
    ptrs = [n for n in names if n not in DIMS and n not in STRUCTS and n not in FLOATS + NEVER_SET + tuple(base_null)]
    for n in ptrs:
        yield "null:" + n, {n: None}
        yield "misaligned:" + n, {n: OFF}
    for s in names:
        if s in STRUCTS and s not in base_null:
            if s == "head":
                yield "null:head", {"head": None}
            for m in STRUCTS[s]:
                yield "null:%s.%s" % (s, m), {s + "." + m: None}
    for n, bad in (("E", 10), ("H", 10), ("C", 0), ("B", 0), ("Ts", 0), ("Tt", 0), ("N", 0), ("M", 0), ("rows", 0), ("V", 0)):
        if n in names:
            yield ("%s%%4" % n if bad == 10 else "%s=0" % n), {n: bad}
    if "ldl" in names:
        yield "ldl<V", {"ldl": 8}
        yield "ldl%4", {"ldl": 14}
    if "rows_per_src" in names:
        yield "rows_per_src=0", {"rows_per_src": 0}
        yield "N%rows_per_src", {"rows_per_src": 3}
    if key.startswith("vag_cgru_attn_decode_step_h"):
        yield "N=257", {"N": 257}
    if key == "vag_derive_weights":
        yield "fp16:H%8", {"with_fp16": 1, "H": 12}
    if key in STORE16:
        # vag_set_operator_context refuses storage 1 without a derived buffer (its own entry below): the call then sees the defaults
        yield "s16:no-derived", {"@ctx": (None, 1)}
        yield "s16:H%8", {"@ctx": (PTR, 1), "H": 12}


def _struct(n, change):
    from vagnmt_hip import _lib
    v = lambda m: change.get(n + "." + m, PTR)      # noqa: E731
    if STRUCTS[n] is GRU:
        return _lib.GruW(*[v(m) for m in GRU])
    if STRUCTS[n] is HEAD:
        return _lib.HeadW(*[v(m) for m in HEAD])
    return _lib.DecW(v("emb"), _lib.GruW(*[v("gru1." + m) for m in GRU]), v("attn_h"), v("attn_v"), v("c2h"),
                     _lib.GruW(*[v("gru2." + m) for m in GRU]))


def _call(L, key, change):
    names, base_null, dims = SPECS[key]
    dims = dict(DIMS, **dims)
    args = []
    for n in names.split():
        if n in base_null and n not in change:
            args.append(None)
        elif n == "head":
            args.append(C.byref(_struct(n, change)) if change.get(n, PTR) else None)
        elif n in STRUCTS:
            args.append(_struct(n, change))
        elif n in dims:
            args.append(change.get(n, dims[n]))
        elif n in FLOATS:
            args.append(0.0)
        elif n in NEVER_SET:
            args.append(None)
        else:
            args.append(change.get(n, PTR))
    if "@ctx" in change:
        L.vag_set_operator_context(*change["@ctx"])
    try:
        return int(getattr(L, key.split("+")[0])(*args))
    finally:
        if "@ctx" in change:
            assert L.vag_set_operator_context(None, 0) == 0


def _all_calls(L):
    calls = {"%s %s" % (key, case): _call(L, key, change) for key in SPECS for case, change in _cases(key)}
    calls["vag_set_operator_context storage-without-derived"] = int(L.vag_set_operator_context(None, 1))
    for name, shapes in QUERIES.items():
        for shape in shapes:
            calls["%s query:%s" % (name, ",".join(map(str, shape)))] = int(getattr(L, name)(*shape))
    return calls


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_moved_function_is_covered():
    from vagnmt_hip import _lib
    moved = {n for n in _lib.PROTOS if n.startswith(("vag_bigru_", "vag_gru_cell_", "vag_attn_keys_", "vag_bahdanau_", "vag_cgru_", "vag_deriv"))}
    assert moved == {k.split("+")[0] for k in SPECS} | set(QUERIES)
    assert all(hasattr(_lib.lib(), n) for n in moved)


def test_golden_holds_one_call_per_condition(golden):
    want = {"%s %s" % (key, case) for key in SPECS for case, _ in _cases(key)}
    want |= {"%s query:%s" % (n, ",".join(map(str, s))) for n, shapes in QUERIES.items() for s in shapes}
    want.add("vag_set_operator_context storage-without-derived")
    assert set(golden["calls"]) == want
    assert set(golden["stricter"]) <= want
    # a stricter answer is allowed only where the recorded library went on to a launch
    assert all(golden["calls"][k] not in (0, -22) and " query:" not in k for k in golden["stricter"])


def test_rejections_match_the_recorded_library(golden):
    got = _all_calls(__import__("vagnmt_hip._lib", fromlist=["lib"]).lib())
    want = {k: (-22 if k in golden["stricter"] else rc) for k, rc in golden["calls"].items()}
    assert {k: (got[k], want[k]) for k in want if got[k] != want[k]} == {}


def test_no_call_of_a_launching_function_is_valid(golden):
    # every condition a function checks is rejected before anything is enqueued; what it does not check fails at the launch
    assert all(rc != 0 for k, rc in golden["calls"].items() if " query:" not in k)


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    from vagnmt_hip import _lib
    calls = _all_calls(_lib.lib())
    stricter = json.load(open(GOLDEN))["stricter"] if os.path.exists(GOLDEN) else []      # (marked by hand: kept)
    with open(GOLDEN, "w") as f:
        json.dump({"library": "vag_version %d" % _lib.lib().vag_version(), "calls": calls, "stricter": stricter}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(calls), "calls recorded from", _lib.LIB_PATH)
