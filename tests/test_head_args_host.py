"""CPU: what every exported vag_head_* function answers to an argument list that breaks ONE of its conditions, pinned against
tests/golden/head_rejections.json (recorded from the library of the commit before the head's host layer moved into
csrc/head_api.hip: `VAG_LIB=<that library> python tests/test_head_args_host.py --record`).

Every call looks valid but for the one condition its name says (non-NULL 16-byte aligned pointers that are never dereferenced
on the host, consistent shapes), as in test_label_smoothing_host.py::_ls_calls.  The golden holds the return code per call: -22
where the function rejects; where it does not check the condition, whatever the launch it then attempts returns on a machine
without a device.  That is why the module runs only without /dev/kfd, and why it makes no valid call of a function that
launches (vag_head_logits_parts_count is a host-side query: it answers 0, or its count where the broken member is one it does not read).

An entry marked "stricter" is one the single validator of head_api.hip now rejects (-22) although the recorded library went on
to launch with a NULL pointer among its operands."""
import ctypes as C
import json
import os
import sys

import pytest

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_rejections.json")
pytestmark = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a call that slips through must end in a no-device error")

PTR, OFF = 4096, 4100          # "valid-looking" and misaligned
MEMBERS = ("w1", "b1", "w2", "b2", "w3", "b3", "out_w", "out_b")
DIMS = {"B": 4, "Tt": 3, "R": 12, "N": 4, "E": 8, "H": 8, "V": 10, "ldl": 12, "logits_ready": 0}
SEQ_FWD = "h2 c e W tgt vw B Tt E H V p_out rng logits_ready tmid logits ldl lse nll inv_cnt loss_mt"
SEQ_BWD = "h2 c e W tgt vw B Tt E H V p_out rng tmid logits ldl lse inv_cnt d_loss d_h2 d_c d_e G scratch"
SEQ_BWD_DATA = "W tgt vw B Tt E H V p_out rng tmid logits ldl lse inv_cnt d_loss d_h2 d_c d_e scratch"
STEP_H = "h2 cw e tables tok W N E H V %s ldl %s scratch stream"
# function (+variant) -> argument names in ABI order, arguments left NULL in the base call
SPECS = {
    "vag_head_ce_seq_fwd": (SEQ_FWD + " stream", ()),
    "vag_head_ce_seq_fwd_ls": (SEQ_FWD + " eps stream", ()),
    "vag_head_ce_seq_bwd": (SEQ_BWD + " stream", ()),
    "vag_head_ce_seq_bwd_ls": (SEQ_BWD + " eps stream", ()),
    "vag_head_ce_seq_bwd_data": (SEQ_BWD_DATA + " stream", ()),
    "vag_head_ce_seq_bwd_data_ls": (SEQ_BWD_DATA + " eps stream", ()),
    "vag_head_bwd_weights": ("h2 c e R E H V tmid dlogits ldl dt G stream", ()),
    "vag_head_logp_seq_fwd": ("h2 c e W R E H V p_out rng tmid logp ldl stream", ()),
    "vag_head_logp_seq_bwd": ("h2 c e W R E H V p_out rng tmid logp d_logp ldl d_h2 d_c d_e G scratch stream", ()),
    "vag_head_logp_step": ("h2 c e W N E H V logp ldl argmax scratch stream", ()),
    "vag_head_logp_step_h": (STEP_H % ("logp", "argmax"), ("tables", "tok")),
    "vag_head_logp_step_h+tables": (STEP_H % ("logp", "argmax"), ("e",)),
    "vag_head_logits_step_h": (STEP_H % ("logits", "parts"), ("tables", "tok")),
    "vag_head_logits_step_h+tables": (STEP_H % ("logits", "parts"), ("e",)),
    "vag_head_logits_step": ("h2 c e W N E H V logits ldl parts scratch stream", ()),
    "vag_head_logits_parts_count": ("W N E V", ()),
}
NEVER_SET = ("rng", "stream")          # NULL in every call: no dropout (p_out = 0), the default stream
MAY_BE_NULL = ("argmax",)              # optional outputs: present in the base call, not a condition


def _cases(key):
    """(case name, {argument or W.member / G.member: value}) for one function: one broken condition each."""
    names, base_null = SPECS[key]
    names = names.split()
    ptrs = [n for n in names if n not in DIMS and n not in ("W", "G", "p_out", "eps") + NEVER_SET + tuple(base_null)]
    for n in ptrs:
        if n not in MAY_BE_NULL:
            yield "null:" + n, {n: None}
        yield "misaligned:" + n, {n: OFF}
    for s in ("W", "G"):
        if s in names:
            for m in MEMBERS:
                yield "null:%s.%s" % (s, m), {s + "." + m: None}
                yield "misaligned:%s.%s" % (s, m), {s + "." + m: OFF}
    if "E" in names:
        yield "E%4", {"E": 10}
    if "H" in names:
        yield "H%4", {"H": 10}
    if "ldl" in names:
        yield "ldl<V", {"ldl": 8}
        yield "ldl%4", {"ldl": 14}
    if "N" in names:
        yield "N=257", {"N": 257}
    rows = "B" if "B" in names else "R" if "R" in names else "N"
    yield rows + "=0", {rows: 0}
    if "eps" in names:
        for e in (-0.1, 1.0, float("nan")):
            yield "eps=%r" % e, {"eps": e}


def _call(L, key, change):
    from vagnmt_hip import _lib
    names, base_null = SPECS[key]
    dims = dict(DIMS, N=128, E=256, V=4096) if key == "vag_head_logits_parts_count" else DIMS
    args = []
    for n in names.split():
        if n in ("W", "G"):
            args.append(_lib.HeadW(*[change.get(n + "." + m, PTR) for m in MEMBERS]))
        elif n in dims:
            args.append(change.get(n, dims[n]))
        elif n == "p_out":
            args.append(0.0)
        elif n == "eps":
            args.append(C.c_float(change.get(n, 0.1)))
        elif n in NEVER_SET or (n in base_null and n not in change):
            args.append(None)
        else:
            args.append(change.get(n, PTR))
    return int(getattr(L, key.split("+")[0])(*args))


def _all_calls(L):
    return {"%s %s" % (key, case): _call(L, key, change) for key in SPECS for case, change in _cases(key)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_exported_head_function_is_covered():
    from vagnmt_hip import _lib
    exported = {n for n in _lib.PROTOS if n.startswith("vag_head_")}
    assert exported == {k.split("+")[0] for k in SPECS}
    assert all(hasattr(_lib.lib(), n) for n in exported)


def test_golden_holds_one_call_per_condition(golden):
    want = {"%s %s" % (key, case) for key in SPECS for case, _ in _cases(key)}
    assert set(golden["calls"]) == want
    assert set(golden["stricter"]) <= want
    # a stricter answer is allowed only where the recorded library launched with a NULL or misaligned pointer
    assert all(k.split(" ")[1].startswith(("null:", "misaligned:")) and golden["calls"][k] != -22 for k in golden["stricter"])


def test_rejections_match_the_recorded_library(golden):
    got = _all_calls(__import__("vagnmt_hip._lib", fromlist=["lib"]).lib())
    want = {k: (-22 if k in golden["stricter"] else rc) for k, rc in golden["calls"].items()}
    assert {k: (got[k], want[k]) for k in want if got[k] != want[k]} == {}


def test_no_call_is_valid(golden):
    # every condition a function checks is rejected before anything is enqueued; what it does not check fails at the launch
    assert all(rc != 0 or k.startswith("vag_head_logits_parts_count ") for k, rc in golden["calls"].items())


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    from vagnmt_hip import _lib
    calls = _all_calls(_lib.lib())
    stricter = json.load(open(GOLDEN))["stricter"] if os.path.exists(GOLDEN) else []      # (marked by hand: kept)
    with open(GOLDEN, "w") as f:
        json.dump({"library": "vag_version %d" % _lib.lib().vag_version(), "calls": calls, "stricter": stricter}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(calls), "calls recorded from", _lib.LIB_PATH)
