"""Every host-side workspace size and offset query, pinned to the values recorded in tests/golden/ws_layout.json: the
layouts are carved by one carver (csrc/kernels.h: WsCarver; DecTables, dec_keys) and a change there must not move a buffer
by accident.  Pure host calls, no device (as test_abi.py::test_workspace_size_queries_are_pure_host_calls relies on)."""
import ctypes as C
import itertools
import json
import os

from conftest import GOLDEN

# (B, Ts, Tt, E, H, V): the three benchmark configurations, the smallest shape, one past the free-table bound (B = 65), and one
# where nothing is a multiple of the 64-float granule
SHAPES = [(64, 40, 40, 256, 512, 9391), (16, 40, 40, 256, 256, 9391), (256, 40, 40, 512, 1024, 40000), (1, 1, 1, 4, 4, 5),
          (65, 40, 40, 256, 512, 9391), (33, 7, 5, 12, 8, 19)]
S, I = 512, 2048


def layout_queries(L, lib_mod):
    out = {}
    for B, Ts, Tt, E, H, V in SHAPES:
        q = {
            "vag_bigru_ws_floats": L.vag_bigru_ws_floats(B, Ts, E, H),
            "vag_cgru_ws_floats": L.vag_cgru_ws_floats(B, Ts, Tt, E, H),
            "vag_cgru_ws_offset": [L.vag_cgru_ws_offset(B, Ts, Tt, E, H, w) for w in range(3)],
            "vag_cgru_bwd_scratch_floats": L.vag_cgru_bwd_scratch_floats(B, Ts, Tt, E, H),
            "vag_cgru_prep_floats": L.vag_cgru_prep_floats(H),
            "vag_cgru_step_scratch_floats": L.vag_cgru_step_scratch_floats(B, Ts, E, H),
            "vag_cgru_free_tables_floats": L.vag_cgru_free_tables_floats(B, Ts, Tt, E, H, V),
            "vag_cgru_decode_keys_floats": L.vag_cgru_decode_keys_floats(B, Ts, E, H),
            "vag_cgru_decode_tables_floats": L.vag_cgru_decode_tables_floats(V, E, H),
            "vag_imagine_ws_floats": [L.vag_imagine_ws_floats(B, Ts, 2 * H, S, m) for m in (0, 1)],
            "vag_derived_floats": L.vag_derived_floats(H),
            "vag_recurrence_sync_words": {"kind%d_T%d" % (k, T): L.vag_recurrence_sync_words(k, B, T)
                                          for k in range(4) for T in sorted({Ts, Tt})},
        }
        step = {}
        for mm, am, st, fr in itertools.product((0, 1), repeat=4):
            c = lib_mod.StepCfg()
            c.B, c.Ts, c.Tt, c.Es, c.Et, c.H, c.S, c.I, c.V, c.ldl = B, Ts, Tt, E, E, H, S, I, V, (V + 3) // 4 * 4
            c.multimodal, c.attn_method, c.storage, c.free_run = mm, am, st, fr
            n = L.vag_step_ws_floats(C.byref(c))
            if n < 0:           # (cfg_ok refused the combination)
                continue
            step["mm%d_am%d_st%d_fr%d" % (mm, am, st, fr)] = {
                "vag_step_ws_floats": n, "vag_step_ws_offset": [L.vag_step_ws_offset(C.byref(c), w) for w in range(9)]}
        q["step"] = step
        out["B%d_Ts%d_Tt%d_E%d_H%d_V%d" % (B, Ts, Tt, E, H, V)] = q
    return out


def test_every_workspace_layout_query_matches_the_recorded_values():
    from vagnmt_hip import _lib
    with open(os.path.join(GOLDEN, "ws_layout.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(layout_queries(_lib.lib(), _lib)))
    assert sorted(got) == sorted(want)
    for shape in want:
        assert len(want[shape]["step"]) == 16
        for name in want[shape]:
            assert got[shape][name] == want[shape][name], (shape, name)
