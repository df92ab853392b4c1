#!/usr/bin/env python3
"""Generate tests/golden/beam_opts.npz by RUNNING THE REFERENCE's beam search with its two options (build container only).

Usage (from the repo root; the reference checkout must exist, it does not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_beam_opts.py

Loads the weights and inputs of three existing fixtures (mm_dot_tied_s0_f32, text_tied_s0_f32, mm_dot_tied_mid_f32) into the
reference models and calls their ``beamsearch`` (models/...V11.py:233, NMT_Seq2Seq_Beam_V2.py:173) with
(avoid_double, avoid_unk) in {(F,F), (T,T), (F,T)} and the default (T,F), for beam sizes 2, 3 and 12.  One more variant per
multimodal/text tiny case raises decoder.out.bias[UNK] so that UNK would win most steps without the avoid_unk mask.

Shims: oracle/make_golden.py's install_shims() plus ``UNK_token = 1`` on the V11 module (V11.py uses UNK_token at :284 but
never defines it; the text model defines it as 1, NMT_Seq2Seq_Beam_V2.py:15).

The fixture holds token lists only (JSON in a uint8 array) and the bias tweak: a few KB."""
import functools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.make_golden import REF, install_shims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam_opts.npz")
CASES = ["mm_dot_tied_s0_f32", "text_tied_s0_f32", "mm_dot_tied_mid_f32"]
OPTS = [(True, False), (False, False), (True, True), (False, True)]
BEAMS = (2, 3, 12)
UNK = 1
UNK_BIAS = 4.0           # added to decoder.out.bias[UNK] in the "unk" variants


def load(name):
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    meta = json.loads(bytes(z.pop("meta")).decode())
    return meta, z


def build(meta, z):
    import machine_translation_vision.models as M
    Vs, Vt, I, E, H, S, B, Ts, Tt = meta["dims"]
    if meta["kind"] == "mm":
        m = M.NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, Vt, I, E, E, H, S, meta["loss_w"], attn_model=meta["attn"],
                                                    tied_emb=meta["tied"], init_split=meta["init_split"])
    else:
        m = M.NMT_Seq2Seq_Beam_V2(Vs, Vt, E, E, H, tied_emb=meta["tied"])
    P = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("P/")}
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected and set(missing) <= {"decoder.out.weight"}, (missing, unexpected)
    return m.eval()


def decode(m, meta, z, k, max_len, ad, au):
    # beamsearch_decode calls self.beamsearch(enc, mask, input, hidden, beam_size, tgt_l) positionally (V11.py:229)
    m.beamsearch = functools.partial(type(m).beamsearch, m, avoid_double=ad, avoid_unk=au)
    src = torch.from_numpy(z["src"])
    with torch.no_grad():
        if meta["kind"] == "mm":
            hyp = m.beamsearch_decode(src, meta["lengths"], torch.from_numpy(z["im"]), k, max_len)
        else:
            hyp = m.beamsearch_decode(src, meta["lengths"], k, max_len)
    del m.beamsearch
    return [[int(t) for t in h] for h in hyp]


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    install_shims()
    import machine_translation_vision.models  # noqa: F401  (the package re-exports the class under the module's name)
    sys.modules["machine_translation_vision.models.NMT_AttentionImagine_Seq2Seq_Beam_V11"].UNK_token = UNK
    out = {"unk_bias": UNK_BIAS, "unk": UNK, "cases": []}
    for name in CASES:
        meta, z = load(name)
        for variant in ("plain", "unk"):
            if variant == "unk" and name == "mm_dot_tied_mid_f32":
                continue
            m = build(meta, z)
            if variant == "unk":
                with torch.no_grad():
                    m.decoder.out.bias[UNK] += UNK_BIAS
            max_len = meta["max_len"]
            dec = {}
            for k in BEAMS:
                for ad, au in OPTS:
                    dec["%d/%d%d" % (k, int(ad), int(au))] = decode(m, meta, z, k, max_len, ad, au)
            out["cases"].append({"fixture": name, "variant": variant, "max_len": max_len, "decode": dec})
            n_unk = sum(h.count(UNK) for h in dec["12/10"])
            print("%-22s %-5s max_len %d  UNK in the default k=12 lists: %d" % (name, variant, max_len, n_unk))
    np.savez_compressed(OUT, meta=np.frombuffer(json.dumps(out).encode(), dtype=np.uint8))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
