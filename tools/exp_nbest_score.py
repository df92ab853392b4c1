"""N-best finish and forced-decoding scores, timed.

1. the n-best finish kernel (vag_beam_finish_nbest, n = 1 and n = 12) against vag_beam_finish at B 16, k 12, max_len 80, on the
   search state a real configs[3]-shaped beam search left behind (untrained model: all 80 steps run);
2. score_translations throughput (sentences/s) at configs[1] size (B 64, Ts = Tt = 40, V 9391, H 512) for M = 1 and M = 3,
   next to the eval forward (model(..., teacher_force_ratio=1) under no_grad) of the same batch.
Every row: host clock around `reps` calls closed by a device synchronise, after a warm-up; median of `rounds`.

Usage (GPU box):  python tools/exp_nbest_score.py [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))

import torch  # noqa: E402


def timed(fn, reps, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return statistics.median(out), out


def model(seed, Vs, V, I, dev):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    torch.manual_seed(seed)
    return NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, V, I, 256, 256, 512, 512, 0.99, tied_emb=True).to(dev).eval()


def inputs(Vs, V, I, B, T, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    lens = sorted([int(x) for x in torch.randint(3, T + 1, (B,), generator=g)], reverse=True)
    lens[0] = T
    src = torch.zeros(B, T, dtype=torch.long)
    for b, L in enumerate(lens):
        src[b, :L] = torch.randint(4, Vs, (L,), generator=g)
    tgt = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        L = int(torch.randint(2, T + 1, (1,), generator=g))
        tgt[b, :L - 1] = torch.randint(4, V, (L - 1,), generator=g)
        tgt[b, L - 1] = 3
    im = torch.randn(B, I, generator=g).abs()
    return src.to(dev), lens, tgt.to(dev), im.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vagnmt_hip._lib import call, ptr, stream
    from vagnmt_hip.ensemble import Ensemble
    dev = torch.device("cuda:0")
    Vs, V, I = 8507, 9391, 2048
    res = {"device": torch.cuda.get_device_name(0)}

    # 1. finish kernels on a real search state
    m = model(1, Vs, V, I, dev)
    B, K, ML = 16, 12, 80
    src, lens, _, im = inputs(Vs, V, I, B, 40, dev)
    m.beamsearch_decode(src, lens, im, K, ML)
    st = [s for key, s in m._decode_cache.items() if key != "__pool__" and key[0] == "beam"][0]
    nll, beam, steps = st["nll"], st["beam"], m.last_decode_steps
    out1 = torch.empty(B, ML, dtype=torch.int64, device=dev)
    best = torch.empty(B, device=dev)
    res["finish_steps"] = steps

    def fin():
        call("vag_beam_finish", ptr(nll), ptr(beam, torch.int64), ML, steps, B, K, ptr(out1, torch.int64), ptr(best), stream())
    res["finish_us"] = timed(fin, 200, a.rounds)[0] * 1e6
    for n in (1, 12):
        outn = torch.empty(B, n, ML, dtype=torch.int64, device=dev)
        scn = torch.empty(B, n, device=dev)

        def finn():
            call("vag_beam_finish_nbest", ptr(nll), ptr(beam, torch.int64), ML, steps, B, K, n, ptr(outn, torch.int64), ptr(scn),
                 stream())
        res["finish_nbest%d_us" % n] = timed(finn, 200, a.rounds)[0] * 1e6
        if n == 1:
            fin()
            torch.cuda.synchronize()
            res["nbest1_equals_finish"] = bool(torch.equal(outn[:, 0], out1) and torch.equal(scn[:, 0], best))

    # 2. forced scores at configs[1] size
    B, T = 64, 40
    src, lens, tgt, im = inputs(Vs, V, I, B, T, dev, seed=5)
    ms = [m] + [model(s, Vs, V, I, dev) for s in (2, 3)]
    vw = torch.ones(V, device=dev)
    vw[0] = 0
    crit = torch.nn.NLLLoss(weight=vw, reduction="none")

    def fwd():
        with torch.no_grad():
            m(src, lens, tgt, im, 1.0, criterion_mt=crit)
    t_fwd = timed(fwd, 10, a.rounds)[0]
    res["eval_forward_ms"] = t_fwd * 1e3
    for M in (1, 3):
        obj = ms[0] if M == 1 else Ensemble(ms[:M])
        t = timed(lambda: obj.score_translations(src, lens, tgt, im), 10, a.rounds)[0]
        res["score_M%d_ms" % M] = t * 1e3
        res["score_M%d_sent_per_s" % M] = B / t
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
