"""Ensemble decoding at configs[3]'s decode shape (V = 9391, H = 512, E = 256, eval batch 16, beam 12, max_length 80, source
length 40): per-step time of the single-model beam search (the path bench.py's extra.beam12_decode times: raw-logit expansion),
of the single model on the log-probability path (what an ensemble member runs), and of ensembles of M = 1, 2, 3; greedy for the
single model and for M = 1, 3.  Every row is one configuration, timed in one process with the others, alternating, host clock
around whole decode calls closed by a device synchronise, after a warm-up; the per-step figure divides by the decoder steps
the call ran.  Members are untrained models of different seeds (no EOS bias: searches run the full 80 steps).

Usage (GPU box):  python tools/exp_ensemble_decode.py [--rounds 5] [--out FILE]
                  python tools/exp_ensemble_decode.py --profile   (one decode each of the single model on the log-probability
                  path and of the M = 3 ensemble: the run to trace, e.g.
                  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp_ensemble_decode.py --profile)"""
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

Vs, V, I, E, H, S, B, Ts, K, ML = 8507, 9391, 2048, 256, 512, 512, 16, 40, 12, 80


def models(n, dev):
    from machine_translation_vision.models import NMT_AttentionImagine_Seq2Seq_Beam_V11
    out = []
    for i in range(n):
        torch.manual_seed(1234 + i)
        out.append(NMT_AttentionImagine_Seq2Seq_Beam_V11(Vs, V, I, E, E, H, S, 0.99, attn_model="dot", tied_emb=True).to(dev).eval())
    return out


def batch(dev):
    g = torch.Generator().manual_seed(1234)
    lens = sorted(torch.clamp((torch.randn(B, generator=g) * 5 + 15).round().long(), 4, Ts).tolist(), reverse=True)
    lens[0] = Ts
    src = torch.randint(4, Vs, (B, Ts), generator=g)
    for b, L in enumerate(lens):
        src[b, L:] = 0
    return src.to(dev), lens, torch.randn(B, I, generator=g).abs().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="decode calls per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    from vagnmt_hip.ensemble import Ensemble
    dev = torch.device("cuda:0")
    ms = models(3, dev)
    src, lens, im = batch(dev)
    single_logp = models(1, dev)[0]
    single_logp.load_state_dict(ms[0].state_dict())
    single_logp.decode_raw_logits = False
    single_logp.decode_persistent = False
    rows = {
        "single_beam12 (raw-logit expansion, as extra.beam12_decode)": (ms[0], K),
        "single_beam12_logp (log-probability expansion)": (single_logp, K),
        "ens_M1_beam12": (Ensemble(ms[:1]), K),
        "ens_M2_beam12": (Ensemble(ms[:2]), K),
        "ens_M3_beam12": (Ensemble(ms[:3]), K),
        "single_greedy (one-launch persistent form)": (ms[0], 1),
        "single_greedy_graph (captured graph, as ensemble members run)": (single_logp, 1),
        "ens_M1_greedy": (Ensemble(ms[:1]), 1),
        "ens_M3_greedy": (Ensemble(ms[:3]), 1),
    }
    if a.profile:
        rows = {k: v for k, v in rows.items() if k.startswith(("single_beam12_logp", "ens_M3_beam12"))}

    def call(obj, k):
        return obj.beamsearch_decode(src, lens, im, beam_size=k, max_length=ML)

    for obj, k in rows.values():                 # warm-up: captures, code objects, allocator
        for _ in range(2):
            call(obj, k)
    torch.cuda.synchronize()
    if a.profile:
        for obj, k in rows.values():
            call(obj, k)
        torch.cuda.synchronize()
        print("profile run done:", list(rows))
        return
    times = {name: [] for name in rows}
    steps = {}
    for _ in range(a.rounds):
        for name, (obj, k) in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(obj, k)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.calls
            steps[name] = int(getattr(obj, "last_decode_steps", ML))
            times[name].append(dt / steps[name] * 1e6)
    res = {}
    lines = ["configs[3] decode shape: V=%d H=%d E=%d B=%d beam=%d max_length=%d Ts=%d; %d rounds x %d calls, alternating"
             % (V, H, E, B, K, ML, Ts, a.rounds, a.calls),
             "%-64s %10s %10s %10s %6s" % ("row", "median_us", "min_us", "max_us", "steps")]
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"us_per_step_median": med, "us_per_step_min": min(ts), "us_per_step_max": max(ts), "steps": steps[name]}
        lines.append("%-64s %10.1f %10.1f %10.1f %6d" % (name, med, min(ts), max(ts), steps[name]))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
