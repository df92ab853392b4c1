"""Diverse beam search against the plain n-best search of the same width, timed at configs[3]'s decode shape (B 16, k 12,
max_length 80, the cfg2 model of bench.py; untrained, so all 80 steps run): microseconds per decode step of

    beamsearch_nbest(beam_size=12, n_best=12)                       the baseline (this change leaves it untouched)
    beamsearch_diverse(beam_size=12, n_groups=G, diversity=0.5)     G = 1, 3, 12

in graph mode (captured chunks of 8 steps) and in eager mode (launch by launch).  The plain search's captured steps expand raw
logits (no normalising pass); a diverse search runs the log-probability steps, so part of the difference is that pass and not
the grouped expansion: `nbest_logp` is the plain search with decode_raw_logits off, the like-for-like baseline.

Every figure: a host clock around `reps` whole decodes closed by a device synchronise, after a warm-up, divided by the steps run;
`windows` such windows per variant, the variants alternating inside every round, all windows reported (median, min, max).
It fails without a GPU.

Usage (GPU box):  python tools/exp_diverse.py [--rounds 3] [--reps 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
B, K, ML = 16, 12, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    if not torch.cuda.is_available():
        sys.exit("exp_diverse: needs a GPU")
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)

    def nbest(raw):
        def run():
            m.decode_raw_logits = raw
            m.beamsearch_nbest(src, lens, im, K, K, ML)
            m.decode_raw_logits = True
        return run

    def diverse(G):
        return lambda: m.beamsearch_diverse(src, lens, im, beam_size=K, n_groups=G, diversity=0.5, max_length=ML)
    variants = [("nbest", nbest(True)), ("nbest_logp", nbest(False)), ("diverse_G1", diverse(1)), ("diverse_G3", diverse(3)),
                ("diverse_G12", diverse(K))]
    lines = ["tools/exp_diverse.py on %s: B %d, beam %d, max_length %d, V %d; us per decode step, %d rounds x %d decodes per window"
             % (torch.cuda.get_device_name(0), B, K, ML, c["V"], a.rounds, a.reps)]
    for graph in (True, False):
        m.decode_graph = graph
        times = {name: [] for name, _ in variants}
        steps = {}
        for name, fn in variants:                      # warm-up: captures, code objects
            for _ in range(2):
                fn()
            steps[name] = int(m.last_decode_steps)
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for name, fn in (variants if r % 2 == 0 else variants[::-1]):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.reps / steps[name] * 1e6)
        lines.append("%s mode" % ("graph" if graph else "eager"))
        base = statistics.median(times["nbest_logp"])
        for name, _ in variants:
            xs = times[name]
            lines.append("  %-12s steps %3d  median %7.1f  min %7.1f  max %7.1f   %+6.1f us vs nbest_logp"
                         % (name, steps[name], statistics.median(xs), min(xs), max(xs), statistics.median(xs) - base))
    d1 = m.beamsearch_diverse(src, lens, im, beam_size=K, n_groups=1, max_length=ML)
    h, s = m.beamsearch_nbest(src, lens, im, K, K, ML)
    lines.append("n_groups=1 equals beamsearch_nbest (lists and score bits): %s" % bool(d1.hyps == h and torch.equal(d1.scores, s)))
    d3 = m.beamsearch_diverse(src, lens, im, beam_size=K, n_groups=3, diversity=0.5, max_length=ML)
    lines.append("distinct first words among the 12 hypotheses, mean over sentences: nbest %.2f, diverse_G3 %.2f"
                 % (sum(len({tuple(x[:1]) for x in hb}) for hb in h) / B, sum(len({tuple(x[:1]) for x in hb}) for hb in d3.hyps) / B))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
