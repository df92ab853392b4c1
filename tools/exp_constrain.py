"""Constrained beam search against the plain n-best search, timed at configs[3]'s decode shape (B 16, k 12, max_length 80, the
cfg2 model of bench.py; untrained, so all 80 steps run): microseconds per decode step of

    beamsearch_nbest(beam_size=12, n_best=1)                          the baseline (this feature leaves it untouched)
    beamsearch_constrained(beam_size=12, n_best=1, ...)               an empty set, a 3-word prefix, 64 phrases, no_repeat_ngram=3

in graph mode (captured chunks of 8 steps) and in eager mode (launch by launch).  The plain search's captured steps expand raw
logits (no normalising pass); a constrained search runs the log-probability steps, so part of the difference is that pass and
not the mask: `nbest_logp` is the plain search with decode_raw_logits off, the like-for-like baseline.  In graph mode every
constrained variant, the empty set included, runs the mask launch (on the entry's zero-padded static buffers); in eager mode the
empty set launches nothing.

Every figure: a host clock around `reps` whole decodes closed by a device synchronise, after a warm-up, divided by the steps run;
`rounds` such windows per variant, the variants alternating inside every round, all windows reported (median, min, max).
It fails without a GPU.

Usage (GPU box):  python tools/exp_constrain.py [--rounds 3] [--reps 5] [--out FILE]"""
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
        sys.exit("exp_constrain: needs a GPU")
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    V = c["V"]

    def nbest(raw):
        def run():
            m.decode_raw_logits = raw
            m.beamsearch_nbest(src, lens, im, K, 1, ML)
            m.decode_raw_logits = True
        return run

    def constrained(**kw):
        return lambda: m.beamsearch_constrained(src, lens, im, beam_size=K, n_best=1, max_length=ML, **kw)
    # the prefix: three distinct content words per sentence; the phrases: 64 bigrams of content words
    prefix = [[4 + (3 * b) % (V - 4), 4 + (3 * b + 1) % (V - 4), 4 + (3 * b + 2) % (V - 4)] for b in range(B)]
    phrases = [[4 + (7 * i) % (V - 4), 4 + (11 * i + 1) % (V - 4)] for i in range(64)]
    variants = [("nbest", nbest(True)), ("nbest_logp", nbest(False)), ("con_empty", constrained()),
                ("con_prefix3", constrained(prefix=prefix)), ("con_64phrases", constrained(banned=phrases)),
                ("con_ngram3", constrained(no_repeat_ngram=3))]
    lines = ["tools/exp_constrain.py on %s: B %d, beam %d, max_length %d, V %d; us per decode step, %d rounds x %d decodes per window"
             % (torch.cuda.get_device_name(0), B, K, ML, V, a.rounds, a.reps)]
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
            lines.append("  %-14s steps %3d  median %7.1f  min %7.1f  max %7.1f   %+6.1f us vs nbest_logp"
                         % (name, steps[name], statistics.median(xs), min(xs), max(xs), statistics.median(xs) - base))
    # at this size two runs of the plain search themselves agree in their lists but not in the last bits of their scores, so
    # the empty set is compared as two plain runs compare (bit for bit at small sizes: tests/test_gpu_constrain.py)
    m.decode_raw_logits = False
    h, s = m.beamsearch_nbest(src, lens, im, K, 1, ML)
    h2, s2 = m.beamsearch_nbest(src, lens, im, K, 1, ML)
    m.decode_raw_logits = True
    e = m.beamsearch_constrained(src, lens, im, beam_size=K, n_best=1, max_length=ML)
    lines.append("two runs of beamsearch_nbest on the log-probability steps: same lists %s, max abs score difference %.2e"
                 % (h == h2, (s - s2).abs().max().item()))
    lines.append("the empty set against beamsearch_nbest:                    same lists %s, max abs score difference %.2e"
                 % (e.hyps == h, (e.scores - s).abs().max().item()))
    p = m.beamsearch_constrained(src, lens, im, beam_size=K, n_best=1, max_length=ML, prefix=prefix)
    lines.append("every best hypothesis begins with its prefix: %s" % all(list(p.hyps[b][0][:3]) == prefix[b] for b in range(B)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
