"""Beam search with required phrases against the plain n-best search, timed at configs[3]'s decode shape (B 16, k 12,
max_length 80, the cfg2 model of bench.py; untrained, so all 80 steps run): microseconds per decode step of

    beamsearch_nbest(beam_size=12, n_best=1)                          the product path (raw logits; this feature leaves it untouched)
    beamsearch_nbest on the log-probability steps                     the baseline: the steps a required search runs
    beamsearch_required(beam_size=12, n_best=1, required=...)         0, 2 and 8 phrases per sentence

in graph mode (captured chunks of 8 steps) and in eager mode (launch by launch).  A required search always runs its own
expansion (vag_beam_req_step: a row-aligned stage 1 and one workgroup per sentence that builds and ranks the pool), with no
phrases too; what it adds to the plain expansion is that second stage.

Every figure: a host clock around `reps` whole decodes closed by a device synchronise, after a warm-up, divided by the steps run;
`rounds` such windows per variant, the variants alternating inside every round, all windows reported (median, min, max).
It fails without a GPU.

Usage (GPU box):  python tools/exp_require.py [--rounds 3] [--reps 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
B, K, ML = 16, 12, 80


def contains(h, ph):
    return any(list(h[i:i + len(ph)]) == list(ph) for i in range(len(h) - len(ph) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    if not torch.cuda.is_available():
        sys.exit("exp_require: needs a GPU")
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

    def required(n):
        # n bigrams of distinct content words per sentence (8: 16 words of the 79 a hypothesis has)
        req = [[[4 + (13 * b + 2 * i) % (V - 4), 4 + (13 * b + 2 * i + 1) % (V - 4)] for i in range(n)] for b in range(B)]
        return req, (lambda: m.beamsearch_required(src, lens, im, beam_size=K, n_best=1, max_length=ML, required=req))
    variants = [("nbest", nbest(True)), ("nbest_logp", nbest(False))] + [("req_%dphrases" % n, required(n)[1]) for n in (0, 2, 8)]
    lines = ["tools/exp_require.py on %s: B %d, beam %d, max_length %d, V %d; us per decode step, %d rounds x %d decodes per window"
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
    m.decode_graph = True
    m.decode_raw_logits = False
    h, s = m.beamsearch_nbest(src, lens, im, K, 1, ML)
    h2, s2 = m.beamsearch_nbest(src, lens, im, K, 1, ML)
    m.decode_raw_logits = True
    e = m.beamsearch_required(src, lens, im, beam_size=K, n_best=1, max_length=ML)
    lines.append("two runs of beamsearch_nbest on the log-probability steps: same lists %s, max abs score difference %.2e"
                 % (h == h2, (s - s2).abs().max().item()))
    lines.append("no phrases against beamsearch_nbest:                       same lists %s, max abs score difference %.2e"
                 % (e.hyps == h, (e.scores - s).abs().max().item()))
    for n in (2, 8):
        req, fn = required(n)
        r = fn()
        ok = all(contains(r.hyps[b][0], ph) for b in range(B) for ph in req[b])
        lines.append("%d phrases per sentence: best hypotheses complete %d / %d, every phrase found in them: %s"
                     % (n, int(r.complete[:, 0].sum().item()), B, ok))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
