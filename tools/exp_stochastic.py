"""Stochastic beam search against the plain n-best search and the sampling decoder, timed at configs[3]'s decode shape (B 16,
k = n = 12, max_length 80, the cfg2 model of bench.py; untrained, so all 80 steps run): microseconds per decode step of

    beamsearch_nbest(beam_size=12, n_best=12)                         the product path (raw logits; this feature leaves it untouched)
    beamsearch_nbest on the log-probability steps                     the yardstick: the steps a stochastic search runs
    beamsearch_stochastic(n_samples=12)                               12 samples without replacement
    sample_decode(n_samples=12)                                       12 samples with replacement (plain, not hoisted, steps)

in graph mode (captured chunks of 8 steps) and in eager mode (launch by launch).  The stochastic search runs its own expansion
(vag_beam_sbs_step: a row-aligned stage 1 that perturbs and ranks, one workgroup per sentence that conditions and selects);
what it adds to the plain expansion is the noise (two logf per word) and the second stage's transform.

Every figure: a host clock around `reps` whole decodes closed by a device synchronise, after a warm-up, divided by the steps run;
`rounds` such windows per variant, the variants alternating inside every round, all windows reported (median, min, max).
It also counts what the feature is for: distinct translations among 12 draws with and without replacement.
It fails without a GPU.

Usage (GPU box):  python tools/exp_stochastic.py [--rounds 3] [--reps 5] [--out FILE]"""
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
    from vagnmt_hip.sampling import Generator
    if not torch.cuda.is_available():
        sys.exit("exp_stochastic: needs a GPU")
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    gen = Generator(1)

    def nbest(raw):
        def run():
            m.decode_raw_logits = raw
            m.beamsearch_nbest(src, lens, im, K, K, ML)
            m.decode_raw_logits = True
        return run

    variants = [("nbest", nbest(True)), ("nbest_logp", nbest(False)),
                ("stochastic", lambda: m.beamsearch_stochastic(src, lens, im, n_samples=K, max_length=ML, generator=gen)),
                ("sample", lambda: m.sample_decode(src, lens, im, n_samples=K, max_length=ML, generator=gen))]
    lines = ["tools/exp_stochastic.py on %s: B %d, beam / samples %d, max_length %d, V %d; us per decode step, %d rounds x %d decodes "
             "per window" % (torch.cuda.get_device_name(0), B, K, ML, c["V"], a.rounds, a.reps)]
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
    # what it is for, on a peaked distribution: the same model with a strong EOS bias, so that sentences are short
    m.decode_graph = True
    with torch.no_grad():
        m.decoder.out.bias[3] += 9.0
    s = m.beamsearch_stochastic(src, lens, im, n_samples=K, max_length=ML, generator=gen)
    d = m.sample_decode(src, lens, im, n_samples=K, max_length=ML, generator=gen)
    with torch.no_grad():
        m.decoder.out.bias[3] -= 9.0
    lines.append("EOS bias +9: distinct translations among %d draws per sentence, mean over %d sentences: without replacement %.1f, "
                 "with replacement %.1f" % (K, B, sum(len({tuple(h) for h in sent}) for sent in s.hyps) / B,
                                            sum(len({tuple(h) for h in sent}) for sent in d.hyps) / B))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
