"""The penalised beam search against the plain n-best and the aligning search, timed at configs[3]'s decode shape (B 16, beam 12,
max_length 80, the cfg2 model of bench.py; untrained, so all 80 steps run): microseconds per decode step of

    beamsearch_nbest(beam_size=12, n_best=12)                      the product path (raw logits; this feature leaves it untouched)
    beamsearch_nbest on the log-probability steps                  the steps a penalised search runs
    beamsearch_align(beam_size=12, n_best=12)                      log-probability steps + the attention record launch
    beamsearch_penalised, stepwise off / on, beta 0 / 0.2          two launches per step (beta 0) or three (the coverage launch)

in graph mode (captured chunks of 8 steps) and in eager mode (launch by launch).  A penalised step is the members' steps (with the
attention rows kept, as in the aligning search), vag_beam_cover when beta > 0, and vag_beam_pen_step (a row-aligned stage 1 that
forms the penalised key of every word, one workgroup per sentence that selects and moves the carried length, penalty and coverage).

Every figure: a host clock around `reps` whole decodes closed by a device synchronise, after a warm-up, divided by the steps run;
`rounds` such windows per variant, the variants alternating inside every round, all windows reported (median, min, max).
It fails without a GPU.

Per-kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp_penalty.py --profile` runs a few
eager decodes of beamsearch_nbest on the log-probability steps, beamsearch_align and the stepwise penalised search with beta 0.2, and
nothing else.

Usage (GPU box):  python tools/exp_penalty.py [--rounds 3] [--reps 5] [--out FILE] [--profile]"""
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
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    if not torch.cuda.is_available():
        sys.exit("exp_penalty: needs a GPU")
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

    def pen(stepwise, beta):
        return lambda: m.beamsearch_penalised(src, lens, im, beam_size=K, n_best=K, max_length=ML, beta=beta, stepwise=stepwise)

    variants = [("nbest", nbest(True)), ("nbest_logp", nbest(False)), ("align", lambda: m.beamsearch_align(src, lens, im, K, K, ML)),
                ("pen_final_b0", pen(False, 0.0)), ("pen_final_b.2", pen(False, 0.2)), ("pen_step_b0", pen(True, 0.0)),
                ("pen_step_b.2", pen(True, 0.2))]
    if a.profile:
        m.decode_graph = False
        for name in ("nbest_logp", "align", "pen_step_b.2"):
            for _ in range(3):
                dict(variants)[name]()
        torch.cuda.synchronize()
        return 0
    lines = ["tools/exp_penalty.py on %s: B %d, beam %d, max_length %d, V %d; us per decode step, %d rounds x %d decodes per window"
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
        base, al = statistics.median(times["nbest_logp"]), statistics.median(times["align"])
        for name, _ in variants:
            xs = times[name]
            med = statistics.median(xs)
            lines.append("  %-14s steps %3d  median %7.1f  min %7.1f  max %7.1f   %+6.1f us vs nbest_logp  %+6.1f us vs align"
                         % (name, steps[name], med, min(xs), max(xs), med - base, med - al))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
