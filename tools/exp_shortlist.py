"""Lexical shortlists (vagnmt_hip.shortlist) timed at configs[3]'s decode shape: the cfg2 model of bench.py (untrained, so all
steps run), batch 16, beam 12, 40 steps, a seeded random lexicon of 100 translations per source word, first = 100.

  1. microseconds per decode step of beamsearch_nbest on the full vocabulary (V 9391) against the shortlist view at capacities
     1024, 2048 and 4096 -- the view's decode alone, the selection made once before the windows -- in graph mode, the variants
     alternating inside every round;
  2. the same with the head as wide as configs[4]'s (V 40 000, the other sizes cfg2's);
  3. the same for an Ensemble of three cfg2 models at capacity 2048;
  4. the per-batch cost of a refill at V 9391, capacity 2048: sl.select alone (select + gathers, device events), and a whole
     sl.beamsearch_nbest (select, gathers, the refresh of prep and the token tables, the decode, the id map) against the view's
     decode alone, as microseconds per batch and as a share of the 40-step decode;
  5. with --parent-lib FILE (the parent commit's libvagnmt.so): beamsearch_nbest's step and the training step of this build
     against that library, each in child processes of its own, alternating, same seeds -- nothing of theirs is touched, so
     they must agree within the windows' spread.

Not measured here: per-kernel times of the vocabulary product and stage 1 (no kernel trace is taken), and translation quality
against the full vocabulary (there is no trained model to measure it with).

Every figure: `rounds` windows, median with min and max.  It fails without a GPU.

Usage (GPU box):  python tools/exp_shortlist.py [--rounds 5] [--reps 2] [--parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
B, K, ML, FIRST, BEST = 16, 12, 40, 100, 100
CAPS = (1024, 2048, 4096)


def fmt(xs, unit):
    return "median %9.1f  min %9.1f  max %9.1f %s" % (statistics.median(xs), min(xs), max(xs), unit)


def random_lexicon(Vs, V, seed=0):
    import numpy as np
    from vagnmt_hip.shortlist import Lexicon
    rng = np.random.default_rng(seed)
    return Lexicon(rng.integers(4, V, size=(Vs, BEST)).astype(np.int32), V)


def wall_windows(variants, rounds, reps, steps_of):
    """us per decode step of every variant, the variants alternating inside every round."""
    import torch
    times, steps = {n: [] for n, _ in variants}, {}
    for name, fn in variants:
        for _ in range(2):
            fn()
        steps[name] = steps_of()
    torch.cuda.synchronize()
    for r in range(rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps / steps[name] * 1e6)
    return times, steps


def ab_child(a):
    """One child of the A/B: beamsearch_nbest's step (graph mode, raw logits as shipped) and the fused training step of cfg2."""
    import torch
    from vagnmt_hip import _lib
    if os.environ.get("VAG_EXP_SHORTLIST_PARENT") == "1":                      # the parent's library has no shortlist entries
        for name in [n for n in _lib.PROTOS if n.startswith("vag_shortlist")]:
            del _lib.PROTOS[name]
    import bench
    from vagnmt_hip.trainer import TrainStep
    from machine_translation_vision.losses import PairwiseRankingLoss
    dev = torch.device("cuda:0")
    c = dict(bench.CFG2)
    m = bench.build_model(c, dev)
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), lr=4e-4, weight_decay=1e-5,
                   clip=1.0, teacher_force_ratio=1.0, use_graph=True)
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    for _ in range(10):
        ts.step(src, lens_t, tgt, im)
    torch.cuda.synchronize()
    step = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(20):
            ts.step(src, lens_t, tgt, im)
        torch.cuda.synchronize()
        step.append((time.perf_counter() - t0) / 20 * 1e3)
    c["B"] = B
    m.eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    for _ in range(2):
        m.beamsearch_nbest(src, lens, im, K, 1, ML)
    torch.cuda.synchronize()
    dec = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            m.beamsearch_nbest(src, lens, im, K, 1, ML)
        torch.cuda.synchronize()
        dec.append((time.perf_counter() - t0) / a.reps / int(m.last_decode_steps) * 1e6)
    print("AB " + json.dumps({"lib": _lib.LIB_PATH, "step_ms": step, "nbest_us": dec}))
    return 0


def decode_table(lines, title, obj, lex, caps, src, lens, im, a):
    """Full vocabulary against the view's decode at every capacity -> lines."""
    from vagnmt_hip.shortlist import Shortlist
    sls = [Shortlist(obj, lex, first=FIRST, best=BEST, capacity=cap) for cap in caps]
    sels = [sl.select(src, lens) for sl in sls]
    last = {"obj": obj}

    def run(o):
        last["obj"] = o
        return o.beamsearch_nbest(src, lens, im, K, 1, ML)

    variants = [("full", lambda: run(obj))] + [("cap%d" % cap, (lambda v: lambda: run(v))(sl.view)) for cap, sl in zip(caps, sls)]
    times, steps = wall_windows(variants, a.rounds, a.reps, lambda: int(last["obj"].last_decode_steps))
    lines.append(title)
    base = statistics.median(times["full"])
    for (name, _), sel in zip(variants, [None] + sels):
        note = "" if sel is None else "  (n %d words, %d ranks applied)" % (int(sel.n), int(sel.rank_used))
        lines.append("  %-8s steps %3d  %s   %+8.1f us vs full%s"
                     % (name, steps[name], fmt(times[name], "us"), statistics.median(times[name]) - base, note))
    return sls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exp_shortlist: needs a GPU")
    if a.ab_child:
        return ab_child(a)
    import bench
    from vagnmt_hip.ensemble import Ensemble
    dev = torch.device("cuda:0")
    c = dict(bench.CFG2)
    c["B"] = B
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    lines = ["tools/exp_shortlist.py on %s: B %d, beam %d, %d steps, first %d, best %d, graph mode; %d rounds x %d decodes per window"
             % (torch.cuda.get_device_name(0), B, K, ML, FIRST, BEST, a.rounds, a.reps)]
    m = bench.build_model(c, dev).eval()
    lex = random_lexicon(c["Vs"], c["V"])
    sls = decode_table(lines, "cfg2, V %d: us per decode step of beamsearch_nbest" % c["V"], m, lex, CAPS, src, lens, im, a)

    # the per-batch cost of a refill, capacity 2048
    sl = sls[1]
    xs = []
    for _ in range(2):
        sl.select(src, lens)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            sl.select(src, lens)
        e1.record()
        torch.cuda.synchronize()
        xs.append(e0.elapsed_time(e1) / 10 * 1e3)
    lines.append("refill at V %d, capacity %d, tied embeddings (one select + two gathers):" % (c["V"], sl.capacity))
    lines.append("  sl.select alone (device events)                     %s per batch" % fmt(xs, "us"))
    variants = [("view", lambda: sl.view.beamsearch_nbest(src, lens, im, K, 1, ML)),
                ("whole", lambda: sl.beamsearch_nbest(src, lens, im, K, 1, ML))]
    times, steps = wall_windows(variants, a.rounds, a.reps, lambda: 1)                  # us per DECODE here
    view_us, whole_us = statistics.median(times["view"]), statistics.median(times["whole"])
    lines.append("  view's decode alone (no refill)                     %s per decode" % fmt(times["view"], "us"))
    lines.append("  sl.beamsearch_nbest (select, gathers, prep + tables, decode, id map) %s per decode" % fmt(times["whole"], "us"))
    lines.append("  refill + table refresh + id map: %+.1f us per batch = %.1f %% of the view's %d-step decode"
                 % (whole_us - view_us, 100.0 * (whole_us - view_us) / view_us, int(sl.view.last_decode_steps)))
    del sls, sl

    # an Ensemble of three
    ens = Ensemble([m] + [bench.build_model(c, dev, seed=s).eval() for s in (11, 12)])
    decode_table(lines, "Ensemble of three cfg2 models, V %d: us per decode step" % c["V"], ens, lex, (2048,), src, lens, im, a)
    del ens

    # the head as wide as configs[4]'s
    c5 = dict(c, V=bench.CFG5["V"])
    m5 = bench.build_model(c5, dev).eval()
    decode_table(lines, "cfg2 sizes with configs[4]'s head, V %d: us per decode step" % c5["V"], m5,
                 random_lexicon(c5["Vs"], c5["V"]), CAPS, src, lens, im, a)
    del m5

    lines.append("per-kernel times of the vocabulary product and stage 1: not measured (no kernel trace taken)")
    lines.append("translation quality against the full vocabulary: not measured (no trained model)")
    if a.parent_lib:
        res = {"new": [], "parent": []}
        for who in ("new", "parent", "new", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env.update(VAG_LIB=os.path.abspath(a.parent_lib), VAG_EXP_SHORTLIST_PARENT="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--rounds", str(a.rounds), "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=600)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")]
            if p.returncode != 0 or not got:
                lines.append("A/B child (%s) failed: %s" % (who, p.stderr[-400:]))
                break
            res[who].append(json.loads(got[0][3:]))
        else:
            lines.append("this build against the parent commit's library (child processes, alternating new / parent / new / parent)")
            for who in ("new", "parent"):
                step = [x for r_ in res[who] for x in r_["step_ms"]]
                dec = [x for r_ in res[who] for x in r_["nbest_us"]]
                lines.append("  %-6s training step %s | beamsearch_nbest step %s" % (who, fmt(step, "ms"), fmt(dec, "us")))
    else:
        lines.append("this build against the parent commit's library: not measured (no --parent-lib)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
