"""Shallow fusion with an n-gram language model (vagnmt_hip.lm) timed at configs[3]'s decode shape: the cfg2 model of bench.py
(untrained, so all steps run), batch 16, beam 12, 40 steps, V 9391, an order-3 model trained on a seeded Zipf corpus of 30 000
sentences of 12 words.

  1. microseconds per decode step of beamsearch_lm (beta 0.3) against beamsearch_nbest on the same log-probability steps
     (decode_raw_logits off), graph and eager mode, the variants alternating inside every round;
  2. the vag_lm_fuse_beam call alone at 192 rows of V = 9391 on a search buffer of random words of the corpus (device events
     around 20 calls), beside the floor by bytes: the rows read and written once, 192 x 9391 x 4 x 2 bytes, at the HBM rate a
     float4 copy reaches on this chip (6.29 TB/s, MI355X notes) -- plus one launch and at most 4 dependent loads, which the floor
     does not count;
  3. NgramLM.train in seconds (host);
  4. with --parent-lib FILE (the parent commit's libvagnmt.so): beamsearch_nbest's step and the training step of this build
     against that library, each in child processes of its own, alternating, same seeds -- nothing of theirs is touched, so
     they must agree within the windows' spread.

Every figure: `rounds` windows, median with min and max.  It fails without a GPU.

Usage (GPU box):  python tools/exp_lm.py [--rounds 5] [--reps 3] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
B, K, ML, ORDER, BETA = 16, 12, 40, 3, 0.3
SENTENCES, WORDS = 30000, 12
HBM_COPY_RATE = 6.29e12            # bytes/s a float4 copy reaches (MI355X notes): the floor's rate


def fmt(xs, unit):
    return "median %9.1f  min %9.1f  max %9.1f %s" % (statistics.median(xs), min(xs), max(xs), unit)


def zipf_corpus(V, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    return (4 + np.minimum(rng.zipf(1.3, size=(SENTENCES, WORDS)), V - 5)).astype(np.int64)


def event_windows(fn, rounds, reps):
    import torch
    out = []
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)                            # us per call
    return out


def ab_child(a):
    """One child of the A/B: beamsearch_nbest's step (graph mode, raw logits as shipped) and the fused training step of cfg2."""
    import torch
    from vagnmt_hip import _lib
    if os.environ.get("VAG_EXP_LM_PARENT") == "1":                             # the parent's library has no LM entries
        for name in [n for n in _lib.PROTOS if n.startswith("vag_lm")]:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exp_lm: needs a GPU")
    if a.ab_child:
        return ab_child(a)
    import bench
    from vagnmt_hip import _lib, lm as lm_mod
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    m.decode_raw_logits = False                                                # the log-probability steps, for both searches
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    V = c["V"]
    lines = ["tools/exp_lm.py on %s: B %d, beam %d, %d steps, V %d, order %d, beta %.1f; %d rounds x %d decodes per window"
             % (torch.cuda.get_device_name(0), B, K, ML, V, ORDER, BETA, a.rounds, a.reps)]
    corpus = zipf_corpus(V)
    train = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        lm = lm_mod.NgramLM.train(corpus, V, ORDER)
        train.append(time.perf_counter() - t0)
    lm.to(dev)
    lines.append("NgramLM.train, %d sentences of %d words, order %d (n-grams per order %s; %.1f MB on the device): %s"
                 % (SENTENCES, WORDS, ORDER, lm.counts, lm.host.nbytes / 1e6, fmt(train, "s")))
    variants = [("nbest_logp", lambda: m.beamsearch_nbest(src, lens, im, K, 1, ML)),
                ("lm_beta%.1f" % BETA, lambda: m.beamsearch_lm(src, lens, im, lm, beta=BETA, beam_size=K, n_best=1, max_length=ML))]
    for graph in (True, False):
        m.decode_graph = graph
        times, steps = {n: [] for n, _ in variants}, {}
        for name, fn in variants:
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
        lines.append("%s mode, us per decode step" % ("graph" if graph else "eager"))
        base = statistics.median(times["nbest_logp"])
        for name, _ in variants:
            lines.append("  %-14s steps %3d  %s   %+9.1f us vs nbest_logp"
                         % (name, steps[name], fmt(times[name], "us"), statistics.median(times[name]) - base))
    m.decode_graph = True
    # the call alone: 192 rows, contexts of corpus words at step 7 of a search buffer
    R = B * K
    ldl = (V + 3) // 4 * 4
    rows = torch.log_softmax(torch.randn(R, ldl, device=dev), 1)
    words = torch.from_numpy(corpus[:ML * R // WORDS + 1].reshape(-1)[:ML * R]).view(ML, B, K)
    parents = torch.randint(0, K, (ML, B, K))
    beam = torch.cat([words, parents]).to(dev).contiguous()
    ptrs, lds = (C.c_void_p * 1)(rows.data_ptr()), (C.c_int64 * 1)(ldl)
    L = _lib.lib()

    def fuse():
        rc = L.vag_lm_fuse_beam(ptrs, lds, 1, beam.data_ptr(), 7, ML, B, K, V, C.byref(lm.struct()), BETA, _lib.stream())
        assert rc == 0, rc

    xs = event_windows(fuse, a.rounds, 20)
    nbytes = R * V * 4 * 2
    floor_us = nbytes / HBM_COPY_RATE * 1e6
    lines.append("vag_lm_fuse_beam alone, %d rows of V = %d: %s   rows read and written once %.1f MB: floor by bytes (%.2f TB/s) "
                 "%.1f us, %.1f %% of the floor's rate" % (R, V, fmt(xs, "us"), nbytes / 1e6, HBM_COPY_RATE / 1e12, floor_us,
                                                           100.0 * floor_us / statistics.median(xs)))
    if a.parent_lib:
        res = {"new": [], "parent": []}
        for who in ("new", "parent", "new", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env.update(VAG_LIB=os.path.abspath(a.parent_lib), VAG_EXP_LM_PARENT="1")
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
