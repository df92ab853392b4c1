"""A validation pass, timed: validate() on the device against the same work done the way it had to be done before.

Workload: the cfg2 model of bench.py (untrained: no hypothesis ends early, every decode runs max_length steps), a seeded synthetic
dev set of 1024 sentence pairs (Multi30K's dev set has 1014), the loss in batches of 64, the decode in batches of 16 with beam 12
and max_length 40, graph mode, every shape warmed by two untimed passes of each side (the first runs eagerly, the second captures).

  side A   validate(ts, loss batches, metrics=("loss",)) + validate(ts, decode batches, metrics=("bleu",)): the dev loss summed on
           the device, the decode's rows kept there, BleuStats.add per batch, one read of the device per call
  side B   the same eval_loss with three .item() per batch, the token lists from beamsearch_decode, and corpus BLEU by the plain
           Python restatement (tests/validate_ref.py) on the host; its parts timed inside the pass
The sides alternate, A B A B .., `windows` times; medians with the extremes.  Then the metric launch alone (vag_corpus_bleu_stats,
rows of 40 tokens, one reference) at N = 16 and N = 1024.

Unchanged paths: `step` (B 64, graph replay) and `beamsearch_decode` (B 16, beam 12, max_length 40) in fresh processes that
alternate between this library and another build of it (--parent-lib, the parent commit's libvagnmt.so), `rounds` times each.

Every part runs in a fresh process under a time limit of its own; after one that fails or runs out of time nothing more is started.

Usage (GPU box):  python tools/exp_validate.py [--windows 5] [--parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 360
N_DEV, B_LOSS, B_DEC, BEAM, MAXLEN = 1024, 64, 16, 12, 40
NEW_SYMBOLS = ("vag_corpus_bleu_supported", "vag_corpus_bleu_stats")


def summary(xs, scale):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale, "max": max(xs) * scale}


def setup(parent):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from vagnmt_hip import _lib
    if parent:                                  # the parent's library does not export what this change adds
        for k in NEW_SYMBOLS:
            _lib.PROTOS.pop(k, None)
    import torch
    import bench
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip.trainer import TrainStep
    dev = torch.device("cuda:0")
    c = dict(bench.CFG2)
    m = bench.build_model(c, dev)
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), lr=4e-4, weight_decay=1e-5,
                   clip=1.0, teacher_force_ratio=1.0)
    return torch, bench, c, m, ts, dev


def dev_set(torch, bench, c, dev, B):
    out = []
    for i in range(N_DEV // B):
        cc = dict(c)
        cc["B"] = B
        src, lens, tgt, im = bench.make_batch(cc, 100 + i, dev, ragged=True)
        g = torch.Generator().manual_seed(i)
        ends = torch.randint(8, cc["Tt"] - 1, (B,), generator=g).tolist()
        tgt = tgt.cpu()
        for b in range(B):                      # targets of 8 .. 38 words, EOS, padding
            tgt[b, ends[b]] = 3
            tgt[b, ends[b] + 1:] = 0
        out.append((src, lens, tgt.to(dev), im))
    return out


def worker_validate(windows):
    torch, bench, c, m, ts, dev = setup(False)
    import validate_ref as R
    from vagnmt_hip.validate import validate
    loss_b, dec_b = dev_set(torch, bench, c, dev, B_LOSS), dev_set(torch, bench, c, dev, B_DEC)
    refs = [[row] for _, _, tgt, _ in dec_b for row in tgt.cpu().tolist()]

    def side_a():
        t0 = time.perf_counter()
        a = validate(ts, loss_b, metrics=("loss",))
        t1 = time.perf_counter()
        b = validate(ts, dec_b, beam_size=BEAM, max_length=MAXLEN, metrics=("bleu",))
        t2 = time.perf_counter()
        return {"total": t2 - t0, "loss": t1 - t0, "decode_bleu": t2 - t1}, (a.loss_mt, b.bleu)

    def side_b():
        m.eval()
        t0 = time.perf_counter()
        tot = [0.0, 0.0, 0.0]
        for batch in loss_b:
            out = ts.eval_loss(*batch)
            for j in range(3):
                tot[j] += out[j].item()
        t1 = time.perf_counter()
        lists = []
        for src, lens, tgt, im in dec_b:
            lists.extend(m.beamsearch_decode(src, lens, im, BEAM, MAXLEN))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        bleu = R.corpus_bleu(lists, refs)
        t3 = time.perf_counter()
        return {"total": t3 - t0, "loss_item": t1 - t0, "decode_lists": t2 - t1, "host_bleu": t3 - t2}, (tot[1] / len(loss_b), bleu)

    ra, rb = side_a()[1], side_b()[1]           # warm-up: every shape captured
    side_a(), side_b()
    A, Bs = [], []
    for _ in range(windows):
        A.append(side_a()[0])
        Bs.append(side_b()[0])
    res = {"mode": "validate", "device": torch.cuda.get_device_name(0), "windows": windows,
           "agree": {"loss_mt": [ra[0], rb[0]], "bleu_A": list(ra[1][:1]) + list(ra[1][2:]), "bleu_B": [rb[1][0]] + list(rb[1][2:])}}
    for name, rows in (("A", A), ("B", Bs)):
        for k in rows[0]:
            res["%s_%s_s" % (name, k)] = summary([r[k] for r in rows], 1.0)
    # the metric launch alone
    from vagnmt_hip.validate import BleuStats
    for N in (16, 1024):
        g = torch.Generator().manual_seed(N)
        h = torch.randint(4, 40, (N, MAXLEN), generator=g)
        r = torch.where(torch.rand(N, MAXLEN, generator=g) < 0.7, h, torch.randint(4, 40, (N, MAXLEN), generator=g))
        h[:, -1] = 3
        r[:, -2] = 3
        h, r = h.to(dev), r[:, None, :].contiguous().to(dev)
        st = BleuStats(dev)
        reps = 200
        for _ in range(10):
            st.add(h, r)
        torch.cuda.synchronize()
        ws = []
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(reps):
                st.add(h, r)
            torch.cuda.synchronize()
            ws.append((time.perf_counter() - t0) / reps)
        res["bleu_stats_N%d_us" % N] = summary(ws, 1e6)
    print("RESULT " + json.dumps(res))


def worker_paths(windows, parent):
    torch, bench, c, m, ts, dev = setup(parent)
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    for _ in range(5):
        ts.step(src, lt, tgt, im, teacher=True)
    torch.cuda.synchronize()
    steps = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(50):
            ts.step(src, lt, tgt, im, teacher=True)
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) / 50)
    cc = dict(c)
    cc["B"] = B_DEC
    s2, l2, _, i2 = bench.make_batch(cc, 0, dev, ragged=True)
    m.eval()
    for _ in range(2):
        m.beamsearch_decode(s2, l2, i2, BEAM, MAXLEN)
    decs = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(3):
            m.beamsearch_decode(s2, l2, i2, BEAM, MAXLEN)
        torch.cuda.synchronize()
        decs.append((time.perf_counter() - t0) / 3)
    print("RESULT " + json.dumps({"mode": "paths", "lib": os.path.basename(os.environ.get("VAG_LIB") or "this"), "step_ms": summary(steps, 1e3),
                                  "beamsearch_decode_ms": summary(decs, 1e3)}))


def run_child(mode, windows, lib=None):
    """A fresh process per part, under its own time limit; None after a failure (the caller then stops)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--windows", str(windows)]
    env = dict(os.environ)
    if lib:
        env["VAG_LIB"] = lib
        cmd.append("--parent")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)
    except subprocess.TimeoutExpired:
        print("%s: no result within %d s -- stopping" % (mode, STEP_LIMIT_S))
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print("%s: exit status %d -- stopping\n%s" % (mode, r.returncode, r.stderr[-2000:]))
        return None
    return json.loads(lines[-1][7:])


def show(got):
    for key, v in sorted((got or {}).items()):
        if isinstance(v, dict) and "median" in v:
            print("  %-28s %10.3f %s (windows %.3f .. %.3f)" % (key[:key.rindex("_")], v["median"], key[key.rindex("_") + 1:], v["min"], v["max"]))
        elif key != "mode":
            print("  %-28s %s" % (key, v))


HEADER = """tools/exp_validate.py -- a validation pass on the device against the same work done on the host, timed

One GPU (the device name below is what the runtime reports).  The cfg2 model of bench.py, untrained (no hypothesis ends early: every
decode runs max_length steps), a seeded synthetic dev set of %(n)d sentence pairs, loss batches of %(bl)d, decode batches of %(bd)d,
beam %(k)d, max_length %(ml)d, graph mode, two untimed passes of each side first.  Host clock around one whole pass, %(w)d passes per
side, the sides alternating A B A B ..: median (windows min .. max), seconds.
  A = validate(metrics=("loss",)) on the loss batches + validate(metrics=("bleu",)) on the decode batches
  B = eval_loss with three .item() per batch (the same forward: there was no dev-loss entry before) + the lists of
      beamsearch_decode + corpus BLEU by the Python restatement on the host; loss_item / decode_lists / host_bleu are its parts
agree: both sides' loss_mt and (bleu, bp, ratio, translation_length, reference_length).
bleu_stats_N*: BleuStats.add alone (one launch of vag_corpus_bleu_stats), rows of %(ml)d tokens, one reference, 200 calls per window.
unchanged paths: step (B 64, graph replay, 50 calls per window) and beamsearch_decode (B %(bd)d, beam %(k)d, max_length %(ml)d, 3 calls
per window), ms, in fresh processes alternating between this build and the library given as --parent-lib, %(r)d rounds.
Per-kernel times, chrF, a trained model (early stops), multi-reference sets and the eager mode are not measured.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["validate", "paths"])
    ap.add_argument("--parent", action="store_true")
    a = ap.parse_args()
    if a.worker == "validate":
        return worker_validate(a.windows)
    if a.worker == "paths":
        return worker_paths(a.windows, a.parent)
    print(HEADER % dict(n=N_DEV, bl=B_LOSS, bd=B_DEC, k=BEAM, ml=MAXLEN, w=a.windows, r=a.rounds))
    res = {"validate": run_child("validate", a.windows), "paths": []}
    ok = res["validate"] is not None
    print("validation pass: %d sentence pairs, loss batches of %d, decode batches of %d, beam %d, max_length %d" % (N_DEV, B_LOSS, B_DEC, BEAM, MAXLEN))
    show(res["validate"])
    if a.parent_lib is None:
        print("unchanged paths: not measured (no --parent-lib)")
    for rnd in range(a.rounds if a.parent_lib else 0):
        for lib in (None, os.path.abspath(a.parent_lib)):
            got = run_child("paths", a.windows, lib) if ok else None
            ok = ok and got is not None
            res["paths"].append(got)
            print("unchanged paths, round %d, %s library:" % (rnd, "the parent's" if lib else "this"))
            show(got)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
