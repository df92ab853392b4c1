"""Beam-12 decoding with and without attention alignments, timed at configs[3]'s decode shape (B 16, k 12, max_length 80, the
cfg2 model of bench.py; untrained, so all 80 steps run).

(a) the default search (beamsearch_decode) in this tree and, with --other-tree DIR, in another checkout of the project (the parent
    commit, built): the two alternate, one fresh process per measurement, so that both see the same box in the same session;
(b) beamsearch_nbest and beamsearch_align (n_best 12) in this tree, and the finish kernels on the state the search left behind
    (vag_beam_finish_nbest against vag_beam_finish_align, n = 1 and 12), timed on their own.

Every figure: host clock around `reps` calls closed by a device synchronise, after a warm-up; `windows` such windows per process,
all of them reported (median, min, max).  Every measuring process runs under a time limit of its own; after one that fails or
runs out of time nothing more is started.

Usage (GPU box):  python tools/exp_align.py [--other-tree DIR] [--rounds 3] [--windows 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 420               # one measuring process: import, build the model, capture, warm up, time
B, K, ML = 16, 12, 80


def windows_of(fn, reps, windows):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return out


def summary(xs, scale):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale, "max": max(xs) * scale,
            "windows": [x * scale for x in xs]}


def worker(mode, tree, windows):
    """One measurement in the checkout `tree` (this process imports that tree's package and bench.py)."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "vag-nmt_amd"))
    import torch
    import bench
    c = dict(bench.CFG2)
    c["B"] = B
    dev = torch.device("cuda:0")
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    res = {"mode": mode, "tree": tree, "device": torch.cuda.get_device_name(0)}
    if mode == "plain":
        xs = windows_of(lambda: m.beamsearch_decode(src, lens, im, K, ML), 10, windows)
        steps = int(m.last_decode_steps)
        res.update(steps=steps, decode_us_per_step=summary(xs, 1e6 / steps), decode_ms_per_batch=summary(xs, 1e3))
    else:
        from vagnmt_hip._lib import call, ptr, stream
        I64 = torch.int64
        for name, fn in (("nbest", lambda: m.beamsearch_nbest(src, lens, im, K, K, ML)),
                         ("align", lambda: m.beamsearch_align(src, lens, im, K, K, ML))):
            xs = windows_of(fn, 10, windows)
            steps = int(m.last_decode_steps)
            res[name] = dict(steps=steps, us_per_step=summary(xs, 1e6 / steps), ms_per_batch=summary(xs, 1e3))
        a = m.beamsearch_align(src, lens, im, K, K, ML)
        h, s = m.beamsearch_nbest(src, lens, im, K, K, ML)
        res["align_equals_nbest"] = bool(a.hyps == h and torch.equal(a.scores, s))
        # the finish kernels alone, on the aligning search's state
        st = [v for key, v in m._decode_cache.items() if isinstance(key, tuple) and "align" in key][0]
        nll, beam, hist, steps = st["nll"], st["beam"], st["attn_hist"], int(m.last_decode_steps)
        Tp, Ts = hist.shape[2], src.shape[1]
        res["attn_hist_bytes"] = hist.numel() * 4
        for n in (1, K):
            out = torch.empty(B, n, ML, dtype=I64, device=dev)
            sc = torch.empty(B, n, device=dev)
            att = torch.empty(B, n, ML, Ts, device=dev)
            pos = torch.empty(B, n, ML, dtype=I64, device=dev)
            xs = windows_of(lambda: call("vag_beam_finish_nbest", ptr(nll), ptr(beam, I64), ML, steps, B, K, n, ptr(out, I64),
                                         ptr(sc), stream()), 200, windows)
            res["finish_nbest%d_us" % n] = summary(xs, 1e6)
            xs = windows_of(lambda: call("vag_beam_finish_align", ptr(nll), ptr(beam, I64), ptr(hist), ML, steps, B, K, n, Tp, Ts,
                                         ptr(out, I64), ptr(sc), ptr(att), ptr(pos, I64), stream()), 200, windows)
            res["finish_align%d_us" % n] = summary(xs, 1e6)
            res["finish_align%d_bytes_written" % n] = att.numel() * 4 + pos.numel() * 8 + out.numel() * 8
        # the record launch alone (the step index by value)
        al = (torch.empty(B * K, Tp, device=dev).uniform_() + 0.1)
        import ctypes as C
        pp = (C.c_void_p * 1)(al.data_ptr())
        xs = windows_of(lambda: call("vag_beam_attn_record", pp, 1, ptr(hist), 5, ML, B, K, Tp, stream()), 500, windows)
        res["record_launch_us"] = summary(xs, 1e6)
        res["record_bytes_per_step"] = al.numel() * 4
    print("RESULT " + json.dumps(res))


def run_child(mode, tree, windows):
    """A fresh process per measurement, under its own time limit; None after a failure (the caller then stops)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--tree", tree, "--windows", str(windows)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print("%s in %s: no result within %d s -- stopping" % (mode, tree, STEP_LIMIT_S))
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print("%s in %s: exit status %d -- stopping\n%s" % (mode, tree, r.returncode, r.stderr[-2000:]))
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-tree", default=None, help="another built checkout (the parent commit) for the A/B of the default search")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["plain", "align"])
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.windows)
    trees = [("this", ROOT)] + ([("other", os.path.abspath(a.other_tree))] if a.other_tree else [])
    res = {"shape": dict(B=B, beam=K, max_length=ML), "plain": {name: [] for name, _ in trees}, "align": None}
    ok = True
    for r in range(a.rounds):
        for name, tree in (trees if r % 2 == 0 else trees[::-1]):          # alternate, and alternate who goes first
            got = run_child("plain", tree, a.windows) if ok else None
            ok = ok and got is not None
            if got:
                res["plain"][name].append(got)
                print("round %d %-5s default beam-12: %.1f us per decode step (windows %.1f .. %.1f)" % (
                    r, name, got["decode_us_per_step"]["median"], got["decode_us_per_step"]["min"], got["decode_us_per_step"]["max"]))
    if ok:
        res["align"] = run_child("align", ROOT, a.windows)
        ok = res["align"] is not None
    for name, _ in trees:
        meds = [g["decode_us_per_step"]["median"] for g in res["plain"][name]]
        allw = [w for g in res["plain"][name] for w in g["decode_us_per_step"]["windows"]]
        if meds:
            res["plain_" + name + "_us_per_step"] = {"median_of_medians": statistics.median(meds), "process_medians": meds,
                                                     "min_window": min(allw), "max_window": max(allw)}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
