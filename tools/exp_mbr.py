"""Minimum-Bayes-risk selection, timed.

(a) vag_mbr_select alone (both launches) at B 64, N 16 and 64 candidates that are their own references, for a Multi30K-like
    length mix (spans of 12..24 words in rows of 25) and for full rows of 80 words without an EOS; both utilities;
(b) the same work in the tests' host restatement (tests/mbr_ref.py: Counter intersections, float64) on one thread -- whole at
    N 16, on the first 4 sentences at N 64 (the figure per pair is what is compared);
(c) mbr_decode on the cfg2 model of bench.py (B 16, max_length 80, graph mode, untrained: nearly every sample runs all 80
    steps): the sample_decode that feeds it, the selection on its samples alone, and mbr_decode as a whole, n_samples 16 and 64.

Every device figure: host clock around `reps` calls closed by a device synchronise, after a warm-up; `windows` such windows, all
reported.  Each part runs in a fresh process under a time limit of its own; after one that fails or runs out of time nothing
more is started.

Usage (GPU box):  python tools/exp_mbr.py [--windows 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 300
B_SEL, NS = 64, (16, 64)
B_DEC, ML = 16, 80
EOS = 3


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


def rows(kind, B, N, seed=0):
    """(B, N, L) int64 on the host: "mix": spans of 12..24 of 9387 words in rows of 25, sentences' candidates share a third of
    their words (as samples of one source do); "full": 80 words, no EOS."""
    import numpy as np
    g = np.random.default_rng(seed)
    if kind == "full":
        return g.integers(4, 200, size=(B, N, 80)).astype(np.int64)
    x = g.integers(4, 9391, size=(B, N, 25)).astype(np.int64)
    base = g.integers(4, 9391, size=(B, 1, 25))
    x = np.where(g.random((B, N, 25)) < 0.33, base, x)
    ends = g.integers(12, 25, size=(B, N))
    for b in range(B):
        for i in range(N):
            x[b, i, ends[b, i]:] = 0
            x[b, i, ends[b, i]] = EOS
    return x


def worker(mode, windows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    res = {"mode": mode}
    if mode == "host":
        import mbr_ref as R
        for kind in ("mix", "full"):
            for N in NS:
                Bh = B_SEL if N == 16 else 4
                x = rows(kind, Bh, N)
                t0 = time.perf_counter()
                m, lh, lr = R.pairwise(x)
                R.utilities(m, lh, lr, "bleu")
                dt = time.perf_counter() - t0
                res["host_%s_N%d" % (kind, N)] = {"sentences": Bh, "pairs": Bh * N * N, "seconds": dt, "us_per_pair": dt / (Bh * N * N) * 1e6,
                                                  "seconds_at_B64": dt * B_SEL / Bh}
        print("RESULT " + json.dumps(res))
        return
    import torch
    from vagnmt_hip import mbr
    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_name(0)
    if mode == "select":
        for kind in ("mix", "full"):
            for N in NS:
                x = torch.from_numpy(rows(kind, B_SEL, N)).to(dev)
                for name, uid in sorted(mbr.UTILITIES.items()):
                    xs = windows_of(lambda: mbr.run(x, None, None, uid), 200 if N == 16 else 50, windows)
                    res["select_%s_N%d_%s_us" % (kind, N, name)] = summary(xs, 1e6)
                    res["pairs_N%d" % N] = B_SEL * N * N
        print("RESULT " + json.dumps(res))
        return
    import bench
    from vagnmt_hip.sampling import Generator
    c = dict(bench.CFG2)
    c["B"] = B_DEC
    m = bench.build_model(c, dev).eval()
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    for n in NS:
        gen = Generator(1)
        kw = dict(n_samples=n, max_length=ML, temperature=1.0, top_k=0, generator=gen)
        xs = windows_of(lambda: m.sample_decode(src, lens, im, **kw), 3, windows)
        res["sample_decode_n%d_ms" % n] = summary(xs, 1e3)
        xs = windows_of(lambda: m.mbr_decode(src, lens, im, **kw), 3, windows)
        res["mbr_decode_n%d_ms" % n] = summary(xs, 1e3)
        drawn = m.sample_decode(src, lens, im, **kw)
        refs = mbr.pack(drawn.hyps).to(dev)
        res["span_mean_n%d" % n] = sum(len(h) for hs in drawn.hyps for h in hs) / (B_DEC * n)
        xs = windows_of(lambda: mbr.run(refs, None, None, 0), 50, windows)
        res["selection_n%d_ms" % n] = summary(xs, 1e3)
    print("RESULT " + json.dumps(res))


def run_child(mode, windows):
    """A fresh process per part, under its own time limit; None after a failure (the caller then stops)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--windows", str(windows)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print("%s: no result within %d s -- stopping" % (mode, STEP_LIMIT_S))
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print("%s: exit status %d -- stopping\n%s" % (mode, r.returncode, r.stderr[-2000:]))
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["select", "host", "decode"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.windows)
    res, ok = {}, True
    for mode in ("select", "decode", "host"):
        got = run_child(mode, a.windows) if ok else None
        ok = ok and got is not None
        res[mode] = got
        for key, v in sorted((got or {}).items()):
            if isinstance(v, dict) and "median" in v:
                print("%-34s %10.3f %s (windows %.3f .. %.3f)" % (key[:key.rindex("_")], v["median"], key[key.rindex("_") + 1:], v["min"], v["max"]))
            elif isinstance(v, dict):
                print("%-34s %s" % (key, json.dumps(v)))
            elif key not in ("mode",):
                print("%-34s %s" % (key, v))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
