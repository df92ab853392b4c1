"""chrF selection against BLEU selection, timed.

(a) mbr_select's device work on the same candidates with utility "chrf" and with "bleu": 16 sentences, N = 16 and N = 64
    candidates that are their own references, rows of 40 tokens whose surfaces average about 5 characters (spans of 24..39
    words; a sentence's candidates share a third of their words, as samples of one source do).  For "chrf" also its two parts:
    the expansion (vag_surface_expand) and the pairs + arg-max (vag_chrf_select) on rows expanded beforehand;
(b) mbr_decode on the cfg2 model of bench.py (B 16, 16 samples, max_length 40, graph mode, untrained) with either utility, and
    the sample_decode that feeds both.

Every device figure: host clock around `reps` calls closed by a device synchronise, after a warm-up; `windows` such windows,
the median and the extremes reported.  Each part runs in a fresh process under a time limit of its own; after one that fails
or runs out of time nothing more is started.

Usage (GPU box):  python tools/exp_chrf.py [--windows 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 240
B, NS, L, V = 16, (16, 64), 40, 9391
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
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale, "max": max(xs) * scale}


def words(V, seed=0):
    """V pseudo-words of 1..9 lower-case letters (mean 5), every fourth a BPE continuation."""
    import numpy as np
    g = np.random.default_rng(seed)
    out = ["<pad>", "<unk>", "<s>", "</s>"]
    for i in range(4, V):
        w = "".join(chr(97 + int(c)) for c in g.integers(0, 26, size=int(g.integers(1, 10))))
        out.append(w + "@@" if i % 4 == 0 else w)
    return out


def rows(N, seed=0):
    import numpy as np
    g = np.random.default_rng(seed)
    x = g.integers(4, V, size=(B, N, L)).astype(np.int64)
    base = g.integers(4, V, size=(B, 1, L))
    x = np.where(g.random((B, N, L)) < 0.33, base, x)
    ends = g.integers(24, L, size=(B, N))
    for b in range(B):
        for i in range(N):
            x[b, i, ends[b, i]:] = 0
            x[b, i, ends[b, i]] = EOS
    return x


def worker(mode, windows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "vag-nmt_amd"))
    import torch
    from vagnmt_hip import mbr
    from vagnmt_hip._lib import call, ptr, stream
    from vagnmt_hip.surface import Surface
    dev = torch.device("cuda:0")
    res = {"mode": mode, "device": torch.cuda.get_device_name(0)}
    if mode == "select":
        table = Surface(words(V))
        for N in NS:
            x = torch.from_numpy(rows(N)).to(dev)
            reps = 100 if N == 16 else 20
            chars, lens = table.expand(x)
            res["chars_mean_N%d" % N] = float(lens.float().mean())
            res["chars_max_N%d" % N] = int(lens.max())
            res["row_chars_N%d" % N] = int(chars.shape[2])
            res["bleu_N%d_us" % N] = summary(windows_of(lambda: mbr.run(x, None, None, 0), reps, windows), 1e6)
            res["chrf_N%d_us" % N] = summary(windows_of(lambda: mbr.run_chrf(x, None, None, table), reps, windows), 1e6)
            res["chrf_expand_N%d_us" % N] = summary(windows_of(lambda: table.expand(x), reps, windows), 1e6)
            expected = torch.empty(B, N, device=dev)
            index = torch.empty(B, dtype=torch.int64, device=dev)

            def pairs():
                call("vag_chrf_select", ptr(chars, torch.int32), ptr(lens, torch.int32), None, None, None, B, N, chars.shape[2], N,
                     chars.shape[2], None, None, ptr(expected), ptr(index, torch.int64), stream())
            res["chrf_pairs_N%d_us" % N] = summary(windows_of(pairs, reps, windows), 1e6)
            res["pairs_N%d" % N] = B * N * N
        print("RESULT " + json.dumps(res))
        return
    import bench
    from vagnmt_hip.sampling import Generator
    c = dict(bench.CFG2)
    c["B"] = B
    m = bench.build_model(c, dev).eval()
    table = Surface(words(m.tgt_size))
    src, lens, _, im = bench.make_batch(c, 0, dev, ragged=True)
    kw = dict(n_samples=16, max_length=L, temperature=1.0, top_k=0, generator=Generator(1))
    res["sample_decode_ms"] = summary(windows_of(lambda: m.sample_decode(src, lens, im, **kw), 3, windows), 1e3)
    res["mbr_decode_bleu_ms"] = summary(windows_of(lambda: m.mbr_decode(src, lens, im, **kw), 3, windows), 1e3)
    res["mbr_decode_chrf_ms"] = summary(windows_of(lambda: m.mbr_decode(src, lens, im, utility="chrf", surface=table, **kw), 3, windows), 1e3)
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
    ap.add_argument("--worker", default=None, choices=["select", "decode"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.windows)
    res, ok = {}, True
    for mode in ("select", "decode"):
        got = run_child(mode, a.windows) if ok else None
        ok = ok and got is not None
        res[mode] = got
        for key, v in sorted((got or {}).items()):
            if isinstance(v, dict):
                print("%-28s %10.3f %s (windows %.3f .. %.3f)" % (key[:key.rindex("_")], v["median"], key[key.rindex("_") + 1:], v["min"], v["max"]))
            elif key != "mode":
                print("%-28s %s" % (key, v))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
